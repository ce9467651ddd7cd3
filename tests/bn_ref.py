"""Plain fp64 definitions (torch on the CPU) of what the streaming passes of csrc/bn.hip compute, and the EXACT case data the GPU tests
of tests/test_gpu_bn_passes.py feed them.  tests/test_cpu_bn_ref.py proves the definitions against torch's own BatchNorm / ReLU /
max-pool and their autograd.

Exact data: x, dout, residual, beta and mean are small integers, invstd and |gamma| come from {0.25, 0.5, 1, 2}, the backward
coefficients are multiples of 1/8, and the ranges shrink with the row count so that every sum of absolute values per column (sum |x|,
sum x^2, sum |g|, sum |g * xhat|) stays below 2^24 — which bounds every per-thread, per-block and per-column partial sum as well.  Every
intermediate of (x - mu) * sc + be, xhat, sc * (g - c1 - xhat * c2) and of the four sums is then a dyadic rational fp32 holds exactly,
whatever the summation order and with or without FMA contraction: the kernels' results must equal these fp64 ones bit for bit.
`check_exact` asserts the 2^24 condition for every case the generators return."""
import torch

LIMIT = float(1 << 24)
POW2 = (0.25, 0.5, 1.0, 2.0)


# ---- the block geometry of csrc/bn.hip (bn_geom): used only to choose and label cases ----------------------------------------------------
def bn_geom(rows, C):
    c4 = C // 4
    lanes = next(l for l in (64, 32, 16, 8, 4, 2, 1) if c4 >= l)
    rowlanes = 256 // lanes
    slabs = -(-c4 // lanes)
    rpb = max(4 * rowlanes, -(-rows * slabs // 1024))
    return {"lanes": lanes, "rowlanes": rowlanes, "slabs": slabs, "rpb": rpb, "chunks": -(-rows // rpb)}


def workspace_bytes(rows, C):
    return (bn_geom(rows, C)["chunks"] * 2 * C + 2 * C) * 4


GEOM_C = (4, 8, 16, 32, 64, 128, 256, 12, 20, 260, 2048)
GROWN_RPB = ((4, 1050000), (64, 70001), (256, 20000), (2048, 2500))        # rpb 1026, 69, 20, 20: above its floor of 4 * rowlanes


def geom_rows(C):
    rl = bn_geom(1, C)["rowlanes"]
    return sorted({1, rl - 1, rl, rl + 1, 4 * rl - 1, 4 * rl, 4 * rl + 1, 9 * rl + 3} - {0})


def geom_cases():
    return [(C, rows) for C in GEOM_C for rows in geom_rows(C)] + list(GROWN_RPB)


# ---- definitions -------------------------------------------------------------------------------------------------------------------------
def pack_mask(bits):
    """[rows, C] bool -> rows * C / 4 bytes: bit e of byte i = element 4 i + e; bits 4-7 zero"""
    b = bits.reshape(-1, 4).to(torch.uint8)
    return b[:, 0] | (b[:, 1] << 1) | (b[:, 2] << 2) | (b[:, 3] << 3)


def unpack_mask(mask, rows, C):
    m = mask.reshape(-1, 1).to(torch.int32)
    return ((m >> torch.arange(4, dtype=torch.int32)) & 1).bool().reshape(rows, C)


def relu(v):
    """fmaxf(v, 0): a NaN becomes 0 (the project's ReLU rule), -0 and negatives become +0"""
    return torch.where(v > 0, v, torch.zeros_like(v))


def apply(x, mean, invstd, gamma, beta, residual=None, relu_flag=False):
    """-> (out fp64 [rows, C], mask bytes): out = [relu]((x - mean) * (invstd * gamma) + beta [+ residual]); the mask holds (v > 0)"""
    v = (x.double() - mean.double()) * (invstd.double() * gamma.double()) + beta.double()
    if residual is not None:
        v = v + residual.double()
    return (relu(v) if relu_flag else v), pack_mask(v > 0)


def gate(dout, g8):
    """g = dout where the ReLU passed: g8 is mask bytes (uint8), the ReLU's output (float: passes where > 0) or None (no ReLU)"""
    d = dout.double()
    if g8 is None:
        return d
    keep = unpack_mask(g8, *dout.shape) if g8.dtype == torch.uint8 else (g8 > 0)
    return torch.where(keep, d, torch.zeros_like(d))


def xhat(x, mean, invstd):
    return (x.double() - mean.double()) * invstd.double()


def backward_sums(dout, g8, x, mean, invstd):
    """-> (sum g, sum g * xhat) per channel, fp64"""
    g = gate(dout, g8)
    return g.sum(0), (g * xhat(x, mean, invstd)).sum(0)


def bwd_apply(dout, g8, x, mean, invstd, gamma, c1, c2):
    """-> (dx, g): dx = gamma * invstd * (g - c1 - xhat * c2)"""
    g = gate(dout, g8)
    return (invstd.double() * gamma.double()) * (g - c1.double() - xhat(x, mean, invstd) * c2.double()), g


def frozen_backward(dout, g8, x, mean, invstd, gamma):
    """F.batch_norm(training=False)'s backward -> dict(dx = gamma * invstd * g, g, dgamma = sum g * xhat, dbeta = sum g); x / mean may be
    None when no sums are wanted"""
    g = gate(dout, g8)
    res = {"dx": invstd.double() * gamma.double() * g, "g": g, "dbeta": g.sum(0)}
    if x is not None:
        res["dgamma"] = (g * xhat(x, mean, invstd)).sum(0)
    return res


def pool_out_size(n, k, s, p, ceil=False):
    """torch's MaxPool2d output size: every window starts inside the input or its left padding"""
    if ceil:
        o = -(-(n + 2 * p - k) // s) + 1
        if (o - 1) * s >= n + p:
            o -= 1
        return o
    return (n + 2 * p - k) // s + 1


def _taps(H, W, k, s, p, Ho, Wo):
    """for every tap (r, q) in (row, column) order: code, clamped input coordinates [Ho] / [Wo] and the in-bounds mask [Ho, Wo]"""
    ho, wo = torch.arange(Ho), torch.arange(Wo)
    for r in range(k):
        hi = ho * s - p + r
        for q in range(k):
            wi = wo * s - p + q
            ok = ((hi >= 0) & (hi < H))[:, None] & ((wi >= 0) & (wi < W))[None, :]
            if bool(ok.any()):
                yield r * k + q, hi.clamp(0, H - 1), wi.clamp(0, W - 1), ok


def stem_fwd(x, mean, invstd, gamma, beta, k, s, p, Ho, Wo):
    """x [B, H, W, C] -> (out fp64 [B, Ho, Wo, C], idx uint8): maxpool(relu(bn(x))); idx = r * k + q of the FIRST maximum in (row, column)
    tap order among the in-bounds taps (a NaN counts as 0: the ReLU comes first); a window without in-bounds taps gives -inf / 0"""
    B, H, W, C = x.shape
    v = apply(x.reshape(-1, C), mean, invstd, gamma, beta, None, True)[0].reshape(B, H, W, C)
    best = torch.full((B, Ho, Wo, C), float("-inf"), dtype=torch.float64)
    idx = torch.zeros((B, Ho, Wo, C), dtype=torch.uint8)
    for code, hi, wi, ok in _taps(H, W, k, s, p, Ho, Wo):
        t = v[:, hi][:, :, wi]
        better = (t > best) & ok[None, :, :, None]
        best = torch.where(better, t, best)
        idx = torch.where(better, torch.full_like(idx, code), idx)
    return best, idx


def stem_gather(dout, idx, x, mean, invstd, gamma, beta, k, s, p):
    """d(relu(bn(x))) per INPUT pixel, fp64 [B, H, W, C]: every pooled gradient goes to the input position its idx names, then the ReLU
    gate relu(bn(x)) > 0 of that position"""
    B, H, W, C = x.shape
    _, Ho, Wo, _ = dout.shape
    g = torch.zeros((B, H, W, C), dtype=torch.float64)
    d = dout.double()
    for code, hi, wi, ok in _taps(H, W, k, s, p, Ho, Wo):
        sel = (idx == code) & ok[None, :, :, None]
        contrib = torch.where(sel, d, torch.zeros_like(d))
        for a in range(Ho):                                   # several windows may name one pixel: add them one output row at a time
            g[:, int(hi[a])].index_add_(1, wi, contrib[:, a])
    v = apply(x.reshape(-1, C), mean, invstd, gamma, beta, None, True)[0].reshape(B, H, W, C)
    return torch.where(v > 0, g, torch.zeros_like(g))


def stem_backward_sums(dout, idx, x, mean, invstd, gamma, beta, k, s, p):
    """-> (sum g, sum g * xhat) per channel over the stem's input pixels"""
    C = x.shape[-1]
    g = stem_gather(dout, idx, x, mean, invstd, gamma, beta, k, s, p).reshape(-1, C)
    return g.sum(0), (g * xhat(x.reshape(-1, C), mean, invstd)).sum(0)


def stem_bwd_apply(dout, idx, x, mean, invstd, gamma, beta, k, s, p, c1, c2):
    """-> dx [B, H, W, C] = gamma * invstd * (g - c1 - xhat * c2)"""
    g = stem_gather(dout, idx, x, mean, invstd, gamma, beta, k, s, p)
    return (invstd.double() * gamma.double()) * (g - c1.double() - xhat(x, mean, invstd) * c2.double())


def stem_frozen_backward(dout, idx, x, mean, invstd, gamma, beta, k, s, p):
    """-> dict(dx = gamma * invstd * g, dgamma, dbeta)"""
    C = x.shape[-1]
    g = stem_gather(dout, idx, x, mean, invstd, gamma, beta, k, s, p)
    return {"dx": invstd.double() * gamma.double() * g, "dbeta": g.reshape(-1, C).sum(0),
            "dgamma": (g * xhat(x, mean, invstd)).reshape(-1, C).sum(0)}


# ---- exact case data ---------------------------------------------------------------------------------------------------------------------
def _ints(g, shape, a):
    return torch.randint(-a, a + 1, tuple(shape), generator=g).float()


def _pick(g, n, values):
    return torch.tensor(values)[torch.randint(0, len(values), (n,), generator=g)]


def amplitudes(rows):
    """(|x| max, |dout| max, |mean| max, invstd choices): the most one element adds to a column sum is ax^2 and ad * (ax + am) * max invstd;
    times rows that stays below 2^24"""
    if rows > 100000:
        return 2, 2, 1, POW2[:3]          # 4 and 2 * 3 * 1 = 6 per row, 1 050 000 rows: 6.3e6
    if rows > 3000:
        return 6, 6, 2, POW2              # 36 and 6 * 8 * 2 = 96 per row, 70 001 rows: 6.7e6
    return 8, 8, 2, POW2                  # 64 and 8 * 10 * 2 = 160 per row, 3 000 rows: 4.8e5


def channel_params(g, C, am, inv_choices):
    """mean (integers), invstd, gamma (signed powers of two), beta (integers).  Channel 0: gamma > 0, beta = +0; channel 1: gamma < 0,
    beta = -0, so x == mean normalises to exactly +0 in channel 0 and to exactly -0 in channel 1."""
    mean = _ints(g, (C,), am)
    invstd = _pick(g, C, inv_choices)
    gamma = _pick(g, C, POW2) * _pick(g, C, (-1.0, 1.0))
    beta = _ints(g, (C,), 3)
    gamma[0], beta[0] = gamma[0].abs(), 0.0
    gamma[1], beta[1] = -gamma[1].abs(), -0.0
    return mean, invstd, gamma, beta


def check_exact(x, g, mean, invstd, rows_note=""):
    """the 2^24 condition: per column, the sums of |x|, x^2, |g| and |g * xhat| are below 2^24"""
    C = x.shape[-1]
    x2, g2 = x.reshape(-1, C).double(), g.reshape(-1, C).double()
    worst = max(float(x2.abs().sum(0).max()), float((x2 * x2).sum(0).max()), float(g2.abs().sum(0).max()))
    if g2.shape == x2.shape:
        worst = max(worst, float((g2 * xhat(x2, mean, invstd)).abs().sum(0).max()))
    assert worst < LIMIT, f"case {rows_note}: a column sum reaches {worst:g} >= 2^24, the data are not exact"
    return worst


_CASES = {}


def case(rows, C):
    """The [rows, C] case (made once, never modified): x, dout, residual, mean, invstd, gamma, beta, mask (random 4-bit bytes), relu_out
    (a float gate: positive where it passes; +0, -0 or negative where not, independent of mask), c1 / c2 (multiples of 1/8)."""
    key = (rows, C)
    if key not in _CASES:
        g = torch.Generator().manual_seed(rows * 4099 + C)
        ax, ad, am, inv_choices = amplitudes(rows)
        mean, invstd, gamma, beta = channel_params(g, C, am, inv_choices)
        x = _ints(g, (rows, C), ax)
        x[::3, :2] = mean[:2]                                                  # exact zeros of both signs after normalisation
        dout = _ints(g, (rows, C), ad)
        mask = torch.randint(0, 16, (rows * C // 4,), generator=g).to(torch.uint8)
        passes = torch.randint(0, 2, (rows, C), generator=g).bool()
        relu_out = torch.where(passes, torch.randint(1, 6, (rows, C), generator=g).float(), _pick(g, rows * C, (0.0, -0.0, -1.0)).view(rows, C))
        c = {"rows": rows, "C": C, "x": x, "dout": dout, "residual": _ints(g, (rows, C), 4), "mean": mean, "invstd": invstd, "gamma": gamma,
             "beta": beta, "mask": mask, "relu_out": relu_out, "c1": _ints(g, (C,), 16) / 8, "c2": _ints(g, (C,), 16) / 8}
        c["worst"] = check_exact(x, dout, mean, invstd, f"rows={rows} C={C}")
        _CASES[key] = c
    return _CASES[key]


def exact_partial_row(rows, mean, invstd):
    """ONE partial row [1][2][C] (sum x, sum x^2) from which the finalize arithmetic with eps = 0 gives back mean and invstd exactly:
    se = rows * mean, sse = rows * (1 / invstd^2 + mean^2).  Asserts that fp32 holds both and that the fp64 finalize returns the bits."""
    m, i = mean.double(), invstd.double()
    se, sse = rows * m, rows * (1.0 / (i * i) + m * m)
    part = torch.stack([se, sse]).float()
    assert torch.equal(part.double(), torch.stack([se, sse])), "the partial row is not exact in fp32"
    var = part[1].double() / rows - (part[0].double() / rows) ** 2
    assert torch.equal((part[0].double() / rows).float(), mean.float()) and torch.equal((1.0 / torch.sqrt(var)).float(), invstd.float())
    return part.view(1, 2, -1)


STEM_KSP = ((3, 2, 1, False), (2, 2, 0, False), (3, 1, 1, False), (2, 3, 0, False), (5, 3, 2, False), (15, 2, 7, False), (3, 2, 1, True))
STEM_HW = ((1, 1), (1, 9), (7, 1), (13, 10))
STEM_B = (1, 3)
STEM_C = (4, 20, 64)
STEM_LARGE = (2, 37, 41, 64)             # several chunks, cursors that wrap across image rows and across images


def stem_defined(H, W, k, s, p):
    """a pool exists only where the padded image holds one whole window (torch refuses the others: no output size)"""
    return H + 2 * p >= k and W + 2 * p >= k


def stem_cases():
    """(B, H, W, C, k, s, p, ceil) of the GPU grid"""
    out = [(B, H, W, C, k, s, p, ceil) for (k, s, p, ceil) in STEM_KSP for (H, W) in STEM_HW for C in STEM_C for B in STEM_B
           if stem_defined(H, W, k, s, p)]
    return out + [STEM_LARGE + (3, 2, 1, False), STEM_LARGE + (5, 3, 2, False)]


def stem_case(B, H, W, C, k, s, p, ceil):
    """x, dout (pooled), mean, invstd, gamma, beta, Ho, Wo, c1 / c2 and the reference forward (out, idx); most windows hold ties at 0"""
    key = ("stem", B, H, W, C, k, s, p, ceil)
    if key not in _CASES:
        g = torch.Generator().manual_seed(((B * 41 + H) * 43 + W) * 47 + C + k * 1009 + s * 101 + p * 11 + int(ceil))
        Ho, Wo = pool_out_size(H, k, s, p, ceil), pool_out_size(W, k, s, p, ceil)
        mean, invstd, gamma, beta = channel_params(g, C, 2, POW2)
        x = _ints(g, (B, H, W, C), 8)
        dout = _ints(g, (B, Ho, Wo, C), 8)
        c = {"B": B, "H": H, "W": W, "C": C, "k": k, "s": s, "p": p, "Ho": Ho, "Wo": Wo, "x": x, "dout": dout, "mean": mean, "invstd": invstd,
             "gamma": gamma, "beta": beta, "c1": _ints(g, (C,), 16) / 8, "c2": _ints(g, (C,), 16) / 8}
        c["out"], c["idx"] = stem_fwd(x, mean, invstd, gamma, beta, k, s, p, Ho, Wo)
        # |dout| gathered per input pixel bounds the gathered g, and the pooled pass's sums, whatever the order of the windows
        dense = stem_gather(dout.abs(), c["idx"], x, mean, invstd, gamma, beta, k, s, p)
        c["worst"] = max(check_exact(x, dense, mean, invstd, str(key)), check_exact(x, dout, mean, invstd, str(key)))
        _CASES[key] = c
    return _CASES[key]
