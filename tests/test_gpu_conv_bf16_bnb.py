"""zsg_conv_igemm_bf16_bnb / _bnb_supported (csrc/igemm_bf16.hip) through the C ABI: the bf16 MFMA data gradient that completes the dout
of a BatchNorm and writes that BatchNorm's backward partial rows [m_tiles][2][N] (enc_bwd_dtype = "bf16"), on data-gradient descriptors
(ops.dgrad_desc; the weight operand is the packed image of the transposed filter WT[cin][k][k][cout]).

Every case runs with and without add_src (aliasing out), with and without mask bits, with epi_flags 0 and 1, on the tile hints 0, 64x64,
128x64 and 128x128 (all three tiles are served).  Bounds, none taken from what the code gives:
  * integer data (dy in [-2, 2], weights in [-1, 1], add_src in [-2, 2], bn_x in [-3, 3], integer mean, invstd a power of two): make_case
    asserts on an int64 reference that every value, and for BM = 64 and 128 every tile's sum of |g| and of |g * xhat| (in units of the
    smallest invstd), stays below 2^24 — every fp32 operation on such values is exact in any order, fused or not, so out and both partial
    rows must equal the integer arithmetic with zero tolerance;
  * standard-normal data: with epi_flags = 0 out must be bit-equal to zsg_conv_igemm_bf16_m's (NULL mask, the same add_src), with
    epi_flags = 1 to that result with the bits applied.  The partial rows are compared with fp64 sums over the kernel's OWN stored rows
    (masked on the host where the kernel stored v) and the given bn_x, mean and invstd.  A tile sums at most BM values per column with
    BM - 1 fp32 additions in a fixed order (include/zsg.h), each off by at most 2^-24 of a partial sum that is at most sum |g|:
    |sum g - ref| <= (BM - 1) * 2^-24 * sum |g|.  A term of the second row carries at most three more fp32 roundings (x - mean, * invstd,
    * g; fewer where the compiler fuses): (BM + 2) * 2^-24 * sum |g * xhat| to first order, (BM + 3) with the second-order terms.
The tile -> partial-row attribution is computed here from zsg_conv_igemm_bf16_partial_rows (of the descriptor without the epi_flags bit)
and BM (one segment: tile t holds the rows [t * BM, min(rows, (t + 1) * BM)))."""
import ctypes as C
import functools
import itertools
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

HINTS = (0, (64, 64), (128, 64), (128, 128))
SENTINEL = -12345.5
PAD_ROWS = 3            # sentinel rows kept behind the partial rows the launch may write
GUARD = 64              # sentinel elements kept behind out
VARIANTS = list(itertools.product((False, True), (False, True), (0, 1)))       # (add_src aliasing out, mask bits, epi_flags)

# name -> (H, W, B, Cin = GEMM N, Cout = reduction C, k, pad) of a stride-1 convolution Cin -> Cout whose data gradient is run
CASES = {
    "pw_tail": (9, 9, 2, 256, 64, 1, 0),          # 1x1, 162 rows: the last M tile partly invalid at BM 64 and 128
    "c3": (10, 10, 2, 64, 64, 3, 1),              # 3x3 / pad 1, 200 rows: border taps, N < BN at BN = 128
    "full": (8, 8, 4, 128, 256, 1, 0),            # 1x1, 256 rows, C = 256: exact multiples, several tiles, four K tiles
    "n192": (10, 10, 1, 192, 64, 1, 0),           # N = 192: a column tile past N (192 against 128 / 256)
}


@pytest.fixture(scope="module")
def Z():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib, ops
    return _lib, ops


def dgrad_ref(dy, wt, k, p):
    """dy [B, H, W, Cout], wt = WT [Cin, k, k, Cout] of one dtype (int64 / float64) -> dx [B * H * W, Cin] of the stride-1 convolution:
    dx[y, x, ci] = sum over (ty, tx, co) of dy[y + p - ty, x + p - tx, co] * WT[ci, ty, tx, co], tap by tap in that dtype's own arithmetic"""
    B, H, W, Co = dy.shape
    q = k - 1 - p
    buf = torch.zeros(B, H + 2 * q, W + 2 * q, Co, dtype=dy.dtype)
    buf[:, q:q + H, q:q + W] = dy
    out = torch.zeros(B * H * W, wt.shape[0], dtype=dy.dtype)
    for ty in range(k):
        for tx in range(k):
            win = buf[:, k - 1 - ty: k - 1 - ty + H, k - 1 - tx: k - 1 - tx + W]
            out += torch.matmul(win.reshape(-1, Co), wt[:, ty, tx].t())
    return out


def bits_of(mask_bytes, rows, N):
    """[rows, N] bool of the 4-bits-per-byte mask (byte o >> 2, bit o & 3 of the element offset o = row * N + n)"""
    b = mask_bytes.to(torch.int32).view(-1, 1)
    return ((b >> torch.arange(4, dtype=torch.int32).view(1, 4)) & 1).bool().view(rows, N)


@functools.lru_cache(maxsize=None)
def make_case(name, kind):
    """operands (CPU) of one case and, for integer data, the int64 references of every variant — computed once, shared, never modified"""
    H, W, B, N, Cc, k, p = CASES[name]
    rows = B * H * W
    g = torch.Generator().manual_seed(700 + sorted(CASES).index(name) * 2 + (kind == "int"))
    want_rows = {"pw_tail": 162, "c3": 200, "full": 256, "n192": 100}[name]
    assert rows == want_rows
    assert {"pw_tail": rows % 64 != 0 and rows % 128 != 0, "c3": N < 128 and k == 3, "full": rows % 128 == 0 and Cc == 256,
            "n192": N % 128 != 0 and N % 64 == 0}[name]
    mask = torch.randint(0, 16, (rows * N // 4,), generator=g).to(torch.uint8)
    cs = dict(rows=rows, mask=mask, bits=bits_of(mask, rows, N))
    if kind == "int":
        dy = torch.randint(-2, 3, (B, H, W, Cc), generator=g).float()
        wt = torch.randint(-1, 2, (N, k, k, Cc), generator=g).float()
        add = torch.randint(-2, 3, (rows, N), generator=g).float()
        x = torch.randint(-3, 4, (rows, N), generator=g).float()
        mean = torch.randint(-1, 2, (N,), generator=g).float()
        e = torch.randint(-1, 2, (N,), generator=g)
        invstd = torch.pow(2.0, e.float())                     # 0.5, 1, 2
        acc = dgrad_ref(dy.to(torch.int64), wt.to(torch.int64), k, p)
        xh2 = (x.to(torch.int64) - mean.to(torch.int64)) * (2 * invstd).to(torch.int64)          # xhat in units of 0.5
        ref = {}
        for has_add, has_mask in itertools.product((False, True), (False, True)):
            v = acc + (add.to(torch.int64) if has_add else 0)
            gi = v * cs["bits"].to(torch.int64) if has_mask else v
            assert int(v.abs().max()) < 2 ** 24
            for bm in (64, 128):      # every partial sum on the way is exactly representable, whatever the order
                for t in range(0, rows, bm):
                    assert int(gi[t:t + bm].abs().sum(0).max()) < 2 ** 24 and int((gi[t:t + bm] * xh2[t:t + bm]).abs().sum(0).max()) < 2 ** 24
            ref[(has_add, has_mask)] = (v, gi, gi * xh2)
        cs.update(ref=ref)
    else:
        dy = torch.randn(B, H, W, Cc, generator=g)
        wt = torch.randn(N, k, k, Cc, generator=g)
        add = torch.randn(rows, N, generator=g)
        x = torch.randn(rows, N, generator=g)
        mean = 0.1 * torch.randn(N, generator=g)
        invstd = 0.5 + 1.5 * torch.rand(N, generator=g)
    cs.update(dy=dy, wt=wt, add=add, x=x, mean=mean, invstd=invstd)
    return cs


def pack(L, w):
    N, k, _, Cc = w.shape
    c8 = (Cc + 7) // 8 * 8
    wd = w.contiguous().cuda()
    wp = torch.full((N, k * k, c8), 0x5555, dtype=torch.int16, device="cuda")
    job = struct.pack("<qqiiiiiiii", wd.data_ptr(), wp.data_ptr(), N, k * k, Cc, 0, Cc, c8, 0, 0)
    dev = torch.frombuffer(bytearray(job), dtype=torch.uint8).cuda()
    L.check(L.lib.zsg_pack_w_bf16_batched(dev.data_ptr(), 1, (N * k * k * c8 // 8 + 255) // 256, L.stream_ptr()), "pack")
    torch.cuda.synchronize()
    return wp


@functools.lru_cache(maxsize=None)
def device_case(name, kind):
    """the case's read-only operands on the device (uploaded and packed once)"""
    from zsgnet_pytorch_amd import _lib as L
    cs = make_case(name, kind)
    return dict(dy=cs["dy"].reshape(-1).cuda(), wp=pack(L, cs["wt"]), x=cs["x"].reshape(-1).cuda(), mean=cs["mean"].cuda(),
                invstd=cs["invstd"].cuda(), mask=cs["mask"].cuda(), add=cs["add"].reshape(-1).cuda())


def launch(Z, name, kind, hint, has_add, has_mask, epi, entry="bnb"):
    """run one variant; returns (out [rows, N], partial buffer [prow + PAD_ROWS, 2, N] or None, partial rows, BM)"""
    L, ops = Z
    H, W, B, N, Cc, k, p = CASES[name]
    cs, dv = make_case(name, kind), device_case(name, kind)
    rows = cs["rows"]
    out = torch.full((rows * N + GUARD,), SENTINEL, device="cuda")
    out[:rows * N] = dv["add"] if has_add else float("nan")
    dyv = ops.TView(dv["dy"], B, Cc, Cc, [ops.Level(0, H, W, H * W * Cc)])
    dxv = ops.TView(out, B, N, N, [ops.Level(0, H, W, H * W * N)])
    desc = ops.dgrad_desc(dyv, dxv, Cc, N, k, 1, p, 1, tile_hint=0 if hint == 0 else ops.tile_hint(hint[0], hint[1], 1))
    assert not desc.zero_fill and desc.nseg == 1
    add_ptr = out.data_ptr() if has_add else None
    if entry == "m":
        L.check(L.lib.zsg_conv_igemm_bf16_m(C.byref(desc), dv["dy"].data_ptr(), dv["wp"].data_ptr(), out.data_ptr(), None, add_ptr, None,
                                            L.stream_ptr()), "bf16_m")
        torch.cuda.synchronize()
        assert bool((out[rows * N:] == SENTINEL).all())
        return out[:rows * N].cpu().view(rows, N), None, 0, 0
    prow = int(L.lib.zsg_conv_igemm_bf16_partial_rows(C.byref(desc)))          # (asked without the bit: that function refuses epi_flags)
    desc.epi_flags = epi
    assert L.lib.zsg_conv_igemm_bf16_bnb_supported(C.byref(desc)) == 1
    bms = [bm for bm in (64, 128) if (rows + bm - 1) // bm == prow]
    if hint != 0:
        assert bms and hint[0] in bms, f"{name} hint {hint}: {prow} partial rows for {rows} rows"
        bm = hint[0]
    else:
        assert bms, f"{name}: the heuristic's {prow} partial rows fit neither BM"
        bm = bms[0]
    part = torch.full((prow + PAD_ROWS, 2, N), SENTINEL, device="cuda")
    L.check(L.lib.zsg_conv_igemm_bf16_bnb(C.byref(desc), dv["dy"].data_ptr(), dv["wp"].data_ptr(), out.data_ptr(), add_ptr, dv["x"].data_ptr(),
                                          dv["mean"].data_ptr(), dv["invstd"].data_ptr(), dv["mask"].data_ptr() if has_mask else None,
                                          part.data_ptr(), L.stream_ptr()), "bf16_bnb")
    torch.cuda.synchronize()
    assert bool((out[rows * N:] == SENTINEL).all()), f"{name} hint {hint}: written behind out"
    return out[:rows * N].cpu().view(rows, N), part.cpu(), prow, bm


def check_frame(name, hint, var, out, part, prow):
    """nothing behind m_tiles rows or N columns is written, every element inside is"""
    assert not torch.isnan(out).any() and not bool((out == SENTINEL).any()), f"{name} hint {hint} {var}: unwritten output elements"
    assert bool((part[prow:] == SENTINEL).all()), f"{name} hint {hint} {var}: rows >= partial_rows changed"
    assert not bool((part[:prow] == SENTINEL).any()) and not torch.isnan(part[:prow]).any(), \
        f"{name} hint {hint} {var}: an element of [m_tiles][2][N] was not written"


@pytest.mark.parametrize("name", sorted(CASES))
def test_integer_data_is_exact(Z, name):
    cs = make_case(name, "int")
    for hint in HINTS:
        for var in VARIANTS:
            has_add, has_mask, epi = var
            v, gi, gx2 = cs["ref"][(has_add, has_mask)]
            out, part, prow, bm = launch(Z, name, "int", hint, *var)
            check_frame(name, hint, var, out, part, prow)
            want = (gi if epi else v).float()
            assert torch.equal(out + 0.0, want + 0.0) and torch.equal(out.double(), want.double()), f"{name} hint {hint} {var}: out"
            for t in range(prow):
                sl = slice(t * bm, (t + 1) * bm)
                assert torch.equal(part[t, 0].double(), gi[sl].sum(0).double()), f"{name} hint {hint} {var} tile {t}: sum g"
                assert torch.equal(part[t, 1].double(), gx2[sl].sum(0).double() / 2), f"{name} hint {hint} {var} tile {t}: sum g * xhat"


@pytest.mark.parametrize("name", sorted(CASES))
def test_random_data_out_bit_equal_and_partials_within_the_summation_bound(Z, name):
    cs = make_case(name, "rand")
    xh = (cs["x"].double() - cs["mean"].double()) * cs["invstd"].double()
    worst = [0.0, 0.0]
    for hint in HINTS:
        plain = {a: launch(Z, name, "rand", hint, a, False, 0, entry="m")[0] for a in (False, True)}
        for var in VARIANTS:
            has_add, has_mask, epi = var
            out, part, prow, bm = launch(Z, name, "rand", hint, *var)
            check_frame(name, hint, var, out, part, prow)
            bits = cs["bits"] if has_mask else torch.ones_like(cs["bits"])
            want = torch.where(bits, plain[has_add], torch.zeros(())) if epi else plain[has_add]
            assert torch.equal(out.view(torch.int32), want.view(torch.int32)), f"{name} hint {hint} {var}: out differs from zsg_conv_igemm_bf16_m"
            gk = torch.where(bits, out, torch.zeros(())).double()         # the kernel's own g (where it stored g the bits change nothing)
            for t in range(prow):
                sl = slice(t * bm, (t + 1) * bm)
                for which, (term, k_) in enumerate(((gk[sl], bm - 1), (gk[sl] * xh[sl], bm + 3))):
                    err = (part[t, which].double() - term.sum(0)).abs()
                    bound = k_ * 2.0 ** -24 * term.abs().sum(0)
                    frac = float((err / bound.clamp(min=1e-300)).max())
                    worst[which] = max(worst[which], frac)
                    assert bool((err <= bound).all()), f"{name} hint {hint} {var} tile {t} [{which}]: max error / bound = {frac:.3f}"
    print(f"bf16_bnb {name}: largest |partial - fp64 sum| / bound over all hints and variants: sum g {worst[0]:.4f}, sum g * xhat {worst[1]:.4f}")


def test_two_runs_write_identical_bits(Z):
    for name in ("pw_tail", "c3"):
        for hint in HINTS:
            a, pa, _, _ = launch(Z, name, "rand", hint, True, True, 1)
            b, pb, _, _ = launch(Z, name, "rand", hint, True, True, 1)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(pa.view(torch.int32), pb.view(torch.int32)), (name, hint)


def test_refusals_launch_nothing(Z):
    L, ops = Z
    dy = torch.zeros(2 * 8 * 8 * 64, device="cuda")
    o = torch.full((2 * 8 * 8 * 64,), 3.0, device="cuda")
    x = torch.zeros(2 * 8 * 8 * 64, device="cuda")
    mu, iv = torch.zeros(64, device="cuda"), torch.ones(64, device="cuda")
    part = torch.full((8 * 2 * 64 + 4,), SENTINEL, device="cuda")
    wp = torch.zeros(64 * 64, dtype=torch.int16, device="cuda")
    lv = [ops.Level(0, 8, 8, 8 * 8 * 64)]

    def desc(N=64, **kw):
        d = ops.dgrad_desc(ops.TView(dy, 2, 64, 64, lv), ops.TView(o, 2, N, 64, lv), 64, N, 1, 1, 0, 1)
        for k_, v in kw.items():
            setattr(d, k_, v)
        return d

    def call(d, op=None, xp=None, mp=None, ip=None, pp=None, null=()):
        a = dict(o=op or o.data_ptr(), x=xp or x.data_ptr(), m=mp or mu.data_ptr(), i=ip or iv.data_ptr(), p=pp or part.data_ptr())
        for n_ in null:
            a[n_] = None
        rc = L.lib.zsg_conv_igemm_bf16_bnb(C.byref(d), dy.data_ptr(), wp.data_ptr(), a["o"], None, a["x"], a["m"], a["i"], None, a["p"], L.stream_ptr())
        return rc, L.lib.zsg_last_error().decode()
    bad = {
        "epi_flags bit 1": desc(epi_flags=2),
        "epi_flags bits 0 and 1": desc(epi_flags=3),
        "relu": desc(relu=1),
        "N % 4": desc(N=62),
        "merge_x": desc(merge_x=1),
        "split-K": desc(tile_hint=ops.tile_hint(64, 64, 2)),
        "stream-K": desc(tile_hint=ops.tile_hint(64, 64, 1) | (1 << 28)),
        "out_ld % 4": desc(out_ld=66),
    }
    for what, d in bad.items():
        assert L.lib.zsg_conv_igemm_bf16_bnb_supported(C.byref(d)) == 0, what
        rc, msg = call(d)
        assert rc == -1 and "conv_igemm_bf16_bnb" in msg and len(msg) > 30, (what, rc, msg)
    good = desc(epi_flags=1)
    assert L.lib.zsg_conv_igemm_bf16_bnb_supported(C.byref(good)) == 1
    ptrs = {"misaligned partials": dict(pp=part.data_ptr() + 4), "null partials": dict(null=("p",)), "misaligned out": dict(op=o.data_ptr() + 4),
            "misaligned bn_x": dict(xp=x.data_ptr() + 4), "null bn_x": dict(null=("x",)), "misaligned bn_mean": dict(mp=mu.data_ptr() + 4),
            "null bn_mean": dict(null=("m",)), "misaligned bn_invstd": dict(ip=iv.data_ptr() + 4), "null bn_invstd": dict(null=("i",))}
    for what, kw in ptrs.items():
        rc, msg = call(good, **kw)
        assert rc == -1 and "conv_igemm_bf16_bnb" in msg and any(w in msg for w in ("partials", "out", "bn_x", "null argument")), (what, rc, msg)
    torch.cuda.synchronize()
    assert float(o.min()) == 3.0 and float(o.max()) == 3.0, "a refused call must launch nothing"
    assert bool((part == SENTINEL).all()), "a refused call must launch nothing"
    good.tile_hint = ops.tile_hint(64, 64, 1)
    rc, msg = call(good)
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert float(o.abs().max()) == 0.0 and float(part[:2 * 2 * 64].abs().max()) == 0.0 and bool((part[2 * 2 * 64:] == SENTINEL).all())
