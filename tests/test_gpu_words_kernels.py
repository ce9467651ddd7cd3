"""csrc/words.hip through the C ABI: zsg_head_words_conv0 and zsg_head_words_conv0_bwd (include/zsg.h), every output between canaries.

IDENTITIES that need no tolerance pin the arithmetic order: Vw = 0 gives zsg_head_shared_conv0's bits (and dYq = dy, dKw = 0), every
len = 1 gives zsg_head_film_conv0's for gamma = Vw[:, 0] (alpha = 1 exactly), len = 0 rows are concat's; rows t >= len of Kw / Vw are never
read (NaN there changes no bit) and rows t >= len of dKw / dVw / alpha are exact zeros; two launches give the same bits; an out-of-range
index gives NaN rows, zero gradients and reads nothing.
RANDOM inputs are compared with tests/words_ref.py's attention on the same operands: the truth is its float64 evaluation, the yardstick
its float32 CPU evaluation, and the GPU may be 6 x as far from the truth as the yardstick + 1e-4 (max-abs, tests/test_gpu_film_net.py's
factor).  Shapes: T at 1, 64 and around the kernel's token chunk (16 tokens staged in LDS at N <= 256; longer phrases read global
memory), lens mixing 0, 1, mid and T in one launch, N = 8 (two live lanes per wave) and 256 (one 16-byte group per lane)."""
import math

import pytest
import torch
import torch.nn.functional as F

import words_ref as WR

pytestmark = pytest.mark.gpu

SIZES_300 = [(38, 38), (19, 19), (10, 10), (5, 5), (3, 3)]
LEVELS = {"1level": [(5, 5)], "3levels": [(3, 4), (2, 2), (1, 1)]}
# (Q, Bi, unused slot, identity index): tests/test_gpu_film_kernels.py's set
GEOM = {"q1b1": (1, 1, None, False), "q6b1": (6, 1, None, False), "q6b3": (6, 3, None, False), "q16b4": (16, 4, None, False),
        "q8b4_unused2": (8, 4, 2, False), "q5b5_null": (5, 5, None, True)}
CHUNK = 16                      # words_chunk(N) of csrc/words.hip at N <= 256
TOKENS = [1, CHUNK - 1, CHUNK, CHUNK + 1, 64]
CANARY = 1024
MARK = 12345.0
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import zsgnet_pytorch_amd._lib as L
    return L


class Guarded:
    """a device buffer of n elements between two canary runs, pre-filled with `fill`"""

    def __init__(self, n, dtype=torch.float32, fill=NAN):
        self.buf = torch.full((2 * CANARY + n,), fill, dtype=dtype, device="cuda")
        self.buf[:CANARY] = MARK
        self.buf[-CANARY:] = MARK
        self.view = self.buf[CANARY:CANARY + n]

    def intact(self):
        return bool((self.buf[:CANARY] == MARK).all()) and bool((self.buf[-CANARY:] == MARK).all())


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def make_idx(Q, Bi, g, unused=None):
    live = [i for i in range(Bi) if i != unused]
    extra = torch.tensor(live)[torch.randint(0, len(live), (max(Q - len(live), 0),), generator=g)]
    idx = torch.cat([torch.tensor(live), extra])[:Q]
    return idx[torch.randperm(Q, generator=g)].long()


def mixed_lens(Q, T):
    """0, 1, mid and T within one launch (Q = 1: T)"""
    pat = [T, 0, 1, max(1, T // 2)]
    return torch.tensor([float(pat[q % 4]) for q in range(Q)])


def operands(sizes, Q, Bi, N, T, seed, lens=None):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(Y=[r(Bi, h, w, N) for h, w in sizes], G=[r(h, w, N) for h, w in sizes], dy=[r(Q, h, w, N) for h, w in sizes], V=r(Q, N, 9),
                bias=r(N), Kw=r(Q, T, N), Vw=0.5 * r(Q, T, N), lens=mixed_lens(Q, T) if lens is None else lens)


def pack(levels):
    return torch.cat([x.reshape(-1) for x in levels]).cuda()


def unpack(flat, B, sizes, N):
    out, p0 = [], 0
    for h, w in sizes:
        out.append(flat[B * p0 * N:B * (p0 + h * w) * N].view(B, h, w, N))
        p0 += h * w
    return out


def hw_of(sizes):
    return torch.tensor([v for s_ in sizes for v in s_], dtype=torch.int32)


def dev_idx(idx, i64, null):
    if null:
        return None, 0
    t = idx.cuda() if i64 else idx.int().cuda()
    return t, t.data_ptr()


def run_forward(L, d, idx_ptr, i64, Bi, Q, sizes, N, T, bf16=False, fill=NAN, kind="words", want_alpha=True):
    """(h1 flat, alpha flat or None).  kind = shared / film run the kernels the identities name (film: gamma = Vw[:, 0])"""
    P = sum(h * w for h, w in sizes)
    hw = hw_of(sizes)
    out = Guarded(Q * P * N, torch.bfloat16 if bf16 else torch.float32, fill)
    al = Guarded(Q * P * T, fill=fill)
    Yd, Gd, Vd, bd = pack(d["Y"]), pack(d["G"]), d["V"].reshape(-1).cuda(), d["bias"].cuda()
    if kind == "shared":
        fn = L.lib.zsg_head_shared_conv0_bf16 if bf16 else L.lib.zsg_head_shared_conv0
        rc = fn(Yd.data_ptr(), idx_ptr, i64, bd.data_ptr(), Gd.data_ptr(), Vd.data_ptr(), Bi, Q, len(sizes), hw.data_ptr(), N, out.view.data_ptr(), L.stream_ptr())
    elif kind == "film":
        gd = d["Vw"][:, 0].contiguous().reshape(-1).cuda()
        rc = L.lib.zsg_head_film_conv0(Yd.data_ptr(), idx_ptr, i64, bd.data_ptr(), Gd.data_ptr(), Vd.data_ptr(), gd.data_ptr(), Bi, Q, len(sizes),
                                       hw.data_ptr(), N, out.view.data_ptr(), int(bf16), L.stream_ptr())
    else:
        Kd, Wd, ld = d["Kw"].reshape(-1).cuda(), d["Vw"].reshape(-1).cuda(), d["lens"].cuda()
        rc = L.lib.zsg_head_words_conv0(Yd.data_ptr(), idx_ptr, i64, bd.data_ptr(), Gd.data_ptr(), Vd.data_ptr(), Kd.data_ptr(), Wd.data_ptr(), ld.data_ptr(),
                                        1.0 / math.sqrt(N), Bi, Q, T, len(sizes), hw.data_ptr(), N, out.view.data_ptr(), int(bf16),
                                        al.view.data_ptr() if want_alpha else None, L.stream_ptr())
    L.check(rc, "head conv0 " + kind)
    torch.cuda.synchronize()
    assert out.intact() and al.intact(), "a canary around h1 / alpha was overwritten"
    if kind == "words" and not want_alpha:
        assert bool((torch.isnan(al.view) if fill != fill else al.view == fill).all()), "alpha was written without being asked for"
    return out.view.clone().cpu(), (al.view.clone().cpu() if kind == "words" and want_alpha else None)


def run_backward(L, d, alpha, idx_ptr, i64, Bi, Q, sizes, N, T, fill=NAN, outs=(True, True, True)):
    """(dYq flat, dKw [Q, T, N], dVw [Q, T, N]) — None where outs says so"""
    P = sum(h * w for h, w in sizes)
    hw = hw_of(sizes)
    nws = int(L.lib.zsg_head_words_bwd_ws_bytes(Q, T, len(sizes), hw.data_ptr(), N))
    assert nws > 0
    ws = Guarded((nws + 7) // 8, torch.float64, fill)
    dYq, dK, dV = Guarded(Q * P * N, fill=fill), Guarded(Q * T * N, fill=fill), Guarded(Q * T * N, fill=fill)
    dyd, Yd, Kd, Wd, ld, ad = pack(d["dy"]), pack(d["Y"]), d["Kw"].reshape(-1).cuda(), d["Vw"].reshape(-1).cuda(), d["lens"].cuda(), alpha.cuda()
    rc = L.lib.zsg_head_words_conv0_bwd(dyd.data_ptr(), Yd.data_ptr(), idx_ptr, i64, Kd.data_ptr(), Wd.data_ptr(), ad.data_ptr(), ld.data_ptr(),
                                        1.0 / math.sqrt(N), Bi, Q, T, len(sizes), hw.data_ptr(), N, dYq.view.data_ptr() if outs[0] else None,
                                        dK.view.data_ptr() if outs[1] else None, dV.view.data_ptr() if outs[2] else None, ws.view.data_ptr(), nws,
                                        L.stream_ptr())
    L.check(rc, "head words conv0 bwd")
    torch.cuda.synchronize()
    assert dYq.intact() and dK.intact() and dV.intact() and ws.intact(), "a canary around a gradient or the workspace was overwritten"
    for o, g in zip(outs, (dYq, dK, dV)):
        if not o:
            assert bool((torch.isnan(g.view) if fill != fill else g.view == fill).all()), "an output was written without being asked for"
    return (dYq.view.clone().cpu() if outs[0] else None, dK.view.clone().cpu().view(Q, T, N) if outs[1] else None,
            dV.view.clone().cpu().view(Q, T, N) if outs[2] else None)


def fold(L, dyq, idx, Bi, Q, sizes, N):
    """zsg_head_shared_conv0_bwd: the segmented sum of per-query rows into the per-image accumulator"""
    P = sum(h * w for h, w in sizes)
    hw = hw_of(sizes)
    out = Guarded(Bi * P * N)
    src, it = dyq.cuda(), idx.cuda()
    L.check(L.lib.zsg_head_shared_conv0_bwd(src.data_ptr(), it.data_ptr(), 1, Bi, Q, len(sizes), hw.data_ptr(), N, out.view.data_ptr(), L.stream_ptr()), "fold")
    torch.cuda.synchronize()
    assert out.intact()
    return out.view.clone().cpu()


def alpha_rows(alpha, Q, sizes, T):
    """[Q, P, T] from the level-major packed alpha"""
    out, p0 = [], 0
    for h, w in sizes:
        out.append(alpha[Q * p0 * T:Q * (p0 + h * w) * T].view(Q, h * w, T))
        p0 += h * w
    return torch.cat(out, dim=1)


def setup(geom, seed):
    Q, Bi, unused, null = geom
    g = torch.Generator().manual_seed(seed)
    idx = torch.arange(Q) if null else make_idx(Q, Bi, g, unused)
    return Q, Bi, null, idx


# ---- identities -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8, 256])
@pytest.mark.parametrize("lv", list(LEVELS))
@pytest.mark.parametrize("geom", list(GEOM))
def test_zero_value_rows_are_the_shared_kernels(L, geom, lv, N):
    """Vw = 0: forward bits of zsg_head_shared_conv0 (fp32 and bf16), dYq folded == zsg_head_shared_conv0_bwd(dy), dKw == 0; int32 / int64 / NULL"""
    sizes, T = LEVELS[lv], 5
    Q, Bi, null, idx = setup(GEOM[geom], sum(map(ord, geom + lv)) + N)
    d = operands(sizes, Q, Bi, N, T, seed=N + len(geom))
    d["Vw"] = torch.zeros_like(d["Vw"])
    keep, ptr = dev_idx(idx, 1, False)                       # (the shared kernels need an index: the identity is passed explicitly to them)
    want = run_forward(L, d, ptr, 1, Bi, Q, sizes, N, T, kind="shared")[0]
    want16 = run_forward(L, d, ptr, 1, Bi, Q, sizes, N, T, kind="shared", bf16=True)[0]
    for i64 in ((1,) if null else (1, 0)):
        keep2, ptr2 = dev_idx(idx, i64, null)
        f, al = run_forward(L, d, ptr2, i64, Bi, Q, sizes, N, T)
        assert torch.equal(bits(f), bits(want)), "Vw = 0: not zsg_head_shared_conv0's bits"
        assert torch.equal(bits(run_forward(L, d, ptr2, i64, Bi, Q, sizes, N, T, bf16=True, want_alpha=False)[0]), bits(want16))
        dYq, dK, dV = run_backward(L, d, al, ptr2, i64, Bi, Q, sizes, N, T)
        assert torch.equal(dYq, pack(d["dy"]).cpu()), "Vw = 0: dYq must carry dy's values"
        assert torch.equal(fold(L, dYq, idx, Bi, Q, sizes, N), fold(L, pack(d["dy"]).cpu(), idx, Bi, Q, sizes, N))
        assert not dK.any(), "Vw = 0: dKw must be 0"
        assert dV[d["lens"] > 0].any() or not (d["lens"] > 0).any()


@pytest.mark.parametrize("N", [8, 256])
@pytest.mark.parametrize("geom", ["q1b1", "q6b3", "q8b4_unused2", "q5b5_null"])
def test_single_token_phrases_are_film(L, geom, N):
    """every len = 1: alpha = 1 exactly, so the forward has zsg_head_film_conv0's bits for gamma = Vw[:, 0]; also the bf16 store"""
    sizes, T = LEVELS["3levels"], 3
    Q, Bi, null, idx = setup(GEOM[geom], 11 + N)
    d = operands(sizes, Q, Bi, N, T, seed=N + 5, lens=torch.ones(Q))
    keep, ptr = dev_idx(idx, 1, null)
    f, al = run_forward(L, d, ptr, 1, Bi, Q, sizes, N, T)
    assert torch.equal(bits(f), bits(run_forward(L, d, ptr, 1, Bi, Q, sizes, N, T, kind="film")[0])), "len = 1: not zsg_head_film_conv0's bits"
    a = alpha_rows(al, Q, sizes, T)
    assert bool((a[:, :, 0] == 1).all()) and not a[:, :, 1:].any()
    h = run_forward(L, d, ptr, 1, Bi, Q, sizes, N, T, bf16=True)[0]
    assert torch.equal(bits(h), bits(run_forward(L, d, ptr, 1, Bi, Q, sizes, N, T, kind="film", bf16=True)[0]))
    assert torch.equal(bits(h), bits(f.to(torch.bfloat16))), "the bf16 store is not the fp32 result rounded to nearest-even"


@pytest.mark.parametrize("N", [8, 256])
@pytest.mark.parametrize("T", TOKENS)
def test_padding_rows_are_never_read_and_get_exact_zeros(L, T, N):
    """NaN in Kw / Vw at t >= len and NaN-prefilled outputs: finite, bit-equal to the run with zeros there (and to a second launch over
    buffers that held something else); rows t >= len of dKw / dVw / alpha are exact zeros; len = 0 rows are concat's bits"""
    sizes = LEVELS["3levels"]
    Q, Bi, null, idx = setup(GEOM["q6b3"], 100 + T + N)
    d = operands(sizes, Q, Bi, N, T, seed=T * 3 + N)
    lens = d["lens"].long()
    tt = torch.arange(T)[None, :, None]
    padmask = (tt >= lens[:, None, None]).expand(Q, T, N)
    clean = dict(d, Kw=d["Kw"].masked_fill(padmask, 0.0), Vw=d["Vw"].masked_fill(padmask, 0.0))
    poison = dict(d, Kw=d["Kw"].masked_fill(padmask, NAN), Vw=d["Vw"].masked_fill(padmask, NAN))
    keep, ptr = dev_idx(idx, 1, False)
    f0, a0 = run_forward(L, clean, ptr, 1, Bi, Q, sizes, N, T, fill=7.0)
    f1, a1 = run_forward(L, poison, ptr, 1, Bi, Q, sizes, N, T)
    assert torch.isfinite(f1).all() and torch.isfinite(a1).all()
    assert torch.equal(bits(f0), bits(f1)) and torch.equal(bits(a0), bits(a1))
    ar = alpha_rows(a1, Q, sizes, T)
    assert not ar.masked_select((tt >= lens[:, None, None]).permute(0, 2, 1).expand_as(ar)).any(), "alpha at t >= len must be exactly 0"
    live = lens > 0
    assert bool(((ar.sum(2) - 1).abs()[live] < 1e-5).all()) and not ar[~live].any()
    shared = unpack(run_forward(L, d, ptr, 1, Bi, Q, sizes, N, T, kind="shared")[0], Q, sizes, N)
    for o, r in zip(unpack(f1, Q, sizes, N), shared):
        assert torch.equal(bits(o[~live]), bits(r[~live])), "len = 0 rows must carry concat's bits"
    g0 = run_backward(L, clean, a0, ptr, 1, Bi, Q, sizes, N, T, fill=7.0)
    g1 = run_backward(L, poison, a1, ptr, 1, Bi, Q, sizes, N, T)
    for x0, x1, name in zip(g0, g1, ("dYq", "dKw", "dVw")):
        assert torch.isfinite(x1).all(), name
        assert torch.equal(bits(x0), bits(x1)), name
    for x, name in ((g1[1], "dKw"), (g1[2], "dVw")):
        assert not x.masked_select(padmask).any(), name + " at t >= len must be exactly 0"
        assert bool((bits(x).view(Q, T, N).masked_select(padmask) == 0).all()), name + ": +0, not -0"
        has = live if name == "dVw" else lens >= 2           # (one token: alpha = 1 whatever the score, so dKw is 0 by the formula)
        assert x[has][:, 0].any() or not has.any()
    assert not g1[1][lens == 1].any()
    # the outputs one by one (a frozen consumer passes NULL for the others): the same bits
    only = run_backward(L, poison, a1, ptr, 1, Bi, Q, sizes, N, T, outs=(False, True, False))
    assert torch.equal(bits(only[1]), bits(g1[1]))
    only = run_backward(L, poison, a1, ptr, 1, Bi, Q, sizes, N, T, outs=(False, False, True))          # (dVw alone: the pixel launch is skipped)
    assert torch.equal(bits(only[2]), bits(g1[2]))
    only = run_backward(L, poison, a1, ptr, 1, Bi, Q, sizes, N, T, outs=(True, False, True))
    assert torch.equal(bits(only[0]), bits(g1[0])) and torch.equal(bits(only[2]), bits(g1[2]))


@pytest.mark.parametrize("i64", [1, 0], ids=["int64", "int32"])
def test_out_of_range_index(L, i64):
    """NaN rows in h1, zero alpha / dYq / dKw / dVw rows, canaries intact (checked by every run_*); the live queries as without the bad ones"""
    sizes, Q, Bi, N, T = [(3, 4), (2, 2), (1, 1)], 5, 2, 8, 4
    d = operands(sizes, Q, Bi, N, T, 77, lens=torch.tensor([4.0, 3.0, 2.0, 1.0, 4.0]))
    idx = torch.tensor([1, 7, -1, 0, 2], dtype=torch.long)
    keep, ptr = dev_idx(idx, i64, False)
    f, al = run_forward(L, d, ptr, i64, Bi, Q, sizes, N, T)
    good = torch.tensor([1, 0, 0, 0, 0])
    keep2, ptr2 = dev_idx(good, i64, False)
    f2, al2 = run_forward(L, d, ptr2, i64, Bi, Q, sizes, N, T)
    bad = torch.tensor([False, True, True, False, True])
    for o, r in zip(unpack(f, Q, sizes, N), unpack(f2, Q, sizes, N)):
        assert torch.isnan(o[bad]).all() and torch.equal(bits(o[~bad]), bits(r[~bad]))
    a, a2 = alpha_rows(al, Q, sizes, T), alpha_rows(al2, Q, sizes, T)
    assert not a[bad].any() and torch.equal(a[~bad], a2[~bad])
    dYq, dK, dV = run_backward(L, d, al, ptr, i64, Bi, Q, sizes, N, T)
    e = run_backward(L, d, al2, ptr2, i64, Bi, Q, sizes, N, T)
    for o, r in zip(unpack(dYq, Q, sizes, N), unpack(e[0], Q, sizes, N)):
        assert not o[bad].any() and torch.equal(bits(o[~bad]), bits(r[~bad]))
    for x, r in ((dK, e[1]), (dV, e[2])):
        assert not x[bad].any() and x[~bad].any() and torch.equal(bits(x[~bad]), bits(r[~bad]))


def test_bad_arguments_are_refused(L):
    N, T = 8, 4
    d = torch.zeros(16 * 9 * N, device="cuda")
    i = torch.zeros(2, dtype=torch.long, device="cuda")
    hw = torch.tensor([3, 3], dtype=torch.int32)
    ws = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    st = L.stream_ptr()
    p, ip, hp, wp = d.data_ptr(), i.data_ptr(), hw.data_ptr(), ws.data_ptr()
    lib = L.lib
    c = 1.0 / math.sqrt(N)
    fwd = lambda idx, Bi, Q, T_, N_: lib.zsg_head_words_conv0(p, idx, 1, p, p, p, p, p, p, c, Bi, Q, T_, 1, hp, N_, p, 0, p, st)
    bwd = lambda idx, Bi, Q, T_, N_, nws: lib.zsg_head_words_conv0_bwd(p, p, idx, 1, p, p, p, p, c, Bi, Q, T_, 1, hp, N_, p, p, p, wp, nws, st)
    assert fwd(ip, 1, 1, T, N) == 0 and bwd(ip, 1, 1, T, N, 1 << 19) == 0           # (the good call, so that the refusals below mean something)
    assert fwd(ip, 1, 1, T, 6) == -1 and bwd(ip, 1, 1, T, 6, 1 << 19) == -1          # N % 4
    assert fwd(ip, 1, 1, 0, N) == -1 and bwd(ip, 1, 1, 0, N, 1 << 19) == -1          # T = 0
    assert fwd(ip, 1, 1, 65, N) == -1 and bwd(ip, 1, 1, 65, N, 1 << 19) == -1        # T = 65
    assert fwd(None, 1, 2, T, N) == -1 and bwd(None, 1, 2, T, N, 1 << 19) == -1      # identity, Bi != Q
    assert fwd(ip, 0, 1, T, N) == -1
    need = int(lib.zsg_head_words_bwd_ws_bytes(1, T, 1, hp, N))
    assert need > 0 and bwd(ip, 1, 1, T, N, need - 8) == -1                          # a short workspace
    assert b"workspace" in lib.zsg_last_error()
    assert lib.zsg_head_words_bwd_ws_bytes(1, T, 1, hp, 6) == -1 and lib.zsg_head_words_bwd_ws_bytes(1, 65, 1, hp, N) == -1
    assert lib.zsg_head_words_conv0_bwd(p, p, ip, 1, p, p, p, p, c, 1, 1, T, 1, hp, N, None, None, None, wp, 1 << 19, st) == -1     # no output
    torch.cuda.synchronize()


# ---- random inputs against tests/words_ref.py ---------------------------------------------------------------------------------------
def host_eval(d, idx, Bi, sizes, N, T, dtype):
    """words_ref's attention on the operands in `dtype` (CPU): h1 [Q, P, N], alpha [Q, P, T], and by autograd dYq, dKw, dVw for the
    ReLU-masked upstream gradient dy (the pre-activation is differentiated: the kernel is handed dy already masked)"""
    Q = idx.numel()
    lens = [max(0, min(int(v), T)) for v in d["lens"].tolist()]
    Kw, Vw = d["Kw"].to(dtype).requires_grad_(True), d["Vw"].to(dtype).requires_grad_(True)
    h1s, als, dYs = [], [], []
    total = 0
    for (h, w), Y, G, dy in zip(sizes, d["Y"], d["G"], d["dy"]):
        y = Y.to(dtype)[idx].permute(0, 3, 1, 2).contiguous().requires_grad_(True)            # [Q, N, h, w]: one row set per query
        taps = F.conv2d(torch.ones(1, 1, h, w, dtype=dtype), d["V"].to(dtype).reshape(Q * N, 1, 3, 3), padding=1).view(Q, N, h, w)
        rest = taps + d["bias"].to(dtype)[None, :, None, None] + G.to(dtype).permute(2, 0, 1)[None]
        gamma, alpha = WR.attention(y, Kw, Vw, lens, 1.0 / math.sqrt(N))
        z = (1 + gamma) * y + rest
        total = total + (z * dy.to(dtype).permute(0, 3, 1, 2)).sum()
        h1s.append(F.relu(z).detach().permute(0, 2, 3, 1).reshape(Q, h * w, N))
        als.append(alpha.detach())
        dYs.append(y)
    total.backward()
    dYq = torch.cat([y.grad.permute(0, 2, 3, 1).reshape(Q, -1, N) for y in dYs], dim=1)
    return dict(h1=torch.cat(h1s, 1), alpha=torch.cat(als, 1), dYq=dYq, dKw=Kw.grad, dVw=Vw.grad)


def rows_of(flat, Q, sizes, N):
    return torch.cat([x.reshape(Q, -1, N) for x in unpack(flat, Q, sizes, N)], dim=1)


def check_random(L, sizes, geom, N, T, seed, tag):
    Q, Bi, null, idx = setup(geom, seed)
    d = operands(sizes, Q, Bi, N, T, seed + 1)
    keep, ptr = dev_idx(idx, 1, null)
    f, al = run_forward(L, d, ptr, 1, Bi, Q, sizes, N, T)
    dYq, dK, dV = run_backward(L, d, al, ptr, 1, Bi, Q, sizes, N, T)
    # two launches, the second over buffers that held something else: the same bits for every output
    f2, al2 = run_forward(L, d, ptr, 1, Bi, Q, sizes, N, T, fill=7.0)
    g2 = run_backward(L, d, al2, ptr, 1, Bi, Q, sizes, N, T, fill=7.0)
    for a, b, name in ((f, f2, "h1"), (al, al2, "alpha"), (dYq, g2[0], "dYq"), (dK, g2[1], "dKw"), (dV, g2[2], "dVw")):
        assert torch.equal(bits(a), bits(b)), name + ": two launches differ"
    got = dict(h1=rows_of(f, Q, sizes, N), alpha=alpha_rows(al, Q, sizes, T), dYq=rows_of(dYq, Q, sizes, N), dKw=dK, dVw=dV)
    truth, yard = host_eval(d, idx, Bi, sizes, N, T, torch.float64), host_eval(d, idx, Bi, sizes, N, T, torch.float32)
    fails = []
    for k in ("h1", "alpha", "dYq", "dKw", "dVw"):
        e_gpu = float((got[k].double() - truth[k]).abs().max())
        e_cpu = float((yard[k].double() - truth[k]).abs().max())
        allowed = 6 * e_cpu + 1e-4
        print(f"words parity {tag} Q={Q} Bi={Bi} N={N} T={T} P={sum(h * w for h, w in sizes)} {k}: gpu {e_gpu:.3e} cpu-fp32 {e_cpu:.3e} "
              f"allowed {allowed:.3e} scale {float(truth[k].abs().max()):.3e}")
        if not e_gpu <= allowed:
            fails.append((k, e_gpu, allowed))
    assert not fails, fails


@pytest.mark.parametrize("N", [8, 256])
@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("lv", list(LEVELS))
def test_random_inputs(L, lv, T, N):
    geom = {1: "q1b1", CHUNK - 1: "q6b3", CHUNK: "q8b4_unused2", CHUNK + 1: "q5b5_null", 64: "q6b1"}[T]
    check_random(L, LEVELS[lv], GEOM[geom], N, T, seed=sum(map(ord, lv)) + 7 * T + N, tag=lv)


def test_random_inputs_on_the_300_pyramid(L):
    check_random(L, SIZES_300, GEOM["q16b4"], 256, 13, seed=301, tag="300px")
