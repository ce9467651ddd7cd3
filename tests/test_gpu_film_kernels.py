"""csrc/film.hip through the C ABI: zsg_head_film_conv0, zsg_head_film_conv0_bwd, zsg_head_film_dgamma (include/zsg.h).

EXACT inputs: every operand a multiple of 1/8 in [-4, 4], gamma a multiple of 1/4 in [-2, 2] — every product and sum below is then exact in
fp32 (the largest intermediate, nine taps + bias + G + 3 * 4, stays under 2^6 with 5 fractional bits), so the forward and the backward
must equal the host loops that restate the formulas, and d(gamma) the float64 sum rounded to fp32, whatever the order of the adds.
RANDOM inputs pin the order instead: with gamma = 0 the forward / backward carry the bits of zsg_head_shared_conv0 / _bwd, the bf16 store
is the fp32 result's round-to-nearest-even, d(gamma) lies within 2^-23 * sum|dy * Y| of the float64 sum (a fixed-order fp64 accumulation
plus the one final rounding) and two launches give the same bits.  Every output sits between canaries."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES_300 = [(38, 38), (19, 19), (10, 10), (5, 5), (3, 3)]
LEVELS = {"1level": [(5, 5)], "3levels": [(3, 4), (2, 2), (1, 1)]}
# (Q, Bi, unused slot, identity index)
GEOM = {"q1b1": (1, 1, None, False), "q6b1": (6, 1, None, False), "q6b3": (6, 3, None, False), "q16b4": (16, 4, None, False),
        "q8b4_unused2": (8, 4, 2, False), "q5b5_null": (5, 5, None, True)}
CANARY = 1024
MARK = 12345.0


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import zsgnet_pytorch_amd._lib as L
    return L


class Guarded:
    """a device buffer of n elements between two canary runs, pre-filled with `fill`"""

    def __init__(self, n, dtype=torch.float32, fill=float("nan")):
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


def draw(g, shape, exact, step=8, lim=4):
    if exact:
        return torch.randint(-lim * step, lim * step + 1, shape, generator=g).float() / step
    return torch.randn(shape, generator=g)


def operands(sizes, Q, Bi, N, seed, exact, zero_gamma=False):
    g = torch.Generator().manual_seed(seed)
    d = dict(Y=[draw(g, (Bi, h, w, N), exact) for h, w in sizes], G=[draw(g, (h, w, N), exact) for h, w in sizes],
             dy=[draw(g, (Q, h, w, N), exact) for h, w in sizes], V=draw(g, (Q, N, 9), exact), bias=draw(g, (N,), exact),
             gamma=draw(g, (Q, N), exact, step=4, lim=2) if exact else 0.5 * torch.randn(Q, N, generator=g))
    if zero_gamma:
        d["gamma"] = torch.zeros(Q, N)
    return d


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


def host_forward(d, idx, Bi, sizes):
    """h1 = relu(((1 + gamma) * Y[idx]) + G) + (taps row-major from 0 + bias)), fp32 operation by operation; NaN rows for a bad index"""
    outs = []
    s = (np.float32(1.0) + d["gamma"].numpy()).astype(np.float32)                 # [Q, N]
    V, bias = d["V"].numpy(), d["bias"].numpy()
    for (h, w), Y, G in zip(sizes, d["Y"], d["G"]):
        Q, N = s.shape
        out = np.full((Q, h, w, N), np.nan, np.float32)
        ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
        for q in range(Q):
            i = int(idx[q])
            if not 0 <= i < Bi:
                continue
            a = np.zeros((h, w, N), np.float32)
            for r in range(3):
                for t in range(3):
                    ok = ((ys + r - 1 >= 0) & (ys + r - 1 < h) & (xs + t - 1 >= 0) & (xs + t - 1 < w))[:, :, None]
                    a = np.where(ok, a + V[q, :, r * 3 + t][None, None, :], a).astype(np.float32)
            c = (a + bias[None, None, :]).astype(np.float32)
            tt = (s[q][None, None, :] * Y[i].numpy()).astype(np.float32)
            out[q] = np.maximum(((tt + G.numpy()).astype(np.float32) + c).astype(np.float32), np.float32(0))
        outs.append(torch.from_numpy(out))
    return outs


def host_backward(d, idx, Bi, sizes):
    """dY[i] = sum over q ascending with idx[q] == i of fl((1 + gamma[q]) * dy[q]), fp32, from 0"""
    s = (np.float32(1.0) + d["gamma"].numpy()).astype(np.float32)
    outs = []
    for dy in d["dy"]:
        out = np.zeros((Bi,) + tuple(dy.shape[1:]), np.float32)
        for q in range(dy.shape[0]):
            i = int(idx[q])
            if 0 <= i < Bi:
                out[i] = (out[i] + (s[q][None, None, :] * dy[q].numpy()).astype(np.float32)).astype(np.float32)
        outs.append(torch.from_numpy(out))
    return outs


def host_dgamma(d, idx, Bi):
    """(float64 sum over all pixels of dy * Y[idx], float64 sum of |dy * Y|); zeros for a bad index"""
    Q, N = d["gamma"].shape
    s, sa = np.zeros((Q, N), np.float64), np.zeros((Q, N), np.float64)
    for dy, Y in zip(d["dy"], d["Y"]):
        for q in range(Q):
            i = int(idx[q])
            if 0 <= i < Bi:
                p = dy[q].numpy().astype(np.float64) * Y[i].numpy().astype(np.float64)
                s[q] += p.reshape(-1, N).sum(0)
                sa[q] += np.abs(p).reshape(-1, N).sum(0)
    return s, sa


def dev_idx(idx, i64, null):
    if null:
        return None, 0
    t = idx.cuda() if i64 else idx.int().cuda()
    return t, t.data_ptr()


def run_forward(L, d, idx_ptr, i64, Bi, Q, sizes, N, bf16=False, fill=float("nan"), shared=False):
    P = sum(h * w for h, w in sizes)
    hw = hw_of(sizes)
    out = Guarded(Q * P * N, torch.bfloat16 if bf16 else torch.float32, fill)
    Yd, Gd, Vd, bd, gd = pack(d["Y"]), pack(d["G"]), d["V"].reshape(-1).cuda(), d["bias"].cuda(), d["gamma"].reshape(-1).cuda()
    if shared:
        fn = L.lib.zsg_head_shared_conv0_bf16 if bf16 else L.lib.zsg_head_shared_conv0
        rc = fn(Yd.data_ptr(), idx_ptr, i64, bd.data_ptr(), Gd.data_ptr(), Vd.data_ptr(), Bi, Q, len(sizes), hw.data_ptr(), N, out.view.data_ptr(), L.stream_ptr())
    else:
        rc = L.lib.zsg_head_film_conv0(Yd.data_ptr(), idx_ptr, i64, bd.data_ptr(), Gd.data_ptr(), Vd.data_ptr(), gd.data_ptr(), Bi, Q, len(sizes),
                                       hw.data_ptr(), N, out.view.data_ptr(), int(bf16), L.stream_ptr())
    L.check(rc, "film conv0")
    torch.cuda.synchronize()
    assert out.intact(), "a canary around h1 was overwritten"
    return out.view.clone().cpu()


def run_backward(L, d, idx_ptr, i64, Bi, Q, sizes, N, fill=float("nan"), shared=False):
    P = sum(h * w for h, w in sizes)
    hw = hw_of(sizes)
    out = Guarded(Bi * P * N, fill=fill)
    dyd, gd = pack(d["dy"]), d["gamma"].reshape(-1).cuda()
    if shared:
        rc = L.lib.zsg_head_shared_conv0_bwd(dyd.data_ptr(), idx_ptr, i64, Bi, Q, len(sizes), hw.data_ptr(), N, out.view.data_ptr(), L.stream_ptr())
    else:
        rc = L.lib.zsg_head_film_conv0_bwd(dyd.data_ptr(), idx_ptr, i64, gd.data_ptr(), Bi, Q, len(sizes), hw.data_ptr(), N, out.view.data_ptr(),
                                           L.stream_ptr())
    L.check(rc, "film conv0 bwd")
    torch.cuda.synchronize()
    assert out.intact(), "a canary around dY was overwritten"
    return out.view.clone().cpu()


def run_dgamma(L, d, idx_ptr, i64, Bi, Q, sizes, N, fill=float("nan"), transposed=True):
    hw = hw_of(sizes)
    nws = int(L.lib.zsg_head_film_dgamma_ws_bytes(Q, len(sizes), hw.data_ptr(), N))
    assert nws > 0 and nws % 8 == 0
    ws = Guarded(nws // 8, torch.float64, fill)
    dg, dgt = Guarded(Q * N, fill=fill), Guarded(N * Q, fill=fill)
    dyd, Yd = pack(d["dy"]), pack(d["Y"])
    L.check(L.lib.zsg_head_film_dgamma(dyd.data_ptr(), Yd.data_ptr(), idx_ptr, i64, Bi, Q, len(sizes), hw.data_ptr(), N, dg.view.data_ptr(),
                                       dgt.view.data_ptr() if transposed else None, ws.view.data_ptr(), nws, L.stream_ptr()), "film dgamma")
    torch.cuda.synchronize()
    assert dg.intact() and dgt.intact() and ws.intact(), "a canary around d(gamma) or its workspace was overwritten"
    if not transposed:
        untouched = torch.isnan(dgt.view) if fill != fill else dgt.view == fill
        assert bool(untouched.all()), "the transposed copy was written without being asked for"
    return dg.view.clone().cpu().view(Q, N), dgt.view.clone().cpu().view(N, Q)


def check_exact(L, sizes, geom, N, seed):
    Q, Bi, unused, null = geom
    g = torch.Generator().manual_seed(seed)
    idx = torch.arange(Q) if null else make_idx(Q, Bi, g, unused)
    d = operands(sizes, Q, Bi, N, seed + 1, exact=True)
    want_f, want_b = host_forward(d, idx, Bi, sizes), host_backward(d, idx, Bi, sizes)
    s64, _ = host_dgamma(d, idx, Bi)
    want_g = torch.from_numpy(s64.astype(np.float32))
    for i64 in ((1,) if null else (1, 0)):
        keep, ptr = dev_idx(idx, i64, null)
        f = run_forward(L, d, ptr, i64, Bi, Q, sizes, N)
        for (h, w), r, o in zip(sizes, want_f, unpack(f, Q, sizes, N)):
            assert torch.equal(o, r), f"forward level {h}x{w}: max |diff| {float((o - r).abs().max()):.3e}"
        b = run_backward(L, d, ptr, i64, Bi, Q, sizes, N)
        for (h, w), r, o in zip(sizes, want_b, unpack(b, Bi, sizes, N)):
            assert torch.equal(o, r), f"backward level {h}x{w}: max |diff| {float((o - r).abs().max()):.3e}"
            if unused is not None:
                assert bool((o[unused] == 0).all()), "an image slot no query points to must get zeros"
        dg, dgt = run_dgamma(L, d, ptr, i64, Bi, Q, sizes, N)
        assert torch.equal(dg, want_g), f"d(gamma): max |diff| {float((dg - want_g).abs().max()):.3e}"
        assert torch.equal(dgt, want_g.t())


@pytest.mark.parametrize("N", [8, 256])
@pytest.mark.parametrize("lv", list(LEVELS))
@pytest.mark.parametrize("geom", list(GEOM))
def test_exact_inputs_equal_the_host_loops(L, geom, lv, N):
    check_exact(L, LEVELS[lv], GEOM[geom], N, seed=sum(map(ord, geom + lv)) + N)


def test_exact_inputs_on_the_300_pyramid(L):
    check_exact(L, SIZES_300, GEOM["q16b4"], 256, seed=300)


def check_random(L, sizes, geom, N, seed):
    Q, Bi, unused, null = geom
    g = torch.Generator().manual_seed(seed)
    idx = torch.arange(Q) if null else make_idx(Q, Bi, g, unused)
    keep, ptr = dev_idx(idx, 1, False)                       # (the shared kernels need an index: the identity is passed explicitly to them)
    keep2, ptr2 = dev_idx(idx, 1, null)
    z = operands(sizes, Q, Bi, N, seed + 1, exact=False, zero_gamma=True)
    # gamma = 0: the bits of the shared kernels
    f0 = run_forward(L, z, ptr2, 1, Bi, Q, sizes, N)
    assert torch.equal(bits(f0), bits(run_forward(L, z, ptr, 1, Bi, Q, sizes, N, shared=True))), "gamma = 0: not zsg_head_shared_conv0's bits"
    b0 = run_backward(L, z, ptr2, 1, Bi, Q, sizes, N)
    assert torch.equal(bits(b0), bits(run_backward(L, z, ptr, 1, Bi, Q, sizes, N, shared=True))), "gamma = 0: not zsg_head_shared_conv0_bwd's bits"
    h0 = run_forward(L, z, ptr2, 1, Bi, Q, sizes, N, bf16=True)
    assert torch.equal(bits(h0), bits(run_forward(L, z, ptr, 1, Bi, Q, sizes, N, bf16=True, shared=True)))
    # a drawn gamma: the bf16 store, the float64 bound, run-to-run bits (the second run over buffers that held something else)
    d = operands(sizes, Q, Bi, N, seed + 1, exact=False)
    f = run_forward(L, d, ptr2, 1, Bi, Q, sizes, N)
    assert not torch.equal(f, f0)
    assert torch.equal(bits(f), bits(run_forward(L, d, ptr2, 1, Bi, Q, sizes, N, fill=7.0)))
    h = run_forward(L, d, ptr2, 1, Bi, Q, sizes, N, bf16=True)
    assert torch.equal(bits(h), bits(f.to(torch.bfloat16))), "the bf16 store is not the fp32 result rounded to nearest-even"
    b = run_backward(L, d, ptr2, 1, Bi, Q, sizes, N)
    assert torch.equal(bits(b), bits(run_backward(L, d, ptr2, 1, Bi, Q, sizes, N, fill=7.0)))
    for r, o in zip(host_backward(d, idx, Bi, sizes), unpack(b, Bi, sizes, N)):
        assert torch.equal(o, r), "backward: not the host loop's bits (product rounded, then added, q ascending)"
    dg, dgt = run_dgamma(L, d, ptr2, 1, Bi, Q, sizes, N)
    dg2, _ = run_dgamma(L, d, ptr2, 1, Bi, Q, sizes, N, fill=7.0, transposed=False)
    assert torch.equal(bits(dg), bits(dg2)) and torch.equal(bits(dgt), bits(dg.t().contiguous()))
    s64, sa = host_dgamma(d, idx, Bi)
    err = np.abs(dg.numpy().astype(np.float64) - s64)
    bound = 2.0 ** -23 * sa
    print(f"d(gamma) Q={Q} Bi={Bi} N={N} P={sum(h * w for h, w in sizes)}: max err {err.max():.3e}, min slack {(bound - err).min():.3e}, "
          f"max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3e}")
    assert (err <= bound).all()


@pytest.mark.parametrize("N", [8, 256])
@pytest.mark.parametrize("lv", list(LEVELS))
@pytest.mark.parametrize("geom", ["q1b1", "q6b3", "q8b4_unused2", "q5b5_null"])
def test_random_inputs(L, geom, lv, N):
    check_random(L, LEVELS[lv], GEOM[geom], N, seed=sum(map(ord, geom + lv)) + N + 1)


def test_random_inputs_on_the_300_pyramid(L):
    check_random(L, SIZES_300, GEOM["q16b4"], 256, seed=301)


@pytest.mark.parametrize("i64", [1, 0], ids=["int64", "int32"])
def test_out_of_range_index(L, i64):
    """NaN rows in h1, no contribution to dY, zeros in d(gamma), canaries intact (checked by every run_*)"""
    sizes, Q, Bi, N = [(3, 4), (2, 2), (1, 1)], 5, 2, 8
    d = operands(sizes, Q, Bi, N, 77, exact=True)
    idx = torch.tensor([1, 7, -1, 0, 2], dtype=torch.long)
    keep, ptr = dev_idx(idx, i64, False)
    f = unpack(run_forward(L, d, ptr, i64, Bi, Q, sizes, N), Q, sizes, N)
    for r, o in zip(host_forward(d, idx, Bi, sizes), f):
        for q in range(Q):
            if 0 <= int(idx[q]) < Bi:
                assert torch.equal(o[q], r[q])
            else:
                assert torch.isnan(o[q]).all()
    b = unpack(run_backward(L, d, ptr, i64, Bi, Q, sizes, N), Bi, sizes, N)
    for r, o in zip(host_backward(d, idx, Bi, sizes), b):
        assert torch.equal(o, r)
    dg, dgt = run_dgamma(L, d, ptr, i64, Bi, Q, sizes, N)
    s64, _ = host_dgamma(d, idx, Bi)
    assert torch.equal(dg, torch.from_numpy(s64.astype(np.float32)))
    assert not dg[1].any() and not dg[2].any() and not dg[4].any() and dg[0].any() and dg[3].any()
    assert torch.equal(dgt, dg.t())


def test_bad_arguments_are_refused(L):
    N = 8
    d = torch.zeros(9 * N, device="cuda")
    v = torch.zeros(9 * N, device="cuda")
    i = torch.zeros(2, dtype=torch.long, device="cuda")
    hw = torch.tensor([3, 3], dtype=torch.int32)
    ws = torch.zeros(4096, dtype=torch.float64, device="cuda")
    st = L.stream_ptr()
    p = d.data_ptr()
    lib = L.lib
    assert lib.zsg_head_film_conv0(p, i.data_ptr(), 1, p, p, v.data_ptr(), p, 0, 1, 1, hw.data_ptr(), N, p, 0, st) != 0          # Bi == 0
    assert lib.zsg_head_film_conv0(p, i.data_ptr(), 1, p, p, v.data_ptr(), p, 1, 1, 1, hw.data_ptr(), 6, p, 0, st) != 0          # N % 4
    assert lib.zsg_head_film_conv0(p, i.data_ptr(), 1, p, p, v.data_ptr(), None, 1, 1, 1, hw.data_ptr(), N, p, 0, st) != 0       # no gamma
    assert lib.zsg_head_film_conv0(p, None, 1, p, p, v.data_ptr(), p, 1, 2, 1, hw.data_ptr(), N, p, 0, st) != 0                  # identity, Bi != Q
    assert lib.zsg_head_film_conv0_bwd(p, None, 1, p, 1, 2, 1, hw.data_ptr(), N, p, st) != 0
    assert lib.zsg_head_film_conv0_bwd(p, i.data_ptr(), 1, None, 1, 1, 1, hw.data_ptr(), N, p, st) != 0
    assert lib.zsg_head_film_dgamma(p, p, None, 1, 1, 2, 1, hw.data_ptr(), N, p, None, ws.data_ptr(), 32768, st) != 0
    assert lib.zsg_head_film_dgamma(p, p, i.data_ptr(), 1, 1, 1, 1, hw.data_ptr(), N, p, None, ws.data_ptr(), 8, st) != 0         # workspace too small
    assert b"workspace" in lib.zsg_last_error()
    torch.cuda.synchronize()
