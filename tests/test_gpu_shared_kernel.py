"""zsg_head_shared_conv0 through the C ABI: conv0's epilogue of the eval-only shared-image plan,
    h1[q][p][n] = relu( Y[img_idx[q]][p][n] + bias[n] + G[p][n] + sum_{tap valid at p} V[q][n*9 + tap] ),
against a torch-CPU float64 evaluation of that formula.  The kernel differs from it by the fp32 summation order of the four addends
only, so the tolerance is the one of test_gpu_ops.py::test_head_lang_map_packed (rtol 1e-5, atol 1e-5), whose kernel this one extends."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 256
SIZES_300 = [(38, 38), (19, 19), (10, 10), (5, 5), (3, 3)]


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import zsgnet_pytorch_amd._lib as L
    return L


def assert_close(got, ref, rtol, atol, what=""):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    err = (got - ref).abs()
    tol = atol + rtol * ref.abs()
    bad = ~(err <= tol)
    if bad.any():
        i = int(torch.argmax(torch.nan_to_num(err - tol, nan=float("inf")).flatten()))
        idx = np.unravel_index(i, tuple(err.shape))
        raise AssertionError(f"{what}: {int(bad.sum())}/{err.numel()} mismatches; worst at {idx}: got {got.flatten()[i]:.6g} ref {ref.flatten()[i]:.6g}")


def make_idx(Q, Bi, g):
    """non-monotone, with repeats; for Bi > 1 one image slot stays unused (returned, else None)"""
    if Bi == 1:
        return torch.zeros(Q, dtype=torch.long), None
    unused = 1 if Bi > 2 else 0
    live = [i for i in range(Bi) if i != unused]
    idx = torch.tensor([live[(3 * q + 1) % len(live)] for q in range(Q)], dtype=torch.long)
    idx = idx[torch.randperm(Q, generator=g)]
    idx[0] = live[-1]
    return idx, unused


def reference(Y, idx, bias, G, V, sizes, Q):
    """float64, level by level: list of [Q][h][w][N]"""
    out, p0 = [], 0
    for h, w in sizes:
        ref = Y[p0][idx].double() + bias.double().view(1, 1, 1, N)
        if G is not None:
            ref = ref + G[p0].double().view(1, h, w, N)
        if V is not None:
            Vc = V.double().view(Q, N, 3, 3)
            for r in range(3):
                for t in range(3):
                    ys = [y for y in range(h) if 0 <= y + r - 1 < h]
                    xs = [x for x in range(w) if 0 <= x + t - 1 < w]
                    if ys and xs:
                        ref[:, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] += Vc[:, None, None, :, r, t]
        out.append(ref.clamp_min(0))
        p0 += 1
    return out


@pytest.mark.parametrize("sizes", [[(5, 5)], [(3, 3)], SIZES_300], ids=["5x5", "3x3", "300sq"])
@pytest.mark.parametrize("Q,Bi", [(1, 1), (5, 1), (5, 3), (5, 5), (16, 1), (16, 3), (16, 16)])
def test_head_shared_conv0(L, sizes, Q, Bi):
    g = torch.Generator().manual_seed(100 * Q + Bi + len(sizes))
    idx, unused = make_idx(Q, Bi, g)
    Ys = [torch.randn(Bi, h, w, N, generator=g) for h, w in sizes]
    if unused is not None:
        assert unused not in idx.tolist()
        for y in Ys:
            y[unused] = float("nan")            # a slot no query points to must never reach an output row
    Gs = [torch.randn(h, w, N, generator=g) for h, w in sizes]
    bias, V = torch.randn(N, generator=g), torch.randn(Q, N * 9, generator=g)
    Yd = torch.cat([y.reshape(-1) for y in Ys]).cuda()
    Gd = torch.cat([x.reshape(-1) for x in Gs]).cuda()
    bd, Vd = bias.cuda(), V.cuda()
    hw = torch.tensor([v for s_ in sizes for v in s_], dtype=torch.int32)
    P = sum(h * w for h, w in sizes)
    st = L.stream_ptr()
    for i64 in (1, 0):
        idd = idx.cuda() if i64 else idx.int().cuda()
        for useG, useV in ((True, True), (False, True), (True, False), (False, False)):
            outs = []
            for _ in range(2):
                out = torch.full((Q * P * N,), float("nan"), device="cuda")
                L.check(L.lib.zsg_head_shared_conv0(Yd.data_ptr(), idd.data_ptr(), i64, bd.data_ptr(), Gd.data_ptr() if useG else None,
                                                    Vd.data_ptr() if useV else None, Bi, Q, len(sizes), hw.data_ptr(), N, out.data_ptr(), st), "shared conv0")
                outs.append(out)
            torch.cuda.synchronize()
            assert torch.equal(outs[0], outs[1]), "two launches must give identical bits"
            assert torch.isfinite(outs[0]).all(), "an unused image slot (NaN) or an unwritten output element was read"
            ref = reference(Ys, idx, bias, Gs if useG else None, V if useV else None, sizes, Q)
            p0 = 0
            for (h, w), r in zip(sizes, ref):
                got = outs[0][Q * p0 * N:Q * (p0 + h * w) * N].view(Q, h, w, N)
                assert_close(got, r, 1e-5, 1e-5, f"level {h}x{w} Q={Q} Bi={Bi} G={useG} V={useV} int64={i64}")
                p0 += h * w


def test_head_shared_conv0_index_out_of_range_is_nan_not_a_read(L):
    """an index outside [0, Bi) gives that query NaN rows (and the others their values): the kernel never reads outside Y"""
    sizes, Q, Bi = [(3, 3)], 3, 2
    g = torch.Generator().manual_seed(9)
    Y, bias = torch.randn(Bi, 3, 3, N, generator=g), torch.randn(N, generator=g)
    idx = torch.tensor([1, 7, -1], dtype=torch.long)
    hw = torch.tensor([3, 3], dtype=torch.int32)
    out = torch.zeros(Q * 9 * N, device="cuda")
    Yd, bd, idd = Y.cuda(), bias.cuda(), idx.cuda()
    L.check(L.lib.zsg_head_shared_conv0(Yd.data_ptr(), idd.data_ptr(), 1, bd.data_ptr(), None, None, Bi, Q, 1, hw.data_ptr(), N, out.data_ptr(), L.stream_ptr()), "oob")
    torch.cuda.synchronize()
    o = out.view(Q, 3, 3, N).cpu()
    assert torch.isnan(o[1]).all() and torch.isnan(o[2]).all()
    assert_close(o[0], (Y[1] + bias).clamp_min(0), 1e-5, 1e-5, "live query")
