"""The hand-written parts of tests/pointwise_ref.py against torch CPU on small inputs (no GPU): the references the GPU edge tests trust
are themselves checked here.  It also holds the exhaustive sweep of the nearest-upsample index rule the kernels compute in fp32, and
prints the torch-CPU fp32 BatchNorm figures that stand beside the kernel's in profiles/bn_stats_conditioning.txt."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pointwise_ref as R


def test_upsample_index_rule_exhaustive():
    """every (Hs, Hd) with Hs in 1..64 and Hd in 1..129: the fp32 rule min(int(floorf(f32(dst) * (f32(Hs) / f32(Hd)))), Hs - 1) is
    F.interpolate's map, and the backward's scan range floorf(ys / sh) - 1 .. ceilf((ys + 1) / sh) + 1 (clamped) contains every
    destination pixel of every source pixel"""
    pairs = 0
    for hs in range(1, 65):
        for hd in range(1, 130):
            src = R.nearest_src_f32(hs, hd)
            assert np.array_equal(src, R.nearest_src_torch(hs, hd)), (hs, hd)
            for ys in range(hs):
                lo, hi = R.upsample_scan_range(ys, hs, hd)
                dst = np.nonzero(src == ys)[0]
                assert dst.size == 0 or (lo <= dst[0] and dst[-1] <= hi), (hs, hd, ys, lo, hi, dst)
            pairs += 1
    assert pairs == 64 * 129


@pytest.mark.parametrize("k,s,p,ceil,H,W", [(3, 2, 1, False, 5, 7), (3, 2, 1, False, 1, 1), (2, 2, 0, True, 5, 7), (3, 1, 1, False, 4, 3),
                                            (3, 3, 0, False, 7, 6), (15, 1, 7, False, 5, 9)])
@pytest.mark.parametrize("kind", ["ties", "nan", "neg_inf"])
def test_maxpool_rule_is_torch(k, s, p, ceil, H, W, kind):
    """the selection rule the forward kernel implements (first maximum wins, NaN propagates and the last NaN keeps the index, an all
    -inf window keeps its first in-bounds tap) gives torch's values and torch's arg-max, so torch's autograd places the gradient where
    the tap code says"""
    g = torch.Generator().manual_seed(H * 31 + W)
    x = torch.randint(-2, 3, (2, H, W, 4), generator=g).float()
    if kind == "nan":
        x.view(-1)[torch.randperm(x.numel(), generator=g)[:max(2, x.numel() // 6)]] = float("nan")
    if kind == "neg_inf":
        x.fill_(float("-inf"))
    out, codes, _ = R.maxpool(x, k, s, p, ceil)
    o2, c2 = R.maxpool_rule(x, k, s, p, out.shape[1], out.shape[2])
    assert torch.equal(torch.isnan(out), torch.isnan(o2)) and torch.equal(out.nan_to_num(7.0), o2.nan_to_num(7.0))
    assert torch.equal(codes, c2)


def test_maxpool_neg_inf_gradient_goes_to_first_in_bounds_element():
    x = torch.full((1, 4, 4, 4), float("-inf"))
    dout = torch.ones(1, 2, 2, 4)
    _, codes, dx = R.maxpool(x, 3, 2, 1, False, dout)
    want = torch.zeros(4, 4)
    want[0, 0] = want[0, 1] = want[1, 0] = want[1, 1] = 1
    assert torch.equal(dx[0, :, :, 0], want)
    assert codes[0, :, :, 0].tolist() == [[4, 3], [1, 0]]
    assert torch.equal(R.maxpool_bwd_ordered(dout, codes, 4, 4, 3, 2, 1), dx)


@pytest.mark.parametrize("k,s,p,H,W", [(3, 2, 1, 5, 7), (3, 1, 1, 6, 5), (15, 1, 7, 5, 9)])
def test_maxpool_bwd_ordered_is_the_gradient(k, s, p, H, W):
    """with integer dout the ordered fp32 sum is exact, so it must equal torch's gradient whatever order torch adds in"""
    g = torch.Generator().manual_seed(k + H)
    x = torch.randint(-2, 3, (2, H, W, 8), generator=g).float()
    _, codes, _ = R.maxpool(x, k, s, p)
    dout = torch.randint(-8, 9, tuple(codes.shape), generator=g).float()
    _, _, dx = R.maxpool(x, k, s, p, False, dout)
    assert torch.equal(R.maxpool_bwd_ordered(dout, codes, H, W, k, s, p), dx)


def test_index_shuffles_and_sums():
    g = torch.Generator().manual_seed(5)
    rows, groups, k, gs, off = 7, 9, 4, 5, 0
    compact = torch.randn(rows * groups * k, generator=g)
    strided = torch.full((rows * groups * gs,), float("nan"))
    s2 = R.interleave_to_strided(compact, strided, rows, groups, k, gs, off)
    for r in (0, 6):
        for a in (0, 8):
            for e in range(k):
                assert s2[(r * groups + a) * gs + off + e] == compact[(r * groups + a) * k + e]
            assert torch.isnan(s2[(r * groups + a) * gs + 4])
    assert torch.equal(R.interleave_to_compact(s2, rows, groups, k, gs, off), compact)
    src = torch.randn(5, 6, generator=g)
    pr = R.pad_rows(src.view(-1), 5, 3, 6, 4)
    assert torch.equal(pr[:, :3], src[:, :3]) and torch.equal(pr[:, 3], torch.zeros(5))
    img = torch.randn(2, 3, 4, 5, generator=g)
    n4 = R.nchw_to_nhwc4(img)
    assert n4.shape == (2, 4, 5, 4) and float(n4[1, 2, 3, 1]) == float(img[1, 1, 2, 3]) and float(n4[..., 3].abs().max()) == 0
    u8 = torch.arange(256, dtype=torch.uint8).repeat(3, 1).t().contiguous()
    assert torch.equal(R.u8hwc_to_nhwc4(u8)[:, 1], torch.arange(256).float() / 255)
    x = torch.randint(-9, 10, (3 * 40,), generator=g).float()
    assert torch.equal(R.batch_sum(x, 3, 40), x.view(3, 40).double().sum(0))
    big = torch.randint(-9, 10, (3 * (700 * 40 + 8),), generator=g).float()
    cs = R.colsum(big, 3, 700 * 40 + 8, 700, 40, 8, 16)
    for gi in range(3):
        blk = big[gi * (700 * 40 + 8):][:700 * 40].view(700, 40)
        assert torch.equal(cs[gi], blk[:, 8:24].sum(0).double())


def test_l2norm_zero_row_is_nan():
    x = torch.randn(3, 36, generator=torch.Generator().manual_seed(1))
    x[1] = 0
    out, nrm, dx = R.l2norm(x, torch.ones(3, 36))
    assert torch.isnan(out[1]).all() and torch.isnan(dx[1]).all() and float(nrm[1]) == 0
    assert not torch.isnan(out[0]).any() and not torch.isnan(dx[2]).any()


def test_bn_finalize_is_torch_batch_norm():
    """the fp64 finalize against torch's training-mode batch_norm in fp64 (statistics and running statistics, unbiased n / (n - 1))"""
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(512, 8, generator=g) * 3 + 1).float()
    rm0, rv0 = torch.randn(8, generator=g), torch.rand(8, generator=g) + 0.5
    xd = x.double()
    ref = R.bn_finalize(xd.sum(0), (xd * xd).sum(0), 512, 1e-5, rm0, rv0, 0.1)
    rm, rv = rm0.double().clone(), rv0.double().clone()
    y = F.batch_norm(xd.t().reshape(1, 8, 512), rm, rv, None, None, True, 0.1, float(np.float32(1e-5)))
    assert torch.allclose(ref["mean"].double(), xd.mean(0), rtol=1e-7, atol=1e-7)
    assert torch.allclose(y[0].t(), (xd - xd.mean(0)) * ref["invstd64"], rtol=1e-9, atol=1e-9)
    assert torch.allclose(ref["running_mean"], rm, rtol=1e-6, atol=1e-7)
    assert torch.allclose(ref["running_var"], rv, rtol=1e-6, atol=1e-7)


def test_bn_conditioning_reference_figures(capsys):
    """torch CPU fp32 F.batch_norm on the conditioning data of tests/test_gpu_bn_finalize.py against fp64 statistics of the same fp32
    data: the reference's own error per mean / std ratio, printed (profiles/bn_stats_conditioning.txt records it beside the kernel's).
    It must sit inside the bound derived for the kernel, or the bound would say nothing."""
    x, ratio, inv64 = R.conditioning_data()
    xn = x.t().reshape(1, 64, 4096).contiguous()
    # (native_batch_norm is what F.batch_norm runs; it also returns the invstd it normalised with)
    _, _, inv_t = torch.native_batch_norm(xn, None, None, None, None, True, 0.1, 1e-5)
    err = (inv_t.double() / inv64 - 1).abs()
    with capsys.disabled():
        for r in (0.0, 8.0, 64.0):
            print(f"\ntorch CPU fp32 batch_norm, mean/std = {r:g}: max |invstd / fp64 - 1| = {float(err[ratio == r].max()):.3e}", end="")
        print()
    assert bool((err <= 1.5 * 64 * 2.0 ** -24 * (1 + ratio.double() ** 2)).all())
