"""The element-wise kernels of csrc/misc.hip at their edges, through the C ABI, against tests/pointwise_ref.py.

Principle: wherever the operation is a permutation, a select or a sum, the inputs are integer-valued fp32 small enough that every partial
sum stays below 2^24, and the comparison is torch.equal: summation order cannot excuse a miss, and a dropped or double-counted element
always shows.  Every output is filled with NaN (uint8: 255) before the call and allocated CANARY elements longer than needed; the tail
must come back untouched.  The grid-stride tests give each kernel one work item, a count that is no multiple of the 256-thread block, and
just over 4096 blocks x 256 threads = 1 048 576 work items, the first size at which `i += gridDim.x * blockDim.x` runs.

Kernel, path, test (every comparison exact unless a tolerance is named):
  maxpool_fwd / maxpool_bwd    grid stride                              test_grid_maxpool[stride]
                               ties, idx == NULL, k = 15, ceil mode     test_maxpool_ties (random dout: bit-equal to the stated order)
                               NaN rule, all -inf windows               test_maxpool_nan, test_maxpool_all_neg_inf
  upsample_add_fwd / _bwd      grid stride (fwd / bwd)                  test_grid_upsample_add[stride_fwd / stride_bwd]
                               ratios 1..7.6 and < 1, accumulate 0 / 1  test_upsample_add_pairs
  relu_fwd / relu_bwd          grid stride, accumulate 0 / 1            test_grid_relu[stride], test_relu_special_values
  avgpool_fwd / avgpool_bwd    accumulate 0 / 1, C = 100, HW = 1 / 25   test_avgpool_exact (HW = 9 random: 1e-6, test_avgpool_random_hw9)
  l2norm_fwd / l2norm_bwd      lane-loop tail, C < 64, zero row         test_l2norm_shapes (1e-5 / 1e-4; NaN pattern exact)
  colsum4 / colsum kernels     both kernels, deterministic form of      test_colsum
                               each, groups, accumulate, unaligned x
  interleave                   grid stride, both directions, refusal    test_grid_interleave[stride], test_interleave
  pad_rows                     grid stride, src_ld > C, dst_ld >= C     test_grid_pad_rows[stride], test_pad_rows
  nchw_to_nhwc4                grid stride, C = 1..4                    test_grid_nchw_to_nhwc4[stride], test_nchw_to_nhwc4_channels
  u8hwc_to_nhwc4               grid stride, every byte value            test_grid_u8hwc_to_nhwc4[stride], test_u8hwc_to_nhwc4_every_byte
  batch_sum                    grid stride, B = 1 / 2 / 16              test_grid_batch_sum[stride], test_batch_sum
  fill (memset_f32)            grid stride, unaligned head and tail     test_grid_memset_f32[stride]
  every entry's ZSG_REQUIRE                                             test_refusals"""
import numpy as np
import pytest
import torch

import pointwise_ref as R

pytestmark = pytest.mark.gpu

CANARY = 8
NAN = float("nan")
GRID_ITEMS = 4096 * 256          # grid_for(): at most ZSG_NUM_CU * 16 blocks of 256 threads


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import zsgnet_pytorch_amd._lib as lib
    return lib


def ints(g, shape, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def fresh(n, dtype=torch.float32):
    """an output buffer of n elements plus the canary tail, every element NaN (uint8: 255)"""
    return torch.full((n + CANARY,), 255 if dtype == torch.uint8 else NAN, dtype=dtype, device="cuda")


def preload(t):
    """an accumulate target: the integers of t on the GPU, plus the NaN tail"""
    buf = fresh(t.numel())
    buf[:t.numel()] = t.reshape(-1).cuda()
    return buf


def taken(buf, n, shape=None):
    """the first n elements on the CPU, after checking the canary tail"""
    torch.cuda.synchronize()
    tail = buf[n:].cpu()
    assert bool((tail == 255).all() if buf.dtype == torch.uint8 else torch.isnan(tail).all()), "the kernel wrote past its output"
    out = buf[:n].cpu()
    return out.view(shape) if shape is not None else out


def same(got, ref, what=""):
    """exact equality, NaN equal to NaN"""
    ref = ref.to(got.dtype)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ng, nr = torch.isnan(got), torch.isnan(ref)
    if not (torch.equal(ng, nr) and torch.equal(got.nan_to_num(0.0, 1e30, -1e30), ref.nan_to_num(0.0, 1e30, -1e30))):
        bad = (ng != nr) | (got.nan_to_num(0.0, 1e30, -1e30) != ref.nan_to_num(0.0, 1e30, -1e30))
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements differ; first at flat index {i}: got {got.reshape(-1)[i]} "
                             f"ref {ref.reshape(-1)[i]}")


def bits(t):
    return t.contiguous().view(torch.int32)


def close(got, ref, rtol, atol, what=""):
    got, ref = got.double(), ref.double()
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"{what}: NaN pattern differs"
    ok = ~torch.isnan(ref)
    err = (got[ok] - ref[ok]).abs()
    tol = atol + rtol * ref[ok].abs()
    assert bool((err <= tol).all()), f"{what}: max abs err {float(err.max()):.3g} (worst excess {float((err - tol).max()):.3g})"


def refused(L, rc, what):
    assert rc == -1, f"{what}: returned {rc}, expected the refusal -1"
    err = L.lib.zsg_last_error()
    assert len(err) > 0 and what.split()[0].rstrip(":").encode() in err, (what, err)       # non-empty, and this entry's own message


# ---- runners ------------------------------------------------------------------------------------------------------------------------------
def run_maxpool_fwd(L, x, k, s, p, Ho, Wo, with_idx=True):
    B, H, W, C = x.shape
    n = B * Ho * Wo * C
    xd = x.cuda()
    out, idx = fresh(n), (fresh(n, torch.uint8) if with_idx else None)
    L.check(L.lib.zsg_maxpool_fwd(xd.data_ptr(), B, H, W, C, k, s, p, Ho, Wo, out.data_ptr(), idx.data_ptr() if with_idx else None,
                                  L.stream_ptr()), "maxpool_fwd")
    return taken(out, n, (B, Ho, Wo, C)), (taken(idx, n, (B, Ho, Wo, C)) if with_idx else None)


def run_maxpool_bwd(L, dout, codes, H, W, k, s, p):
    B, Ho, Wo, C = dout.shape
    n = B * H * W * C
    dd, cd = dout.cuda(), codes.cuda()
    dx = fresh(n)
    L.check(L.lib.zsg_maxpool_bwd(dd.data_ptr(), cd.data_ptr(), B, H, W, C, k, s, p, Ho, Wo, dx.data_ptr(), L.stream_ptr()), "maxpool_bwd")
    return taken(dx, n, (B, H, W, C))


def run_upsample_fwd(L, a, p):
    B, Hd, Wd, C = a.shape
    ad, pd = a.cuda(), p.cuda()
    out = fresh(a.numel())
    L.check(L.lib.zsg_upsample_add_fwd(ad.data_ptr(), pd.data_ptr(), B, p.shape[1], p.shape[2], Hd, Wd, C, out.data_ptr(), L.stream_ptr()),
            "upsample_add_fwd")
    return taken(out, a.numel(), tuple(a.shape))


def run_upsample_bwd(L, dout, Hs, Ws, pre=None):
    B, Hd, Wd, C = dout.shape
    n = B * Hs * Ws * C
    dd = dout.cuda()
    dp = fresh(n) if pre is None else preload(pre)
    L.check(L.lib.zsg_upsample_add_bwd(dd.data_ptr(), B, Hs, Ws, Hd, Wd, C, dp.data_ptr(), 0 if pre is None else 1, L.stream_ptr()),
            "upsample_add_bwd")
    return taken(dp, n, (B, Hs, Ws, C))


# ---- grid-stride loops: one work item / no multiple of 256 / just over 4096 x 256 ----------------------------------------------------------
@pytest.mark.parametrize("B,C,H,W", [(1, 4, 1, 1), (1, 12, 21, 21), (2, 256, 192, 192)], ids=["one", "odd", "stride"])
def test_grid_maxpool(L, B, C, H, W):
    """maxpool_fwd_kernel over B*Ho*Wo*C/4 items and maxpool_bwd_kernel over B*H*W*C/4: values, tap codes and gradient exact"""
    k, s, p = 3, 2, 1
    g = torch.Generator().manual_seed(H)
    x = ints(g, (B, H, W, C), -3, 3)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    if B == 2:
        assert B * Ho * Wo * C // 4 > GRID_ITEMS
    dout = ints(g, (B, Ho, Wo, C))
    ref_out, ref_codes, ref_dx = R.maxpool(x, k, s, p, False, dout)
    out, codes = run_maxpool_fwd(L, x, k, s, p, Ho, Wo)
    same(out, ref_out, "maxpool values")
    assert torch.equal(codes, ref_codes)
    same(run_maxpool_bwd(L, dout, codes, H, W, k, s, p), ref_dx, "maxpool gradient")


@pytest.mark.parametrize("B,C,Hs,Ws,Hd,Wd", [(1, 4, 1, 1, 1, 1), (1, 12, 10, 11, 19, 23), (2, 256, 48, 50, 95, 99), (2, 256, 95, 99, 48, 50)],
                         ids=["one", "odd", "stride_fwd", "stride_bwd"])
def test_grid_upsample_add(L, B, C, Hs, Ws, Hd, Wd):
    """upsample_add_fwd_kernel runs over the DESTINATION pixels and upsample_add_bwd_kernel over the SOURCE pixels, so 48x50 -> 95x99
    strides the forward only (1 203 840 against 307 200 items); the reversed pair strides the backward"""
    g = torch.Generator().manual_seed(Hs + Wd)
    a, p, dout = ints(g, (B, Hd, Wd, C)), ints(g, (B, Hs, Ws, C)), ints(g, (B, Hd, Wd, C))
    if Hd == 95:
        assert a.numel() // 4 > GRID_ITEMS
    if Hs == 95:
        assert p.numel() // 4 > GRID_ITEMS
    ref_out, ref_dp = R.upsample_add(a, p, dout)
    same(run_upsample_fwd(L, a, p), ref_out, "upsample_add")
    same(run_upsample_bwd(L, dout, Hs, Ws), ref_dp, "upsample_add gradient")


@pytest.mark.parametrize("n", [4, 4 * 333, 4 * (GRID_ITEMS + 257)], ids=["one", "odd", "stride"])
def test_grid_relu(L, n):
    g = torch.Generator().manual_seed(n % 1000)
    x, dout, pre = ints(g, (n,)), ints(g, (n,)), ints(g, (n,))
    xd, dd = x.cuda(), dout.cuda()
    out = fresh(n)
    L.check(L.lib.zsg_relu_fwd(xd.data_ptr(), n, out.data_ptr(), L.stream_ptr()), "relu_fwd")
    same(taken(out, n), torch.relu(x), "relu")
    for acc in (0, 1):
        dx = preload(pre) if acc else fresh(n)
        L.check(L.lib.zsg_relu_bwd(dd.data_ptr(), xd.data_ptr(), n, dx.data_ptr(), acc, L.stream_ptr()), "relu_bwd")
        same(taken(dx, n), dout * (x > 0) + (pre if acc else 0), f"relu gradient, accumulate={acc}")


@pytest.mark.parametrize("rows,groups,k,gs,off", [(1, 1, 1, 5, 4), (37, 9, 1, 5, 4), (16 * 1940, 9, 4, 5, 0)], ids=["one", "odd", "stride"])
def test_grid_interleave(L, rows, groups, k, gs, off):
    n, ns = rows * groups * k, rows * groups * gs
    if rows > 37:
        assert n > GRID_ITEMS
    g = torch.Generator().manual_seed(rows)
    compact = ints(g, (n,), -1000, 1000)
    cd = compact.cuda()
    strided = fresh(ns)
    L.check(L.lib.zsg_interleave(cd.data_ptr(), rows, groups, k, strided.data_ptr(), gs, off, 0, L.stream_ptr()), "interleave 0")
    same(taken(strided, ns), R.interleave_to_strided(compact, torch.full((ns,), NAN), rows, groups, k, gs, off), "compact -> strided")
    src = ints(g, (ns,), -1000, 1000)
    sd = src.cuda()
    back = fresh(n)
    L.check(L.lib.zsg_interleave(back.data_ptr(), rows, groups, k, sd.data_ptr(), gs, off, 1, L.stream_ptr()), "interleave 1")
    same(taken(back, n), R.interleave_to_compact(src, rows, groups, k, gs, off), "strided -> compact")
    assert torch.equal(sd.cpu(), src), "direction 1 must not write the strided tensor"


@pytest.mark.parametrize("rows,C,src_ld,dst_ld", [(1, 1, 1, 1), (7, 45, 45, 48), (25000, 45, 45, 48)], ids=["one", "odd", "stride"])
def test_grid_pad_rows(L, rows, C, src_ld, dst_ld):
    if rows == 25000:
        assert rows * dst_ld > GRID_ITEMS
    src = ints(torch.Generator().manual_seed(rows), (rows * src_ld,), -1000, 1000)
    sd = src.cuda()
    dst = fresh(rows * dst_ld)
    L.check(L.lib.zsg_pad_rows(sd.data_ptr(), rows, C, src_ld, dst.data_ptr(), dst_ld, L.stream_ptr()), "pad_rows")
    got = taken(dst, rows * dst_ld, (rows, dst_ld))
    assert torch.equal(bits(got), bits(R.pad_rows(src, rows, C, src_ld, dst_ld)))


@pytest.mark.parametrize("pixels", [1, 333, 1100003], ids=["one", "odd", "stride"])
def test_grid_u8hwc_to_nhwc4(L, pixels):
    img = torch.randint(0, 256, (pixels, 3), generator=torch.Generator().manual_seed(pixels % 97), dtype=torch.uint8)
    imd = img.cuda()
    out = fresh(pixels * 4)
    L.check(L.lib.zsg_u8hwc_to_nhwc4(imd.data_ptr(), pixels, out.data_ptr(), L.stream_ptr()), "u8hwc_to_nhwc4")
    assert torch.equal(bits(taken(out, pixels * 4, (pixels, 4))), bits(R.u8hwc_to_nhwc4(img)))


@pytest.mark.parametrize("B,C,H,W", [(1, 1, 1, 1), (1, 3, 17, 19), (2, 3, 800, 700)], ids=["one", "odd", "stride"])
def test_grid_nchw_to_nhwc4(L, B, C, H, W):
    if B == 2:
        assert B * H * W > GRID_ITEMS
    img = ints(torch.Generator().manual_seed(H), (B, C, H, W), -1000, 1000)
    imd = img.cuda()
    out = fresh(B * H * W * 4)
    L.check(L.lib.zsg_nchw_to_nhwc4(imd.data_ptr(), B, C, H, W, out.data_ptr(), L.stream_ptr()), "nchw_to_nhwc4")
    assert torch.equal(bits(taken(out, B * H * W * 4, (B, H, W, 4))), bits(R.nchw_to_nhwc4(img)))


@pytest.mark.parametrize("B,stride", [(3, 4), (3, 4 * 333), (3, 4 * (GRID_ITEMS + 5))], ids=["one", "odd", "stride"])
def test_grid_batch_sum(L, B, stride):
    x = ints(torch.Generator().manual_seed(stride % 1000), (B * stride,), -1000, 1000)
    xd = x.cuda()
    out = fresh(stride)
    L.check(L.lib.zsg_batch_sum(xd.data_ptr(), B, stride, out.data_ptr(), L.stream_ptr()), "batch_sum")
    same(taken(out, stride).double(), R.batch_sum(x, B, stride), "batch_sum")


@pytest.mark.parametrize("n,lead", [(1, 1), (1, 0), (4 * 333 + 3, 2), (4 * GRID_ITEMS + 7, 1)], ids=["one", "one_aligned", "odd", "stride"])
def test_grid_memset_f32(L, n, lead):
    """fill_kernel: scalar head up to the 16-byte boundary, 16-byte body (the grid-stride loop), scalar tail; `lead` floats before the
    pointer and the canary after it stay NaN.  n = 4 * 1 048 576 + 7 from 4 bytes past alignment: head 3, body 1 048 577 x 16 bytes"""
    buf = fresh(lead + n)
    assert buf.data_ptr() % 16 == 0
    L.check(L.lib.zsg_memset_f32(buf.data_ptr() + 4 * lead, n, 3.5, L.stream_ptr()), "memset_f32")
    got = taken(buf, lead + n)
    assert bool(torch.isnan(got[:lead]).all()), "the fill wrote before its pointer"
    assert bool((got[lead:] == 3.5).all()), f"{int((got[lead:] != 3.5).sum())} of {n} elements not filled"


# ---- max pool --------------------------------------------------------------------------------------------------------------------------------
POOL_GEOMS = [  # k, s, p, ceil, H, W
    (3, 2, 1, False, 5, 7),
    (3, 2, 1, False, 1, 1),
    (2, 2, 0, True, 7, 9),          # odd sizes: the last window of each axis hangs over the edge
    (3, 1, 1, False, 6, 5),
    (3, 3, 0, False, 9, 7),         # disjoint windows (the last input column belongs to no window)
    (15, 1, 7, False, 9, 16),       # the largest window whose tap code r * k + q fits a byte (224)
]
POOL_IDS = [f"k{k}s{s}p{p}{'c' if c else ''}_{H}x{W}" for k, s, p, c, H, W in POOL_GEOMS]


def pool_out_size(n, k, s, p, ceil):
    o = (n + 2 * p - k + (s - 1 if ceil else 0)) // s + 1
    if ceil and (o - 1) * s >= n + p:
        o -= 1
    return o


@pytest.mark.parametrize("C", [4, 12, 64])
@pytest.mark.parametrize("geom", POOL_GEOMS, ids=POOL_IDS)
def test_maxpool_ties(L, geom, C):
    """integer maps with many ties: values, tap codes (first maximum wins) and the integer gradient equal torch's; the values do not
    depend on whether the codes are asked for; a random gradient is bit-equal to the fp32 sum in the order the backward's comment states"""
    k, s, p, ceil, H, W = geom
    B = 2
    g = torch.Generator().manual_seed(k * 100 + H * 10 + C)
    x = ints(g, (B, H, W, C), -2, 2)
    Ho, Wo = pool_out_size(H, k, s, p, ceil), pool_out_size(W, k, s, p, ceil)
    dout = ints(g, (B, Ho, Wo, C), -8, 8)
    ref_out, ref_codes, ref_dx = R.maxpool(x, k, s, p, ceil, dout)
    assert tuple(ref_out.shape) == (B, Ho, Wo, C)
    out, codes = run_maxpool_fwd(L, x, k, s, p, Ho, Wo, True)
    out_noidx, _ = run_maxpool_fwd(L, x, k, s, p, Ho, Wo, False)
    same(out, ref_out, "values")
    same(out_noidx, ref_out, "values without idx")
    assert torch.equal(codes, ref_codes)
    same(run_maxpool_bwd(L, dout, ref_codes, H, W, k, s, p), ref_dx, "integer gradient")
    dr = torch.randn(B, Ho, Wo, C, generator=g)
    got = run_maxpool_bwd(L, dr, ref_codes, H, W, k, s, p)
    assert torch.equal(bits(got), bits(R.maxpool_bwd_ordered(dr, ref_codes, H, W, k, s, p))), "not the stated summation order"


@pytest.mark.parametrize("C", [4, 12])
@pytest.mark.parametrize("geom", POOL_GEOMS, ids=POOL_IDS)
def test_maxpool_nan(L, geom, C):
    """NaN propagates to every window that contains one; the tap code and the gradient go where torch puts them (the LAST NaN of the window)"""
    k, s, p, ceil, H, W = geom
    B = 2
    g = torch.Generator().manual_seed(k + H + C)
    x = ints(g, (B, H, W, C), -2, 2)
    x[0, 0, 0, :] = NAN                                   # a corner: inside the padding-clipped windows
    x[1, H - 1, W - 1, 0] = NAN
    x[1, H // 2, W // 2, 1:3] = NAN                       # two NaN in one window where the window is wider than one pixel
    x[1, H // 2, max(W // 2 - 1, 0), 1] = NAN
    Ho, Wo = pool_out_size(H, k, s, p, ceil), pool_out_size(W, k, s, p, ceil)
    dout = ints(g, (B, Ho, Wo, C), 1, 8)
    ref_out, ref_codes, ref_dx = R.maxpool(x, k, s, p, ceil, dout)
    assert bool(torch.isnan(ref_out).any())
    out, codes = run_maxpool_fwd(L, x, k, s, p, Ho, Wo, True)
    out_noidx, _ = run_maxpool_fwd(L, x, k, s, p, Ho, Wo, False)
    same(out, ref_out, "values")
    same(out_noidx, ref_out, "values without idx")
    assert torch.equal(codes, ref_codes)
    same(run_maxpool_bwd(L, dout, codes, H, W, k, s, p), ref_dx, "gradient placement")


@pytest.mark.parametrize("geom", POOL_GEOMS, ids=POOL_IDS)
def test_maxpool_all_neg_inf(L, geom):
    """a map of -inf: no tap beats the initial maximum, so the code must be the window's first IN-BOUNDS tap (torch's rule) and the
    gradient must reach that element; with code 0 — a tap in the padding wherever p > 0 — the backward would give it to no pixel"""
    k, s, p, ceil, H, W = geom
    B, C = 2, 4
    x = torch.full((B, H, W, C), float("-inf"))
    Ho, Wo = pool_out_size(H, k, s, p, ceil), pool_out_size(W, k, s, p, ceil)
    dout = ints(torch.Generator().manual_seed(k), (B, Ho, Wo, C), 1, 8)
    ref_out, ref_codes, ref_dx = R.maxpool(x, k, s, p, ceil, dout)
    out, codes = run_maxpool_fwd(L, x, k, s, p, Ho, Wo, True)
    out_noidx, _ = run_maxpool_fwd(L, x, k, s, p, Ho, Wo, False)
    same(out, ref_out, "values")
    same(out_noidx, ref_out, "values without idx")
    assert torch.equal(codes, ref_codes)
    dx = run_maxpool_bwd(L, dout, codes, H, W, k, s, p)
    same(dx, ref_dx, "gradient placement")
    assert float(dx.double().sum()) == float(dout.double().sum()), "gradient lost in the padding"


# ---- nearest upsample + add ------------------------------------------------------------------------------------------------------------------
UPS_PAIRS = [(1, 1, 7, 5), (3, 3, 3, 3), (3, 5, 7, 11), (5, 5, 38, 38), (38, 38, 75, 75), (7, 9, 3, 4),
             (3, 3, 5, 5), (5, 5, 10, 10), (10, 10, 19, 19), (19, 19, 38, 38)]           # the last four: the pyramid's own chain


@pytest.mark.parametrize("C", [4, 256])
@pytest.mark.parametrize("Hs,Ws,Hd,Wd", UPS_PAIRS, ids=[f"{a}x{b}_to_{c}x{d}" for a, b, c, d in UPS_PAIRS])
def test_upsample_add_pairs(L, Hs, Ws, Hd, Wd, C):
    B = 2
    g = torch.Generator().manual_seed(Hs * 1000 + Hd + C)
    a, p, dout, pre = ints(g, (B, Hd, Wd, C)), ints(g, (B, Hs, Ws, C)), ints(g, (B, Hd, Wd, C)), ints(g, (B, Hs, Ws, C))
    ref_out, ref_dp = R.upsample_add(a, p, dout)
    same(run_upsample_fwd(L, a, p), ref_out, "upsample_add")
    dp0 = run_upsample_bwd(L, dout, Hs, Ws)
    same(dp0, ref_dp, "gradient, accumulate=0")
    dp1 = run_upsample_bwd(L, dout, Hs, Ws, pre)
    same(dp1, ref_dp + pre, "gradient, accumulate=1")
    # every destination pixel has exactly one source (a down-sample leaves some sources without any: their gradient is 0)
    assert float(dp0.double().sum()) == float(dout.double().sum())
    assert float((dp1 - pre).double().sum()) == float(dout.double().sum())


# ---- ReLU, average pool --------------------------------------------------------------------------------------------------------------------
def test_relu_special_values(L):
    """+0, -0, denormals, infinities and NaN: out = max(x, 0) with a NaN giving 0, dx = dout where x > 0 (a NaN: 0), both accumulate modes"""
    tiny = float(np.float32(1e-45))
    x = torch.tensor([0.0, -0.0, tiny, -tiny, 1e-39, -1e-39, float("inf"), float("-inf"), NAN, -NAN, 1.0, -1.0, 3.0, -3.0, 2.0 ** -126, 7.0])
    n = x.numel()
    dout = torch.arange(1, n + 1).float()
    pre = torch.arange(n).float() * 16
    want = torch.where(x > 0, x, torch.zeros(()))
    xd, dd = x.cuda(), dout.cuda()
    out = fresh(n)
    L.check(L.lib.zsg_relu_fwd(xd.data_ptr(), n, out.data_ptr(), L.stream_ptr()), "relu_fwd")
    same(taken(out, n), want, "relu")
    for acc in (0, 1):
        dx = preload(pre) if acc else fresh(n)
        L.check(L.lib.zsg_relu_bwd(dd.data_ptr(), xd.data_ptr(), n, dx.data_ptr(), acc, L.stream_ptr()), "relu_bwd")
        same(taken(dx, n), torch.where(x > 0, dout, torch.zeros(())) + (pre if acc else 0), f"relu gradient, accumulate={acc}")


@pytest.mark.parametrize("C", [4, 256, 100])
@pytest.mark.parametrize("HW", [1, 9, 25])
def test_avgpool_exact(L, HW, C):
    """integer data divisible by HW: the sum, its quotient and the spread gradient are exact, accumulate 0 and 1"""
    B = 3
    g = torch.Generator().manual_seed(HW * 7 + C)
    x = ints(g, (B, HW, C), -50, 50) * HW
    dout = ints(g, (B, C), -50, 50) * HW
    pre = ints(g, (B, HW, C), -50, 50)
    xd, dd = x.cuda(), dout.cuda()
    out = fresh(B * C)
    L.check(L.lib.zsg_avgpool_fwd(xd.data_ptr(), B, HW, C, out.data_ptr(), L.stream_ptr()), "avgpool_fwd")
    same(taken(out, B * C, (B, C)).double(), x.double().sum(1) / HW, "avgpool")
    for acc in (0, 1):
        dx = preload(pre) if acc else fresh(B * HW * C)
        L.check(L.lib.zsg_avgpool_bwd(dd.data_ptr(), B, HW, C, dx.data_ptr(), acc, L.stream_ptr()), "avgpool_bwd")
        want = (dout.double() / HW)[:, None, :].expand(B, HW, C) + (pre.double() if acc else 0)
        same(taken(dx, B * HW * C, (B, HW, C)).double(), want, f"avgpool gradient, accumulate={acc}")


@pytest.mark.parametrize("C", [4, 256, 100])
def test_avgpool_random_hw9(L, C):
    B, HW = 3, 9
    g = torch.Generator().manual_seed(C)
    x, dout, pre = torch.randn(B, HW, C, generator=g), torch.randn(B, C, generator=g), torch.randn(B, HW, C, generator=g)
    xd, dd = x.cuda(), dout.cuda()
    out = fresh(B * C)
    L.check(L.lib.zsg_avgpool_fwd(xd.data_ptr(), B, HW, C, out.data_ptr(), L.stream_ptr()), "avgpool_fwd")
    close(taken(out, B * C, (B, C)), x.double().mean(1), 1e-6, 1e-6, "avgpool")
    for acc in (0, 1):
        dx = preload(pre) if acc else fresh(B * HW * C)
        L.check(L.lib.zsg_avgpool_bwd(dd.data_ptr(), B, HW, C, dx.data_ptr(), acc, L.stream_ptr()), "avgpool_bwd")
        want = (dout.double() / 9)[:, None, :].expand(B, HW, C) + (pre.double() if acc else 0)
        close(taken(dx, B * HW * C, (B, HW, C)), want, 1e-6, 1e-7, f"avgpool gradient, accumulate={acc}")


# ---- channel L2 norm -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3, 50])
@pytest.mark.parametrize("C", [4, 36, 64, 100, 512])
def test_l2norm_shapes(L, C, rows):
    """the lane loop's tail (C no multiple of 64), C below one wave, rows that do not fill a block, and one zero row: NaN exactly where
    torch's x / x.norm() has NaN, in out and in dx"""
    g = torch.Generator().manual_seed(C * 100 + rows)
    x, dout = torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g)
    if rows >= 3:
        x[1] = 0
    ref_out, ref_norm, ref_dx = R.l2norm(x, dout)
    xd, dd = x.cuda(), dout.cuda()
    out, nrm, dx = fresh(rows * C), fresh(rows), fresh(rows * C)
    L.check(L.lib.zsg_l2norm_fwd(xd.data_ptr(), rows, C, out.data_ptr(), nrm.data_ptr(), L.stream_ptr()), "l2norm_fwd")
    got_out, got_norm = taken(out, rows * C, (rows, C)), taken(nrm, rows)
    close(got_out, ref_out, 1e-5, 1e-6, "l2norm")
    close(got_norm, x.double().pow(2).sum(1).sqrt(), 1e-5, 1e-6, "norm = sqrt(sum x^2)")
    close(got_norm, ref_norm, 1e-5, 1e-6, "norm")
    L.check(L.lib.zsg_l2norm_bwd(dd.data_ptr(), out.data_ptr(), nrm.data_ptr(), rows, C, dx.data_ptr(), L.stream_ptr()), "l2norm_bwd")
    close(taken(dx, rows * C, (rows, C)), ref_dx, 1e-4, 1e-5, "l2norm gradient")
    if rows >= 3:
        assert float(got_norm[1]) == 0 and bool(torch.isnan(got_out[1]).all())


# ---- column sums -----------------------------------------------------------------------------------------------------------------------------
COLSUM_SHAPES = [  # rows, ld, c0, C, floats the x pointer is moved off 16-byte alignment
    (700, 40, 8, 16, 0),
    (31040, 48, 0, 45, 0),          # the head's bias gradient: scalar kernel
    (3, 256, 0, 256, 0),            # fewer rows than row lanes
    (1, 8, 4, 4, 0),
    (5000, 12, 2, 8, 0),            # c0 % 4 != 0: scalar kernel
    (700, 40, 8, 16, 1),            # an aligned shape from a pointer 4 bytes off: scalar kernel
]


def run_colsum(L, xd, lead, groups, gstride, rows, ld, c0, C, pre):
    n = groups * C
    out = fresh(n) if pre is None else preload(pre)
    L.check(L.lib.zsg_colsum(xd.data_ptr() + 4 * lead, groups, gstride, rows, ld, c0, C, out.data_ptr(), 0 if pre is None else 1,
                             L.stream_ptr()), "colsum")
    return taken(out, n, (groups, C))


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("shape", COLSUM_SHAPES, ids=[f"r{r}_ld{ld}_c{c0}_C{C}{'_off4' if o else ''}" for r, ld, c0, C, o in COLSUM_SHAPES])
def test_colsum(L, shape, groups):
    """the 16-byte kernel, the scalar kernel and the single-block deterministic form of each, accumulate 0 and 1, exact on integers;
    in deterministic mode random data sums to the same bits twice and matches fp64"""
    rows, ld, c0, C, lead = shape
    gstride = rows * ld + 8
    g = torch.Generator().manual_seed(rows + C + groups)
    x = ints(g, (groups * gstride,), -8, 8)
    xr = torch.randn(groups * gstride, generator=g)
    pre = ints(g, (groups, C), -100, 100)
    buf, bufr = torch.zeros(lead + x.numel(), device="cuda"), torch.zeros(lead + x.numel(), device="cuda")
    assert buf.data_ptr() % 16 == 0 and bufr.data_ptr() % 16 == 0
    buf[lead:] = x.cuda()
    bufr[lead:] = xr.cuda()
    ref, refr = R.colsum(x, groups, gstride, rows, ld, c0, C), R.colsum(xr, groups, gstride, rows, ld, c0, C)
    try:
        for det in (0, 1):
            L.lib.zsg_set_deterministic(det)
            same(run_colsum(L, buf, lead, groups, gstride, rows, ld, c0, C, None).double(), ref, f"deterministic={det} accumulate=0")
            same(run_colsum(L, buf, lead, groups, gstride, rows, ld, c0, C, pre).double(), ref + pre.double(),
                 f"deterministic={det} accumulate=1")
        r1 = run_colsum(L, bufr, lead, groups, gstride, rows, ld, c0, C, None)
        r2 = run_colsum(L, bufr, lead, groups, gstride, rows, ld, c0, C, None)
        assert torch.equal(bits(r1), bits(r2)), "deterministic mode gave two different sums"
        close(r1, refr, 1e-4, 1e-4, "random data, deterministic")
    finally:
        L.lib.zsg_set_deterministic(0)


# ---- interleave, pad_rows, layout conversions, batch_sum ---------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 9])
@pytest.mark.parametrize("rows", [1, 7])
@pytest.mark.parametrize("k,off,gs", [(4, 0, 5), (1, 4, 5), (2, 1, 6)])
def test_interleave(L, k, off, gs, rows, groups):
    n, ns = rows * groups * k, rows * groups * gs
    g = torch.Generator().manual_seed(k * 10 + rows + groups)
    compact = ints(g, (n,), -1000, 1000)
    cd = compact.cuda()
    strided = fresh(ns)
    L.check(L.lib.zsg_interleave(cd.data_ptr(), rows, groups, k, strided.data_ptr(), gs, off, 0, L.stream_ptr()), "interleave 0")
    got = taken(strided, ns)
    same(got, R.interleave_to_strided(compact, torch.full((ns,), NAN), rows, groups, k, gs, off), "compact -> strided")
    outside = torch.ones(gs, dtype=torch.bool)
    outside[off:off + k] = False
    assert bool(torch.isnan(got.view(rows * groups, gs)[:, outside]).all()), "wrote outside [off, off + k)"
    back = fresh(n)
    L.check(L.lib.zsg_interleave(back.data_ptr(), rows, groups, k, strided.data_ptr(), gs, off, 1, L.stream_ptr()), "interleave 1")
    same(taken(back, n), compact, "round trip")
    refused(L, L.lib.zsg_interleave(cd.data_ptr(), rows, groups, k, strided.data_ptr(), off + k - 1, off, 0, L.stream_ptr()),
            "interleave: offset + k > group_stride")


@pytest.mark.parametrize("rows,C,src_ld,dst_ld", [(7, 45, 48, 45), (7, 45, 45, 48), (5, 3, 8, 4), (300, 5, 7, 9)])
def test_pad_rows(L, rows, C, src_ld, dst_ld):
    src = ints(torch.Generator().manual_seed(C + dst_ld), (rows * src_ld,), -1000, 1000)
    sd = src.cuda()
    dst = fresh(rows * dst_ld)
    L.check(L.lib.zsg_pad_rows(sd.data_ptr(), rows, C, src_ld, dst.data_ptr(), dst_ld, L.stream_ptr()), "pad_rows")
    assert torch.equal(bits(taken(dst, rows * dst_ld, (rows, dst_ld))), bits(R.pad_rows(src, rows, C, src_ld, dst_ld)))


@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_nchw_to_nhwc4_channels(L, C):
    B, H, W = 2, 5, 7
    img = ints(torch.Generator().manual_seed(C), (B, C, H, W), -1000, 1000)
    imd = img.cuda()
    out = fresh(B * H * W * 4)
    L.check(L.lib.zsg_nchw_to_nhwc4(imd.data_ptr(), B, C, H, W, out.data_ptr(), L.stream_ptr()), "nchw_to_nhwc4")
    assert torch.equal(bits(taken(out, B * H * W * 4, (B, H, W, 4))), bits(R.nchw_to_nhwc4(img)))


def test_u8hwc_to_nhwc4_every_byte(L):
    """all 256 byte values in every channel position, bit-equal to .float().div_(255); fourth channel +0"""
    i = torch.arange(256)
    img = torch.stack([i, (i + 85) % 256, (i * 7 + 3) % 256], 1).to(torch.uint8)
    assert all(len(set(img[:, c].tolist())) == 256 for c in range(3))
    imd = img.cuda()
    out = fresh(256 * 4)
    L.check(L.lib.zsg_u8hwc_to_nhwc4(imd.data_ptr(), 256, out.data_ptr(), L.stream_ptr()), "u8hwc_to_nhwc4")
    assert torch.equal(bits(taken(out, 256 * 4, (256, 4))), bits(R.u8hwc_to_nhwc4(img)))


@pytest.mark.parametrize("B", [1, 2, 16])
def test_batch_sum(L, B):
    stride = 4 * 77
    x = ints(torch.Generator().manual_seed(B), (B * stride,), -1000, 1000)
    xd = x.cuda()
    out = fresh(stride)
    L.check(L.lib.zsg_batch_sum(xd.data_ptr(), B, stride, out.data_ptr(), L.stream_ptr()), "batch_sum")
    same(taken(out, stride).double(), R.batch_sum(x, B, stride), "batch_sum")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals(L):
    """arguments each entry's own ZSG_REQUIRE rejects before any launch: -1 and a message.  Every pointer is a real 4096-float buffer and
    every size is tiny, so nothing here could touch foreign memory even if an entry launched."""
    a, b, c = (torch.zeros(4096, device="cuda") for _ in range(3))
    u = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    A, Bp, Cp, U, st = a.data_ptr(), b.data_ptr(), c.data_ptr(), u.data_ptr(), L.stream_ptr()
    lib = L.lib
    cases = [
        ("maxpool_fwd C % 4", lambda: lib.zsg_maxpool_fwd(A, 1, 2, 2, 6, 3, 2, 1, 1, 1, Bp, U, st)),
        ("maxpool_fwd k = 0", lambda: lib.zsg_maxpool_fwd(A, 1, 2, 2, 4, 0, 2, 1, 1, 1, Bp, U, st)),
        ("maxpool_fwd k = 16", lambda: lib.zsg_maxpool_fwd(A, 1, 2, 2, 4, 16, 2, 1, 1, 1, Bp, U, st)),
        ("maxpool_fwd s = 0", lambda: lib.zsg_maxpool_fwd(A, 1, 2, 2, 4, 3, 0, 1, 1, 1, Bp, U, st)),
        ("maxpool_fwd x = NULL", lambda: lib.zsg_maxpool_fwd(None, 1, 2, 2, 4, 3, 2, 1, 1, 1, Bp, U, st)),
        ("maxpool_bwd k = 16", lambda: lib.zsg_maxpool_bwd(A, U, 1, 2, 2, 4, 16, 2, 1, 1, 1, Bp, st)),
        ("maxpool_bwd C % 4", lambda: lib.zsg_maxpool_bwd(A, U, 1, 2, 2, 6, 3, 2, 1, 1, 1, Bp, st)),
        ("maxpool_bwd s = 0", lambda: lib.zsg_maxpool_bwd(A, U, 1, 2, 2, 4, 3, 0, 1, 1, 1, Bp, st)),
        ("maxpool_bwd idx = NULL", lambda: lib.zsg_maxpool_bwd(A, None, 1, 2, 2, 4, 3, 2, 1, 1, 1, Bp, st)),
        ("upsample_add_fwd C % 4", lambda: lib.zsg_upsample_add_fwd(A, Bp, 1, 1, 1, 2, 2, 6, Cp, st)),
        ("upsample_add_bwd C % 4", lambda: lib.zsg_upsample_add_bwd(A, 1, 1, 1, 2, 2, 6, Bp, 0, st)),
        ("relu_fwd n % 4", lambda: lib.zsg_relu_fwd(A, 6, Bp, st)),
        ("relu_bwd n % 4", lambda: lib.zsg_relu_bwd(A, Bp, 6, Cp, 0, st)),
        ("avgpool_fwd B = 0", lambda: lib.zsg_avgpool_fwd(A, 0, 9, 4, Bp, st)),
        ("avgpool_fwd HW = 0", lambda: lib.zsg_avgpool_fwd(A, 1, 0, 4, Bp, st)),
        ("avgpool_bwd C = 0", lambda: lib.zsg_avgpool_bwd(A, 1, 9, 0, Bp, 0, st)),
        ("l2norm_fwd rows = 0", lambda: lib.zsg_l2norm_fwd(A, 0, 4, Bp, Cp, st)),
        ("l2norm_fwd C = 0", lambda: lib.zsg_l2norm_fwd(A, 1, 0, Bp, Cp, st)),
        ("l2norm_bwd rows = 0", lambda: lib.zsg_l2norm_bwd(A, Bp, Cp, 0, 4, Cp, st)),
        ("nchw_to_nhwc4 C = 5", lambda: lib.zsg_nchw_to_nhwc4(A, 1, 5, 2, 2, Bp, st)),
        ("nchw_to_nhwc4 C = 0", lambda: lib.zsg_nchw_to_nhwc4(A, 1, 0, 2, 2, Bp, st)),
        ("u8hwc_to_nhwc4 pixels = 0", lambda: lib.zsg_u8hwc_to_nhwc4(U, 0, Bp, st)),
        ("colsum groups = 0", lambda: lib.zsg_colsum(A, 0, 0, 4, 8, 0, 8, Bp, 0, st)),
        ("colsum rows = 0", lambda: lib.zsg_colsum(A, 1, 0, 0, 8, 0, 8, Bp, 0, st)),
        ("colsum C = 0", lambda: lib.zsg_colsum(A, 1, 0, 4, 8, 0, 0, Bp, 0, st)),
        ("pad_rows dst_ld < C", lambda: lib.zsg_pad_rows(A, 2, 5, 5, Bp, 4, st)),
        ("pad_rows src_ld < C", lambda: lib.zsg_pad_rows(A, 2, 5, 4, Bp, 8, st)),
        ("pad_rows rows = 0", lambda: lib.zsg_pad_rows(A, 0, 5, 5, Bp, 8, st)),
        ("interleave offset < 0", lambda: lib.zsg_interleave(A, 2, 3, 1, Bp, 5, -1, 0, st)),
        ("interleave k = 0", lambda: lib.zsg_interleave(A, 2, 3, 0, Bp, 5, 0, 0, st)),
        ("interleave offset + k > stride", lambda: lib.zsg_interleave(A, 2, 3, 4, Bp, 5, 2, 0, st)),
        ("batch_sum stride % 4", lambda: lib.zsg_batch_sum(A, 2, 6, Bp, st)),
        ("batch_sum B = 0", lambda: lib.zsg_batch_sum(A, 0, 8, Bp, st)),
        ("memset_f32 NULL", lambda: lib.zsg_memset_f32(None, 4, 1.0, st)),
    ]
    for what, call in cases:
        refused(L, call(), what)
    torch.cuda.synchronize()
    assert float(a.abs().sum() + b.abs().sum() + c.abs().sum()) == 0 and int(u.sum()) == 0, "a refused call wrote something"
