"""The element-wise kernels of a bf16_act eval plan (csrc/bf16_act.hip), each bit-equal to torch on the CPU: the contract is "fp32
arithmetic on the widened inputs in the fp32 kernel's order, ONE round-to-nearest-even at the store", which is what
op(x.float()).to(torch.bfloat16) computes when op itself is exact (max, ReLU, a single fp32 add) or is evaluated in the documented
order (the average pool's pixel-ascending sum, head conv0's ((Y + G) + (taps + bias)))."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from test_gpu_conv_bf16 import special_values  # noqa: E402

BF = torch.bfloat16


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib
    return _lib


def bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def same_bf16(got, want):
    """bit equality; NaN must sit where NaN is expected (its payload is free)"""
    got, want = got.cpu(), want.cpu()
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(bits16(got)[~nan], bits16(want)[~nan])


def poison16(*shape):
    return torch.full(shape, 0x7FC0, dtype=torch.int16, device="cuda").view(BF)


def nhwc_pool(x, k, s, p, ceil):
    return F.max_pool2d(x.permute(0, 3, 1, 2), k, s, p, ceil_mode=ceil).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("geo", [(2, 9, 11, 64, 3, 2, 1, False), (2, 7, 7, 64, 2, 2, 0, True), (1, 6, 5, 36, 3, 2, 1, False)],
                         ids=["stem_3_2_1", "ssd_ceil_2_2_0", "c36_groups_of_4"])
def test_maxpool(L, geo):
    B, H, W, Cc, k, s, p, ceil = geo
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, H, W, Cc, generator=g)
    x[0, 0, 0, :4] = torch.tensor([float("inf"), float("-inf"), float("nan"), 0.0])
    want32 = nhwc_pool(x, k, s, p, ceil)
    Ho, Wo = want32.shape[1:3]
    for x_bf16 in (0, 1):
        xin = x.to(BF) if x_bf16 else x
        want = nhwc_pool(xin.float(), k, s, p, ceil).to(BF)
        xd = xin.cuda()
        out = poison16(B * Ho * Wo * Cc + 16)
        L.check(L.lib.zsg_maxpool_fwd_bf16(xd.data_ptr(), x_bf16, B, H, W, Cc, k, s, p, Ho, Wo, out.data_ptr(), L.stream_ptr()), "maxpool")
        torch.cuda.synchronize()
        assert same_bf16(out[:-16].view(B, Ho, Wo, Cc), want), f"x_bf16={x_bf16}"
        assert bool(torch.isnan(out[-16:]).all()), "wrote past the output"


@pytest.mark.parametrize("geo", [(2, 3, 3, 5, 5, 256), (2, 5, 5, 10, 10, 256), (1, 2, 3, 4, 5, 36)], ids=["3to5", "5to10", "c36"])
def test_upsample_add(L, geo):
    B, Hs, Ws, Hd, Wd, Cc = geo
    g = torch.Generator().manual_seed(4)
    a, p = torch.randn(B, Hd, Wd, Cc, generator=g).to(BF), torch.randn(B, Hs, Ws, Cc, generator=g).to(BF)
    up = F.interpolate(p.float().permute(0, 3, 1, 2), size=(Hd, Wd), mode="nearest").permute(0, 2, 3, 1)
    want = (a.float() + up).to(BF)
    ad, pd, out = a.cuda(), p.cuda(), poison16(B * Hd * Wd * Cc + 16)
    L.check(L.lib.zsg_upsample_add_fwd_bf16(ad.data_ptr(), pd.data_ptr(), B, Hs, Ws, Hd, Wd, Cc, out.data_ptr(), L.stream_ptr()), "upsample_add")
    torch.cuda.synchronize()
    assert same_bf16(out[:-16].view(B, Hd, Wd, Cc), want)
    assert bool(torch.isnan(out[-16:]).all())
    assert not torch.equal(want.float(), a.float() + up), "the sum must need rounding somewhere, else the store's rounding is not tested"


@pytest.mark.parametrize("n", [2 * 3 * 3 * 256, 4 * 37])
def test_relu(L, n):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, generator=g)
    x[:4] = torch.tensor([float("inf"), float("-inf"), -0.0, 0.0])
    x = x.to(BF)
    want = torch.clamp(x.float(), min=0).to(BF)
    xd, out = x.cuda(), poison16(n + 16)
    L.check(L.lib.zsg_relu_fwd_bf16(xd.data_ptr(), n, out.data_ptr(), L.stream_ptr()), "relu")
    torch.cuda.synchronize()
    assert torch.equal(out[:n].float().cpu(), want.float())
    assert bool(torch.isnan(out[n:]).all())


def test_avgpool_is_the_pixel_ascending_fp32_sum(L):
    B, HW, Cc = 2, 4, 256
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, HW, Cc, generator=g).to(BF)
    s = torch.zeros(B, Cc)
    for k in range(HW):
        s = s + x[:, k].float()
    want = (s / float(HW)).to(BF)
    xd, out = x.cuda(), poison16(B * Cc + 16)
    L.check(L.lib.zsg_avgpool_fwd_bf16(xd.data_ptr(), B, HW, Cc, out.data_ptr(), L.stream_ptr()), "avgpool")
    torch.cuda.synchronize()
    assert same_bf16(out[:-16].view(B, Cc), want) and bool(torch.isnan(out[-16:]).all())


@pytest.mark.parametrize("n,shift", [(4096 + 18, 0), (1031, 1)], ids=["aligned", "odd_offset_and_tail"])
def test_casts_on_the_special_values(L, n, shift):
    """+-0, +-inf preserved, NaN stays NaN, ties to even, overflow to inf: Tensor.to(torch.bfloat16); widening is exact"""
    g = torch.Generator().manual_seed(7)
    sv = special_values()
    x = torch.randn(n, generator=g)
    x[5:5 + len(sv)] = sv
    x[n - len(sv):] = sv
    want = x.to(BF)
    assert int(torch.isinf(want).sum()) > int(torch.isinf(x).sum()), "an overflow-to-inf case must be among the values"
    xd = torch.zeros(n + shift, device="cuda")
    xd[shift:].copy_(x)
    out = poison16(n + shift + 16)
    L.check(L.lib.zsg_cast_f32_bf16(xd[shift:].data_ptr(), n, out[shift:].data_ptr(), L.stream_ptr()), "cast_f32_bf16")
    torch.cuda.synchronize()
    assert same_bf16(out[shift:shift + n], want)
    z = want.float() == 0
    assert int(z.sum()) >= 4 and torch.equal(torch.signbit(out[shift:shift + n].float().cpu())[z], torch.signbit(want.float())[z]), "the sign of zero"
    assert bool(torch.isnan(out[:shift]).all()) and bool(torch.isnan(out[shift + n:]).all())
    back = torch.full((n + shift + 16,), float("nan"), device="cuda")
    src16 = out.clone()
    L.check(L.lib.zsg_cast_bf16_f32(src16[shift:].data_ptr(), n, back[shift:].data_ptr(), L.stream_ptr()), "cast_bf16_f32")
    torch.cuda.synchronize()
    w32, b32 = want.float(), back[shift:shift + n].cpu()
    nan = torch.isnan(w32)
    assert torch.equal(torch.isnan(b32), nan) and torch.equal(b32[~nan].view(torch.int32), w32[~nan].view(torch.int32))
    assert bool(torch.isnan(back[shift + n:]).all())


def shared_conv0_ref(Y, idx, bias, G, V, sizes, Q):
    """h1 in the documented order, fp32 on the CPU: c = (taps in row-major order, summed from 0) + bias; relu((Y + G) + c)"""
    N = bias.numel()
    outs, p0 = [], 0
    for (h, w) in sizes:
        o = torch.empty(Q, h, w, N)
        for q in range(Q):
            for y in range(h):
                for x in range(w):
                    a = torch.zeros(N)
                    for r in range(3):
                        if (r == 0 and y == 0) or (r == 2 and y == h - 1):
                            continue
                        for t in range(3):
                            if (t == 0 and x == 0) or (t == 2 and x == w - 1):
                                continue
                            a = a + V[q, :, r * 3 + t]
                    c = a + bias
                    i = int(idx[q])
                    if 0 <= i < Y[0].shape[0]:
                        o[q, y, x] = torch.clamp((Y[len(outs)][i, y, x] + G[len(outs)][y, x]) + c, min=0)
                    else:
                        o[q, y, x] = float("nan")
        outs.append(o)
        p0 += h * w
    return outs


@pytest.mark.parametrize("i64", [1, 0])
def test_head_shared_conv0_bf16(L, i64):
    sizes, Bi, Q, N = [(4, 3), (2, 2), (1, 1)], 2, 4, 64
    g = torch.Generator().manual_seed(8)
    Y = [torch.randn(Bi, h, w, N, generator=g) for (h, w) in sizes]
    G = [torch.randn(h, w, N, generator=g) for (h, w) in sizes]
    V = torch.randn(Q, N, 9, generator=g)
    bias = torch.randn(N, generator=g)
    idx = torch.tensor([1, 0, 7, 1], dtype=torch.int64 if i64 else torch.int32)         # query 2 points outside [0, Bi)
    want = [o.to(BF) for o in shared_conv0_ref(Y, idx, bias, G, V, sizes, Q)]
    Yd = torch.cat([t.reshape(-1) for t in Y]).cuda()
    Gd = torch.cat([t.reshape(-1) for t in G]).cuda()
    Vd, bd, idd = V.reshape(-1).cuda(), bias.cuda(), idx.cuda()
    hw = torch.tensor([v for s in sizes for v in s], dtype=torch.int32)
    P = sum(h * w for h, w in sizes)
    out = poison16(Q * P * N + 16)
    L.check(L.lib.zsg_head_shared_conv0_bf16(Yd.data_ptr(), idd.data_ptr(), i64, bd.data_ptr(), Gd.data_ptr(), Vd.data_ptr(), Bi, Q, len(sizes),
                                             hw.data_ptr(), N, out.data_ptr(), L.stream_ptr()), "shared conv0")
    torch.cuda.synchronize()
    o = 0
    for (h, w), wt in zip(sizes, want):
        got = out[o:o + Q * h * w * N].view(Q, h, w, N)
        assert same_bf16(got, wt), (h, w)
        assert bool(torch.isnan(got[2]).all()) and not bool(torch.isnan(got[0]).any())
        o += Q * h * w * N
    assert bool(torch.isnan(out[o:]).all())
    # the fp32 kernel on the same inputs, rounded afterwards, gives the same bits: one order, one rounding
    o32 = torch.full((Q * P * N,), float("nan"), device="cuda")
    L.check(L.lib.zsg_head_shared_conv0(Yd.data_ptr(), idd.data_ptr(), i64, bd.data_ptr(), Gd.data_ptr(), Vd.data_ptr(), Bi, Q, len(sizes),
                                        hw.data_ptr(), N, o32.data_ptr(), L.stream_ptr()), "shared conv0 fp32")
    torch.cuda.synchronize()
    assert same_bf16(out[:Q * P * N], o32.to(BF))
