"""tests/bn_ref.py against torch's own fp64 BatchNorm / ReLU / max-pool and their autograd on random real-valued data (1e-12 relative),
and the properties of its exact case data that tests/test_gpu_bn_passes.py relies on (the 2^24 condition above all)."""
import pytest
import torch
import torch.nn.functional as F

import bn_ref as R

EPS = 1e-5


def close(a, b, what):
    err = float((a - b).abs().max())
    scale = max(float(b.abs().max()), 1.0)
    assert err <= 1e-12 * scale, f"{what}: off by {err:.3g} (scale {scale:.3g})"


def real_case(rows, C, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return r(rows, C) * 3 + r(C), r(rows, C), r(rows, C), r(C) + 1.5, r(C)          # x, dout, residual, gamma, beta


def test_geom_tables():
    """the tables of the geometry grid: lanes and slabs per C, and the four cases whose rpb grows past 4 * rowlanes"""
    want = {4: (1, 1), 8: (2, 1), 16: (4, 1), 32: (8, 1), 64: (16, 1), 128: (32, 1), 256: (64, 1), 12: (2, 2), 20: (4, 2), 260: (64, 2),
            2048: (64, 8)}
    for C, (lanes, slabs) in want.items():
        g = R.bn_geom(1, C)
        assert (g["lanes"], g["slabs"], g["rowlanes"]) == (lanes, slabs, 256 // lanes), C
    assert set(R.GEOM_C) == set(want)
    for (C, rows), (rpb, rem) in zip(R.GROWN_RPB, ((1026, 2), (69, 5), (20, 0), (20, 0))):
        g = R.bn_geom(rows, C)
        assert g["rpb"] == rpb and rpb % g["rowlanes"] == rem and rpb > 4 * g["rowlanes"], (C, rows, g)
    for C in R.GEOM_C:                       # the per-C rows: fewer rows than row lanes, and a last chunk of a single row
        rl = R.bn_geom(1, C)["rowlanes"]
        assert R.bn_geom(4 * rl, C)["chunks"] == 1 and R.bn_geom(4 * rl + 1, C)["chunks"] == 2 and R.bn_geom(9 * rl + 3, C)["chunks"] == 3
    assert R.workspace_bytes(70001, 64) == (R.bn_geom(70001, 64)["chunks"] * 128 + 128) * 4


def test_mask_packing():
    bits = torch.tensor([[1, 0, 0, 0, 0, 1, 0, 0], [0, 0, 1, 0, 0, 0, 0, 1], [1, 1, 1, 1, 0, 0, 0, 0]]).bool()
    want = bits.view(-1, 4).int()
    want = (want[:, 0] | want[:, 1] << 1 | want[:, 2] << 2 | want[:, 3] << 3).to(torch.uint8)
    assert want.tolist() == [1, 2, 4, 8, 15, 0]
    assert torch.equal(R.pack_mask(bits), want)
    assert torch.equal(R.unpack_mask(want, 3, 8), bits)
    g = torch.Generator().manual_seed(1)
    m = torch.randint(0, 16, (35,), generator=g).to(torch.uint8)
    assert torch.equal(R.pack_mask(R.unpack_mask(m, 7, 20)), m)


@pytest.mark.parametrize("rows,C", [(37, 20), (5, 4), (129, 64)])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("with_relu", [False, True])
def test_train_matches_torch(rows, C, with_res, with_relu):
    """F.batch_norm(train) [+ residual] [+ relu] and its autograd: apply, backward_sums and bwd_apply with c1 = sum g / n, c2 = sum g xhat / n"""
    x, dout, res, gamma, beta = real_case(rows, C, rows * 7 + C)
    x.requires_grad_(True)
    res.requires_grad_(True)
    y = F.batch_norm(x, None, None, gamma, beta, True, 0.0, EPS)
    if with_res:
        y = y + res
    if with_relu:
        y = F.relu(y)
    (y * dout).sum().backward()
    xd = x.detach()
    mean = xd.mean(0)
    invstd = 1.0 / torch.sqrt(xd.var(0, unbiased=False) + EPS)
    out, mask = R.apply(xd, mean, invstd, gamma, beta, res.detach() if with_res else None, with_relu)
    close(out, y.detach(), "out")
    for g8 in ((mask, out) if with_relu else (None,)):                   # the mask bytes and the ReLU's output gate alike
        se, sse = R.backward_sums(dout, g8, xd, mean, invstd)
        dx, g = R.bwd_apply(dout, g8, xd, mean, invstd, gamma, se / rows, sse / rows)
        close(dx, x.grad, "dx")
        if with_res:
            close(g, res.grad, "g (the residual branch's gradient)")


@pytest.mark.parametrize("rows,C", [(37, 20), (129, 64)])
def test_frozen_matches_torch(rows, C):
    x, dout, res, gamma, beta = real_case(rows, C, rows * 11 + C)
    g = torch.Generator().manual_seed(5)
    rm, rv = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    x.requires_grad_(True)
    gamma.requires_grad_(True)
    beta.requires_grad_(True)
    y = F.relu(F.batch_norm(x, rm, rv, gamma, beta, False, 0.0, EPS) + res)
    (y * dout).sum().backward()
    invstd = 1.0 / torch.sqrt(rv + EPS)
    out, mask = R.apply(x.detach(), rm, invstd, gamma.detach(), beta.detach(), res, True)
    close(out, y.detach(), "out")
    ref = R.frozen_backward(dout, mask, x.detach(), rm, invstd, gamma.detach())
    close(ref["dx"], x.grad, "dx")
    close(ref["dgamma"], gamma.grad, "dgamma")
    close(ref["dbeta"], beta.grad, "dbeta")


def torch_codes(ind, W, k, s, p):
    """torch's flat input index h * W + w of [B, Ho, Wo, C] -> the window code r * k + q"""
    _, Ho, Wo, _ = ind.shape
    h, w = ind // W, ind % W
    r = h - (torch.arange(Ho) * s - p)[None, :, None, None]
    q = w - (torch.arange(Wo) * s - p)[None, None, :, None]
    assert bool(((r >= 0) & (r < k) & (q >= 0) & (q < k)).all())
    return (r * k + q).to(torch.uint8)


@pytest.mark.parametrize("k,s,p,ceil", R.STEM_KSP)
@pytest.mark.parametrize("H,W", [(13, 10), (7, 9)])
def test_stem_matches_torch(k, s, p, ceil, H, W):
    """max_pool2d(relu(batch_norm(x))) in train and frozen form, forward, indices and autograd, ceil-mode output sizes included"""
    B, C = 2, 8
    g = torch.Generator().manual_seed(k * 100 + s * 10 + p + H)
    r = lambda *sh: torch.randn(*sh, generator=g, dtype=torch.float64)
    x, gamma, beta = r(B, H, W, C) * 2 + r(C), r(C) + 1.5, r(C) * 0.3
    for frozen in (False, True):
        xt = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        ga, be = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        if frozen:
            mean, var = r(C) * 0.5, torch.rand(C, generator=g, dtype=torch.float64) + 0.5
            y = F.batch_norm(xt, mean, var, ga, be, False, 0.0, EPS)
        else:
            mean, var = x.reshape(-1, C).mean(0), x.reshape(-1, C).var(0, unbiased=False)
            y = F.batch_norm(xt, None, None, ga, be, True, 0.0, EPS)
        pooled, ind = F.max_pool2d(F.relu(y), k, s, p, ceil_mode=ceil, return_indices=True)
        Ho, Wo = pooled.shape[2:]
        assert (Ho, Wo) == (R.pool_out_size(H, k, s, p, ceil), R.pool_out_size(W, k, s, p, ceil))
        dout = r(B, Ho, Wo, C)
        (pooled.permute(0, 2, 3, 1) * dout).sum().backward()
        invstd = 1.0 / torch.sqrt(var + EPS)
        out, idx = R.stem_fwd(x, mean, invstd, gamma, beta, k, s, p, Ho, Wo)
        close(out, pooled.detach().permute(0, 2, 3, 1), "out")
        positive = out > 0                                     # (a window of zeros: any tap serves torch's gradient, none passes the ReLU)
        assert torch.equal(idx[positive], torch_codes(ind.permute(0, 2, 3, 1), W, k, s, p)[positive])
        dx_t = xt.grad.permute(0, 2, 3, 1)
        if frozen:
            ref = R.stem_frozen_backward(dout, idx, x, mean, invstd, gamma, beta, k, s, p)
            close(ref["dx"], dx_t, "frozen dx")
            close(ref["dgamma"], ga.grad, "frozen dgamma")
            close(ref["dbeta"], be.grad, "frozen dbeta")
        else:
            n = B * H * W
            se, sse = R.stem_backward_sums(dout, idx, x, mean, invstd, gamma, beta, k, s, p)
            close(se, be.grad, "dbeta")
            close(sse, ga.grad, "dgamma")
            close(R.stem_bwd_apply(dout, idx, x, mean, invstd, gamma, beta, k, s, p, se / n, sse / n), dx_t, "dx")


def f32_exact(t):
    return torch.equal(t.float().double(), t)


def test_geom_cases_are_exact():
    """every [rows, C] case of the GPU grid: the 2^24 condition (asserted inside case()), zeros of both signs after normalisation, and every
    reference value a number fp32 holds"""
    for C, rows in R.geom_cases():
        c = R.case(rows, C)
        assert c["worst"] < R.LIMIT
        assert R.exact_partial_row(rows, c["mean"], c["invstd"]).shape == (1, 2, C)          # (asserts its own exactness)
        for name in ("c1", "c2"):
            assert torch.equal(c[name] * 8, (c[name] * 8).round())
        if rows > 3000:
            continue
        out, mask = R.apply(c["x"], c["mean"], c["invstd"], c["gamma"], c["beta"], c["residual"], False)
        dx, g = R.bwd_apply(c["dout"], c["mask"], c["x"], c["mean"], c["invstd"], c["gamma"], c["c1"], c["c2"])
        assert f32_exact(out) and f32_exact(dx) and int(mask.max()) < 16
        plain = R.apply(c["x"], c["mean"], c["invstd"], c["gamma"], c["beta"], None, False)[0]
        zeros = plain[::3, :2]
        assert bool((zeros[:, 0] == 0).all()) and not bool(torch.signbit(zeros[:, 0]).any()), "+0 in channel 0"
        assert bool((zeros[:, 1] == 0).all()) and bool(torch.signbit(zeros[:, 1]).all()), "-0 in channel 1"


def test_stem_cases_are_exact_and_match_torch_indices():
    """every stem case of the GPU grid: the 2^24 condition, and on this integer data (most windows tie, at 0 above all) stem_fwd's idx
    equals torch's indices for ALL windows — torch's CPU pool keeps the first maximum too"""
    tied = 0
    for key in R.stem_cases():
        B, H, W, C, k, s, p, ceil = key
        c = R.stem_case(*key)
        assert c["worst"] < R.LIMIT and f32_exact(c["out"])
        v = R.apply(c["x"].reshape(-1, C), c["mean"], c["invstd"], c["gamma"], c["beta"], None, True)[0].reshape(B, H, W, C)
        pooled, ind = F.max_pool2d(v.permute(0, 3, 1, 2), k, s, p, ceil_mode=ceil, return_indices=True)
        assert tuple(pooled.shape[2:]) == (c["Ho"], c["Wo"]), key
        assert torch.equal(pooled.permute(0, 2, 3, 1), c["out"]), key
        assert torch.equal(torch_codes(ind.permute(0, 2, 3, 1), W, k, s, p), c["idx"]), key
        tied += int((c["out"] == 0).sum())
        dx = R.stem_bwd_apply(c["dout"], c["idx"], c["x"], c["mean"], c["invstd"], c["gamma"], c["beta"], k, s, p, c["c1"], c["c2"])
        assert f32_exact(dx), key
    assert tied > 1000, "the stem data must hold windows whose maximum is the ReLU's zero"


def test_special_values():
    """the rules the GPU tests pin: relu turns a NaN into 0 with mask bit 0, a NaN tap counts as 0 in the pool, and gates the gradient"""
    nan, inf = float("nan"), float("inf")
    tiny = 2.0 ** -140                                          # an fp32 denormal
    x = torch.tensor([[nan, 1.0, -0.0, inf], [-inf, 0.0, tiny, -tiny]])
    one, zero = torch.ones(4), torch.zeros(4)
    out, mask = R.apply(x, zero, one, one, zero, None, True)
    assert out.tolist() == [[0.0, 1.0, 0.0, inf], [0.0, 0.0, tiny, 0.0]] and mask.tolist() == [0b1010, 0b0100]
    assert not bool(torch.signbit(out).any())
    kept = R.apply(x, zero, one, one, zero, None, False)[0]
    assert bool(torch.isnan(kept[0, 0])) and not bool(torch.signbit(kept[0, 2]))          # (-0 - 0) * 1 + (+0) = +0 in IEEE arithmetic
    assert kept[1].tolist() == [-inf, 0.0, tiny, -tiny]
    xs = torch.tensor([[nan, -3.0, nan, nan], [nan, nan, 2.0, nan]]).view(1, 2, 1, 4)          # one window over two rows of one pixel
    o, i = R.stem_fwd(xs, zero, one, one, zero, 2, 2, 0, 1, 1)
    assert o.flatten().tolist() == [0.0, 0.0, 2.0, 0.0] and i.flatten().tolist() == [0, 0, 2, 0]
    g = R.stem_gather(torch.ones(1, 1, 1, 4), i, xs, zero, one, one, zero, 2, 2, 0)
    assert float(g.sum()) == 1 and float(g[0, 1, 0, 2]) == 1
