"""The host reference of the exact fp32 convolution tests (tests/conv_exact_ref.py) against torch's float64 convolution and autograd on
every case geometry, the fp32 exactness conditions of every case (conditions on the INPUTS, asserted from the reference alone — what
allows tests/test_gpu_conv_exact.py to compare at zero tolerance), negative controls (a comparison that cannot fail proves nothing)
and the operand builder's poison / guard / sentinel placement.  No GPU, nothing of the product."""
import pytest
import torch
import torch.nn.functional as F

import conv_exact_ref as R
from wgrad_bf16_ref import wgrad_ref_levels

NAMES = [c.name for c in R.CASES]


def _dense(cd):
    """per level: x [B,H,W,C], dy [B,Ho,Wo,N] as dense float64 tensors read back through the views"""
    c = cd.c
    sv, gv = c.src_view(), c.out_view(c.dy_ld)
    xs = [cd.x[sv.index(l)] for l in range(len(c.sizes))]
    gs = [cd.dy_w[gv.index(l)] for l in range(len(c.sizes))]
    return xs, gs


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_torch_float64(name):
    cd = R.case_data(name)
    c = cd.c
    xs, gs = _dense(cd)
    w = cd.w_dense.permute(0, 3, 1, 2).contiguous().requires_grad_()            # OIHW
    gw = torch.zeros_like(w)
    dx_ref = R.forward(cd.G, cd.dy_d, cd.wt.reshape(-1), torch.zeros(R.out_extent(cd.G), dtype=R.DT))      # (zero_fill: the caller clears dx)
    for l, (x, g) in enumerate(zip(xs, gs)):
        xt = x.permute(0, 3, 1, 2).contiguous().requires_grad_()
        y = F.conv2d(xt, w, None, c.s, c.p, c.d)
        assert torch.equal(cd.fwd_rows()[l], y.detach().permute(0, 2, 3, 1)), "forward"
        gi, gwl = torch.autograd.grad(y, (xt, w), g.permute(0, 3, 1, 2))
        gw += gwl
        assert torch.equal(dx_ref[c.src_view().index(l)], gi.permute(0, 2, 3, 1)), "data gradient (all parity classes)"
    assert torch.equal(cd.dw(), gw.permute(0, 2, 3, 1)), "weight gradient (levels add)"
    assert torch.equal(cd.dw(), wgrad_ref_levels(xs, gs, c.k, c.s, c.p, c.d)), "weight gradient vs wgrad_bf16_ref"
    # window, wt_ld slack and accumulate: only the window changes, by exactly the gradient
    init = torch.full((R.wt_extent(cd.W),), 5.0, dtype=R.DT)
    for acc in (0, 1):
        dw = R.wgrad(cd.W, cd.x, cd.dy_w, init, acc)
        keep = torch.ones_like(init, dtype=torch.bool)
        keep[cd.w_idx.reshape(-1)] = False
        assert torch.equal(dw[keep], init[keep]) and torch.equal(dw[cd.w_idx], cd.dw() + 5.0 * acc)


@pytest.mark.parametrize("name", NAMES)
def test_epilogue_and_partials(name):
    cd = R.case_data(name)
    c, D = cd.c, cd.c.fwd(relu=True)
    init = torch.full((R.out_extent(D),), R.SENTINEL, dtype=R.DT)
    out = R.forward(D, cd.x, cd.w, init, cd.bias, cd.add, cd.mask)
    ov = c.out_view()
    for l, acc in enumerate(cd.fwd_rows()):
        i = ov.index(l)
        want = torch.clamp(acc + cd.bias + cd.add[i], min=0) * (cd.mask[i] > 0)
        assert torch.equal(out[i], want)
    keep = torch.ones_like(init, dtype=torch.bool)
    keep[cd.o_idx] = False
    assert torch.equal(out[keep], init[keep]), "nothing outside the addressed rows is written"
    rows = torch.cat([r.reshape(-1, c.N) for r in cd.fwd_rows()])
    for bm in (64, 128):
        part = R.tile_partials(cd.fwd_rows(), bm)
        assert part.shape == (sum(-(-c.B * h * w // bm) for h, w in c.osizes), 2, c.N)
        assert torch.equal(part[:, 0].sum(0), rows.sum(0)) and torch.equal(part[:, 1].sum(0), (rows * rows).sum(0))
        assert torch.equal(part[0, 0], cd.fwd_rows()[0].reshape(-1, c.N)[:bm].sum(0))
    if c.wino:
        for tb in (32, 64):
            part = R.wino_tile_partials(cd.fwd_rows(), tb)
            assert part.shape[0] == sum(-(-c.B * ((h + 1) // 2) * ((w + 1) // 2) // tb) for h, w in c.osizes)
            assert torch.equal(part[:, 0].sum(0), rows.sum(0)) and torch.equal(part[:, 1].sum(0), (rows * rows).sum(0))


@pytest.mark.parametrize("name", NAMES)
def test_exactness_conditions(name):
    """sum_K |x||w| (times the Winograd-domain amplification, conv_exact_ref.wino_amplification: derived from the transform matrices)
    < 2^22 — two bits below 2^24 for the transformed filter's quarter-integers; fused statistics: sum_rows y^2 < 2^24 per column;
    accumulate / add epilogues: |sum| + |operands| < 2^24.  Every fp32 partial sum, in any order, of any kernel variant is then an
    exactly representable (quarter-)integer."""
    cd = R.case_data(name)
    e = R.exactness(cd)
    amp = R.wino_amplification() if cd.c.wino else 1.0
    amp_wg = R.wino_amplification(R.WINOWG_G, R.WINOWG_BT, R.WINOWG_AT) if cd.c.wino else 1.0
    assert amp == 9.0 or amp == 1.0
    assert e["fwd_abs"] * amp < 2 ** 22 and e["dgrad_abs"] * amp < 2 ** 22 and e["wgrad_abs"] * amp_wg < 2 ** 22, e
    assert e["sumsq"] < 2 ** 24 and e["sum_abs"] < 2 ** 24, e
    assert e["fwd_epi"] < 2 ** 24 and e["dgrad_epi"] < 2 ** 24 and e["wgrad_epi"] < 2 ** 24, e
    # the data themselves: non-zero integers of the stated range
    for v, a in ((cd.x[cd.x_idx], cd.c.amp), (cd.w[cd.w_idx], cd.c.amp), (cd.dy_w[cd.g_idx], cd.c.amp_g)):
        assert bool(((v != 0) & (v.abs() <= a) & (v == v.round())).all())


def test_winograd_matrices():
    """the matrices behind the amplification bound ARE F(2x2,3x3) / F(3x3,2x2): the transformed products reproduce the direct sums"""
    g = torch.Generator().manual_seed(5)
    d = R.rand_int((4, 4), 3, g)
    w = R.rand_int((1, 3, 3, 1), 3, g)
    U = R.wino_filter_image(w)[0, :, :, 0]
    assert torch.equal(U * 4, (U * 4).round()), "quarter-integers"
    Y = R.WINO_AT @ (U * (R.WINO_BT @ d @ R.WINO_BT.t())) @ R.WINO_AT.t()
    want = torch.stack([torch.stack([(d[i:i + 3, j:j + 3] * w[0, :, :, 0]).sum() for j in range(2)]) for i in range(2)])
    assert torch.equal(Y, want)
    Uf = R.wino_filter_image(w, flip=True)[0, :, :, 0]
    assert torch.equal(Uf, R.wino_filter_image(w.flip((1, 2)))[0, :, :, 0])
    gy = R.rand_int((2, 2), 3, g)
    dW = R.WINOWG_AT @ ((R.WINOWG_G @ gy @ R.WINOWG_G.t()) * (R.WINOWG_BT @ d @ R.WINOWG_BT.t())) @ R.WINOWG_AT.t()
    want = torch.stack([torch.stack([(d[i:i + 2, j:j + 2] * gy).sum() for j in range(3)]) for i in range(3)])
    assert torch.equal(dW, want)
    assert R.wino_amplification() == 9.0 and R.wino_amplification(R.WINOWG_G, R.WINOWG_BT, R.WINOWG_AT) == 9.0


@pytest.mark.parametrize("name", NAMES)
def test_negative_controls(name):
    """a reference with the last K element dropped, one tap shifted, one parity class / one level omitted differs from the true one"""
    cd = R.case_data(name)
    true_f, true_d, true_w = cd.fwd_rows(), cd.dg_rows(), cd.dw()
    differs = lambda a, b: any(not torch.equal(p, q) for p, q in zip(a, b))
    for m in ("drop_last_k", "shift_tap"):
        assert differs(cd.fwd_rows(m), true_f), m
        assert differs(cd.dg_rows(m), true_d), m
        assert not torch.equal(cd.dw(m), true_w), m
    if cd.F.nseg > 1:
        assert differs(cd.fwd_rows("drop_seg"), true_f) and not torch.equal(cd.dw("drop_seg"), true_w), "a level omitted"
    if cd.G.nseg > 1:
        assert differs(cd.dg_rows("drop_seg"), true_d), "a parity class / level omitted"
    assert sum(d.G.nseg > 1 and d.c.s > 1 for d in map(R.case_data, NAMES)) >= 1
    # ... and a neighbouring geometry (the GPU test's own negative control: pad 0 instead of 1)
    if cd.c.p == 1:
        assert differs(R.pad0_neighbour_rows(cd), true_f)


@pytest.mark.parametrize("name", NAMES)
def test_builder_places_poison_guards_sentinels(name):
    cd = R.case_data(name)
    c = cd.c
    nan = torch.isnan
    for D, data, idx in ((cd.F, cd.x, cd.x_idx), (cd.G, cd.dy_d, cd.dy_d_idx)):
        b = R.build_input(R.src_extent(D), idx, data[idx])
        assert b.t.numel() == 2 * R.GUARD + R.src_extent(D)
        assert bool(nan(b.t[:R.GUARD]).all() and nan(b.t[-R.GUARD:]).all()), "NaN guards"
        assert not bool(nan(b.body).any())
        assert torch.equal(b.body[idx].double(), data[idx]) and not bool((b.body[idx] == R.POISON).any()), "an addressed element is never poisoned"
        rest = torch.ones(b.extent, dtype=torch.bool)
        rest[idx] = False
        assert bool((b.body[rest] == R.POISON).all())
        assert int(rest.sum()) == b.extent - len(idx)
    if c.src_ld > c.C or c.src_gap:
        assert R.src_extent(cd.F) > len(cd.x_idx), "padded rows / gaps hold poison"
    # the data gradient's pad lanes are operand zeros (C_red = dy.ld), the weight gradient's are poison
    if c.dy_ld > c.N:
        pad = c.out_view(c.dy_ld).index(0, c.dy_ld)[..., c.N:]
        assert bool((cd.dy_d[pad] == 0).all()) and bool((cd.dy_w[pad] == R.POISON).all())
        assert bool((cd.wt[..., c.N:] == 0).all())
    w = R.build_input(R.wt_extent(cd.F), cd.w_idx, cd.w[cd.w_idx])
    assert int((w.body == R.POISON).sum()) == c.N * c.wt_ld - c.N * c.k * c.k * c.C
    # outputs: NaN exactly where the launch writes, sentinel everywhere else (guards included)
    for shift in (0, c.out_shift):
        o = R.build_output(R.out_extent(cd.F), cd.o_idx, shift=shift)
        assert int(nan(o.t).sum()) == len(cd.o_idx) == c.N * sum(c.B * h * w for h, w in c.osizes)
        assert bool(nan(o.body[cd.o_idx]).all())
        assert bool((o.t[~nan(o.t)] == R.SENTINEL).all())
        assert o.lo == R.GUARD + shift
        e = R.expected_output(o, torch.zeros(o.extent, dtype=R.DT), cd.o_idx)
        assert not bool(nan(e).any()) and int((e == 0).sum()) == len(cd.o_idx)
    if c.out_ld > c.N or c.out_gap or c.scatter:
        assert R.out_extent(cd.F) > len(cd.o_idx) or len(c.sizes) > 1
    dwb = R.build_output(R.wt_extent(cd.W), cd.w_idx)
    assert int(nan(dwb.t).sum()) == cd.w_idx.numel()


def test_descriptor_builders():
    """the stride-parity decomposition covers every dx pixel at most once and drops only tap-less classes"""
    for name in NAMES:
        cd = R.case_data(name)
        i = R.out_written(cd.G)
        assert len(torch.unique(i)) == len(i)
        full = sum(cd.c.B * h * w for h, w in cd.c.sizes) * cd.c.C
        assert (len(i) < full) == cd.G.zero_fill
    assert R.case_data("pws2").G.zero_fill and R.case_data("pws2").G.nseg == 1
    assert R.case_data("c3s2").G.nseg == 4 and not R.case_data("c3s2").G.zero_fill
