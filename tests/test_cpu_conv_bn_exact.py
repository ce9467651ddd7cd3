"""The host reference of the exact BatchNorm-fused convolution tests (tests/conv_bn_exact_ref.py) against independent float64 torch —
autograd through F.conv2d followed by aten's native_batch_norm_backward for the backward sums and coefficients, F.batch_norm in
training mode for the forward statistics and running buffers, F.batch_norm in eval mode + ReLU + F.conv2d for the BatchNorm-applying
loader —, the fp32 exactness conditions of every case (conditions on the INPUTS: what lets tests/test_gpu_conv_bn_exact.py compare at
zero tolerance), and the mutation check: every subtly wrong reference differs from the true one on every case that claims the edge.
No GPU, nothing of the product."""
import pytest
import torch
import torch.nn.functional as F

import conv_bn_exact_ref as B
import conv_exact_ref as R

NAMES = [c.name for c in B.CASES]
BIG = {"d_r128", "d_r129", "d_r128b", "d_r129b", "f_r128", "f_r129", "f_r128b", "f_r129b"}          # (row-count limits: data as the small cases)
TORCH = [n for n in NAMES if n not in BIG]


def _views(c):
    k, s, p, d = c.k, c.s, c.p, c.d
    osz = [(R.conv_out(h, k, s, p, d), R.conv_out(w, k, s, p, d)) for h, w in c.sizes]
    if c.mode == "dg":
        return R.make_view(c.B, c.K, osz), R.make_view(c.B, c.N, c.sizes)
    return R.make_view(c.B, c.K, c.sizes), R.make_view(c.B, c.N, osz)


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("name", [n for n in TORCH if B.CASE[n].mode == "dg"])
def test_bnb_reference_equals_torch(name):
    bd = B.data(name)
    c = bd.c
    dyv, dxv = _views(c)
    w = bd.w.view(c.N, c.k, c.k, c.K).permute(3, 0, 1, 2).contiguous()                  # the transposed image -> OIHW of the forward
    douts = []
    for l, (h, wd) in enumerate(c.sizes):
        xin = torch.zeros(c.B, c.N, h, wd, dtype=R.DT, requires_grad=True)
        y = F.conv2d(xin, w, None, c.s, c.p, c.d)
        gi, = torch.autograd.grad(y, xin, _nchw(bd.x[dyv.index(l)]))
        douts.append((gi.permute(0, 2, 3, 1), dxv.index(l)))
    n = float(B.total_rows(bd.D))
    for mask in (True, False):
        for add in (True, False):
            out, part = bd.bnb(64, False, mask, add)
            outm, partm = bd.bnb(64, False, mask, add, epi=1)
            assert torch.equal(part, partm), "the masked store changes no sum"
            gs, xs = [], []
            for gi, idx in douts:
                v = gi + (bd.add[idx] if add else 0)
                assert torch.equal(out[idx], v), "stored dout"
                g = v * bd.bits[idx] if mask else v
                assert torch.equal(outm[idx], g), "epi_flags bit 0: stored g"
                gs.append(g.reshape(-1, c.N))
                xs.append(bd.bn_x[idx].reshape(-1, c.N))
            g, x = torch.cat(gs), torch.cat(xs)
            dx, dgamma, dbeta = torch.ops.aten.native_batch_norm_backward(g, x, torch.ones(c.N, dtype=R.DT), None, None, bd.mean, bd.invstd,
                                                                          True, 1e-5, [True, True, True])
            S, SS = part[:, 0].sum(0), part[:, 1].sum(0)
            assert torch.equal(S, dbeta) and torch.equal(SS, dgamma), "column totals = native_batch_norm_backward's dbeta / dgamma"
            for tile, wino in ((128, False), (None, False)) + (((32, True), (64, True)) if c.wino else ()):
                p2 = bd.bnb(tile, wino, mask, add)[1]
                assert torch.equal(p2[:, 0].sum(0), S) and torch.equal(p2[:, 1].sum(0), SS), (tile, wino)
            fin = B.finalize_bwd(S, SS, n, 1, bd.dg0, bd.db0)
            xh = (x - bd.mean) * bd.invstd
            assert torch.allclose(bd.invstd * (g - fin["coef"][0] - xh * fin["coef"][1]), dx, rtol=1e-12, atol=1e-12), "coef: the input gradient's formula"
            assert torch.equal(fin["dbeta"], bd.db0 + dbeta) and torch.equal(fin["dgamma"], bd.dg0 + dgamma)
            fin0 = B.finalize_bwd(S, SS, n, 0, bd.dg0, bd.db0)
            assert torch.equal(fin0["dbeta"], dbeta) and torch.equal(fin0["dgamma"], dgamma)


def _forward_rows(bd, src):
    c = bd.c
    sv, ov = _views(c)
    w = bd.w.view(c.N, c.k, c.k, c.K).permute(0, 3, 1, 2).contiguous()
    ys = []
    for l in range(len(c.sizes)):
        y = F.conv2d(_nchw(src[sv.index(l)]), w, None, c.s, c.p, c.d).permute(0, 2, 3, 1)
        assert torch.equal(bd.rows[l], y), "convolution"
        ys.append(y.reshape(-1, c.N))
    return torch.cat(ys)


def _check_forward_statistics(bd, y):
    c = bd.c
    n = float(y.shape[0])
    assert n == B.total_rows(bd.D)
    for tile, wino in ((64, False), (128, False)) + (((32, True), (64, True)) if c.wino else ()):
        part = bd.stat(tile, wino)
        S, SS = part[:, 0].sum(0), part[:, 1].sum(0)
        assert torch.equal(S, y.sum(0)) and torch.equal(SS, (y * y).sum(0)), (tile, wino)
    if not c.wino:
        assert torch.equal(bd.stat(64), R.tile_partials(bd.rows, 64)) and torch.equal(bd.stat(128), R.tile_partials(bd.rows, 128))
    else:
        assert torch.equal(bd.stat(32, True), R.wino_tile_partials(bd.rows, 32))
    fin = B.finalize_fwd(S, SS, n, bd.rm0, bd.rv0)
    var = y.var(0, unbiased=False)
    assert torch.allclose(fin["mean"], y.mean(0), rtol=1e-12, atol=1e-12)
    assert torch.allclose(fin["invstd"], 1 / torch.sqrt(var + B.EPS), rtol=1e-9)
    if n > 1:
        rm, rv = bd.rm0.clone(), bd.rv0.clone()
        F.batch_norm(y, rm, rv, None, None, True, B.MOM, B.EPS)
        assert torch.allclose(fin["rmean"], rm, rtol=1e-6, atol=1e-6) and torch.allclose(fin["rvar"], rv, rtol=1e-6), "running buffers (f32(m) in between)"
    else:
        assert torch.equal(fin["rvar"], 0.75 * bd.rv0) and bool((var == 0).all())
    # no cancellation in the running-mean update: 1 ulp of f32(m) stays below 1 ulp of the result
    assert bool((fin["rmean"].abs() >= B.MOM * fin["mean"].abs()).all())


@pytest.mark.parametrize("name", [n for n in TORCH if B.CASE[n].mode == "fw"])
def test_bnstat_reference_equals_torch(name):
    bd = B.data(name)
    _check_forward_statistics(bd, _forward_rows(bd, bd.x))


@pytest.mark.parametrize("name", [n for n in NAMES if B.CASE[n].mode == "pre"])
def test_bnpre_reference_equals_torch(name):
    bd = B.data(name)
    c = bd.c
    eps = 2.0 ** -20          # (var + eps is 1 or 4 exactly in fp64: F.batch_norm's rsqrt returns the power of two)
    y = F.relu(F.batch_norm(bd.x, bd.pre_mean.clone(), 1 / bd.pre_invstd ** 2 - eps, bd.pre_gamma, bd.pre_beta, False, 0.0, eps) + bd.pre_res)
    assert torch.equal(y, bd.pre_y), "the materialised activation"
    assert torch.equal(bd.pre_bits, (y > 0).to(R.DT))
    assert int((bd.pre_v == 0).sum()) >= y.shape[0], "exact zeros before the ReLU (bit 0) in every row"
    last = bd.pre_v[:, c.K - 4:]
    assert bool(((last[:, 0] > 0) & (last[:, 1] == 0) & (last[:, 2] < 0) & (last[:, 3] > 0)).all()), "every row's last column group: +, 0, -, +"
    assert B.pack_bits(bd.pre_bits)[c.K // 4 - 1::c.K // 4].tolist() == [0b1001] * y.shape[0]
    _check_forward_statistics(bd, _forward_rows(bd, bd.pre_y.reshape(-1)))


def test_pack_bits_layout():
    """include/zsg.h: bit e of byte i = element 4i+e, bits 4-7 zero"""
    bits = torch.tensor([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 1, 1, 1])
    assert B.pack_bits(bits).tolist() == [1, 2, 4, 8, 15]


@pytest.mark.parametrize("name", NAMES)
def test_exactness_conditions(name):
    """sum_K |x||w| (x 9 in the Winograd domain, conv_exact_ref.wino_amplification) < 2^22; every column total of absolute values
    < 2^23 for the sums (the 1-ulp argument of the finalize: |S| < 2^23) and < 2^24 for the second sums, half-integers counted double;
    every partial row and every workgroup total of the streaming kernel is a part of those"""
    bd = B.data(name)
    e = B.exactness(bd)
    amp = R.wino_amplification() if bd.c.wino else 1.0
    assert e["conv_abs"] * amp < 2 ** 22, e
    assert e["S_abs"] < 2 ** 23 and e["SS"] < 2 ** 24, e
    if bd.c.mode == "dg":
        assert e["acc_abs"] + e["SS"] < 2 ** 24
        for tile, wino in ((64, False), (128, False)) + (((32, True), (64, True)) if bd.c.wino else ()):
            part = bd.bnb(tile, wino)[1]
            assert torch.equal(part * 2, (part * 2).round()) and float(part.abs().max()) < 2 ** 23
        rows = bd.bits.view(-1, bd.c.N)
        assert bool((rows.min(1).values == 0).all() and (rows.max(1).values == 1).all()), "zeros and ones in every row"
        lg = rows[:, -4:]
        assert bool((lg.min(1).values == 0).all() and (lg.max(1).values == 1).all()), "... and in every row's last column group"
        assert len(torch.unique(bd.invstd)) > 1
    if bd.c.mode == "pre":
        assert e["pre_abs"] < 2 ** 20
        assert len(torch.unique(bd.pre_invstd * bd.pre_gamma.abs())) > 1 and bool((bd.pre_gamma < 0).any() and (bd.pre_gamma > 0).any())
    assert bool((bd.rm0 % 4 == 0).all() and (bd.rv0 % 4 == 0).all())


def _mutants(bd, m):
    """(true, mutated) result pairs of mutation m on every launch form of the case"""
    c = bd.c
    forms = [(64, False), (128, False)] + ([(32, True), (64, True)] if c.wino else [])
    if m == "count_overhang":
        forms = [f for f in forms if f[1]]
    if m in ("n_minus_1", "seg0_rows"):
        part = bd.bnb(64)[1] if c.mode == "dg" else bd.stat(64)
        S, SS = part[:, 0].sum(0), part[:, 1].sum(0)
        n0, n1 = B.finalize_n(bd.D), B.finalize_n(bd.D, m)
        if c.mode == "dg":
            return [(B.finalize_bwd(S, SS, n0, 0, bd.dg0, bd.db0)["coef"], B.finalize_bwd(S, SS, n1, 0, bd.dg0, bd.db0)["coef"])]
        a, b = B.finalize_fwd(S, SS, n0, bd.rm0, bd.rv0), B.finalize_fwd(S, SS, n1, bd.rm0, bd.rv0)
        return [(torch.stack([B.f32(a[k]) for k in ("mean", "rvar")]), torch.stack([B.f32(b[k]) for k in ("mean", "rvar")]))]
    if c.mode == "dg":
        return [(bd.bnb(t, w)[1], bd.bnb(t, w, mutate=m)[1]) for t, w in forms]
    return [(bd.stat(t, w), bd.stat(t, w, mutate=m)) for t, w in forms]


@pytest.mark.parametrize("name", [n for n in NAMES if B.CASE[n].covers])
def test_mutations_are_detected(name):
    bd = B.data(name)
    for m in bd.c.covers:
        pairs = _mutants(bd, m)
        assert pairs, m
        for true, mut in pairs:
            assert true.shape != mut.shape or not torch.equal(torch.nan_to_num(true, nan=-1.0), torch.nan_to_num(mut, nan=-2.0)), f"{name}: mutation {m} goes unnoticed"


def test_every_mutation_and_edge_has_a_case():
    for m in B.MUTATIONS:
        assert any(m in c.covers for c in B.CASES), m
    for c in B.CASES:
        assert set(c.covers) <= set(B.MUTATIONS)
        if c.mode == "dg" and c.name not in BIG:
            assert {"shift_bit", "ignore_add", "drop_last_row", "skip_last_group"} <= set(c.covers), c.name
        if c.wino and any(h % 2 or w % 2 for h, w in c.sizes):
            assert "count_overhang" in c.covers, c.name
        if len(c.sizes) > 1 or (c.mode == "dg" and c.s > 1):
            assert "seg0_rows" in c.covers and len({g.rows_y * g.rows_x for g in c.desc().segs}) > 1, c.name
    rows = lambda c: B.total_rows(c.desc())
    assert {rows(B.CASE[n]) for n in ("d_m1", "d_m65", "d_m722")} == {1, 65, 722}
    assert rows(B.CASE["d_r128"]) == 128 * 64 and rows(B.CASE["d_r129"]) == 129 * 64 and rows(B.CASE["d_r128b"]) == 128 * 128 and rows(B.CASE["d_r129b"]) == 129 * 128
    assert B.CASE["d_s2"].desc().nseg == 4 and B.CASE["d_pyr"].desc().nseg == 4
