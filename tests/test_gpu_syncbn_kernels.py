"""Synchronized-BatchNorm kernels (zsg_bn_sync_*) with two ranks emulated in one process: each half of a batch reduces its rank-local
fp64 sums, the host adds the two halves' sums (the all-reduce), and the finalize / apply launches restart from the global sums.  Checked
against fp64 torch over the concatenated batch: mean / invstd / running statistics against F.batch_norm(training=True), dx against
autograd, each half's d(gamma) / d(beta) against that half's own autograd sums (torch's SyncBatchNorm returns the rank-local ones), the
stem pair against bn -> relu -> maxpool autograd.  Inputs come from x and from the partial rows of real zsg_conv_igemm /
zsg_conv_igemm_bnb launches; with one rank the results equal the unsynchronized kernels' bit for bit, and two runs are bit-identical."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from test_gpu_ops import Z, dev, nhwc, ohwi, view_of  # noqa: F401

pytestmark = pytest.mark.gpu


def _ws(L, rows, Cc):
    return torch.zeros(int(L.lib.zsg_bn_workspace_bytes(rows, Cc)) // 4 + 64, device="cuda")


def _fwd_sums(L, x=None, rows=0, Cc=0, part=None, chunks=0):
    s = torch.full((2 * Cc + 1,), float("nan"), dtype=torch.float64, device="cuda")
    ws = _ws(L, rows, Cc) if part is None else None
    L.check(L.lib.zsg_bn_sync_fwd_sums(x.data_ptr() if x is not None else None, rows, Cc, part.data_ptr() if part is not None else None,
                                       chunks, s.data_ptr(), ws.data_ptr() if ws is not None else None, ws.numel() * 4 if ws is not None else 0,
                                       L.stream_ptr()), "bn_sync_fwd_sums")
    return s


def _finalize(L, s, Cc, rm=None, rv=None):
    mean, invstd = torch.empty(Cc, device="cuda"), torch.empty(Cc, device="cuda")
    L.check(L.lib.zsg_bn_sync_fwd_finalize(s.data_ptr(), Cc, mean.data_ptr(), invstd.data_ptr(), rm.data_ptr() if rm is not None else None,
                                           rv.data_ptr() if rv is not None else None, 0.1, 1e-5, L.stream_ptr()), "bn_sync_fwd_finalize")
    return mean, invstd


def _pack_bits(bits):
    bb = bits.reshape(-1, 4).to(torch.uint8)
    return dev((bb[:, 0] | (bb[:, 1] << 1) | (bb[:, 2] << 2) | (bb[:, 3] << 3)).contiguous())


def _ref_stats(xcat, rm0, rv0):
    """fp64 F.batch_norm(training=True) over the concatenated batch [N, C]: mean, invstd, running statistics after one update"""
    xd = xcat.double()
    rm, rv = rm0.double().clone(), rv0.double().clone()
    F.batch_norm(xd[:, :, None], rm, rv, training=True, momentum=0.1, eps=1e-5)
    m, v = xd.mean(0), xd.var(0, unbiased=False)
    return m, 1.0 / torch.sqrt(v + 1e-5), rm, rv


@pytest.mark.parametrize("Cc,ra,rb", [(64, 2 * 19 * 19, 1 * 19 * 19), (256, 3 * 10 * 10, 5 * 10 * 10), (32, 4 * 75 * 75, 4 * 75 * 75)])
def test_forward_stats_from_x(Z, Cc, ra, rb):
    L, ops = Z
    g = torch.Generator().manual_seed(Cc + ra)
    xa, xb = torch.randn(ra, Cc, generator=g) * 1.7 + 0.4, torch.randn(rb, Cc, generator=g) * 0.6 - 1.1
    rm0, rv0 = torch.randn(Cc, generator=g) * 0.1, torch.rand(Cc, generator=g) + 0.5
    sa, sb = _fwd_sums(L, dev(xa), ra, Cc), _fwd_sums(L, dev(xb), rb, Cc)
    assert float(sa[2 * Cc]) == ra and float(sb[2 * Cc]) == rb
    s = sa + sb                                                  # the all-reduce of two ranks
    rm, rv = dev(rm0), dev(rv0)
    mean, invstd = _finalize(L, s, Cc, rm, rv)
    m_ref, is_ref, rm_ref, rv_ref = _ref_stats(torch.cat([xa, xb]), rm0, rv0)
    assert float((mean.double().cpu() - m_ref).abs().max()) < 1e-6 * (1 + float(m_ref.abs().max()))
    assert float(((invstd.double().cpu() - is_ref) / is_ref).abs().max()) < 1e-6
    assert float((rm.double().cpu() - rm_ref).abs().max()) < 1e-6
    assert float(((rv.double().cpu() - rv_ref) / rv_ref).abs().max()) < 1e-6       # unbiased variance, N = ra + rb
    # one rank: the unsynchronized kernel's mean / invstd / running statistics, bit for bit
    x1 = dev(xa)
    m1, i1 = _finalize(L, _fwd_sums(L, x1, ra, Cc), Cc)
    m0, i0 = torch.empty(Cc, device="cuda"), torch.empty(Cc, device="cuda")
    ws = _ws(L, ra, Cc)
    L.check(L.lib.zsg_bn_stats(x1.data_ptr(), ra, Cc, m0.data_ptr(), i0.data_ptr(), None, None, 0.1, 1e-5, ws.data_ptr(), ws.numel() * 4,
                               L.stream_ptr()), "bn_stats")
    assert torch.equal(m0, m1) and torch.equal(i0, i1)


def test_forward_stats_from_conv_partial_rows(Z):
    """the statistics of a convolution's output from its epilogue's partial rows (zsg_conv_igemm, two 'ranks' of 2 and 3 images)"""
    L, ops = Z
    Ci, Co, H, W = 64, 128, 19, 19
    g = torch.Generator().manual_seed(7)
    w = torch.randn(Co, Ci, 1, 1, generator=g) / Ci ** 0.5
    wd = dev(ohwi(w))
    st = L.stream_ptr()
    ys, sums = [], []
    for B in (2, 3):
        x = torch.randn(B, Ci, H, W, generator=g) + 0.3
        xd, y = dev(nhwc(x)), torch.empty(B, H, W, Co, device="cuda")
        d = ops.fwd_desc(view_of(ops, xd, B, H, W, Ci), view_of(ops, y, B, H, W, Co), Ci, Co, 1, 1, 0, 1, wC=Ci,
                         tile_hint=ops.tile_hint(64, 64, 1))
        chunks = int(L.lib.zsg_conv_igemm_partial_rows(C.byref(d)))
        part = torch.full((chunks, 2, Co), float("nan"), device="cuda")
        L.check(L.lib.zsg_conv_igemm(C.byref(d), xd.data_ptr(), wd.data_ptr(), y.data_ptr(), None, None, None, part.data_ptr(), st), "conv")
        s = _fwd_sums(L, part=part, rows=B * H * W, Cc=Co, chunks=chunks)
        if B == 2:           # one rank: zsg_bn_stats_from_partials's mean / invstd, bit for bit
            m1, i1 = _finalize(L, s, Co)
            m0, i0 = torch.empty(Co, device="cuda"), torch.empty(Co, device="cuda")
            L.check(L.lib.zsg_bn_stats_from_partials(part.data_ptr(), chunks, B * H * W, Co, m0.data_ptr(), i0.data_ptr(), None, None, 0.1,
                                                     1e-5, st), "bn_stats_from_partials")
            assert torch.equal(m0, m1) and torch.equal(i0, i1)
        ys.append(y.reshape(-1, Co).cpu())
        sums.append(s)
    mean, invstd = _finalize(L, sums[0] + sums[1], Co)
    m_ref, is_ref, _, _ = _ref_stats(torch.cat(ys), torch.zeros(Co), torch.ones(Co))
    assert float((mean.double().cpu() - m_ref).abs().max()) < 1e-5 * (1 + float(m_ref.abs().max()))
    assert float(((invstd.double().cpu() - is_ref) / is_ref).abs().max()) < 1e-5


def _bwd_reference(xcat, doutcat, bitscat, gamma, splits):
    """fp64 autograd of sum(dout * bits * bn(x)) over the concatenated batch [N, C]: dx, and d(gamma) / d(beta) per split"""
    x = xcat.double().requires_grad_(True)
    gam = gamma.double()
    m, v = x.mean(0), x.var(0, unbiased=False)
    xh = (x - m) / torch.sqrt(v + 1e-5)
    gm = doutcat.double() * (bitscat.double() if bitscat is not None else 1.0)
    (gm * (xh * gam)).sum().backward()
    xh = xh.detach()
    per = [(gm[a:b] * xh[a:b]).sum(0) for a, b in splits], [gm[a:b].sum(0) for a, b in splits]
    return x.grad, per


@pytest.mark.parametrize("use_mask", [True, False])
def test_backward_from_x(Z, use_mask):
    L, ops = Z
    Cc, ra, rb = 128, 2 * 10 * 13, 1 * 10 * 13
    g = torch.Generator().manual_seed(11 + use_mask)
    x = torch.randn(ra + rb, Cc, generator=g) * 1.3 + 0.2
    dout = torch.randn(ra + rb, Cc, generator=g)
    bits = (torch.rand(ra + rb, Cc, generator=g) > 0.4) if use_mask else None
    gamma = torch.rand(Cc, generator=g) + 0.5
    st = L.stream_ptr()

    def run():
        halves = [(0, ra), (ra, ra + rb)]
        fs = [_fwd_sums(L, dev(x[a:b]), b - a, Cc) for a, b in halves]
        fsum = fs[0] + fs[1]
        mean, invstd = _finalize(L, fsum, Cc)
        bs, dgs, dbs, dxs = [], [], [], []
        for a, b in halves:
            xd, dd = dev(x[a:b]), dev(dout[a:b])
            mk = _pack_bits(bits[a:b]) if use_mask else None
            s = torch.full((2 * Cc,), float("nan"), dtype=torch.float64, device="cuda")
            dg, db = torch.ones(Cc, device="cuda"), torch.full((Cc,), 2.0, device="cuda")      # accumulate onto what is there
            ws = _ws(L, b - a, Cc)
            L.check(L.lib.zsg_bn_sync_bwd_sums(dd.data_ptr(), mk.data_ptr() if mk is not None else None, xd.data_ptr(), b - a, Cc,
                                               mean.data_ptr(), invstd.data_ptr(), None, 0, s.data_ptr(), dg.data_ptr(), db.data_ptr(), 1,
                                               ws.data_ptr(), ws.numel() * 4, st), "bn_sync_bwd_sums")
            bs.append(s)
            dgs.append(dg - 1)
            dbs.append(db - 2)
        bsum = bs[0] + bs[1]
        for a, b in halves:
            xd, dd = dev(x[a:b]), dev(dout[a:b])
            mk = _pack_bits(bits[a:b]) if use_mask else None
            dx, go = torch.full((b - a, Cc), float("nan"), device="cuda"), torch.full((b - a, Cc), float("nan"), device="cuda")
            L.check(L.lib.zsg_bn_sync_bwd_apply(dd.data_ptr(), mk.data_ptr() if mk is not None else None, xd.data_ptr(), b - a, Cc,
                                                mean.data_ptr(), invstd.data_ptr(), dev(gamma).data_ptr(), bsum.data_ptr(), fsum.data_ptr(),
                                                dx.data_ptr(), go.data_ptr(), st), "bn_sync_bwd_apply")
            torch.cuda.synchronize()
            dxs.append((dx.cpu(), go.cpu()))
        return dxs, dgs, dbs

    dxs, dgs, dbs = run()
    dx_ref, (dg_ref, db_ref) = _bwd_reference(x, dout, bits, gamma, [(0, ra), (ra, ra + rb)])
    dx = torch.cat([d for d, _ in dxs]).double()
    assert float((dx - dx_ref).abs().max()) < 2e-4 * float(dx_ref.abs().max())
    gm = dout * (bits.float() if use_mask else 1.0)
    assert torch.equal(torch.cat([go for _, go in dxs]), gm)                     # g_out = the ReLU-masked gradient
    for i in range(2):
        assert float((dgs[i].double().cpu() - dg_ref[i]).abs().max()) < 1e-4 * (1 + float(dg_ref[i].abs().max()))
        assert float((dbs[i].double().cpu() - db_ref[i]).abs().max()) < 1e-4 * (1 + float(db_ref[i].abs().max()))
    dxs2, dgs2, dbs2 = run()                                                     # bit-reproducible
    for (a, _), (b, _) in zip(dxs, dxs2):
        assert torch.equal(a, b)
    assert all(torch.equal(a, b) for a, b in zip(dgs, dgs2)) and all(torch.equal(a, b) for a, b in zip(dbs, dbs2))


def test_backward_from_bnb_partial_rows(Z):
    """the backward sums from the partial rows of a real zsg_conv_igemm_bnb data gradient (a 1x1 convolution's, per 'rank'); with one
    rank the apply equals zsg_bn_backward_from_partials bit for bit"""
    L, ops = Z
    Ci, Co, H, W = 64, 256, 19, 19
    g = torch.Generator().manual_seed(23)
    w = torch.randn(Co, Ci, 1, 1, generator=g) / Ci ** 0.5
    wt = torch.empty((Ci, 1, 1, Co), device="cuda")
    st = L.stream_ptr()
    L.check(L.lib.zsg_transpose_w(dev(ohwi(w)).data_ptr(), wt.data_ptr(), Co, 1, Ci, Co, st), "transpose_w")
    gamma = dev(torch.rand(Ci, generator=g) + 0.5)
    Bs = (2, 1)
    xs = [torch.randn(B, H, W, Ci, generator=g) * 1.5 + 0.3 for B in Bs]
    dys = [torch.randn(B, Co, H, W, generator=g) for B in Bs]
    bits = [torch.rand(B, H, W, Ci, generator=g) > 0.5 for B in Bs]
    fs = [_fwd_sums(L, dev(x.reshape(-1, Ci)), x.numel() // Ci, Ci) for x in xs]
    fsum = fs[0] + fs[1]
    mean, invstd = _finalize(L, fsum, Ci)
    douts, sums, dgs, dbs, parts = [], [], [], [], []
    for B, x, dy, bt in zip(Bs, xs, dys, bits):
        dyd = dev(nhwc(dy))
        dout = torch.empty(B, H, W, Ci, device="cuda")
        d = ops.dgrad_desc(view_of(ops, dyd, B, H, W, Co), view_of(ops, dout, B, H, W, Ci), Co, Ci, 1, 1, 0, 1, tile_hint=ops.tile_hint(64, 64, 1))
        chunks = int(L.lib.zsg_conv_igemm_partial_rows(C.byref(d)))
        part = torch.full((chunks, 2, Ci), float("nan"), device="cuda")
        mk = _pack_bits(bt)
        L.check(L.lib.zsg_conv_igemm_bnb(C.byref(d), dyd.data_ptr(), wt.data_ptr(), dout.data_ptr(), None, dev(x).data_ptr(), mean.data_ptr(),
                                         invstd.data_ptr(), mk.data_ptr(), part.data_ptr(), st), "dgrad + bn sums")
        s = torch.full((2 * Ci,), float("nan"), dtype=torch.float64, device="cuda")
        dg, db = torch.zeros(Ci, device="cuda"), torch.zeros(Ci, device="cuda")
        L.check(L.lib.zsg_bn_sync_bwd_sums(None, None, None, B * H * W, Ci, None, None, part.data_ptr(), chunks, s.data_ptr(), dg.data_ptr(),
                                           db.data_ptr(), 1, None, 0, st), "bn_sync_bwd_sums(partials)")
        douts.append(dout)
        sums.append(s)
        dgs.append(dg)
        dbs.append(db)
        parts.append((part, chunks, mk))
    bsum = sums[0] + sums[1]
    dxs = []
    for B, x, dout, (part, chunks, mk) in zip(Bs, xs, douts, parts):
        dx = torch.empty(B * H * W, Ci, device="cuda")
        L.check(L.lib.zsg_bn_sync_bwd_apply(dout.data_ptr(), mk.data_ptr(), dev(x).data_ptr(), B * H * W, Ci, mean.data_ptr(), invstd.data_ptr(),
                                            gamma.data_ptr(), bsum.data_ptr(), fsum.data_ptr(), dx.data_ptr(), None, st), "bn_sync_bwd_apply")
        dxs.append(dx.cpu())
    xcat = torch.cat([x.reshape(-1, Ci) for x in xs])
    dcat = torch.cat([d.reshape(-1, Ci).cpu() for d in douts])
    bcat = torch.cat([b.reshape(-1, Ci) for b in bits])
    n0 = Bs[0] * H * W
    dx_ref, (dg_ref, db_ref) = _bwd_reference(xcat, dcat, bcat, gamma.cpu(), [(0, n0), (n0, xcat.shape[0])])
    dx = torch.cat(dxs).double()
    assert float((dx - dx_ref).abs().max()) < 2e-4 * float(dx_ref.abs().max())
    for i in range(2):
        assert float((dgs[i].double().cpu() - dg_ref[i]).abs().max()) < 1e-4 * (1 + float(dg_ref[i].abs().max()))
        assert float((dbs[i].double().cpu() - db_ref[i]).abs().max()) < 1e-4 * (1 + float(db_ref[i].abs().max()))
    # one rank, the same partial rows and statistics: zsg_bn_backward_from_partials's dx / d(gamma) / d(beta), bit for bit
    B, x, dout, (part, chunks, mk) = Bs[0], xs[0], douts[0], parts[0]
    rows = B * H * W
    s1 = torch.empty(2 * Ci, dtype=torch.float64, device="cuda")
    dg1, db1 = torch.zeros(Ci, device="cuda"), torch.zeros(Ci, device="cuda")
    L.check(L.lib.zsg_bn_sync_bwd_sums(None, None, None, rows, Ci, None, None, part.data_ptr(), chunks, s1.data_ptr(), dg1.data_ptr(),
                                       db1.data_ptr(), 1, None, 0, st), "bn_sync_bwd_sums(partials)")
    f1 = _fwd_sums(L, dev(x.reshape(-1, Ci)), rows, Ci)
    dx1 = torch.empty(rows, Ci, device="cuda")
    L.check(L.lib.zsg_bn_sync_bwd_apply(dout.data_ptr(), mk.data_ptr(), dev(x).data_ptr(), rows, Ci, mean.data_ptr(), invstd.data_ptr(),
                                        gamma.data_ptr(), s1.data_ptr(), f1.data_ptr(), dx1.data_ptr(), None, st), "bn_sync_bwd_apply")
    dx0, dg0, db0 = torch.empty(rows, Ci, device="cuda"), torch.zeros(Ci, device="cuda"), torch.zeros(Ci, device="cuda")
    ws = torch.zeros(2 * Ci, device="cuda")
    L.check(L.lib.zsg_bn_backward_from_partials(dout.data_ptr(), mk.data_ptr(), dev(x).data_ptr(), rows, Ci, mean.data_ptr(), invstd.data_ptr(),
                                                gamma.data_ptr(), dx0.data_ptr(), None, dg0.data_ptr(), db0.data_ptr(), 1, part.data_ptr(), chunks,
                                                ws.data_ptr(), ws.numel() * 4, st), "bn_backward_from_partials")
    assert torch.equal(dx0, dx1) and torch.equal(dg0, dg1) and torch.equal(db0, db1)


def test_stem_pair(Z):
    """zsg_bn_sync_relu_maxpool_bwd_sums / _apply (two 'ranks' of 2 and 1 images) against fp64 autograd of maxpool(relu(bn(x)), 3, 2, 1)"""
    L, ops = Z
    Cc, H, W = 64, 30, 30
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    g = torch.Generator().manual_seed(5)
    Bs = (2, 1)
    xs = [torch.randn(B, H, W, Cc, generator=g) * 1.2 + 0.1 for B in Bs]
    dps = [torch.randn(B, Ho, Wo, Cc, generator=g) for B in Bs]
    gamma, beta = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.2
    gd, bd = dev(gamma), dev(beta)
    st = L.stream_ptr()

    def run():
        fs = [_fwd_sums(L, dev(x.reshape(-1, Cc)), x.numel() // Cc, Cc) for x in xs]
        fsum = fs[0] + fs[1]
        mean, invstd = _finalize(L, fsum, Cc)
        outs, sums, dgs = [], [], []
        for B, x, dp in zip(Bs, xs, dps):
            xd = dev(x)
            out, idx = torch.empty(B, Ho, Wo, Cc, device="cuda"), torch.empty(B * Ho * Wo * Cc, dtype=torch.uint8, device="cuda")
            L.check(L.lib.zsg_bn_relu_maxpool_fwd(xd.data_ptr(), B, H, W, Cc, mean.data_ptr(), invstd.data_ptr(), gd.data_ptr(), bd.data_ptr(),
                                                  3, 2, 1, Ho, Wo, out.data_ptr(), idx.data_ptr(), st), "bn_relu_maxpool_fwd")
            s = torch.empty(2 * Cc, dtype=torch.float64, device="cuda")
            dg, db = torch.zeros(Cc, device="cuda"), torch.zeros(Cc, device="cuda")
            ws = _ws(L, B * Ho * Wo, Cc)
            L.check(L.lib.zsg_bn_sync_relu_maxpool_bwd_sums(dev(dp).data_ptr(), idx.data_ptr(), xd.data_ptr(), B, H, W, Cc, mean.data_ptr(),
                                                            invstd.data_ptr(), gd.data_ptr(), bd.data_ptr(), 3, 2, 1, Ho, Wo, s.data_ptr(),
                                                            dg.data_ptr(), db.data_ptr(), 1, ws.data_ptr(), ws.numel() * 4, st), "sums")
            outs.append((xd, idx))
            sums.append(s)
            dgs.append((dg.cpu(), db.cpu()))
        bsum = sums[0] + sums[1]
        dxs = []
        for B, (xd, idx), dp in zip(Bs, outs, dps):
            dx = torch.full((B, H, W, Cc), float("nan"), device="cuda")
            L.check(L.lib.zsg_bn_sync_relu_maxpool_bwd_apply(dev(dp).data_ptr(), idx.data_ptr(), xd.data_ptr(), B, H, W, Cc, mean.data_ptr(),
                                                             invstd.data_ptr(), gd.data_ptr(), bd.data_ptr(), 3, 2, 1, Ho, Wo, bsum.data_ptr(),
                                                             fsum.data_ptr(), dx.data_ptr(), st), "apply")
            dxs.append(dx.cpu())
        return dxs, dgs

    dxs, dgs = run()
    x = torch.cat(xs).permute(0, 3, 1, 2).double().requires_grad_(True)
    m, v = x.mean((0, 2, 3), keepdim=True), x.var((0, 2, 3), unbiased=False, keepdim=True)
    xh = (x - m) / torch.sqrt(v + 1e-5)
    y = F.max_pool2d(F.relu(xh * gamma.double()[None, :, None, None] + beta.double()[None, :, None, None]), 3, 2, 1)
    dp = torch.cat(dps).permute(0, 3, 1, 2).double()
    (y * dp).sum().backward()
    dx = torch.cat(dxs).double()
    dx_ref = x.grad.permute(0, 2, 3, 1)
    assert float((dx - dx_ref).abs().max()) < 2e-4 * float(dx_ref.abs().max())
    # d(gamma) / d(beta) per 'rank': that half's own sums
    ga = gamma.double().clone().requires_grad_(True)
    be = beta.double().clone().requires_grad_(True)
    xhd = xh.detach()
    b0 = Bs[0]
    for i, sl in enumerate((slice(0, b0), slice(b0, None))):
        ga.grad = be.grad = None
        yy = F.max_pool2d(F.relu(xhd[sl] * ga[None, :, None, None] + be[None, :, None, None]), 3, 2, 1)
        (yy * dp[sl]).sum().backward()
        assert float((dgs[i][0].double() - ga.grad).abs().max()) < 1e-4 * (1 + float(ga.grad.abs().max()))
        assert float((dgs[i][1].double() - be.grad).abs().max()) < 1e-4 * (1 + float(be.grad.abs().max()))
    dxs2, dgs2 = run()
    assert all(torch.equal(a, b) for a, b in zip(dxs, dxs2))
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(dgs, dgs2))
