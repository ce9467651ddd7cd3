"""GPU tests of the task-aligned anchor assignment (zsg_match_tal, cfg matcher = "tal") against tests/tal_ref.py, through the raw C ABI
unless stated: the metric against the fp64 reference (relative tal_ref.metric_tolerance(alpha, beta) = alpha e_s + beta e_u, from the
fp32 formats; outside anchors exactly -1), the mask against the selection redone on the host from the kernel's own metric (exact), the
mask against the reference's on the seeded inputs whose gaps tests/test_cpu_tal.py asserts (exact), ties, fewer candidates than topk and
none, the NaN rule, the limits, determinism, ZSGLoss(matcher="tal") against the raw chain (bit for bit) and against the fp64 criterion on
the GPU's mask (the bounds of tests/test_gpu_atss.py: loss scalars rel 1e-5, gradients max|gpu - ref| <= 2e-5 max|ref| per tensor), and
the full width (A = 17460).  Run with -rP to see the measured distances (profiles/tal_parity_measured.txt)."""
import numpy as np
import pytest
import torch

import atss_ref as T
import tal_ref as R

pytestmark = pytest.mark.gpu

from oracle import zsg_oracle as O  # noqa: E402

GRAD_TOL, LOSS_RTOL = 2e-5, 1e-5          # tests/test_gpu_atss.py
VARIANTS = {"plain": dict(), "giou": dict(box_iou_loss="giou"), "qfl": dict(cls_quality="qfl"), "vfl": dict(cls_quality="vfl")}
SCALARS = ("loss", "cls_ls", "box_ls", "iou_ls", "pos_iou")


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib, config, loss
    return _lib, config, loss


def out5_of(att, reg):
    return torch.cat([torch.from_numpy(reg), torch.from_numpy(att)[..., None]], dim=2).cuda().contiguous()


def raw_match(M, att, reg, annot, anc, k, alpha=1.0, beta=6.0, B=None, short_ws=0, want_metric=True):
    """zsg_match_tal -> (rc, pos_mask [B, A] uint8 pre-filled with 0xFF, metric [B, A] float64 pre-filled with -7) as numpy"""
    lib = M[0].lib
    B0, A = att.shape
    o5, bx, an = out5_of(att, reg), torch.from_numpy(annot).cuda(), torch.from_numpy(anc).cuda()
    mask = torch.full((B0, A), 0xFF, dtype=torch.uint8, device="cuda")
    metric = torch.full((B0, A), -7.0, dtype=torch.float64, device="cuda")
    wsb = lib.zsg_match_tal_workspace_bytes(B0, A)
    assert wsb == B0 * A * 8
    ws = torch.empty(B0 * A, dtype=torch.float64, device="cuda")
    rc = lib.zsg_match_tal(o5.data_ptr(), bx.data_ptr(), an.data_ptr(), B0 if B is None else B, A, k, alpha, beta, mask.data_ptr(),
                           metric.data_ptr() if want_metric else None, ws.data_ptr(), wsb - short_ws, M[0].stream_ptr())
    torch.cuda.synchronize()
    return rc, mask.cpu().numpy(), metric.cpu().numpy()


def raw_loss_m(M, att, reg, annot, anc, mask, iou_kind=0, cls_kind=0, lamb_iou=1.0):
    """zsg_loss_fwd_bwd_m with the default criterion -> (rc, losses [5], grad5, match_idx, npos) as numpy"""
    lib = M[0].lib
    B, A = att.shape
    o5, bx, an = out5_of(att, reg), torch.from_numpy(annot).cuda(), torch.from_numpy(anc).cuda()
    pm = torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)).cuda()
    losses, grad = torch.full((5,), -7.0, device="cuda"), torch.full_like(o5, -7.0)
    midx, npos = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    wsb = lib.zsg_loss_workspace_bytes(B, A)
    ws = torch.empty((wsb + 7) // 8, dtype=torch.float64, device="cuda")
    rc = lib.zsg_loss_fwd_bwd_m(o5.data_ptr(), bx.data_ptr(), an.data_ptr(), B, A, 0.25, 2.0, 1.0, 0.6, 3, 1.0, iou_kind, lamb_iou, cls_kind,
                                pm.data_ptr(), losses.data_ptr(), grad.data_ptr(), midx.data_ptr(), npos.data_ptr(), ws.data_ptr(), wsb,
                                M[0].stream_ptr())
    torch.cuda.synchronize()
    return rc, losses.cpu().numpy(), grad.cpu().numpy(), midx.cpu().numpy(), npos.cpu().numpy()


def run(M, att, reg, annot, anc, **cfg_kw):
    """ZSGLoss on the GPU -> (losses dict of floats, grad [B, A, 5] numpy, match_idx, npos, the loss module)"""
    _, config, loss = M
    cfg = config.get_cfg(**cfg_kw)
    r, s = config.ratios_scales(cfg)
    lf = loss.get_default_loss(r, s, cfg)
    lf.anchs = torch.from_numpy(anc).cuda()
    out5 = out5_of(att, reg).requires_grad_()
    ls = lf(dict(att_bbx_out=out5, feat_sizes=None, num_f_out=torch.tensor([1])), dict(annot=torch.from_numpy(annot).cuda()))
    assert list(ls) == lf.loss_keys
    ls["loss"].backward()
    return ({k: float(v) for k, v in ls.items()}, out5.grad.cpu().numpy(), lf.match_idx.cpu().numpy(), lf.npos.cpu().numpy(), lf)


def host_selection(metric, k):
    """the selection redone from the metric array alone: key order t descending then index ascending, t > 0"""
    mask = np.zeros(metric.shape, np.uint8)
    for b in range(metric.shape[0]):
        mask[b, R.select(metric[b], k)[1]] = 1
    return mask


def metric_distance(metric, ref):
    """(max relative distance over the inside anchors with a positive reference t, all the structural checks asserted)"""
    ins = ref["inside"]
    assert np.all(metric[~ins] == -1.0)                          # exactly -1 outside
    want = ref["metric"]
    pos = ins & (want > 0)
    assert np.array_equal(ins & (metric > 0), pos) and np.all(metric[ins & (want == 0)] == 0.0)
    assert np.array_equal(np.isnan(metric), np.isnan(want))
    return float(np.abs(metric[pos] / want[pos] - 1.0).max()) if pos.any() else 0.0


def all_inputs(name, B):
    """the "trained" inputs (exact masks) and the "wild" ones of tests/atss_ref.py (IoUs of every size)"""
    att, reg, annot, anc, _ = T.inputs(O, name, B)
    return {"trained": R.inputs(O, name, B), "wild": (att, reg, annot, anc)}


# ---- 1 / 2 / 3: the metric, the selection on the kernel's own bits, the selection against the reference -----------------------------
@pytest.mark.parametrize("name,B", R.CASES)
def test_metric_parity_and_exact_selection(M, name, B):
    for kind, (att, reg, annot, anc) in all_inputs(name, B).items():
        for k in R.TOPKS:
            for alpha, beta in R.EXPONENTS:
                ref = R.matched(O, name, B, k, alpha, beta) if kind == "trained" else R.tal_match(att, reg, annot, anc, k, alpha, beta)
                rc, mask, metric = raw_match(M, att, reg, annot, anc, k, alpha, beta)
                assert rc == 0
                tol = R.metric_tolerance(alpha, beta)
                d = metric_distance(metric, ref)
                print(f"{name} B={B} {kind} k={k} alpha={alpha} beta={beta}: max rel |t - ref| {d:.3g} (tolerance {tol:.3g}); "
                      f"positives {mask.sum(1).tolist()}")
                assert d <= tol
                assert set(np.unique(mask).tolist()) <= {0, 1}   # every byte of the 0xFF pre-fill was written
                assert np.array_equal(mask, host_selection(metric, k))
                if kind == "trained":
                    assert np.array_equal(mask.astype(bool), ref["mask"])
                assert np.array_equal(mask.sum(1), [min(k, len(c)) for c in ref["order"]])
    # without the optional output: the same mask
    att, reg, annot, anc = R.inputs(O, name, B)
    a, b = raw_match(M, att, reg, annot, anc, 13), raw_match(M, att, reg, annot, anc, 13, want_metric=False)
    assert a[0] == 0 and b[0] == 0 and np.array_equal(a[1], b[1]) and np.all(b[2] == -7.0)


@pytest.mark.parametrize("name,B", R.CASES)
def test_the_two_factors_alone_keep_their_bounds(M, name, B):
    """alpha = 1, beta = 0 makes t the score s; alpha = 0, beta = 1 makes it the IoU u: e_s and e_u themselves, measured on the device"""
    for kind, (att, reg, annot, anc) in all_inputs(name, B).items():
        for what, alpha, beta, bound in (("s", 1.0, 0.0, R.E_S), ("u", 0.0, 1.0, R.E_U)):
            ref = R.tal_match(att, reg, annot, anc, 13, alpha, beta)
            rc, mask, metric = raw_match(M, att, reg, annot, anc, 13, alpha, beta)
            assert rc == 0
            d = metric_distance(metric, ref)
            print(f"{name} B={B} {kind}: max rel |{what} - ref| {d:.3g} (e_{what} {bound:.3g})")
            assert d <= bound and np.array_equal(mask, host_selection(metric, 13))


# ---- 4: ties ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(T.PYRAMIDS))
def test_ties_go_to_the_lower_index(M, name):
    att, reg, annot, anc = R.inputs(O, name, 3)
    same = np.full_like(att, -0.75)
    for k in (4, 13, 32):
        rc, mask, metric = raw_match(M, same, reg, annot, anc, k, 1.0, 0.0)
        assert rc == 0
        for b in range(3):
            ins = np.nonzero(R.inside_mask(annot[b], anc))[0]
            assert len(ins) > k and len(np.unique(metric[b, ins])) == 1 and metric[b, ins[0]] > 0
            assert np.nonzero(mask[b])[0].tolist() == ins[:k].tolist()


# ---- 5: fewer candidates than topk, and none ------------------------------------------------------------------------------------------
def test_fewer_candidates_than_topk_and_none(M):
    att, reg, _, anc = R.inputs(O, "P126", 1)
    acy, acx = T.centres(anc)
    # a box round the centre of one cell of the finest level: the 9 anchors of that cell and nothing else
    cy, cx = float(acy[0]), float(acx[0])
    annot = np.array([[cy - 0.05, cx - 0.05, cy + 0.05, cx + 0.05]], np.float32)
    ins = np.nonzero(R.inside_mask(annot[0], anc))[0]
    assert 0 < len(ins) < 13
    zero = np.zeros_like(reg)                                    # (the anchors themselves: every inside anchor overlaps the box)
    ref = R.tal_match(att, zero, annot, anc, 13, 1.0, 6.0)
    rc, mask, metric = raw_match(M, att, zero, annot, anc, 13)
    assert rc == 0 and np.array_equal(mask.astype(bool), ref["mask"]) and mask.sum() == len(ref["order"][0]) == len(ins)
    assert np.all(metric[0, ins] > 0)
    # one of them decodes to a box that misses the annotation: t = 0 there, inside but no candidate
    zero[0, ins[1], 0] = 40.0
    rc, mask, metric = raw_match(M, att, zero, annot, anc, 13)
    assert rc == 0 and metric[0, ins[1]] == 0.0 and mask.sum() == len(ins) - 1 and mask[0, ins[1]] == 0
    # a box between anchor centres: no candidate, an all-zero mask, and the loss keeps the arg-max anchor alone
    annot = np.array([[0.2, 0.2, 0.3, 0.3]], np.float32)
    assert not R.inside_mask(annot[0], anc).any()
    rc, mask, metric = raw_match(M, att, reg, annot, anc, 13)
    assert rc == 0 and not mask.any() and np.all(metric == -1.0)
    best = R.with_best(mask, annot, anc)[1]
    rc, losses, grad, midx, npos = raw_loss_m(M, att, reg, annot, anc, mask)
    assert rc == 0 and npos.tolist() == [1] and midx.tolist() == [int(best[0])] and np.isfinite(losses).all()
    got, _, midx, npos, lf = run(M, att, reg, annot, anc, matcher="tal")
    assert npos.tolist() == [1] and midx.tolist() == [int(best[0])] and not lf.pos_mask.any()


# ---- 6: the NaN rule ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [6.0, 0.0])
def test_nan_rows_are_never_selected(M, beta):
    att, reg, annot, anc = R.inputs(O, "P189", 3)
    ref = R.matched(O, "P189", 3, 13, 1.0, 6.0)
    att, reg = att.copy(), reg.copy()
    hit = []
    for b in range(3):                                           # the two best anchors of every sample: one NaN score, one NaN regression value
        a0, a1 = ref["order"][b][:2]
        att[b, a0] = np.nan
        reg[b, a1, b] = np.nan
        hit.append((a0, a1))
    want = R.tal_match(att, reg, annot, anc, 13, 1.0, beta)
    rc, mask, metric = raw_match(M, att, reg, annot, anc, 13, 1.0, beta)
    assert rc == 0 and np.array_equal(mask, host_selection(metric, 13))
    for b, (a0, a1) in enumerate(hit):
        assert np.isnan(metric[b, a0]) and np.isnan(metric[b, a1]) and mask[b, a0] == 0 and mask[b, a1] == 0
    assert np.array_equal(np.isnan(metric), np.isnan(want["metric"])) and mask.sum(1).tolist() == [min(13, len(c)) for c in want["order"]]


@pytest.mark.parametrize("beta", [6.0, 0.0])
def test_decodes_that_overflow_are_never_selected(M, beta):
    """inputs without a NaN whose decoded box is not finite: an infinite size gives u = 0, an infinite centre gives inf - inf, a NaN u and
    a NaN t whatever beta is"""
    att, reg, annot, anc = R.inputs(O, "P189", 3)
    ref = R.matched(O, "P189", 3, 13, 1.0, 6.0)
    reg = reg.copy()
    rows = []
    for b in range(3):
        a0, a1, a2 = ref["order"][b][:3]
        reg[b, a0, 2 + b % 2] = 1000.0                           # exp overflows
        reg[b, a1, b % 2] = np.inf                               # the centre at infinity
        reg[b, a2, 0], reg[b, a2, 2] = -np.inf, 1000.0           # both
        rows.append((a0, a1, a2))
    with np.errstate(all="ignore"):
        want = R.tal_match(att, reg, annot, anc, 13, 1.0, beta)
    rc, mask, metric = raw_match(M, att, reg, annot, anc, 13, 1.0, beta)
    assert rc == 0 and np.array_equal(mask, host_selection(metric, 13))
    assert np.array_equal(np.isnan(metric), np.isnan(want["metric"])) and np.array_equal(metric == 0, want["metric"] == 0)
    for b, (a0, a1, a2) in enumerate(rows):
        assert metric[b, a0] == (0.0 if beta else want["metric"][b, a0]) or abs(metric[b, a0] / want["metric"][b, a0] - 1) <= R.E_S
        assert np.isnan(metric[b, a1]) and np.isnan(metric[b, a2]) and mask[b, a1] == 0 and mask[b, a2] == 0
        assert mask[b, a0] == 0 or not beta
    assert mask.sum(1).tolist() == [min(13, len(c)) for c in want["order"]]


@pytest.mark.parametrize("variant", ["plain", "qfl"])
def test_a_sample_that_is_nan_everywhere_gives_an_empty_mask_and_the_loss_its_constants(M, variant):
    att, reg, annot, anc = R.inputs(O, "P189", 3)
    att, reg = att.copy(), reg.copy()
    att[1], reg[1] = np.nan, np.nan
    rc, mask, metric = raw_match(M, att, reg, annot, anc, 13)
    assert rc == 0 and not mask[1].any() and mask[0].sum() == 13 and mask[2].sum() > 0
    ins = R.inside_mask(annot[1], anc)
    assert np.all(np.isnan(metric[1, ins])) and np.all(metric[1, ~ins] == -1.0)
    got, grad, _, npos, lf = run(M, att, reg, annot, anc, matcher="tal", **VARIANTS[variant])
    assert got["cls_ls"] == 1.0 and got["box_ls"] == np.float32(0.01) and got.get("pos_iou", 0.0) == 0.0, got
    np.testing.assert_allclose(got["loss"], 1.01, rtol=1e-6)
    assert np.all(grad == 0) and npos.tolist()[1] == 1 and np.array_equal(lf.pos_mask.cpu().numpy(), mask)


# ---- 7: the limits ------------------------------------------------------------------------------------------------------------------------
def test_limits_are_rejected_before_anything_is_launched(M):
    lib = M[0].lib
    att, reg, annot, anc = R.inputs(O, "P126", 3)

    def refused(word, **kw):
        rc, mask, metric = raw_match(M, att, reg, annot, anc, **{**dict(k=13), **kw})
        assert rc == -1 and word in lib.zsg_last_error(), (kw, rc, lib.zsg_last_error())
        assert np.all(mask == 0xFF) and np.all(metric == -7.0)

    refused(b"topk=0", k=0)
    refused(b"topk=33", k=33)
    refused(b"B=513", B=513)
    refused(b"alpha=", alpha=-1.0)
    refused(b"beta=", beta=-0.25)
    refused(b"alpha=", alpha=float("nan"))
    refused(b"beta=", beta=float("nan"))
    refused(b"alpha=", alpha=float("inf"))
    refused(b"ws_bytes=", short_ws=1)
    rc, mask, _ = raw_match(M, att, reg, annot, anc, 32, 0.0, 0.0)
    assert rc == 0 and mask.sum(1).tolist() == [32, 32, 32]
    big = [np.ascontiguousarray(np.resize(x, (512,) + x.shape[1:])) for x in (att, reg, annot)]
    rc, mask, _ = raw_match(M, big[0], big[1], big[2], anc, 13)
    assert rc == 0 and np.array_equal(mask[:3].astype(bool), R.matched(O, "P126", 3, 13, 1.0, 6.0)["mask"]) and np.array_equal(mask[3:6], mask[:3])


# ---- 8: determinism -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["P126", "P261"])
def test_two_runs_are_bit_identical(M, name):
    att, reg, annot, anc, _ = T.inputs(O, name, 3)
    a, b = raw_match(M, att, reg, annot, anc, 13), raw_match(M, att, reg, annot, anc, 13)
    assert a[0] == 0 and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.int64), b[2].view(np.int64))
    kw = dict(matcher="tal", cls_quality="qfl", box_iou_loss="giou")
    x, y = run(M, att, reg, annot, anc, **kw), run(M, att, reg, annot, anc, **kw)
    assert x[0] == y[0] and np.array_equal(x[1].view(np.int32), y[1].view(np.int32))
    assert torch.equal(x[4].pos_mask, y[4].pos_mask) and torch.equal(x[4].tal_metric.view(torch.int64), y[4].tal_metric.view(torch.int64))


# ---- 9: through ZSGLoss -------------------------------------------------------------------------------------------------------------------
def check(tag, got, grad, ref):
    got = dict(got)
    got.setdefault("iou_ls", 0.0)
    got.setdefault("pos_iou", ref["pos_iou"])
    dist = {}
    for name, g, r in (("cls", grad[..., 4], ref["g_att"]), ("box", grad[..., :4], ref["g_reg"])):
        scale = np.abs(r).max()
        dist[name] = (np.abs(g - r).max(), scale)
        print(f"{tag} {name} gradient: max|gpu - ref| / max|ref| = {dist[name][0] / scale:.3g}  (max|ref| {scale:.4g})")
    for k in SCALARS:
        print(f"{tag} {k}: gpu {got[k]:.8g} ref {ref[k]:.8g}")
        np.testing.assert_allclose(got[k], ref[k], rtol=LOSS_RTOL, err_msg=f"{tag} {k}")
    for name, (d, scale) in dist.items():
        assert scale > 0 and d <= GRAD_TOL * scale, f"{tag}: {name} gradient off by {d / scale:.3g} of max|ref|"
    assert np.all(grad[..., :4][~ref["mask"]] == 0), f"{tag}: a negative anchor got a box gradient"


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name,B", R.CASES)
def test_zsgloss_is_the_raw_chain_and_the_fp64_criterion_on_its_mask(M, name, B, variant):
    att, reg, annot, anc = R.inputs(O, name, B)
    kw = VARIANTS[variant]
    iou_kind = {"none": 0, "giou": 1}[kw.get("box_iou_loss", "none")]
    cls_kind = {"none": 0, "qfl": 1, "vfl": 2}[kw.get("cls_quality", "none")]
    for k, (alpha, beta) in ((13, (1.0, 6.0)), (4, (0.5, 2.0))):
        got, grad, midx, npos, lf = run(M, att, reg, annot, anc, matcher="tal", tal_topk=k, tal_alpha=alpha, tal_beta=beta, **kw)
        assert ("iou_ls" in got) == ("box_iou_loss" in kw) and ("pos_iou" in got) == ("cls_quality" in kw)
        rc, mask, metric = raw_match(M, att, reg, annot, anc, k, alpha, beta)
        rc2, losses, g, mi, n = raw_loss_m(M, att, reg, annot, anc, mask, iou_kind=iou_kind, cls_kind=cls_kind)
        assert rc == 0 and rc2 == 0
        assert np.array_equal(lf.pos_mask.cpu().numpy(), mask)
        assert np.array_equal(lf.tal_metric.cpu().numpy().view(np.int64), metric.view(np.int64))
        assert np.array_equal(lf._last_losses.cpu().numpy().view(np.int32), losses.view(np.int32))
        assert np.array_equal(grad.view(np.int32), g.view(np.int32)) and np.array_equal(midx, mi) and np.array_equal(npos, n)
        full, best = R.with_best(mask, annot, anc)
        assert np.array_equal(midx, best.astype(np.int32)) and np.array_equal(npos, full.sum(1).astype(np.int32))
        ref = T.compose(att, reg, annot, anc, full, best, kind=kw.get("cls_quality", "none"), box_iou=kw.get("box_iou_loss", "none"))
        check(f"tal {variant} {name} B={B} k={k}", got, grad, ref)
        assert np.abs(grad[..., :4][full]).max() > 0
    # the keys of the other matchers are not read
    other = run(M, att, reg, annot, anc, matcher="tal", tal_topk=4, tal_alpha=0.5, tal_beta=2.0, matching_threshold=0.9, atss_topk=3, **kw)
    assert other[0] == got and np.array_equal(other[1].view(np.int32), grad.view(np.int32))


def test_lamb_reg_zero_trains_on_the_iou_term_alone(M):
    att, reg, annot, anc = R.inputs(O, "P261", 3)
    got, grad, _, npos, lf = run(M, att, reg, annot, anc, matcher="tal", box_iou_loss="giou", cls_quality="qfl", lamb_reg=0)
    np.testing.assert_allclose(got["loss"], got["iou_ls"] + got["cls_ls"], rtol=1e-6)
    assert np.isfinite(grad).all() and np.abs(grad[..., :4]).max() > 0 and npos.min() >= 13


# ---- 10: the full width ---------------------------------------------------------------------------------------------------------------------
def test_full_width(M):
    """A = 17460 (the 300 x 300 network's six levels), B = 2, topk = 13"""
    att, reg, annot, anc = R.inputs(O, "full", 2)
    assert anc.shape == (17460, 4)
    ref = R.matched(O, "full", 2, 13, 1.0, 6.0)
    rc, mask, metric = raw_match(M, att, reg, annot, anc, 13)
    assert rc == 0
    d = metric_distance(metric, ref)
    print(f"full B=2 k=13: positives per sample {mask.sum(1).tolist()}, candidates {[len(c) for c in ref['order']]}, "
          f"max rel |t - ref| {d:.3g} (tolerance {R.metric_tolerance(1.0, 6.0):.3g})")
    assert d <= R.metric_tolerance(1.0, 6.0)
    assert set(np.unique(mask).tolist()) <= {0, 1}
    assert np.array_equal(mask, host_selection(metric, 13))
    assert np.array_equal(mask.astype(bool), ref["mask"]) and mask.sum(1).tolist() == [13, 13]
