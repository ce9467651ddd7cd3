"""GPU tests of the ATSS anchor assignment (zsg_match_atss, zsg_loss_fwd_bwd_m, cfg matcher = "atss") against tests/atss_ref.py: the mask,
the candidates and the thresholds of the raw matcher (exact; thresholds rel 1e-12: an fp64 sum of <= 128 values in [0, 1]), the masked
loss entry against zsg_loss_fwd_bwd_q on the fixed rule's mask (bit for bit), ZSGLoss(matcher="atss") against the fp64 criterion on the
reference's mask (loss scalars rel 1e-5, gradients max|gpu - ref| <= 2e-5 max|ref| per tensor: the bounds of tests/test_gpu_boxiou.py),
and the default configuration against a raw zsg_loss_fwd_bwd call.  Pyramids, seeded inputs and k are those of tests/atss_ref.py, whose
conditions tests/test_cpu_atss.py asserts.  Run with -rP to see the measured distances (profiles/atss_parity_measured.txt)."""
import ctypes

import numpy as np
import pytest
import torch

import atss_ref as T

pytestmark = pytest.mark.gpu

from oracle import zsg_oracle as O  # noqa: E402

GRAD_TOL, LOSS_RTOL = 2e-5, 1e-5
CASES = [(name, B) for name in T.PYRAMIDS for B in T.BATCHES]
VARIANTS = {"focal": dict(), "giou": dict(box_iou_loss="giou"), "qfl_giou": dict(cls_quality="qfl", box_iou_loss="giou"),
            "vfl": dict(cls_quality="vfl")}
SCALARS = ("loss", "cls_ls", "box_ls", "iou_ls", "pos_iou")


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib, config, loss
    return _lib, config, loss


def raw_match(M, annot, anc, off, k, L=None, A=None, B=None):
    """zsg_match_atss -> (rc, pos_mask [B, A] uint8 pre-filled with 0xFF, thr [B], cand [B, 128]) as numpy"""
    lib = M[0].lib
    B0, A0 = annot.shape[0], anc.shape[0]
    bx, an = torch.from_numpy(annot).cuda(), torch.from_numpy(anc).cuda()
    lv = np.ascontiguousarray(off, dtype=np.int32)
    L = len(lv) - 1 if L is None else L
    mask = torch.full((B0, A0), 0xFF, dtype=torch.uint8, device="cuda")
    thr = torch.full((B0,), -7.0, dtype=torch.float64, device="cuda")
    cand = torch.full((B0, T.MAX_CAND), -7, dtype=torch.int32, device="cuda")
    wsb = lib.zsg_match_atss_workspace_bytes(B0, max(1, min(L, 8)))
    ws = torch.empty((wsb + 7) // 8, dtype=torch.float64, device="cuda")
    rc = lib.zsg_match_atss(bx.data_ptr(), an.data_ptr(), lv.ctypes.data_as(ctypes.c_void_p), L, B0 if B is None else B,
                            A0 if A is None else A, k, mask.data_ptr(), thr.data_ptr(), cand.data_ptr(), ws.data_ptr(), wsb,
                            M[0].stream_ptr())
    torch.cuda.synchronize()
    return rc, mask.cpu().numpy(), thr.cpu().numpy(), cand.cpu().numpy()


def raw_loss(M, entry, att, reg, annot, anc, flags, mask=None, scale=1.0, iou_kind=0, cls_kind=0, alpha=0.25, gamma=2.0, lamb_iou=1.5):
    """zsg_loss_fwd_bwd / _q / _m -> (rc, losses, grad5, match_idx, npos) as numpy"""
    lib = M[0].lib
    B, A = att.shape
    out5 = torch.cat([torch.from_numpy(reg), torch.from_numpy(att)[..., None]], dim=2).cuda().contiguous()
    an, bx = torch.from_numpy(anc).cuda(), torch.from_numpy(annot).cuda()
    losses = torch.full((3 if entry == "zsg_loss_fwd_bwd" else 5,), -7.0, device="cuda")
    grad = torch.full_like(out5, -7.0)
    midx, npos = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    wsb = lib.zsg_loss_workspace_bytes(B, A)
    ws = torch.empty((wsb + 7) // 8, dtype=torch.float64, device="cuda")
    head = (out5.data_ptr(), bx.data_ptr(), an.data_ptr(), B, A, alpha, gamma, 1.0, 0.6, flags, scale)
    tail = (losses.data_ptr(), grad.data_ptr(), midx.data_ptr(), npos.data_ptr(), ws.data_ptr(), wsb, M[0].stream_ptr())
    if entry == "zsg_loss_fwd_bwd":
        mid = ()
    elif entry == "zsg_loss_fwd_bwd_q":
        mid = (iou_kind, lamb_iou, cls_kind)
    else:
        pm = torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)).cuda()
        mid = (iou_kind, lamb_iou, cls_kind, pm.data_ptr())
    rc = getattr(lib, entry)(*head, *mid, *tail)
    torch.cuda.synchronize()
    return rc, losses.cpu().numpy(), grad.cpu().numpy(), midx.cpu().numpy(), npos.cpu().numpy()


def run(M, att, reg, annot, anc, feat_sizes, **cfg_kw):
    """ZSGLoss on the GPU -> (losses dict of floats, grad [B, A, 5] numpy, match_idx, npos, the loss module)"""
    _, config, loss = M
    cfg = config.get_cfg(**cfg_kw)
    r, s = config.ratios_scales(cfg)
    lf = loss.get_default_loss(r, s, cfg)
    lf.set_anchors(torch.from_numpy(anc).cuda(), feat_sizes)
    out5 = torch.cat([torch.from_numpy(reg), torch.from_numpy(att)[..., None]], dim=2).cuda().requires_grad_()
    ls = lf(dict(att_bbx_out=out5, feat_sizes=None, num_f_out=torch.tensor([1])), dict(annot=torch.from_numpy(annot).cuda()))
    assert list(ls) == lf.loss_keys
    ls["loss"].backward()
    return ({k: float(v) for k, v in ls.items()}, out5.grad.cpu().numpy(), lf.match_idx.cpu().numpy(), lf.npos.cpu().numpy(), lf)


def feat_sizes(name):
    return O.feat_sizes_for(300, 300) if name == "full" else T.PYRAMIDS[name]


def check(tag, got, grad, ref):
    got = dict(got)
    got.setdefault("iou_ls", 0.0)
    got.setdefault("pos_iou", ref["pos_iou"])
    for k in SCALARS:
        print(f"{tag} {k}: gpu {got[k]:.8g} ref {ref[k]:.8g}")
    dist = {}
    for name, g, r in (("cls", grad[..., 4], ref["g_att"]), ("box", grad[..., :4], ref["g_reg"])):
        scale = np.abs(r).max()
        dist[name] = (np.abs(g - r).max(), scale)
        print(f"{tag} {name} gradient: max|gpu - ref| / max|ref| = {dist[name][0] / scale:.3g}  (max|ref| {scale:.4g})")
    for k in SCALARS:
        np.testing.assert_allclose(got[k], ref[k], rtol=LOSS_RTOL, err_msg=f"{tag} {k}")
    for name, (d, scale) in dist.items():
        assert scale > 0 and d <= GRAD_TOL * scale, f"{tag}: {name} gradient off by {d / scale:.3g} of max|ref|"
    assert np.all(grad[..., :4][~ref["mask"]] == 0), f"{tag}: a negative anchor got a box gradient"


# ---- 1 / 2: the raw matcher ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B", CASES)
def test_match_is_the_references(M, name, B):
    _, _, annot, anc, off = T.inputs(O, name, B)
    for k in T.TOPKS:
        ref = T.matched(O, name, B, k)
        rc, mask, thr, cand = raw_match(M, annot, anc, off, k)
        assert rc == 0
        print(f"{name} B={B} k={k}: positives {mask.sum(1).tolist()}, max rel thr distance {np.abs(thr / ref['thr'] - 1).max():.3g}")
        assert np.array_equal(cand, ref["cand"]), (k, cand[:, :48], ref["cand"][:, :48])
        assert set(np.unique(mask).tolist()) <= {0, 1}           # every byte of the 0xFF pre-fill was written
        assert np.array_equal(mask.astype(bool), ref["mask"]), k
        np.testing.assert_allclose(thr, ref["thr"], rtol=1e-12)


def test_match_breaks_ties_of_the_distance_by_index(M):
    cell = np.array([[-0.25, -0.25, 0.25, 0.25], [-0.5, -0.125, 0.5, 0.125], [-0.125, -0.5, 0.125, 0.5]], np.float32)
    anc = np.ascontiguousarray(np.concatenate([cell + np.float32(0.5), cell, cell + np.float32(0.5), cell], axis=0))
    annot = np.array([[-0.3, -0.2, 0.3, 0.2]], np.float32)
    for off, k in (([0, 12], 4), ([0, 6, 12], 2), ([0, 12], 16), ([0, 1, 12], 1)):
        ref = T.atss_match(annot, anc, np.array(off, np.int32), k)
        rc, mask, thr, cand = raw_match(M, annot, anc, off, k)
        assert rc == 0 and np.array_equal(cand, ref["cand"]) and np.array_equal(mask.astype(bool), ref["mask"]), (off, k, cand[0, :14])
        np.testing.assert_allclose(thr, ref["thr"], rtol=1e-12)


def test_match_full_width(M):
    """A = 17460, six levels, B = 2"""
    _, _, annot, anc, off = T.inputs(O, "full", 2)
    assert anc.shape == (17460, 4) and len(off) == 7
    ref = T.matched(O, "full", 2, 9)
    for b in range(2):                                           # what an exact mask relies on
        C = ref["cand"][b, :ref["ncand"][b]]
        assert np.abs(ref["iou"][b, C].astype(np.float64) - ref["thr"][b]).min() >= 1e-6
    rc, mask, thr, cand = raw_match(M, annot, anc, off, 9)
    print(f"full B=2 k=9: positives {mask.sum(1).tolist()}, thresholds {thr.tolist()}")
    assert rc == 0 and np.array_equal(cand, ref["cand"])
    assert np.array_equal(mask.astype(bool), ref["mask"]) and ref["mask"].sum(1).min() > 1
    np.testing.assert_allclose(thr, ref["thr"], rtol=1e-12)


# ---- 3: a box that holds no anchor centre ---------------------------------------------------------------------------------------------
def test_box_without_an_anchor_centre_keeps_the_arg_max_alone(M):
    att, reg, _, anc, off = T.inputs(O, "P126", 1)
    annot = np.array([[0.2, 0.2, 0.3, 0.3]], np.float32)
    ref = T.atss_match(annot, anc, off, 9)
    assert ref["mask"].sum() == 1
    _, _, midx, npos, lf = run(M, att, reg, annot, anc, T.PYRAMIDS["P126"], matcher="atss")
    assert npos.tolist() == [1] and midx.tolist() == [int(ref["best"][0])]
    assert np.array_equal(lf.pos_mask.cpu().numpy().astype(bool), ref["mask"])


# ---- 4: the masked entry on the fixed rule's mask ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B", CASES)
def test_masked_entry_equals_the_q_entry_on_the_fixed_rules_mask(M, name, B):
    att, reg, annot, anc, _ = T.inputs(O, name, B)
    iou = O.iou_values(annot, anc)
    multi, _ = O.match_mask(iou, 0.6)
    top1, _ = O.match_mask(iou, 0.6, use_multi=False)
    assert multi.sum() > top1.sum() == B
    combos = [(3, multi, ck, ik) for ck in (0, 1, 2) for ik in (0, 1)] + [(1, top1, 0, 0), (1, top1, 1, 1), (5, top1, 0, 0), (5, top1, 0, 1)]
    for flags, mask, cls_kind, iou_kind in combos:
        old = raw_loss(M, "zsg_loss_fwd_bwd_q", att, reg, annot, anc, flags, iou_kind=iou_kind, cls_kind=cls_kind)
        new = raw_loss(M, "zsg_loss_fwd_bwd_m", att, reg, annot, anc, flags, mask=mask, iou_kind=iou_kind, cls_kind=cls_kind)
        tag = (flags, cls_kind, iou_kind)
        assert old[0] == 0 and new[0] == 0, tag
        assert np.array_equal(new[1].view(np.int32), old[1].view(np.int32)), (tag, new[1], old[1])
        assert np.array_equal(new[2].view(np.int32), old[2].view(np.int32)), tag
        assert np.array_equal(new[3], old[3]) and np.array_equal(new[4], old[4]) and np.array_equal(new[4], mask.sum(1)), tag
    # the arg-max anchor is positive whatever the mask says
    none = raw_loss(M, "zsg_loss_fwd_bwd_m", att, reg, annot, anc, 3, mask=np.zeros_like(multi))
    one = raw_loss(M, "zsg_loss_fwd_bwd_m", att, reg, annot, anc, 3, mask=top1)
    assert none[4].tolist() == [1] * B and all(np.array_equal(a, b) for a, b in zip(none[1:], one[1:]))


# ---- 5: ZSGLoss(matcher="atss") against the fp64 criterion on the reference's mask ----------------------------------------------------
@pytest.mark.parametrize("name,B,variant", [(n, B, v) for n, B in CASES for v in VARIANTS] + [("full", 2, "qfl_giou")])     # (full width once)
def test_loss_parity_with_fp64_reference(M, name, B, variant):
    att, reg, annot, anc, off = T.inputs(O, name, B)
    kw = VARIANTS[variant]
    for k in ((9,) if name == "full" else T.TOPKS):
        m = T.matched(O, name, B, k)
        ref = T.compose(att, reg, annot, anc, m["mask"], m["best"], kind=kw.get("cls_quality", "none"), box_iou=kw.get("box_iou_loss", "none"))
        got, grad, midx, npos, lf = run(M, att, reg, annot, anc, feat_sizes(name), matcher="atss", atss_topk=k, **kw)
        assert ("iou_ls" in got) == ("box_iou_loss" in kw) and ("pos_iou" in got) == ("cls_quality" in kw)
        check(f"atss {variant} {name} B={B} k={k}", got, grad, ref)
        assert np.array_equal(midx, m["best"].astype(np.int32)) and np.array_equal(npos, m["mask"].sum(1).astype(np.int32))
        assert np.array_equal(lf.pos_mask.cpu().numpy().astype(bool), m["mask"])
        np.testing.assert_allclose(lf.atss_thr.cpu().numpy(), m["thr"], rtol=1e-12)
        assert np.abs(grad[..., :4][m["mask"]]).max() > 0


# ---- 6: further properties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["P126", "P261"])
def test_two_runs_are_bit_identical(M, name):
    att, reg, annot, anc, off = T.inputs(O, name, 3)
    kw = dict(matcher="atss", cls_quality="qfl", box_iou_loss="giou")
    a, b = run(M, att, reg, annot, anc, T.PYRAMIDS[name], **kw), run(M, att, reg, annot, anc, T.PYRAMIDS[name], **kw)
    assert a[0] == b[0] and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    assert torch.equal(a[4].pos_mask, b[4].pos_mask) and torch.equal(a[4].atss_thr, b[4].atss_thr)
    m1, m2 = raw_match(M, annot, anc, off, 12), raw_match(M, annot, anc, off, 12)
    assert all(np.array_equal(x, y) for x, y in zip(m1[1:], m2[1:]))


@pytest.mark.parametrize("name", ["P126", "P261"])
def test_grad_scale_quarters_the_gradient_exactly(M, name):
    att, reg, annot, anc, _ = T.inputs(O, name, 3)
    mask = T.matched(O, name, 3, 9)["mask"]
    res = [raw_loss(M, "zsg_loss_fwd_bwd_m", att, reg, annot, anc, 3, mask=mask, scale=s, iou_kind=1, cls_kind=1) for s in (1.0, 0.25)]
    assert res[0][0] == 0 and res[1][0] == 0
    assert np.array_equal(res[0][1], res[1][1])                  # the loss values are not scaled
    assert np.abs(res[0][2][..., 4]).min() > 0
    assert np.array_equal((res[0][2] * np.float32(0.25)).view(np.int32), res[1][2].view(np.int32))


@pytest.mark.parametrize("variant", ["focal", "qfl_giou"])
@pytest.mark.parametrize("name", ["P126", "P261"])
def test_nan_rule(M, name, variant):
    """a NaN att logit (at a negative and at a positive anchor): the constants and no gradient anywhere"""
    att, reg, annot, anc, _ = T.inputs(O, name, 3)
    mask = T.matched(O, name, 3, 9)["mask"]
    for where in (np.nonzero(~mask[1])[0][-1], np.nonzero(mask[1])[0][-1]):
        bad = att.copy()
        bad[1, where] = float("nan")
        got, grad, _, npos, _ = run(M, bad, reg, annot, anc, T.PYRAMIDS[name], matcher="atss", **VARIANTS[variant])
        assert got["cls_ls"] == 1.0 and got["box_ls"] == np.float32(0.01) and got.get("iou_ls", 0.0) == 0.0 and got.get("pos_iou", 0.0) == 0.0, got
        np.testing.assert_allclose(got["loss"], 1.01, rtol=1e-6)
        assert np.all(grad == 0)
        assert np.array_equal(npos, mask.sum(1))                 # the matching does not look at the network's output


def test_limits_are_rejected_before_anything_is_launched(M):
    lib = M[0].lib
    _, _, annot, anc, off = T.inputs(O, "P126", 3)

    def refused(word, **kw):
        args = dict(annot=annot, anc=anc, off=off, k=9)
        args.update(kw)
        rc, mask, thr, cand = raw_match(M, **args)
        assert rc == -1 and word in lib.zsg_last_error(), (kw, rc, lib.zsg_last_error())
        assert np.all(mask == 0xFF) and np.all(thr == -7.0) and np.all(cand == -7)

    refused(b"L=9", off=list(range(0, 127, 14)), L=9)
    refused(b"topk=0", k=0)
    refused(b"topk=17", k=17)
    refused(b"B=513", B=513)
    refused(b"=117", off=[0, 81, 117])                           # the table ends below A = 126
    refused(b"=126", off=[0, 81, 126], A=125)
    refused(b"level_off[2]=81", off=[0, 81, 81, 126])            # an empty level
    refused(b"level_off[0]=1", off=[1, 81, 126])
    rc, mask, _, _ = raw_match(M, annot, anc, off, 16)
    assert rc == 0 and set(np.unique(mask).tolist()) <= {0, 1}
    big = np.ascontiguousarray(np.resize(annot, (512, 4)))
    rc, mask, _, _ = raw_match(M, big, anc, off, 9)
    assert rc == 0 and np.array_equal(mask[:3].astype(bool), T.matched(O, "P126", 3, 9)["mask"]) and np.array_equal(mask[3:6], mask[:3])


# ---- 7: the default configuration ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B", [("P126", 3), ("P261", 3)])
def test_default_matcher_gives_the_bits_of_the_raw_entry(M, name, B):
    att, reg, annot, anc, _ = T.inputs(O, name, B)
    got, grad, midx, npos, lf = run(M, att, reg, annot, anc, T.PYRAMIDS[name])
    assert lf.matcher == "iou" and not hasattr(lf, "pos_mask")
    rc, losses, g, mi, n = raw_loss(M, "zsg_loss_fwd_bwd", att, reg, annot, anc, 3, lamb_iou=1.0)
    assert rc == 0 and len(lf._last_losses) == 3
    assert np.array_equal(lf._last_losses.cpu().numpy().view(np.int32), losses.view(np.int32))
    assert np.array_equal(grad.view(np.int32), g.view(np.int32)) and np.array_equal(midx, mi) and np.array_equal(npos, n)
    assert np.array_equal(n, O.match_mask(O.iou_values(annot, anc), 0.6)[0].sum(1))
