"""CPU-only checks of the task-aligned anchor assignment (cfg matcher = "tal"): the cfg keys and ZSGLoss's validation of them, the
properties of the numpy reference (tests/tal_ref.py) on the seeded inputs the GPU tests use, the conditions that let tests/test_gpu_tal.py
compare masks exactly (so that a failure there is the kernel's and not the inputs'), and the declaration / binding of the new symbols with
the refusals that need no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import atss_ref as T
import tal_ref as R

from oracle import zsg_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every (pyramid, B, topk, (alpha, beta)) whose mask tests/test_gpu_tal.py compares exactly with the reference's
EXACT = [(name, B, k, e) for name, B in R.CASES for k in R.TOPKS for e in R.EXPONENTS] + [("full", 2, 13, (1.0, 6.0))]


def test_config_keys_and_validation():
    from zsgnet_pytorch_amd import config, loss
    cfg = config.get_cfg()
    assert cfg["matcher"] == "iou" and (cfg["tal_topk"], cfg["tal_alpha"], cfg["tal_beta"]) == (13, 1.0, 6.0)
    r, s = config.ratios_scales(cfg)
    assert "tal" in loss.ZSGLoss.MATCHERS
    lf = loss.get_default_loss(r, s, config.get_cfg(matcher="tal"))
    assert lf.matcher == "tal" and (lf.tal_topk, lf.tal_alpha, lf.tal_beta) == (13, 1.0, 6.0) and lf.loss_keys == ["loss", "cls_ls", "box_ls"]
    lf = loss.get_default_loss(r, s, config.get_cfg(matcher="tal", tal_topk=32, tal_alpha=0.0, tal_beta=0.0, cls_quality="qfl", box_iou_loss="giou"))
    assert lf.tal_topk == 32 and lf.loss_keys == ["loss", "cls_ls", "box_ls", "iou_ls", "pos_iou"]
    assert loss.get_default_loss(r, s, config.get_cfg(matcher="tal", lamb_reg=0, box_iou_loss="diou")).loss_keys == ["loss", "cls_ls", "box_ls", "iou_ls"]
    for bad, key in ((dict(matcher="TAL"), "matcher"), (dict(matcher="tal", use_multi=False), "use_multi"),
                     (dict(matcher="tal", use_multi=False, use_softmax=True), "use_multi"), (dict(matcher="tal", use_softmax=True), "use_softmax"),
                     (dict(matcher="tal", tal_topk=0), "tal_topk"), (dict(matcher="tal", tal_topk=33), "tal_topk"),
                     (dict(matcher="tal", tal_topk=-1), "tal_topk"),
                     (dict(matcher="tal", tal_alpha=-0.5), "tal_alpha"), (dict(matcher="tal", tal_alpha=float("nan")), "tal_alpha"),
                     (dict(matcher="tal", tal_alpha=float("inf")), "tal_alpha"),
                     (dict(matcher="tal", tal_beta=-1.0), "tal_beta"), (dict(matcher="tal", tal_beta=float("nan")), "tal_beta"),
                     (dict(matcher="tal", tal_beta=float("inf")), "tal_beta")):
        with pytest.raises(ValueError, match=key):
            loss.get_default_loss(r, s, config.get_cfg(**bad))
    cfg = config.get_cfg(matcher="tal")
    cfg["tal_topk"] = 13.0                                # (not an integer)
    with pytest.raises(ValueError, match="tal_topk"):
        loss.get_default_loss(r, s, cfg)
    # under the other matchers the keys are not looked at, and tal does not look at theirs
    assert loss.get_default_loss(r, s, config.get_cfg(tal_topk=99, tal_alpha=-1.0)).matcher == "iou"
    assert loss.get_default_loss(r, s, config.get_cfg(matcher="atss", tal_beta=-1.0)).matcher == "atss"
    assert loss.get_default_loss(r, s, config.get_cfg(matcher="tal", atss_topk=99, matching_threshold=7.0)).matcher == "tal"
    cfg = config.update_from_dict(config.get_cfg(), {"matcher": "tal", "tal_topk": "9", "tal_alpha": "0.5", "tal_beta": "2"})
    assert (cfg["matcher"], cfg["tal_topk"], cfg["tal_alpha"], cfg["tal_beta"]) == ("tal", 9, 0.5, 2.0)


@pytest.mark.parametrize("name,B,k,expo", EXACT)
def test_reference_properties_and_the_conditions_for_exact_masks(name, B, k, expo):
    alpha, beta = expo
    m = R.matched(O, name, B, k, alpha, beta)
    att, reg, annot, anc = R.inputs(O, name, B)
    assert m["mask"].shape == att.shape and np.all(m["metric"][~m["inside"]] == -1.0) and not np.isnan(m["metric"]).any()
    for b in range(B):
        t, cand, sel = m["metric"][b], m["order"][b], np.nonzero(m["mask"][b])[0]
        assert set(cand) == set(np.nonzero(m["inside"][b] & (t > 0))[0].tolist())
        assert set(sel.tolist()) <= set(cand)                                           # selected is a subset of the candidates
        assert len(sel) == min(k, len(cand))
        rest = [a for a in cand if not m["mask"][b, a]]
        if rest and len(sel):                                                           # no unselected candidate has a larger key
            worst = max(sel.tolist(), key=lambda a: (-t[a], a))
            assert all((-t[a], a) > (-t[worst], worst) for a in rest)
    gap, low = R.gaps(m, k)
    need = R.GAP_FACTOR * R.metric_tolerance(alpha, beta)
    print(f"{name} B={B} k={k} alpha={alpha} beta={beta}: candidates {[len(c) for c in m['order']]}, smallest relative gap {gap:.3g}, "
          f"smallest candidate t {low:.3g}, needed {need:.3g}")
    assert max(len(c) for c in m["order"]) > k and np.isfinite(gap)                     # the selection has something to leave out
    assert gap >= need and low >= need
    # the task-aligned positives are not those of the fixed rule
    fixed = O.match_mask(O.iou_values(annot, anc), 0.6)[0]
    assert not np.array_equal(R.with_best(m["mask"], annot, anc)[0], fixed)


def test_reference_on_small_hand_made_cases():
    anc = np.array([[-0.5, -0.5, 0.5, 0.5], [-0.25, -0.25, 0.25, 0.25], [-0.5, -0.25, 0.5, 0.25], [0.5, 0.5, 1.0, 1.0]], np.float32)
    annot = np.array([[-0.4, -0.4, 0.4, 0.4]], np.float32)
    reg = np.zeros((1, 4, 4), np.float32)                 # a zero regression output decodes to the anchor itself
    att = np.zeros((1, 4), np.float32)
    m = R.tal_match(att, reg, annot, anc, 2, 1.0, 1.0)
    iou = T.iou_f32(annot[0], anc).astype(np.float64)
    assert m["inside"][0].tolist() == [True, True, True, False] and m["metric"][0, 3] == -1.0
    np.testing.assert_allclose(m["metric"][0, :3], 0.5 * iou[:3], rtol=1e-6)            # score x anchor IoU at initialisation
    assert m["mask"][0].tolist() == [True, False, True, False]
    # ties go to the lower index; beta = 0 with one score makes every inside anchor tie
    m = R.tal_match(att, reg, annot, anc, 2, 1.0, 0.0)
    assert m["mask"][0].tolist() == [True, True, False, False] and np.all(m["metric"][0, :3] == 0.5)
    # a NaN anywhere in a row: never a candidate (also where the power would hide it), stored as NaN
    bad = reg.copy()
    bad[0, 0, 2] = np.nan
    m = R.tal_match(att, bad, annot, anc, 2, 1.0, 0.0)
    assert np.isnan(m["metric"][0, 0]) and m["mask"][0].tolist() == [False, True, True, False]
    # decodes that overflow, from inputs without a NaN: an infinite size gives u = 0, an infinite centre inf - inf, hence a NaN u and a
    # NaN t whatever beta is; neither is a candidate
    with np.errstate(all="ignore"):
        big = reg.copy()
        big[0, 0, 2] = 1000.0                             # exp overflows: the box is the whole plane
        big[0, 1, 0] = np.inf                             # the centre is at infinity
        big[0, 2, 0], big[0, 2, 2] = np.inf, 1000.0       # both
        for beta in (6.0, 0.0):
            m = R.tal_match(att, big, annot, anc, 13, 1.0, beta)
            assert m["u"][0, 0] == 0.0 and np.isnan(m["u"][0, 1:3]).all() and np.isnan(m["metric"][0, 1:3]).all()
            assert m["metric"][0, 0] == (0.0 if beta else 0.5) and m["mask"][0].tolist() == [not beta, False, False, False]
    # fewer candidates than topk, and none
    m = R.tal_match(att, reg, annot, anc, 13, 1.0, 6.0)
    assert m["mask"][0].tolist() == [True, True, True, False]
    m = R.tal_match(att, reg, np.array([[0.6, 0.6, 0.7, 0.7]], np.float32), anc, 13, 1.0, 6.0)
    assert not m["mask"].any() and np.all(m["metric"] == -1.0)
    # a decoded box that misses the annotation: t = 0, inside but no candidate
    far = reg.copy()
    far[0, 1, 0] = 8.0
    m = R.tal_match(att, far, annot, anc, 13, 1.0, 6.0)
    assert m["metric"][0, 1] == 0.0 and m["mask"][0].tolist() == [True, False, True, False]


def test_tolerance_comes_from_the_formats():
    assert R.E_S == 2.0 ** -22 and R.E_U == 2.0 ** -23
    assert R.metric_tolerance(1.0, 6.0) == R.E_S + 6 * R.E_U and R.metric_tolerance(0.5, 2.0) == 0.5 * R.E_S + 2 * R.E_U
    assert R.metric_tolerance(1.0, 6.0) < 1e-6


def test_header_declares_and_the_binding_resolves_the_new_symbols():
    from zsgnet_pytorch_amd import _lib
    header = open(os.path.join(ROOT, "include", "zsg.h")).read()
    for sym in ("zsg_match_tal", "zsg_match_tal_workspace_bytes"):
        assert re.search(r"\b%s\(" % sym, header), sym
        assert sym in _lib.SIGNATURES
        getattr(_lib.lib, sym)
    assert _lib.lib.zsg_match_tal_workspace_bytes(3, 261) == 3 * 261 * 8
    # bad arguments are refused before any launch (no GPU is touched)
    one = ctypes.c_void_p(8)                             # (a non-null pointer that is never followed: every call below fails its checks)
    big = 1 << 30

    def call(B=1, A=12, k=13, alpha=1.0, beta=6.0, ws=big, mask=one):
        return _lib.lib.zsg_match_tal(one, one, one, B, A, k, alpha, beta, mask, None, one, ws, None)

    for kw, word in ((dict(k=0), b"topk=0"), (dict(k=33), b"topk=33"), (dict(B=513), b"B=513"), (dict(alpha=-1.0), b"alpha="),
                     (dict(alpha=float("nan")), b"alpha="), (dict(alpha=float("inf")), b"alpha="), (dict(beta=-0.5), b"beta="),
                     (dict(beta=float("nan")), b"beta="), (dict(ws=12 * 8 - 1), b"ws_bytes="), (dict(mask=None), b"null pointer")):
        assert call(**kw) == -1 and word in _lib.lib.zsg_last_error(), (kw, _lib.lib.zsg_last_error())
