"""CPU-only checks of the ATSS anchor assignment (cfg matcher = "atss"): the fp64 criterion of tests/atss_ref.py pinned to the oracle on
the oracle's own mask, the conditions the GPU tests rely on (so that a failure there is the kernel's and not the inputs'), the cfg keys and
ZSGLoss's validation of them, loss_keys, and the declaration / binding of the new symbols."""
import os
import re

import numpy as np
import pytest
import torch

import atss_ref as T

from oracle import zsg_oracle as O  # noqa: E402

GRAD_TOL, LOSS_RTOL = 2e-5, 1e-5          # the bounds of tests/test_gpu_boxiou.py
CASES = [(name, B) for name in T.PYRAMIDS for B in T.BATCHES]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,B", CASES)
def test_criterion_on_the_oracles_mask_is_the_oracles(name, B):
    att, reg, annot, anc, _ = T.inputs(O, name, B)
    for kw in (dict(), dict(alpha=0.75, gamma=1.5, lamb_reg=2.0)):
        r = O.zsg_loss(att, reg, annot, anc, **kw)
        assert not r["nan"] and r["mask"].sum(1).max() > 1
        c = T.compose(att, reg, annot, anc, r["mask"], r["best"], **kw)
        for k in ("loss", "cls_ls", "box_ls"):
            np.testing.assert_allclose(c[k], float(r[k]), rtol=LOSS_RTOL, err_msg=k)
        for k in ("g_att", "g_reg"):
            scale = np.abs(r[k]).max()
            assert scale > 0 and np.abs(c[k] - r[k]).max() <= GRAD_TOL * scale, k
        assert np.all(c["g_reg"][~r["mask"]] == 0)


def test_reference_iou_is_the_oracles():
    for name, B in CASES:
        _, _, annot, anc, _ = T.inputs(O, name, B)
        m = T.matched(O, name, B, 9)
        assert np.array_equal(m["iou"], O.iou_values(annot, anc))
        assert np.array_equal(m["best"], O.match_mask(m["iou"], 0.6)[1])


@pytest.mark.parametrize("name,B", CASES)
def test_conditions_the_gpu_tests_rely_on(name, B):
    _, _, annot, anc, off = T.inputs(O, name, B)
    n_l = np.diff(off)
    fixed = O.match_mask(O.iou_values(annot, anc), 0.6)[0]
    for k in T.TOPKS:
        m = T.matched(O, name, B, k)
        assert np.array_equal(m["per_level"], np.broadcast_to(np.minimum(k, n_l), (B, len(n_l))))
        assert np.array_equal(m["ncand"], np.full(B, np.minimum(k, n_l).sum()))
        for b in range(B):
            C = m["cand"][b, :m["ncand"][b]]
            assert len(set(C.tolist())) == len(C) and np.all(m["cand"][b, m["ncand"][b]:] == -1)
            assert m["mask"][b, m["best"][b]]
            gap = np.abs(m["iou"][b, C].astype(np.float64) - m["thr"][b]).min()
            assert gap >= 1e-6, (k, b, gap)
            if k == 9:
                assert m["mask"][b].sum() > 1
            assert not np.array_equal(m["mask"][b], fixed[b]), (k, b)
    assert 12 > n_l.min() == 9                           # k = 12 exceeds the smallest level, k = 9 equals it


def test_ties_of_the_distance_go_to_the_lower_index():
    """anchors with one centre (exactly, in fp32) tie in d: the lower index is the nearer one"""
    cell = np.array([[-0.25, -0.25, 0.25, 0.25], [-0.5, -0.125, 0.5, 0.125], [-0.125, -0.5, 0.125, 0.5]], np.float32)
    anc = np.concatenate([cell + np.float32(0.5), cell, cell + np.float32(0.5), cell], axis=0)      # cells 1 and 3 share the centre (0, 0)
    m = T.atss_match(np.array([[-0.3, -0.2, 0.3, 0.2]], np.float32), anc, np.array([0, 12], np.int32), 4)
    assert m["cand"][0, :5].tolist() == [3, 4, 5, 9, -1]
    m = T.atss_match(np.array([[-0.3, -0.2, 0.3, 0.2]], np.float32), anc, np.array([0, 6, 12], np.int32), 2)
    assert m["cand"][0, :5].tolist() == [3, 4, 9, 10, -1]


def test_a_box_that_holds_no_anchor_centre_keeps_the_arg_max_alone():
    anc, off = T.pyramid_anchors(O, "P126")
    g = np.array([[0.2, 0.2, 0.3, 0.3]], np.float32)
    acy, acx = T.centres(anc)
    assert not np.any((g[0, 0] < acy) & (acy < g[0, 2]) & (g[0, 1] < acx) & (acx < g[0, 3]))
    m = T.atss_match(g, anc, off, 9)
    assert m["mask"].sum() == 1 and m["mask"][0, m["best"][0]] and m["iou"][0, m["best"][0]] > 0


def test_one_candidate_has_no_deviation():
    anc = np.array([[-0.5, -0.5, 0.5, 0.5]], np.float32)
    m = T.atss_match(np.array([[-0.4, -0.4, 0.4, 0.4]], np.float32), anc, np.array([0, 1], np.int32), 9)
    assert m["thr"][0] == float(m["iou"][0, 0]) and m["mask"][0, 0] and m["ncand"][0] == 1


def test_config_keys_and_validation():
    from zsgnet_pytorch_amd import config, loss
    cfg = config.get_cfg()
    assert cfg["matcher"] == "iou" and cfg["atss_topk"] == 9
    r, s = config.ratios_scales(cfg)
    off = loss.get_default_loss(r, s, cfg)
    assert off.matcher == "iou" and off.loss_keys == ["loss", "cls_ls", "box_ls"]
    lf = loss.get_default_loss(r, s, config.get_cfg(matcher="atss"))
    assert lf.matcher == "atss" and lf.atss_topk == 9 and lf.loss_keys == ["loss", "cls_ls", "box_ls"]
    lf = loss.get_default_loss(r, s, config.get_cfg(matcher="atss", atss_topk=16, cls_quality="qfl", box_iou_loss="giou"))
    assert lf.atss_topk == 16 and lf.loss_keys == ["loss", "cls_ls", "box_ls", "iou_ls", "pos_iou"]
    assert loss.get_default_loss(r, s, config.get_cfg(matcher="atss", box_iou_loss="diou")).loss_keys == ["loss", "cls_ls", "box_ls", "iou_ls"]
    for bad, key in ((dict(matcher="ATSS"), "matcher"), (dict(matcher=""), "matcher"), (dict(matcher="atss", use_multi=False), "use_multi"),
                     (dict(matcher="atss", use_multi=False, use_softmax=True), "use_multi"),
                     (dict(matcher="atss", use_softmax=True), "use_softmax"),
                     (dict(matcher="atss", atss_topk=0), "atss_topk"), (dict(matcher="atss", atss_topk=17), "atss_topk")):
        with pytest.raises(ValueError, match=key):
            loss.get_default_loss(r, s, config.get_cfg(**bad))
    # the same settings under the fixed rule stay valid, and atss_topk is not looked at there
    assert loss.get_default_loss(r, s, config.get_cfg(use_multi=False, use_softmax=True)).matcher == "iou"
    assert loss.get_default_loss(r, s, config.get_cfg(atss_topk=99)).matcher == "iou"
    cfg = config.update_from_dict(config.get_cfg(), {"matcher": "atss", "atss_topk": "12"})
    assert cfg["matcher"] == "atss" and cfg["atss_topk"] == 12


def test_set_anchors_builds_the_level_table():
    from zsgnet_pytorch_amd import config, loss
    cfg = config.get_cfg(matcher="atss")
    r, s = config.ratios_scales(cfg)
    lf = loss.get_default_loss(r, s, cfg)
    assert lf.anchs is None and lf.level_off is None
    anc, off = T.pyramid_anchors(O, "P261")
    lf.set_anchors(torch.from_numpy(anc), T.PYRAMIDS["P261"])
    assert lf.level_off.dtype == torch.int32 and lf.level_off.device.type == "cpu" and lf.level_off.tolist() == off.tolist()
    assert lf.anchs.shape == (261, 4)
    lf.set_anchors(torch.from_numpy(anc), torch.tensor(T.PYRAMIDS["P261"]))
    assert lf.level_off.tolist() == [0, 180, 234, 252, 261]
    with pytest.raises(ValueError, match="261"):
        lf.set_anchors(torch.from_numpy(anc), T.PYRAMIDS["P189"])
    with pytest.raises(ValueError, match="9 pyramid levels"):
        lf.set_anchors(torch.from_numpy(anc[:81]), [(1, 1)] * 9)
    lf.set_anchors(torch.from_numpy(anc[:72]), [(1, 1)] * 8)
    assert lf.level_off.tolist() == list(range(0, 73, 9))


def test_header_declares_and_the_binding_resolves_the_new_symbols():
    import ctypes
    from zsgnet_pytorch_amd import _lib
    header = open(os.path.join(ROOT, "include", "zsg.h")).read()
    for sym in ("zsg_match_atss", "zsg_match_atss_workspace_bytes", "zsg_loss_fwd_bwd_m"):
        assert re.search(r"\b%s\(" % sym, header), sym
        assert sym in _lib.SIGNATURES
        getattr(_lib.lib, sym)
    assert len(_lib.SIGNATURES["zsg_loss_fwd_bwd_m"][1]) == len(_lib.SIGNATURES["zsg_loss_fwd_bwd_q"][1]) + 1
    # per (sample, level): 16 slot records of 8 bytes and one arg-max record
    assert _lib.lib.zsg_match_atss_workspace_bytes(3, 6) == 3 * 6 * (16 * 8 + 8)
    # bad arguments are refused before any launch (no GPU is touched)
    lv = (ctypes.c_int32 * 10)(0, 5, 9, 12, 14, 15, 16, 17, 18, 19)
    one = ctypes.c_void_p(8)                             # (a non-null pointer that is never followed: every call below fails its checks)
    call = lambda L, B, A, k: _lib.lib.zsg_match_atss(one, one, ctypes.addressof(lv), L, B, A, k, one, None, None, one, 1 << 20, None)
    for args, word in (((9, 1, 19, 9), b"L=9"), ((3, 1, 12, 0), b"topk=0"), ((3, 1, 12, 17), b"topk=17"), ((3, 513, 12, 9), b"B=513"),
                       ((3, 1, 13, 9), b"expected A=13")):
        assert call(*args) == -1 and word in _lib.lib.zsg_last_error(), (args, _lib.lib.zsg_last_error())
    assert _lib.lib.zsg_loss_fwd_bwd_m(None, None, None, 1, 1, 0.25, 2.0, 1.0, 0.6, 3, 1.0, 0, 1.0, 0, None, None, None, None, None, None, 0,
                                       None) == -1
    assert b"loss_fwd_bwd_m" in _lib.lib.zsg_last_error()
