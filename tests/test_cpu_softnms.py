"""Soft-NMS selection in the evaluator (cfg eval_nms = soft_linear / soft_gauss) without a GPU: the properties of the definition
tests/softnms_ref.py, the cfg keys and their validation, the new symbols in include/zsg.h and the ctypes table, an Evaluator with the
default cfg that never touches them, and — on the reference alone — that the inputs of tests/softnms_cases.py are safe to compare
exactly on the GPU: no pick, threshold compare, stop decision or hit decision of any case and query close enough to a tie for the
device's expf (a few 1e-7 on a score or an IoU, over at most 64 factors; 1e-4 leaves a decade of margin) to turn it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import softnms_cases as C  # noqa: E402
import softnms_ref  # noqa: E402
import topk_ref  # noqa: E402
from oracle import zsg_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def Z():
    from zsgnet_pytorch_amd import _lib, config, evaluator
    return _lib, config, evaluator


# ---- the definition --------------------------------------------------------------------------------------------------------------------------
def _boxes_case(boxes_norm, logits, img=(200.0, 400.0)):
    """candidates given as decoded boxes: anchors = the boxes, regressions zero"""
    anc = np.asarray(boxes_norm, F32)
    att = np.asarray(logits, F32)[None]
    return att, np.zeros((1, anc.shape[0], 4), F32), np.array([img], F32), anc


def test_hand_computed_three_boxes():
    # two boxes that overlap with IoU 0.6 / (0.8 + 0.8 - 0.6) = 0.6 and one far away; logits ln 9, ln 3, 0 -> scores 0.9, 0.75, 0.5
    att, reg, sz, anc = _boxes_case([[-0.5, -0.5, 0.5, 0.3], [-0.5, -0.3, 0.5, 0.5], [0.6, 0.6, 0.9, 0.9]], [np.log(9.0), np.log(3.0), 0.0])
    hard = topk_ref.topk(att, reg, None, sz, anc, 3, 3, nms_thr=0.5)
    assert hard["topk_idx"].tolist() == [[0, 2, -1]], "hard NMS removes the neighbour for good"
    lin = softnms_ref.soft_topk(att, reg, None, sz, anc, 3, 3, "soft_linear", nms_thr=0.5, min_score=0.001)
    assert lin["topk_idx"].tolist() == [[0, 2, 1]] and lin["topk_n"].tolist() == [3]      # 0.75 * (1 - 0.6) = 0.3 < 0.5
    np.testing.assert_allclose(lin["topk_scores"][0], [0.9, 0.5, 0.3], rtol=1e-6)
    gau = softnms_ref.soft_topk(att, reg, None, sz, anc, 3, 3, "soft_gauss", sigma=0.5, min_score=0.001)
    assert gau["topk_idx"].tolist() == [[0, 2, 1]]                                        # 0.75 * exp(-0.36 / 0.5) = 0.365 < 0.5
    np.testing.assert_allclose(gau["topk_scores"][0], [0.9, 0.5, 0.75 * np.exp(-0.72)], rtol=1e-6)
    wide = softnms_ref.soft_topk(att, reg, None, sz, anc, 3, 3, "soft_gauss", sigma=4.0, min_score=0.001)
    assert wide["topk_idx"].tolist() == [[0, 1, 2]]                                       # 0.75 * exp(-0.09) = 0.685 > 0.5
    stop = softnms_ref.soft_topk(att, reg, None, sz, anc, 3, 3, "soft_linear", nms_thr=0.5, min_score=0.4)
    assert stop["topk_idx"].tolist() == [[0, 2, -1]] and stop["topk_n"].tolist() == [2] and (stop["topk_boxes"][0, 2] == 0).all()
    assert np.array_equal(lin["topk_boxes"][0, :2], hard["topk_boxes"][0, :2])


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_properties_on_the_shared_cases(case):
    table, method, p, k, thr, sig, floor = case
    d = C.inputs(table, method)
    r = C.reference(case)
    o = d["out5"]
    hard = topk_ref.topk(o[..., 4], o[..., :4], d["annot"], d["img_size"], d["anchors"], p, k, thr, C.ACC_THR)
    B = o.shape[0]
    for b in range(B):
        n = int(r["topk_n"][b])
        s = r["topk_scores"][b, :n]
        assert 1 <= n <= k
        assert n == 1 or (np.diff(s[~np.isnan(s)]) <= 0).all(), "emitted scores do not increase"
        assert (s[1:] >= F32(floor)).all() and not np.isnan(s[1:]).any()
        assert (r["topk_idx"][b, n:] == -1).all() and (r["topk_scores"][b, n:] == 0).all() and (r["topk_boxes"][b, n:] == 0).all()
        assert len(set(r["topk_idx"][b, :n].tolist())) == n, "no anchor twice"
        # a NaN-score candidate is never picked after row 0
        assert not np.isnan(o[b, r["topk_idx"][b, 1:n], 4]).any()
    for key in ("topk_boxes", "topk_scores", "topk_idx"):                                 # row 0 is the hard rule's row 0 (the arg-max box)
        assert r[key][:, 0].tobytes() == hard[key][:, 0].tobytes(), key
    assert r["acc_at"].shape == (k,) and (np.diff(r["acc_at"]) >= 0).all()
    assert ((r["hit_rank"] < r["topk_n"]) | (r["hit_rank"] == k)).all()


def test_the_cases_hold_the_special_rows():
    lin = C.reference(("pooled", "soft_linear", 512, 5, 0.5, 0.5, 0.001))
    assert lin["topk_idx"][0, 0] == 40 and lin["topk_idx"][1].tolist() != list(range(5)) and lin["topk_idx"][1, 0] == 0
    assert (lin["topk_scores"][1] == lin["topk_scores"][1, 0]).all(), "the tie sample picks undecayed candidates, bit-equal scores"
    assert lin["topk_idx"][2, 0] == 200 and np.isnan(lin["topk_boxes"][2, 0]).any()
    deep = C.reference(("pooled", "soft_linear", 512, 64, 0.3, 0.5, 0.0))
    assert all(any(not cl for _, _, cl in tr["picks"]) for tr in deep["trace"]), "decayed weights really compete, in every sample"
    cell = C.reference(("cell", "soft_linear", 16, 5, 0.5, 0.5, 0.0))
    assert cell["topk_n"].tolist() == [5, 3, 1], "min_score 0: the rows end when the non-NaN candidates are used up"
    assert np.isnan(cell["topk_scores"][2, 0]) and cell["topk_idx"][2, 0] == 0
    assert C.reference(("cell", "soft_linear", 16, 5, 0.5, 0.5, 0.05))["topk_n"].tolist() == [5, 2, 1], "min_score stops the rows"
    deep = C.reference(("pooled", "soft_gauss", 64, 64, 0.5, 0.25, 0.05))
    assert (deep["topk_n"] < 64).all() and (deep["topk_n"] > 5).all()
    a, b = (C.reference(("pooled", "soft_linear", 64, 5, t, 0.5, 0.001))["topk_idx"] for t in (0.3, 0.5))
    assert not np.array_equal(a, b), "nms_thr matters"
    a, b = (C.reference(("pooled", "soft_gauss", 64, 5, 0.5, s, 0.001))["topk_idx"] for s in (0.25, 0.5))
    assert not np.array_equal(a, b), "sigma matters"
    assert C.inputs("pooled", "soft_gauss")["rows"] == [0, 2] and C.inputs("pooled", "soft_linear")["rows"] == [0, 1, 2]
    assert C.LDS_PRE in C.PRE_N and C.LDS_PRE + 1 in C.PRE_N
    src = open(os.path.join(ROOT, "zsgnet-pytorch_amd", "csrc", "softnms.hip")).read()
    assert f"#define SN_LDS_PRE {C.LDS_PRE} " in src, "the grid brackets the finishing block's LDS limit"


def test_without_overlap_linear_is_the_hard_rule():
    """candidates whose pairwise IoU is <= nms_thr: nothing decays, nothing is suppressed — soft_linear returns topk_ref.topk's arrays"""
    ctr = (-0.6, 0.0, 0.6)                                                                # nine boxes of side 0.5 on a 3 x 3 grid: side by side
    anc = np.array([[cy - 0.25, cx - 0.25, cy + 0.25, cx + 0.25] for cy in ctr for cx in ctr], F32)
    g = np.random.default_rng(3)
    att = (g.standard_normal((2, 9)) * 1.5).astype(F32)
    att[1, 4] = np.nan                                                                    # ranked last, not among pre_n = 8
    reg = (g.standard_normal((2, 9, 4)) * 0.02).astype(F32)
    annot = np.array([[-1.0, -1.0, -0.3, -0.3], [0.3, 0.3, 1.0, 1.0]], F32)
    sz = np.array([[300, 400], [200, 200]], F32)
    for b in range(2):
        boxes = O.reg_params_to_bbox(anc, reg[b][None])[0]
        iou = O.iou_values(boxes, boxes)
        assert (iou[~np.eye(9, dtype=bool)] <= F32(0.3)).all()
    for pre_n, K in ((8, 5), (8, 8), (3, 1)):
        hard = topk_ref.topk(att, reg, annot, sz, anc, pre_n, K, 0.3, 0.5)
        soft = softnms_ref.soft_topk(att, reg, annot, sz, anc, pre_n, K, "soft_linear", 0.3, 0.5, 0.0, 0.5)
        assert set(hard) == set(soft)
        for key in hard:
            assert hard[key].dtype == soft[key].dtype and hard[key].tobytes() == soft[key].tobytes(), key


# ---- safety of the GPU inputs ----------------------------------------------------------------------------------------------------------------
def _unsafe(case):
    """the decisions of one case (every query) that lie too close to a tie to be required exactly of the device"""
    table, method, p, k, thr, sig, floor = case
    bad = []
    for b, tr in enumerate(C.reference(case)["trace"]):
        for best, second, clean in tr["picks"]:                    # 1. the runner-up is clearly behind, or an exact tie of undecayed scores
            if not (second <= best * (1 - 1e-4) or (second == best and clean)):
                bad.append(("pick", b, best, second))
        if method == "soft_linear":                                # 2. no compared IoU at the threshold
            for u in tr["ious"]:
                if (np.abs(u.astype(np.float64) - float(F32(thr))) <= 1e-6).any():
                    bad.append(("nms_thr", b))
        for w in tr["floor"]:                                      # 3. no stop decision at the floor
            if abs(w - float(F32(floor))) <= 1e-4 * float(F32(floor)) and floor > 0:
                bad.append(("min_score", b, w))
        for u in tr["hit_iou"]:                                    # 4. no hit decision at acc_thr
            if abs(u - float(F32(C.ACC_THR))) <= 1e-6:
                bad.append(("acc_thr", b, u))
    return bad


def test_every_shared_case_is_safe_to_compare_exactly():
    excluded = {C.case_id(c): bad for c in C.CASES if (bad := _unsafe(c))}
    assert not excluded, f"{len(excluded)} cases hold a decision near a tie (the cap is zero; choose other seeds): {excluded}"
    assert sum(len(tr["picks"]) for c in C.CASES for tr in C.reference(c)["trace"]) > 1000, "the check looked at real picks"


# ---- the switches ----------------------------------------------------------------------------------------------------------------------------
def test_cfg_keys_defaults_and_validation(Z):
    _, config, evaluator = Z
    cfg = config.get_cfg()
    assert cfg["eval_nms"] == "hard" and cfg["eval_soft_sigma"] == 0.5 and cfg["eval_soft_min_score"] == 0.001
    r, s = config.ratios_scales(cfg)
    ev = evaluator.get_default_eval(r, s, cfg)
    assert ev.nms == "hard" and ev.met_keys == ["Acc", "MaxPos"]
    cfg2 = config.get_cfg()
    del cfg2["eval_nms"], cfg2["eval_soft_sigma"], cfg2["eval_soft_min_score"]
    assert evaluator.get_default_eval(r, s, cfg2).nms == "hard", "a cfg without the keys = the default"
    cfg3 = config.update_from_dict(config.get_cfg(), {"eval_nms": "soft_gauss", "eval_soft_sigma": "0.25", "eval_soft_min_score": "0", "eval_topk": "5"})
    ev = evaluator.get_default_eval(r, s, cfg3)
    assert (ev.nms, ev.soft_sigma, ev.soft_min_score) == ("soft_gauss", 0.25, 0.0) and ev.met_keys == ["Acc", "MaxPos", "Acc@5"]
    assert evaluator.get_default_eval(r, s, config.get_cfg(eval_nms="soft_linear", eval_soft_sigma=2)).soft_sigma == 2.0
    assert evaluator.SOFT_METHODS == {"soft_linear": 1, "soft_gauss": 2}


@pytest.mark.parametrize("key,bad", [("eval_nms", v) for v in ("soft", "linear", "HARD", "", None, 1, True, ["hard"])]
                         + [("eval_soft_sigma", v) for v in (0, -0.5, float("nan"), float("inf"), "0.5", None, True, [0.5])]
                         + [("eval_soft_min_score", v) for v in (-0.001, 1, 1.5, float("nan"), float("inf"), "0.001", None, True, [0.0])],
                         ids=lambda v: repr(v))
def test_bad_values_raise(Z, key, bad):
    _, config, evaluator = Z
    cfg = config.get_cfg(eval_nms="soft_gauss")
    cfg[key] = bad
    with pytest.raises(ValueError, match=key):
        evaluator.get_default_eval(*config.ratios_scales(cfg), cfg)


class _Spy:
    """the ctypes library with every call recorded and the new entry points forbidden"""

    def __init__(self, lib, forbid):
        self._lib, self._forbid, self.calls = lib, forbid, []

    def __getattr__(self, name):
        if name in self._forbid:
            raise AssertionError(f"{name} touched")
        self.calls.append(name)
        return lambda *a: 0


def test_the_default_evaluator_never_touches_the_new_symbols(Z, monkeypatch):
    L, config, evaluator = Z
    spy = _Spy(L.lib, {"zsg_eval_topk_soft", "zsg_eval_topk_soft_workspace_bytes"})
    monkeypatch.setattr(evaluator, "lib", spy)
    monkeypatch.setattr(evaluator, "stream_ptr", lambda: None)
    fs = [(2, 2), (1, 1)]
    A = 45
    out = dict(att_bbx_out=torch.zeros(2, A, 5), feat_sizes=torch.tensor(fs))
    inp = dict(annot=torch.zeros(2, 4), img_size=torch.full((2, 2), 100.0), idxs=torch.arange(2))
    for over in (dict(), dict(eval_topk=5), dict(eval_box_vote=0.6), dict(eval_topk=5, eval_box_vote=0.6)):
        cfg = config.get_cfg(**over)
        ev = evaluator.get_default_eval(*config.ratios_scales(cfg), cfg).eval()
        ev(out, inp)
        ev.predict(out, inp)
    assert "zsg_eval_topk" in spy.calls and "zsg_eval_vote" in spy.calls and not any("soft" in c for c in spy.calls)
    # the switch reaches the new entry, in eval mode only; training mode and eval_topk = 1 without voting launch no top-k at all
    spy2 = _Spy(L.lib, set())
    monkeypatch.setattr(evaluator, "lib", spy2)
    cfg = config.get_cfg(eval_nms="soft_linear", eval_topk=5)
    ev = evaluator.get_default_eval(*config.ratios_scales(cfg), cfg)
    ev.train()(out, inp)
    assert spy2.calls == ["zsg_eval_workspace_bytes", "zsg_eval"]
    cfg1 = config.get_cfg(eval_nms="soft_linear")
    evaluator.get_default_eval(*config.ratios_scales(cfg1), cfg1).eval()(out, inp)
    assert spy2.calls == ["zsg_eval_workspace_bytes", "zsg_eval"] * 2
    ev.eval()(out, inp)
    assert spy2.calls[4:] == ["zsg_eval_workspace_bytes", "zsg_eval", "zsg_eval_topk_soft_workspace_bytes", "zsg_eval_topk_soft"]


def test_new_symbols_are_declared_exported_and_bound(Z):
    L, _, _ = Z
    P, I32, F32_, SZ = L.P, L.I32, L.F32, L.SZ
    assert L.SIGNATURES["zsg_eval_topk_soft_workspace_bytes"] == (SZ, [I32, I32, I32, I32])
    assert L.SIGNATURES["zsg_eval_topk_soft"] == (I32, [P, P, P, P, I32, I32, I32, I32, F32_, F32_, I32, F32_, F32_, P, P, P, P, P, P, P, SZ, P])
    hdr = open(os.path.join(ROOT, "include", "zsg.h")).read()
    assert "int zsg_eval_topk_soft(" in hdr and "size_t zsg_eval_topk_soft_workspace_bytes(" in hdr
    mk = open(os.path.join(ROOT, "zsgnet-pytorch_amd", "csrc", "Makefile")).read()
    assert "softnms.hip" in mk and "$(OBJD)/softnms.hip.o: CXXFLAGS += -ffp-contract=off" in mk
    assert L.lib.zsg_eval_topk_soft_workspace_bytes(16, 17460, 128, 5) == L.lib.zsg_eval_topk_workspace_bytes(16, 17460, 128, 5)
    assert L.lib.zsg_eval_topk_soft_workspace_bytes(0, 10, 8, 1) == 0
    p = 4096                                                       # refused before anything could be launched: no GPU is needed
    ok = [p, None, p, p, 2, 100, 128, 5, 0.5, 0.5, 1, 0.5, 0.001, p, p, p, p, None, None, p, 1 << 20, None]
    cases = ((0, None, "null"), (2, None, "null"), (3, None, "null"), (13, None, "null"), (14, None, "null"), (15, None, "null"),
             (16, None, "null"), (19, None, "null"), (4, 0, "B="), (4, 65536, "B="), (5, 0, "A="), (6, 0, "pre_n"), (6, 513, "pre_n"),
             (7, 0, "K="), (7, 65, "K="), (6, 4, "K="), (10, 0, "method"), (10, 3, "method"), (8, -0.1, "nms_thr"), (8, 1.5, "nms_thr"),
             (8, float("nan"), "nms_thr"), (11, 0.0, "sigma"), (11, float("inf"), "sigma"), (11, float("nan"), "sigma"),
             (12, -0.1, "min_score"), (12, 1.0, "min_score"), (12, float("nan"), "min_score"), (20, 8, "ws_bytes"), (19, p + 4, "aligned"))
    for i, v, word in cases:
        bad = list(ok)
        bad[i] = v
        assert L.lib.zsg_eval_topk_soft(*bad) == -1, (i, v)
        assert word in L.lib.zsg_last_error().decode(), (i, v, L.lib.zsg_last_error())
    bad = list(ok)
    bad[17] = p                                                    # hit_rank without annot
    assert L.lib.zsg_eval_topk_soft(*bad) == -1 and b"annot" in L.lib.zsg_last_error()
    bad = list(ok)
    bad[1], bad[18] = p, p                                         # acc_at without hit_rank
    assert L.lib.zsg_eval_topk_soft(*bad) == -1 and b"hit_rank" in L.lib.zsg_last_error()
