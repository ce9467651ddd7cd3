"""Top-k grounding, host side: the numpy restatement (tests/topk_ref.py) is pinned to the fixture made from the reference's functions
(tests/golden/g17_topk.npz), the config keys, eval_script.evaluate(topk=k), and the C ABI of the two new symbols."""
import os
import pickle
import re

import numpy as np
import pytest

import topk_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases(gold):
    g = gold("g17_topk")
    return g, [str(n) for n in g["cases"]]


def test_fixture_plants_every_required_case(gold):
    g, names = _cases(gold)
    assert set(names) == {"b16", "b1", "ties", "saturated", "collapse", "k1", "pre_gt_A", "nan", "full", "limits"}
    c = {n: topk_ref.load_case(g, n) for n in names}
    assert c["b1"]["out5"].shape[0] == 1 and c["b16"]["out5"].shape[0] == 16 and c["full"]["out5"].shape[1] == 17460
    assert (c["limits"]["pre_n"], c["limits"]["K"]) == (512, 64) and c["limits"]["out5"].shape[1] > 16 * (2048 - 512)
    assert c["k1"]["K"] == 1 and c["pre_gt_A"]["pre_n"] > c["pre_gt_A"]["out5"].shape[1]
    assert c["collapse"]["want"]["topk_n"].min() < c["collapse"]["K"]
    assert np.isnan(c["nan"]["out5"][..., 4]).sum() >= 2 and np.isnan(c["pre_gt_A"]["out5"][..., 4]).any()
    for n in ("saturated", "full", "limits"):                      # several logits > 20: the score is exactly 1
        assert ((c[n]["out5"][..., 4] > 20).sum(1) >= 3).all()
        assert (c[n]["want"]["topk_scores"][:, 0] == 1.0).all()
    for n in ("ties", "full", "limits"):                           # bit-equal logits inside the top pre_n and across the cut
        for row in c[n]["out5"][..., 4]:
            x = row[topk_ref.rank_order(topk_ref.O._sigmoid(row))]
            p = c[n]["pre_n"]
            assert x[p - 2] == x[p - 1] == x[p] == x[p + 1] and x[10] == x[11]
    # hits at several ranks, and misses
    assert len(set(c["b16"]["want"]["hit_rank"].tolist())) >= 4


@pytest.mark.parametrize("name", ["b16", "b1", "ties", "saturated", "collapse", "k1", "pre_gt_A", "nan", "full", "limits"])
def test_restatement_matches_reference_fixture(gold, name):
    g, _ = _cases(gold)
    c = topk_ref.load_case(g, name)
    r = topk_ref.topk(c["out5"][..., 4], c["out5"][..., :4], c["annot"], c["img_size"], c["anchors"], c["pre_n"], c["K"],
                      c["nms_thr"], c["acc_thr"])
    w = c["want"]
    for k in ("topk_idx", "topk_n", "hit_rank"):
        assert r[k].dtype == np.int32 and np.array_equal(r[k], w[k]), k
    assert np.array_equal(r["acc_at"], w["acc_at"])
    np.testing.assert_allclose(r["topk_boxes"], w["topk_boxes"], rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(r["topk_scores"], w["topk_scores"], rtol=1e-6)
    # rank 0 is the anchor the evaluator picks; rows past topk_n are empty
    assert np.array_equal(r["topk_idx"][:, 0], np.array([topk_ref.rank_order(s)[0] for s in topk_ref.O._sigmoid(c["out5"][..., 4])]))
    for b, n in enumerate(r["topk_n"]):
        assert (r["topk_idx"][b, n:] == -1).all() and (r["topk_boxes"][b, n:] == 0).all() and (r["topk_scores"][b, n:] == 0).all()
    # without ground truth: the same boxes, no metrics
    r2 = topk_ref.topk(c["out5"][..., 4], c["out5"][..., :4], None, c["img_size"], c["anchors"], c["pre_n"], c["K"], c["nms_thr"])
    assert "hit_rank" not in r2 and np.array_equal(r2["topk_idx"], r["topk_idx"])


def test_config_keys_and_defaults():
    from zsgnet_pytorch_amd.config import get_cfg, update_from_dict
    cfg = get_cfg()
    assert cfg["eval_topk"] == 1 and cfg["eval_nms_thr"] == 0.5 and cfg["eval_pre_nms"] == 128
    assert type(cfg["eval_topk"]) is int and type(cfg["eval_nms_thr"]) is float and type(cfg["eval_pre_nms"]) is int
    update_from_dict(cfg, {"eval_topk": "5", "eval_nms_thr": "0.4", "eval_pre_nms": "256"})      # the CLI override rule
    assert (cfg.eval_topk, cfg.eval_nms_thr, cfg.eval_pre_nms) == (5, 0.4, 256)


def test_eval_script_topk(tmp_path):
    from zsgnet_pytorch_amd import eval_script
    gt = tmp_path / "gt.csv"
    gt.write_text('bbox\n"[10, 10, 50, 50]"\n"[0, 0, 20, 20]"\n"[30, 30, 60, 60]"\n')
    far, near, exact = [200, 200, 240, 240], [12, 12, 50, 50], [0, 0, 20, 20]
    preds = [
        {"id": 0, "pred_boxes": far, "pred_scores": 0.9, "topk_boxes": [far, [100, 100, 120, 120], near], "topk_scores": [0.9, 0.8, 0.7]},
        {"id": 1, "pred_boxes": exact, "pred_scores": 0.9, "topk_boxes": [exact], "topk_scores": [0.9]},
        {"id": 2, "pred_boxes": far, "pred_scores": 0.5, "topk_boxes": [far, far], "topk_scores": [0.5, 0.4]},
        {"id": 1, "pred_boxes": far, "pred_scores": 0.1, "topk_boxes": [far], "topk_scores": [0.1]},      # repeated id: counted once
    ]
    pf = tmp_path / "p.pkl"
    pf.write_bytes(pickle.dumps(preds))
    assert eval_script.evaluate(pf, gt) == (1 / 3, 1, 3)
    assert eval_script.evaluate(pf, gt, topk=1) == (1 / 3, 1, 3)
    assert eval_script.evaluate(pf, gt, topk=2) == (1 / 3, 1, 3)          # the near box is third
    assert eval_script.evaluate(pf, gt, topk=3) == (2 / 3, 2, 3)
    assert eval_script.evaluate(pf, gt, topk=3, acc_iou_thresh=0.95) == (1 / 3, 1, 3)
    # strict comparison: an IoU equal to the threshold is not a hit
    half = tmp_path / "h.pkl"
    half.write_bytes(pickle.dumps([{"id": 1, "pred_boxes": far, "pred_scores": 1.0, "topk_boxes": [far, [0, 0, 20, 10]], "topk_scores": [1.0, 0.5]}]))
    assert eval_script.evaluate(half, gt, topk=2)[1] == 0 and eval_script.evaluate(half, gt, topk=2, acc_iou_thresh=0.49)[1] == 1
    assert eval_script.main([str(pf), str(gt), "--topk=3"]) == (2 / 3, 2, 3)
    old = tmp_path / "old.pkl"
    old.write_bytes(pickle.dumps([{"id": 0, "pred_boxes": far, "pred_scores": 0.9}]))
    assert eval_script.evaluate(old, gt)[2] == 1
    with pytest.raises(KeyError, match="topk_boxes"):
        eval_script.evaluate(old, gt, topk=2)


def test_cabi_declares_exports_and_binds_the_topk_symbols():
    import ctypes
    from zsgnet_pytorch_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zsg.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("zsg_eval_topk_workspace_bytes", 4), ("zsg_eval_topk", 18)):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(raw, name) and len(_lib.SIGNATURES[name][1]) == nargs
    # host-side argument checks: -1 with a message, before anything is launched (no device is touched)
    L = _lib.lib
    assert L.zsg_eval_topk_workspace_bytes(16, 17460, 128, 5) >= 16 * 128 * 8
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    args = lambda pre_n, K, boxes=p: (p, None, p, p, 2, 100, pre_n, K, 0.5, 0.5, boxes, p, p, p, None, None, p, None)
    for bad, word in ((args(0, 1), "pre_n"), (args(513, 5), "pre_n"), (args(128, 0), "K="), (args(128, 65), "K="), (args(4, 5), "exceeds"),
                      (args(128, 5, None), "null")):
        assert L.zsg_eval_topk(*bad) == -1
        assert word in L.zsg_last_error().decode()
    assert L.zsg_eval_topk(p, None, p, p, 2, 100, 128, 5, 0.5, 0.5, p, p, p, p, p, None, p, None) == -1      # hit_rank without annot
