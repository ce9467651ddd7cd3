"""GPU parity of top-k grounding (csrc/loss.hip: zsg_eval_topk) against tests/golden/g17_topk.npz — the reference's own functions
composed by tests/golden/make_topk_fixture.py — through the raw C ABI and through Evaluator / Learner.validate: anchor indices, counts
and hit ranks bit-exact, acc_at equal, boxes rtol 1e-5 / atol 1e-3 and scores rtol 1e-6 (the tolerances of test_gpu_loss.py for
pred_boxes / pred_scores); row 0 bit-identical to the plain evaluator's prediction."""
import numpy as np
import pytest
import torch

import topk_ref

pytestmark = pytest.mark.gpu

CASES = ["b16", "b1", "ties", "saturated", "collapse", "k1", "pre_gt_A", "nan", "full", "limits"]
TODAY = {"Acc", "MaxPos", "idxs", "pred_boxes", "pred_scores"}


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib, config, evaluator
    return _lib, config, evaluator


def _dev(c):
    return {k: torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("out5", "annot", "img_size", "anchors")}


def _raw_topk(L, c, d, with_annot=True, pre_n=None, K=None):
    """one zsg_eval_topk call through ctypes -> (rc, outputs on the host)"""
    B, A, _ = d["out5"].shape
    pre_n, K = c["pre_n"] if pre_n is None else pre_n, c["K"] if K is None else K
    o = dict(topk_boxes=torch.full((B, K, 4), -7.0, device="cuda"), topk_scores=torch.full((B, K), -7.0, device="cuda"),
             topk_idx=torch.full((B, K), -7, dtype=torch.int32, device="cuda"), topk_n=torch.full((B,), -7, dtype=torch.int32, device="cuda"),
             hit_rank=torch.full((B,), -7, dtype=torch.int32, device="cuda"), acc_at=torch.full((K,), -7.0, device="cuda"))
    ws = torch.empty(max(1, int(L.lib.zsg_eval_topk_workspace_bytes(B, A, pre_n, K)) // 8), dtype=torch.int64, device="cuda")
    rc = L.lib.zsg_eval_topk(d["out5"].data_ptr(), d["annot"].data_ptr() if with_annot else None, d["anchors"].data_ptr(),
                             d["img_size"].data_ptr(), B, A, pre_n, K, c["nms_thr"], c["acc_thr"], o["topk_boxes"].data_ptr(),
                             o["topk_scores"].data_ptr(), o["topk_idx"].data_ptr(), o["topk_n"].data_ptr(),
                             o["hit_rank"].data_ptr() if with_annot else None, o["acc_at"].data_ptr() if with_annot else None,
                             ws.data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in o.items()}


def _raw_eval(L, c, d):
    B, A, _ = d["out5"].shape
    met, pb, ps = torch.empty(2, device="cuda"), torch.empty(B, 4, device="cuda"), torch.empty(B, device="cuda")
    pi, bi = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    ws = torch.empty((int(L.lib.zsg_eval_workspace_bytes(B)) + 3) // 4, device="cuda")
    L.check(L.lib.zsg_eval(d["out5"].data_ptr(), d["annot"].data_ptr(), d["anchors"].data_ptr(), d["img_size"].data_ptr(), B, A, c["acc_thr"],
                           met.data_ptr(), pb.data_ptr(), ps.data_ptr(), pi.data_ptr(), bi.data_ptr(), ws.data_ptr(), L.stream_ptr()), "zsg_eval")
    torch.cuda.synchronize()
    return met.cpu().numpy(), pb.cpu().numpy(), ps.cpu().numpy(), pi.cpu().numpy()


def _check(got, want, with_annot=True):
    for k in ("topk_idx", "topk_n") + (("hit_rank",) if with_annot else ()):
        print(k, got[k].tolist(), "want", want[k].tolist())
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
    if with_annot:
        print("acc_at", got["acc_at"].tolist(), "want", want["acc_at"].tolist())
        assert np.array_equal(got["acc_at"], want["acc_at"])
    fin = np.isfinite(want["topk_boxes"])
    print("max |box err|", float(np.abs(got["topk_boxes"] - want["topk_boxes"])[fin].max(initial=0.0)))
    np.testing.assert_allclose(got["topk_boxes"], want["topk_boxes"], rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(got["topk_scores"], want["topk_scores"], rtol=1e-6)


@pytest.mark.parametrize("name", CASES)
def test_raw_cabi_vs_fixture(M, gold, name):
    L, *_ = M
    c = topk_ref.load_case(gold("g17_topk"), name)
    d = _dev(c)
    rc, got = _raw_topk(L, c, d)
    assert rc == 0, L.lib.zsg_last_error().decode()
    _check(got, c["want"])
    # row 0 is the plain evaluator's prediction, bit for bit, and acc_at[0] its Acc
    met, pb, ps, pi = _raw_eval(L, c, d)
    assert got["topk_boxes"][:, 0].tobytes() == pb.tobytes()
    assert got["topk_scores"][:, 0].tobytes() == ps.tobytes()
    assert np.array_equal(got["topk_idx"][:, 0], pi)
    assert got["acc_at"][0] == met[0]
    # a second run writes the same bytes
    rc2, again = _raw_topk(L, c, d)
    assert rc2 == 0 and all(again[k].tobytes() == got[k].tobytes() for k in got)
    # without ground truth: the same boxes; hit_rank / acc_at are not touched
    rc3, noan = _raw_topk(L, c, d, with_annot=False)
    assert rc3 == 0
    assert all(noan[k].tobytes() == got[k].tobytes() for k in ("topk_boxes", "topk_scores", "topk_idx", "topk_n"))
    assert (noan["hit_rank"] == -7).all() and (noan["acc_at"] == -7).all()


def _ev(M, c, **over):
    _, config, evaluator = M
    cfg = config.get_cfg(eval_topk=c["K"], eval_nms_thr=c["nms_thr"], eval_pre_nms=c["pre_n"], acc_iou_threshold=c["acc_thr"], **over)
    ev = evaluator.get_default_eval(*config.ratios_scales(cfg), cfg)
    return ev


@pytest.mark.parametrize("name", CASES)
def test_evaluator_vs_fixture(M, gold, name):
    c = topk_ref.load_case(gold("g17_topk"), name)
    d = _dev(c)
    K, B = c["K"], d["out5"].shape[0]
    ev = _ev(M, c)
    ev.anchs = d["anchors"]
    out = dict(att_bbx_out=d["out5"], feat_sizes=None, num_f_out=torch.tensor([1]))
    inp = dict(annot=d["annot"], img_size=d["img_size"], idxs=torch.arange(B).float().cuda())
    assert ev.training and set(ev(out, inp)) == TODAY                 # training mode: nothing is added to the per-step path
    ev.eval()
    em = ev(out, inp)
    pr = ev.predict(out, dict(img_size=d["img_size"]))
    assert set(pr) == {"topk_boxes", "topk_scores", "topk_n"}
    got = {k: v.cpu().numpy() for k, v in pr.items()}
    got["topk_idx"] = ev.topk_idx.cpu().numpy()
    _check(got, c["want"], with_annot=False)
    if K == 1:                                                         # eval_topk = 1: exactly today's keys
        assert set(em) == TODAY and ev.met_keys == ["Acc", "MaxPos"]
        assert got["topk_boxes"][:, 0].tobytes() == em["pred_boxes"].cpu().numpy().tobytes()
        return
    assert ev.met_keys == ["Acc", "MaxPos", f"Acc@{K}"]
    assert set(em) == TODAY | {"topk_boxes", "topk_scores", "topk_n", "hit_rank", f"Acc@{K}"}
    got = {k: em[k].cpu().numpy() for k in ("topk_boxes", "topk_scores", "topk_n", "hit_rank")}
    got["topk_idx"], got["acc_at"] = ev.topk_idx.cpu().numpy(), ev.acc_at.cpu().numpy()
    _check(got, c["want"])
    assert em[f"Acc@{K}"].item() == c["want"]["acc_at"][K - 1]
    assert got["topk_boxes"][:, 0].tobytes() == em["pred_boxes"].cpu().numpy().tobytes()
    assert got["topk_scores"][:, 0].tobytes() == em["pred_scores"].cpu().numpy().tobytes()
    assert np.array_equal(got["topk_idx"][:, 0], ev.pred_idx.cpu().numpy()) and got["acc_at"][0] == em["Acc"].item()
    # predict (no annot) gives the boxes of the annotated call
    for k in ("topk_boxes", "topk_scores", "topk_n"):
        assert pr[k].cpu().numpy().tobytes() == em[k].cpu().numpy().tobytes(), k


def test_eval_topk_1_is_todays_evaluator(M, gold):
    c = topk_ref.load_case(gold("g17_topk"), "b16")
    d = _dev(c)
    _, config, evaluator = M
    cfg = config.get_cfg()
    assert cfg["eval_topk"] == 1
    ev = evaluator.get_default_eval(*config.ratios_scales(cfg), cfg)
    ev.anchs = d["anchors"]
    out = dict(att_bbx_out=d["out5"], feat_sizes=None, num_f_out=torch.tensor([1]))
    inp = dict(annot=d["annot"], img_size=d["img_size"], idxs=torch.arange(16).float().cuda())
    for mode in (ev.train, ev.eval):
        mode()
        assert set(ev(out, inp)) == TODAY and ev.met_keys == ["Acc", "MaxPos"]


def test_bad_arguments_return_minus_one_and_launch_nothing(M, gold):
    L, *_ = M
    c = topk_ref.load_case(gold("g17_topk"), "b1")
    d = _dev(c)
    for pre_n, K, word in ((0, 1, "pre_n"), (513, 5, "pre_n"), (128, 65, "K="), (4, 5, "exceeds")):
        rc, got = _raw_topk(L, c, d, pre_n=pre_n, K=K)
        assert rc == -1 and word in L.lib.zsg_last_error().decode(), (pre_n, K, L.lib.zsg_last_error())
        assert all((v == -7).all() for v in got.values())              # no output was written
    o = torch.empty(64, device="cuda")
    p = o.data_ptr()
    assert L.lib.zsg_eval_topk(d["out5"].data_ptr(), None, d["anchors"].data_ptr(), d["img_size"].data_ptr(), 1, 756, 128, 5, 0.5, 0.5,
                               None, p, p, p, None, None, p, L.stream_ptr()) == -1
    assert "null" in L.lib.zsg_last_error().decode()
    with pytest.raises(L.ZsgError, match="exceeds"):
        ev = _ev(M, dict(c, K=5, pre_n=4))
        ev.anchs = d["anchors"]
        ev.predict(dict(att_bbx_out=d["out5"]), dict(img_size=d["img_size"]))


def test_learner_validate_reports_acc_at_k(M, tmp_path):
    from oracle import zsg_oracle as O
    from zsgnet_pytorch_amd import loss, mdl, synth
    from zsgnet_pytorch_amd.trainer import Learner
    _, config, evaluator = M
    cfg = config.get_cfg(eval_topk=5, resnet_arch="resnet18", resize_img=[96, 96], bs=4, bsv=4, steps_per_epoch=15, tmp_path=str(tmp_path))
    net = mdl.get_default_net(9, cfg)
    net.load_state_dict(O.seeded_state_dict("resnet18", 2))
    net.to("cuda")
    r, s = config.ratios_scales(cfg)
    lf, ev = loss.get_default_loss(r, s, cfg), evaluator.get_default_eval(r, s, cfg)
    learn = Learner("topk", synth.get_data(cfg), net, lf, cfg, ev, None)
    assert learn.met_keys == ["Acc", "MaxPos", "Acc@5"]
    res, preds = learn.validate(with_predictions=True)
    print("validate", res)
    assert not ev.training and set(res) == set(lf.loss_keys) | {"Acc", "MaxPos", "Acc@5"}
    assert 0.0 <= res["Acc"] <= res["Acc@5"] <= 1.0
    assert len(preds) == 12
    for p in preds:
        n = len(p["topk_boxes"])
        assert 1 <= n <= 5 and len(p["topk_scores"]) == n and all(len(b) == 4 for b in p["topk_boxes"])
        assert p["topk_boxes"][0] == p["pred_boxes"] and p["topk_scores"][0] == p["pred_scores"]
        assert all(a >= b for a, b in zip(p["topk_scores"], p["topk_scores"][1:]))
    learn.update_prediction_file(preds, tmp_path / "p.pkl")
    import pickle
    with open(tmp_path / "p.pkl", "rb") as f:
        assert pickle.load(f) == preds
