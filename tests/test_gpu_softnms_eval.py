"""The Evaluator with cfg eval_nms = soft_linear / soft_gauss on a synthetic output dict (no network): the pooled table of
tests/softnms_cases.py handed over once as a plain six-level output and once as a two-pass multi-scale output (`tta_att_bbx_out` /
`tta_feat_sizes`), against tests/softnms_ref.py at the grid case (pre_n 64, K 5, nms_thr 0.5, sigma 0.5, min_score 0.001) that
tests/test_cpu_softnms.py shows to be safe to compare exactly; predict; training mode; voting over soft rows; and eval_nms = "hard",
which returns what the raw zsg_eval / zsg_eval_topk / zsg_eval_vote calls of the evaluator before the switch return, bit for bit."""
import numpy as np
import pytest
import torch

import softnms_cases as C
from test_gpu_softnms import BOUND

pytestmark = pytest.mark.gpu

K, PRE = 5, 64
A0 = 9 * (16 + 4 + 1)            # the anchors of the first pass's three levels


@pytest.fixture(scope="module")
def Z():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib, config, evaluator
    return dict(L=_lib, config=config, evaluator=evaluator)


def make_eval(Z, **over):
    cfg = Z["config"].get_cfg(eval_pre_nms=PRE, **over)
    return Z["evaluator"].get_default_eval(*Z["config"].ratios_scales(cfg), cfg).eval()


def dicts(method):
    """-> (the plain output dict, the two-pass output dict, inp) of the pooled samples listed for the method"""
    d = C.inputs("pooled", method)
    o5 = torch.from_numpy(d["out5"]).cuda()
    B = o5.shape[0]
    plain = dict(att_bbx_out=o5, feat_sizes=torch.tensor(C.LEVELS))
    tta = dict(att_bbx_out=o5[:, :A0].contiguous(), feat_sizes=torch.tensor(C.LEVELS[:3]), tta_att_bbx_out=o5,
               tta_feat_sizes=[C.LEVELS[:3], C.LEVELS[3:]])
    inp = dict(annot=torch.from_numpy(d["annot"]).cuda(), img_size=torch.from_numpy(d["img_size"]).cuda(), idxs=torch.arange(B).cuda())
    return plain, tta, inp


def _np(d):
    return {k: v.detach().cpu().numpy() for k, v in d.items() if torch.is_tensor(v)}


def _bits_equal(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("method", ["soft_linear", "soft_gauss"])
def test_soft_rows_match_the_definition_plain_and_two_pass(Z, method):
    want = C.reference(("pooled", method, PRE, K, 0.5, 0.5, 0.001))
    plain, tta, inp = dicts(method)
    ev = make_eval(Z, eval_nms=method, eval_topk=K)
    assert ev.met_keys == ["Acc", "MaxPos", f"Acc@{K}"]
    em = ev(plain, inp)
    pr = ev.predict(plain, inp)
    torch.cuda.synchronize()
    assert np.array_equal(ev.anchs.cpu().numpy(), C.inputs("pooled", method)["anchors"]), "the evaluator scores against the cases' table"
    got = _np(em)
    assert set(got) == {"Acc", "MaxPos", "idxs", "pred_boxes", "pred_scores", "topk_boxes", "topk_scores", "topk_n", "hit_rank", f"Acc@{K}"}
    print("topk_idx", ev.topk_idx.tolist(), "want", want["topk_idx"].tolist(), "hit", got["hit_rank"].tolist(), want["hit_rank"].tolist())
    assert np.array_equal(ev.topk_idx.cpu().numpy(), want["topk_idx"]) and np.array_equal(got["topk_n"], want["topk_n"])
    assert np.array_equal(got["hit_rank"], want["hit_rank"]) and np.array_equal(ev.acc_at.cpu().numpy(), want["acc_at"])
    assert got[f"Acc@{K}"] == want["acc_at"][K - 1]
    assert got["topk_boxes"][:, 0].tobytes() == got["pred_boxes"].tobytes() and got["topk_scores"][:, 0].tobytes() == got["pred_scores"].tobytes()
    assert np.array_equal(np.isnan(got["topk_scores"]), np.isnan(want["topk_scores"]))
    fin = ~np.isnan(want["topk_scores"])
    err = float(np.abs(got["topk_scores"].astype(np.float64) - want["topk_scores"].astype(np.float64))[fin].max(initial=0.0))
    print(f"PARITY evaluator {method} max|topk_scores - ref| = {err:.6e} (bound {BOUND:.6e})")
    assert err <= BOUND
    assert set(pr) == {"topk_boxes", "topk_scores", "topk_n"}
    for k in pr:
        assert torch.equal(pr[k].view(torch.int32), em[k].view(torch.int32)), k
    # the same table as two passes of a multi-scale forward: the same rows, bit for bit; self.anchs stays pass 0's table
    ev2 = make_eval(Z, eval_nms=method, eval_topk=K)
    em2 = ev2(tta, inp)
    pr2 = ev2.predict(tta, inp)
    torch.cuda.synchronize()
    assert tuple(ev2.anchs.shape) == (A0, 4) and len(ev2._tta_anchs) == 1
    _bits_equal(got, _np(em2))
    assert torch.equal(ev2.topk_idx, ev.topk_idx) and torch.equal(pr2["topk_boxes"].view(torch.int32), pr["topk_boxes"].view(torch.int32))


class _Counting:
    """the ctypes library, every call counted by name and passed on"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        self.calls.append(name)
        return fn


def test_training_mode_and_topk_1_launch_no_topk(Z, monkeypatch):
    plain, _, inp = dicts("soft_linear")
    spy = _Counting(Z["L"].lib)
    monkeypatch.setattr(Z["evaluator"], "lib", spy)
    ev = make_eval(Z, eval_nms="soft_gauss", eval_topk=K, eval_box_vote=0.6)
    ev.train()
    assert set(ev(plain, inp)) == {"Acc", "MaxPos", "idxs", "pred_boxes", "pred_scores"}
    assert set(make_eval(Z, eval_nms="soft_gauss")(plain, inp)) == {"Acc", "MaxPos", "idxs", "pred_boxes", "pred_scores"}
    assert spy.calls == ["zsg_eval_workspace_bytes", "zsg_eval"] * 2
    ev.eval()(plain, inp)
    torch.cuda.synchronize()
    assert spy.calls[4:] == ["zsg_eval_workspace_bytes", "zsg_eval", "zsg_eval_topk_soft_workspace_bytes", "zsg_eval_topk_soft",
                             "zsg_eval_vote_workspace_bytes", "zsg_eval_vote"]


@pytest.mark.parametrize("method,thr", [("soft_linear", 0.3), ("soft_gauss", 0.5)])
def test_voting_reads_soft_rows_as_it_reads_hard_ones(Z, method, thr):
    """zsg_eval_vote does not read topk_scores and votes over all candidates: an anchor kept by both pipelines gets the same voted box
    (linear at eval_nms_thr 0.3: at 0.5 its first five rows on these inputs are the hard rule's)"""
    plain, _, inp = dicts(method)
    evh = make_eval(Z, eval_topk=K, eval_box_vote=0.6, eval_nms_thr=thr)
    evs = make_eval(Z, eval_nms=method, eval_topk=K, eval_box_vote=0.6, eval_nms_thr=thr)
    h, s = _np(evh(plain, inp)), _np(evs(plain, inp))
    torch.cuda.synchronize()
    assert set(h) == set(s) and "vote_n" in s and "topk_boxes_raw" in s
    hi, si = evh.topk_idx.cpu().numpy(), evs.topk_idx.cpu().numpy()
    both = 0
    for b in range(hi.shape[0]):
        for r in range(int(s["topk_n"][b])):
            at = np.nonzero(hi[b, :int(h["topk_n"][b])] == si[b, r])[0]
            if at.size:
                both += 1
                assert s["topk_boxes"][b, r].tobytes() == h["topk_boxes"][b, at[0]].tobytes(), (b, r)
                assert s["vote_n"][b, r] == h["vote_n"][b, at[0]] and s["topk_boxes_raw"][b, r].tobytes() == h["topk_boxes_raw"][b, at[0]].tobytes()
    assert both > hi.shape[0], "more than the arg-max rows are shared"
    assert not np.array_equal(hi, si), "and the two rules really keep different rows"
    assert s["pred_boxes"].tobytes() == h["pred_boxes"].tobytes() and s["pred_boxes_raw"].tobytes() == h["pred_boxes_raw"].tobytes()
    want = C.reference(("pooled", method, PRE, K, thr, 0.5, 0.001))
    assert np.array_equal(si, want["topk_idx"]), "the rows under the vote are the soft rows"


def test_hard_is_what_the_evaluator_did_before_the_switch(Z):
    """eval_nms = "hard" (given, defaulted, or missing from the cfg): the dict of the raw calls the evaluator made before the key existed"""
    L = Z["L"]
    plain, tta, inp = dicts("soft_linear")
    o5, annot, sz = plain["att_bbx_out"], inp["annot"], inp["img_size"]
    B, A, _ = o5.shape
    anc = torch.from_numpy(C.inputs("pooled", "soft_linear")["anchors"]).cuda()
    met, pb, ps = torch.empty(2, device="cuda"), torch.empty(B, 4, device="cuda"), torch.empty(B, device="cuda")
    pi, bi = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    ews = torch.empty((int(L.lib.zsg_eval_workspace_bytes(B)) + 3) // 4, device="cuda")
    L.check(L.lib.zsg_eval(o5.data_ptr(), annot.data_ptr(), anc.data_ptr(), sz.data_ptr(), B, A, 0.5, met.data_ptr(), pb.data_ptr(), ps.data_ptr(),
                           pi.data_ptr(), bi.data_ptr(), ews.data_ptr(), L.stream_ptr()), "zsg_eval")
    tb, ts = torch.empty(B, K, 4, device="cuda"), torch.empty(B, K, device="cuda")
    ti, tn = torch.empty(B, K, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    hit, acc = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(K, device="cuda")
    ws = torch.empty(int(L.lib.zsg_eval_topk_workspace_bytes(B, A, PRE, K)) // 8, dtype=torch.int64, device="cuda")
    L.check(L.lib.zsg_eval_topk(o5.data_ptr(), annot.data_ptr(), anc.data_ptr(), sz.data_ptr(), B, A, PRE, K, 0.5, 0.5, tb.data_ptr(), ts.data_ptr(),
                                ti.data_ptr(), tn.data_ptr(), hit.data_ptr(), acc.data_ptr(), ws.data_ptr(), L.stream_ptr()), "zsg_eval_topk")
    torch.cuda.synchronize()
    want = _np({"Acc": met[0], "MaxPos": met[1], "idxs": inp["idxs"], "pred_boxes": pb, "pred_scores": ps, "topk_boxes": tb, "topk_scores": ts,
                "topk_n": tn, "hit_rank": hit, f"Acc@{K}": acc[K - 1]})
    cfg = Z["config"].get_cfg(eval_pre_nms=PRE, eval_topk=K)
    del cfg["eval_nms"], cfg["eval_soft_sigma"], cfg["eval_soft_min_score"]
    bare = Z["evaluator"].get_default_eval(*Z["config"].ratios_scales(cfg), cfg).eval()
    for ev in (make_eval(Z, eval_topk=K), make_eval(Z, eval_topk=K, eval_nms="hard", eval_soft_sigma=0.1, eval_soft_min_score=0.5), bare):
        for out in (plain, tta):
            got = _np(ev(out, inp))
            torch.cuda.synchronize()
            _bits_equal(got, want)
            assert torch.equal(ev.topk_idx, ti) and torch.equal(ev.pred_idx, pi) and torch.equal(ev.best_idx, bi)
    # ... and under the vote
    vb, vn = torch.empty(B, K, 4, device="cuda"), torch.empty(B, K, dtype=torch.int32, device="cuda")
    vhit, vacc = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(K, device="cuda")
    nb = int(L.lib.zsg_eval_vote_workspace_bytes(B, A, PRE, K))
    vws = torch.empty(nb // 8, dtype=torch.int64, device="cuda")
    L.check(L.lib.zsg_eval_vote(o5.data_ptr(), annot.data_ptr(), anc.data_ptr(), sz.data_ptr(), B, A, PRE, K, 0.6, 0.5, tb.data_ptr(), ts.data_ptr(),
                                ti.data_ptr(), tn.data_ptr(), vb.data_ptr(), vn.data_ptr(), vhit.data_ptr(), vacc.data_ptr(), vws.data_ptr(), nb,
                                L.stream_ptr()), "zsg_eval_vote")
    torch.cuda.synchronize()
    wantv = dict(want, **_np({"topk_boxes": vb, "topk_boxes_raw": tb, "vote_n": vn, "hit_rank": vhit, f"Acc@{K}": vacc[K - 1], "Acc": vacc[0],
                              "pred_boxes": vb[:, 0], "pred_boxes_raw": pb}))
    _bits_equal(_np(make_eval(Z, eval_topk=K, eval_box_vote=0.6, eval_nms="hard")(plain, inp)), wantv)
