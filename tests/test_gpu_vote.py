"""GPU parity of score-weighted box voting (csrc/vote.hip: zsg_eval_vote) through the raw C ABI against tests/vote_ref.py.

Shapes: the pooled anchor table of a two-pass multi-scale forward — levels (4,4),(2,2),(1,1) plus (5,5),(3,3),(2,2), nine anchors a cell,
A = 531 — and B = 3 queries whose regressions are noise around zero, so that neighbouring anchors, and the two passes, really overlap.
Sample 0 carries an isolated tiny box with the best score (a kept row with no other member), sample 1 equal logits everywhere (ties go
to the lower index), sample 2 anchors with NaN logits and one with a NaN regression.

Exact: vote_n, the untouched topk_* arrays, rows past topk_n, hit_rank and acc_at (the reference alone shows that no voted IoU lies within
1e-6 of acc_thr, asserted below; decode and IoU are the evaluator's bit-exact expressions, as for g3_iou / g17_topk).
Voted coordinates differ from the fp64 reference only through the device's expf in the scores and the decode: the largest |difference|
over all cases was measured on an MI355X (profiles/tta_ms_parity_measured.txt), the bound is 4 x that."""
import itertools

import numpy as np
import pytest
import torch

import topk_ref
import vote_ref
from oracle import zsg_oracle as O

pytestmark = pytest.mark.gpu

F32 = np.float32
LEVELS = [(4, 4), (2, 2), (1, 1), (5, 5), (3, 3), (2, 2)]
MEASURED_PX = 1.220703e-04       # largest |voted - vote_ref| in pixels over CASES (profiles/tta_ms_parity_measured.txt)
BOUND_PX = 4 * MEASURED_PX
NMS_THR, ACC_THR = 0.5, 0.5
CASES = [(p, k, t) for p, k, t in itertools.product((1, 8, 128), (1, 3, 5), (0.5, 0.75, 1.0)) if k <= p]


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib
    return _lib


def make_inputs():
    ratios, scales = O.default_ratios_scales()
    anchors = O.create_anchors(LEVELS, ratios, scales).astype(F32)
    A = anchors.shape[0]
    assert A == 531
    g = torch.Generator().manual_seed(20)
    att = (torch.randn(3, A, generator=g) * 1.5 - 3.0).numpy()
    reg = (torch.randn(3, A, 4, generator=g) * 0.08).numpy()
    att[0, 40], reg[0, 40] = 6.0, (0.3, -0.2, -3.0, -3.0)          # the best score of sample 0 on a box no other candidate overlaps
    att[1, :] = -1.25                                               # ties everywhere: candidates are anchors 0 .. pre_n - 1
    att[2, [3, 100, 317]] = np.nan
    att[2, 200], reg[2, 200, 2] = 5.0, np.nan                       # a finite best score on a box that does not decode
    img_size = np.array([[360, 480], [300, 300], [333, 500]], F32)
    # annotations that some kept rows hit: the voted boxes of rows 2 / 0 / 1 at (pre_n 128, K 5, thr 0.5), back in [-1, 1], rounded to 2 digits
    w = vote_ref.vote(att, reg, None, img_size, anchors, 128, 5, 0.5, NMS_THR, ACC_THR)["vote_boxes"]
    px = np.stack([w[0, 2], w[1, 0], w[2, 1]])
    annot = np.round(np.stack([px[:, 1] / img_size[:, 0], px[:, 0] / img_size[:, 1], px[:, 3] / img_size[:, 0], px[:, 2] / img_size[:, 1]],
                              axis=1) * 2 - 1, 2)
    out5 = np.concatenate([reg, att[..., None]], axis=2).astype(F32)
    return dict(out5=out5, annot=annot.astype(F32), img_size=img_size, anchors=anchors)


@pytest.fixture(scope="module")
def data():
    d = make_inputs()
    d["dev"] = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in ("out5", "annot", "img_size", "anchors")}
    d["ref"] = {}
    return d


def ref_for(data, case):
    if case not in data["ref"]:
        p, k, t = case
        o = data["out5"]
        data["ref"][case] = vote_ref.vote(o[..., 4], o[..., :4], data["annot"], data["img_size"], data["anchors"], p, k, t, NMS_THR, ACC_THR)
    return data["ref"][case]


def run(L, dev, case, with_annot=True, **bad):
    """zsg_eval_topk then zsg_eval_vote -> (rc of the vote, outputs on the host, the topk outputs before the vote)"""
    p, k, t = case
    B, A, _ = dev["out5"].shape
    tk = dict(topk_boxes=torch.empty(B, k, 4, device="cuda"), topk_scores=torch.empty(B, k, device="cuda"),
              topk_idx=torch.empty(B, k, dtype=torch.int32, device="cuda"), topk_n=torch.empty(B, dtype=torch.int32, device="cuda"))
    ws = torch.empty(max(1, int(L.lib.zsg_eval_topk_workspace_bytes(B, A, p, k)) // 8), dtype=torch.int64, device="cuda")
    L.check(L.lib.zsg_eval_topk(dev["out5"].data_ptr(), None, dev["anchors"].data_ptr(), dev["img_size"].data_ptr(), B, A, p, k, NMS_THR,
                                ACC_THR, tk["topk_boxes"].data_ptr(), tk["topk_scores"].data_ptr(), tk["topk_idx"].data_ptr(),
                                tk["topk_n"].data_ptr(), None, None, ws.data_ptr(), L.stream_ptr()), "zsg_eval_topk")
    before = {n: v.clone() for n, v in tk.items()}
    o = dict(vote_boxes=torch.full((B, k, 4), -7.0, device="cuda"), vote_n=torch.full((B, k), -7, dtype=torch.int32, device="cuda"),
             hit_rank=torch.full((B,), -7, dtype=torch.int32, device="cuda"), acc_at=torch.full((k,), -7.0, device="cuda"))
    nb = int(L.lib.zsg_eval_vote_workspace_bytes(B, A, p, k))
    vws = torch.zeros(max(1, nb // 8), dtype=torch.int64, device="cuda")
    a = dict(out5=dev["out5"].data_ptr(), annot=dev["annot"].data_ptr() if with_annot else None, anchors=dev["anchors"].data_ptr(),
             img_size=dev["img_size"].data_ptr(), B=B, A=A, pre_n=p, K=k, vote_thr=t, acc_thr=ACC_THR, tb=tk["topk_boxes"].data_ptr(),
             ts=tk["topk_scores"].data_ptr(), ti=tk["topk_idx"].data_ptr(), tn=tk["topk_n"].data_ptr(), vb=o["vote_boxes"].data_ptr(),
             vn=o["vote_n"].data_ptr(), hit=o["hit_rank"].data_ptr() if with_annot else None,
             acc=o["acc_at"].data_ptr() if with_annot else None, ws=vws.data_ptr(), ws_bytes=nb)
    a.update(bad)
    rc = L.lib.zsg_eval_vote(a["out5"], a["annot"], a["anchors"], a["img_size"], a["B"], a["A"], a["pre_n"], a["K"], a["vote_thr"],
                             a["acc_thr"], a["tb"], a["ts"], a["ti"], a["tn"], a["vb"], a["vn"], a["hit"], a["acc"], a["ws"], a["ws_bytes"],
                             L.stream_ptr())
    torch.cuda.synchronize()
    got = {n: v.cpu().numpy() for n, v in o.items()}
    got.update({n: v.cpu().numpy() for n, v in tk.items()})
    got["ws"] = vws.cpu().numpy()
    return rc, got, {n: v.cpu().numpy() for n, v in before.items()}


def test_the_inputs_hold_the_special_rows(data):
    """from the reference alone: ties resolved by index, a NaN row that never votes, a kept row that stands alone, and no voted IoU
    within 1e-6 of acc_thr in any case (so hit_rank is required exactly)"""
    for case in CASES:
        w = ref_for(data, case)
        kept = np.arange(case[1])[None, :] < w["topk_n"][:, None]
        assert not (np.abs(w["vote_iou"][kept] - F32(ACC_THR)) <= 1e-6).any(), case          # (a NaN IoU is no hit on either side)
    w = ref_for(data, (128, 5, 0.5))
    assert w["topk_idx"][0, 0] == 40 and w["vote_n"][0, 0] == 1                 # alone
    assert w["vote_n"][0, 1:].max() > 1 and w["vote_n"][2].max() > 1            # neighbouring anchors really vote
    assert w["topk_idx"][1, 0] == 0 and (w["topk_scores"][1, :w["topk_n"][1]] == w["topk_scores"][1, 0]).all()
    assert w["topk_idx"][2, 0] == 200 and w["vote_n"][2, 0] == 0                # the box that does not decode keeps its NaNs, no member
    assert np.isnan(w["vote_boxes"][2, 0]).any()
    assert len({tuple(w["vote_n"].ravel()) for w in (ref_for(data, (128, 5, t)) for t in (0.5, 0.75, 1.0))}) == 3


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"pre{c[0]}-K{c[1]}-thr{c[2]}")
def test_vote_matches_the_definition(L, data, case):
    want = ref_for(data, case)
    rc, got, before = run(L, data["dev"], case)
    assert rc == 0, L.lib.zsg_last_error()
    for k in ("topk_boxes", "topk_scores", "topk_idx", "topk_n"):                # untouched, bit for bit
        assert got[k].tobytes() == before[k].tobytes(), k
    assert np.array_equal(got["topk_idx"], want["topk_idx"]) and np.array_equal(got["topk_n"], want["topk_n"])
    print("vote_n", got["vote_n"].tolist(), "want", want["vote_n"].tolist())
    assert got["vote_n"].dtype == np.int32 and np.array_equal(got["vote_n"], want["vote_n"])
    print("hit_rank", got["hit_rank"].tolist(), "want", want["vote_hit_rank"].tolist())
    assert np.array_equal(got["hit_rank"], want["vote_hit_rank"])
    assert np.array_equal(got["acc_at"], want["vote_acc_at"])
    past = np.arange(case[1])[None, :] >= want["topk_n"][:, None]
    assert (got["vote_boxes"][past] == 0).all() and (got["vote_n"][past] == 0).all()
    assert np.array_equal(np.isnan(got["vote_boxes"]), np.isnan(want["vote_boxes"]))
    fin = np.isfinite(want["vote_boxes"])
    err = float(np.abs(got["vote_boxes"].astype(np.float64) - want["vote_boxes"].astype(np.float64))[fin].max(initial=0.0))
    print(f"PARITY case={case} max|voted - ref| = {err:.6e} px (bound {BOUND_PX:.6e})")
    assert err <= BOUND_PX
    one = want["vote_n"] == 1       # a row that stands alone is the unvoted row, bit for bit: s * x is exact in fp64 and (s * x) / s is x
    assert np.array_equal(got["vote_boxes"][one], got["topk_boxes"][one])


def test_without_annot_and_twice_the_same_bits(L, data):
    case = (128, 5, 0.5)
    rc, a, _ = run(L, data["dev"], case)
    rc2, b, _ = run(L, data["dev"], case)
    rc3, c, _ = run(L, data["dev"], case, with_annot=False)
    assert rc == 0 and rc2 == 0 and rc3 == 0
    for k in ("vote_boxes", "vote_n", "hit_rank", "acc_at"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["vote_boxes"].tobytes() == c["vote_boxes"].tobytes() and a["vote_n"].tobytes() == c["vote_n"].tobytes()
    assert (c["hit_rank"] == -7).all() and (c["acc_at"] == -7).all()               # not written without annot


@pytest.mark.parametrize("bad,word", [(dict(out5=None), "null"), (dict(anchors=None), "null"), (dict(img_size=None), "null"),
                                      (dict(tb=None), "null"), (dict(ts=None), "null"), (dict(ti=None), "null"), (dict(tn=None), "null"),
                                      (dict(vb=None), "null"), (dict(vn=None), "null"), (dict(ws=None), "null"),
                                      (dict(B=0), "B="), (dict(A=0), "A="), (dict(pre_n=0), "pre_n"), (dict(pre_n=513), "pre_n"),
                                      (dict(K=0), "K="), (dict(K=65, pre_n=128), "K="), (dict(K=9, pre_n=8), "K="),
                                      (dict(vote_thr=0.0), "vote_thr"), (dict(vote_thr=1.5), "vote_thr"), (dict(vote_thr=float("nan")), "vote_thr"),
                                      (dict(annot=None), "annot"), (dict(hit=None), "hit_rank"), (dict(ws_bytes=8), "ws_bytes")],
                         ids=lambda v: "-".join(f"{k}" for k in v) if isinstance(v, dict) else None)
def test_bad_arguments_return_minus_one_and_write_nothing(L, data, bad, word):
    rc, got, _ = run(L, data["dev"], (8, 5, 0.5), **bad)
    assert rc == -1
    assert word in L.lib.zsg_last_error().decode()
    assert (got["vote_boxes"] == -7).all() and (got["vote_n"] == -7).all() and (got["hit_rank"] == -7).all() and (got["acc_at"] == -7).all()
    assert (got["ws"] == 0).all()
