"""GPU parity of the Soft-NMS selection (csrc/softnms.hip: zsg_eval_topk_soft) through the raw C ABI against tests/softnms_ref.py, on the
inputs and the case grid of tests/softnms_cases.py (tests/test_cpu_softnms.py shows on the reference alone that no pick, threshold
compare, stop or hit decision of any case lies near a tie, so the selection is required exactly).

Exact: topk_idx, topk_n, rows past topk_n, hit_rank, acc_at; row 0 bit-identical to zsg_eval (the NaN score of an all-NaN query: to the
hard call's row 0); every emitted box bit-identical to the box
zsg_eval_topk emits for the same anchor (taken from a hard call with nms_thr = 1, K = min(pre_n, 64), where the anchor is among its
rows); linear rows whose candidate was never decayed carry that call's score bits.
topk_scores differ from the fp64 reference only through the device's expf in the score and the decode: the largest |difference| over
all cases was measured on an MI355X (profiles/softnms_parity_measured.txt), the bound is 4 x that."""
import numpy as np
import pytest
import torch

import softnms_cases as C

pytestmark = pytest.mark.gpu

F32 = np.float32
MEASURED = 8.940697e-08          # largest |topk_scores - softnms_ref| over CASES (profiles/softnms_parity_measured.txt)
BOUND = 4 * MEASURED
METHOD = {"soft_linear": 1, "soft_gauss": 2}
OUT_NAMES = ("topk_boxes", "topk_scores", "topk_idx", "topk_n", "hit_rank", "acc_at")


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def dev():
    """the inputs of every (table, method) on the device, and what the hard calls return for them (filled on demand)"""
    return {}


def on_device(dev, table, method):
    key = (table, method)
    if key not in dev:
        d = C.inputs(table, method)
        dev[key] = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in ("out5", "annot", "img_size", "anchors")}
    return dev[key]


def run(L, d, case, with_annot=True, **bad):
    """one zsg_eval_topk_soft call on sentinel-filled outputs -> (rc, the outputs and the workspace on the host)"""
    _, method, p, k, thr, sig, floor = case
    B, A, _ = d["out5"].shape
    o = dict(topk_boxes=torch.full((B, k, 4), -7.0, device="cuda"), topk_scores=torch.full((B, k), -7.0, device="cuda"),
             topk_idx=torch.full((B, k), -7, dtype=torch.int32, device="cuda"), topk_n=torch.full((B,), -7, dtype=torch.int32, device="cuda"),
             hit_rank=torch.full((B,), -7, dtype=torch.int32, device="cuda"), acc_at=torch.full((k,), -7.0, device="cuda"))
    nb = int(L.lib.zsg_eval_topk_soft_workspace_bytes(B, A, p, k))
    ws = torch.zeros(max(1, nb // 8), dtype=torch.int64, device="cuda")
    a = dict(out5=d["out5"].data_ptr(), annot=d["annot"].data_ptr() if with_annot else None, anchors=d["anchors"].data_ptr(),
             img_size=d["img_size"].data_ptr(), B=B, A=A, pre_n=p, K=k, nms_thr=thr, acc_thr=C.ACC_THR, method=METHOD[method], sigma=sig,
             min_score=floor, tb=o["topk_boxes"].data_ptr(), ts=o["topk_scores"].data_ptr(), ti=o["topk_idx"].data_ptr(),
             tn=o["topk_n"].data_ptr(), hit=o["hit_rank"].data_ptr() if with_annot else None,
             acc=o["acc_at"].data_ptr() if with_annot else None, ws=ws.data_ptr(), ws_bytes=nb)
    a.update(bad)
    rc = L.lib.zsg_eval_topk_soft(a["out5"], a["annot"], a["anchors"], a["img_size"], a["B"], a["A"], a["pre_n"], a["K"], a["nms_thr"],
                                  a["acc_thr"], a["method"], a["sigma"], a["min_score"], a["tb"], a["ts"], a["ti"], a["tn"], a["hit"],
                                  a["acc"], a["ws"], a["ws_bytes"], L.stream_ptr())
    torch.cuda.synchronize()
    got = {n: v.cpu().numpy() for n, v in o.items()}
    got["ws"] = ws.cpu().numpy()
    return rc, got


def hard_rows(L, dev, table, method, p):
    """zsg_eval_topk with nms_thr = 1 and K = min(pre_n, 64) (nothing suppressed: the first K candidates as the hard call emits them) and
    zsg_eval's arg-max row, once per (table, method, pre_n) -> (per query {anchor: (box bits, score bits)}, pred_boxes, pred_scores, pred_idx)"""
    key = ("hard", table, method, p)
    if key not in dev:
        d = on_device(dev, table, method)
        B, A, _ = d["out5"].shape
        k = min(p, 64)
        tb, ts = torch.empty(B, k, 4, device="cuda"), torch.empty(B, k, device="cuda")
        ti, tn = torch.empty(B, k, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
        ws = torch.empty(max(1, int(L.lib.zsg_eval_topk_workspace_bytes(B, A, p, k)) // 8), dtype=torch.int64, device="cuda")
        L.check(L.lib.zsg_eval_topk(d["out5"].data_ptr(), None, d["anchors"].data_ptr(), d["img_size"].data_ptr(), B, A, p, k, 1.0, C.ACC_THR,
                                    tb.data_ptr(), ts.data_ptr(), ti.data_ptr(), tn.data_ptr(), None, None, ws.data_ptr(), L.stream_ptr()),
                "zsg_eval_topk")
        met, pb, ps = torch.empty(2, device="cuda"), torch.empty(B, 4, device="cuda"), torch.empty(B, device="cuda")
        pi, bi = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
        ews = torch.empty((int(L.lib.zsg_eval_workspace_bytes(B)) + 3) // 4, device="cuda")
        L.check(L.lib.zsg_eval(d["out5"].data_ptr(), d["annot"].data_ptr(), d["anchors"].data_ptr(), d["img_size"].data_ptr(), B, A, C.ACC_THR,
                               met.data_ptr(), pb.data_ptr(), ps.data_ptr(), pi.data_ptr(), bi.data_ptr(), ews.data_ptr(), L.stream_ptr()),
                "zsg_eval")
        torch.cuda.synchronize()
        tb, ts, ti, tn = tb.cpu().numpy(), ts.cpu().numpy(), ti.cpu().numpy(), tn.cpu().numpy()
        rows = [{int(ti[b, r]): (tb[b, r].tobytes(), ts[b, r].tobytes()) for r in range(int(tn[b]))} for b in range(B)]
        dev[key] = (rows, pb.cpu().numpy(), ps.cpu().numpy(), pi.cpu().numpy())
    return dev[key]


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_soft_nms_matches_the_definition(L, dev, case):
    table, method, p, k, thr, sig, floor = case
    want = C.reference(case)
    d = on_device(dev, table, method)
    rc, got = run(L, d, case)
    assert rc == 0, L.lib.zsg_last_error()
    for name in ("topk_idx", "topk_n", "hit_rank"):
        print(name, got[name].tolist(), "want", want[name].tolist())
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name
    assert np.array_equal(got["acc_at"], want["acc_at"])
    past = np.arange(k)[None, :] >= want["topk_n"][:, None]
    assert (got["topk_boxes"][past] == 0).all() and (got["topk_scores"][past] == 0).all() and (got["topk_idx"][past] == -1).all()
    # row 0 is zsg_eval's prediction, bit for bit; every emitted box and every never-decayed linear score is the hard call's, bit for bit
    rows, pb, ps, pi = hard_rows(L, dev, table, method, p)
    assert got["topk_boxes"][:, 0].tobytes() == pb.tobytes() and np.array_equal(got["topk_idx"][:, 0], pi)
    # (the score of a query whose logits are all NaN is NaN in both top-k entries — the candidate's own score — where zsg_eval leaves
    # its arg-max's initial value: that row is held to the hard call's row 0 below, every other row to zsg_eval)
    some = ~np.isnan(C.inputs(table, method)["out5"][..., 4]).all(axis=1)
    assert got["topk_scores"][some, 0].tobytes() == ps[some].tobytes()
    for b in np.flatnonzero(~some):
        assert got["topk_scores"][b, 0].tobytes() == rows[b][int(pi[b])][1] and np.isnan(got["topk_scores"][b, 0])
    seen = 0
    for b in range(got["topk_n"].shape[0]):
        for r in range(int(got["topk_n"][b])):
            a = int(got["topk_idx"][b, r])
            if a not in rows[b]:
                continue
            seen += 1
            assert got["topk_boxes"][b, r].tobytes() == rows[b][a][0], (b, r, a)
            if method == "soft_linear" and want["trace"][b]["clean"][r]:
                assert got["topk_scores"][b, r].tobytes() == rows[b][a][1], (b, r, a)
    assert seen >= got["topk_n"].shape[0], "at least every row 0 is among the hard call's rows"
    # the scores within the measured bound
    assert np.array_equal(np.isnan(got["topk_boxes"]), np.isnan(want["topk_boxes"]))
    assert np.array_equal(np.isnan(got["topk_scores"]), np.isnan(want["topk_scores"]))
    fin = ~np.isnan(want["topk_scores"])
    err = float(np.abs(got["topk_scores"].astype(np.float64) - want["topk_scores"].astype(np.float64))[fin].max(initial=0.0))
    print(f"PARITY case={C.case_id(case)} max|topk_scores - ref| = {err:.6e} (bound {BOUND:.6e})")
    assert err <= BOUND
    # without annot: the same rows, hit_rank / acc_at not written
    rc, bare = run(L, d, case, with_annot=False)
    assert rc == 0, L.lib.zsg_last_error()
    for name in ("topk_boxes", "topk_scores", "topk_idx", "topk_n"):
        assert bare[name].tobytes() == got[name].tobytes(), name
    assert (bare["hit_rank"] == -7).all() and (bare["acc_at"] == -7).all()


@pytest.mark.parametrize("case", [("pooled", "soft_linear", 512, 64, 0.3, 0.5, 0.0), ("pooled", "soft_gauss", 257, 64, 0.5, 0.25, 0.001),
                                  ("cell", "soft_gauss", 16, 5, 0.5, 0.5, 0.0)], ids=C.case_id)
def test_twice_the_same_bits(L, dev, case):
    d = on_device(dev, case[0], case[1])
    rc, a = run(L, d, case)
    rc2, b = run(L, d, case)
    assert rc == 0 and rc2 == 0
    for name in OUT_NAMES:
        assert a[name].tobytes() == b[name].tobytes(), name


@pytest.mark.parametrize("bad,word", [(dict(out5=None), "null"), (dict(anchors=None), "null"), (dict(img_size=None), "null"),
                                      (dict(tb=None), "null"), (dict(ts=None), "null"), (dict(ti=None), "null"), (dict(tn=None), "null"),
                                      (dict(ws=None), "null"), (dict(B=0), "B="), (dict(B=65536), "B="), (dict(A=0), "A="),
                                      (dict(pre_n=0), "pre_n"), (dict(pre_n=513), "pre_n"), (dict(K=0), "K="), (dict(K=65, pre_n=128), "K="),
                                      (dict(K=9, pre_n=8), "K="), (dict(method=0), "method"), (dict(method=3), "method"),
                                      (dict(nms_thr=-0.1), "nms_thr"), (dict(nms_thr=1.5), "nms_thr"), (dict(nms_thr=float("nan")), "nms_thr"),
                                      (dict(sigma=0.0), "sigma"), (dict(sigma=-1.0), "sigma"), (dict(sigma=float("inf")), "sigma"),
                                      (dict(sigma=float("nan")), "sigma"), (dict(min_score=-0.1), "min_score"), (dict(min_score=1.0), "min_score"),
                                      (dict(min_score=float("nan")), "min_score"), (dict(annot=None), "annot"), (dict(hit=None), "hit_rank"),
                                      (dict(ws_bytes=8), "ws_bytes"), (dict(ws="odd"), "aligned")],
                         ids=lambda v: "-".join(f"{k}" for k in v) if isinstance(v, dict) else None)
def test_bad_arguments_return_minus_one_and_write_nothing(L, dev, bad, word):
    case = ("pooled", "soft_linear", 8, 5, 0.5, 0.5, 0.001)
    d = on_device(dev, "pooled", "soft_linear")
    if bad.get("ws") == "odd":
        spare = torch.zeros(1024, dtype=torch.int64, device="cuda")          # large enough for the case, four bytes off
        bad = dict(ws=spare.data_ptr() + 4, ws_bytes=8 * 1000)
    rc, got = run(L, d, case, **bad)
    assert rc == -1
    assert word in L.lib.zsg_last_error().decode()
    assert (got["topk_boxes"] == -7).all() and (got["topk_scores"] == -7).all() and (got["topk_idx"] == -7).all()
    assert (got["topk_n"] == -7).all() and (got["hit_rank"] == -7).all() and (got["acc_at"] == -7).all()
    assert (got["ws"] == 0).all()
