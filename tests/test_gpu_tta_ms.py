"""Multi-scale test-time augmentation on the network and in the evaluator: cfg eval_scales / ZSGNet.eval_scales, cfg eval_box_vote.
ResNet-18, base 128 x 128 (the size of g10_e2e_128), B = 2, eval_scales = [0.75, 1.25] (passes at 96 and 160 px), seeded_weights() below,
the uint8 form of O.synthetic_batch(2, 128, 128, seed=3), fixed h0 / c0.  The module runs with ZSG_AUTOTUNE=0 and ZSG_DETERMINISTIC=1 as
tests/test_gpu_tta_net.py does (no tile choice by timing, no fp32 atomics: two forwards of one plan give the same bits).

tests/tta_ms_ref.py is the definition: pass s of the pooled output is the PLAIN eval forward of the same net on Pillow's resize of the
batch's own pixels — bit for bit, in every mode the plain forward has (flip TTA, shared images, bf16) — and the evaluator on the pooled
output is the oracle's evaluator / tests/topk_ref.py / tests/vote_ref.py on the concatenated arrays."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tta_ms_ref as MS  # noqa: E402
from oracle import zsg_oracle as O  # noqa: E402
from test_gpu_vote import BOUND_PX  # noqa: E402

N_ANCH = 9
SCALES = [0.75, 1.25]
SIZES = [(96, 96), (160, 160)]


@pytest.fixture(scope="module")
def Z():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib, config, evaluator, loss, mdl, synth
    return dict(L=_lib, config=config, evaluator=evaluator, loss=loss, mdl=mdl, synth=synth)


@pytest.fixture(scope="module", autouse=True)
def fixed_tiles(Z):
    L = Z["L"]
    old = {k: os.environ.get(k) for k in ("ZSG_DETERMINISTIC", "ZSG_AUTOTUNE")}
    os.environ["ZSG_DETERMINISTIC"], os.environ["ZSG_AUTOTUNE"] = "1", "0"
    L.lib.zsg_set_deterministic(1)
    yield
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    L.lib.zsg_set_deterministic(1 if old["ZSG_DETERMINISTIC"] == "1" else 0)


def seeded_weights():
    """O.seeded_state_dict("resnet18", 1) with the rows of the head's last convolution scaled by powers of two (exact scalings; the
    regression biases are zero, the logit bias stays -4): the four regression rows of every anchor by 2^-7, its logit row by 2^-4.
    He-initialised random weights give dh, dw of order 10 — boxes of 10^5 .. 10^9 pixels that overlap nothing — and logits of +-80,
    whose scores saturate at 1.0 so that the ranking is the anchor index: no detector's output, and nothing for a vote to average.
    Scaled, the regressions are noise around zero (|.| < 1), the decoded boxes are the anchors slightly moved and the scores are
    distinct, so neighbouring anchors and the three passes overlap and compete — the set-up tests/test_gpu_vote.py builds by hand,
    here from a real forward.  The CPU oracle's forward of these weights gives 3 .. 17 members per kept row at vote_thr 0.6."""
    sd = O.seeded_state_dict("resnet18", 1)
    w = sd["att_reg_box.5.weight"]
    rows = w.view(N_ANCH, 5, *w.shape[1:])
    rows[:, :4] *= 2.0 ** -7
    rows[:, 4:] *= 2.0 ** -4
    assert float(sd["att_reg_box.5.bias"].view(N_ANCH, 5)[:, :4].abs().max()) == 0.0
    return sd


def build(Z, **flags):
    cfg = Z["config"].get_cfg(resnet_arch="resnet18", **flags)
    net = Z["mdl"].get_default_net(N_ANCH, cfg)
    net.load_state_dict(seeded_weights())
    return cfg, net.to("cuda")


def to_u8(img):
    return (img.permute(0, 2, 3, 1) * 255).round().to(torch.uint8).contiguous()


def host_batch():
    bt = O.synthetic_batch(2, 128, 128, seed=3)
    g = torch.Generator().manual_seed(0)
    h0, c0 = torch.randn(2, 2, 128, generator=g), torch.randn(2, 2, 128, generator=g)
    bt["qvec_flip"] = torch.randn(bt["qvec"].shape, generator=g) * 0.35
    bt["img"] = to_u8(bt["img"])
    return bt, h0, c0


def dev(bt, h0, c0):
    inp = {k: v.cuda() for k, v in bt.items()}
    inp["h0"], inp["c0"] = h0, c0
    return inp


def run(net, inp):
    with torch.no_grad():
        out = net(inp)
    torch.cuda.synchronize()
    return {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in out.items()}


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def resampled(inp, hw):
    """the batch with its images replaced by the host definition's resize"""
    return dict(inp, img=torch.from_numpy(MS.resample(inp["img"].cpu().numpy(), *hw)).cuda())


def check_passes(net, inp):
    """the multi-scale forward of `net` against its own plain forwards on the host-resampled batches, bit for bit -> the multi-scale dict"""
    ms = run(net, inp)
    net.eval_scales(())
    try:
        plain = [run(net, inp)] + [run(net, resampled(inp, hw)) for hw in SIZES]
    finally:
        net.eval_scales(SCALES)
    assert all("tta_att_bbx_out" not in p and "tta_feat_sizes" not in p for p in plain)
    for k in ("att_bbx_out", "att_out", "bbx_out", "feat_sizes", "num_f_out"):
        assert torch.equal(bits(ms[k]) if ms[k].is_floating_point() else ms[k], bits(plain[0][k]) if ms[k].is_floating_point() else plain[0][k]), k
    A = [p["att_bbx_out"].shape[1] for p in plain]
    Q = plain[0]["att_bbx_out"].shape[0]
    assert tuple(ms["tta_att_bbx_out"].shape) == (Q, sum(A), 5) and len(set(A)) == 3
    assert ms["tta_feat_sizes"] == [[tuple(x) for x in p["feat_sizes"].tolist()] for p in plain]
    assert ms["tta_feat_sizes"] == [O.feat_sizes_for(128, 128)] + [O.feat_sizes_for(*hw) for hw in SIZES]
    off = 0
    for i, p in enumerate(plain):
        assert torch.equal(bits(ms["tta_att_bbx_out"][:, off:off + A[i]]), bits(p["att_bbx_out"])), f"pass {i}"
        off += A[i]
    assert not torch.equal(bits(plain[1]["att_bbx_out"][:, :64]), bits(plain[2]["att_bbx_out"][:, :64])), "the passes differ"
    return ms


@pytest.fixture(scope="module")
def ref(Z, fixed_tiles):
    bt, h0, c0 = host_batch()
    cfg, net = build(Z, eval_scales=SCALES)
    net.eval()
    inp = dev(bt, h0, c0)
    return dict(cfg=cfg, net=net, bt=bt, h0=h0, c0=c0, inp=inp)


def test_a_every_pass_is_the_plain_forward_on_the_resampled_batch(Z, ref):
    net = ref["net"]
    assert net._eval_scales == (0.75, 1.25)
    ms = check_passes(net, ref["inp"])
    ref["ms"] = ms
    assert [k for k in net._plans if not k[-1]] == [(2, 128, 128, 20, False), (2, 96, 96, 20, False), (2, 160, 160, 20, False)]
    again = run(net, ref["inp"])
    assert again["tta_att_bbx_out"].data_ptr() != ms["tta_att_bbx_out"].data_ptr() and torch.equal(bits(again["tta_att_bbx_out"]), bits(ms["tta_att_bbx_out"]))
    # the device resample is the host definition's, byte for byte, and a second batch of the geometry reuses resizer and output batch
    for hw in SIZES:
        got = net._resample(ref["inp"]["img"], *hw)
        assert got.data_ptr() == net._ms_resize[(2, 128, 128) + hw][1].data_ptr()
        assert np.array_equal(got.cpu().numpy(), MS.resample(ref["bt"]["img"].numpy(), *hw))
    assert len(net._ms_resize) == 2


def test_b_with_flip_tta_every_scale_runs_its_own_mirrored_rows_and_merge(Z, ref):
    net = ref["net"]
    net.eval_tta("flip")
    try:
        ms = check_passes(net, ref["inp"])
    finally:
        net.eval_tta("none")
    assert {(4, 128, 128, 20, False), (4, 96, 96, 20, False), (4, 160, 160, 20, False)} <= set(net._plans)
    assert not torch.equal(bits(ms["tta_att_bbx_out"]), bits(ref["ms"]["tta_att_bbx_out"]))


def test_c_shared_image_batch(Z, ref):
    net, mdl = ref["net"], Z["mdl"]
    bt = Z["synth"].synthetic_shared_batch(2, 4, 128, 128, seed=5)
    bt["img"] = to_u8(bt["img"])
    g = torch.Generator().manual_seed(1)
    h0, c0 = torch.randn(2, 4, 128, generator=g), torch.randn(2, 4, 128, generator=g)
    ms = check_passes(net, dev(bt, h0, c0))
    assert tuple(ms["att_bbx_out"].shape)[0] == 4
    shared = [k for k in net._plans if "shared" in k]
    assert sorted(k[2:4] for k in shared) == [(96, 96), (128, 128), (160, 160)]
    # a multi-scale set never evicts its own members: the bound on shared plans counts the passes
    net2 = build(Z, eval_scales=SCALES)[1].eval()
    made = []

    class Fake:
        def __init__(self, *a, **k):
            made.append(a[1:5])
    real, mdl._Plan = mdl._Plan, Fake
    try:
        for T in range(60, 60 + mdl.SHARED_PLANS_MAX):             # SHARED_PLANS_MAX token buckets, three plans each, twice round
            for hw in [(128, 128)] + SIZES:
                net2._plan_for(2, hw[0], hw[1], T, Q=4)
        n = len(made)
        for T in range(60, 60 + mdl.SHARED_PLANS_MAX):
            for hw in [(128, 128)] + SIZES:
                net2._plan_for(2, hw[0], hw[1], T, Q=4)
        assert n == 3 * mdl.SHARED_PLANS_MAX and len(made) == n, "nothing was evicted and lowered again"
        net2._plan_for(2, 128, 128, 99, Q=4)
        assert len([k for k in net2._plans if "shared" in k]) == 3 * mdl.SHARED_PLANS_MAX, "the bound holds"
        net2.eval_scales(())
        net2._plan_for(2, 128, 128, 100, Q=4)
        assert len([k for k in net2._plans if "shared" in k]) == mdl.SHARED_PLANS_MAX, "without the switch the bound is what it was"
    finally:
        mdl._Plan = real


def test_d_bf16_eval_plans(Z, ref):
    net = ref["net"]
    net.eval_precision("bf16")
    try:
        ms = check_passes(net, ref["inp"])
    finally:
        net.eval_precision("fp32")
    assert not torch.equal(bits(ms["tta_att_bbx_out"]), bits(ref["ms"]["tta_att_bbx_out"]))


def test_e_fp32_nchw_images_are_refused_and_unlowerable_sizes_name_the_scale(Z, ref):
    net = ref["net"]
    f32 = dict(ref["inp"], img=ref["inp"]["img"].permute(0, 3, 1, 2).float() / 255)
    with pytest.raises(ValueError, match="uint8"):
        net(f32)
    net.eval_scales(())
    run(net, f32)                                                   # (the plain forward takes it)
    net.eval_scales([0.75, 0.751])
    try:
        with pytest.raises(ValueError, match="eval_scales"):
            net(ref["inp"])
    finally:
        net.eval_scales(SCALES)
    real = net._plan_for

    def refuse(B, H, W, T, Q=None):
        if H == 160:
            raise RuntimeError("no lowering for this size")
        return real(B, H, W, T, Q=Q)
    net._plan_for = refuse
    launched = []
    real_one = net._forward_one
    net._forward_one = lambda inp: launched.append(1) or real_one(inp)
    try:
        with pytest.raises(ValueError, match=r"eval_scales: scale 1\.25 \(160 x 160"):
            net(ref["inp"])
        assert not launched, "refused before any pass ran"
    finally:
        del net._plan_for, net._forward_one


def test_f_training_mode_ignores_the_switch(Z, ref):
    _, never = build(Z)
    _, net = build(Z, eval_scales=SCALES)
    never.train(), net.train()
    inp = ref["inp"]
    with torch.no_grad():
        a, b = never(inp), net(inp)
    torch.cuda.synchronize()
    assert "tta_att_bbx_out" not in b and "tta_feat_sizes" not in b and set(a) == set(b)
    assert torch.equal(bits(a["att_bbx_out"]), bits(b["att_bbx_out"]))
    assert [k[:4] for k in net._plans] == [(2, 128, 128, 20)] and not net._ms_resize


def _np(d):
    return {k: v.detach().cpu().numpy() for k, v in d.items() if torch.is_tensor(v)}


def test_g_evaluator_on_the_pooled_output(Z, ref):
    config, evaluator = Z["config"], Z["evaluator"]
    ms, inp = ref["ms"], ref["inp"]
    cfg = config.get_cfg(resnet_arch="resnet18", eval_scales=SCALES, eval_topk=3)
    r, s = config.ratios_scales(cfg)
    anc = MS.pooled_anchors(ms["tta_feat_sizes"], r, s)
    o5 = ms["tta_att_bbx_out"].cpu().numpy()
    annot, sz = ref["bt"]["annot"].numpy(), ref["bt"]["img_size"].numpy()
    A0 = ms["att_bbx_out"].shape[1]
    ev = evaluator.get_default_eval(r, s, cfg).eval()
    em = ev(ms, inp)
    pr = ev.predict(ms, inp)
    torch.cuda.synchronize()
    got, want = _np(em), MS.evaluate(o5, annot, sz, anc, K=3)
    assert tuple(ev.anchs.shape) == (A0, 4) and np.array_equal(next(iter(ev._tta_anchs.values())).cpu().numpy(), anc)
    print("pred_idx", ev.pred_idx.tolist(), "want", want["pred_ids"].tolist(), "A0", A0, "topk_idx", ev.topk_idx.tolist(), "want", want["topk_idx"].tolist())
    assert ev.pred_idx.cpu().tolist() == want["pred_ids"].tolist() and ev.best_idx.cpu().tolist() == want["best_ids"].tolist()
    assert got["Acc"] == want["Acc"] and got["MaxPos"] == want["MaxPos"]
    np.testing.assert_allclose(got["pred_boxes"], want["pred_boxes"], rtol=1e-5, atol=1e-3)        # (the tolerances of tests/test_gpu_topk.py)
    np.testing.assert_allclose(got["pred_scores"], want["pred_scores"], rtol=1e-6)
    for k in ("topk_idx", "topk_n", "hit_rank"):
        assert np.array_equal(ev.topk_idx.cpu().numpy() if k == "topk_idx" else got[k], want[k]), k
    assert got["Acc@3"] == want["acc_at"][2] and np.array_equal(ev.acc_at.cpu().numpy(), want["acc_at"])
    np.testing.assert_allclose(got["topk_boxes"], want["topk_boxes"], rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(got["topk_scores"], want["topk_scores"], rtol=1e-6)
    assert got["topk_boxes"][:, 0].tobytes() == got["pred_boxes"].tobytes()
    assert torch.equal(pr["topk_boxes"], em["topk_boxes"]) and set(pr) == {"topk_boxes", "topk_scores", "topk_n"}
    # the pooled output is what is scored: the pass-0 dict alone gives pass 0's evaluation
    base = {k: v for k, v in ms.items() if not k.startswith("tta_")}
    e0 = _np(evaluator.get_default_eval(r, s, cfg).eval()(base, inp))
    w0 = MS.evaluate(o5[:, :A0], annot, sz, anc[:A0], K=3)
    assert np.array_equal(e0["hit_rank"], w0["hit_rank"]) and e0["Acc"] == w0["Acc"]
    # the vote, K = 3 and K = 1
    for K in (3, 1):
        cfgv = config.get_cfg(resnet_arch="resnet18", eval_scales=SCALES, eval_topk=K, eval_box_vote=0.6)
        evv = evaluator.get_default_eval(r, s, cfgv).eval()
        assert evv.met_keys == ["Acc", "MaxPos"] + (["Acc@3"] if K > 1 else [])
        emv = evv(ms, inp)
        prv = evv.predict(ms, inp)
        torch.cuda.synchronize()
        g, w = _np(emv), MS.evaluate(o5, annot, sz, anc, K=K, vote_thr=0.6)
        print(f"K={K} vote_n", g["vote_n"].tolist(), "want", w["vote_n"].tolist(), "hit", g["hit_rank"].tolist(), w["vote_hit_rank"].tolist())
        assert np.array_equal(evv.topk_idx.cpu().numpy(), w["topk_idx"]) and np.array_equal(g["vote_n"], w["vote_n"])
        # from the definition alone: the set-up really votes, and its pixel boxes (img_size 360 x 480) have the magnitude, below 1024 px, at
        # which tests/test_gpu_vote.py measured the absolute bound
        assert w["vote_n"].max() > 1 and float(np.abs(w["vote_boxes"]).max()) < 1024.0
        err = float(np.abs(g["topk_boxes"].astype(np.float64) - w["vote_boxes"]).max())
        print(f"K={K} max|voted - ref| = {err:.3e} px (bound {BOUND_PX:.3e}); largest |coordinate| {float(np.abs(w['vote_boxes']).max()):.1f} px")
        assert err <= BOUND_PX
        alone = w["vote_n"] == 1
        assert np.array_equal(g["topk_boxes"][alone], g["topk_boxes_raw"][alone]), "a row without another member keeps its box, bit for bit"
        assert g["pred_boxes"].tobytes() == g["topk_boxes"][:, 0].tobytes()
        assert g["pred_boxes_raw"].tobytes() == got["pred_boxes"].tobytes() and g["topk_boxes_raw"].tobytes() == got["topk_boxes"][:, :K].tobytes()
        assert not (np.abs(w["vote_iou"] - np.float32(0.5)) <= 1e-6).any()
        assert np.array_equal(g["hit_rank"], w["vote_hit_rank"]) and g["Acc"] == w["vote_acc_at"][0] and g["MaxPos"] == want["MaxPos"]
        assert ("Acc@3" in g) == (K == 3) and (K == 1 or g["Acc@3"] == w["vote_acc_at"][2])
        assert torch.equal(prv["topk_boxes"], emv["topk_boxes"]) and torch.equal(prv["vote_n"], emv["vote_n"])
        # training mode: what the evaluator always did
        evv.train()
        assert set(evv(ms, inp)) == {"Acc", "MaxPos", "idxs", "pred_boxes", "pred_scores"}


def test_h_defaults_lower_the_plan_they_always_did_and_never_call_the_vote(Z, ref, monkeypatch):
    """both switches at their defaults: the eval plans' launch lists are the ones recorded from the tree before the keys existed
    (tests/golden/tta_ms_default_plan.json: ResNet-18, B = 2, 128 x 128, plain and shared (2 images, 4 queries), ZSG_AUTOTUNE=0), name for name"""
    with open(os.path.join(HERE, "golden", "tta_ms_default_plan.json")) as f:
        want = json.load(f)
    evaluator = Z["evaluator"]
    called = []
    monkeypatch.setattr(evaluator.lib, "zsg_eval_vote", lambda *a: called.append(a) or -1)
    cfg, net = build(Z)
    net.eval()
    assert net._eval_scales == ()
    inp = ref["inp"]
    out = run(net, inp)
    bt = Z["synth"].synthetic_shared_batch(2, 4, 128, 128, seed=5)
    g = torch.Generator().manual_seed(1)
    run(net, dev(bt, torch.randn(2, 4, 128, generator=g), torch.randn(2, 4, 128, generator=g)))
    assert list(net._plans) == [(2, 128, 128, 20, False), (2, 4, 128, 128, 20, "shared", False)] and not net._ms_resize
    assert [c[2] for c in net._plans[(2, 128, 128, 20, False)].fwd.calls] == want["plain"]
    assert [c[2] for c in net._plans[(2, 4, 128, 128, 20, "shared", False)].fwd.calls] == want["shared"]
    r, s = Z["config"].ratios_scales(cfg)
    for flags in (dict(), dict(eval_topk=3)):
        ev = evaluator.get_default_eval(r, s, Z["config"].get_cfg(resnet_arch="resnet18", **flags)).eval()
        em = ev(out, inp)
        ev.predict(out, inp)
        assert "pred_boxes_raw" not in em and "vote_n" not in em and not ev._tta_anchs
    torch.cuda.synchronize()
    assert not called


def test_learner_validates_with_both_switches(Z, tmp_path):
    from zsgnet_pytorch_amd.main_dist import learner_init
    cfg = Z["config"].get_cfg(resnet_arch="resnet18", bs=2, bsv=2, resize_img=[96, 96], steps_per_epoch=2, tmp_path=str(tmp_path), synthetic=True,
                              eval_scales=SCALES, eval_box_vote=0.6, eval_topk=3)
    cfg.freeze()
    learn = learner_init("ttams", cfg)
    assert learn.mdl._eval_scales == (0.75, 1.25) and learn.eval_fn.box_vote == 0.6
    dl = []
    for seed in (11, 12):
        bt = O.synthetic_batch(2, 96, 96, seed=seed)
        bt["img"] = to_u8(bt["img"])
        bt["idxs"] = bt["idxs"] + 2.0 * (seed - 11)
        dl.append(bt)
    torch.manual_seed(0)
    res, preds = learn._validate(dl, with_predictions=True)
    assert set(res) == set(learn.loss_keys + ["Acc", "MaxPos", "Acc@3"]) and all(np.isfinite(v) for v in res.values())
    assert 0.0 <= res["Acc"] <= res["Acc@3"] <= 1.0
    assert sorted(k[1:3] for k in learn.mdl._plans if not k[-1]) == [(72, 72), (96, 96), (120, 120)]
    assert [p["id"] for p in preds] == [0.0, 1.0, 2.0, 3.0]
    for p in preds:
        assert set(p) == {"id", "pred_boxes", "pred_scores", "topk_boxes", "topk_scores"}
        assert len(p["pred_boxes"]) == 4 and 1 <= len(p["topk_boxes"]) <= 3 and len(p["topk_boxes"]) == len(p["topk_scores"])
        assert p["topk_boxes"][0] == p["pred_boxes"] and np.isfinite(p["topk_boxes"]).all()
