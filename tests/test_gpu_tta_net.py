"""Flip test-time augmentation on the network: cfg eval_tta / ZSGNet.eval_tta.  ResNet-18, 128 px, B = 2, O.seeded_state_dict("resnet18", 1),
O.synthetic_batch(2, 128, 128, seed=3), fixed h0 / c0 as in tests/test_gpu_net_bf16.py, and a `qvec_flip` that differs from `qvec`.

tests/tta_ref.py is the definition: the TTA forward of B rows is merge_ref of ONE eval forward of the 2B rows tta_batch builds.  Against the
CPU oracle the tolerance is the project's for fp32 network outputs (rtol 2e-3, atol 5e-3, tests/test_gpu_net.py): a mean of two outputs each
within it is within it.  Against the net's own plain forward of the hand-built 2B rows the check is bit-equality: the same plan (hence the
same tiles), the same staged inputs, and the merge is reproducible in numpy.  The module runs with ZSG_AUTOTUNE=0 and ZSG_DETERMINISTIC=1
(no tile choice by timing, no fp32 atomics: two forwards of one plan give the same bits)."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tta_ref as R  # noqa: E402
from oracle import zsg_oracle as O  # noqa: E402

N_ANCH = 9


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


def build(Z, **flags):
    cfg = Z["config"].get_cfg(resnet_arch="resnet18", **flags)
    net = Z["mdl"].get_default_net(N_ANCH, cfg)
    net.load_state_dict(O.seeded_state_dict("resnet18", 1))
    return cfg, net.to("cuda")


def host_batch(B=2):
    bt = O.synthetic_batch(B, 128, 128, seed=3)
    g = torch.Generator().manual_seed(0)
    h0, c0 = torch.randn(2, B, 128, generator=g), torch.randn(2, B, 128, generator=g)
    bt["qvec_flip"] = torch.randn(bt["qvec"].shape, generator=g) * 0.35
    return bt, h0, c0


def dev(bt, h0, c0):
    inp = {k: v.cuda() for k, v in bt.items()}
    inp["h0"], inp["c0"] = h0, c0
    return inp


def out5(net, inp):
    with torch.no_grad():
        out = net(inp)
    torch.cuda.synchronize()
    return out["att_bbx_out"].detach().clone(), out


def bits(t):
    t = t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
    return t.detach().cpu().contiguous().view(torch.int32)


def merged(x2, sizes):
    return R.merge_ref(x2.cpu().numpy(), sizes, N_ANCH)


@pytest.fixture(scope="module")
def ref(Z, fixed_tiles):
    """the module's set-up, its TTA output and the hand-built 2B rows (computed once, never modified)"""
    bt, h0, c0 = host_batch()
    cfg, net = build(Z, eval_tta="flip")
    net.eval()
    inp = dev(bt, h0, c0)
    o, out = out5(net, inp)
    bt2, h2, c2 = R.tta_batch(bt, h0, c0)
    sizes = [tuple(s) for s in out["feat_sizes"].tolist()]
    return dict(cfg=cfg, net=net, bt=bt, h0=h0, c0=c0, inp=inp, o=o, out=out, bt2=bt2, h2=h2, c2=c2, inp2=dev(bt2, h2, c2), sizes=sizes)


def test_output_contract(Z, ref):
    out, o = ref["out"], ref["o"]
    A = sum(h * w * N_ANCH for h, w in ref["sizes"])
    assert tuple(o.shape) == (2, A, 5) and tuple(out["att_out"].shape) == (2, A, 1) and tuple(out["bbx_out"].shape) == (2, A, 4)
    assert ref["sizes"] == O.feat_sizes_for(128, 128) and int(out["num_f_out"]) == len(ref["sizes"])
    assert bool(torch.isfinite(o).all())
    assert [k for k in ref["net"]._plans if not k[-1]] == [(4, 128, 128, 20, False)], "the plain eval plan of 2B rows"
    plan = ref["net"]._plans[(4, 128, 128, 20, False)]
    assert np.array_equal(plan._tta_levels(), R.level_table(ref["sizes"], N_ANCH)) and plan._tta_levels() is plan._tta_levels()
    o2, _ = out5(ref["net"], ref["inp"])
    assert o2.data_ptr() != o.data_ptr() and torch.equal(bits(o2), bits(o)), "a fresh tensor, the same bits"


def test_parity_with_the_cpu_oracle(Z, ref):
    sd = O.seeded_state_dict("resnet18", 1)
    with torch.no_grad():
        want2 = O.zsgnet_forward(sd, ref["bt2"], ref["h2"], ref["c2"], arch="resnet18", training=False)
    assert [tuple(s) for s in want2["feat_sizes"].tolist()] == ref["sizes"]
    want = merged(torch.cat([want2["bbx_out"], want2["att_out"]], dim=2).float(), ref["sizes"])
    got = ref["o"].cpu().numpy()
    print(f"TTA vs oracle: max|diff| box {np.abs(got[..., :4] - want[..., :4]).max():.3e}, att {np.abs(got[..., 4] - want[..., 4]).max():.3e}")
    np.testing.assert_allclose(got[..., 4], want[..., 4], rtol=2e-3, atol=5e-3)
    np.testing.assert_allclose(got[..., :4], want[..., :4], rtol=2e-3, atol=5e-3)
    # the mirrored pass matters on this set-up: the rows as given alone do not pass this check
    plain = torch.cat([want2["bbx_out"], want2["att_out"]], dim=2)[:2].float().numpy()
    assert not np.allclose(plain, want, rtol=2e-3, atol=5e-3)


def test_bit_equal_to_merge_ref_of_the_plain_forward_of_the_hand_built_rows(Z, ref):
    net = ref["net"]
    net.eval_tta("none")
    try:
        x2, _ = out5(net, ref["inp2"])
    finally:
        net.eval_tta("flip")
    assert tuple(x2.shape)[0] == 4 and list(net._plans) == [(4, 128, 128, 20, False)], "the same plan"
    assert torch.equal(bits(merged(x2, ref["sizes"])), bits(ref["o"]))
    # uint8 HWC images go through the other staging entry
    u8 = (ref["bt"]["img"].permute(0, 2, 3, 1) * 255).round().to(torch.uint8).contiguous()
    bt8 = dict(ref["bt"], img=u8)
    o8, _ = out5(net, dev(bt8, ref["h0"], ref["c0"]))
    b82, h2, c2 = R.tta_batch(bt8, ref["h0"], ref["c0"])
    net.eval_tta("none")
    try:
        x82, _ = out5(net, dev(b82, h2, c2))
    finally:
        net.eval_tta("flip")
    assert torch.equal(bits(merged(x82, ref["sizes"])), bits(o8)) and not torch.equal(bits(o8), bits(ref["o"]))


def test_without_qvec_flip_the_mirrored_rows_read_qvec(Z, ref):
    net = ref["net"]
    bt = {k: v for k, v in ref["bt"].items() if k != "qvec_flip"}
    o, _ = out5(net, dev(bt, ref["h0"], ref["c0"]))
    bt2, h2, c2 = R.tta_batch(bt, ref["h0"], ref["c0"])
    assert torch.equal(bt2["qvec"][2:], bt["qvec"])
    net.eval_tta("none")
    try:
        x2, _ = out5(net, dev(bt2, h2, c2))
    finally:
        net.eval_tta("flip")
    assert torch.equal(bits(merged(x2, ref["sizes"])), bits(o)) and not torch.equal(bits(o), bits(ref["o"]))
    with pytest.raises(ValueError, match="qvec_flip"):
        net(dict(ref["inp"], qvec_flip=ref["inp"]["qvec"][:, :5]))


def test_none_and_train_mode_are_untouched_and_switching_reuses_plans(Z, ref):
    plain_bt = {k: v for k, v in ref["bt"].items()}
    inp = dev(plain_bt, ref["h0"], ref["c0"])
    _, never = build(Z)
    never.eval()
    want, _ = out5(never, inp)
    _, net = build(Z, eval_tta="flip")
    net.eval()
    a, _ = out5(net, inp)
    assert net.eval_tta("none") is net
    b, _ = out5(net, inp)
    assert torch.equal(bits(b), bits(want)) and not torch.equal(bits(a), bits(want)), '"none": the bits of a net that never saw the switch'
    assert [k for k in net._plans if k[0] == 2] == list(never._plans) == [(2, 128, 128, 20, False)]
    plans = dict(net._plans)
    net.eval_tta("flip")
    a2, _ = out5(net, inp)
    net.eval_tta("none")
    out5(net, inp)
    net.eval_tta("flip")
    assert torch.equal(bits(a2), bits(a)) and list(net._plans) == list(plans) and all(net._plans[k] is p for k, p in plans.items())
    # train mode ignores the switch: the plain training output bits, B rows, the training plan
    never.train(), net.train()
    with torch.no_grad():
        tw, tg = never(inp)["att_bbx_out"].clone(), net(inp)["att_bbx_out"].clone()
    torch.cuda.synchronize()
    assert tuple(tg.shape)[0] == 2 and torch.equal(bits(tg), bits(tw))
    assert [k[:4] for k in net._plans if k[-1]] == [(2, 128, 128, 20)] and set(net._plans) - set(plans) == {k for k in net._plans if k[-1]}


def test_shared_image_plan(Z, ref):
    synth = Z["synth"]
    net = ref["net"]
    bt = synth.synthetic_shared_batch(2, 4, 128, 128, seed=5)
    g = torch.Generator().manual_seed(1)
    h0, c0 = torch.randn(2, 4, 128, generator=g), torch.randn(2, 4, 128, generator=g)
    bt["qvec_flip"] = torch.randn(bt["qvec"].shape, generator=g) * 0.35
    o, out = out5(net, dev(bt, h0, c0))
    assert tuple(o.shape)[0] == 4 and (4, 8, 128, 128, 20, "shared", False) in net._plans
    bt2, h2, c2 = R.tta_batch(bt, h0, c0)
    assert bt2["img"].shape[0] == 4 and bt2["qvec"].shape[0] == 8 and bt2["img_idx"].tolist() == bt["img_idx"].tolist() + (bt["img_idx"] + 2).tolist()
    net.eval_tta("none")
    try:
        x2, _ = out5(net, dev(bt2, h2, c2))
    finally:
        net.eval_tta("flip")
    assert len([k for k in net._plans if "shared" in k]) == 1, "the same shared plan"
    assert torch.equal(bits(merged(x2, ref["sizes"])), bits(o))


def test_evaluator_accepts_the_merged_output(Z, ref):
    config, evaluator = Z["config"], Z["evaluator"]
    cfg = config.get_cfg(resnet_arch="resnet18", eval_tta="flip", eval_topk=3)
    r, s = config.ratios_scales(cfg)
    ev = evaluator.get_default_eval(r, s, cfg).eval()
    em = ev(ref["out"], ref["inp"])
    pr = ev.predict(ref["out"], ref["inp"])
    torch.cuda.synchronize()
    o = ref["o"].cpu().numpy()
    anc = O.create_anchors(ref["sizes"], r, s).astype(np.float32)
    # the arg-max anchors of the MERGED rows: the evaluator ranks fp32 sigmoid scores, where neighbouring logits of this seeded net tie to
    # within the rounding of expf, so its pick is checked as "a maximum within 4 ulp of a score in [0.5, 1]" rather than against numpy's
    # own tie-break; the box is then the oracle's decode of the merged row at that anchor (tolerance of tests/test_gpu_loss.py)
    ids = ev.pred_idx.cpu().tolist()
    score = 1.0 / (1.0 + np.exp(-o[..., 4].astype(np.float64)))
    sz = ref["bt"]["img_size"].numpy().astype(np.float32)
    want = []
    print("evaluator picks", ids, "scores", [float(score[b, a]) for b, a in enumerate(ids)], "numpy arg-max", score.argmax(1).tolist(), score.max(1).tolist())
    for b, a in enumerate(ids):
        assert 0 <= a < o.shape[1] and score[b, a] >= score[b].max() - 4 * 2.0 ** -24, (b, a)
        y1, x1, y2, x2 = (O.reg_params_to_bbox(anc[a:a + 1], o[b:b + 1, a:a + 1, :4])[0, 0] + np.float32(1)) / np.float32(2)
        want.append([sz[b, 1] * x1, sz[b, 0] * y1, sz[b, 1] * x2, sz[b, 0] * y2])
    np.testing.assert_allclose(em["pred_boxes"].cpu().numpy(), np.array(want, np.float32), rtol=1e-5, atol=1e-3)
    assert tuple(em["topk_boxes"].shape) == (2, 3, 4) and tuple(pr["topk_boxes"].shape) == (2, 3, 4)
    assert em["topk_boxes"][:, 0].cpu().numpy().tobytes() == em["pred_boxes"].cpu().numpy().tobytes()
    assert torch.equal(pr["topk_boxes"], em["topk_boxes"]) and bool((pr["topk_n"] >= 1).all())


def test_learner_validates_and_writes_predictions_with_tta_and_ema(Z, tmp_path):
    from zsgnet_pytorch_amd.main_dist import learner_init
    cfg = Z["config"].get_cfg(resnet_arch="resnet18", bs=2, bsv=2, resize_img=[96, 96], steps_per_epoch=2, tmp_path=str(tmp_path), synthetic=True,
                              eval_tta="flip", ema_decay=0.9)
    cfg.freeze()
    learn = learner_init("tta", cfg)
    assert learn.mdl._eval_tta == "flip"
    learn.fit(epochs=1, lr=1e-3)
    assert learn.num_it == 2 and learn.ema is not None and learn.ema.n_averaged == 2
    keys = list(learn.mdl._plans)
    assert [k[:4] for k in keys if k[-1]] == [(2, 96, 96, 20)] and [k for k in keys if not k[-1]] == [(4, 96, 96, 20, False)], keys
    torch.manual_seed(0)
    va = learn.validate()
    assert all(np.isfinite(v) for v in va.values()) and 0.0 <= va["Acc"] <= 1.0
    learn.mdl.eval_tta("none")
    torch.manual_seed(0)
    plain = learn.validate()
    learn.mdl.eval_tta("flip")
    assert plain["loss"] != va["loss"], "the validation loss is the merged output's"
    res = learn.testing(learn.data.test_dl)
    pf = learn.predictions_dir / "synthetic_test_preds.pkl"
    preds = pickle.load(open(pf, "rb"))
    dl = learn.data.test_dl["synthetic_test"]
    assert len(preds) == len(dl) * 2 and set(preds[0]) == {"id", "pred_boxes", "pred_scores"} and 0.0 <= res["synthetic_test"]["Acc"] <= 1.0
