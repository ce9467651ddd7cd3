"""eval_dtype = "bf16" on the network: ZSGNet.eval_precision / cfg eval_dtype, the bf16 eval plan (plain and shared-image), its weight
refresh, mode switches and EMA validation.  ResNet-18, 128 px, B = 2, O.seeded_state_dict("resnet18", 1), O.synthetic_batch(2, 128, 128,
seed=3), fixed h0 / c0 as in smoke().

The accuracy reference is the fp32 eval plan of the SAME weights (itself pinned to the oracle by test_gpu_net.py).  Metric:
max|out5_bf16 - out5_fp32| / max|out5_fp32|, separately for the box channels (0..3) and the att channel (4).  The bound is 4 x the
value measured on an MI355X, rounded up to one digit (profiles/bf16_eval_parity_measured.txt: box 1.154e-2, att 1.390e-2 on this
set-up; the shared-image plan 1.307e-2 / 1.518e-2, the EMA twin 1.9e-3 / 2.3e-5) and may not exceed 0.1 — bf16 rounding flips cascade
through 20 layers; a CPU emulation of this network (operands rounded to bf16, fp32 or fp64 accumulation) gave 1.0-1.8e-2 against fp32
and about 1e-2 between the two accumulation orders themselves.

The module runs with ZSG_DETERMINISTIC=1 (as test_gpu_ema_net.py does): without it the fp32 tuner may pick split-K tiles that add with
fp32 atomics, and two fp32 forwards of one net differ in their last bits — nothing a bit-equality check of this file is about."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import zsg_oracle as O  # noqa: E402

BOUND_BOX = 5e-2          # 4 x 1.154e-2 = 4.6e-2, rounded up to one digit
BOUND_ATT = 6e-2          # 4 x 1.390e-2 = 5.6e-2, rounded up to one digit
assert BOUND_BOX <= 0.1 and BOUND_ATT <= 0.1


@pytest.fixture(scope="module")
def Z():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib, config, ema, evaluator, loss, mdl, optim, synth
    return dict(L=_lib, config=config, ema=ema, evaluator=evaluator, loss=loss, mdl=mdl, optim=optim, synth=synth)


@pytest.fixture(scope="module", autouse=True)
def deterministic(Z):
    L = Z["L"]
    old = os.environ.get("ZSG_DETERMINISTIC")
    os.environ["ZSG_DETERMINISTIC"] = "1"
    L.lib.zsg_set_deterministic(1)
    yield
    if old is None:
        os.environ.pop("ZSG_DETERMINISTIC", None)
    else:
        os.environ["ZSG_DETERMINISTIC"] = old
    L.lib.zsg_set_deterministic(1 if old == "1" else 0)


def build(Z, sd=None, **flags):
    cfg = Z["config"].get_cfg(resnet_arch="resnet18", **flags)
    net = Z["mdl"].get_default_net(9, cfg)
    net.load_state_dict(sd if sd is not None else O.seeded_state_dict("resnet18", 1))
    return cfg, net.to("cuda")


def batch(B=2):
    bt = O.synthetic_batch(B, 128, 128, seed=3)
    g = torch.Generator().manual_seed(0)
    inp = {k: v.cuda() for k, v in bt.items()}
    inp["h0"], inp["c0"] = torch.randn(2, B, 128, generator=g), torch.randn(2, B, 128, generator=g)
    return inp


def fwd(net, inp):
    with torch.no_grad():
        out = net(inp)
    torch.cuda.synchronize()
    return out


def out5(net, inp):
    return fwd(net, inp)["att_bbx_out"].detach().clone()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def rel(a, b):
    """(box, att): max|a - b| / max|b| over the box channels and over the att channel of a [B, A, 5] output"""
    a, b = a.double().cpu(), b.double().cpu()
    return (float((a[..., :4] - b[..., :4]).abs().max() / b[..., :4].abs().max()),
            float((a[..., 4] - b[..., 4]).abs().max() / b[..., 4].abs().max()))


def names(prog):
    return [fn.__name__ for fn, _, _ in prog.calls]


def eval_plan(net, dtype):
    ks = [k for k in net._plans if not k[-1] and (("bf16" in k) == (dtype == "bf16"))]
    assert len(ks) == 1, ks
    return net._plans[ks[0]]


@pytest.fixture(scope="module")
def ref(Z, deterministic):
    """the fp32 eval output, the bf16 eval output and their evaluator picks on the module's set-up (computed once, never modified)"""
    inp = batch()
    cfg, net = build(Z)
    net.eval()
    o32 = out5(net, inp)
    cfgb, netb = build(Z, eval_dtype="bf16")
    netb.eval()
    ob = out5(netb, inp)
    r, s = Z["config"].ratios_scales(cfg)
    ev = Z["evaluator"].get_default_eval(r, s, cfg)
    picks = []
    for n_ in (net, netb):
        ev(fwd(n_, inp), inp)
        torch.cuda.synchronize()
        picks.append(ev.pred_idx.cpu().clone())
    return dict(inp=inp, net=net, netb=netb, o32=o32, ob=ob, picks=picks)


def test_default_is_untouched(Z, ref):
    _, net2 = build(Z, eval_dtype="fp32")
    net2.eval()
    assert torch.equal(bits(out5(net2, ref["inp"])), bits(ref["o32"]))
    for n_ in (ref["net"], net2):
        assert list(n_._plans) == [(2, 128, 128, list(n_._plans)[0][3], False)]          # the key the default always had
        nm = names(eval_plan(n_, "fp32").fwd)
        assert "zsg_conv_igemm_bf16" not in nm and "zsg_pack_w_bf16_batched" not in nm
        assert not eval_plan(n_, "fp32").pack_jobs


def test_bf16_plan_wiring(Z, ref):
    L, netb = Z["L"], ref["netb"]
    plan = eval_plan(netb, "bf16")
    convs = [(fn.__name__, what) for fn, _, what in plan.fwd.calls if fn.__name__ in ("zsg_conv_igemm", "zsg_conv_wino", "zsg_conv_igemm_bf16")]
    fp32 = [w for n, w in convs if n != "zsg_conv_igemm_bf16"]
    # what stays fp32: the stem (merge_x), the LSTM input projections, the language map's two tiny GEMMs (V: language columns of conv0,
    # G: grid columns)
    assert all(w.endswith("encoder.conv1+bn") or w.startswith("lstm_in") or w.endswith("0.V") or w.endswith("0.G") for w in fp32), fp32
    assert sum(w.endswith("encoder.conv1+bn") for w in fp32) == 1
    n_bf = sum(n == "zsg_conv_igemm_bf16" for n, _ in convs)
    # ResNet-18: 19 encoder convolutions behind the stem (16 in the blocks + 3 downsample), the FPN's, the head's 6
    assert n_bf >= 19 + 6 and n_bf == len(plan.pack_jobs), (n_bf, len(plan.pack_jobs))
    assert "zsg_wino_weights" not in names(plan.fwd) and "zsg_conv_wino" not in names(plan.fwd)
    # exactly one pack launch per forward (it is issued next to the BatchNorm fold, in front of the program), two added launches at most
    L.lib.zsg_prof_enable(1)
    try:
        ents = (L.ProfEntry * 256)()
        L.lib.zsg_prof_collect(ents, 256)
        fwd(netb, ref["inp"])
        n = L.lib.zsg_prof_collect(ents, 256)
    finally:
        L.lib.zsg_prof_enable(0)
    got = {ents[i].name.decode(): ents[i].launches for i in range(n)}
    assert got.get("pack_w_bf16_kernel") == 1, got
    assert sum(v for k, v in got.items() if k.startswith("igemm_bf16_kernel")) == n_bf, got
    assert len(plan.fwd.calls) == len(eval_plan(ref["net"], "fp32").fwd.calls) - names(eval_plan(ref["net"], "fp32").fwd).count("zsg_wino_weights")
    # really taken, and deterministic
    assert not torch.equal(ref["ob"], ref["o32"])
    assert torch.equal(bits(out5(netb, ref["inp"])), bits(ref["ob"]))
    assert plan._out_slots(), "the fresh-output slot patching must keep working"


def test_accuracy_against_the_fp32_plan(Z, ref):
    rb, ra = rel(ref["ob"], ref["o32"])
    print(f"bf16 eval parity (resnet18, 128 px, B=2): box {rb:.3e} att {ra:.3e} of max|fp32|; pred_idx fp32 {ref['picks'][0].tolist()} "
          f"bf16 {ref['picks'][1].tolist()}")
    assert rb <= BOUND_BOX and ra <= BOUND_ATT
    assert torch.equal(ref["picks"][0], ref["picks"][1])


def test_switching_reuses_plans_and_bad_values_are_refused(Z, ref):
    _, net = build(Z)
    net.eval()
    a = out5(net, ref["inp"])
    assert net.eval_precision("bf16") is net
    b = out5(net, ref["inp"])
    p32, pb = eval_plan(net, "fp32"), eval_plan(net, "bf16")
    net.eval_precision("fp32")
    a2 = out5(net, ref["inp"])
    net.eval_precision("bf16")
    b2 = out5(net, ref["inp"])
    assert eval_plan(net, "fp32") is p32 and eval_plan(net, "bf16") is pb and len(net._plans) == 2
    assert torch.equal(bits(a), bits(a2)) and torch.equal(bits(b), bits(b2))
    assert torch.equal(bits(a), bits(ref["o32"])) and torch.equal(bits(b), bits(ref["ob"]))
    with pytest.raises(ValueError, match="eval_dtype"):
        net.eval_precision("fp16")
    with pytest.raises(TypeError, match="eval_precision"):
        net.to(torch.bfloat16)


def test_weights_are_repacked_every_forward(Z, ref):
    _, net = build(Z, eval_dtype="bf16")
    net.eval()
    before = out5(net, ref["inp"])
    with torch.no_grad():
        w = dict(net.named_parameters())["att_reg_box.2.0.weight"]
        w[3:40].mul_(1.5)
        w[100, 7] += 0.25
    after = out5(net, ref["inp"])
    assert not torch.equal(after, before)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    _, fresh = build(Z, sd=sd, eval_dtype="bf16")
    fresh.eval()
    assert torch.equal(bits(out5(fresh, ref["inp"])), bits(after))


def test_mode_switches_leave_the_training_plan_alone(Z, ref):
    inp = ref["inp"]

    def step(net, lf, opt):
        opt.zero_grad()
        ls = lf(net(inp), inp)["loss"]
        ls.backward()
        opt.step()
        torch.cuda.synchronize()
        return float(ls)
    progs = []
    for dtype in ("bf16", None):
        cfg, net = build(Z, **({"eval_dtype": dtype} if dtype else {}))
        r, s = Z["config"].ratios_scales(cfg)
        lf, opt = Z["loss"].get_default_loss(r, s, cfg), Z["optim"].FusedAdam(net, lr=1e-4, betas=(0.9, 0.99))
        net.train()
        l0 = step(net, lf, opt)
        if dtype:
            net.eval()
            o = out5(net, inp)
            assert torch.isfinite(o).all() and "zsg_conv_igemm_bf16" in names(eval_plan(net, "bf16").fwd)
            net.train()
        l1 = step(net, lf, opt)
        assert l0 == l0 and l1 == l1
        tp = [p for k, p in net._plans.items() if k[-1]]
        assert len(tp) == 1 and not tp[0].bf16 and not tp[0].pack_jobs
        progs.append((names(tp[0].fwd), names(tp[0].bwd), names(tp[0].prep)))
    assert progs[0] == progs[1], "the training plan's launches must be those of a net that never heard of bf16"
    assert "zsg_conv_igemm_bf16" not in progs[0][0] + progs[0][1] + progs[0][2]


def test_shared_image_plan(Z):
    synth = Z["synth"]
    bt = synth.synthetic_shared_batch(2, 4, 128, 128, seed=21)
    g = torch.Generator().manual_seed(22)
    h0, c0 = torch.randn(2, 4, 128, generator=g), torch.randn(2, 4, 128, generator=g)
    inp = {k: v.cuda() for k, v in bt.items()}
    inp["h0"], inp["c0"] = h0, c0
    _, net = build(Z)
    net.eval()
    a = out5(net, inp)
    b = out5(net.eval_precision("bf16"), inp)
    kb = [k for k in net._plans if "bf16" in k]
    assert len(kb) == 1 and kb[0][5] == "shared" and len([k for k in net._plans if k[5:6] == ("shared",)]) == 2
    nm = [(fn.__name__, what) for fn, _, what in net._plans[kb[0]].fwd.calls]
    assert ("zsg_conv_igemm_bf16", "att_reg_box.0.0.feat+bf16") in nm and "zsg_head_shared_conv0" in [n for n, _ in nm]
    rb, ra = rel(b, a)
    print(f"bf16 shared-image eval parity (4 queries over 2 images): box {rb:.3e} att {ra:.3e} of max|fp32|")
    assert not torch.equal(a, b) and rb <= BOUND_BOX and ra <= BOUND_ATT
    assert torch.equal(bits(out5(net, inp)), bits(b))


def test_ema_validation_goes_through_the_bf16_plan(Z, ref, tmp_path):
    """Learner.validate with a weight average applies it INTO the same net (ModelEma.applied), so with eval_dtype = bf16 the averaged
    weights are what the pack launch reads: the learner's validation runs, and under applied() the bf16 output is the fp32 output of
    the same averaged weights within the bound (and not the output of the raw weights)."""
    from zsgnet_pytorch_amd.main_dist import learner_init
    cfg = Z["config"].get_cfg(resnet_arch="resnet18", bs=2, bsv=2, resize_img=[128, 128], steps_per_epoch=2, tmp_path=str(tmp_path), synthetic=True,
                              ema_decay=0.5, eval_dtype="bf16")
    cfg.freeze()
    learn = learner_init("bf16ema", cfg)
    learn.fit(epochs=1, lr=1e-3)
    net, avg = learn.mdl, learn.ema
    assert avg is not None and net._eval_dtype == "bf16"
    torch.manual_seed(0)
    vb = learn.validate()
    assert any("bf16" in k for k in net._plans), list(net._plans)
    net.eval_precision("fp32")
    torch.manual_seed(0)
    v32 = learn.validate()
    print("EMA validate bf16:", vb, "fp32:", v32)
    assert all(v == v for v in vb.values())
    inp = ref["inp"]
    net.eval()
    with avg.applied():
        a = out5(net, inp)
        b = out5(net.eval_precision("bf16"), inp)
    raw = out5(net, inp)
    rb, ra = rel(b, a)
    print(f"bf16 EMA eval parity: box {rb:.3e} att {ra:.3e} of max|fp32|")
    assert rb <= BOUND_BOX and ra <= BOUND_ATT
    assert not torch.equal(raw, b)
