"""enc_dtype = "bf16_fwd" on the network: ZSGNet.encoder_precision / cfg enc_dtype, the training plan whose encoder forward convolutions
behind the stem run on zsg_conv_igemm_bf16_bn (fused BatchNorm partial rows) or zsg_conv_igemm_bf16 (frozen BatchNorm), with the fp32
plan's backward.  The set-up of tests/test_gpu_net_train_bf16_head.py: ResNet-18, 128 px, B = 2, O.seeded_state_dict("resnet18", 1),
O.synthetic_batch(2, 128, 128, seed=3), fixed h0 / c0, under ZSG_DETERMINISTIC=1.

Exact part: the stem (its output, behind the max-pool, feeds the first covered convolution) and the LSTM are untouched: bit-equal to the
fp32 net's.  With the switch back at "fp32" a step gives the fp32 plan's bits; eval ignores the switch.

Layer-local part (the rigorous one), for every "enc_fwd" entry of plan._b16_log:
  * the convolution, recomputed on the host from the GPU's OWN source bits and the current parameters, both rounded to bf16 (torch's
    round-to-nearest-even), fp64 sums, under the project's bound |out - ref| <= (K + 4) * 2^-23 * S, K = taps * C, S the same sum of
    absolute values (tests/test_gpu_conv_bf16.py);
  * the BatchNorm statistics, against the fp64 statistics of the GPU's own raw convolution output v [n rows]: a partial row sums at
    most BM = 128 values in fp32, off by at most (BM - 1) * 2^-24 < 2^-17 of sum |v| (tests/test_gpu_conv_bf16_bn.py); the rows are
    then reduced in fp64 and the mean is rounded to fp32 once:
        dmean <= 2^-17 * E|v| + 2^-24 * |m|,        dvar <= 2^-17 * (E[v^2] + 2 |m| E|v|)        (var = E[v^2] - m^2, biased)
    and invstd = (var + eps)^-1/2 lies within 0.5 * (var + eps - dvar)^-3/2 * dvar (the derivative's largest value over the interval)
    + 2^-22 * invstd (its own fp32 arithmetic) of the fp64 value;
  * where the net has run ONE forward from the seeded state: running_mean = 0.9 * old + 0.1 * m and running_var = 0.9 * old +
    0.1 * var * n / (n - 1) (momentum 0.1) within 0.1 x the bounds above + 2^-22 of the terms' magnitudes.

Rounded part against the fp32 plan of the same tree: each bound is 4 x the value measured on an MI355X, rounded up to one digit
(profiles/enc_bf16_parity_measured.txt, which also holds the CPU emulation the measured values are compared with)."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import zsg_oracle as O  # noqa: E402

# measured on an MI355X (profiles/enc_bf16_parity_measured.txt); bound = 4 x measured, rounded up to one digit.  The CPU emulation
# (tools/enc_bf16_emul.py, fp64: the oracle with the encoder's forward operands rounded to bf16, its backward unrounded) gives box
# 2.467e-2, att 1.750e-2, loss 8.344e-3, flat L2 1.727e-1, 1 - cosine 1.491e-2: the measured values sit where it predicts
MEASURED = dict(box=2.385e-2, att=1.617e-2, loss=9.585e-3, l2=1.778e-1, one_minus_cos=1.572e-2)
BOUND_BOX = 1e-1          # 4 x 2.385e-2 = 9.54e-2, rounded up to one digit
BOUND_ATT = 7e-2          # 4 x 1.617e-2 = 6.47e-2
BOUND_LOSS = 4e-2         # 4 x 9.585e-3 = 3.83e-2
BOUND_L2 = 0.8            # 4 x 1.778e-1 = 7.11e-1
BOUND_COS = 1 - 7e-2      # 1 - 4 x 1.572e-2 = 1 - 6.29e-2

ENC = "backbone.encoder."
STEM = ENC + "conv1"
ENC_FNS = ("zsg_conv_igemm_bf16_bn", "zsg_conv_igemm_bf16")
FP32_CONVS = ("zsg_conv_igemm", "zsg_conv_wino", "zsg_conv_igemm_bnstat", "zsg_conv_wino_bnstat")
SUFFIXES = ("+bf16bn", "+bf16", "+bnstat")


@pytest.fixture(scope="module")
def Z():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib, config, loss, mdl, optim, synth
    return dict(L=_lib, config=config, loss=loss, mdl=mdl, optim=optim, synth=synth)


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


def build(Z, arch="resnet18", drop_key=False, **flags):
    cfg = Z["config"].get_cfg(resnet_arch=arch, **flags)
    if drop_key:
        cfg.pop("enc_dtype")
    net = Z["mdl"].get_default_net(9, cfg)
    net.load_state_dict(O.seeded_state_dict(arch, 1))
    return cfg, net.to("cuda")


def batch(B=2):
    bt = O.synthetic_batch(B, 128, 128, seed=3)
    g = torch.Generator().manual_seed(0)
    inp = {k: v.cuda() for k, v in bt.items()}
    inp["h0"], inp["c0"] = torch.randn(2, B, 128, generator=g), torch.randn(2, B, 128, generator=g)
    return inp


def shared_batch(Z):
    bt = Z["synth"].synthetic_shared_batch(2, 4, 128, 128, seed=5)
    bt["img_idx"] = torch.tensor([1, 0, 0, 1])
    inp = {k: v.cuda() for k, v in bt.items()}
    inp["h0"], inp["c0"] = torch.zeros(2, 4, 128), torch.zeros(2, 4, 128)
    return inp


def loss_fn(Z, cfg):
    r, s = Z["config"].ratios_scales(cfg)
    return Z["loss"].get_default_loss(r, s, cfg)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def train_plan(net):
    ks = [k for k in net._plans if k[-1]]
    assert len(ks) == 1, ks
    return net._plans[ks[0]]


def listing(prog):
    return [(lane, fn.__name__, what) for (fn, _, what), lane in zip(prog.calls, prog.lanes)]


def step(Z, cfg, net, inp):
    """zero_grad + forward + loss + backward; returns (att_bbx_out, loss terms, the flat gradient) on the CPU"""
    net.train()
    net.store.grad.zero_()
    out = net(inp)
    ls = loss_fn(Z, cfg)(out, inp)
    ls["loss"].mean().backward()
    torch.cuda.synchronize()
    return out["att_bbx_out"].detach().cpu().clone(), {k: v.detach().cpu().clone() for k, v in ls.items() if torch.is_tensor(v)}, net.store.grad.detach().cpu().clone()


def grad_of(net, flat, name):
    e = net.store.entries[name]
    return flat[e.offset:e.offset + e.size]


def base_what(what):
    for s in SUFFIXES:
        if what.endswith(s):
            return what[:-len(s)]
    return what


def enc_convs(lst):
    """(lane, function, layer) of the encoder's forward convolutions behind the stem, in program order (bnpre launches apart)"""
    return [(lane, n, base_what(w)) for lane, n, w in lst
            if w.startswith(ENC) and not w.startswith(STEM) and n.startswith("zsg_conv") and "+bnpre(" not in w]


# ---- the layer-local reference ----------------------------------------------------------------------------------------------------------
def level_view(act, buf, i, Cc):
    lv = act.levels[i]
    return torch.as_strided(buf, (act.B, lv.H, lv.W, Cc), (lv.bstride, lv.W * act.ld, act.ld, 1), lv.off)


def conv_ref(src, w, k, s, p, Ho, Wo):
    B, H, W, Cc = src.shape
    pad = torch.zeros(B, H + 2 * p, W + 2 * p, Cc, dtype=src.dtype)
    pad[:, p:p + H, p:p + W] = src
    out = torch.zeros(B, Ho, Wo, w.shape[0], dtype=src.dtype)
    for ty in range(k):
        for tx in range(k):
            win = pad[:, ty: ty + (Ho - 1) * s + 1: s, tx: tx + (Wo - 1) * s + 1: s]
            out += torch.matmul(win.reshape(-1, Cc), w[:, ty, tx].t()).view(B, Ho, Wo, -1)
    return out


def local_check(net, e, flat, running0=None):
    """the logged launch `e` from the GPU's own bits; returns (conv, mean, invstd, running) error / bound, each <= 1 passes (None: not
    applicable).  running0: (running_mean, running_var) of the whole net BEFORE the one forward that ran, or None"""
    L = net.convs[e["pname"][:-len(".weight")]]
    assert L.dil == 1 and not L.bias and e["kind"] == "enc_fwd" and e["add"] is None and len(e["out"].levels) == 1
    ent = net.store.entries[e["pname"]]
    w = flat[ent.offset:ent.offset + L.cout * L.k * L.k * L.cpad].view(L.cout, L.k, L.k, L.cpad)
    d = e["d"]
    assert (d.C, d.N, d.relu) == (L.cpad, L.cout, 0)
    lo = e["out"].levels[0]
    x = level_view(e["src"], e["src"].buf.detach().cpu(), 0, d.C).to(torch.bfloat16).double()
    wb = w.to(torch.bfloat16).double()
    r, S = conv_ref(x, wb, L.k, L.stride, L.pad, lo.H, lo.W), conv_ref(x.abs(), wb.abs(), L.k, L.stride, L.pad, lo.H, lo.W)
    got = level_view(e["out"], e["out"].buf.detach().cpu(), 0, L.cout).double()
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    bound = (L.k * L.k * d.C + 4) * 2.0 ** -23 * S
    res = [float(((got - r).abs() / bound.clamp(min=1e-300)).max()), None, None, None]
    assert e["bn"] is not None and e["mean"] is not None and e["invstd"] is not None, "bn() fills the log entry"
    Lb = net.bns[e["bn"]]
    mean_g, inv_g = e["mean"].detach().cpu().double(), e["invstd"].detach().cpu().double()
    rm = net._rm[Lb.index:Lb.index + Lb.c].detach().cpu().double()
    rv = net._rv[Lb.index:Lb.index + Lb.c].detach().cpu().double()
    if e["frozen"]:
        # running statistics: mean is the running mean itself, invstd its (var + eps)^-1/2 in fp32
        assert torch.equal(mean_g, rm)
        res[2] = float(((inv_g - (rv + 1e-5).rsqrt()).abs() / (2.0 ** -22 * (rv + 1e-5).rsqrt())).max())
        return res
    v = got.reshape(-1, L.cout)
    n = v.shape[0]
    m, ea, e2 = v.mean(0), v.abs().mean(0), (v * v).mean(0)
    var = e2 - m * m
    dmean = 2.0 ** -17 * ea + 2.0 ** -24 * m.abs()
    dvar = 2.0 ** -17 * (e2 + 2 * m.abs() * ea)
    assert bool((dvar < var + 1e-5).all())
    inv = (var + 1e-5).rsqrt()
    dinv = 0.5 * (var + 1e-5 - dvar) ** -1.5 * dvar + 2.0 ** -22 * inv
    res[1] = float(((mean_g - m).abs() / dmean.clamp(min=1e-300)).max())
    res[2] = float(((inv_g - inv).abs() / dinv).max())
    if running0 is not None:
        rm0 = running0[0][Lb.index:Lb.index + Lb.c].double()
        rv0 = running0[1][Lb.index:Lb.index + Lb.c].double()
        unb = n / (n - 1.0)
        brm = 0.1 * dmean + 2.0 ** -22 * (0.9 * rm0.abs() + 0.1 * m.abs())
        brv = 0.1 * unb * dvar + 2.0 ** -22 * (0.9 * rv0.abs() + 0.1 * unb * var.abs())
        res[3] = max(float(((rm - (0.9 * rm0 + 0.1 * m)).abs() / brm.clamp(min=1e-300)).max()),
                     float(((rv - (0.9 * rv0 + 0.1 * unb * var)).abs() / brv.clamp(min=1e-300)).max()))
    return res


def check_all(net, plan, running0=None, label="enc"):
    flat = net.store.flat.detach().cpu()
    entries = [e for e in plan._b16_log if e["kind"] == "enc_fwd"]
    assert entries
    bad = {}
    for e in entries:
        r = local_check(net, e, flat, running0)
        print(f"{label} layer-local {e['what']:44s} error / bound: conv {r[0]:.4f}  mean {r[1] if r[1] is None else round(r[1], 4)}  "
              f"invstd {r[2] if r[2] is None else round(r[2], 4)}  running {r[3] if r[3] is None else round(r[3], 4)}")
        if not all(x is None or x <= 1.0 for x in r):
            bad[e["what"]] = r
    assert not bad, bad
    return entries


@pytest.fixture(scope="module")
def ref(Z, deterministic):
    """one step of the fp32 net and of the bf16_fwd net on the module's set-up (computed once, never modified)"""
    inp = batch()
    cfg, net32 = build(Z)
    o32, l32, g32 = step(Z, cfg, net32, inp)
    cfg16, net16 = build(Z, enc_dtype="bf16_fwd")
    assert net16._enc_dtype == "bf16_fwd"
    running0 = (net16._rm.detach().cpu().clone(), net16._rv.detach().cpu().clone())
    o16, l16, g16 = step(Z, cfg16, net16, inp)
    return dict(inp=inp, cfg=cfg, cfg16=cfg16, net32=net32, net16=net16, o32=o32, l32=l32, g32=g32, o16=o16, l16=l16, g16=g16, running0=running0)


def test_programs(Z, ref):
    p32, p16 = train_plan(ref["net32"]), train_plan(ref["net16"])
    (key,) = [k for k in ref["net16"]._plans if k[-1]]
    assert ("enc", "bf16_fwd") in key and not any(isinstance(e, tuple) and e and e[0] == "enc" for e in list(ref["net32"]._plans)[0])
    f32, f16, b32, b16 = listing(p32.fwd), listing(p16.fwd), listing(p32.bwd), listing(p16.bwd)
    assert not any("bf16" in n or "+bf16" in w for prog in (f32, b32, listing(p32.prep), listing(p32.prep_u)) for _, n, w in prog)
    assert not p32._b16_log
    # forward: the same encoder convolutions on the same lanes in the same order, every one behind the stem on a bf16 entry
    c32, c16 = enc_convs(f32), enc_convs(f16)
    assert len(c16) == 19 and [(l, w) for l, _, w in c32] == [(l, w) for l, _, w in c16]          # ResNet-18: 16 block convolutions + 3 projections
    assert all(n in FP32_CONVS for _, n, _ in c32) and all(n in ENC_FNS for _, n, _ in c16)
    assert all(n == "zsg_conv_igemm_bf16_bn" for _, n, _ in c16), "every BatchNorm is live: all carry the fused statistics"
    stem16 = [(l, n, w) for l, n, w in f16 if w.startswith(STEM)]
    assert stem16 and stem16 == [(l, n, w) for l, n, w in f32 if w.startswith(STEM)] and not any("bf16" in n for _, n, _ in stem16)
    assert not any(n.startswith("zsg_conv_wino") and w.startswith(ENC) for _, n, w in f16)
    # everything outside the encoder is the fp32 plan's, launch for launch
    assert [x for x in f16 if not x[2].startswith((ENC, "stats:" + ENC))] == [x for x in f32 if not x[2].startswith((ENC, "stats:" + ENC))]
    # the backward is the fp32 plan's
    assert b16 == b32 and listing(p16.prep) == listing(p32.prep)
    assert set(p16.grad_ready) == set(p32.grad_ready)
    # ONE pack launch per forward, on the side stream with the weight-only work; the main stream waits in front of the first reader
    pu = listing(p16.prep_u)
    assert [n for _, n, _ in pu].count("zsg_pack_w_bf16_batched") == 1 and not any(n == "zsg_pack_w_bf16_batched" for _, n, _ in f16)
    assert len(p16.pack_jobs) == len(c16)
    log = [e for e in p16._b16_log if e["kind"] == "enc_fwd"]
    assert len(log) == len(p16._b16_log) == len(c16)
    assert p16._wait_idx <= min(e["idx"] for e in log)
    for e in log:
        fn, _, what = p16.fwd.calls[e["idx"]]
        assert fn.__name__ == "zsg_conv_igemm_bf16_bn" and what == e["what"] + "+bf16bn"
        assert e["pname"] in ref["net16"].store.entries and e["bn"] in ref["net16"].bns and e["frozen"] is False
        assert e["mean"].numel() == e["invstd"].numel() == e["d"].N


def test_switch_off_lowers_what_a_net_that_never_saw_the_key_lowers(Z, ref):
    cfg, net0 = build(Z, drop_key=True)
    assert "enc_dtype" not in cfg and net0._enc_dtype == "fp32"
    o0, _, g0 = step(Z, cfg, net0, ref["inp"])
    p0, p32 = train_plan(net0), train_plan(ref["net32"])
    assert listing(p0.bwd) == listing(p32.bwd) and listing(p0.fwd) == listing(p32.fwd)
    assert listing(p0.prep) == listing(p32.prep) and listing(p0.prep_u) == listing(p32.prep_u)
    assert list(net0._plans) == list(ref["net32"]._plans)
    assert torch.equal(bits(g0), bits(ref["g32"])) and torch.equal(bits(o0), bits(ref["o32"]))


def test_layer_local(Z, ref):
    """every covered launch of the step in `ref`: the convolution, the statistics it fed its BatchNorm, the running statistics"""
    entries = check_all(ref["net16"], train_plan(ref["net16"]), ref["running0"])
    assert len(entries) == 19


def test_exact_part(Z, ref):
    n32, n16 = ref["net32"], ref["net16"]
    p32, p16 = train_plan(n32), train_plan(n16)
    first = min((e for e in p16._b16_log), key=lambda e: e["idx"])
    a = first["src"]                                                 # the stem's output behind the max-pool
    assert a.name in p32.acts and float(a.buf.abs().max()) > 0
    assert torch.equal(bits(a.buf), bits(p32.acts[a.name].buf)), "the stem's output"
    assert torch.equal(bits(p16.acts["we"].buf), bits(p32.acts["we"].buf)), "the LSTM's output"
    Lb = n16.bns[ENC + "bn1"]
    assert torch.equal(bits(n16._rm[Lb.index:Lb.index + Lb.c]), bits(n32._rm[Lb.index:Lb.index + Lb.c])), "the stem BatchNorm's running mean"
    assert torch.equal(n32._nbt.cpu(), n16._nbt.cpu())


def test_switching_back_gives_fp32_bits_and_eval_ignores_the_switch(Z, ref):
    cfg, net = build(Z)
    assert net.encoder_precision("bf16_fwd") is net
    _, _, g16 = step(Z, cfg, net, ref["inp"])
    assert torch.equal(bits(g16), bits(ref["g16"]))
    assert net.encoder_precision("fp32") is net
    # (a train-mode step reads the batch statistics only: the running statistics the bf16 step left do not enter it)
    o32, _, g32 = step(Z, cfg, net, ref["inp"])
    assert torch.equal(bits(g32), bits(ref["g32"])) and torch.equal(bits(o32), bits(ref["o32"]))
    assert [k for k in net._plans if k[-1]] == [k for k in ref["net32"]._plans if k[-1]], "one training plan, the fp32 key"
    # eval: two nets in the seeded state, one with the switch on
    (_, na), (_, nb) = build(Z, enc_dtype="bf16_fwd"), build(Z)
    na.eval()
    nb.eval()
    with torch.no_grad():
        a, b = na(ref["inp"])["att_bbx_out"], nb(ref["inp"])["att_bbx_out"]
    torch.cuda.synchronize()
    assert torch.equal(bits(a), bits(b))
    ek = [k for k in na._plans if not k[-1]]
    assert ek == list(na._plans) == list(nb._plans) and len(ek) == 1
    assert listing(na._plans[ek[0]].fwd) == listing(nb._plans[ek[0]].fwd) and not na._plans[ek[0]]._b16_log


def test_two_bf16_steps_are_bit_identical(Z, ref):
    cfg, net = build(Z, enc_dtype="bf16_fwd")
    o, _, g = step(Z, cfg, net, ref["inp"])
    assert torch.equal(bits(g), bits(ref["g16"])) and torch.equal(bits(o), bits(ref["o16"]))


def test_bottleneck_and_the_deferred_batchnorm(Z, monkeypatch):
    """ResNet-50 with the deferral threshold at 0: a block's closing BatchNorm is applied by the next block's conv1 (zsg_conv_igemm_bnpre,
    fp32, untouched); its producer conv3 is a bf16 launch whose statistics reach that loader"""
    monkeypatch.setattr(Z["mdl"], "BN_PRE_MIN_MB", 0)
    inp = batch()
    cfg, net = build(Z, arch="resnet50", enc_dtype="bf16_fwd")
    running0 = (net._rm.detach().cpu().clone(), net._rv.detach().cpu().clone())
    _, ls, g = step(Z, cfg, net, inp)
    plan = train_plan(net)
    f = listing(plan.fwd)
    pre = [(i, n, w) for i, (_, n, w) in enumerate(f) if "+bnpre(" in w]
    assert len(pre) >= 8 and all(n == "zsg_conv_igemm_bnpre" for _, n, _ in pre), pre
    log = {e["what"]: e for e in plan._b16_log}
    assert all(e["kind"] == "enc_fwd" for e in log.values())
    for i, _, w in pre:
        consumer, bn_name = w[:w.index("+bnpre(")], w[w.index("+bnpre(") + 7:w.index(")")]
        assert consumer not in log, "the convolution that applies a pending BatchNorm stays fp32"
        prod = bn_name.replace(".bn3", ".conv3")
        assert prod in log and log[prod]["bn"] == bn_name, (prod, bn_name)
        fn, _, what = plan.fwd.calls[log[prod]["idx"]]
        assert fn.__name__ == "zsg_conv_igemm_bf16_bn" and log[prod]["idx"] < i
        ptrs = {getattr(a, "value", None) for a in plan.fwd.calls[i][1]}
        assert log[prod]["mean"].data_ptr() in ptrs and log[prod]["invstd"].data_ptr() in ptrs, "the producer's statistics are the loader's"
    convs = enc_convs(f)
    assert convs and all(n in ENC_FNS for _, n, _ in convs) and len(convs) + len(pre) == 52         # ResNet-50: 48 block convolutions + 4 projections
    assert len(log) == len(convs)
    check_all(net, plan, running0, label="enc r50")
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 and bool(torch.isfinite(ls["loss"]).all())


def test_frozen_encoder_batchnorm(Z, ref):
    """a frozen BatchNorm needs no batch statistics: the plain bf16 launch, normalised with the running statistics"""
    cfg, net = build(Z, enc_dtype="bf16_fwd")
    frozen = set(net.freeze_batchnorm((ENC + "layer3.", ENC + "layer4.0.bn1")))
    assert len(frozen) == 6
    _, ls, g = step(Z, cfg, net, ref["inp"])
    plan = train_plan(net)
    entries = check_all(net, plan, label="enc frozen")
    fns = {e["bn"]: plan.fwd.calls[e["idx"]][0].__name__ for e in entries}
    assert set(fns) >= frozen and len(entries) == 19
    for bn, fn in fns.items():
        assert fn == ("zsg_conv_igemm_bf16" if bn in frozen else "zsg_conv_igemm_bf16_bn"), (bn, fn)
    assert {e["bn"] for e in entries if e["frozen"]} == frozen
    assert [k for k in net._plans if k[-1]][0][5] != () and bool(torch.isfinite(g).all()) and bool(torch.isfinite(ls["loss"]).all())


def test_shared_training(Z):
    inp = shared_batch(Z)
    cfg, net = build(Z, enc_dtype="bf16_fwd")
    net.shared_training(True)
    _, ls, g = step(Z, cfg, net, inp)
    (key,) = [k for k in net._plans if k[-1]]
    assert ("shared", 4) in key and ("enc", "bf16_fwd") in key
    entries = check_all(net, train_plan(net), label="enc shared")
    assert len(entries) == 19 and all(e["out"].B == 2 for e in entries)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 and bool(torch.isfinite(ls["loss"]).all())


def test_all_three_training_switches_together(Z, ref):
    cfg, net = build(Z, enc_dtype="bf16_fwd", train_dtype="bf16_head", wgrad_dtype="bf16")
    cfgh, neth = build(Z, train_dtype="bf16_head", wgrad_dtype="bf16")
    _, _, g = step(Z, cfg, net, ref["inp"])
    step(Z, cfgh, neth, ref["inp"])
    (key,) = [k for k in net._plans if k[-1]]
    assert key[7:-1] == (("wgrad", "bf16"), ("train", "bf16_head"), ("enc", "bf16_fwd"))
    plan, planh = train_plan(net), train_plan(neth)
    assert listing(plan.bwd) == listing(planh.bwd), "the backward is what the other two switches make it"
    assert [n for _, n, _ in listing(plan.prep_u)].count("zsg_pack_w_bf16_batched") == 1, "still one pack launch per forward"
    assert len(plan.pack_jobs) == len(planh.pack_jobs) + 19
    assert sorted({e["kind"] for e in plan._b16_log}) == ["dgrad", "enc_fwd", "fwd"]
    assert [(e["kind"], e["what"]) for e in plan._b16_log if e["kind"] != "enc_fwd"] == [(e["kind"], e["what"]) for e in planh._b16_log]
    check_all(net, plan, label="enc + head + wgrad")
    assert bool(torch.isfinite(g).all())


def test_two_steps_with_clipping_and_adam_stay_finite(Z, ref):
    cfg, net = build(Z, enc_dtype="bf16_fwd")
    opt = Z["optim"].FusedAdam(net, lr=1e-4, betas=(0.9, 0.99))
    w0 = net.store.flat.clone()
    lf = loss_fn(Z, cfg)
    net.train()
    for _ in range(2):
        opt.zero_grad()
        ls = lf(net(ref["inp"]), ref["inp"])
        ls["loss"].mean().backward()
        tn = Z["optim"].clip_grad_norm_(net.parameters(), 1.0)
        opt.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tn)) and float(tn) > 0 and bool(torch.isfinite(net.store.flat).all()) and bool(torch.isfinite(ls["loss"]).all())
    assert not torch.equal(net.store.flat, w0)


def test_rounded_part_against_the_fp32_plan(Z, ref):
    o32, o16, g32, g16 = ref["o32"].double(), ref["o16"].double(), ref["g32"].double(), ref["g16"].double()
    box = float((o16[..., :4] - o32[..., :4]).abs().max() / o32[..., :4].abs().max())
    att = float((o16[..., 4] - o32[..., 4]).abs().max() / o32[..., 4].abs().max())
    l32, l16 = float(ref["l32"]["loss"].double().mean()), float(ref["l16"]["loss"].double().mean())
    rel_loss = abs(l16 - l32) / abs(l32)
    l2 = float((g16 - g32).norm() / g32.norm())
    cos = float((g16 * g32).sum() / (g16.norm() * g32.norm()))
    print(f"enc_bf16 parity: box {box:.3e} att {att:.3e} loss {rel_loss:.3e} ({l32:.6f} -> {l16:.6f}) flat l2 {l2:.3e} 1-cos {1 - cos:.3e}")
    assert not torch.equal(bits(ref["g16"]), bits(ref["g32"])), "the gradient equals the fp32 plan's bit for bit: the switch is not engaged"
    assert not torch.equal(bits(ref["o16"]), bits(ref["o32"]))
    assert math.isfinite(l16) and bool(torch.isfinite(g16).all())
    assert box <= BOUND_BOX and att <= BOUND_ATT, (box, att)
    assert rel_loss <= BOUND_LOSS, rel_loss
    assert l2 <= BOUND_L2 and cos >= BOUND_COS, (l2, cos)
