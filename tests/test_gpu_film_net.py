"""cfg lang_fuse = "film" on the network, against tests/film_ref.py.

Geometry and rules of tests/test_gpu_langpool_net.py (ResNet-18, B = 3, 96 x 128, queries of up to 13 tokens, seeded_state_dict seed 12):
the float64 twin of film_ref.zsgnet_forward is the truth, the same code in float32 on the CPU the yardstick — forward max error within
6 x CPU-fp32 + 1e-4, every parameter gradient (film.weight included) within grad_tol, losses rel 2e-4.  film.weight is not in the oracle's
seeded weights: it is drawn here (seeded, N(0, 0.05^2): gamma of a few tenths), so that the scale is not 1.

The shared-image, flip-TTA, reduced-precision and checkpoint tests use the set-ups of the tests they name (ResNet-18, 128 px,
ZSG_AUTOTUNE=0 and ZSG_DETERMINISTIC=1: two forwards of one plan give the same bits), with those tests' own bounds.
No SSD-VGG case: its 300 x 300 plan takes well over the few seconds a case of this suite may take (tests/test_gpu_shared_train.py's
ssd_vgg case is the slowest of that file); the lowering under test sits behind the pyramid and does not see the trunk's kind."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import film_ref as FR  # noqa: E402
import test_gpu_net_lstm as TN  # noqa: E402
import tta_ref  # noqa: E402
from oracle import zsg_oracle as O  # noqa: E402
from test_gpu_net import Z, grad_tol, to_dev  # noqa: E402,F401

ARCH, B = TN.ARCH, TN.B
# tests/test_gpu_net_bf16.py, tests/test_gpu_net_bf16_act.py, tests/test_gpu_net_train_bf16_head.py: their bounds against the fp32 plan
BF16_BOX, BF16_ATT = 5e-2, 6e-2
ACT_BOX, ACT_ATT = 6e-2, 7e-2
HEAD_BOX, HEAD_ATT, HEAD_LOSS, HEAD_L2, HEAD_COS = 4e-2, 3e-2, 7e-3, 0.3, 1 - 8e-3


@pytest.fixture(scope="module", autouse=True)
def _leave_the_tuner_as_found():
    """as tests/test_gpu_net_lstm.py: the launch shapes tuned for this module's plans must not outlive it"""
    if not torch.cuda.is_available():
        yield
        return
    from zsgnet_pytorch_amd import ops
    saved = dict(ops._TUNE_CACHE)
    yield
    ops._TUNE_CACHE.clear()
    ops._TUNE_CACHE.update(saved)


@pytest.fixture()
def fixed_tiles(monkeypatch):
    """no tile choice by timing, no fp32 atomics (tests/test_gpu_tta_net.py)"""
    from zsgnet_pytorch_amd._lib import lib
    monkeypatch.setenv("ZSG_DETERMINISTIC", "1")
    monkeypatch.setenv("ZSG_AUTOTUNE", "0")
    lib.zsg_set_deterministic(1)
    yield
    lib.zsg_set_deterministic(0)


def film_keys(cfg):
    return ["att_reg_box.film.weight"] if cfg["use_same_atb"] else ["att_box.film.weight", "reg_box.film.weight"]


def seeded(cfg, seed, head_in, zero=False):
    """the oracle's seeded weights of the cfg's heads, plus drawn film weights (and a drawn scorer for attn)"""
    sd = O.seeded_state_dict(ARCH, seed, head_in=head_in, same_atb=bool(cfg["use_same_atb"]))
    D = cfg["lstm_dim"] * (2 if cfg["use_bidirectional"] else 1)
    g = torch.Generator().manual_seed(seed + 200)
    if cfg["lang_pool"] == "attn":
        sd["lang_pool.weight"] = torch.randn(1, D, generator=g) * 0.25
    if cfg["lang_fuse"] == "film":
        for k in film_keys(cfg):
            sd[k] = torch.zeros(256, D) if zero else torch.randn(256, D, generator=g) * 0.05
    return sd


def build(Z, seed, zero=False, **flags):
    config, evaluator, loss, mdl, optim = Z
    cfg = config.get_cfg(resnet_arch=ARCH, **flags)
    net = mdl.get_default_net(9, cfg)
    sd = seeded(cfg, seed, net.start_dim_head, zero)
    assert set(net.state_dict().keys()) == set(sd.keys())
    net.load_state_dict(sd)
    net.to("cuda")
    r, s = config.ratios_scales(cfg)
    return cfg, net, sd, loss.get_default_loss(r, s, cfg)


def ref_kw(cfg, training=True):
    return dict(arch=ARCH, training=training, do_norm=bool(cfg["do_norm"]), bidirectional=cfg["use_bidirectional"], lang_pool=cfg["lang_pool"])


def with_zero_film(sd, cfg):
    """the weights as film_ref reads them, film.weight = 0 where the state dict has none: the `concat` network's function"""
    D = cfg["lstm_dim"] * (2 if cfg["use_bidirectional"] else 1)
    out = dict(sd)
    for k in (["att_reg_box.film.weight"] if cfg["use_same_atb"] else ["att_box.film.weight", "reg_box.film.weight"]):
        out[k] = torch.zeros(256, D, dtype=next(iter(sd.values())).dtype)
    return out


def twin64(sd, bt, h0, c0, anc, **kw):
    """test_gpu_net.fp64_twin on film_ref.zsgnet_forward"""
    sd64 = {k: (v.detach().double().requires_grad_(v.requires_grad) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    bt64 = {k: v.double() for k, v in bt.items()}
    ref = FR.zsgnet_forward(sd64, bt64, h0.double(), c0.double(), rank=O.sort_rank(bt["qlens"]), **kw)
    ls = O.torch_loss(ref, bt["annot"], anc)
    ls["loss"].backward()
    return sd64, ref, ls


def out5(ref):
    return torch.cat([ref["bbx_out"], ref["att_out"]], 2).detach().double()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def whats(prog):
    return [c[2] for c in prog.calls]


def names(prog):
    return [c[0].__name__ for c in prog.calls]


def train_plan(net):
    ps = [p for k, p in net._plans.items() if k[-1]]
    assert len(ps) == 1
    return ps[0]


def dev_inp(bt, h0, c0):
    inp = to_dev(bt)
    inp["h0"], inp["c0"] = h0, c0
    return inp


CASES = {"same_atb": dict(), "two_heads": dict(use_same_atb=False), "do_norm": dict(do_norm=True), "attn": dict(lang_pool="attn")}


def check_against_reference(cfg, net, sd, lf, bt, h0, c0, tag, sd_ref=None, gap_from_concat=True):
    """one training forward + loss + backward of `net` against film_ref on the weights sd_ref (default: sd); returns (sd32, sd64)"""
    inp = dev_inp(bt, h0, c0)
    out = net(inp)
    kw = ref_kw(cfg)
    sd32 = TN.leaves(sd if sd_ref is None else sd_ref)
    ref = FR.zsgnet_forward(sd32, bt, h0, c0, **kw)
    assert out["feat_sizes"].tolist() == ref["feat_sizes"].tolist()
    anc, A = TN.anchors_of(ref)
    assert out["att_bbx_out"].shape == (B, A, 5)
    sd64, ref64, ls64 = twin64(sd32, bt, h0, c0, anc, **kw)
    o_gpu, o_cpu, o_64 = out["att_bbx_out"].detach().cpu().double(), out5(ref), out5(ref64)
    e_gpu, e_cpu = float((o_gpu - o_64).abs().max()), float((o_cpu - o_64).abs().max())
    tol = 6 * e_cpu + 1e-4
    print(f"forward {tag}: HIP err {e_gpu:.3g} vs fp64, CPU fp32 err {e_cpu:.3g}")
    if gap_from_concat:
        # the switch matters on this batch: the float64 output of the same weights under `concat` is far outside what is allowed
        with torch.no_grad():
            c64 = FR.zsgnet_forward(with_zero_film({k: v.detach() for k, v in sd64.items()}, cfg), {k: v.double() for k, v in bt.items()},
                                    h0.double(), c0.double(), rank=O.sort_rank(bt["qlens"]), **kw)
        gap = float((out5(c64) - o_64).abs().max())
        print(f"forward {tag}: |film - concat| {gap:.3g} in float64, allowed error {tol:.3g}")
        assert gap > 100 * tol, f"{tag}: the float64 outputs of film and concat differ by {gap:.3g} only (allowed error {tol:.3g})"
    assert e_gpu <= tol, f"forward: HIP err {e_gpu:.3g} vs fp64, CPU fp32 err {e_cpu:.3g}"
    ls = lf(out, inp)
    for k in ("loss", "cls_ls", "box_ls"):
        np.testing.assert_allclose(ls[k].item(), ls64[k].item(), rtol=2e-4, err_msg=k)
    O.torch_loss(ref, bt["annot"], anc)["loss"].backward()
    ls["loss"].backward()
    torch.cuda.synchronize()
    return sd32, sd64


@pytest.mark.parametrize("tag", list(CASES))
def test_forward_backward_vs_reference(Z, tag):
    cfg, net, sd, lf = build(Z, 12, lang_fuse="film", **CASES[tag])
    net.train()
    bt, h0, c0 = TN.batch(cfg)
    sd32, sd64 = check_against_reference(cfg, net, sd, lf, bt, h0, c0, tag)
    for k in film_keys(cfg):
        assert float(sd64[k].grad.abs().max()) > 0
    worst = TN.grad_errors(net, sd32, sd64)
    assert not worst, f"gradient error vs fp64 (HIP rel, CPU-fp32 rel): {worst[:8]}"
    plan = train_plan(net)
    fw, bw = whats(plan.fwd), whats(plan.bwd)
    for p in (k[:-len(".film.weight")] for k in film_keys(cfg)):
        assert p + "0.gamma" in fw and p + ".0.0.film" in fw and p + ".0.0.feat" in fw and "lmap" not in fw
        assert p + ".0.0.film_bwd" in bw and "dgamma:" + p in bw and "wgrad:" + p + ".film" in bw and "dwe.film:" + p in bw
        assert p + ".film.weight" in plan.grad_ready, "the DDP bucket plan must know when the new gradient is complete"
        # gamma sits on the side stream beside V, hoisted with the language maps in front of the pyramid
        i = fw.index(p + "0.gamma")
        assert plan.fwd.lanes[i] == 1 and plan.fwd.lanes[fw.index(p + "0.V")] == 1 and abs(i - fw.index(p + "0.V")) == 1
        assert i < max(j for j, w in enumerate(fw) if w.startswith("backbone.")), "not hoisted: it sits behind the whole trunk"


def test_zero_weight_is_concat(Z):
    """film.weight = 0 (its initial value): the film net computes the concat net's function.  Both plans form conv0 differently (one
    GEMM with an additive map against a raw accumulator with an epilogue launch: the difference between the plain and the shared form
    of tests/test_gpu_shared_train.py), so each is held to that file's bounds against the SAME float64 reference — the forward within
    6 x CPU-fp32 + 1e-4, the loss to 2e-4, every shared gradient within grad_tol."""
    cfg_f, net_f, sd_f, lf = build(Z, 12, zero=True, lang_fuse="film")
    cfg_c, net_c, sd_c, _ = build(Z, 12)
    assert {k: v for k, v in sd_f.items() if k in sd_c}.keys() == sd_c.keys() and all(torch.equal(sd_f[k], sd_c[k]) for k in sd_c)
    bt, h0, c0 = TN.batch(cfg_f)
    net_f.train(), net_c.train()
    sd32, sd64 = check_against_reference(cfg_f, net_f, sd_f, lf, bt, h0, c0, "film(0)", gap_from_concat=False)
    worst = TN.grad_errors(net_f, sd32, sd64)
    assert not worst, f"film(0) gradient error vs fp64: {worst[:8]}"
    assert float(dict(net_f.named_parameters())["att_reg_box.film.weight"].grad.abs().max()) > 0, "a zero weight still gets a gradient"
    # the concat net against the very same float64 twin (film_ref with a zero weight IS the oracle: tests/test_cpu_film.py)
    sd32c, sd64c = check_against_reference(cfg_c, net_c, sd_c, lf, bt, h0, c0, "concat", sd_ref=sd_f, gap_from_concat=False)
    worst = TN.grad_errors(net_c, sd32c, sd64c)
    assert not worst, f"concat gradient error vs the film(0) twin: {worst[:8]}"
    with torch.no_grad():
        d = float((net_f(dev_inp(bt, h0, c0))["att_bbx_out"] - net_c(dev_inp(bt, h0, c0))["att_bbx_out"]).abs().max())
    print(f"film(0) vs concat: max|diff| of the outputs {d:.3e}")


def test_concat_builds_no_film_launch(Z, fixed_tiles):
    """the default keeps its programs: no film / gamma launch, conv0 with its fused epilogue and the packed language map"""
    from zsgnet_pytorch_amd import synth
    cfg, net, sd, lf = build(Z, 12)
    net.train()
    bt, h0, c0 = TN.batch(cfg)
    inp = dev_inp(bt, h0, c0)
    lf(net(inp), inp)["loss"].backward()
    net.eval()
    with torch.no_grad():
        net(inp)
        sb = synth.synthetic_shared_batch(2, 4, 128, 128, seed=5)
        g = torch.Generator().manual_seed(1)
        net(dev_inp(sb, torch.randn(2, 4, 128, generator=g), torch.randn(2, 4, 128, generator=g)))
    torch.cuda.synchronize()
    assert len(net._plans) == 3
    for p in net._plans.values():
        for prog in (p.fwd, p.bwd):
            assert not [n for n in names(prog) if "film" in n], names(prog)
            assert not [w for w in whats(prog) if "film" in w or "gamma" in w]
    tp = train_plan(net)
    assert "lmap" in whats(tp.fwd) and "att_reg_box.0.0" in whats(tp.fwd) and "att_reg_box.0.0.feat" not in whats(tp.fwd)
    assert "zsg_head_shared_conv0" in [n for p in net._plans.values() for n in names(p.fwd)]


def tta_build(Z, zero=False, **flags):
    """tests/test_gpu_tta_net.py's network (ResNet-18, seeded_state_dict seed 1) with drawn film weights"""
    config, evaluator, loss, mdl, optim = Z
    cfg = config.get_cfg(resnet_arch=ARCH, **flags)
    net = mdl.get_default_net(9, cfg)
    net.load_state_dict(seeded(cfg, 1, net.start_dim_head, zero))
    return cfg, net.to("cuda").eval()


def fwd5(net, bt, h0, c0):
    with torch.no_grad():
        out = net(dev_inp(bt, h0, c0))
    torch.cuda.synchronize()
    return out["att_bbx_out"].detach().clone(), out


def test_shared_image_eval(Z, fixed_tiles):
    """Q = 6 queries over 3 images against the plain film forward of the expanded batch, by the rule of tests/test_gpu_shared_net.py as
    tests/test_gpu_langpool_net.py states it: within 2e-4 of the output's scale of the CPU definition, and no further from it than
    max(4 x the plain path's distance, 2e-3).  Under film both plans run the same kind of launches (the plain plan passes the identity
    index)."""
    from zsgnet_pytorch_amd import synth
    cfg, net = tta_build(Z, lang_fuse="film")
    bt = synth.synthetic_shared_batch(3, 6, 128, 128, seed=5)
    g = torch.Generator().manual_seed(1)
    h0, c0 = torch.randn(2, 6, 128, generator=g), torch.randn(2, 6, 128, generator=g)
    s, _ = fwd5(net, bt, h0, c0)
    p, _ = fwd5(net, synth.expand_shared(bt), h0, c0)
    shared = [pl for k, pl in net._plans.items() if "shared" in k]
    plain = [pl for k, pl in net._plans.items() if "shared" not in k]
    assert len(shared) == 1 and len(plain) == 1 and tuple(s.shape) == tuple(p.shape) and s.shape[0] == 6
    assert "zsg_head_film_conv0" in names(shared[0].fwd) and "zsg_head_film_conv0" in names(plain[0].fwd)
    assert "zsg_head_shared_conv0" not in names(shared[0].fwd)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        ref = FR.zsgnet_forward(sd, synth.expand_shared(bt), h0, c0, **ref_kw(cfg, training=False))
    want = torch.cat([ref["bbx_out"], ref["att_out"]], 2)
    scale = float(want.abs().max())
    d_s, d_p = float((s.cpu() - want).abs().max()), float((p.cpu() - want).abs().max())
    print(f"shared film eval: max|shared - ref| {d_s:.3e}, max|plain - ref| {d_p:.3e}, max|shared - plain| {float((s - p).abs().max()):.3e}, scale {scale:.3e}")
    assert d_s < 2e-4 * scale and d_s <= max(4 * d_p, 2e-3)
    # and the scale is engaged: the same weights with film.weight = 0 give another output
    with torch.no_grad():
        net.state_dict()["att_reg_box.film.weight"].zero_()
    z, _ = fwd5(net, bt, h0, c0)
    assert float((z - s).abs().max()) > 1e-2 * scale


def test_shared_image_training(Z):
    """6 queries over 3 images, BatchNorm frozen (then the shared step IS the plain step on the expanded batch): the shared film step and
    the plain film step, each against the float64 twin of film_ref on the expanded batch with tests/test_gpu_shared_train.py's bounds"""
    from zsgnet_pytorch_amd import synth
    bt = synth.synthetic_shared_batch(3, 6, 96, 96, seed=21, tmax=13)
    bt["img_idx"] = torch.tensor([1, 0, 2, 0, 2, 1])
    bt["qlens"][-1] = bt["qlens"][0]
    g = torch.Generator().manual_seed(22)
    h0, c0 = torch.randn(2, 6, 128, generator=g), torch.randn(2, 6, 128, generator=g)
    ex = synth.expand_shared(bt)
    cfg, net, sd, lf = build(Z, 11, lang_fuse="film")
    kw = ref_kw(cfg, training=False)
    sd32 = TN.leaves(sd)
    ref = FR.zsgnet_forward(sd32, ex, h0, c0, **kw)
    anc, A = TN.anchors_of(ref)
    O.torch_loss(ref, ex["annot"], anc)["loss"].backward()
    sd64, ref64, ls64 = twin64(sd32, ex, h0, c0, anc, **kw)
    o_64 = out5(ref64)
    e_cpu = float((out5(ref) - o_64).abs().max())
    outs = {}
    for form in ("shared", "plain"):
        cfg, net, sd, lf = build(Z, 11, lang_fuse="film")
        net.train()
        net.freeze_batchnorm()
        net.shared_training(form == "shared")
        inp = dev_inp(bt if form == "shared" else ex, h0, c0)
        out = net(inp)
        o = out["att_bbx_out"].detach().cpu().double()
        outs[form] = o
        e = float((o - o_64).abs().max())
        ls = lf(out, inp)
        print(f"film {form} training step: max|out - fp64| {e:.3e} (CPU fp32 {e_cpu:.3e}), loss {ls['loss'].item():.6f} vs {ls64['loss'].item():.6f}")
        assert e <= 6 * e_cpu + 1e-4
        np.testing.assert_allclose(ls["loss"].item(), ls64["loss"].item(), rtol=2e-4)
        ls["loss"].backward()
        torch.cuda.synchronize()
        worst = TN.grad_errors(net, sd32, sd64)
        assert not worst, f"{form}: gradient error vs fp64 (HIP rel, CPU-fp32 rel): {worst[:8]}"
        bw = names(train_plan(net).bwd)
        assert "zsg_head_film_conv0_bwd" in bw and "zsg_head_film_dgamma" in bw and "zsg_head_shared_conv0_bwd" not in bw
    print(f"film shared vs plain training forward: max|diff| {float((outs['shared'] - outs['plain']).abs().max()):.3e}")


def test_flip_tta(Z, fixed_tiles):
    """eval_tta = flip: merge_ref of ONE plain eval forward of the 2B rows tta_batch builds, bit for bit (tests/test_gpu_tta_net.py)"""
    cfg, net = tta_build(Z, lang_fuse="film", eval_tta="flip")
    bt = O.synthetic_batch(2, 128, 128, seed=3)
    g = torch.Generator().manual_seed(0)
    h0, c0 = torch.randn(2, 2, 128, generator=g), torch.randn(2, 2, 128, generator=g)
    bt["qvec_flip"] = torch.randn(bt["qvec"].shape, generator=g) * 0.35
    o, out = fwd5(net, bt, h0, c0)
    sizes = [tuple(s) for s in out["feat_sizes"].tolist()]
    bt2, h2, c2 = tta_ref.tta_batch(bt, h0, c0)
    net.eval_tta("none")
    x2, _ = fwd5(net, bt2, h2, c2)
    assert tuple(x2.shape)[0] == 4 and tuple(o.shape)[0] == 2
    assert torch.equal(bits(torch.from_numpy(np.ascontiguousarray(tta_ref.merge_ref(x2.cpu().numpy(), sizes, 9)))), bits(o))
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        want = FR.zsgnet_forward(sd, bt2, h2, c2, **ref_kw(cfg, training=False))
    np.testing.assert_allclose(x2.cpu().numpy(), torch.cat([want["bbx_out"], want["att_out"]], 2).numpy(), rtol=2e-3, atol=5e-3)


def rel(a, b):
    """(box, att): max|a - b| / max|b| over the box channels and over the att channel (tests/test_gpu_net_bf16.py)"""
    a, b = a.double().cpu(), b.double().cpu()
    return (float((a[..., :4] - b[..., :4]).abs().max() / b[..., :4].abs().max()), float((a[..., 4] - b[..., 4]).abs().max() / b[..., 4].abs().max()))


@pytest.mark.parametrize("dtype,bb,ba", [("bf16", BF16_BOX, BF16_ATT), ("bf16_act", ACT_BOX, ACT_ATT)])
def test_reduced_precision_eval(Z, fixed_tiles, dtype, bb, ba):
    """eval_dtype = bf16 / bf16_act against the fp32 film plan, within the bounds of those switches' own net tests"""
    cfg, net = tta_build(Z, lang_fuse="film")
    bt = O.synthetic_batch(2, 128, 128, seed=3)
    g = torch.Generator().manual_seed(0)
    h0, c0 = torch.randn(2, 2, 128, generator=g), torch.randn(2, 2, 128, generator=g)
    o32, _ = fwd5(net, bt, h0, c0)
    net.eval_precision(dtype)
    o16, _ = fwd5(net, bt, h0, c0)
    plan = [p for k, p in net._plans.items() if dtype in k][0]
    i = names(plan.fwd).index("zsg_head_film_conv0")
    flag = plan.fwd.calls[i][1][-1]
    assert int(getattr(flag, "value", flag)) == int(dtype == "bf16_act"), "h1 is stored as bf16 exactly under bf16_act"
    assert ("zsg_conv_igemm_bf16_io" if dtype == "bf16_act" else "zsg_conv_igemm_bf16") in names(plan.fwd)
    rb, ra = rel(o16, o32)
    print(f"film {dtype} eval parity: box {rb:.3e} att {ra:.3e} of max|fp32|")
    assert not torch.equal(o16, o32) and rb <= bb and ra <= ba


def test_bf16_head_training(Z, fixed_tiles):
    """train_dtype = bf16_head against the fp32 film plan, within the bounds of tests/test_gpu_net_train_bf16_head.py"""
    res = {}
    bt = O.synthetic_batch(2, 128, 128, seed=3)
    g = torch.Generator().manual_seed(0)
    h0, c0 = torch.randn(2, 2, 128, generator=g), torch.randn(2, 2, 128, generator=g)
    for dt in ("fp32", "bf16_head"):
        config, evaluator, loss, mdl, optim = Z
        cfg, net = tta_build(Z, lang_fuse="film")
        net.train()
        net.train_precision(dt)
        r, s = config.ratios_scales(cfg)
        inp = dev_inp(bt, h0, c0)
        net.store.grad.zero_()
        out = net(inp)
        ls = loss.get_default_loss(r, s, cfg)(out, inp)["loss"].mean()
        ls.backward()
        torch.cuda.synchronize()
        res[dt] = (out["att_bbx_out"].detach().cpu().double(), float(ls), net.store.grad.detach().cpu().double().clone())
        if dt == "bf16_head":
            assert "att_reg_box.0.0.feat+bf16" in whats(train_plan(net).fwd)
    (o32, l32, g32), (o16, l16, g16) = res["fp32"], res["bf16_head"]
    box, att = rel(o16, o32)
    rel_loss, l2 = abs(l16 - l32) / abs(l32), float((g16 - g32).norm() / g32.norm())
    cos = float((g16 * g32).sum() / (g16.norm() * g32.norm()))
    print(f"film bf16_head parity: box {box:.3e} att {att:.3e} loss {rel_loss:.3e} flat l2 {l2:.3e} 1-cos {1 - cos:.3e}")
    assert not torch.equal(g16, g32)
    assert box <= HEAD_BOX and att <= HEAD_ATT and rel_loss <= HEAD_LOSS and l2 <= HEAD_L2 and cos >= HEAD_COS


@pytest.mark.parametrize("only_film", [True, False], ids=["only_film_trains", "film_frozen"])
def test_frozen_parameters(Z, only_film):
    """as tests/test_gpu_finetune.py: a frozen tensor keeps p.grad None and its bits across an optimizer step; a frozen film.weight
    still passes the gradient on to `we` and Y, a frozen rest still trains film.weight"""
    config, evaluator, loss, mdl, optim = Z
    cfg, net, sd, lf = build(Z, 12, lang_fuse="film")
    net.train()
    name = "att_reg_box.film.weight"
    for n, p in net.named_parameters():
        p.requires_grad_((n == name) == only_film)
    opt = optim.FusedAdam(net, lr=1e-3, betas=(0.9, 0.99))
    before = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    bt, h0, c0 = TN.batch(cfg)
    inp = dev_inp(bt, h0, c0)
    opt.zero_grad()
    lf(net(inp), inp)["loss"].backward()
    torch.cuda.synchronize()
    # the gradients that exist are the float64 twin's
    kw = ref_kw(cfg)
    sd32 = TN.leaves(sd)
    ref = FR.zsgnet_forward(sd32, bt, h0, c0, **kw)
    anc, _ = TN.anchors_of(ref)
    sd64, _, _ = twin64(sd32, bt, h0, c0, anc, **kw)
    O.torch_loss(ref, bt["annot"], anc)["loss"].backward()
    for n, p in net.named_parameters():
        if not p.requires_grad:
            assert p.grad is None, n
            continue
        g64 = sd64[n].grad.flatten()
        eg, ec = float((p.grad.cpu().double().flatten() - g64).norm()), float((sd32[n].grad.double().flatten() - g64).norm())
        assert eg <= grad_tol(ec, g64), (n, eg, ec)
    bw = whats(train_plan(net).bwd)
    if only_film:
        assert "dgamma:att_reg_box" in bw and "wgrad:att_reg_box.film" in bw
        assert not [w for w in bw if w.endswith(".film_bwd") or w.startswith(("dwe", "dgrad:att_reg_box.0.0", "wgrad:att_reg_box.0.0")) or "backbone" in w or "lstm" in w], bw
    else:
        assert "att_reg_box.0.0.film_bwd" in bw and "dgamma:att_reg_box" in bw and "dwe.film:att_reg_box" in bw and "wgrad:att_reg_box.film" not in bw
    opt.step()
    torch.cuda.synchronize()
    after = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    for n, p in net.named_parameters():
        same = torch.equal(bits(after[n]), bits(before[n]))
        assert same == (not p.requires_grad), f"{n}: {'moved' if not same else 'did not move'}"


@pytest.mark.parametrize("opt_fn", ["Adam", "LAMB"])
def test_an_optimizer_step_moves_the_weight(Z, opt_fn):
    config, evaluator, loss, mdl, optim = Z
    cfg, net, sd, lf = build(Z, 12, zero=True, lang_fuse="film", opt_fn=opt_fn)
    net.train()
    opt = optim.make_opt_fn(cfg)(net, lr=1e-3)
    bt, h0, c0 = TN.batch(cfg)
    inp = dev_inp(bt, h0, c0)
    for _ in range(2):          # (LAMB's trust ratio of a zero tensor: the first step leaves zero weights to the plain rule; two steps move either way)
        opt.zero_grad()
        lf(net(inp), inp)["loss"].backward()
        opt.step()
    torch.cuda.synchronize()
    w = net.state_dict()["att_reg_box.film.weight"]
    assert bool(torch.isfinite(w).all()) and float(w.abs().max()) > 0, "film.weight did not move from its zero start"


def test_checkpoint_round_trip_through_learner(Z, fixed_tiles, tmp_path):
    from zsgnet_pytorch_amd.trainer import Learner
    config, evaluator, loss, mdl, optim = Z

    def learner(uid, **flags):
        cfg = config.get_cfg(resnet_arch=ARCH, tmp_path=str(tmp_path), **flags)
        net = mdl.get_default_net(9, cfg)
        r, s = config.ratios_scales(cfg)
        return cfg, net, Learner(uid, None, net, loss.get_default_loss(r, s, cfg), cfg, evaluator.get_default_eval(r, s, cfg), None)
    cfg, net, la = learner("film_a", lang_fuse="film")
    net.load_state_dict(seeded(cfg, 1, net.start_dim_head))
    net.to("cuda").eval()
    la.save_model_dict()
    ck = torch.load(la.model_file)["model_state_dict"]
    assert float(ck["att_reg_box.film.weight"].abs().max()) > 0
    cfg_b, other, lb = learner("film_b", lang_fuse="film")
    assert not other.state_dict()["att_reg_box.film.weight"].any()
    assert lb.load_model_dict(str(la.model_file))
    other.to("cuda").eval()
    assert torch.equal(bits(other.state_dict()["att_reg_box.film.weight"]), bits(ck["att_reg_box.film.weight"]))
    bt = O.synthetic_batch(2, 128, 128, seed=3)
    g = torch.Generator().manual_seed(0)
    h0, c0 = torch.randn(2, 2, 128, generator=g), torch.randn(2, 2, 128, generator=g)
    o_a = fwd5(net, bt, h0, c0)[0]
    assert torch.equal(bits(o_a), bits(fwd5(other, bt, h0, c0)[0]))
    # a concat checkpoint into a film net: refused by default, taken with strict_load = False and then the concat net's function
    cfg_c, plain, lc = learner("concat_c")
    plain.load_state_dict({k: v for k, v in ck.items() if "film" not in k})
    plain.to("cuda").eval()
    lc.save_model_dict()
    _, strict, ls_ = learner("film_strict", lang_fuse="film")
    with pytest.raises(RuntimeError, match="film.weight"):
        ls_.load_model_dict(str(lc.model_file))
    _, loose, ll = learner("film_loose", lang_fuse="film", strict_load=False)
    assert ll.load_model_dict(str(lc.model_file))
    loose.to("cuda").eval()
    assert not loose.state_dict()["att_reg_box.film.weight"].any()
    o_c, o_l = fwd5(plain, bt, h0, c0)[0], fwd5(loose, bt, h0, c0)[0]
    scale = float(o_c.abs().max())
    print(f"concat checkpoint in a film net: max|diff| {float((o_l - o_c).abs().max()):.3e} at scale {scale:.3e}; film vs concat weights {float((o_a - o_c).abs().max()):.3e}")
    assert float((o_l - o_c).abs().max()) <= 1e-4 * max(1.0, scale)       # (two fp32 evaluations of one function: tests/test_gpu_langpool_net.py's floor)
    assert float((o_a - o_c).abs().max()) > 1e-2 * scale
