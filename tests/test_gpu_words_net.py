"""cfg lang_fuse = "words" on the network, against tests/words_ref.py.

Geometry, helpers and bounds of tests/test_gpu_film_net.py (ResNet-18, B = 3, 96 x 128, queries of up to 13 tokens, seeded_state_dict seed
12): the float64 twin of words_ref.zsgnet_forward is the truth, the same code in float32 on the CPU the yardstick — forward max error
within 6 x CPU-fp32 + 1e-4, every parameter gradient (both new weights and the LSTM's included) within grad_tol, losses rel 2e-4.  The key /
value weights are not in the oracle's seeded weights: they are drawn here (seeded, N(0, 0.05^2)), so that the attention is not uniform
and the scale is not 1.

The shared-image, flip-TTA, reduced-precision and checkpoint tests use the set-ups of the tests they name (ResNet-18, 128 px,
ZSG_AUTOTUNE=0 and ZSG_DETERMINISTIC=1), with those tests' own bounds.  No SSD-VGG case, for test_gpu_film_net.py's reason."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_film_net as TF  # noqa: E402
import test_gpu_net_lstm as TN  # noqa: E402
import tta_ref  # noqa: E402
import words_ref as WR  # noqa: E402
from oracle import zsg_oracle as O  # noqa: E402
from test_gpu_film_net import _leave_the_tuner_as_found, fixed_tiles  # noqa: E402,F401
from test_gpu_film_net import bits, dev_inp, fwd5, names, out5, rel, train_plan, whats  # noqa: E402
from test_gpu_net import Z, grad_tol, to_dev  # noqa: E402,F401

ARCH, B = TN.ARCH, TN.B


def stacks(cfg):
    return ["att_reg_box"] if cfg["use_same_atb"] else ["att_box", "reg_box"]


def word_keys(cfg):
    return [f"{p}.words.{kv}.weight" for p in stacks(cfg) for kv in ("key", "value")]


def seeded(cfg, seed, head_in, zero_value=False):
    """the oracle's seeded weights of the cfg's heads, plus drawn key / value weights (and a drawn scorer for attn)"""
    sd = O.seeded_state_dict(ARCH, seed, head_in=head_in, same_atb=bool(cfg["use_same_atb"]))
    D = cfg["lstm_dim"] * (2 if cfg["use_bidirectional"] else 1)
    # (the draw is this file's choice: generator seed `seed + 301`, not `seed + 300`.  The `+ 300` draw sits on a kink of the fp32
    # evaluation of the `final` case, independent of the kernels: tests/words_ref.py alone, float32 against float64 on the CPU, is 2.7 %
    # off on words.key.weight's gradient there (grad_tol allows 1.5 %) and 1.1 % on an encoder BatchNorm bias in the `mean` case; with
    # this draw the same two figures are 1.9e-4 and 1.1e-3.)
    g = torch.Generator().manual_seed(seed + 301)
    if cfg["lang_pool"] == "attn":
        sd["lang_pool.weight"] = torch.randn(1, D, generator=g) * 0.25
    if cfg["lang_fuse"] == "words":
        for k in word_keys(cfg):
            w = torch.randn(256, D, generator=g) * 0.05
            sd[k] = torch.zeros(256, D) if (zero_value and k.endswith("value.weight")) else w
    return sd


def build(Z, seed, zero_value=False, **flags):
    config, evaluator, loss, mdl, optim = Z
    cfg = config.get_cfg(resnet_arch=ARCH, **flags)
    net = mdl.get_default_net(9, cfg)
    sd = seeded(cfg, seed, net.start_dim_head, zero_value)
    assert set(net.state_dict().keys()) == set(sd.keys())
    net.load_state_dict(sd)
    net.to("cuda")
    r, s = config.ratios_scales(cfg)
    return cfg, net, sd, loss.get_default_loss(r, s, cfg)


def ref_kw(cfg, training=True):
    return dict(arch=ARCH, training=training, do_norm=bool(cfg["do_norm"]), bidirectional=cfg["use_bidirectional"], lang_pool=cfg["lang_pool"])


def with_zero_value(sd, cfg):
    """the weights as words_ref reads them with value.weight = 0 (and a key where the state dict has none): the `concat` network's function"""
    D = cfg["lstm_dim"] * (2 if cfg["use_bidirectional"] else 1)
    out = dict(sd)
    dt = next(v for v in sd.values() if v.is_floating_point()).dtype
    for p in stacks(cfg):
        out[p + ".words.value.weight"] = torch.zeros(256, D, dtype=dt)
        out.setdefault(p + ".words.key.weight", torch.zeros(256, D, dtype=dt))
    return out


def twin64(sd, bt, h0, c0, anc, **kw):
    """test_gpu_net.fp64_twin on words_ref.zsgnet_forward"""
    sd64 = {k: (v.detach().double().requires_grad_(v.requires_grad) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    bt64 = {k: v.double() for k, v in bt.items()}
    ref = WR.zsgnet_forward(sd64, bt64, h0.double(), c0.double(), rank=O.sort_rank(bt["qlens"]), **kw)
    ls = O.torch_loss(ref, bt["annot"], anc)
    ls["loss"].backward()
    return sd64, ref, ls


CASES = {"final": dict(lang_pool="final"), "mean": dict(lang_pool="mean"), "attn": dict(lang_pool="attn"),
         "two_heads": dict(lang_pool="mean", use_same_atb=False), "do_norm": dict(lang_pool="final", do_norm=True)}


def check_against_reference(cfg, net, sd, lf, bt, h0, c0, tag, sd_ref=None, gap_from_concat=True):
    """one training forward + loss + backward of `net` against words_ref on the weights sd_ref (default: sd); returns (sd32, sd64)"""
    inp = dev_inp(bt, h0, c0)
    out = net(inp)
    kw = ref_kw(cfg)
    sd32 = TN.leaves(sd if sd_ref is None else sd_ref)
    ref = WR.zsgnet_forward(sd32, bt, h0, c0, **kw)
    assert out["feat_sizes"].tolist() == ref["feat_sizes"].tolist()
    anc, A = TN.anchors_of(ref)
    assert out["att_bbx_out"].shape == (B, A, 5)
    sd64, ref64, ls64 = twin64(sd32, bt, h0, c0, anc, **kw)
    o_gpu, o_cpu, o_64 = out["att_bbx_out"].detach().cpu().double(), out5(ref), out5(ref64)
    e_gpu, e_cpu = float((o_gpu - o_64).abs().max()), float((o_cpu - o_64).abs().max())
    tol = 6 * e_cpu + 1e-4
    print(f"forward {tag}: HIP err {e_gpu:.3g} vs fp64, CPU fp32 err {e_cpu:.3g}")
    if gap_from_concat:
        with torch.no_grad():
            c64 = WR.zsgnet_forward(with_zero_value({k: v.detach() for k, v in sd64.items()}, cfg), {k: v.double() for k, v in bt.items()},
                                    h0.double(), c0.double(), rank=O.sort_rank(bt["qlens"]), **kw)
        gap = float((out5(c64) - o_64).abs().max())
        print(f"forward {tag}: |words - concat| {gap:.3g} in float64, allowed error {tol:.3g}")
        assert gap > 100 * tol, f"{tag}: the float64 outputs of words and concat differ by {gap:.3g} only (allowed error {tol:.3g})"
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
    cfg, net, sd, lf = build(Z, 12, lang_fuse="words", **CASES[tag])
    net.train()
    bt, h0, c0 = TN.batch(cfg)
    sd32, sd64 = check_against_reference(cfg, net, sd, lf, bt, h0, c0, tag)
    for k in word_keys(cfg):
        assert float(sd64[k].grad.abs().max()) > 0
    worst = TN.grad_errors(net, sd32, sd64)
    assert not worst, f"gradient error vs fp64 (HIP rel, CPU-fp32 rel): {worst[:8]}"
    plan = train_plan(net)
    fw, bw = whats(plan.fwd), whats(plan.bwd)
    assert "lmap" not in fw
    for p in stacks(cfg):
        assert p + ".0.0.words" in fw and p + ".0.0.feat" in fw and p + "0.gamma" not in fw
        assert p + ".0.0.words_bwd" in bw and f"wgrad:{p}.words.key" in bw and f"wgrad:{p}.words.value" in bw
        assert f"dhseq.key:{p}" in bw and f"dhseq.value:{p}" in bw
        # the heads' d(o) lands behind the pool's backward and ahead of the two sweeps
        if cfg["lang_pool"] != "final":
            assert bw.index("lang_pool_bwd") < bw.index(f"dhseq.key:{p}")
        else:
            assert "lang_pool_bwd" not in bw
        assert bw.index(f"dhseq.value:{p}") < min(bw.index("lstm_seq_bwd"), bw.index("lstm_seq_bwd_reverse"))
        for kv in ("key", "value"):
            assert f"{p}.words.{kv}.weight" in plan.grad_ready, "the DDP bucket plan must know when the new gradients are complete"
        # Kw / Vw sit on the side stream beside V, hoisted with the language maps in front of the pyramid
        for nm in ("0.Kw", "0.Vw"):
            i = fw.index(p + nm)
            assert plan.fwd.lanes[i] == 1 and plan.fwd.lanes[fw.index(p + "0.V")] == 1 and 0 < i - fw.index(p + "0.V") <= 2
            assert i < max(j for j, w in enumerate(fw) if w.startswith("backbone.")), "not hoisted: it sits behind the whole trunk"
    assert "zsg_head_words_conv0" in names(plan.fwd) and "zsg_head_words_conv0_bwd" in names(plan.bwd)


def test_zero_value_weight_is_concat(Z):
    """value.weight = 0 (its initial value): the words net computes the concat net's function; each plan is held to
    tests/test_gpu_film_net.py's bounds against the SAME float64 reference (test_zero_weight_is_concat there)"""
    cfg_w, net_w, sd_w, lf = build(Z, 12, zero_value=True, lang_fuse="words", lang_pool="mean")
    cfg_c, net_c, sd_c, _ = build(Z, 12, lang_pool="mean")
    assert all(torch.equal(sd_w[k], sd_c[k]) for k in sd_c)
    bt, h0, c0 = TN.batch(cfg_w)
    net_w.train(), net_c.train()
    sd32, sd64 = check_against_reference(cfg_w, net_w, sd_w, lf, bt, h0, c0, "words(0)", gap_from_concat=False)
    worst = TN.grad_errors(net_w, sd32, sd64)
    assert not worst, f"words(0) gradient error vs fp64: {worst[:8]}"
    named = dict(net_w.named_parameters())
    assert float(named["att_reg_box.words.value.weight"].grad.abs().max()) > 0, "a zero value weight still gets a gradient"
    assert float(named["att_reg_box.words.key.weight"].grad.abs().max()) == 0.0, "with value = 0 the key's gradient is exactly 0"
    sd32c, sd64c = check_against_reference(cfg_c, net_c, sd_c, lf, bt, h0, c0, "concat", sd_ref=sd_w, gap_from_concat=False)
    worst = TN.grad_errors(net_c, sd32c, sd64c)
    assert not worst, f"concat gradient error vs the words(0) twin: {worst[:8]}"
    with torch.no_grad():
        d = float((net_w(dev_inp(bt, h0, c0))["att_bbx_out"] - net_c(dev_inp(bt, h0, c0))["att_bbx_out"]).abs().max())
    print(f"words(0) vs concat: max|diff| of the outputs {d:.3e}")


def plan_calls(net):
    return {k: (names(p.fwd), names(p.bwd)) for k, p in net._plans.items()}


@pytest.mark.parametrize("fuse", ["concat", "film"])
def test_concat_and_film_build_no_words_launch(Z, fixed_tiles, fuse):
    """the other modes keep their programs: no words / Kw / Vw launch in a training, an eval and a shared-image eval plan (call names
    compared as tests/test_gpu_film_net.py's test_concat_builds_no_film_launch does), and the parent's launch lists — pinned here by
    their fusion-point launches, which is all the lowering of this mode could have touched"""
    from zsgnet_pytorch_amd import synth
    if fuse == "film":
        cfg, net, sd, lf = TF.build(Z, 12, lang_fuse="film", lang_pool="mean")
    else:
        cfg, net, sd, lf = build(Z, 12, lang_pool="mean")
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
            assert not [n for n in names(prog) if "words" in n], names(prog)
            assert not [w for w in whats(prog) if "words" in w or ".Kw" in w or ".Vw" in w or "dhseq" in w or "transpose:" in w]
    tp = train_plan(net)
    fw, bw = whats(tp.fwd), whats(tp.bwd)
    assert "lang_pool" in fw and "lang_pool_bwd" in bw and bw.index("lang_pool_bwd") < bw.index("lstm_seq_bwd")
    if fuse == "concat":
        assert "lmap" in fw and "att_reg_box.0.0" in fw and "att_reg_box.0.0.feat" not in fw
        assert "zsg_head_shared_conv0" in [n for p in net._plans.values() for n in names(p.fwd)]
        assert [w for w in bw if w.startswith("dwe")] == ["dwe:att_reg_box"]
    else:
        assert "att_reg_box0.gamma" in fw and "att_reg_box.0.0.film" in fw and "lmap" not in fw
        assert [w for w in bw if w.startswith(("dwe", "dgamma"))] == ["dwe:att_reg_box", "dgamma:att_reg_box", "dwe.film:att_reg_box"]
        assert all("zsg_head_film_conv0" in names(p.fwd) for p in net._plans.values())


def tta_build(Z, **flags):
    """tests/test_gpu_tta_net.py's network (ResNet-18, seeded_state_dict seed 1) with drawn key / value weights"""
    config, evaluator, loss, mdl, optim = Z
    cfg = config.get_cfg(resnet_arch=ARCH, **flags)
    net = mdl.get_default_net(9, cfg)
    net.load_state_dict(seeded(cfg, 1, net.start_dim_head))
    return cfg, net.to("cuda").eval()


def test_shared_image_eval(Z, fixed_tiles):
    """Q = 6 queries over 3 images against the plain words forward of the expanded batch, by tests/test_gpu_film_net.py's rule"""
    from zsgnet_pytorch_amd import synth
    cfg, net = tta_build(Z, lang_fuse="words", lang_pool="mean")
    bt = synth.synthetic_shared_batch(3, 6, 128, 128, seed=5)
    g = torch.Generator().manual_seed(1)
    h0, c0 = torch.randn(2, 6, 128, generator=g), torch.randn(2, 6, 128, generator=g)
    s, _ = fwd5(net, bt, h0, c0)
    p, _ = fwd5(net, synth.expand_shared(bt), h0, c0)
    shared = [pl for k, pl in net._plans.items() if "shared" in k]
    plain = [pl for k, pl in net._plans.items() if "shared" not in k]
    assert len(shared) == 1 and len(plain) == 1 and tuple(s.shape) == tuple(p.shape) and s.shape[0] == 6
    assert "zsg_head_words_conv0" in names(shared[0].fwd) and "zsg_head_words_conv0" in names(plain[0].fwd)
    assert "zsg_head_shared_conv0" not in names(shared[0].fwd)
    i = names(plain[0].fwd).index("zsg_head_words_conv0")
    a = plain[0].fwd.calls[i][1][-1]
    assert not getattr(a, "value", a), "an eval plan keeps no alpha"
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        ref = WR.zsgnet_forward(sd, synth.expand_shared(bt), h0, c0, **ref_kw(cfg, training=False))
    want = torch.cat([ref["bbx_out"], ref["att_out"]], 2)
    scale = float(want.abs().max())
    d_s, d_p = float((s.cpu() - want).abs().max()), float((p.cpu() - want).abs().max())
    print(f"shared words eval: max|shared - ref| {d_s:.3e}, max|plain - ref| {d_p:.3e}, max|shared - plain| {float((s - p).abs().max()):.3e}, scale {scale:.3e}")
    assert d_s < 2e-4 * scale and d_s <= max(4 * d_p, 2e-3)
    with torch.no_grad():
        net.state_dict()["att_reg_box.words.value.weight"].zero_()
    z, _ = fwd5(net, bt, h0, c0)
    assert float((z - s).abs().max()) > 1e-2 * scale


def test_shared_image_training(Z):
    """6 queries over 3 images, BatchNorm frozen: the shared words step and the plain words step, each against the float64 twin of
    words_ref on the expanded batch with tests/test_gpu_shared_train.py's bounds; the shared step folds dYq with zsg_head_shared_conv0_bwd"""
    from zsgnet_pytorch_amd import synth
    bt = synth.synthetic_shared_batch(3, 6, 96, 96, seed=21, tmax=13)
    bt["img_idx"] = torch.tensor([1, 0, 2, 0, 2, 1])
    bt["qlens"][-1] = bt["qlens"][0]
    g = torch.Generator().manual_seed(22)
    h0, c0 = torch.randn(2, 6, 128, generator=g), torch.randn(2, 6, 128, generator=g)
    ex = synth.expand_shared(bt)
    cfg, net, sd, lf = build(Z, 11, lang_fuse="words", lang_pool="attn")
    kw = ref_kw(cfg, training=False)
    sd32 = TN.leaves(sd)
    ref = WR.zsgnet_forward(sd32, ex, h0, c0, **kw)
    anc, A = TN.anchors_of(ref)
    O.torch_loss(ref, ex["annot"], anc)["loss"].backward()
    sd64, ref64, ls64 = twin64(sd32, ex, h0, c0, anc, **kw)
    o_64 = out5(ref64)
    e_cpu = float((out5(ref) - o_64).abs().max())
    outs = {}
    for form in ("shared", "plain"):
        cfg, net, sd, lf = build(Z, 11, lang_fuse="words", lang_pool="attn")
        net.train()
        net.freeze_batchnorm()
        net.shared_training(form == "shared")
        inp = dev_inp(bt if form == "shared" else ex, h0, c0)
        out = net(inp)
        o = out["att_bbx_out"].detach().cpu().double()
        outs[form] = o
        e = float((o - o_64).abs().max())
        ls = lf(out, inp)
        print(f"words {form} training step: max|out - fp64| {e:.3e} (CPU fp32 {e_cpu:.3e}), loss {ls['loss'].item():.6f} vs {ls64['loss'].item():.6f}")
        assert e <= 6 * e_cpu + 1e-4
        np.testing.assert_allclose(ls["loss"].item(), ls64["loss"].item(), rtol=2e-4)
        ls["loss"].backward()
        torch.cuda.synchronize()
        worst = TN.grad_errors(net, sd32, sd64)
        assert not worst, f"{form}: gradient error vs fp64 (HIP rel, CPU-fp32 rel): {worst[:8]}"
        bw = names(train_plan(net).bwd)
        assert "zsg_head_words_conv0_bwd" in bw and ("zsg_head_shared_conv0_bwd" in bw) == (form == "shared")
    print(f"words shared vs plain training forward: max|diff| {float((outs['shared'] - outs['plain']).abs().max()):.3e}")


def test_flip_tta(Z, fixed_tiles):
    """eval_tta = flip: merge_ref of ONE plain eval forward of the 2B rows tta_batch builds, bit for bit (tests/test_gpu_tta_net.py)"""
    cfg, net = tta_build(Z, lang_fuse="words", lang_pool="final", eval_tta="flip")
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
        want = WR.zsgnet_forward(sd, bt2, h2, c2, **ref_kw(cfg, training=False))
    np.testing.assert_allclose(x2.cpu().numpy(), torch.cat([want["bbx_out"], want["att_out"]], 2).numpy(), rtol=2e-3, atol=5e-3)


@pytest.mark.parametrize("dtype,bb,ba", [("bf16", TF.BF16_BOX, TF.BF16_ATT), ("bf16_act", TF.ACT_BOX, TF.ACT_ATT)])
def test_reduced_precision_eval(Z, fixed_tiles, dtype, bb, ba):
    """eval_dtype = bf16 / bf16_act against the fp32 words plan, within the bounds of those switches' own net tests"""
    cfg, net = tta_build(Z, lang_fuse="words", lang_pool="mean")
    bt = O.synthetic_batch(2, 128, 128, seed=3)
    g = torch.Generator().manual_seed(0)
    h0, c0 = torch.randn(2, 2, 128, generator=g), torch.randn(2, 2, 128, generator=g)
    o32, _ = fwd5(net, bt, h0, c0)
    net.eval_precision(dtype)
    o16, _ = fwd5(net, bt, h0, c0)
    plan = [p for k, p in net._plans.items() if dtype in k][0]
    i = names(plan.fwd).index("zsg_head_words_conv0")
    flag = plan.fwd.calls[i][1][-2]
    assert int(getattr(flag, "value", flag)) == int(dtype == "bf16_act"), "h1 is stored as bf16 exactly under bf16_act"
    assert ("zsg_conv_igemm_bf16_io" if dtype == "bf16_act" else "zsg_conv_igemm_bf16") in names(plan.fwd)
    rb, ra = rel(o16, o32)
    print(f"words {dtype} eval parity: box {rb:.3e} att {ra:.3e} of max|fp32|")
    assert not torch.equal(o16, o32) and rb <= bb and ra <= ba


def test_bf16_head_training(Z, fixed_tiles):
    """train_dtype = bf16_head against the fp32 words plan, within the bounds of tests/test_gpu_net_train_bf16_head.py"""
    res = {}
    bt = O.synthetic_batch(2, 128, 128, seed=3)
    g = torch.Generator().manual_seed(0)
    h0, c0 = torch.randn(2, 2, 128, generator=g), torch.randn(2, 2, 128, generator=g)
    for dt in ("fp32", "bf16_head"):
        config, evaluator, loss, mdl, optim = Z
        cfg, net = tta_build(Z, lang_fuse="words", lang_pool="mean")
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
    print(f"words bf16_head parity: box {box:.3e} att {att:.3e} loss {rel_loss:.3e} flat l2 {l2:.3e} 1-cos {1 - cos:.3e}")
    assert not torch.equal(g16, g32)
    assert box <= TF.HEAD_BOX and att <= TF.HEAD_ATT and rel_loss <= TF.HEAD_LOSS and l2 <= TF.HEAD_L2 and cos >= TF.HEAD_COS


@pytest.mark.parametrize("only_words", [True, False], ids=["only_words_train", "words_frozen"])
def test_frozen_parameters(Z, only_words):
    """as tests/test_gpu_finetune.py: a frozen tensor keeps p.grad None and its bits across an optimizer step; frozen key / value weights
    still pass the gradient on to o, `we` and Y, a frozen rest still trains them"""
    config, evaluator, loss, mdl, optim = Z
    cfg, net, sd, lf = build(Z, 12, lang_fuse="words", lang_pool="mean")
    net.train()
    new = set(word_keys(cfg))
    for n, p in net.named_parameters():
        p.requires_grad_((n in new) == only_words)
    opt = optim.FusedAdam(net, lr=1e-3, betas=(0.9, 0.99))
    before = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    bt, h0, c0 = TN.batch(cfg)
    inp = dev_inp(bt, h0, c0)
    opt.zero_grad()
    lf(net(inp), inp)["loss"].backward()
    torch.cuda.synchronize()
    kw = ref_kw(cfg)
    sd32 = TN.leaves(sd)
    ref = WR.zsgnet_forward(sd32, bt, h0, c0, **kw)
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
    if only_words:
        assert "att_reg_box.0.0.words_bwd" in bw and "wgrad:att_reg_box.words.key" in bw and "wgrad:att_reg_box.words.value" in bw
        assert not [w for w in bw if w.startswith(("dwe", "dhseq", "transpose:", "dgrad:att_reg_box.0.0", "wgrad:att_reg_box.0.0")) or "backbone" in w
                    or "lstm" in w or "lang_pool" in w], bw
    else:
        assert "att_reg_box.0.0.words_bwd" in bw and "dhseq.key:att_reg_box" in bw and "dhseq.value:att_reg_box" in bw
        assert not [w for w in bw if w.startswith("wgrad:att_reg_box.words")]
    opt.step()
    torch.cuda.synchronize()
    after = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    for n, p in net.named_parameters():
        same = torch.equal(bits(after[n]), bits(before[n]))
        assert same == (not p.requires_grad), f"{n}: {'moved' if not same else 'did not move'}"


@pytest.mark.parametrize("opt_fn", ["Adam", "LAMB"])
def test_optimizer_steps_move_both_weights(Z, opt_fn):
    """from the zero (value) / drawn (key) start: key's gradient is exactly 0 at the first step while value = 0, nonzero at the second"""
    config, evaluator, loss, mdl, optim = Z
    cfg, net, sd, lf = build(Z, 12, zero_value=True, lang_fuse="words", lang_pool="mean", opt_fn=opt_fn)
    net.train()
    opt = optim.make_opt_fn(cfg)(net, lr=1e-3)
    bt, h0, c0 = TN.batch(cfg)
    inp = dev_inp(bt, h0, c0)
    named = dict(net.named_parameters())
    k0 = net.state_dict()["att_reg_box.words.key.weight"].detach().cpu().clone()
    gk = []
    for _ in range(3):          # (LAMB's trust ratio of a zero tensor: tests/test_gpu_film_net.py; key moves from the second gradient on)
        opt.zero_grad()
        lf(net(inp), inp)["loss"].backward()
        torch.cuda.synchronize()
        gk.append(float(named["att_reg_box.words.key.weight"].grad.abs().max()))
        opt.step()
    torch.cuda.synchronize()
    assert gk[0] == 0.0 and gk[1] > 0.0, gk
    wv, wk = net.state_dict()["att_reg_box.words.value.weight"], net.state_dict()["att_reg_box.words.key.weight"]
    assert bool(torch.isfinite(wv).all()) and float(wv.abs().max()) > 0, "value.weight did not move from its zero start"
    assert bool(torch.isfinite(wk).all()) and not torch.equal(wk.cpu(), k0), "key.weight did not move from its drawn start"


def test_checkpoint_round_trip_through_learner(Z, fixed_tiles, tmp_path):
    from zsgnet_pytorch_amd.trainer import Learner
    config, evaluator, loss, mdl, optim = Z

    def learner(uid, **flags):
        cfg = config.get_cfg(resnet_arch=ARCH, tmp_path=str(tmp_path), lang_pool="mean", **flags)
        net = mdl.get_default_net(9, cfg)
        r, s = config.ratios_scales(cfg)
        return cfg, net, Learner(uid, None, net, loss.get_default_loss(r, s, cfg), cfg, evaluator.get_default_eval(r, s, cfg), None)
    kk, kv = "att_reg_box.words.key.weight", "att_reg_box.words.value.weight"
    cfg, net, la = learner("words_a", lang_fuse="words")
    net.load_state_dict(seeded(cfg, 1, net.start_dim_head))
    net.to("cuda").eval()
    la.save_model_dict()
    ck = torch.load(la.model_file)["model_state_dict"]
    assert float(ck[kk].abs().max()) > 0 and float(ck[kv].abs().max()) > 0
    cfg_b, other, lb = learner("words_b", lang_fuse="words")
    assert lb.load_model_dict(str(la.model_file))
    other.to("cuda").eval()
    assert torch.equal(bits(other.state_dict()[kk]), bits(ck[kk])) and torch.equal(bits(other.state_dict()[kv]), bits(ck[kv]))
    bt = O.synthetic_batch(2, 128, 128, seed=3)
    g = torch.Generator().manual_seed(0)
    h0, c0 = torch.randn(2, 2, 128, generator=g), torch.randn(2, 2, 128, generator=g)
    o_a = fwd5(net, bt, h0, c0)[0]
    assert torch.equal(bits(o_a), bits(fwd5(other, bt, h0, c0)[0]))
    # a concat checkpoint into a words net: refused by default, taken with strict_load = False and then the concat net's function
    cfg_c, plain, lc = learner("concat_c")
    plain.load_state_dict({k: v for k, v in ck.items() if "words" not in k})
    plain.to("cuda").eval()
    lc.save_model_dict()
    _, strict, ls_ = learner("words_strict", lang_fuse="words")
    with pytest.raises(RuntimeError, match="words"):
        ls_.load_model_dict(str(lc.model_file))
    _, loose, ll = learner("words_loose", lang_fuse="words", strict_load=False)
    assert ll.load_model_dict(str(lc.model_file))
    loose.to("cuda").eval()
    assert not loose.state_dict()[kv].any()
    o_c, o_l = fwd5(plain, bt, h0, c0)[0], fwd5(loose, bt, h0, c0)[0]
    scale = float(o_c.abs().max())
    print(f"concat checkpoint in a words net: max|diff| {float((o_l - o_c).abs().max()):.3e} at scale {scale:.3e}; words vs concat weights {float((o_a - o_c).abs().max()):.3e}")
    assert float((o_l - o_c).abs().max()) <= 1e-4 * max(1.0, scale)
    assert float((o_a - o_c).abs().max()) > 1e-2 * scale


def test_concat_and_film_launch_lists_are_the_parents(Z, fixed_tiles):
    """tests/golden/words_parent_launches.json: the launch lists (entry point, name in the plan, lane) of a training, an eval and a
    shared-image eval plan of lang_fuse = concat / film at lang_pool = mean, recorded from the commit BEFORE this mode existed.  This
    tree must build them launch for launch.  The convolution entry points are recorded as one name: which of them a convolution takes
    (direct, Winograd, a tile hint) is the tuner's choice on the day, not the lowering's.
    A later change that legitimately adds or moves a launch of a default plan regenerates the file from ITS parent commit: run the body
    of this test there (ZSG_AUTOTUNE=0, ZSG_DETERMINISTIC=1), dump `got` of every plan and program as
    {"concat": [{"fwd": [...], "bwd": [...]} x 3 plans], "film": [...]} with json.dump, and say so in the commit."""
    import json
    import os
    from zsgnet_pytorch_amd import synth
    config, evaluator, loss, mdl, optim = Z
    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "words_parent_launches.json")))
    for fuse in ("concat", "film"):
        cfg = config.get_cfg(resnet_arch=ARCH, lang_fuse=fuse, lang_pool="mean")
        net = mdl.get_default_net(9, cfg)
        net.reset_parameters(seed=3)
        net.to("cuda").train()
        r, s = config.ratios_scales(cfg)
        lf = loss.get_default_loss(r, s, cfg)
        bt = O.synthetic_batch(3, 96, 128, seed=5, tmax=13)
        g = torch.Generator().manual_seed(2)
        inp = dev_inp(bt, torch.randn(2, 3, 128, generator=g), torch.randn(2, 3, 128, generator=g))
        lf(net(inp), inp)["loss"].backward()
        net.eval()
        with torch.no_grad():
            net(inp)
            sb = synth.synthetic_shared_batch(2, 4, 128, 128, seed=5)
            net(dev_inp(sb, torch.randn(2, 4, 128, generator=g), torch.randn(2, 4, 128, generator=g)))
        torch.cuda.synchronize()
        plans = list(net._plans.values())
        assert len(plans) == len(want[fuse]) == 3
        for p, w in zip(plans, want[fuse]):
            for tag, prog in (("fwd", p.fwd), ("bwd", p.bwd)):
                got = [[("conv" if c[0].__name__.startswith("zsg_conv") else c[0].__name__), c[2], int(l)] for c, l in zip(prog.calls, prog.lanes)]
                assert got == w[tag], (fuse, tag, [x for x in zip(got, w[tag]) if x[0] != x[1]][:4])


def test_more_than_64_token_positions_are_refused_by_name(Z):
    """the kernel's 1 <= T <= 64 contract surfaces where the plan learns T, as a ValueError naming lang_fuse — not as the C ABI's -1 at replay;
    64 positions run"""
    cfg, net = tta_build(Z, lang_fuse="words", lang_pool="mean")
    g = torch.Generator().manual_seed(0)
    h0, c0 = torch.randn(2, 2, 128, generator=g), torch.randn(2, 2, 128, generator=g)
    for T in (65, 64):
        bt = O.synthetic_batch(2, 128, 128, seed=3)
        E = bt["qvec"].shape[2]
        bt["qvec"] = torch.cat([bt["qvec"], torch.zeros(2, T - bt["qvec"].shape[1], E)], dim=1)
        if T > 64:
            with pytest.raises(ValueError, match="lang_fuse"):
                net(dev_inp(bt, h0, c0))
        else:
            o, _ = fwd5(net, bt, h0, c0)
            assert bool(torch.isfinite(o).all())
