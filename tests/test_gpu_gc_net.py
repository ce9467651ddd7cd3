"""cfg head_ctx = "gc" on the network, against tests/gc_ref.py.

Geometry, seeds and bounds of tests/test_gpu_film_net.py (ResNet-18, B = 3, 96 x 128 — a pyramid of 12 x 16 down to 1 x 1, where the
block's softmax runs over one row — queries of up to 13 tokens, seeded_state_dict seed 12): the float64 twin of gc_ref.zsgnet_forward is
the truth, the same code in float32 on the CPU the yardstick — forward max error within 6 x CPU-fp32 + 1e-4, every parameter gradient
(the seven gc tensors included) within grad_tol, losses rel 2e-4.  The gc tensors are not in the oracle's seeded weights: they are drawn
here (seeded; fc2 non-zero, so that the block is engaged).

The shared-image, flip-TTA, reduced-precision and checkpoint tests use the set-ups of the tests they name (ResNet-18, 128 px,
ZSG_AUTOTUNE=0 and ZSG_DETERMINISTIC=1: two forwards of one plan give the same bits), with those tests' own bounds."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gc_ref as GR  # noqa: E402
import test_gpu_film_net as FN  # noqa: E402
import test_gpu_net_lstm as TN  # noqa: E402
import tta_ref  # noqa: E402
from oracle import zsg_oracle as O  # noqa: E402
from test_gpu_net import Z, grad_tol, to_dev  # noqa: E402,F401

ARCH, B = TN.ARCH, TN.B
fixed_tiles = FN.fixed_tiles
_leave_the_tuner_as_found = FN._leave_the_tuner_as_found
bits, whats, names, train_plan, dev_inp, fwd5, rel, out5 = FN.bits, FN.whats, FN.names, FN.train_plan, FN.dev_inp, FN.fwd5, FN.rel, FN.out5
GC_SHAPES = {"key.weight": (1, 256), "fc1.weight": (64, 256), "fc1.bias": (64,), "ln.weight": (64,), "ln.bias": (64,), "fc2.weight": (256, 64),
             "fc2.bias": (256,)}
assert tuple(GC_SHAPES) == GR.NAMES


def stacks(cfg):
    return ["att_reg_box"] if cfg["use_same_atb"] else ["att_box", "reg_box"]


def gc_keys(cfg):
    return [f"{p}.gc.{n}" for p in stacks(cfg) for n in GR.NAMES]


def seeded(cfg, seed, head_in, zero=False):
    """the oracle's seeded weights of the cfg's heads (+ film_net's drawn film weights), plus drawn gc tensors (zero: fc2 = 0)"""
    sd = FN.seeded(cfg, seed, head_in)
    g = torch.Generator().manual_seed(seed + 300)
    for p in stacks(cfg):
        for n, shp in GC_SHAPES.items():
            v = torch.randn(*shp, generator=g) * 0.1
            if n == "ln.weight":
                v = v + 1.0
            if n.startswith("fc2") and zero:
                v = torch.zeros(*shp)
            sd[f"{p}.gc.{n}"] = v
    return sd


def build(Z, seed, zero=False, **flags):
    config, evaluator, loss, mdl, optim = Z
    cfg = config.get_cfg(resnet_arch=ARCH, **flags)
    net = mdl.get_default_net(9, cfg)
    sd = seeded(cfg, seed, net.start_dim_head, zero) if cfg["head_ctx"] == "gc" else FN.seeded(cfg, seed, net.start_dim_head)
    assert set(net.state_dict().keys()) == set(sd.keys())
    net.load_state_dict(sd)
    net.to("cuda")
    r, s = config.ratios_scales(cfg)
    return cfg, net, sd, loss.get_default_loss(r, s, cfg)


def ref_kw(cfg, training=True):
    return dict(arch=ARCH, training=training, do_norm=bool(cfg["do_norm"]), bidirectional=cfg["use_bidirectional"], lang_pool=cfg["lang_pool"],
                lang_fuse=cfg["lang_fuse"], use_lang=bool(cfg["use_lang"]), use_img=bool(cfg["use_img"]))


def with_zero_fc2(sd, cfg):
    out = dict(sd)
    for p in stacks(cfg):
        for n in ("fc2.weight", "fc2.bias"):
            out[f"{p}.gc.{n}"] = torch.zeros_like(sd[f"{p}.gc.{n}"])
    return out


def twin64(sd, bt, h0, c0, anc, **kw):
    """test_gpu_net.fp64_twin on gc_ref.zsgnet_forward"""
    sd64 = {k: (v.detach().double().requires_grad_(v.requires_grad) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    bt64 = {k: v.double() for k, v in bt.items()}
    ref = GR.zsgnet_forward(sd64, bt64, h0.double(), c0.double(), rank=O.sort_rank(bt["qlens"]), **kw)
    ls = O.torch_loss(ref, bt["annot"], anc)
    ls["loss"].backward()
    return sd64, ref, ls


def check_against_reference(cfg, net, sd, lf, bt, h0, c0, tag, gap_from_none=True):
    """one training forward + loss + backward of `net` against gc_ref on the weights sd; returns (sd32, sd64)"""
    inp = dev_inp(bt, h0, c0)
    out = net(inp)
    kw = ref_kw(cfg)
    sd32 = TN.leaves(sd)
    ref = GR.zsgnet_forward(sd32, bt, h0, c0, **kw)
    assert out["feat_sizes"].tolist() == ref["feat_sizes"].tolist()
    anc, A = TN.anchors_of(ref)
    assert out["att_bbx_out"].shape == (B, A, 5)
    sd64, ref64, ls64 = twin64(sd32, bt, h0, c0, anc, **kw)
    o_gpu, o_cpu, o_64 = out["att_bbx_out"].detach().cpu().double(), out5(ref), out5(ref64)
    e_gpu, e_cpu = float((o_gpu - o_64).abs().max()), float((o_cpu - o_64).abs().max())
    tol = 6 * e_cpu + 1e-4
    print(f"forward {tag}: HIP err {e_gpu:.3g} vs fp64, CPU fp32 err {e_cpu:.3g}")
    if gap_from_none:
        # the block matters on this batch: the float64 output of the same weights with fc2 = 0 (the `none` function) is far outside the bound
        with torch.no_grad():
            n64 = GR.zsgnet_forward(with_zero_fc2({k: v.detach() for k, v in sd64.items()}, cfg), {k: v.double() for k, v in bt.items()},
                                    h0.double(), c0.double(), rank=O.sort_rank(bt["qlens"]), **kw)
        gap = float((out5(n64) - o_64).abs().max())
        print(f"forward {tag}: |gc - none| {gap:.3g} in float64, allowed error {tol:.3g}")
        assert gap > 100 * tol, f"{tag}: the float64 outputs of gc and none differ by {gap:.3g} only (allowed error {tol:.3g})"
    assert e_gpu <= tol, f"forward: HIP err {e_gpu:.3g} vs fp64, CPU fp32 err {e_cpu:.3g}"
    ls = lf(out, inp)
    for k in ("loss", "cls_ls", "box_ls"):
        np.testing.assert_allclose(ls[k].item(), ls64[k].item(), rtol=2e-4, err_msg=k)
    O.torch_loss(ref, bt["annot"], anc)["loss"].backward()
    ls["loss"].backward()
    torch.cuda.synchronize()
    return sd32, sd64


CASES = {"same_atb": dict(), "two_heads": dict(use_same_atb=False), "do_norm": dict(do_norm=True), "film": dict(lang_fuse="film"),
         "lang_blind": dict(use_lang=False), "img_blind": dict(use_img=False)}


@pytest.mark.parametrize("tag", list(CASES))
def test_forward_backward_vs_reference(Z, tag):
    cfg, net, sd, lf = build(Z, 12, head_ctx="gc", **CASES[tag])
    net.train()
    bt, h0, c0 = TN.batch(cfg)
    sd32, sd64 = check_against_reference(cfg, net, sd, lf, bt, h0, c0, tag)
    for k in gc_keys(cfg):
        assert float(sd64[k].grad.abs().max()) > 0, k
    worst = TN.grad_errors(net, sd32, sd64)
    assert not worst, f"gradient error vs fp64 (HIP rel, CPU-fp32 rel): {worst[:8]}"
    plan = train_plan(net)
    fw, bw = whats(plan.fwd), whats(plan.bwd)
    assert out_sizes_end_in_one_row(net)
    for p in stacks(cfg):
        assert fw.count(p + ".gc") == 1 and bw.count(p + ".gc_bwd") == 1
        assert fw.index(p + ".gc") < min(i for i, w in enumerate(fw) if w.startswith(p + ".1.0")), "the block sits in front of conv1"
        assert "mask+acc:" + p + ".h1" in bw, "h1's ReLU mask is applied by its own handling"
        for n in GR.NAMES:
            assert f"{p}.gc.{n}" in plan.grad_ready, "the DDP bucket plan must know when the new gradients are complete"


def out_sizes_end_in_one_row(net):
    return [tuple(s) for s in train_plan(net).feat_sizes][-1] == (1, 1)


def test_zero_fc2_is_the_none_net(Z, fixed_tiles):
    """fc2 = 0 (its initial value): y = x and dx = g exactly (tests/test_gpu_gc_kernels.py), and both nets run the same launches with the
    same tile shapes around the block, so the outputs and every shared parameter's gradient carry the none net's bits"""
    cfg_g, net_g, sd_g, lf = build(Z, 12, zero=True, head_ctx="gc")
    cfg_n, net_n, sd_n, _ = build(Z, 12)
    assert all(torch.equal(sd_g[k], sd_n[k]) for k in sd_n)
    bt, h0, c0 = TN.batch(cfg_g)
    res = {}
    for tag, net in (("gc", net_g), ("none", net_n)):
        net.train()
        inp = dev_inp(bt, h0, c0)
        net.store.grad.zero_()
        out = net(inp)
        ls = lf(out, inp)["loss"]
        ls.backward()
        torch.cuda.synchronize()
        res[tag] = (out["att_bbx_out"].detach().cpu().clone(), float(ls), {n: p.grad.detach().cpu().clone() for n, p in net.named_parameters()})
    assert torch.equal(bits(res["gc"][0]), bits(res["none"][0])), float((res["gc"][0] - res["none"][0]).abs().max())
    assert res["gc"][1] == res["none"][1]
    for n, g in res["none"][2].items():
        assert torch.equal(bits(res["gc"][2][n]), bits(g)), (n, float((res["gc"][2][n] - g).abs().max()))
    gg = res["gc"][2]
    assert float(gg["att_reg_box.gc.fc2.weight"].abs().max()) > 0 and float(gg["att_reg_box.gc.fc2.bias"].abs().max()) > 0, "a zero layer still gets a gradient"
    for n in ("key.weight", "fc1.weight", "fc1.bias", "ln.weight", "ln.bias"):
        assert not gg["att_reg_box.gc." + n].any(), n + ": nothing flows in front of a zero fc2.weight"


def test_words_plan_with_zero_fc2_is_the_words_none_net(Z, fixed_tiles):
    """lang_fuse = words (lang_pool = mean, drawn key / value weights): the block sits behind zsg_head_words_conv0's h1.  No reference
    is needed: with fc2 = 0 the training step carries the bits of the words net without the block (outputs, loss, every shared
    gradient); with a drawn fc2 the same plan runs, stays finite, moves the output and gives all seven tensors a gradient"""
    config, evaluator, loss, mdl, optim = Z
    nets = {}
    for ctx in ("none", "gc"):
        cfg = config.get_cfg(resnet_arch=ARCH, lang_fuse="words", lang_pool="mean", head_ctx=ctx)
        net = mdl.get_default_net(9, cfg)
        net.reset_parameters(seed=3)
        nets[ctx] = (cfg, net)
    g = torch.Generator().manual_seed(17)
    sd = {k: v.detach().clone() for k, v in nets["none"][1].state_dict().items()}
    for kv in ("key", "value"):
        sd[f"att_reg_box.words.{kv}.weight"] = torch.randn(sd[f"att_reg_box.words.{kv}.weight"].shape, generator=g) * 0.05
    gc = {f"att_reg_box.gc.{n}": torch.randn(*shp, generator=g) * 0.1 + (1.0 if n == "ln.weight" else 0.0) for n, shp in GC_SHAPES.items()}
    zero = dict(gc, **{"att_reg_box.gc.fc2.weight": torch.zeros(256, 64), "att_reg_box.gc.fc2.bias": torch.zeros(256)})
    cfg = nets["gc"][0]
    r, s = config.ratios_scales(cfg)
    lf = loss.get_default_loss(r, s, cfg)
    bt, h0, c0 = TN.batch(cfg)
    res = {}
    for tag, ctx, extra in (("none", "none", {}), ("zero", "gc", zero), ("drawn", "gc", gc)):
        net = nets[ctx][1]
        net.load_state_dict(dict(sd, **extra))
        net.to("cuda").train()
        inp = dev_inp(bt, h0, c0)
        net.store.grad.zero_()
        out = net(inp)
        ls = lf(out, inp)["loss"]
        ls.backward()
        torch.cuda.synchronize()
        res[tag] = (out["att_bbx_out"].detach().cpu().clone(), float(ls.detach()), {n: p.grad.detach().cpu().clone() for n, p in net.named_parameters()})
    fw, bw = whats(train_plan(nets["gc"][1]).fwd), whats(train_plan(nets["gc"][1]).bwd)
    assert fw.index("att_reg_box.0.0.words") < fw.index("att_reg_box.gc") < min(i for i, w in enumerate(fw) if w.startswith("att_reg_box.1.0"))
    assert bw.index("att_reg_box.gc_bwd") < bw.index("att_reg_box.0.0.words_bwd")
    assert torch.equal(bits(res["zero"][0]), bits(res["none"][0])) and res["zero"][1] == res["none"][1]
    for n, gn in res["none"][2].items():
        assert torch.equal(bits(res["zero"][2][n]), bits(gn)), (n, float((res["zero"][2][n] - gn).abs().max()))
    assert float(res["zero"][2]["att_reg_box.gc.fc2.weight"].abs().max()) > 0
    o, _, gd = res["drawn"]
    # engaged: the output moves by far more than two fp32 evaluations of one function differ (1e-4 * max(1, scale), the floor of
    # tests/test_gpu_film_net.py's checkpoint test).  The scale is no yardstick for more than that here: a freshly reset net's output is
    # its last bias (-4 on the att channel) plus values of order 1e-3.
    assert bool(torch.isfinite(o).all()) and float((o - res["none"][0]).abs().max()) > 10 * 1e-4 * max(1.0, float(res["none"][0].abs().max()))
    for n in GC_SHAPES:
        t = gd["att_reg_box.gc." + n]
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0, n
    assert all(bool(torch.isfinite(t).all()) for t in gd.values())


def test_none_builds_no_gc_launch(Z, fixed_tiles):
    """the default keeps its programs: no gc launch, no h1g buffer, conv1 reads h1"""
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
        assert not [a for a in p.acts if a.endswith(".h1g")]
        for prog in (p.fwd, p.bwd):
            assert not [n for n in names(prog) if "_gc_" in n], names(prog)
            assert not [w for w in whats(prog) if ".gc" in w]


def test_words_launch_lists_under_none_are_the_parents(Z, fixed_tiles):
    """tests/golden/head_ctx_parent_launches.json: the launch lists (entry point, name in the plan, lane) of a training, an eval and a
    shared-image eval plan of lang_fuse = words at lang_pool = mean, recorded from the commit BEFORE head_ctx existed by the body of this
    test (the way tests/golden/words_parent_launches.json was; tests/test_gpu_words_net.py pins concat and film).  head_ctx = none must
    build them launch for launch.  The convolution entry points are recorded as one name: which of them a convolution takes is the
    tuner's choice on the day, not the lowering's."""
    from zsgnet_pytorch_amd import synth
    config, evaluator, loss, mdl, optim = Z
    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_ctx_parent_launches.json")))
    for fuse in ("words",):
        cfg = config.get_cfg(resnet_arch=ARCH, lang_fuse=fuse, lang_pool="mean", head_ctx="none")
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


def tta_build(Z, zero=False, **flags):
    """tests/test_gpu_tta_net.py's network (ResNet-18, seeded_state_dict seed 1) with drawn gc tensors"""
    config, evaluator, loss, mdl, optim = Z
    cfg = config.get_cfg(resnet_arch=ARCH, **flags)
    net = mdl.get_default_net(9, cfg)
    net.load_state_dict(seeded(cfg, 1, net.start_dim_head, zero))
    return cfg, net.to("cuda").eval()


def test_shared_image_eval(Z, fixed_tiles):
    """Q = 6 queries over 3 images against the plain gc forward of the expanded batch, by the rule of tests/test_gpu_film_net.py: within
    2e-4 of the output's scale of the CPU definition, and no further from it than max(4 x the plain path's distance, 2e-3).  The block
    pools per QUERY: a shared plan runs it on the six rows of h1, not on the three image slots."""
    from zsgnet_pytorch_amd import synth
    cfg, net = tta_build(Z, head_ctx="gc")
    bt = synth.synthetic_shared_batch(3, 6, 128, 128, seed=5)
    g = torch.Generator().manual_seed(1)
    h0, c0 = torch.randn(2, 6, 128, generator=g), torch.randn(2, 6, 128, generator=g)
    s, _ = fwd5(net, bt, h0, c0)
    p, _ = fwd5(net, synth.expand_shared(bt), h0, c0)
    shared = [pl for k, pl in net._plans.items() if "shared" in k]
    plain = [pl for k, pl in net._plans.items() if "shared" not in k]
    assert len(shared) == 1 and len(plain) == 1 and tuple(s.shape) == tuple(p.shape) and s.shape[0] == 6
    for pl in (shared[0], plain[0]):
        assert names(pl.fwd).count("zsg_head_gc_fwd") == 1
        i = names(pl.fwd).index("zsg_head_gc_fwd")
        args = pl.fwd.calls[i][1]
        assert int(getattr(args[8], "value", args[8])) == 6, "Q of the block is the query count"
        assert all(getattr(a, "value", a) in (None, 0) for a in args[13:15]), "the eval forward saves nothing"
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        ref = GR.zsgnet_forward(sd, synth.expand_shared(bt), h0, c0, **ref_kw(cfg, training=False))
    want = torch.cat([ref["bbx_out"], ref["att_out"]], 2)
    scale = float(want.abs().max())
    d_s, d_p = float((s.cpu() - want).abs().max()), float((p.cpu() - want).abs().max())
    print(f"shared gc eval: max|shared - ref| {d_s:.3e}, max|plain - ref| {d_p:.3e}, max|shared - plain| {float((s - p).abs().max()):.3e}, scale {scale:.3e}")
    assert d_s < 2e-4 * scale and d_s <= max(4 * d_p, 2e-3)
    # and the block is engaged: the same weights with fc2 = 0 give another output
    with torch.no_grad():
        net.state_dict()["att_reg_box.gc.fc2.weight"].zero_()
        net.state_dict()["att_reg_box.gc.fc2.bias"].zero_()
    z, _ = fwd5(net, bt, h0, c0)
    assert float((z - s).abs().max()) > 1e-2 * scale


def test_shared_image_training(Z):
    """6 queries over 3 images, BatchNorm frozen (then the shared step IS the plain step on the expanded batch): the shared gc step and
    the plain gc step, each against the float64 twin of gc_ref on the expanded batch with tests/test_gpu_shared_train.py's bounds"""
    from zsgnet_pytorch_amd import synth
    bt = synth.synthetic_shared_batch(3, 6, 96, 96, seed=21, tmax=13)
    bt["img_idx"] = torch.tensor([1, 0, 2, 0, 2, 1])
    bt["qlens"][-1] = bt["qlens"][0]
    g = torch.Generator().manual_seed(22)
    h0, c0 = torch.randn(2, 6, 128, generator=g), torch.randn(2, 6, 128, generator=g)
    ex = synth.expand_shared(bt)
    cfg, net, sd, lf = build(Z, 11, head_ctx="gc")
    kw = ref_kw(cfg, training=False)
    sd32 = TN.leaves(sd)
    ref = GR.zsgnet_forward(sd32, ex, h0, c0, **kw)
    anc, A = TN.anchors_of(ref)
    O.torch_loss(ref, ex["annot"], anc)["loss"].backward()
    sd64, ref64, ls64 = twin64(sd32, ex, h0, c0, anc, **kw)
    o_64 = out5(ref64)
    e_cpu = float((out5(ref) - o_64).abs().max())
    for form in ("shared", "plain"):
        cfg, net, sd, lf = build(Z, 11, head_ctx="gc")
        net.train()
        net.freeze_batchnorm()
        net.shared_training(form == "shared")
        inp = dev_inp(bt if form == "shared" else ex, h0, c0)
        out = net(inp)
        o = out["att_bbx_out"].detach().cpu().double()
        e = float((o - o_64).abs().max())
        ls = lf(out, inp)
        print(f"gc {form} training step: max|out - fp64| {e:.3e} (CPU fp32 {e_cpu:.3e}), loss {ls['loss'].item():.6f} vs {ls64['loss'].item():.6f}")
        assert e <= 6 * e_cpu + 1e-4
        np.testing.assert_allclose(ls["loss"].item(), ls64["loss"].item(), rtol=2e-4)
        ls["loss"].backward()
        torch.cuda.synchronize()
        worst = TN.grad_errors(net, sd32, sd64)
        assert not worst, f"{form}: gradient error vs fp64 (HIP rel, CPU-fp32 rel): {worst[:8]}"
        bw = names(train_plan(net).bwd)
        assert bw.count("zsg_head_gc_bwd") == 1 and ("zsg_head_shared_conv0_bwd" in bw) == (form == "shared")


def test_flip_tta(Z, fixed_tiles):
    """eval_tta = flip: merge_ref of ONE plain eval forward of the 2B rows tta_batch builds, bit for bit (tests/test_gpu_tta_net.py)"""
    cfg, net = tta_build(Z, head_ctx="gc", eval_tta="flip")
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
        want = GR.zsgnet_forward(sd, bt2, h2, c2, **ref_kw(cfg, training=False))
    np.testing.assert_allclose(x2.cpu().numpy(), torch.cat([want["bbx_out"], want["att_out"]], 2).numpy(), rtol=2e-3, atol=5e-3)


@pytest.mark.parametrize("dtype,bb,ba", [("bf16", FN.BF16_BOX, FN.BF16_ATT), ("bf16_act", FN.ACT_BOX, FN.ACT_ATT)])
def test_reduced_precision_eval(Z, fixed_tiles, dtype, bb, ba):
    """eval_dtype = bf16 / bf16_act against the fp32 gc plan, within the bounds of those switches' own net tests; the block's math stays
    fp32: under bf16_act it runs between a cast of h1 to fp32 and a cast of y back to bf16"""
    cfg, net = tta_build(Z, head_ctx="gc")
    bt = O.synthetic_batch(2, 128, 128, seed=3)
    g = torch.Generator().manual_seed(0)
    h0, c0 = torch.randn(2, 2, 128, generator=g), torch.randn(2, 2, 128, generator=g)
    o32, _ = fwd5(net, bt, h0, c0)
    net.eval_precision(dtype)
    o16, _ = fwd5(net, bt, h0, c0)
    plan = [p for k, p in net._plans.items() if dtype in k][0]
    nm, wh = names(plan.fwd), whats(plan.fwd)
    i = nm.index("zsg_head_gc_fwd")
    if dtype == "bf16_act":
        assert nm[i - 1] == "zsg_cast_bf16_f32" and wh[i - 1] == "cast f32<-att_reg_box.h1"
        assert nm[i + 1] == "zsg_cast_f32_bf16" and wh[i + 1] == "cast bf16<-att_reg_box.h1g"
    else:
        assert "cast" not in wh[i - 1] and "cast" not in wh[i + 1]
    assert ("zsg_conv_igemm_bf16_io" if dtype == "bf16_act" else "zsg_conv_igemm_bf16") in nm
    rb, ra = rel(o16, o32)
    print(f"gc {dtype} eval parity: box {rb:.3e} att {ra:.3e} of max|fp32|")
    assert not torch.equal(o16, o32) and rb <= bb and ra <= ba


def test_bf16_head_training(Z, fixed_tiles):
    """train_dtype = bf16_head against the fp32 gc plan, within the bounds of tests/test_gpu_net_train_bf16_head.py"""
    res = {}
    bt = O.synthetic_batch(2, 128, 128, seed=3)
    g = torch.Generator().manual_seed(0)
    h0, c0 = torch.randn(2, 2, 128, generator=g), torch.randn(2, 2, 128, generator=g)
    for dt in ("fp32", "bf16_head"):
        config, evaluator, loss, mdl, optim = Z
        cfg, net = tta_build(Z, head_ctx="gc")
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
        fw = whats(train_plan(net).fwd)
        assert "att_reg_box.gc" in fw
        if dt == "bf16_head":
            assert [w for w in fw if w.startswith("att_reg_box.1.0") and w.endswith("+bf16")], "conv1 reads y on the bf16 path"
    (o32, l32, g32), (o16, l16, g16) = res["fp32"], res["bf16_head"]
    box, att = rel(o16, o32)
    rel_loss, l2 = abs(l16 - l32) / abs(l32), float((g16 - g32).norm() / g32.norm())
    cos = float((g16 * g32).sum() / (g16.norm() * g32.norm()))
    print(f"gc bf16_head parity: box {box:.3e} att {att:.3e} loss {rel_loss:.3e} flat l2 {l2:.3e} 1-cos {1 - cos:.3e}")
    assert not torch.equal(g16, g32)
    assert box <= FN.HEAD_BOX and att <= FN.HEAD_ATT and rel_loss <= FN.HEAD_LOSS and l2 <= FN.HEAD_L2 and cos >= FN.HEAD_COS


@pytest.mark.parametrize("only_gc", [True, False], ids=["only_gc_trains", "gc_frozen"])
def test_frozen_parameters(Z, only_gc):
    """as tests/test_gpu_finetune.py: a frozen tensor keeps p.grad None and its bits across an optimizer step; frozen gc tensors still
    pass the gradient on to h1, a frozen rest still trains the seven (and then nothing in front of h1 runs a backward)"""
    config, evaluator, loss, mdl, optim = Z
    cfg, net, sd, lf = build(Z, 12, head_ctx="gc")
    net.train()
    for n, p in net.named_parameters():
        p.requires_grad_((".gc." in n) == only_gc)
    opt = optim.FusedAdam(net, lr=1e-3, betas=(0.9, 0.99))
    before = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    bt, h0, c0 = TN.batch(cfg)
    inp = dev_inp(bt, h0, c0)
    opt.zero_grad()
    lf(net(inp), inp)["loss"].backward()
    torch.cuda.synchronize()
    kw = ref_kw(cfg)
    sd32 = TN.leaves(sd)
    ref = GR.zsgnet_forward(sd32, bt, h0, c0, **kw)
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
    plan = train_plan(net)
    bw, nm = whats(plan.bwd), names(plan.bwd)
    i = nm.index("zsg_head_gc_bwd")
    ptr = [getattr(a, "value", a) for a in plan.bwd.calls[i][1][12:20]]          # dx, then the seven gradients
    if only_gc:
        assert ptr[0] in (None, 0) and all(x not in (None, 0) for x in ptr[1:]), "no d(h1): nothing in front of it trains"
        assert not [w for w in bw if w.startswith(("mask+acc:", "dwe", "dgrad:att_reg_box.0.0", "wgrad:att_reg_box.0.0", "bsum")) or "backbone" in w
                    or "lstm" in w], bw
    else:
        assert ptr[0] not in (None, 0) and all(x in (None, 0) for x in ptr[1:]), "d(h1) alone: the seven gradient launches are skipped"
        assert "mask+acc:att_reg_box.h1" in bw and "wgrad:att_reg_box.0.0" in bw
    opt.step()
    torch.cuda.synchronize()
    after = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    for n, p in net.named_parameters():
        same = torch.equal(bits(after[n]), bits(before[n]))
        assert same == (not p.requires_grad), f"{n}: {'moved' if not same else 'did not move'}"


def test_everything_frozen_in_front_skips_the_backward(Z):
    """only the last convolution trains: neither h1 nor any gc tensor needs a gradient, so the block has no backward launch at all"""
    config, evaluator, loss, mdl, optim = Z
    cfg, net, sd, lf = build(Z, 12, head_ctx="gc")
    net.train()
    for n, p in net.named_parameters():
        p.requires_grad_(n.startswith("att_reg_box.5."))
    bt, h0, c0 = TN.batch(cfg)
    inp = dev_inp(bt, h0, c0)
    lf(net(inp), inp)["loss"].backward()
    torch.cuda.synchronize()
    plan = train_plan(net)
    assert "zsg_head_gc_fwd" in names(plan.fwd) and "zsg_head_gc_bwd" not in names(plan.bwd)
    assert dict(net.named_parameters())["att_reg_box.5.weight"].grad is not None


@pytest.mark.parametrize("opt_fn", ["Adam", "AdamW", "SGD", "LAMB"])
def test_an_optimizer_step_moves_the_seven_weights(Z, opt_fn):
    config, evaluator, loss, mdl, optim = Z
    cfg, net, sd, lf = build(Z, 12, head_ctx="gc", opt_fn=opt_fn)
    net.train()
    opt = optim.make_opt_fn(cfg)(net, lr=1e-3)
    before = {k: v.detach().cpu().clone() for k, v in net.state_dict().items() if ".gc." in k}
    bt, h0, c0 = TN.batch(cfg)
    inp = dev_inp(bt, h0, c0)
    opt.zero_grad()
    lf(net(inp), inp)["loss"].backward()
    opt.step()
    torch.cuda.synchronize()
    assert len(before) == 7
    for k, v in before.items():
        w = net.state_dict()[k].detach().cpu()
        assert bool(torch.isfinite(w).all()) and not torch.equal(bits(w), bits(v)), k + " did not move"


def test_checkpoint_round_trip_through_learner(Z, fixed_tiles, tmp_path):
    from zsgnet_pytorch_amd.trainer import Learner
    config, evaluator, loss, mdl, optim = Z

    def learner(uid, **flags):
        cfg = config.get_cfg(resnet_arch=ARCH, tmp_path=str(tmp_path), **flags)
        net = mdl.get_default_net(9, cfg)
        r, s = config.ratios_scales(cfg)
        return cfg, net, Learner(uid, None, net, loss.get_default_loss(r, s, cfg), cfg, evaluator.get_default_eval(r, s, cfg), None)
    cfg, net, la = learner("gc_a", head_ctx="gc")
    net.load_state_dict(seeded(cfg, 1, net.start_dim_head))
    net.to("cuda").eval()
    la.save_model_dict()
    ck = torch.load(la.model_file)["model_state_dict"]
    keys = gc_keys(cfg)
    assert all(float(ck[k].abs().max()) > 0 for k in keys)
    cfg_b, other, lb = learner("gc_b", head_ctx="gc")
    assert not other.state_dict()["att_reg_box.gc.fc2.weight"].any()
    assert lb.load_model_dict(str(la.model_file))
    other.to("cuda").eval()
    assert all(torch.equal(bits(other.state_dict()[k]), bits(ck[k])) for k in keys)
    bt = O.synthetic_batch(2, 128, 128, seed=3)
    g = torch.Generator().manual_seed(0)
    h0, c0 = torch.randn(2, 2, 128, generator=g), torch.randn(2, 2, 128, generator=g)
    o_a = fwd5(net, bt, h0, c0)[0]
    assert torch.equal(bits(o_a), bits(fwd5(other, bt, h0, c0)[0]))
    # a none checkpoint into a gc net: refused by default, taken with strict_load = False and then the none net's function, bit for bit
    cfg_c, plain, lc = learner("none_c")
    plain.load_state_dict({k: v for k, v in ck.items() if ".gc." not in k})
    plain.to("cuda").eval()
    lc.save_model_dict()
    _, strict, ls_ = learner("gc_strict", head_ctx="gc")
    with pytest.raises(RuntimeError, match="gc"):
        ls_.load_model_dict(str(lc.model_file))
    _, loose, ll = learner("gc_loose", head_ctx="gc", strict_load=False)
    assert ll.load_model_dict(str(lc.model_file))
    loose.to("cuda").eval()
    assert not loose.state_dict()["att_reg_box.gc.fc2.weight"].any() and not loose.state_dict()["att_reg_box.gc.fc2.bias"].any()
    o_c, o_l = fwd5(plain, bt, h0, c0)[0], fwd5(loose, bt, h0, c0)[0]
    scale = float(o_c.abs().max())
    print(f"none checkpoint in a gc net: max|diff| {float((o_l - o_c).abs().max()):.3e} at scale {scale:.3e}; gc vs none weights {float((o_a - o_c).abs().max()):.3e}")
    assert torch.equal(bits(o_l), bits(o_c)), "y = x + 0: the same values into the same launches"
    assert float((o_a - o_c).abs().max()) > 1e-2 * scale
