"""cfg lang_pool on the network: final / mean / attn against tests/langpool_ref.py, and that `last` is the program it was.

Geometry and rule of tests/test_gpu_net_lstm.py (ResNet-18, B = 3, 96 x 128, queries of up to 13 tokens with one tied pair of lengths,
seeded_state_dict seed 12): the float64 twin (langpool_ref.zsgnet_forward in float64) is the truth, the same code in float32 on the CPU the
yardstick — forward max error within 6 x CPU-fp32 + 1e-4, every parameter gradient within grad_tol, losses rel 2e-4.  The attention's
scorer lang_pool.weight is not in the oracle's seeded weights: it is drawn here (seeded, N(0, 1/16)), so that the attention is not the mean.

The shared-image, flip-TTA, frozen-encoder and checkpoint tests use the set-ups of tests/test_gpu_tta_net.py (ResNet-18, 128 px,
ZSG_AUTOTUNE=0 and ZSG_DETERMINISTIC=1: two forwards of one plan give the same bits)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import langpool_ref as R  # noqa: E402
import test_gpu_net_lstm as TN  # noqa: E402
import tta_ref  # noqa: E402
from oracle import zsg_oracle as O  # noqa: E402
from test_gpu_net import Z, grad_tol, to_dev  # noqa: E402,F401

ARCH, B = TN.ARCH, TN.B
HERE = os.path.dirname(os.path.abspath(__file__))


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


def seeded(cfg, seed, head_in):
    """the oracle's seeded weights at the cfg's language sizes, plus a drawn scorer for attn"""
    E, H, bid = cfg["emb_dim"], cfg["lstm_dim"], cfg["use_bidirectional"]
    sd = O.seeded_state_dict(ARCH, seed, emb_dim=E, lstm_dim=H, head_in=head_in)
    if not bid:
        sd = {k: v for k, v in sd.items() if not k.endswith("_reverse")}
    if cfg["lang_pool"] == "attn":
        sd["lang_pool.weight"] = torch.randn(1, H * (2 if bid else 1), generator=torch.Generator().manual_seed(seed + 100)) * 0.25
    return sd


def build(Z, seed, **flags):
    config, evaluator, loss, mdl, optim = Z
    cfg = config.get_cfg(resnet_arch=ARCH, **flags)
    net = mdl.get_default_net(9, cfg)
    sd = seeded(cfg, seed, net.start_dim_head)
    assert set(net.state_dict().keys()) == set(sd.keys())
    net.load_state_dict(sd)
    net.to("cuda")
    r, s = config.ratios_scales(cfg)
    return cfg, net, sd, loss.get_default_loss(r, s, cfg)


def twin64(sd, bt, h0, c0, anc, **kw):
    """test_gpu_net.fp64_twin on langpool_ref.zsgnet_forward"""
    sd64 = {k: (v.detach().double().requires_grad_(v.requires_grad) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    bt64 = {k: v.double() for k, v in bt.items()}
    ref = R.zsgnet_forward(sd64, bt64, h0.double(), c0.double(), arch=ARCH, rank=O.sort_rank(bt["qlens"]), **kw)
    ls = O.torch_loss(ref, bt["annot"], anc)
    ls["loss"].backward()
    return sd64, ref, ls


def out5(ref):
    return torch.cat([ref["bbx_out"], ref["att_out"]], 2).detach().double()


CASES = {"final_h128": dict(lang_pool="final"), "mean_h128": dict(lang_pool="mean"), "attn_h128": dict(lang_pool="attn"),
         "attn_h32": dict(lang_pool="attn", lstm_dim=32), "attn_uni_h128": dict(lang_pool="attn", use_bidirectional=False),
         "mean_h256": dict(lang_pool="mean", lstm_dim=256)}


@pytest.mark.parametrize("tag", list(CASES))
def test_forward_backward_vs_reference(Z, tag):
    """test_gpu_net_lstm.check_step with langpool_ref's twin"""
    cfg, net, sd, lf = build(Z, 12, **CASES[tag])
    net.train()
    bt, h0, c0 = TN.batch(cfg)
    assert len(set(bt["qlens"].tolist())) < B and int(bt["qlens"].max()) == TN.TMAX
    inp = to_dev(bt)
    inp["h0"], inp["c0"] = h0, c0
    out = net(inp)
    kw = dict(bidirectional=cfg["use_bidirectional"], lang_pool=cfg["lang_pool"])
    sd32 = TN.leaves(sd)
    ref = R.zsgnet_forward(sd32, bt, h0, c0, arch=ARCH, **kw)
    assert out["feat_sizes"].tolist() == ref["feat_sizes"].tolist()
    anc, A = TN.anchors_of(ref)
    assert out["att_bbx_out"].shape == (B, A, 5)
    sd64, ref64, ls64 = twin64(sd32, bt, h0, c0, anc, **kw)
    o_gpu, o_cpu, o_64 = out["att_bbx_out"].detach().cpu().double(), out5(ref), out5(ref64)
    e_gpu, e_cpu = float((o_gpu - o_64).abs().max()), float((o_cpu - o_64).abs().max())
    tol = 6 * e_cpu + 1e-4
    print(f"forward {tag}: HIP err {e_gpu:.3g} vs fp64, CPU fp32 err {e_cpu:.3g}")
    # the mode matters on this batch: the float64 output of the reference's own vector (`last`) is far outside what is allowed
    with torch.no_grad():
        last64 = R.zsgnet_forward({k: v.detach() for k, v in sd64.items()}, {k: v.double() for k, v in bt.items()}, h0.double(), c0.double(),
                                  arch=ARCH, rank=O.sort_rank(bt["qlens"]), bidirectional=cfg["use_bidirectional"], lang_pool="last")
    gap = float((out5(last64) - o_64).abs().max())
    print(f"forward {tag}: |{cfg['lang_pool']} - last| {gap:.3g} in float64, allowed error {tol:.3g}")
    assert gap > 100 * tol, f"{tag}: the float64 outputs of {cfg['lang_pool']} and last differ by {gap:.3g} only (allowed error {tol:.3g})"
    assert e_gpu <= tol, f"forward: HIP err {e_gpu:.3g} vs fp64, CPU fp32 err {e_cpu:.3g}"
    ls = lf(out, inp)
    for k in ("loss", "cls_ls", "box_ls"):
        np.testing.assert_allclose(ls[k].item(), ls64[k].item(), rtol=2e-4, err_msg=k)
    O.torch_loss(ref, bt["annot"], anc)["loss"].backward()
    ls["loss"].backward()
    torch.cuda.synchronize()
    if cfg["lang_pool"] == "attn":
        assert float(sd64["lang_pool.weight"].grad.abs().max()) > 0
    worst = TN.grad_errors(net, sd32, sd64)
    assert not worst, f"gradient error vs fp64 (HIP rel, CPU-fp32 rel): {worst[:8]}"


def test_attn_from_its_initial_weight_is_mean(Z, fixed_tiles):
    """lang_pool.weight = 0 (its initial value): the forward output of the attn net is the mean net's"""
    cfg_a, net_a, sd, _ = build(Z, 12, lang_pool="attn")
    cfg_m, net_m, _, _ = build(Z, 12, lang_pool="mean")
    with torch.no_grad():
        net_a.state_dict()["lang_pool.weight"].zero_()
    net_a.eval(), net_m.eval()
    bt, h0, c0 = TN.batch(cfg_a)
    inp = to_dev(bt)
    inp["h0"], inp["c0"] = h0, c0
    with torch.no_grad():
        a, m = net_a(inp)["att_bbx_out"].clone(), net_m(inp)["att_bbx_out"].clone()
    torch.cuda.synchronize()
    # alpha_t = 1 / len exactly, but sum_t (1/len) o_t and (sum_t o_t) / len round differently: a few ulps of `we`, through the head.
    # Two fp32 evaluations of one function: the floor of the project's forward criterion for eval outputs, which grow with the seeded
    # running statistics (tests/test_gpu_net_lstm.py::test_eval_forward_lstm_dim_32: 1e-4 * max(1, max|out|))
    scale = float(m.abs().max())
    print(f"attn(w = 0) vs mean: max|diff| {float((a - m).abs().max()):.3e}, scale {scale:.3e}")
    assert float((a - m).abs().max()) <= 1e-4 * max(1.0, scale)


def whats(prog):
    return [c[2] for c in prog.calls]


def test_last_builds_the_plan_it_was(Z, fixed_tiles):
    """lang_pool = "last" (the default): the training plan's forward and backward launch lists are the ones recorded from the plan before
    the key existed (tests/golden/langpool_last_plan.json: ResNet-18, B = 3, 96 x 128, ZSG_AUTOTUNE=0), name for name"""
    with open(os.path.join(HERE, "golden", "langpool_last_plan.json")) as f:
        want = json.load(f)
    for flags in (dict(), dict(lang_pool="last")):
        cfg, net, sd, lf = build(Z, 12, **flags)
        net.train()
        bt, h0, c0 = TN.batch(cfg)
        inp = to_dev(bt)
        inp["h0"], inp["c0"] = h0, c0
        lf(net(inp), inp)["loss"].backward()
        torch.cuda.synchronize()
        plan = [p for k, p in net._plans.items() if k[-1]][0]
        assert whats(plan.fwd) == want["fwd"] and whats(plan.bwd) == want["bwd"]
        enc = [w for w in want["fwd"] if w.startswith(("gather_last", "lstm"))]
        assert enc == ["lstm_in", "lstm", "gather_last", "lstm_in_reverse", "lstm_reverse"]
    cfg, net, sd, lf = build(Z, 12, lang_pool="final")
    net.train()
    lf(net(inp), inp)["loss"].backward()
    plan = [p for k, p in net._plans.items() if k[-1]][0]
    enc = [w for w in whats(plan.fwd) if w.startswith(("gather_last", "lstm", "lang_pool"))]
    assert enc == ["lstm_in", "lstm_seq", "lstm_in_reverse", "lstm_seq_reverse"]
    assert [w for w in whats(plan.fwd) if w not in enc] == [w for w in want["fwd"] if not w.startswith(("gather_last", "lstm"))]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def tta_build(Z, **flags):
    """tests/test_gpu_tta_net.py's network: ResNet-18, seeded_state_dict seed 1"""
    config, evaluator, loss, mdl, optim = Z
    cfg = config.get_cfg(resnet_arch=ARCH, **flags)
    net = mdl.get_default_net(9, cfg)
    net.load_state_dict(seeded(cfg, 1, net.start_dim_head))
    return cfg, net.to("cuda").eval()


def fwd5(net, bt, h0, c0):
    inp = {k: v.cuda() for k, v in bt.items()}
    inp["h0"], inp["c0"] = h0, c0
    with torch.no_grad():
        out = net(inp)
    torch.cuda.synchronize()
    return out["att_bbx_out"].detach().clone(), out


def test_shared_image_eval_under_attn(Z, fixed_tiles):
    """4 queries over 2 images.  The query encoder of the shared plan runs the Q rows the plain plan of the expanded batch runs: the
    pooled vector `we` is the same bits in both.  The outputs follow the rule of tests/test_gpu_shared_net.py (which holds for `last`
    as for every mode: the shared plan forms conv0 as a per-image feature GEMM plus a per-query language map, another summation order
    than the plain plan's one GEMM, so its rows agree with the plain forward to rounding, not to the bit — measured on this batch with
    ZSG_DETERMINISTIC=1: max|shared - plain| 1.7e-4 under `last`, 1.9e-4 under `attn`, at an output scale of 98.6): within 2e-4 of the
    output's scale of the CPU oracle, and no further from it than max(4 x the plain path's distance, 2e-3)."""
    from zsgnet_pytorch_amd import synth
    cfg, net = tta_build(Z, lang_pool="attn")
    bt = synth.synthetic_shared_batch(2, 4, 128, 128, seed=5)
    g = torch.Generator().manual_seed(1)
    h0, c0 = torch.randn(2, 4, 128, generator=g), torch.randn(2, 4, 128, generator=g)
    s, _ = fwd5(net, bt, h0, c0)
    shared = [p for k, p in net._plans.items() if "shared" in k]
    assert len(shared) == 1
    we_s = shared[0].acts["we"].buf.clone()
    p, _ = fwd5(net, synth.expand_shared(bt), h0, c0)
    plain = [p_ for k, p_ in net._plans.items() if "shared" not in k]
    assert len(plain) == 1 and tuple(s.shape) == tuple(p.shape) and s.shape[0] == 4
    assert torch.equal(bits(we_s), bits(plain[0].acts["we"].buf)), "the pooled vectors of the shared and the plain plan differ"
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        ref = R.zsgnet_forward(sd, synth.expand_shared(bt), h0, c0, arch=ARCH, training=False, lang_pool="attn")
    want = torch.cat([ref["bbx_out"], ref["att_out"]], 2)
    scale = float(want.abs().max())
    d_s, d_p = float((s.cpu() - want).abs().max()), float((p.cpu() - want).abs().max())
    print(f"shared eval under attn: max|shared - ref| {d_s:.3e}, max|plain - ref| {d_p:.3e}, max|shared - plain| {float((s - p).abs().max()):.3e}, scale {scale:.3e}")
    assert d_s < 2e-4 * scale and d_s <= max(4 * d_p, 2e-3)
    # and it is the attention's output: not what the same weights give with the scorer at 0
    with torch.no_grad():
        net.state_dict()["lang_pool.weight"].zero_()
    fwd5(net, bt, h0, c0)
    # (|we| < 1 and fp32 rounds it at 1e-7: a uniform attention moves it a thousand times further)
    assert float((shared[0].acts["we"].buf - we_s).abs().max()) > 1e-4


def test_flip_tta_under_mean(Z, fixed_tiles):
    """eval_tta = flip: merge_ref of ONE plain eval forward of the 2B rows tta_batch builds, bit for bit (tests/test_gpu_tta_net.py)"""
    cfg, net = tta_build(Z, lang_pool="mean", eval_tta="flip")
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
    # the 2B rows are the mean-pooled network's: the float32 host definition agrees with them
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        want = R.zsgnet_forward(sd, bt2, h2, c2, arch=ARCH, training=False, lang_pool="mean")
    np.testing.assert_allclose(x2.cpu().numpy(), torch.cat([want["bbx_out"], want["att_out"]], 2).numpy(), rtol=2e-3, atol=5e-3)


def test_frozen_lstm_leaves_the_scorer_training(Z):
    """requires_grad = False on lstm.*: one optimizer step moves lang_pool.weight (and the head) and leaves the LSTM's bits alone; the
    backward holds the pool's launches and no BPTT sweep"""
    config, evaluator, loss, mdl, optim = Z
    cfg, net, sd, lf = build(Z, 12, lang_pool="attn")
    net.train()
    for n, p in net.named_parameters():
        p.requires_grad_(not n.startswith("lstm."))
    opt = optim.FusedAdam(net, lr=1e-3, betas=(0.9, 0.99))
    before = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    bt, h0, c0 = TN.batch(cfg)
    inp = to_dev(bt)
    inp["h0"], inp["c0"] = h0, c0
    opt.zero_grad()
    lf(net(inp), inp)["loss"].backward()
    g = dict(net.named_parameters())["lang_pool.weight"].grad
    assert g is not None and float(g.abs().max()) > 0
    # the scorer's gradient is the host definition's
    sd32 = TN.leaves(sd)
    ref = R.zsgnet_forward(sd32, bt, h0, c0, arch=ARCH, lang_pool="attn")
    anc, _ = TN.anchors_of(ref)
    sd64, _, _ = twin64(sd32, bt, h0, c0, anc, lang_pool="attn")
    O.torch_loss(ref, bt["annot"], anc)["loss"].backward()
    g64 = sd64["lang_pool.weight"].grad.flatten()
    eg, ec = float((g.cpu().double().flatten() - g64).norm()), float((sd32["lang_pool.weight"].grad.double().flatten() - g64).norm())
    assert eg <= grad_tol(ec, g64), (eg, ec)
    opt.step()
    torch.cuda.synchronize()
    after = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    assert not torch.equal(after["lang_pool.weight"], before["lang_pool.weight"]), "the scorer did not move"
    assert not torch.equal(after["att_reg_box.0.0.weight"], before["att_reg_box.0.0.weight"])
    for k in before:
        if k.startswith("lstm."):
            assert torch.equal(bits(after[k]), bits(before[k])), f"the frozen {k} moved"
    plan = [p for k, p in net._plans.items() if k[-1]][0]
    bw = whats(plan.bwd)
    assert "lang_pool_bwd" in bw and "wgrad:lang_pool" in bw and not [w for w in bw if w.startswith(("lstm_seq_bwd", "wgrad:w_", "bgrad:lstm"))]
    # frozen itself, with the LSTM training: the sweeps run, the scorer's gradient launch does not
    cfg, net, sd, lf = build(Z, 12, lang_pool="attn")
    net.train()
    dict(net.named_parameters())["lang_pool.weight"].requires_grad_(False)
    lf(net(inp), inp)["loss"].backward()
    torch.cuda.synchronize()
    bw = whats([p for k, p in net._plans.items() if k[-1]][0].bwd)
    assert "lang_pool_bwd" in bw and "wgrad:lang_pool" not in bw and "lstm_seq_bwd" in bw and "lstm_seq_bwd_reverse" in bw


def test_checkpoint_round_trip(Z, fixed_tiles, tmp_path):
    config, evaluator, loss, mdl, optim = Z
    cfg, net = tta_build(Z, lang_pool="attn")
    path = str(tmp_path / "attn.pt")
    torch.save({k: v.detach().cpu() for k, v in net.state_dict().items()}, path)
    ck = torch.load(path)
    assert "lang_pool.weight" in ck and float(ck["lang_pool.weight"].abs().max()) > 0
    other = mdl.get_default_net(9, cfg)
    assert not other.state_dict()["lang_pool.weight"].any()
    other.load_state_dict(ck)
    other.to("cuda").eval()
    assert torch.equal(bits(other.state_dict()["lang_pool.weight"]), bits(ck["lang_pool.weight"]))
    bt = O.synthetic_batch(2, 128, 128, seed=3)
    g = torch.Generator().manual_seed(0)
    h0, c0 = torch.randn(2, 2, 128, generator=g), torch.randn(2, 2, 128, generator=g)
    assert torch.equal(bits(fwd5(net, bt, h0, c0)[0]), bits(fwd5(other, bt, h0, c0)[0]))
    # the other modes keep the reference's keys: they refuse the extra one, and attn misses it in theirs
    mean = mdl.get_default_net(9, config.get_cfg(resnet_arch=ARCH, lang_pool="mean"))
    with pytest.raises(RuntimeError, match="lang_pool.weight"):
        mean.load_state_dict(ck)
    with pytest.raises(RuntimeError, match="lang_pool.weight"):
        mdl.get_default_net(9, cfg).load_state_dict({k: v for k, v in ck.items() if k != "lang_pool.weight"})
