"""The network at the language widths nothing else runs: cfg lstm_dim 32 / 64 / 256, use_bidirectional=False, emb_dim 100 / 200,
and the image-blind head at lstm_dim 64.  These change the width of `we` (Cw = lstm_dim x directions), with it the K extent and
the weight-column offsets of the head's language / grid decomposition (_lower_head), the h0 | c0 staging (one direction: half of
it, no gather_last launch) and the K extent of the input projection.  Same method as test_forward_backward_vs_oracle in
tests/test_gpu_net.py: the float64 oracle is the truth, the CPU-fp32 oracle the yardstick (forward max error within
6 x + 1e-4, every parameter gradient within grad_tol, losses rel 2e-4).

Weights: seeded_state_dict seed 12.  With seed 11 and this batch one layer4.0 activation of the TRUNK sits on a ReLU boundary
(grad_tol's docstring): the gradients of layer4.0 and of everything below it are then 0.7 - 0.8 % off the float64 ones at the
default lstm_dim = 128 as well, with the head / LSTM gradients at 3e-6, and 1.5 - 1.7 % at lstm_dim = 256 where the loss weighs
that element more; seed 12 on the same geometry agrees to 5e-6 everywhere.  The trunk does not depend on the language width,
so these tests use weights without such a tie instead of spending grad_tol's allowance on it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import zsg_oracle as O  # noqa: E402
from test_gpu_net import RATIOS, SCALES, Z, fp64_twin, grad_tol, to_dev  # noqa: E402,F401

ARCH, B, IMG_H, IMG_W, TMAX = "resnet18", 3, 96, 128, 13


@pytest.fixture(scope="module", autouse=True)
def _leave_the_tuner_as_found():
    """The plans built here autotune their launch shapes into the process-wide cache, and ResNet-18 at B = 3 shares its deep
    pyramid levels (3 x 4, 2 x 2, 1 x 1) with other tests' geometries: tests/test_gpu_tuner.py counts the candidates tuned
    from scratch in its own forward, so the choices made here must not outlive this module."""
    if not torch.cuda.is_available():
        yield
        return
    from zsgnet_pytorch_amd import ops
    saved = dict(ops._TUNE_CACHE)
    yield
    ops._TUNE_CACHE.clear()
    ops._TUNE_CACHE.update(saved)


def build(Z, seed, **flags):
    """network + the seeded state dict of its sizes (no `_reverse` keys for the single-direction encoder)"""
    config, evaluator, loss, mdl, optim = Z
    cfg = config.get_cfg(resnet_arch=ARCH, **flags)
    net = mdl.get_default_net(9, cfg)
    E, H, bid = cfg["emb_dim"], cfg["lstm_dim"], cfg["use_bidirectional"]
    Cw = H * (2 if bid else 1)
    if cfg["use_img"]:
        assert net.start_dim_head == 256 + Cw + 2
    sd = O.seeded_state_dict(ARCH, seed, emb_dim=E, lstm_dim=H, head_in=net.start_dim_head)
    if not bid:
        sd = {k: v for k, v in sd.items() if not k.endswith("_reverse")}
        assert not [n for n, _ in net.named_parameters() if n.endswith("_reverse")]
        h0, c0 = net.lstm_init_hidden(B)
        assert h0.shape == c0.shape == (1, B, H)
    assert set(net.state_dict().keys()) == set(sd.keys())
    net.load_state_dict(sd)
    net.to("cuda")
    r, s = config.ratios_scales(cfg)
    return cfg, net, sd, loss.get_default_loss(r, s, cfg)


def batch(cfg, seed=5, lens=None):
    """B = 3 images of 96 x 128, queries of up to 13 tokens with one tied pair of lengths; h0 / c0 [directions, B, H]"""
    bt = O.synthetic_batch(B, IMG_H, IMG_W, seed=seed, tmax=TMAX)
    bt["qlens"][-1] = bt["qlens"][0]
    if lens is not None:
        bt["qlens"] = torch.tensor(lens, dtype=torch.float32)
    bt["qvec"] = bt["qvec"][..., :cfg["emb_dim"]].contiguous()
    gq = torch.Generator().manual_seed(2)
    nd, H = (2 if cfg["use_bidirectional"] else 1), cfg["lstm_dim"]
    return bt, torch.randn(nd, B, H, generator=gq), torch.randn(nd, B, H, generator=gq)


def oracle_kw(cfg):
    return dict(use_img=cfg["use_img"], use_lang=cfg["use_lang"], bidirectional=cfg["use_bidirectional"])


def leaves(sd):
    sd = {k: v.clone() for k, v in sd.items()}
    for k, v in sd.items():
        if v.is_floating_point() and "running" not in k:
            v.requires_grad_()
    return sd


def grad_errors(net, sd32, sd64, only=None):
    """parameters whose HIP gradient is further from the float64 one than grad_tol allows: (name, HIP rel, CPU-fp32 rel)"""
    worst = []
    for n, p in net.named_parameters():
        if only is not None and not n.startswith(only):
            continue
        assert p.grad is not None, n
        if sd64[n].grad is None:          # (image-blind: the trunk feeds nothing, the reference leaves its gradients unset)
            assert float(p.grad.abs().max()) == 0.0, n
            continue
        g64 = sd64[n].grad.flatten()
        eg = float((p.grad.cpu().double().flatten() - g64).norm())
        ec = float((sd32[n].grad.double().flatten() - g64).norm())
        if eg > grad_tol(ec, g64):
            worst.append((n, eg / (float(g64.norm()) + 1e-30), ec / (float(g64.norm()) + 1e-30)))
    return worst


def anchors_of(ref):
    fs = [tuple(r) for r in ref["feat_sizes"].tolist()]
    return torch.from_numpy(O.create_anchors(fs, RATIOS, SCALES).astype(np.float32)), 9 * sum(h * w for h, w in fs)


def check_step(cfg, net, lf, sd, bt, h0, c0, only=None):
    """one forward + loss + backward of `net` (train mode) against the oracle on the weights `sd`"""
    inp = to_dev(bt)
    inp["h0"], inp["c0"] = h0, c0
    out = net(inp)
    kw = oracle_kw(cfg)
    sd32 = leaves(sd)
    ref = O.zsgnet_forward(sd32, bt, h0, c0, arch=ARCH, **kw)
    assert out["feat_sizes"].tolist() == ref["feat_sizes"].tolist()
    anc, A = anchors_of(ref)
    assert out["att_bbx_out"].shape == (B, A, 5)
    sd64, ref64, ls64 = fp64_twin(sd32, bt, h0, c0, ARCH, anc, **kw)
    o_gpu = out["att_bbx_out"].detach().cpu().double()
    o_cpu = torch.cat([ref["bbx_out"], ref["att_out"]], 2).detach().double()
    o_64 = torch.cat([ref64["bbx_out"], ref64["att_out"]], 2).detach()
    e_gpu, e_cpu = float((o_gpu - o_64).abs().max()), float((o_cpu - o_64).abs().max())
    print(f"forward: HIP err {e_gpu:.3g} vs fp64, CPU fp32 err {e_cpu:.3g}")
    assert e_gpu <= 6 * e_cpu + 1e-4, f"forward: HIP err {e_gpu:.3g} vs fp64, CPU fp32 err {e_cpu:.3g}"
    ls = lf(out, inp)
    for k in ("loss", "cls_ls", "box_ls"):
        np.testing.assert_allclose(ls[k].item(), ls64[k].item(), rtol=2e-4, err_msg=k)
    O.torch_loss(ref, bt["annot"], anc)["loss"].backward()
    ls["loss"].backward()
    torch.cuda.synchronize()
    worst = grad_errors(net, sd32, sd64, only)
    assert not worst, f"gradient error vs fp64 (HIP rel, CPU-fp32 rel): {worst[:8]}"


CASES = {"h32": dict(lstm_dim=32), "h64": dict(lstm_dim=64), "h256": dict(lstm_dim=256),
         "uni_h128": dict(use_bidirectional=False), "uni_h32": dict(use_bidirectional=False, lstm_dim=32),
         "e100": dict(emb_dim=100), "e200_h64": dict(emb_dim=200, lstm_dim=64), "img_blind_h64": dict(use_img=False, lstm_dim=64)}


@pytest.mark.parametrize("tag", list(CASES))
def test_forward_backward_vs_oracle(Z, tag):
    cfg, net, sd, lf = build(Z, 12, **CASES[tag])
    net.train()
    bt, h0, c0 = batch(cfg)
    assert len(set(bt["qlens"].tolist())) < B and int(bt["qlens"].max()) == TMAX
    check_step(cfg, net, lf, sd, bt, h0, c0)


def test_short_queries_after_long_ones_on_one_plan(Z):
    """A step with queries of up to 13 tokens, then one with every query <= 3 tokens on the same plan: the saved gates / cell states /
    hidden states beyond the new lengths are the first step's.  None of it may reach the second step's gradients."""
    config, evaluator, loss, mdl, optim = Z
    cfg, net, sd, lf = build(Z, 13, lstm_dim=64)
    net.train()
    opt = optim.FusedAdam(net, lr=1e-3, betas=(0.9, 0.99))
    bt, h0, c0 = batch(cfg)
    inp = to_dev(bt)
    inp["h0"], inp["c0"] = h0, c0
    opt.zero_grad()
    lf(net(inp), inp)["loss"].backward()
    opt.step()
    torch.cuda.synchronize()
    sd2 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    assert not torch.equal(sd2["lstm.weight_hh_l0"], sd["lstm.weight_hh_l0"])
    bt2, h0, c0 = batch(cfg, lens=[3.0, 1.0, 3.0])
    opt.zero_grad()
    check_step(cfg, net, lf, sd2, bt2, h0, c0, only=("lstm.", "att_reg_box.0.0."))
    assert len(net._plans) == 1, "both steps must run on one plan"


def test_eval_forward_lstm_dim_32(Z):
    """eval mode (the folded-BatchNorm plan) with non-trivial running statistics at lstm_dim = 32.  The activations grow with
    random statistics, so the floor of the forward criterion scales with the output: 6 x CPU-fp32 error + 1e-4 * max(1, max|out|)."""
    cfg, net, sd, lf = build(Z, 3, lstm_dim=32)
    g = torch.Generator().manual_seed(1)
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.05
        if k.endswith("running_var"):
            sd[k] = torch.rand(sd[k].shape, generator=g) + 0.5
    net.load_state_dict(sd)
    net.eval()
    bt, h0, c0 = batch(cfg, seed=9)
    inp = to_dev(bt)
    inp["h0"], inp["c0"] = h0, c0
    with torch.no_grad():
        out = net(inp)
        ref = O.zsgnet_forward({k: v.clone() for k, v in sd.items()}, bt, h0, c0, arch=ARCH, training=False)
        ref64 = O.zsgnet_forward({k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()},
                                 {k: v.double() for k, v in bt.items()}, h0.double(), c0.double(), arch=ARCH, training=False,
                                 rank=O.sort_rank(bt["qlens"]))
    anc, A = anchors_of(ref)
    assert out["att_bbx_out"].shape == (B, A, 5)
    o_gpu = out["att_bbx_out"].cpu().double()
    o_cpu = torch.cat([ref["bbx_out"], ref["att_out"]], 2).double()
    o_64 = torch.cat([ref64["bbx_out"], ref64["att_out"]], 2)
    e_gpu, e_cpu, scale = float((o_gpu - o_64).abs().max()), float((o_cpu - o_64).abs().max()), float(o_64.abs().max())
    print(f"eval forward: HIP err {e_gpu:.3g} vs fp64, CPU fp32 err {e_cpu:.3g}, scale {scale:.3g}")
    assert e_gpu <= 6 * e_cpu + 1e-4 * max(1.0, scale), f"eval forward: HIP err {e_gpu:.3g} vs fp64, CPU fp32 err {e_cpu:.3g}, scale {scale:.3g}"
