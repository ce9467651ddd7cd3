"""Shared-image TRAINING (ZSGNet.shared_training: a train-mode batch with `img_idx`, the trunk and head conv0's feature GEMM once per
distinct image, forward and backward) against the float64 twin of the composed oracle (tests/shared_train_ref.py, itself pinned to
oracle.zsgnet_forward by tests/test_cpu_shared_train_oracle.py).

Bounds — those tests/test_gpu_net.py::test_forward_backward_vs_oracle applies to the plain path, unchanged, none taken from what the
code gives: forward e_gpu <= 6 * e_cpu + 1e-4 (e_cpu: the CPU fp32 composed oracle's own distance to fp64), loss rtol 2e-4, every
gradient within grad_tol (6x the CPU fp32 error + 2e-4 of the norm, or 1.5 % of the norm for ReLU-boundary flips).  Running statistics:
test_gpu_net.py's rtol 1e-4 (mean) / 1e-3 (variance)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import zsg_oracle as O  # noqa: E402
from shared_train_ref import as_fp64, shared_forward, want_grads  # noqa: E402

RATIOS, SCALES = O.default_ratios_scales()

CASES = {
    "r18_equal": dict(arch="resnet18", flags={}, hw=96, idx=[1, 0, 2, 0, 2, 1], training=True),
    "r18_unequal": dict(arch="resnet18", flags={}, hw=96, idx=[1, 0, 2, 0, 2, 1, 1, 1], training=True),
    "r50_frozen_bn_unequal": dict(arch="resnet50", flags={}, hw=128, idx=[1, 0, 2, 0, 2, 1, 1, 1], training=False),
    "ssd_vgg": dict(arch="ssd_vgg", flags=dict(mdl_to_use="ssd_vgg"), hw=300, idx=[1, 0, 0, 1, 0], training=True),
    "do_norm": dict(arch="resnet18", flags=dict(do_norm=True), hw=96, idx=[1, 0, 2, 0, 2, 1], training=True),
    "two_heads": dict(arch="resnet18", flags=dict(use_same_atb=False), hw=96, idx=[1, 0, 2, 0, 2, 1], training=True),
}


@pytest.fixture(scope="module")
def Z():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import config, loss, mdl, optim, synth
    return config, loss, mdl, optim, synth


def grad_tol(ec: float, g64: torch.Tensor) -> float:
    """tests/test_gpu_net.py::grad_tol"""
    n = float(g64.norm())
    return max(6 * ec + 2e-4 * n, 1.5e-2 * n) + 1e-9


def build(Z, tag, seed=11, shared=True):
    config, loss, mdl, optim, synth = Z
    c = CASES[tag]
    if c["arch"] == "ssd_vgg":
        cfg = config.get_cfg(**c["flags"])
        sd = O.seeded_ssd_state_dict(seed)
    else:
        cfg = config.get_cfg(resnet_arch=c["arch"], **c["flags"])
        sd = O.seeded_state_dict(c["arch"], seed, same_atb=bool(cfg["use_same_atb"]))
    net = mdl.get_default_net(9, cfg)
    net.load_state_dict(sd)
    net.to("cuda").train()
    if not c["training"]:
        net.freeze_batchnorm()
    if shared:
        assert net.shared_training(True) is net
    r, s = config.ratios_scales(cfg)
    return cfg, net, sd, loss.get_default_loss(r, s, cfg)


def make_batch(Z, hw, idx, seed=21, tmax=13):
    synth = Z[4]
    Bi, Q = max(idx) + 1, len(idx)
    bt = synth.synthetic_shared_batch(Bi, Q, hw, hw, seed=seed, tmax=tmax)
    bt["img_idx"] = torch.tensor(idx, dtype=torch.long)
    bt["qlens"][-1] = bt["qlens"][0]
    gq = torch.Generator().manual_seed(seed + 1)
    h0, c0 = torch.randn(2, Q, 128, generator=gq), torch.randn(2, Q, 128, generator=gq)
    return bt, h0, c0


def to_dev(bt, h0, c0):
    inp = {k: v.cuda() for k, v in bt.items()}
    inp["h0"], inp["c0"] = h0, c0
    return inp


def oracle_pair(c, cfg, sd, bt, h0, c0):
    """the CPU fp32 composed oracle and its fp64 twin, both back-propagated; returns (sd, out, sd64, out64, loss64)"""
    want_grads(sd)
    kw = dict(arch=c["arch"], training=c["training"], do_norm=bool(cfg["do_norm"]))
    ref = shared_forward(sd, bt, h0, c0, **kw)
    fs = [tuple(r) for r in ref["feat_sizes"].tolist()]
    anc = torch.from_numpy(O.create_anchors(fs, RATIOS, SCALES).astype(np.float32))
    O.torch_loss(ref, bt["annot"], anc)["loss"].backward()
    sd64, bt64 = as_fp64(sd, bt)
    ref64 = shared_forward(sd64, bt64, h0.double(), c0.double(), rank=O.sort_rank(bt["qlens"]), **kw)
    ls64 = O.torch_loss(ref64, bt["annot"], anc)
    ls64["loss"].backward()
    return ref, sd64, ref64, ls64


def cat5(o):
    return torch.cat([o["bbx_out"], o["att_out"]], 2).detach().double()


def check_grads(net, sd, sd64, only=None):
    worst = []
    for n, p in net.named_parameters():
        if only is not None and not only(n):
            continue
        g64 = sd64[n].grad
        if g64 is None:                          # a parameter nothing reads (SSD-VGG's unused extras): the reference leaves it unset
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
            continue
        assert p.grad is not None, n
        g64 = g64.flatten()
        eg = float((p.grad.cpu().double().flatten() - g64).norm())
        ec = float((sd[n].grad.double().flatten() - g64).norm())
        if eg > grad_tol(ec, g64):
            worst.append((n, eg / (float(g64.norm()) + 1e-30), ec / (float(g64.norm()) + 1e-30)))
    assert not worst, f"gradient error vs fp64 (HIP rel, CPU-fp32 rel): {worst[:8]}"


@pytest.mark.parametrize("tag", list(CASES))
def test_shared_training_forward_loss_backward_vs_fp64_oracle(Z, tag):
    synth = Z[4]
    c = CASES[tag]
    cfg, net, sd, lf = build(Z, tag)
    bt, h0, c0 = make_batch(Z, c["hw"], c["idx"])
    inp = to_dev(bt, h0, c0)
    out = net(inp)
    ref, sd64, ref64, ls64 = oracle_pair(c, cfg, sd, bt, h0, c0)
    assert out["feat_sizes"].tolist() == ref["feat_sizes"].tolist()
    o_gpu, o_cpu, o_64 = out["att_bbx_out"].detach().cpu().double(), cat5(ref), cat5(ref64)
    assert o_gpu.shape == o_64.shape and o_gpu.shape[0] == len(c["idx"])
    e_gpu, e_cpu = float((o_gpu - o_64).abs().max()), float((o_cpu - o_64).abs().max())
    # the plain path on the expanded batch, beside it (a fresh network: the running statistics of `net` must see ONE forward).  With
    # unequal groups and train-mode BatchNorm it computes a different function: printed, never asserted
    _, net_p, _, _ = build(Z, tag, shared=False)
    with torch.no_grad():
        o_pl = net_p(to_dev(synth.expand_shared(bt), h0, c0))["att_bbx_out"].cpu().double()
    e_pl = float((o_pl - o_64).abs().max())
    ls = lf(out, inp)
    print(f"shared-train parity {tag} (Bi={max(c['idx']) + 1}, Q={len(c['idx'])}, {c['hw']}^2): max|out - fp64| shared {e_gpu:.3e}, "
          f"CPU fp32 oracle {e_cpu:.3e}, plain path on the expanded batch {e_pl:.3e}; loss {ls['loss'].item():.6f} vs fp64 {ls64['loss'].item():.6f}")
    assert e_gpu <= 6 * e_cpu + 1e-4, f"forward: HIP err {e_gpu:.3g} vs fp64, CPU fp32 err {e_cpu:.3g}"
    np.testing.assert_allclose(ls["loss"].item(), ls64["loss"].item(), rtol=2e-4)
    ls["loss"].backward()
    torch.cuda.synchronize()
    check_grads(net, sd, sd64)


def test_running_statistics_are_those_of_the_distinct_images(Z):
    synth = Z[4]
    c = CASES["r18_equal"]
    cfg, net, sd, lf = build(Z, "r18_equal")
    bt, h0, c0 = make_batch(Z, c["hw"], c["idx"])
    net(to_dev(bt, h0, c0))
    _, net_p, _, _ = build(Z, "r18_equal", shared=False)
    plain = {k: (v if k == "img" else v[:3]) for k, v in bt.items() if k != "img_idx"}       # the 3 distinct images, any 3 queries
    net_p(to_dev(plain, h0[:, :3].contiguous(), c0[:, :3].contiguous()))
    torch.cuda.synchronize()
    a, b = net.state_dict(), net_p.state_dict()
    n = 0
    for k in a:
        if k.endswith("running_mean"):
            np.testing.assert_allclose(a[k].cpu().numpy(), b[k].cpu().numpy(), rtol=1e-4, atol=1e-6, err_msg=k)
            n += 1
        elif k.endswith("running_var"):
            np.testing.assert_allclose(a[k].cpu().numpy(), b[k].cpu().numpy(), rtol=1e-3, atol=1e-6, err_msg=k)
        elif k.endswith("num_batches_tracked"):
            assert int(a[k]) == 1, k
    assert n >= 20
    # frozen BatchNorm: bit-unchanged
    cfg, net, sd, lf = build(Z, "r50_frozen_bn_unequal")
    before = {k: v.clone() for k, v in net.state_dict().items() if "running" in k or k.endswith("num_batches_tracked")}
    c = CASES["r50_frozen_bn_unequal"]
    bt, h0, c0 = make_batch(Z, c["hw"], c["idx"])
    net(to_dev(bt, h0, c0))
    torch.cuda.synchronize()
    after = net.state_dict()
    assert before and all(torch.equal(v, after[k]) for k, v in before.items())


def test_frozen_trunk_has_no_conv0_data_gradient_and_no_trunk_launch(Z):
    c = CASES["r18_unequal"]
    cfg, net, sd, lf = build(Z, "r18_unequal")
    for n, p in net.named_parameters():
        if n.startswith("backbone."):
            p.requires_grad_(False)
    bt, h0, c0 = make_batch(Z, c["hw"], c["idx"])
    inp = to_dev(bt, h0, c0)
    out = net(inp)
    ls = lf(out, inp)
    ls["loss"].backward()
    torch.cuda.synchronize()
    plans = [p for k, p in net._plans.items() if len(k) == 9]
    assert len(plans) == 1
    whats = [w for _, _, w in plans[0].bwd.calls]
    assert any(w.endswith(".shared_bwd") for w in whats), "conv0's feature weight gradient needs the segmented sum"
    assert not any(w == "dgrad:att_reg_box.0.0" for w in whats), whats
    assert not any("backbone" in w for w in whats), whats
    assert plans[0].Fpack.grad is None, "no gradient buffer for the pyramid: nothing upstream of the head is lowered"
    ref, sd64, ref64, ls64 = oracle_pair(c, cfg, sd, bt, h0, c0)
    np.testing.assert_allclose(ls["loss"].item(), ls64["loss"].item(), rtol=2e-4)
    check_grads(net, sd, sd64, only=lambda n: not n.startswith("backbone."))
    assert all(p.grad is None for n, p in net.named_parameters() if n.startswith("backbone."))
    # everything of conv0's feature path frozen as well: no segmented-sum launch at all
    cfg, net, sd, lf = build(Z, "r18_unequal")
    for n, p in net.named_parameters():
        if n.startswith("backbone.") or n == "att_reg_box.0.0.weight":
            p.requires_grad_(False)
    out = net(inp)
    lf(out, inp)["loss"].backward()
    torch.cuda.synchronize()
    whats = [w for k, p in net._plans.items() if len(k) == 9 for _, _, w in p.bwd.calls]
    assert whats and not any(w.endswith(".shared_bwd") for w in whats), whats


def test_deterministic_mode_is_bit_reproducible_and_the_plain_path_is_untouched(Z, monkeypatch):
    from zsgnet_pytorch_amd import ops
    from zsgnet_pytorch_amd._lib import lib
    config, loss, mdl, optim, synth = Z
    saved = dict(ops._TUNE_CACHE)
    monkeypatch.setenv("ZSG_DETERMINISTIC", "1")
    lib.zsg_set_deterministic(1)
    try:
        c = CASES["r18_unequal"]
        cfg, net, sd, lf = build(Z, "r18_unequal")
        opt = optim.FusedAdam(net, lr=1e-3)
        bt, h0, c0 = make_batch(Z, c["hw"], c["idx"])
        shared, plain = to_dev(bt, h0, c0), to_dev(synth.expand_shared(bt), h0, c0)

        def grads(inp):
            opt.zero_grad()
            lf(net(inp), inp)["loss"].backward()
            torch.cuda.synchronize()
            return net.store.grad.clone()
        p0 = grads(plain)
        s0 = grads(shared)
        s1 = grads(shared)
        p1 = grads(plain)
        assert torch.equal(s0, s1), "two identical shared training steps must give bit-identical gradients"
        assert torch.equal(p0, p1), "a plain training step must give the same bits before and after a shared one"
        assert float(s0.abs().max()) > 0
    finally:
        lib.zsg_set_deterministic(0)
        ops._TUNE_CACHE.clear()
        ops._TUNE_CACHE.update(saved)


def test_adam_steps_and_plan_cache(Z):
    config, loss, mdl, optim, synth = Z
    c = CASES["r18_equal"]
    cfg, net, sd, lf = build(Z, "r18_equal")
    opt = optim.FusedAdam(net, lr=1e-4, betas=(0.9, 0.99))
    bt, h0, c0 = make_batch(Z, c["hw"], c["idx"])
    inp = to_dev(bt, h0, c0)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        ls = lf(net(inp), inp)["loss"]
        ls.backward()
        opt.step()
        losses.append(float(ls))
    assert all(np.isfinite(losses)), losses
    keys = [k for k in net._plans if len(k) == 9]
    assert len(keys) == 1 and keys[0][0] == 3 and keys[0][7] == ("shared", 6) and keys[0][3] == 20, keys
    # the other query-length bucket: a second plan of the same (Bi, Q)
    bt50, _, _ = make_batch(Z, c["hw"], c["idx"])
    bt50["qvec"] = torch.cat([bt50["qvec"], torch.zeros(6, 10, 300)], 1)
    opt.zero_grad()
    lf(net(to_dev(bt50, h0, c0)), inp)["loss"].backward()
    assert sorted(k[3] for k in net._plans if len(k) == 9) == [20, 50]
    # a new (Bi, Q) leaves none of the old
    bt2, h2, c2 = make_batch(Z, c["hw"], [0, 1, 1, 0])
    inp2 = to_dev(bt2, h2, c2)
    opt.zero_grad()
    ls = lf(net(inp2), inp2)["loss"]
    ls.backward()
    opt.step()
    torch.cuda.synchronize()
    keys = [k for k in net._plans if len(k) == 9]
    assert len(keys) == 1 and keys[0][0] == 2 and keys[0][7] == ("shared", 4), keys
    assert np.isfinite(float(ls))
    # a batch whose image count does not match its plan's slots cannot happen (the plan is keyed on it); a stale index length is refused
    bad = dict(inp2)
    bad["img_idx"] = bad["img_idx"][:3]
    with pytest.raises(ValueError):
        net(bad)


def test_without_the_opt_in_a_training_batch_with_img_idx_is_refused(Z):
    cfg, net, sd, lf = build(Z, "r18_equal", shared=False)
    c = CASES["r18_equal"]
    bt, h0, c0 = make_batch(Z, c["hw"], c["idx"])
    with pytest.raises(RuntimeError, match="eval-only"):
        net(to_dev(bt, h0, c0))
    net.shared_training(True)
    net(to_dev(bt, h0, c0))
    net.shared_training(False)
    with pytest.raises(RuntimeError, match="eval-only"):
        net(to_dev(bt, h0, c0))
    # eval mode keeps the forward-only plan and its error on backward()
    net.shared_training(True).eval()
    out = net(to_dev(bt, h0, c0))
    if out["att_bbx_out"].requires_grad:
        with pytest.raises(RuntimeError, match="eval-only"):
            out["att_bbx_out"].sum().backward()
