"""Fine-tuning a subset: parameters with requires_grad=False get no gradient, no p.grad, no weight-gradient, data-gradient
or BatchNorm-backward launch upstream of every trainable parameter, and FusedAdam never steps them; parameter groups, late bias correction
after unfreezing and the optimizer state round trip match torch.optim.Adam.  ResNet-18, 96 px, B = 2 (as test_gpu_net.py)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import zsg_oracle as O  # noqa: E402

RATIOS, SCALES = O.default_ratios_scales()
ENC = "backbone.encoder."
STEM_L1 = (ENC + "conv1.", ENC + "bn1.", ENC + "layer1.")


@pytest.fixture(scope="module")
def Z():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib, config, loss, mdl, optim
    return _lib, config, loss, mdl, optim


def build(Z, seed=11):
    _lib, config, loss, mdl, optim = Z
    cfg = config.get_cfg(resnet_arch="resnet18")
    net = mdl.get_default_net(9, cfg)
    sd = O.seeded_state_dict("resnet18", seed)
    net.load_state_dict(sd)
    net.to("cuda").train()
    r, s = config.ratios_scales(cfg)
    return net, sd, loss.get_default_loss(r, s, cfg)


def batch(B=2, hw=96, seed=5):
    bt = O.synthetic_batch(B, hw, hw + 32, seed=seed, tmax=13)
    gq = torch.Generator().manual_seed(2)
    h0, c0 = torch.randn(2, B, 128, generator=gq), torch.randn(2, B, 128, generator=gq)
    inp = {k: v.cuda() for k, v in bt.items()}
    inp["h0"], inp["c0"] = h0, c0
    return bt, inp, h0, c0


def freeze(net, prefixes):
    for n, p in net.named_parameters():
        p.requires_grad_(not n.startswith(prefixes))


def train_plan(net):
    plans = [p for k, p in net._plans.items() if k[-1]]
    assert len(plans) == 1, "one training plan per trainable set: the old set's plans are dropped"
    return plans[0]


def backward(net, lf, inp):
    out = net(inp)
    lf(out, inp)["loss"].backward()
    torch.cuda.synchronize()
    return out


class deterministic:
    """ZSG_DETERMINISTIC=1 for the plans lowered inside (the tuner offers no atomic split-K) and the library's reductions"""
    def __init__(self, L):
        self.L = L

    def __enter__(self):
        self.old = os.environ.get("ZSG_DETERMINISTIC")
        os.environ["ZSG_DETERMINISTIC"] = "1"
        self.L.lib.zsg_set_deterministic(1)

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("ZSG_DETERMINISTIC", None)
        else:
            os.environ["ZSG_DETERMINISTIC"] = self.old
        self.L.lib.zsg_set_deterministic(1 if self.old == "1" else 0)


@pytest.mark.parametrize("prefixes", [(ENC,), STEM_L1], ids=["encoder", "stem_layer1"])
def test_frozen_subset_grads_program_and_steps(Z, prefixes):
    L, config, loss, mdl, optim = Z
    net, sd, lf = build(Z)
    bt, inp, h0, c0 = batch()
    with deterministic(L):
        backward(net, lf, inp)
        full = train_plan(net)
        n_full = len(full.bwd.calls)
        n_sub = sum(1 for w in (c[2] for c in full.bwd.calls) if any(p[:-1] in w for p in prefixes))
        g_full = {n: p.grad.clone() for n, p in net.named_parameters()}
        freeze(net, prefixes)
        net.zero_grad(set_to_none=True)
        backward(net, lf, inp)
    plan = train_plan(net)
    assert plan is not full
    frozen = [n for n, p in net.named_parameters() if n.startswith(prefixes)]
    trainable = [n for n, p in net.named_parameters() if not n.startswith(prefixes)]
    assert frozen and all(p.grad is None for n, p in net.named_parameters() if n in frozen)
    # the backward program holds nothing of the frozen part
    leaked = [w for _, _, w in plan.bwd.calls if w.startswith(("wgrad", "bgrad", "dgrad", "bnbwd")) and any(p[:-1] in w for p in prefixes)]
    assert not leaked, leaked
    assert n_sub > 0 and len(plan.bwd.calls) <= n_full - n_sub, (len(plan.bwd.calls), n_full, n_sub)
    assert not set(plan.grad_ready) & set(frozen)
    # the trainable gradients are the ones of the unfrozen network, bit for bit (deterministic reductions in both)
    differ = [n for n in trainable if not torch.equal(dict(net.named_parameters())[n].grad, g_full[n])]
    assert not differ, differ
    # ... and the fp64 oracle's, with requires_grad on the trainable tensors only
    for k, v in sd.items():
        if v.is_floating_point() and k in trainable:
            v.requires_grad_()
    ref = O.zsgnet_forward(sd, bt, h0, c0, arch="resnet18")
    fs = [tuple(r) for r in ref["feat_sizes"].tolist()]
    anc = torch.from_numpy(O.create_anchors(fs, RATIOS, SCALES).astype(np.float32))
    O.torch_loss(ref, bt["annot"], anc)["loss"].backward()
    sd64 = {k: (v.detach().double().requires_grad_(v.requires_grad) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    ref64 = O.zsgnet_forward(sd64, {k: v.double() for k, v in bt.items()}, h0.double(), c0.double(), arch="resnet18", rank=O.sort_rank(bt["qlens"]))
    O.torch_loss(ref64, bt["annot"], anc)["loss"].backward()
    assert all(sd64[n].grad is None for n in frozen)
    bad = []
    for n in trainable:
        g64 = sd64[n].grad.flatten()
        e = float((dict(net.named_parameters())[n].grad.cpu().double().flatten() - g64).norm())
        ec = float((sd[n].grad.double().flatten() - g64).norm())
        if e > max(6 * ec + 2e-4 * float(g64.norm()), 1.5e-2 * float(g64.norm())) + 1e-9:       # test_gpu_net.grad_tol
            bad.append((n, e / (float(g64.norm()) + 1e-30)))
    assert not bad, bad[:8]
    # three optimizer steps: the frozen parameters and their moments do not move
    w0 = {n: p.detach().clone() for n, p in net.named_parameters()}
    opt = optim.FusedAdam(net, lr=1e-3, weight_decay=1e-2)
    for it in range(3):
        opt.zero_grad()
        backward(net, lf, inp)
        opt.step()
    torch.cuda.synchronize()
    ps = dict(net.named_parameters())
    assert all(torch.equal(ps[n].detach(), w0[n]) and ps[n].grad is None for n in frozen)
    assert all(not torch.equal(ps[n].detach(), w0[n]) for n in trainable if n.endswith(".weight"))
    assert all(not bool(net.store.view(n, opt.m).any()) for n in frozen)


def test_all_frozen_backward_records_no_launches(Z):
    L, config, loss, mdl, optim = Z
    net, sd, lf = build(Z)
    _, inp, _, _ = batch()
    for p in net.parameters():
        p.requires_grad_(False)
    out = net(inp)
    lf(out, inp)["loss"].backward()
    torch.cuda.synchronize()
    plan = train_plan(net)
    assert len(plan.bwd.calls) == 0 and not plan.grad_ready
    assert all(p.grad is None for p in net.parameters())
    # encoder + LSTM frozen: the query encoder's backward is gone, the head's language columns stay
    freeze(net, (ENC, "lstm."))
    net.zero_grad(set_to_none=True)
    backward(net, lf, inp)
    ws = [w for _, _, w in train_plan(net).bwd.calls]
    assert not [w for w in ws if "lstm" in w or "w_ih" in w or "w_hh" in w or w.startswith("dwe:") or ENC in w], ws
    assert "wgrad:att_reg_box.0.0.lang" in ws


def _torch_twin(net, groups_spec):
    """GPU copies of the parameters in torch.optim.Adam with the same groups"""
    names = [n for n, _ in net.named_parameters()]
    twins = {n: torch.nn.Parameter(p.detach().clone()) for n, p in net.named_parameters()}
    groups = [dict(g, params=[twins[n] for n in names if sel(n)]) for sel, g in groups_spec]
    return twins, groups


def _feed(net, twins):
    for n, p in net.named_parameters():
        twins[n].grad = None if p.grad is None else p.grad.detach().clone()


def _check_twin(net, opt, twins, topt, what):
    for n, p in net.named_parameters():
        torch.testing.assert_close(p.detach(), twins[n].detach(), rtol=1e-5, atol=1e-6, msg=f"{what}: {n}")
        st = topt.state.get(twins[n])
        if st:
            # (torch updates exp_avg with lerp, the kernel as b1 * m + (1 - b1) * g: a few ulp apart, relative to the largest moment)
            for mine, ref, k in ((net.store.view(n, opt.m), st["exp_avg"], "exp_avg"), (net.store.view(n, opt.v), st["exp_avg_sq"], "exp_avg_sq")):
                err = float((mine - ref).abs().max())
                assert err <= 1e-5 * float(ref.abs().max()) + 1e-12, f"{what}: {k} of {n} off by {err:.3g} (max {float(ref.abs().max()):.3g})"
        else:
            assert not bool(net.store.view(n, opt.m).any()), f"{what}: {n} has moments but was never stepped"


def test_unfreezing_matches_torch_adam_with_late_bias_correction(Z):
    L, config, loss, mdl, optim = Z
    net, sd, lf = build(Z, seed=12)
    _, inp, _, _ = batch(seed=6)
    opt = optim.FusedAdam(net, lr=1e-3, betas=(0.9, 0.99))
    twins, groups = _torch_twin(net, [(lambda n: True, dict(lr=1e-3, betas=(0.9, 0.99)))])
    topt = torch.optim.Adam(groups)
    freeze(net, (ENC,))
    for it in range(4):
        if it == 2:
            first = train_plan(net)
            freeze(net, ())                     # unfreeze everything
        opt.zero_grad()
        backward(net, lf, inp)
        _feed(net, twins)
        opt.step()
        topt.step()
    torch.cuda.synchronize()
    assert train_plan(net) is not first
    steps = opt.param_steps().tolist()
    names = [n for n, _ in net.named_parameters()]
    assert [s for n, s in zip(names, steps)] == [2 if n.startswith(ENC) else 4 for n in names]
    assert all(int(topt.state[twins[n]]["step"]) == s for n, s in zip(names, steps))
    _check_twin(net, opt, twins, topt, "unfreeze")


def test_param_groups_with_plateau_scheduler_and_state_round_trip(Z):
    L, config, loss, mdl, optim = Z
    net, sd, lf = build(Z, seed=13)
    _, inp, _, _ = batch(seed=7)
    freeze(net, STEM_L1)
    head = lambda n: not n.startswith(ENC)                  # noqa: E731
    body = lambda n: n.startswith(ENC) and not n.startswith(STEM_L1)      # noqa: E731
    spec = [(head, dict(lr=1e-3, weight_decay=1e-2)), (body, dict(lr=2e-4, weight_decay=0.0))]
    ps = dict(net.named_parameters())
    opt = optim.FusedAdam(net, lr=5e-4, betas=(0.9, 0.99), params=[dict(g, params=[p for n, p in ps.items() if sel(n)]) for sel, g in spec])
    twins, groups = _torch_twin(net, spec)
    topt = torch.optim.Adam(groups, lr=5e-4, betas=(0.9, 0.99))
    # the plateau scheduler lowers the head group only (the body's lr is its floor already)
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=0.5, patience=0, min_lr=[0.0, 2e-4])
    tsch = torch.optim.lr_scheduler.ReduceLROnPlateau(topt, factor=0.5, patience=0, min_lr=[0.0, 2e-4])
    for it in range(3):
        opt.zero_grad()
        backward(net, lf, inp)
        _feed(net, twins)
        opt.step()
        topt.step()
        sch.step(1.0)
        tsch.step(1.0)
    torch.cuda.synchronize()
    assert opt.param_groups[0]["lr"] < 1e-3 and opt.param_groups[1]["lr"] == 2e-4
    _check_twin(net, opt, twins, topt, "groups")
    with pytest.raises(ValueError, match="not a parameter"):
        opt.add_param_group(dict(params=[torch.nn.Parameter(torch.zeros(3, device="cuda"))]))
    # round trip: a fresh optimizer loaded from the state continues bit for bit
    state = {k: v for k, v in opt.state_dict().items()}
    state["zsg"] = {k: v.clone() for k, v in state["zsg"].items()}
    w = net.store.flat.clone()
    opt.step()
    ref = net.store.flat.clone()
    net.store.flat.copy_(w)
    opt2 = optim.FusedAdam(net, lr=1.0, params=[dict(params=[p for n, p in ps.items() if sel(n)]) for sel, _ in spec])
    opt2.load_state_dict(state)
    assert [g["lr"] for g in opt2.param_groups] == [g["lr"] for g in opt.param_groups]
    opt2.step()
    torch.cuda.synchronize()
    assert torch.equal(net.store.flat.view(torch.int32), ref.view(torch.int32))
