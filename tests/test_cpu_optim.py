"""optim.make_opt_fn and the fused optimizer classes on the host (no GPU): cfg opt_fn / opt_fn_params reach the optimizer, the three
rules give the three classes, bad combinations are ValueErrors, state buffers exist only where the rule needs them, checkpoints carry
the rule's name and are refused by another rule, and the C ABI binding lists the general entry points."""
import pytest
import torch

from zsgnet_pytorch_amd import _lib, ema, mdl, optim
from zsgnet_pytorch_amd.config import get_cfg, update_from_dict


@pytest.fixture(scope="module")
def net():
    return mdl.get_default_net(9, get_cfg(resnet_arch="resnet18"))


def test_default_cfg_builds_the_reference_adam(net):
    opt = optim.make_opt_fn(get_cfg())(net, lr=3e-4)
    assert type(opt) is optim.FusedAdam and not opt.amsgrad and opt.vmax is None
    g = opt.param_groups[0]
    assert (g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]) == (3e-4, (0.9, 0.99), 1e-8, 0.0)
    assert set(g) >= {"lr", "betas", "eps", "weight_decay", "params"} and "amsgrad" not in g
    assert set(opt.state_dict()["zsg"]) == {"m", "v", "step", "steps"}
    assert isinstance(opt, optim.FusedOptimizer) and isinstance(opt, torch.optim.Optimizer)


def test_each_opt_fn_gives_its_class_with_the_params_applied(net):
    cfg = get_cfg(opt_fn="AdamW")
    update_from_dict(cfg, {"opt_fn_params.weight_decay": "0.05", "opt_fn_params.amsgrad": "True", "opt_fn_params.betas": "[0.8, 0.95]",
                           "opt_fn_params.eps": "1e-6", "opt_fn_params.momentum": "0.9"})          # (momentum: not AdamW's, ignored)
    opt = optim.make_opt_fn(cfg)(net, lr=1e-3)
    assert type(opt) is optim.FusedAdamW and opt.amsgrad and opt.vmax is not None and opt.vmax.shape == net.store.flat.shape
    g = opt.param_groups[0]
    assert (g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]) == (1e-3, (0.8, 0.95), 1e-6, 0.05)
    assert set(opt.state_dict()["zsg"]) == {"algo", "m", "v", "vmax", "step", "steps"} and opt.state_dict()["zsg"]["algo"] == "AdamW with amsgrad"

    cfg = get_cfg(opt_fn="SGD")
    update_from_dict(cfg, {"opt_fn_params.momentum": "0.9", "opt_fn_params.nesterov": "True", "opt_fn_params.weight_decay": "1e-4",
                           "opt_fn_params.eps": "1e-3"})                                            # (eps: not SGD's, ignored)
    opt = optim.make_opt_fn(cfg)(net, lr=1e-2, params=list(net.parameters()))
    assert type(opt) is optim.FusedSGD
    g = opt.param_groups[0]
    assert (g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"]) == (1e-2, 0.9, 0.0, 1e-4, True)
    assert opt.momentum_buffer is not None and set(opt.state_dict()["zsg"]) == {"algo", "momentum_buffer", "step", "steps"}

    cfg = get_cfg(opt_fn="Adam")
    update_from_dict(cfg, {"opt_fn_params.amsgrad": "True"})
    opt = optim.make_opt_fn(cfg)(net, lr=1e-3)
    assert type(opt) is optim.FusedAdam and opt.amsgrad and opt.state_dict()["zsg"]["algo"] == "Adam with amsgrad"
    # the defaults of the new classes are torch's
    w = optim.FusedAdamW(net)
    assert w.defaults == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2) and not w.amsgrad
    assert optim.FusedSGD(net).defaults == dict(lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False)


def test_bad_combinations_are_value_errors(net):
    with pytest.raises(ValueError, match="Adam, AdamW, SGD"):
        optim.make_opt_fn(get_cfg(opt_fn="RMSprop"))
    cfg = get_cfg(opt_fn="SGD")
    update_from_dict(cfg, {"opt_fn_params.amsgrad": "True"})
    with pytest.raises(ValueError, match="amsgrad"):
        optim.make_opt_fn(cfg)
    cfg = get_cfg(opt_fn="SGD")
    update_from_dict(cfg, {"opt_fn_params.betas": "[0.9, 0.999]"})
    with pytest.raises(ValueError, match="betas"):
        optim.make_opt_fn(cfg)
    cfg = get_cfg(opt_fn="SGD")
    update_from_dict(cfg, {"opt_fn_params.nesterov": "True"})
    with pytest.raises(ValueError, match="Nesterov momentum requires a momentum and zero dampening"):
        optim.make_opt_fn(cfg)
    with pytest.raises(ValueError, match="Nesterov momentum requires a momentum and zero dampening"):
        optim.FusedSGD(net, lr=1e-2, nesterov=True)
    with pytest.raises(ValueError, match="Nesterov momentum requires a momentum and zero dampening"):
        optim.FusedSGD(net, lr=1e-2, momentum=0.9, dampening=0.1, nesterov=True)
    ps = list(net.parameters())
    with pytest.raises(ValueError, match="Nesterov"):          # per group, as torch checks it
        optim.FusedSGD(net, lr=1e-2, momentum=0.9, params=[dict(params=ps[:2]), dict(params=ps[2:], nesterov=True, dampening=0.5)])
    with pytest.raises(ValueError, match="one update rule"):
        optim.FusedAdam(net, params=[dict(params=ps[:2]), dict(params=ps[2:], amsgrad=True)])
    with pytest.raises(AssertionError):                          # an unknown key is still refused by the configuration itself
        update_from_dict(get_cfg(), {"opt_fn_params.rho": "0.9"})


def test_state_buffers_exist_only_where_the_rule_needs_them(net):
    n = net.store.flat.numel()
    a = optim.FusedAdam(net, lr=1e-4)
    assert a.m.numel() == a.v.numel() == n and a.vmax is None and list(a._buffers()) == ["m", "v"]
    assert optim.FusedAdam(net, amsgrad=True).vmax.numel() == n
    assert optim.FusedAdamW(net).vmax is None and list(optim.FusedAdamW(net, amsgrad=True)._buffers()) == ["m", "v", "vmax"]
    plain = optim.FusedSGD(net, lr=1e-2, weight_decay=1e-4)
    assert plain.momentum_buffer is None and plain._buffers() == {} and plain._state_ptrs() == [None, None, None]
    assert set(plain.state_dict()["zsg"]) == {"algo", "step", "steps"}
    ps = list(net.parameters())
    grouped = optim.FusedSGD(net, lr=1e-2, params=[dict(params=ps[:3]), dict(params=ps[3:], momentum=0.8, lr=1e-3)])
    assert grouped.momentum_buffer is not None and grouped.momentum_buffer.numel() == n
    assert [g["momentum"] for g in grouped.param_groups] == [0.0, 0.8]
    # a momentum set later (a group added, a schedule) gets its buffer at the next use
    plain.param_groups[0]["momentum"] = 0.9
    assert list(plain._buffers()) == ["momentum_buffer"] and not bool(plain.momentum_buffer.any())
    # the hyperparameter set that travels to the kernel
    g = grouped._group(grouped.param_groups[1])
    assert (g.lr, g.momentum, g.dampening, g.nesterov) == (pytest.approx(1e-3), pytest.approx(0.8), 0.0, 0)


def test_checkpoints_carry_the_rule_and_another_rule_refuses_them(net):
    sgd = optim.FusedSGD(net, lr=1e-2, momentum=0.9)
    sgd.momentum_buffer.normal_()
    sgd.step_count.fill_(7)
    sgd.param_groups[0]["lr"] = 2e-3
    sd = sgd.state_dict()
    fresh = optim.FusedSGD(net, lr=1e-2)          # (no momentum of its own: the saved group brings it, and with it the buffer)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.momentum_buffer, sgd.momentum_buffer) and int(fresh.step_count) == 7
    assert fresh.param_groups[0]["lr"] == 2e-3 and fresh.param_groups[0]["momentum"] == 0.9
    adam = optim.FusedAdam(net, lr=1e-4)
    with pytest.raises(ValueError, match="SGD.*Adam"):
        adam.load_state_dict(sd)
    with pytest.raises(ValueError, match="Adam.*SGD"):
        sgd.load_state_dict(adam.state_dict())
    with pytest.raises(ValueError, match="Adam, this optimizer is AdamW"):
        optim.FusedAdamW(net).load_state_dict(adam.state_dict())
    with pytest.raises(ValueError, match="Adam, this optimizer is Adam with amsgrad"):          # it lacks vmax
        optim.FusedAdam(net, amsgrad=True).load_state_dict(adam.state_dict())
    z = dict(sd, zsg={k: v for k, v in sd["zsg"].items() if k != "momentum_buffer"})
    with pytest.raises(ValueError, match="momentum_buffer"):
        optim.FusedSGD(net, lr=1e-2, momentum=0.9).load_state_dict(z)
    with pytest.raises(ValueError, match="not a FusedSGD state"):
        sgd.load_state_dict(torch.optim.SGD([torch.nn.Parameter(torch.zeros(2))], lr=0.1).state_dict())
    ams = optim.FusedAdamW(net, amsgrad=True)
    ams.vmax.uniform_()
    ams.m.normal_()
    again = optim.FusedAdamW(net, amsgrad=True)
    again.load_state_dict(ams.state_dict())
    assert torch.equal(again.vmax, ams.vmax) and torch.equal(again.m, ams.m)


def test_model_ema_attaches_to_every_fused_optimizer(net):
    avg = ema.ModelEma(net, decay=0.9)
    for opt in (optim.FusedAdamW(net), optim.FusedSGD(net, momentum=0.9), optim.FusedAdam(net, amsgrad=True)):
        avg.attach(opt)
        assert opt._ema is avg
        with pytest.raises(RuntimeError, match="no CPU fallback"):          # the attached step checks before it launches anything
            opt.step()
        avg.detach()
        assert opt._ema is None
    with pytest.raises(ValueError, match="FusedOptimizer"):
        avg.attach(torch.optim.SGD(net.parameters(), lr=0.1))


def test_general_entry_points_are_bound():
    for name in ("zsg_optim_step", "zsg_optim_step_ema", "zsg_optim_step_segments"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert (_lib.OPT_ADAM, _lib.OPT_ADAMW, _lib.OPT_SGD, _lib.OPT_AMSGRAD) == (0, 1, 2, 1)
    import ctypes
    assert ctypes.sizeof(_lib.OptimGroup) == 32 and _lib.OptimGroup.nesterov.offset == 28


def test_learner_init_uses_the_configured_optimizer(tmp_path):
    from zsgnet_pytorch_amd.main_dist import learner_init
    cfg = get_cfg(resnet_arch="resnet18", device="cpu", tmp_path=str(tmp_path), opt_fn="SGD", steps_per_epoch=1, bs=2, bsv=2, resize_img=[96, 96])
    update_from_dict(cfg, {"opt_fn_params.momentum": "0.9"})
    cfg.freeze()
    learn = learner_init("o", cfg)
    learn.prepare_optimizer(1e-2)
    assert type(learn.optimizer) is optim.FusedSGD and learn.optimizer.param_groups[0]["momentum"] == 0.9
    assert learn.lr_scheduler is not None
