"""The LAMB feature on the host (no GPU): tests/lamb_ref.py against a three-element case worked out by hand, its ratio rules, the groups
cfg opt_fn "LAMB" builds (tensors of >= 2 dimensions adaptive, 1-D ones plain and undecayed; cfg lamb_adapt_1d), the warm-up schedule
of cfg warmup_iters and its continuation after a resume, the C ABI binding of csrc/lamb.hip's entry points."""
import ctypes
import math

import numpy as np
import pytest
import torch

import lamb_ref
from zsgnet_pytorch_amd import _lib, mdl, optim
from zsgnet_pytorch_amd.config import get_cfg, update_from_dict


@pytest.fixture(scope="module")
def net():
    return mdl.get_default_net(9, get_cfg(resnet_arch="resnet18"))


def test_reference_matches_a_hand_computed_case():
    """t = 1, beta1 = 1/2, beta2 = 3/4, eps = 0: m = g / 2, v = g^2 / 4, bc1 = 1/2, bc2 = 1/4, so m / bc1 = g and sqrt(v / bc2) = |g| and the
    Adam part of u is sign(g).  With wd = 1/4 and w = (4, -4, 2): u = (1 + 1, -1 - 1, 1 + 1/2) = (2, -2, 3/2), |w| = 6, |u| = sqrt(10.25)."""
    w, g = [4.0, -4.0, 2.0], [2.0, -8.0, 0.5]
    w1, m1, v1, info = lamb_ref.lamb_step(w, g, [0, 0, 0], [0, 0, 0], t=1, lr=0.5, beta1=0.5, beta2=0.75, eps=0.0, wd=0.25)
    assert m1.dtype == v1.dtype == w1.dtype == np.float32
    assert m1.tolist() == [1.0, -4.0, 0.25] and v1.tolist() == [1.0, 16.0, 0.0625]
    assert info["u"].tolist() == [2.0, -2.0, 1.5]
    assert float(info["norm_w"]) == 6.0 and float(info["norm_u"]) == pytest.approx(math.sqrt(10.25), rel=1e-7)
    r = 6.0 / math.sqrt(10.25)
    assert float(info["ratio"]) == pytest.approx(r, rel=2e-7)
    assert w1.tolist() == pytest.approx([4.0 - 0.5 * r * 2.0, -4.0 + 0.5 * r * 2.0, 2.0 - 0.5 * r * 1.5], rel=5e-7)
    # the second step of the same tensor uses t = 2: bc1 = 1 - 1/4, bc2 = 1 - 9/16
    assert float(lamb_ref.bias_correction(0.5, 2)) == 0.75 and float(lamb_ref.bias_correction(0.75, 2)) == 0.4375
    w2, m2, v2, _ = lamb_ref.lamb_step(w1, [0.0, 0.0, 0.0], m1, v1, t=2, lr=0.5, beta1=0.5, beta2=0.75, eps=0.0, wd=0.0)
    assert m2.tolist() == [0.5, -2.0, 0.125] and v2.tolist() == [0.75, 12.0, 0.046875]
    # grad_scale multiplies the gradient first
    _, ms, _, _ = lamb_ref.lamb_step(w, g, [0, 0, 0], [0, 0, 0], t=1, lr=0.5, beta1=0.5, beta2=0.75, eps=0.0, wd=0.25, grad_scale=0.5)
    assert ms.tolist() == [0.5, -2.0, 0.125]


def test_adapt_false_gives_ratio_one():
    w, g = [4.0, -4.0, 2.0], [2.0, -8.0, 0.5]
    w1, _, _, info = lamb_ref.lamb_step(w, g, [0, 0, 0], [0, 0, 0], t=1, lr=0.5, beta1=0.5, beta2=0.75, eps=0.0, wd=0.25, adapt=False)
    assert float(info["ratio"]) == 1.0 and float(info["norm_w"]) == 6.0
    assert w1.tolist() == [4.0 - 0.5 * 2.0, -4.0 + 0.5 * 2.0, 2.0 - 0.5 * 1.5]          # the Adam step itself


def test_zero_weights_or_zero_gradients_give_ratio_one_and_nan_propagates():
    z = np.zeros(5, np.float32)
    g = np.array([1, -2, 3, 0.5, 4], np.float32)
    w1, m1, v1, info = lamb_ref.lamb_step(z, z, z, z, t=1, lr=0.1, beta1=0.9, beta2=0.99, eps=1e-6, wd=0.01)
    assert float(info["ratio"]) == 1.0 and float(info["norm_w"]) == 0.0 and float(info["norm_u"]) == 0.0
    assert not w1.any() and not m1.any() and not v1.any(), "the store's padding (w = g = 0) stays 0"
    _, _, _, info = lamb_ref.lamb_step(z, g, z, z, t=1, lr=0.1, beta1=0.9, beta2=0.99, eps=1e-6, wd=0.01)
    assert float(info["ratio"]) == 1.0 and float(info["norm_u"]) > 0, "w = 0: nothing to scale by"
    w1, _, _, info = lamb_ref.lamb_step(g, z, z, z, t=1, lr=0.1, beta1=0.9, beta2=0.99, eps=1e-6, wd=0.0)
    assert float(info["ratio"]) == 1.0 and np.array_equal(w1, g), "g = 0 at t = 1 without decay: u = 0, w keeps its bits"
    bad = g.copy()
    bad[2] = np.nan
    w1, _, _, info = lamb_ref.lamb_step(g, bad, z, z, t=1, lr=0.1, beta1=0.9, beta2=0.99, eps=1e-6, wd=0.0)
    assert np.isnan(info["ratio"]) and np.isnan(w1).all()
    assert np.isnan(lamb_ref.trust_ratio(np.nan, 1.0)) and float(lamb_ref.trust_ratio(np.nan, 1.0, adapt=False)) == 1.0


def test_opt_fn_lamb_no_longer_raises_and_groups_by_dimension(net):
    cfg = get_cfg(opt_fn="LAMB")
    update_from_dict(cfg, {"opt_fn_params.betas": "[0.9, 0.999]", "opt_fn_params.eps": "1e-6", "opt_fn_params.weight_decay": "0.01",
                           "opt_fn_params.momentum": "0.9"})          # (momentum: not LAMB's, ignored)
    opt = optim.make_opt_fn(cfg)(net, lr=2e-3)
    assert type(opt) is optim.FusedLAMB and isinstance(opt, optim.FusedOptimizer) and optim.FusedLAMB.NAME == "LAMB"
    many, one = opt.param_groups
    assert many["params"] and all(p.dim() >= 2 for p in many["params"]) and one["params"] and all(p.dim() == 1 for p in one["params"])
    assert len(many["params"]) + len(one["params"]) == len(list(net.parameters()))
    assert (many["lr"], tuple(many["betas"]), many["eps"], many["weight_decay"], many["adapt"]) == (2e-3, (0.9, 0.999), 1e-6, 0.01, True)
    assert (one["lr"], tuple(one["betas"]), one["eps"], one["weight_decay"], one["adapt"]) == (2e-3, (0.9, 0.999), 1e-6, 0.0, False)
    g = opt._group(one)
    assert (g.lr, g.eps, g.weight_decay, g.adapt) == (pytest.approx(2e-3), pytest.approx(1e-6), 0.0, 0) and opt._group(many).adapt == 1
    # every step is segmented: there is never a single-launch selection, with or without gradients
    assert opt._stepped() == ()
    # cfg lamb_adapt_1d: one adaptive group of everything
    opt = optim.make_opt_fn(get_cfg(opt_fn="LAMB", lamb_adapt_1d=True))(net, lr=1e-3)
    assert len(opt.param_groups) == 1 and opt.param_groups[0]["adapt"] is True and len(opt.param_groups[0]["params"]) == len(list(net.parameters()))
    assert tuple(opt.param_groups[0]["betas"]) == (0.9, 0.99) and opt.param_groups[0]["eps"] == 1e-8          # opt_fn_params' defaults
    # the trainer's own params= are taken as they are
    ps = list(net.parameters())
    opt = optim.make_opt_fn(get_cfg(opt_fn="LAMB"))(net, lr=1e-3, params=[dict(params=ps[:3], adapt=False), dict(params=ps[3:], lr=5e-4)])
    assert [len(g["params"]) for g in opt.param_groups] == [3, len(ps) - 3] and [g["adapt"] for g in opt.param_groups] == [False, True]
    assert [len(g["params"]) for g in optim.lamb_param_groups([torch.zeros(3), torch.zeros(2, 2), torch.zeros(1, 1, 1, 1)])] == [2, 1]
    assert len(optim.lamb_param_groups([torch.zeros(2, 2)])) == 1          # (no empty group)
    with pytest.raises(ValueError, match="Adam, AdamW, SGD, LAMB"):
        optim.make_opt_fn(get_cfg(opt_fn="LARS"))


def test_lamb_state_and_checkpoint_frame(net):
    lamb = optim.FusedLAMB(net)
    assert lamb.defaults == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, adapt=True)
    assert list(lamb._buffers()) == ["m", "v"] and lamb.m.numel() == lamb.v.numel() == net.store.flat.numel()
    sd = lamb.state_dict()
    assert sd["zsg"]["algo"] == "LAMB" and set(sd["zsg"]) == {"algo", "m", "v", "step", "steps"}
    lamb.m.normal_()
    lamb.param_groups[0]["lr"], lamb.param_groups[0]["adapt"] = 3e-4, False
    again = optim.FusedLAMB(net)
    again.load_state_dict(lamb.state_dict())
    assert torch.equal(again.m, lamb.m) and again.param_groups[0]["lr"] == 3e-4 and again.param_groups[0]["adapt"] is False
    adam = optim.FusedAdam(net)
    with pytest.raises(ValueError, match="belongs to Adam, this optimizer is LAMB"):
        again.load_state_dict(adam.state_dict())
    with pytest.raises(ValueError, match="belongs to LAMB, this optimizer is Adam"):
        adam.load_state_dict(sd)
    n = len(list(net.parameters()))
    assert lamb.trust_ratios().tolist() == [1.0] * n, "before the first step"


def test_lamb_entry_points_are_bound():
    for name in ("zsg_lamb_moments", "zsg_lamb_apply"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert len(_lib.SIGNATURES["zsg_lamb_moments"][1]) == 17 and len(_lib.SIGNATURES["zsg_lamb_apply"][1]) == 12
    assert ctypes.sizeof(_lib.LambGroup) == 24 and _lib.LambGroup.adapt.offset == 20 and _lib.LambGroup.weight_decay.offset == 16


def _learner(tmp_path, **kw):
    from zsgnet_pytorch_amd.main_dist import learner_init
    cfg = get_cfg(resnet_arch="resnet18", device="cpu", tmp_path=str(tmp_path), steps_per_epoch=1, bs=2, bsv=2, resize_img=[96, 96], **kw)
    cfg.freeze()
    return learner_init("w", cfg)


def _lrs(learn):
    return [g["lr"] for g in learn.optimizer.param_groups]


def test_warmup_schedule_and_its_continuation_after_a_resume(tmp_path):
    base, W = 8e-3, 4
    learn = _learner(tmp_path, opt_fn="LAMB", warmup_iters=W)
    learn.prepare_optimizer(base)
    assert len(learn.optimizer.param_groups) == 2 and _lrs(learn) == [base, base]
    seen = []
    for k in range(1, 7):          # what train_epoch does around every step
        learn.num_it = k
        learn._warmup_lr()
        seen.append(_lrs(learn))
        if k == 5:                 # a scheduler's cut behind the warm-up stays
            for g in learn.optimizer.param_groups:
                g["lr"] *= 0.1
    assert seen[:5] == [[base * k / W] * 2 for k in (1, 2, 3, 4, 4)] and seen[3] == [base, base]
    assert seen[5] == [base * 0.1] * 2
    # per-group base rates, and a cut DURING the warm-up moves the base with it
    learn = _learner(tmp_path, opt_fn="Adam", warmup_iters=W)
    ps = list(learn.mdl.parameters())
    learn.prepare_optimizer(base, params=[dict(params=ps[:2]), dict(params=ps[2:], lr=base / 2)])
    out = []
    for k in range(1, 6):
        learn.num_it = k
        learn._warmup_lr()
        out.append(_lrs(learn))
        if k == 2:
            learn.optimizer.param_groups[0]["lr"] *= 0.5
    assert out[1] == [base * 2 / W, base / 2 * 2 / W]
    assert out[2] == pytest.approx([base * 0.5 * 3 / W, base / 2 * 3 / W]) and out[4] == pytest.approx([base * 0.5, base / 2])
    # warmup_iters = 0: the groups are never touched
    off = _learner(tmp_path, opt_fn="LAMB")
    off.prepare_optimizer(base)
    off.num_it = 1
    off._warmup_lr()
    assert _lrs(off) == [base, base]
    # a resume with load_opt continues from the checkpoint's num_it; one without starts the fresh optimizer's warm-up over
    learn = _learner(tmp_path / "r", opt_fn="LAMB", warmup_iters=W, lr=base)
    learn.prepare_optimizer(base)
    for k in (1, 2):
        learn.num_it = k
        learn._warmup_lr()
    learn.save_model_dict()
    again = _learner(tmp_path / "r", opt_fn="LAMB", warmup_iters=W, lr=base, load_opt=True)
    assert again.num_it == 2 and _lrs(again) == [base * 2 / W] * 2, "the saved (warming) rate comes back with the groups"
    cont = []
    for k in (3, 4, 5):
        again.num_it = k
        again._warmup_lr()
        cont.append(_lrs(again)[0])
    assert cont == [base * 3 / W, base, base]
    fresh = _learner(tmp_path / "r", opt_fn="LAMB", warmup_iters=W, lr=base)
    assert fresh.num_it == 2 and fresh.optimizer is None
    fresh.prepare_optimizer(base)
    fresh.num_it = 3
    fresh._warmup_lr()
    assert _lrs(fresh) == [base * 1 / W] * 2
