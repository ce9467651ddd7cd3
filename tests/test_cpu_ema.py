"""Weight EMA on the host side (no GPU): the config keys, the decay schedule, ModelEma's checkpoint views on a CPU network, and the
argument checks that run before anything is launched.  The error bound of tests/ema_ref.py is checked here on the CPU too, on torch.lerp
and on the unfused expression."""
import pytest
import torch

import ema_ref


def _net():
    from zsgnet_pytorch_amd import config, mdl
    return mdl.get_default_net(9, config.get_cfg(resnet_arch="resnet18"))


def test_config_keys_defaults_and_parsing():
    from zsgnet_pytorch_amd import config
    from zsgnet_pytorch_amd.main_dist import parse_argv
    cfg = config.get_cfg()
    assert cfg["ema_decay"] == 0.0 and cfg["ema_warmup"] is False and cfg["ema_eval"] is True
    uid, kw = parse_argv(["run", "--ema_decay=0.999", "--ema_warmup", "--ema_eval=False"])
    cfg = config.update_from_dict(config.get_cfg(), kw)
    assert cfg["ema_decay"] == 0.999 and isinstance(cfg["ema_decay"], float)
    assert cfg["ema_warmup"] is True and cfg["ema_eval"] is False
    assert config.get_cfg(ema_decay=1)["ema_decay"] == 1.0           # an int on the command line is a float
    with pytest.raises(AssertionError):
        config.get_cfg(ema_decay="on")
    with pytest.raises(AssertionError):
        config.get_cfg(ema_warmup=0.5)
    with pytest.raises(AssertionError):
        config.get_cfg(ema_eval="yes")


def test_decay_schedule_hand_values():
    from zsgnet_pytorch_amd import ema
    for f in (ema.decay_at, ema_ref.decay_at):
        assert f(0.999, True, 0) == 0.1
        assert f(0.999, True, 1) == 2.0 / 11.0
        assert f(0.999, True, 90) == 91.0 / 100.0
        assert f(0.999, True, 8991) == 0.999 and f(0.999, True, 10 ** 6) == 0.999
        assert f(0.5, True, 7) == 8.0 / 17.0 and f(0.5, True, 8) == 0.5
        assert all(f(0.9, False, n) == 0.9 for n in (0, 1, 5, 1000))
    # the first update is a copy; later ones use 1 - decay_t rounded to fp32
    assert ema_ref.weight(0.9, False, 0) == 1.0 and ema_ref.weight(0.9, True, 0) == 1.0
    assert ema_ref.weight(0.9, False, 3) == float(torch.tensor(1.0 - 0.9, dtype=torch.float32))


def test_model_ema_counts_updates_as_the_schedule_says():
    from zsgnet_pytorch_amd import ema
    e = ema.ModelEma(_net(), decay=0.9, warmup=True)
    ws = [e._next_weight() for _ in range(12)]
    assert e.n_averaged == 12
    assert ws[0] == 1.0
    assert ws[1:] == [1.0 - min(0.9, (1.0 + n) / (10.0 + n)) for n in range(1, 12)]


@pytest.mark.parametrize("decay", [0.999, 0.9998, 0.9, 0.5, 0.3])
def test_bound_holds_for_fused_and_unfused_fp32_updates(decay):
    g = torch.Generator().manual_seed(int(decay * 1e4))
    e, p = torch.randn(1 << 20, generator=g), torch.randn(1 << 20, generator=g)
    w = ema_ref.weight(decay, False, 1)
    ref, bnd = ema_ref.step64(e, p, w), ema_ref.bound1(e, p)
    ema_ref.assert_within(torch.lerp(e, p, w), ref, bnd, f"torch.lerp decay {decay}")
    ema_ref.assert_within(e + torch.tensor(w) * (p - e), ref, bnd, f"unfused decay {decay}")


def test_state_dict_views_round_trip_and_validation():
    from zsgnet_pytorch_amd import ema, optim
    net = _net()
    net.reset_parameters(seed=3)
    with torch.no_grad():
        net._rmv.copy_(torch.rand(net._rmv.numel()) + 0.5)
        net._nbt.fill_(7)
    avg = ema.ModelEma(net, decay=0.99)
    assert avg.n_averaged == 0 and avg.decay == 0.99 and avg.warmup is False
    nsd, esd = net.state_dict(), avg.state_dict()
    meta = esd.pop(ema.META_KEY)
    assert meta == dict(n_averaged=0, decay=0.99, warmup=False)
    assert list(esd) == list(nsd)
    for k in nsd:
        assert esd[k].shape == nsd[k].shape and esd[k].dtype == nsd[k].dtype, k
        assert torch.equal(esd[k], nsd[k]), k
        assert esd[k].untyped_storage().data_ptr() != nsd[k].untyped_storage().data_ptr(), k          # a copy, not the network's storage
    assert esd["backbone.encoder.layer1.0.conv1.weight"].untyped_storage().data_ptr() == avg.flat.untyped_storage().data_ptr()

    # round trip through another network's average, with and without the extra key; DDP's 'module.' prefix is stripped
    other = ema.ModelEma(_net(), decay=0.5, warmup=True)
    full = avg.state_dict()
    full[ema.META_KEY] = dict(n_averaged=41, decay=0.99, warmup=False)
    other.load_state_dict(full)
    assert (other.n_averaged, other.decay, other.warmup) == (41, 0.99, False)
    for k, v in other.state_dict().items():
        if k != ema.META_KEY:
            assert torch.equal(v, nsd[k]), k
    plain = ema.ModelEma(_net(), decay=0.5, warmup=True)
    plain.load_state_dict({"module." + k: v for k, v in nsd.items()})
    assert (plain.n_averaged, plain.decay, plain.warmup) == (1, 0.5, True)
    assert all(torch.equal(v, nsd[k]) for k, v in plain.state_dict().items() if k != ema.META_KEY)
    # the network itself takes the average as its weights
    fresh = _net()
    fresh.load_state_dict({k: v for k, v in avg.state_dict().items() if k != ema.META_KEY})
    assert all(torch.equal(v, nsd[k]) for k, v in fresh.state_dict().items())
    missing, unexpected = torch.nn.Module.load_state_dict(fresh, avg.state_dict(), strict=False)
    assert not missing and unexpected == [ema.META_KEY]

    bad = {k: v for k, v in nsd.items()}
    del bad["lstm.bias_ih_l0"]
    with pytest.raises(ValueError, match="missing"):
        plain.load_state_dict(bad)
    bad = dict(nsd)
    bad["lstm.bias_ih_l0"] = torch.zeros(3)
    with pytest.raises(ValueError, match="shape"):
        plain.load_state_dict(bad)

    # reset re-copies and restarts the count
    with torch.no_grad():
        net.store.flat.add_(1.0)
    other2 = avg.state_dict()["lstm.bias_ih_l0"].clone()
    avg.n_averaged = 5
    avg.reset()
    assert avg.n_averaged == 0
    assert torch.equal(avg.state_dict()["lstm.bias_ih_l0"], other2 + 1.0)

    for d in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match="decay"):
            ema.ModelEma(net, decay=d)
    with pytest.raises(ValueError, match="ZSGNet"):
        ema.ModelEma(torch.nn.Linear(2, 2))

    # no CPU fallback: whatever would launch raises
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        avg.update()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        with avg.applied():
            pass
    assert avg.n_averaged == 0
    # an optimizer of another network (or no FusedAdam at all) is rejected
    with pytest.raises(ValueError, match="not a FusedAdam of this"):
        avg.attach(optim.FusedAdam(_net(), lr=1e-4))
    with pytest.raises(ValueError, match="not a FusedAdam of this"):
        avg.attach(torch.optim.Adam(net.parameters(), lr=1e-4))
    opt = optim.FusedAdam(net, lr=1e-4)
    avg.attach(opt)
    assert opt._ema is avg
    with pytest.raises(RuntimeError, match="attached"):
        avg.update()
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # the attached step checks before it launches anything
        opt.step()
    assert avg.n_averaged == 0
    avg.detach()
    assert opt._ema is None and avg._opt is None
