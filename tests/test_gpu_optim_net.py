"""optim.FusedAdamW / FusedAdam(amsgrad=True) / FusedSGD on the network (Optimizers): over real training steps each follows
its torch.optim twin (foreach=False, CPU copies of the parameters, fed the network's own gradients) within the tolerances of
tests/test_gpu_adam_segments.py; parameter groups and a frozen FPN take the segmented path, leave what is frozen bit for bit alone and
start a late parameter as torch does; checkpoints continue bit for bit and are refused by another rule; the weight average rides in the one
launch; clip_grad_norm_ composes; Learner trains, checkpoints and resumes with cfg opt_fn.  ResNet-18, 96 px, B = 2 (as
test_gpu_ema_net.py), ZSG_DETERMINISTIC=1."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import zsg_oracle as O  # noqa: E402

ENC, FPN = "backbone.encoder.", "backbone.fpn."


@pytest.fixture(scope="module")
def Z():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import _lib, config, ema, loss, mdl, optim
    return _lib, config, ema, loss, mdl, optim


@pytest.fixture(autouse=True)
def deterministic(Z):
    """ZSG_DETERMINISTIC=1 for the plans lowered inside and the library's reductions (two runs on the same seeds give the same bits)"""
    L = Z[0]
    old = os.environ.get("ZSG_DETERMINISTIC")
    os.environ["ZSG_DETERMINISTIC"] = "1"
    L.lib.zsg_set_deterministic(1)
    yield
    if old is None:
        os.environ.pop("ZSG_DETERMINISTIC", None)
    else:
        os.environ["ZSG_DETERMINISTIC"] = old
    L.lib.zsg_set_deterministic(1 if old == "1" else 0)


def build(Z, seed=41):
    _lib, config, ema, loss, mdl, optim = Z
    cfg = config.get_cfg(resnet_arch="resnet18")
    net = mdl.get_default_net(9, cfg)
    net.load_state_dict(O.seeded_state_dict("resnet18", seed))
    net.to("cuda").train()
    r, s = config.ratios_scales(cfg)
    return net, loss.get_default_loss(r, s, cfg)


def batch(B=2, hw=96, seed=5):
    bt = O.synthetic_batch(B, hw, hw + 32, seed=seed, tmax=13)
    gq = torch.Generator().manual_seed(2)
    inp = {k: v.cuda() for k, v in bt.items()}
    inp["h0"], inp["c0"] = torch.randn(2, B, 128, generator=gq), torch.randn(2, B, 128, generator=gq)
    return inp


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# name -> (the fused optimizer of (optim, net, **kw), its torch twin of (groups), [(our buffer, torch's state key, atol)])
KINDS = {
    "adamw": (lambda optim, net, **kw: optim.FusedAdamW(net, lr=1e-3, betas=(0.9, 0.99), weight_decay=0.05, **kw),
              lambda gs: torch.optim.AdamW(gs, lr=1e-3, betas=(0.9, 0.99), weight_decay=0.05, foreach=False),
              [("m", "exp_avg", 1e-7), ("v", "exp_avg_sq", 1e-9)]),
    "adam_amsgrad": (lambda optim, net, **kw: optim.FusedAdam(net, lr=1e-3, betas=(0.9, 0.99), weight_decay=1e-2, amsgrad=True, **kw),
                     lambda gs: torch.optim.Adam(gs, lr=1e-3, betas=(0.9, 0.99), weight_decay=1e-2, amsgrad=True, foreach=False),
                     [("m", "exp_avg", 1e-7), ("v", "exp_avg_sq", 1e-9), ("vmax", "max_exp_avg_sq", 1e-9)]),
    "sgd_nesterov": (lambda optim, net, **kw: optim.FusedSGD(net, lr=1e-3, momentum=0.9, nesterov=True, weight_decay=1e-4, **kw),
                     lambda gs: torch.optim.SGD(gs, lr=1e-3, momentum=0.9, nesterov=True, weight_decay=1e-4, foreach=False),
                     [("momentum_buffer", "momentum_buffer", 1e-7)]),
}


def twins_of(net):
    """CPU copies of the parameters, by name"""
    return {n: torch.nn.Parameter(p.detach().cpu().clone()) for n, p in net.named_parameters()}


def feed(net, twins):
    """the network's own gradients to the twins (None stays None: torch's rule, no gradient, no step)"""
    torch.cuda.synchronize()
    for n, p in net.named_parameters():
        twins[n].grad = None if p.grad is None else p.grad.detach().cpu().clone()


def check_twin(net, opt, twins, topt, state, what):
    torch.cuda.synchronize()
    for n, p in net.named_parameters():
        torch.testing.assert_close(p.detach().cpu(), twins[n].detach(), rtol=1e-5, atol=1e-6, msg=lambda m, n=n: f"{what}: {n}: {m}")
        st = topt.state.get(twins[n])
        for mine, key, atol in state:
            got = net.store.view(n, getattr(opt, mine)).cpu()
            if st and st.get(key) is not None:
                torch.testing.assert_close(got, st[key], rtol=1e-4, atol=atol, msg=lambda m, n=n, key=key: f"{what}: {key} of {n}: {m}")
            else:
                assert not bool(got.any()), f"{what}: {n} has a {mine} but was never stepped"


def train_step(net, lf, opt, seed):
    opt.zero_grad()
    lf(net(batch(seed=seed)), batch(seed=seed))["loss"].backward()


def saved(opt):
    sd = opt.state_dict()
    sd["zsg"] = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in sd["zsg"].items()}
    return sd


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_step_matches_the_torch_twin_and_a_checkpoint_continues_bit_for_bit(Z, kind):
    optim = Z[5]
    make, ttwin, state = KINDS[kind]
    net, lf = build(Z)
    opt = make(optim, net)
    twins = twins_of(net)
    topt = ttwin([twins[n] for n, _ in net.named_parameters()])
    for it in range(3):
        train_step(net, lf, opt, 5 + it)
        feed(net, twins)
        opt.step()
        topt.step()
        check_twin(net, opt, twins, topt, state if it == 2 else [], f"{kind} step {it + 1}")
    assert not opt._seg and opt.step_count.tolist() == [3], "every parameter in one group: the single launch"
    # state_dict -> fresh optimizer -> load_state_dict: the next step gives the uninterrupted run's bits
    train_step(net, lf, opt, 9)
    torch.cuda.synchronize()
    sd, w = saved(opt), net.store.flat.clone()
    opt.step()
    ref = net.store.flat.clone()
    ref_state = [getattr(opt, mine).clone() for mine, _, _ in state]
    net.store.flat.copy_(w)
    opt2 = make(optim, net)
    opt2.load_state_dict(sd)
    opt2.step()
    torch.cuda.synchronize()
    assert torch.equal(bits(net.store.flat), bits(ref)) and opt2.step_count.tolist() == [4]
    for (mine, _, _), r in zip(state, ref_state):
        assert torch.equal(bits(getattr(opt2, mine)), bits(r)), mine
    # another rule's state is refused, both ways, and nothing is half-loaded
    other = optim.FusedAdam(net, lr=1e-3) if kind == "sgd_nesterov" else optim.FusedSGD(net, lr=1e-3, momentum=0.9)
    with pytest.raises(ValueError, match=f"{opt.NAME}.*{other.NAME}"):
        other.load_state_dict(sd)
    with pytest.raises(ValueError, match=f"{other.NAME}.*{opt.NAME}"):
        opt2.load_state_dict(other.state_dict())
    assert opt2.step_count.tolist() == [4]


@pytest.mark.parametrize("kind", list(KINDS))
def test_groups_and_a_frozen_fpn_take_the_segmented_path_and_unfreezing_matches_torch(Z, kind):
    optim = Z[5]
    make, ttwin, state = KINDS[kind]
    net, lf = build(Z, seed=42)
    names = [n for n, _ in net.named_parameters()]
    ps = dict(net.named_parameters())
    for n, p in ps.items():
        p.requires_grad_(not n.startswith(FPN))
    # the encoder at a lower lr without decay, the rest (the frozen FPN among it) with the kind's decay
    enc = dict(lr=2e-4, weight_decay=0.0)
    opt = make(optim, net, params=[dict(enc, params=[p for n, p in ps.items() if n.startswith(ENC)]),
                                   dict(params=[p for n, p in ps.items() if not n.startswith(ENC)])])
    twins = twins_of(net)
    topt = ttwin([dict(enc, params=[twins[n] for n in names if n.startswith(ENC)]), dict(params=[twins[n] for n in names if not n.startswith(ENC)])])
    fpn0 = {n: bits(p) for n, p in ps.items() if n.startswith(FPN)}
    assert fpn0
    for it in range(4):
        if it == 2:
            # two steps with the FPN frozen: its weights and every state buffer of its ranges are the bits they were
            torch.cuda.synchronize()
            assert opt._seg
            for n, b in fpn0.items():
                assert torch.equal(bits(ps[n]), b), f"the frozen {n} moved"
                for mine, _, _ in state:
                    assert not bool(net.store.view(n, getattr(opt, mine)).any()), f"{mine} of the frozen {n} was written"
            for p in ps.values():
                p.requires_grad_(True)
        train_step(net, lf, opt, 5 + it)
        feed(net, twins)
        assert all((ps[n].grad is None) == (it < 2) for n in fpn0)
        opt.step()
        topt.step()
        check_twin(net, opt, twins, topt, state if it == 3 else [], f"{kind} step {it + 1}")
    assert opt._seg, "two groups: the segmented path throughout"
    steps = opt.param_steps().tolist()
    assert steps == [2 if n.startswith(FPN) else 4 for n in names]
    assert all(int(topt.state[twins[n]]["step"]) == s for n, s in zip(names, steps) if "step" in topt.state[twins[n]])


def _launches(L, fn):
    L.lib.zsg_prof_enable(1)
    try:
        L.lib.zsg_prof_collect((L.ProfEntry * 256)(), 256)          # (drop earlier records)
        fn()
        torch.cuda.synchronize()
        ents = (L.ProfEntry * 256)()
        n = L.lib.zsg_prof_collect(ents, 256)
    finally:
        L.lib.zsg_prof_enable(0)
    return {ents[i].name.decode(): ents[i].launches for i in range(n)}


def _steps_of(got):
    """the optimizer-family launches among the recorded ones"""
    return {k: v for k, v in got.items() if k.startswith(("optim_", "adam_", "ema_", "swap_"))}


def test_average_attached_to_adamw_rides_in_the_one_launch(Z):
    L, ema, optim = Z[0], Z[2], Z[5]
    make = KINDS["adamw"][0]
    runs = []
    for attached in (True, False):
        net, lf = build(Z, seed=43)
        opt = make(optim, net)
        avg = ema.ModelEma(net, decay=0.9)
        if attached:
            avg.attach(opt)
        for it in range(3):
            train_step(net, lf, opt, 5 + it)
            got = _launches(L, opt.step)
            if attached:
                assert _steps_of(got) == {"optim_adamw_step_ema": 1, "ema_update": 1}, got          # (ema_update: the BatchNorm statistics)
            else:
                assert _steps_of(got) == {"optim_adamw_step": 1}, got
                avg.update()
        torch.cuda.synchronize()
        assert avg.n_averaged == 3 and not opt._seg
        runs.append((net, opt, avg))
    (na, oa, aa), (nb, ob, ab) = runs
    assert torch.equal(bits(aa.flat), bits(ab.flat)) and torch.equal(bits(aa.rmv), bits(ab.rmv)) and torch.equal(aa.nbt, ab.nbt)
    assert torch.equal(bits(na.store.flat), bits(nb.store.flat)) and torch.equal(bits(oa.m), bits(ob.m)) and torch.equal(bits(oa.v), bits(ob.v))
    assert not torch.equal(bits(aa.flat), bits(na.store.flat))
    # behind a segmented step the average is one zsg_ema_update over everything, as with FusedAdam
    for n, p in na.named_parameters():
        p.requires_grad_(not n.startswith(FPN))
    na.zero_grad(set_to_none=True)
    train_step(na, lf, oa, 9)
    got = _launches(L, oa.step)
    assert _steps_of(got) == {"optim_adamw_step_segments": 1, "ema_update": 1}, got
    assert aa.n_averaged == 4


def test_clip_grad_norm_in_front_of_fused_sgd_tracks_torch(Z):
    """tests/test_gpu_clip_net.py::test_clipped_fused_adam_tracks_torch_adam with SGD: the twins live on the GPU, where torch's own norm
    is accurate enough to be compared at rtol 1e-5 (its fp32 CPU norm of these 11 M gradients is 1.9e-5 off the fp64 sum zsg_grad_norm
    forms: measured, 933.897 against 933.915)"""
    optim = Z[5]
    net, lf = build(Z, seed=44)
    opt = optim.FusedSGD(net, lr=1e-3, momentum=0.9)
    names = [n for n, _ in net.named_parameters()]
    twins = {n: torch.nn.Parameter(p.detach().clone()) for n, p in net.named_parameters()}
    topt = torch.optim.SGD([twins[n] for n in names], lr=1e-3, momentum=0.9, foreach=False)
    for it in range(3):
        train_step(net, lf, opt, 5 + it)
        for n, p in net.named_parameters():
            twins[n].grad = p.grad.detach().clone()
        max_norm = 0.5 * float(torch.nn.utils.get_total_norm([twins[n].grad for n in names]))
        tn = optim.clip_grad_norm_(net.parameters(), max_norm)
        tt = torch.nn.utils.clip_grad_norm_([twins[n] for n in names], max_norm)
        torch.testing.assert_close(tn, tt, rtol=1e-5, atol=0)
        opt.step()
        topt.step()
        torch.cuda.synchronize()
        for n, p in net.named_parameters():
            torch.testing.assert_close(p.detach(), twins[n].detach(), rtol=1e-5, atol=1e-6, msg=lambda m, n=n: f"clipped step {it + 1}: {n}: {m}")
            torch.testing.assert_close(net.store.view(n, opt.momentum_buffer), topt.state[twins[n]]["momentum_buffer"], rtol=1e-4, atol=1e-7,
                                       msg=lambda m, n=n: f"clipped step {it + 1}: momentum buffer of {n}: {m}")


def _learner(Z, tmp_path, uid, **kw):
    config = Z[1]
    from zsgnet_pytorch_amd.main_dist import learner_init
    cfg = config.get_cfg(resnet_arch="resnet18", bs=2, bsv=2, resize_img=[96, 96], steps_per_epoch=2, tmp_path=str(tmp_path), synthetic=True,
                         **kw)
    cfg.freeze()
    return learner_init(uid, cfg)


def test_learner_trains_checkpoints_and_resumes_with_opt_fn_adamw(Z, tmp_path):
    L, config, optim = Z[0], Z[1], Z[5]
    hp = dict(config.DEFAULTS["opt_fn_params"], weight_decay=0.05)
    learn = _learner(Z, tmp_path, "adamw", opt_fn="AdamW", opt_fn_params=hp)
    learn.prepare_optimizer(1e-3)
    opt = learn.optimizer
    assert type(opt) is optim.FusedAdamW and opt.param_groups[0]["weight_decay"] == 0.05 and tuple(opt.param_groups[0]["betas"]) == (0.9, 0.99)
    got = _launches(L, learn.train_epoch)
    assert got.get("optim_adamw_step") == 2 and not {"adam_step", "adam_step_ema", "adam_step_segments"} & set(got), got
    assert learn.num_it == 2 and opt.step_count.tolist() == [2]
    learn.save_model_dict()
    ck = torch.load(learn.model_file, map_location="cpu")
    assert ck["optimizer_state_dict"]["zsg"]["algo"] == "AdamW" and set(ck["optimizer_state_dict"]["zsg"]) == {"algo", "m", "v", "step", "steps"}
    again = _learner(Z, tmp_path, "adamw", opt_fn="AdamW", opt_fn_params=hp, load_opt=True)
    assert again.num_it == 2 and type(again.optimizer) is optim.FusedAdamW and again.optimizer.step_count.tolist() == [2]
    assert torch.equal(bits(again.optimizer.m), bits(opt.m)) and torch.equal(bits(again.optimizer.v), bits(opt.v))
    assert torch.equal(bits(again.mdl.store.flat), bits(learn.mdl.store.flat))
    assert again.optimizer.param_groups[0]["weight_decay"] == 0.05
    # the checkpoint of one rule is refused by a Learner configured for another
    with pytest.raises(ValueError, match="AdamW.*SGD"):
        _learner(Z, tmp_path, "adamw", opt_fn="SGD", load_opt=True)
