"""optim.FusedLAMB on the network (Optimizers): over real training steps it follows tests/lamb_ref.py applied on the host
to the network's own gradients, with the groups cfg opt_fn "LAMB" builds (1-D tensors not adaptive: their trust ratio is 1), also behind
clip_grad_norm_; a frozen parameter keeps its value, state and counter; an attached weight average is zsg_ema_update of the post-step
weights; a checkpoint continues bit for bit and another rule's is refused; Learner warms the learning rate up (cfg warmup_iters).
ResNet-18, 96 px, B = 2 (as test_gpu_optim_net.py), ZSG_DETERMINISTIC=1."""
import os

import numpy as np
import pytest
import torch

import lamb_ref

pytestmark = pytest.mark.gpu

from oracle import zsg_oracle as O  # noqa: E402

FPN = "backbone.fpn."
HP = dict(lr=2e-3, betas=(0.9, 0.99), eps=1e-6, weight_decay=0.01)


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


def make(Z, net, **kw):
    """FusedLAMB with the groups of cfg opt_fn "LAMB": >= 2-D adaptive with decay, 1-D plain without"""
    optim = Z[5]
    return optim.FusedLAMB(net, params=optim.lamb_param_groups(net._ordered_params()), **dict(HP, **kw))


def train_step(net, lf, opt, seed):
    opt.zero_grad()
    lf(net(batch(seed=seed)), batch(seed=seed))["loss"].backward()


def saved(opt):
    sd = opt.state_dict()
    sd["zsg"] = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in sd["zsg"].items()}
    return sd


class HostLamb:
    """lamb_ref over host copies of the parameters, by name: the twin the device optimizer is held against"""

    def __init__(self, net):
        self.w = {n: p.detach().cpu().numpy().copy() for n, p in net.named_parameters()}
        self.m = {n: np.zeros_like(w) for n, w in self.w.items()}
        self.v = {n: np.zeros_like(w) for n, w in self.w.items()}
        self.t = {n: 0 for n in self.w}
        self.info = {}

    def step(self, net):
        """one step from the network's current gradients (None: no step, torch's rule)"""
        torch.cuda.synchronize()
        for n, p in net.named_parameters():
            if p.grad is None:
                self.info[n] = None
                continue
            self.t[n] += 1
            adapt = p.dim() >= 2
            self.w[n], self.m[n], self.v[n], self.info[n] = lamb_ref.lamb_step(
                self.w[n], p.grad.detach().cpu().numpy(), self.m[n], self.v[n], self.t[n], HP["lr"], HP["betas"][0], HP["betas"][1], HP["eps"],
                HP["weight_decay"] if adapt else 0.0, adapt)

    def check(self, net, opt, what, state):
        torch.cuda.synchronize()
        ratios = opt.trust_ratios().cpu().tolist()
        nw, nu = (x.cpu().tolist() for x in opt.norms())
        for k, (n, p) in enumerate(net.named_parameters()):
            torch.testing.assert_close(p.detach().cpu(), torch.from_numpy(self.w[n]), rtol=1e-5, atol=1e-6, msg=lambda s, n=n: f"{what}: {n}: {s}")
            if state:
                torch.testing.assert_close(net.store.view(n, opt.m).cpu(), torch.from_numpy(self.m[n]), rtol=1e-4, atol=1e-7,
                                           msg=lambda s, n=n: f"{what}: m of {n}: {s}")
                torch.testing.assert_close(net.store.view(n, opt.v).cpu(), torch.from_numpy(self.v[n]), rtol=1e-4, atol=1e-9,
                                           msg=lambda s, n=n: f"{what}: v of {n}: {s}")
            info = self.info[n]
            if info is None:
                assert ratios[k] == 1.0, f"{what}: {n} was not stepped"
                continue
            for a, b, q in ((ratios[k], info["ratio"], "ratio"), (nw[k], info["norm_w"], "|w|"), (nu[k], info["norm_u"], "|u|")):
                assert abs(a - float(b)) <= 1e-5 * abs(float(b)), f"{what}: {q} of {n}: {a} against {float(b)}"
            if p.dim() < 2:
                assert ratios[k] == 1.0, f"{what}: the 1-D {n} has a trust ratio"


@pytest.mark.parametrize("clip", [False, True])
def test_three_steps_follow_the_host_reference(Z, clip):
    optim = Z[5]
    net, lf = build(Z)
    opt = make(Z, net)
    assert [g["adapt"] for g in opt.param_groups] == [True, False] and opt.param_groups[1]["weight_decay"] == 0.0
    host = HostLamb(net)
    for it in range(3):
        train_step(net, lf, opt, 5 + it)
        if clip:
            torch.cuda.synchronize()
            g64 = torch.cat([p.grad.detach().double().reshape(-1) for p in net.parameters()])
            norm = float(g64.norm())
            before = {n: p.grad.detach().clone() for n, p in net.named_parameters()}
            tn = optim.clip_grad_norm_(net.parameters(), 0.5 * norm)
            assert float(tn) == pytest.approx(norm, rel=1e-5)
            n0, p0 = next(iter(net.named_parameters()))
            torch.testing.assert_close(p0.grad, before[n0] * 0.5, rtol=1e-5, atol=0)          # the step below sees the clipped gradients
        host.step(net)
        opt.step()
        host.check(net, opt, f"step {it + 1}" + (" (clipped)" if clip else ""), state=it == 2)
    n = len(list(net.parameters()))
    assert opt._seg and opt.param_steps().tolist() == [3] * n, "per-parameter counters from the first step"
    r = opt.trust_ratios()
    one_d = torch.tensor([p.dim() < 2 for p in net.parameters()])
    assert r.is_cuda and bool((r.cpu()[one_d] == 1.0).all()) and bool((r.cpu()[~one_d] != 1.0).any())


def test_a_frozen_parameter_keeps_its_value_state_and_counter(Z):
    net, lf = build(Z, seed=42)
    ps = dict(net.named_parameters())
    for n, p in ps.items():
        p.requires_grad_(not n.startswith(FPN))
    opt = make(Z, net)
    host = HostLamb(net)
    fpn0 = {n: bits(p) for n, p in ps.items() if n.startswith(FPN)}
    assert fpn0
    for it in range(2):
        train_step(net, lf, opt, 5 + it)
        host.step(net)
        opt.step()
    host.check(net, opt, "frozen FPN, step 2", state=True)
    for n, b in fpn0.items():
        assert torch.equal(bits(ps[n]), b), f"the frozen {n} moved"
        assert not bool(net.store.view(n, opt.m).any()) and not bool(net.store.view(n, opt.v).any()), f"the state of the frozen {n} was written"
    assert opt.param_steps().tolist() == [0 if n.startswith(FPN) else 2 for n in ps]
    # unfrozen, it starts at its own t = 1 beside the others' t = 3
    for p in ps.values():
        p.requires_grad_(True)
    train_step(net, lf, opt, 7)
    host.step(net)
    opt.step()
    host.check(net, opt, "unfrozen, step 3", state=True)
    assert opt.param_steps().tolist() == [1 if n.startswith(FPN) else 3 for n in ps]


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


def test_attached_average_is_ema_update_of_the_post_step_weights(Z):
    L, ema = Z[0], Z[2]
    net, lf = build(Z, seed=43)
    opt = make(Z, net)
    avg = ema.ModelEma(net, decay=0.9).attach(opt)
    mine = net.store.flat.clone()
    for it, w in enumerate((1.0, 1.0 - 0.9, 1.0 - 0.9)):
        train_step(net, lf, opt, 5 + it)
        got = _launches(L, opt.step)
        steps = {k: v for k, v in got.items() if k.startswith(("optim_", "adam_", "ema_", "lamb_", "swap_"))}
        assert steps == {"lamb_moments": 1, "lamb_apply": 1, "ema_update": 1}, got
        L.check(L.lib.zsg_ema_update(mine.data_ptr(), net.store.flat.data_ptr(), mine.numel(), None, None, 0, w, L.stream_ptr()), "ema_update")
        torch.cuda.synchronize()
        assert torch.equal(bits(avg.flat), bits(mine)), f"step {it + 1}"
    assert avg.n_averaged == 3 and not torch.equal(bits(avg.flat), bits(net.store.flat))


def test_checkpoint_continues_bit_for_bit_and_an_adam_state_is_refused(Z):
    optim = Z[5]
    net, lf = build(Z, seed=44)
    opt = make(Z, net)
    for it in range(2):
        train_step(net, lf, opt, 5 + it)
        opt.step()
    train_step(net, lf, opt, 9)
    torch.cuda.synchronize()
    sd, w = saved(opt), net.store.flat.clone()
    assert sd["zsg"]["algo"] == "LAMB" and set(sd["zsg"]) == {"algo", "m", "v", "step", "steps"}
    opt.step()
    ref, ref_m, ref_v, ref_r = net.store.flat.clone(), opt.m.clone(), opt.v.clone(), opt.trust_ratios()
    net.store.flat.copy_(w)
    opt2 = make(Z, net, lr=1.0)          # (the saved groups bring the lr back)
    opt2.load_state_dict(sd)
    opt2.step()
    torch.cuda.synchronize()
    n = len(list(net.parameters()))
    assert torch.equal(bits(net.store.flat), bits(ref)) and opt2.param_steps().tolist() == [3] * n
    assert torch.equal(bits(opt2.m), bits(ref_m)) and torch.equal(bits(opt2.v), bits(ref_v)) and torch.equal(bits(opt2.trust_ratios()), bits(ref_r))
    adam = optim.FusedAdam(net, lr=1e-3)
    with pytest.raises(ValueError, match="belongs to Adam, this optimizer is LAMB"):
        opt2.load_state_dict(adam.state_dict())
    with pytest.raises(ValueError, match="belongs to LAMB, this optimizer is Adam"):
        adam.load_state_dict(sd)
    assert opt2.param_steps().tolist() == [3] * n


def test_learner_warms_the_learning_rate_up(Z, tmp_path):
    config, optim = Z[1], Z[5]
    from zsgnet_pytorch_amd.main_dist import learner_init
    base, W = 4e-3, 4
    cfg = config.get_cfg(resnet_arch="resnet18", bs=2, bsv=2, resize_img=[96, 96], steps_per_epoch=5, tmp_path=str(tmp_path), synthetic=True,
                         opt_fn="LAMB", warmup_iters=W)
    cfg.freeze()
    learn = learner_init("warm", cfg)
    learn.prepare_optimizer(base)
    opt = learn.optimizer
    assert type(opt) is optim.FusedLAMB and [g["adapt"] for g in opt.param_groups] == [True, False]
    seen, step = [], opt.step

    def recording_step(*a, **kw):
        seen.append([g["lr"] for g in opt.param_groups])
        return step(*a, **kw)
    opt.step = recording_step
    res = learn.train_epoch()
    assert learn.num_it == 5 and opt.param_steps().tolist() == [5] * len(list(learn.mdl.parameters()))
    assert seen == [[base * k / W] * 2 for k in (1, 2, 3, 4, 4)] and seen[3] == [base, base]
    assert all(np.isfinite(v) for v in res.values()) and bool(torch.isfinite(learn.mdl.store.flat).all())
