"""optim.clip_grad_norm_ on the network (gradient clipping): after a real backward it matches
torch.nn.utils.clip_grad_norm_ on cloned gradients, counts and scales only the given parameters whose p.grad is not None (frozen
parameters and a frozen BatchNorm's d(gamma) / d(beta) by-products stay out), drives FusedAdam as torch's clip drives torch.optim.Adam, and
Learner clips with cfg clip_grad_norm.  ResNet-18, 96 px, B = 2 (as test_gpu_finetune.py)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import zsg_oracle as O  # noqa: E402

ENC = "backbone.encoder."


@pytest.fixture(scope="module")
def Z():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import config, loss, mdl, optim
    return config, loss, mdl, optim


def build(Z, seed=21):
    config, loss, mdl, optim = Z
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


def backward(net, lf, inp):
    net.zero_grad(set_to_none=True)
    lf(net(inp), inp)["loss"].backward()
    torch.cuda.synchronize()


def spans(net, params):
    """mask of the flat buffer: the storage ranges (padding included) of `params`"""
    ents, names = net.store.entries, dict((id(p), n) for n, p in net.named_parameters())
    m = torch.zeros(net.store.flat.numel(), dtype=torch.bool, device="cuda")
    for p in params:
        e = ents[names[id(p)]]
        m[e.offset:e.offset + (e.size + 3) // 4 * 4] = True
    return m


def exposed(net):
    """mask of the flat buffer: the elements some p.grad view shows (a convolution's padded input channels and the tail padding are not)"""
    m = torch.zeros(net.store.flat.numel(), dtype=torch.bool, device="cuda")
    for n in net._param_names:
        net.store.view(n, m).fill_(True)
    return m


def check_against_torch(Z, net, params, frac=0.5, norm_type=2.0):
    optim = Z[3]
    params = list(params)
    live = [p for p in params if p.grad is not None]
    assert live
    twins = [torch.nn.Parameter(p.detach().clone()) for p in live]
    for t, p in zip(twins, live):
        t.grad = p.grad.detach().clone()
    max_norm = frac * float(torch.nn.utils.get_total_norm([t.grad for t in twins], norm_type))
    tt = torch.nn.utils.clip_grad_norm_(twins, max_norm, norm_type)
    g0 = net.store.grad.clone()
    inside = spans(net, live)
    pad = inside & ~exposed(net)
    assert not bool(g0[pad].any()), "padding inside a listed range holds a nonzero gradient"
    tn = optim.clip_grad_norm_(params, max_norm, norm_type)
    torch.cuda.synchronize()
    assert tn.dim() == 0 and tn.dtype == torch.float32 and tn.is_cuda
    assert tn.untyped_storage().data_ptr() != net._clip_scratch[3].untyped_storage().data_ptr()
    torch.testing.assert_close(tn, tt, rtol=1e-5, atol=0)
    for t, p in zip(twins, live):
        torch.testing.assert_close(p.grad, t.grad, rtol=1e-6, atol=1e-12)
    assert torch.equal(net.store.grad[~inside].view(torch.int32), g0[~inside].view(torch.int32)), "a gradient outside the set was touched"
    assert not bool(net.store.grad[pad].any())
    return float(tn), max_norm


def test_all_trainable_both_norms(Z):
    net, lf = build(Z)
    inp = batch()
    for norm_type in (2.0, math.inf):
        backward(net, lf, inp)
        check_against_torch(Z, net, net.parameters(), norm_type=norm_type)


def test_frozen_encoder(Z):
    net, lf = build(Z, seed=22)
    for n, p in net.named_parameters():
        p.requires_grad_(not n.startswith(ENC))
    backward(net, lf, batch(seed=6))
    assert all(p.grad is None for n, p in net.named_parameters() if n.startswith(ENC))
    check_against_torch(Z, net, net.parameters())


def test_frozen_batchnorm_by_products_are_neither_counted_nor_scaled(Z):
    net, lf = build(Z, seed=23)
    bns = net.freeze_batchnorm()
    assert bns
    bn_params = {n for n, _ in net.named_parameters() if n.rsplit(".", 1)[0] in bns}
    for n, p in net.named_parameters():
        p.requires_grad_(n not in bn_params)
    backward(net, lf, batch(seed=7))
    assert all(p.grad is None for n, p in net.named_parameters() if n in bn_params)
    check_against_torch(Z, net, net.parameters())


def test_lstm_subset(Z):
    net, lf = build(Z, seed=24)
    backward(net, lf, batch(seed=8))
    lstm = [p for n, p in net.named_parameters() if n.startswith("lstm.")]
    assert len(lstm) == 8
    check_against_torch(Z, net, lstm, frac=0.3)


def test_clipped_fused_adam_tracks_torch_adam(Z):
    config, loss, mdl, optim = Z
    net, lf = build(Z, seed=25)
    inp = batch(seed=9)
    opt = optim.FusedAdam(net, lr=1e-3, betas=(0.9, 0.99))
    names = [n for n, _ in net.named_parameters()]
    twins = {n: torch.nn.Parameter(p.detach().clone()) for n, p in net.named_parameters()}
    topt = torch.optim.Adam([twins[n] for n in names], lr=1e-3, betas=(0.9, 0.99))
    for it in range(3):
        opt.zero_grad()
        lf(net(inp), inp)["loss"].backward()
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
        torch.testing.assert_close(p.detach(), twins[n].detach(), rtol=1e-5, atol=1e-6, msg=n)


def test_nonfinite_error_validation_and_no_gradients(Z):
    config, loss, mdl, optim = Z
    net, lf = build(Z, seed=26)
    backward(net, lf, batch(seed=10))
    bias = dict(net.named_parameters())["lstm.bias_ih_l0"]
    bias.grad[3] = float("inf")
    with pytest.raises(RuntimeError, match="non-finite"):
        optim.clip_grad_norm_(net.parameters(), 1.0, error_if_nonfinite=True)
    assert float(optim.clip_grad_norm_(net.parameters(), 1.0)) == math.inf
    with pytest.raises(ValueError, match="norm_type"):
        optim.clip_grad_norm_(net.parameters(), 1.0, norm_type=1.0)
    with pytest.raises(ValueError, match="not a parameter"):
        optim.clip_grad_norm_(list(net.parameters()) + [torch.nn.Parameter(torch.zeros(4, device="cuda"))], 1.0)
    other, _ = build(Z, seed=27)
    with pytest.raises(ValueError, match="same ZSGNet"):
        optim.clip_grad_norm_([next(net.parameters()), next(other.parameters())], 1.0)
    net.zero_grad(set_to_none=True)
    g0 = net.store.grad.clone()
    z = optim.clip_grad_norm_(net.parameters(), 1.0)
    assert z.dim() == 0 and float(z) == 0.0 and not z.is_cuda
    torch.cuda.synchronize()
    assert torch.equal(net.store.grad.view(torch.int32), g0.view(torch.int32))          # (bits: the inf clip above left NaN)


def test_learner_clips_and_logs_grad_norm(Z, tmp_path):
    config = Z[0]
    from zsgnet_pytorch_amd.main_dist import learner_init
    max_norm = 0.05
    cfg = config.get_cfg(resnet_arch="resnet18", bs=2, bsv=2, resize_img=[96, 96], steps_per_epoch=6, tmp_path=str(tmp_path),
                         synthetic=True, clip_grad_norm=max_norm)
    cfg.freeze()
    learn = learner_init("clip", cfg)
    learn.prepare_optimizer(1e-4)
    net = learn.mdl
    consumed = []
    step = learn.optimizer.step

    def spy(*a, **k):
        consumed.append(torch.linalg.vector_norm(net.store.grad, dtype=torch.float64))       # every parameter trains: the whole buffer
        return step(*a, **k)
    learn.optimizer.step = spy
    res = learn.train_epoch()
    assert len(consumed) == 6
    assert "grad_norm" in res and res["grad_norm"] > max_norm, res          # the pre-clip norm: clipping engaged
    for c in consumed:
        assert float(c) <= max_norm * (1 + 1e-6), float(c)
