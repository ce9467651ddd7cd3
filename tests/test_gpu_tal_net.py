"""The task-aligned anchor assignment on the network: one training step (ResNet-18, 128 px, B = 2) with cfg matcher = "tal",
cls_quality = "qfl", box_iou_loss = "giou" (the TOOD-style recipe) through the fast path: the loss and every gradient are finite, every
sample has a positive, the mask is the selection redone from the metric the module keeps, and two fresh networks with one seed give the
same bits (the assignment reads the forward's output: no atomics, fixed orders).  The same step on a batch grouped by image runs and is
finite."""
import os

import numpy as np
import pytest
import torch

import tal_ref as R

pytestmark = pytest.mark.gpu

from oracle import zsg_oracle as O  # noqa: E402

RECIPE = dict(matcher="tal", cls_quality="qfl", box_iou_loss="giou")
KEYS = ["loss", "cls_ls", "box_ls", "iou_ls", "pos_iou"]


@pytest.fixture(scope="module")
def Z():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import config, loss, mdl, optim, synth
    return config, loss, mdl, optim, synth


@pytest.fixture(autouse=True)
def deterministic(Z):
    """ZSG_DETERMINISTIC=1 for the plans lowered inside (as tests/test_gpu_atss_net.py): the same batch gives the same bits"""
    from zsgnet_pytorch_amd import _lib as L
    old = os.environ.get("ZSG_DETERMINISTIC")
    os.environ["ZSG_DETERMINISTIC"] = "1"
    L.lib.zsg_set_deterministic(1)
    yield
    if old is None:
        os.environ.pop("ZSG_DETERMINISTIC", None)
    else:
        os.environ["ZSG_DETERMINISTIC"] = old
    L.lib.zsg_set_deterministic(1 if old == "1" else 0)


def fresh(Z, shared=False):
    config, loss, mdl, optim, _ = Z
    cfg = config.get_cfg(resnet_arch="resnet18", **RECIPE)
    net = mdl.get_default_net(9, cfg)
    net.load_state_dict(O.seeded_state_dict("resnet18", 41))
    net.to("cuda").train()
    if shared:
        net.shared_training(True)
    r, s = config.ratios_scales(cfg)
    return net, loss.get_default_loss(r, s, cfg), optim.FusedAdam(net, lr=1e-4, betas=(0.9, 0.99))


def step(net, lf, opt, inp):
    """one training step -> (losses as floats, the flat gradient, the module's mask / metric / npos as numpy)"""
    opt.zero_grad()
    ls = lf(net(inp), inp)
    assert list(ls) == KEYS
    ls["loss"].mean().backward()
    torch.cuda.synchronize()
    flat = net.store.grad.clone()
    before = net.store.flat.clone()
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(net.store.flat, before)                # the step was taken
    return ({k: float(v) for k, v in ls.items()}, flat, lf.pos_mask.cpu().numpy(), lf.tal_metric.cpu().numpy(), lf.npos.cpu().numpy(),
            lf.match_idx.cpu().numpy())


def check_step(res, Q):
    ls, flat, mask, metric, npos, midx = res
    assert all(np.isfinite(v) for v in ls.values()), ls
    assert bool(torch.isfinite(flat).all()) and float(flat.abs().max()) > 0
    assert mask.shape == metric.shape and mask.shape[0] == Q and set(np.unique(mask).tolist()) <= {0, 1}
    assert npos.min() >= 1
    for b in range(Q):                                            # the mask is the selection from the metric; the loss adds the arg-max anchor
        _, sel = R.select(metric[b], 13)
        want = np.zeros(mask.shape[1], np.uint8)
        want[sel] = 1
        assert np.array_equal(mask[b], want), b
        assert npos[b] == len(set(sel) | {int(midx[b])})
    return ls


def test_one_training_step_is_finite_and_two_fresh_networks_agree_bit_for_bit(Z):
    bt = O.synthetic_batch(2, 128, 128, seed=7)
    gq = torch.Generator().manual_seed(2)
    inp = {k: v.cuda() for k, v in bt.items()}
    inp["h0"], inp["c0"] = torch.randn(2, 2, 128, generator=gq), torch.randn(2, 2, 128, generator=gq)
    a = step(*fresh(Z), inp)
    ls = check_step(a, 2)
    print("tal + qfl + giou, ResNet-18 128 px B = 2:", ls, "positives per sample", a[4].tolist(), "selected by the assignment", a[2].sum(1).tolist())
    assert a[2].sum() > 0                                         # the assignment itself selected anchors at initialisation
    b = step(*fresh(Z), inp)
    assert a[0] == b[0]
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3].view(np.int64), b[3].view(np.int64)) and np.array_equal(a[4], b[4])


def test_the_step_on_a_batch_grouped_by_image_runs_and_is_finite(Z):
    synth = Z[4]
    idx = [1, 0, 0, 1]
    bt = synth.synthetic_shared_batch(2, len(idx), 128, 128, seed=21, tmax=13)
    bt["img_idx"] = torch.tensor(idx, dtype=torch.long)
    gq = torch.Generator().manual_seed(22)
    inp = {k: v.cuda() for k, v in bt.items()}
    inp["h0"], inp["c0"] = torch.randn(2, len(idx), 128, generator=gq), torch.randn(2, len(idx), 128, generator=gq)
    check_step(step(*fresh(Z, shared=True), inp), len(idx))
