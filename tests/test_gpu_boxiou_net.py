"""The box IoU loss on the network: one training step (ResNet-18, 128 px, B = 2) with cfg box_iou_loss = "giou" through the fast path
(the loss kernel writes d loss / d out5 into the plan's incoming-gradient buffer, _LossScalar.backward, FusedAdam) gives the head the
gradients of the unfused composition: the plain loss's d / d out5 plus lamb_iou x the fp64 reference's IoU gradient (tests/boxiou_ref.py),
fed through the same backward by out5.backward(gradient=...).  Tolerance: the head-gradient bound of tests/test_gpu_net.py (relative
error of the norm < 5e-2).  And Learner trains, logs and validates with the four loss keys, a pure IoU box criterion (lamb_reg = 0) included."""
import os

import numpy as np
import pytest
import torch

import boxiou_ref as R

pytestmark = pytest.mark.gpu

from oracle import zsg_oracle as O  # noqa: E402

HEAD = "att_reg_box."
LAMB_IOU = 2.0


@pytest.fixture(scope="module")
def Z():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import config, loss, mdl, optim
    return config, loss, mdl, optim


@pytest.fixture(autouse=True)
def deterministic(Z):
    """ZSG_DETERMINISTIC=1 for the plans lowered inside (as tests/test_gpu_ema_net.py): three passes over one batch give the same bits"""
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


def rel_err(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def test_fast_path_carries_the_iou_term(Z):
    config, loss, mdl, optim = Z
    cfg = config.get_cfg(resnet_arch="resnet18", box_iou_loss="giou", lamb_iou=LAMB_IOU)
    net = mdl.get_default_net(9, cfg)
    net.load_state_dict(O.seeded_state_dict("resnet18", 41))
    net.to("cuda").train()
    r, s = config.ratios_scales(cfg)
    lf = loss.get_default_loss(r, s, cfg)
    plain = loss.get_default_loss(r, s, config.get_cfg(resnet_arch="resnet18"))
    opt = optim.FusedAdam(net, lr=1e-4, betas=(0.9, 0.99))
    bt = O.synthetic_batch(2, 128, 128, seed=7)
    gq = torch.Generator().manual_seed(2)
    inp = {k: v.cuda() for k, v in bt.items()}
    inp["h0"], inp["c0"] = torch.randn(2, 2, 128, generator=gq), torch.randn(2, 2, 128, generator=gq)
    head = [n for n, _ in net.named_parameters() if n.startswith(HEAD)]
    assert head

    def head_grads():
        torch.cuda.synchronize()
        return {n: p.grad.detach().clone() for n, p in net.named_parameters() if n in head}

    # the unfused composition: plain loss on a detached copy of the output (its own gradient buffer), the reference's IoU gradient on top
    opt.zero_grad()
    out = net(inp)
    o = out["att_bbx_out"].detach().clone().requires_grad_()
    plain(dict(att_bbx_out=o, feat_sizes=out["feat_sizes"], num_f_out=out["num_f_out"]), inp)["loss"].backward()
    anc = plain.anchs.cpu().numpy()
    on = o.detach().cpu().numpy()
    ref = O.zsg_loss(on[..., 4], on[..., :4], bt["annot"].numpy(), anc)
    _, gi = R.iou_ls_and_grad(on[..., :4], bt["annot"].numpy(), anc, ref["mask"], "giou")
    assert float(gi.abs().max()) > 0
    g5 = o.grad.clone()
    out["att_bbx_out"].backward(gradient=g5.clone())
    without = head_grads()
    opt.zero_grad()
    out = net(inp)
    g5[..., :4] += (LAMB_IOU * gi).float().cuda()
    out["att_bbx_out"].backward(gradient=g5)
    want = head_grads()

    # the training step
    opt.zero_grad()
    out = net(inp)
    ls = lf(out, inp)
    assert list(ls) == ["loss", "cls_ls", "box_ls", "iou_ls"]
    ls["loss"].mean().backward()
    got = head_grads()
    before = {n: p.detach().clone() for n, p in net.named_parameters() if n in head}
    opt.step()
    torch.cuda.synchronize()
    carried = 0
    for n in head:
        e, share = rel_err(got[n], want[n]), rel_err(without[n], want[n])
        print(f"{n}: relative error {e:.3g}; the IoU term's share of the gradient {share:.3g}")
        assert e < 5e-2, f"{n}: relative error {e:.3g}"
        # The classification gradient (every anchor) can dwarf the box terms in a parameter's gradient, so the bound above alone need
        # not notice a missing IoU term.  The backward is linear in d loss / d out5: what the term adds to the step's gradient must be
        # what it adds to the composition, to the same bound, wherever its share stands clear of fp32 summation noise (1e-3 >> 1e-6).
        if share > 1e-3:
            carried += 1
            ec = rel_err(got[n] - without[n], want[n] - without[n])
            print(f"{n}: relative error of the IoU term's contribution {ec:.3g}")
            assert ec < 5e-2, f"{n}: the IoU term's contribution is off by {ec:.3g}"
    assert carried > 0
    assert any(not torch.equal(p.detach(), before[n]) for n, p in net.named_parameters() if n in head)      # the step was taken
    np.testing.assert_allclose(float(ls["loss"]), float(ls["box_ls"]) + LAMB_IOU * float(ls["iou_ls"]) + float(ls["cls_ls"]), rtol=1e-5)


@pytest.mark.parametrize("lamb_reg", [1, 0])
def test_learner_trains_and_validates_with_four_loss_keys(Z, tmp_path, lamb_reg):
    config = Z[0]
    from zsgnet_pytorch_amd.main_dist import learner_init
    cfg = config.get_cfg(resnet_arch="resnet18", bs=2, bsv=2, resize_img=[96, 96], steps_per_epoch=4, tmp_path=str(tmp_path),
                         synthetic=True, box_iou_loss="giou", lamb_reg=lamb_reg)
    cfg.freeze()
    learn = learner_init("boxiou", cfg)
    assert learn.loss_keys == ["loss", "cls_ls", "box_ls", "iou_ls"]
    learn.prepare_optimizer(1e-4)
    w0 = learn.mdl.store.flat.clone()
    tr = learn.train_epoch()
    assert set(learn.loss_keys) <= set(tr) and all(np.isfinite(tr[k]) for k in learn.loss_keys), tr
    assert tr["iou_ls"] > 0
    assert not torch.equal(learn.mdl.store.flat, w0)
    va = learn.validate()
    assert set(va) == set(learn.loss_keys) | set(learn.met_keys) and all(np.isfinite(v) for v in va.values()), va
    np.testing.assert_allclose(va["loss"], lamb_reg * va["box_ls"] + va["iou_ls"] + va["cls_ls"], rtol=1e-4)
