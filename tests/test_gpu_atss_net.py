"""The ATSS anchor assignment on the network: one training step (ResNet-18, 128 px, B = 2) with cfg matcher = "atss" through the fast path
(the loss kernel writes d loss / d out5 into the plan's incoming-gradient buffer, _LossScalar.backward, FusedAdam) gives the head the
gradients of the unfused composition: the fp64 reference's d loss / d out5 (tests/atss_ref.py: the numpy matcher, then the criterion on
its mask) fed through the same backward by out5.backward(gradient=...).  Tolerance: the head-gradient bound of tests/test_gpu_net.py
(relative error of the norm < 5e-2), as tests/test_gpu_quality_net.py.  And Learner trains two epochs and validates with atss, also with
qfl + GIoU on batches grouped by image."""
import os

import numpy as np
import pytest
import torch

import atss_ref as T

pytestmark = pytest.mark.gpu

from oracle import zsg_oracle as O  # noqa: E402

HEAD = "att_reg_box."


@pytest.fixture(scope="module")
def Z():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from zsgnet_pytorch_amd import config, loss, mdl, optim
    return config, loss, mdl, optim


@pytest.fixture(autouse=True)
def deterministic(Z):
    """ZSG_DETERMINISTIC=1 for the plans lowered inside (as tests/test_gpu_quality_net.py): three passes over one batch give the same bits"""
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


def test_fast_path_carries_the_atss_assignment(Z):
    config, loss, mdl, optim = Z
    cfg = config.get_cfg(resnet_arch="resnet18", matcher="atss")
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

    # the fixed rule's gradient through the backward (what the step would get without the feature) ...
    opt.zero_grad()
    out = net(inp)
    o = out["att_bbx_out"].detach().clone().requires_grad_()
    plain(dict(att_bbx_out=o, feat_sizes=out["feat_sizes"], num_f_out=out["num_f_out"]), inp)["loss"].backward()
    anc = plain.anchs.cpu().numpy()
    fs = out["feat_sizes"][:int(out["num_f_out"][0])].tolist()
    on = o.detach().cpu().numpy()
    out["att_bbx_out"].backward(gradient=o.grad.clone())
    without = head_grads()
    # ... and the unfused composition: the numpy matcher, then the reference's d loss / d out5 of the criterion on its mask
    annot = bt["annot"].numpy()
    m = T.atss_match(annot, anc, T.level_table(fs, 9), 9)
    fixed = O.match_mask(O.iou_values(annot, anc), 0.6)[0]
    print("positives: atss", m["mask"].sum(1).tolist(), "fixed rule", fixed.sum(1).tolist(), "thresholds", m["thr"].tolist())
    assert not np.array_equal(m["mask"], fixed)
    for b in range(2):                                           # what an exact mask relies on
        C = m["cand"][b, :m["ncand"][b]]
        assert np.abs(m["iou"][b, C].astype(np.float64) - m["thr"][b]).min() >= 1e-6
    ref = T.compose(on[..., 4], on[..., :4], annot, anc, m["mask"], m["best"])
    g5 = torch.from_numpy(np.concatenate([ref["g_reg"], ref["g_att"][..., None]], axis=2)).float().cuda()
    opt.zero_grad()
    out = net(inp)
    out["att_bbx_out"].backward(gradient=g5)
    want = head_grads()

    # the training step
    opt.zero_grad()
    out = net(inp)
    ls = lf(out, inp)
    assert list(ls) == ["loss", "cls_ls", "box_ls"]
    ls["loss"].mean().backward()
    got = head_grads()
    before = {n: p.detach().clone() for n, p in net.named_parameters() if n in head}
    opt.step()
    torch.cuda.synchronize()
    assert lf.level_off.tolist() == T.level_table(fs, 9).tolist()
    assert np.array_equal(lf.pos_mask.cpu().numpy().astype(bool), m["mask"])
    assert np.array_equal(lf.npos.cpu().numpy(), m["mask"].sum(1)) and np.array_equal(lf.match_idx.cpu().numpy(), m["best"])
    carried = 0
    for n in head:
        e, share = rel_err(got[n], want[n]), rel_err(without[n], want[n])
        print(f"{n}: relative error {e:.3g}; distance of the fixed rule's gradient {share:.3g}")
        assert e < 5e-2, f"{n}: relative error {e:.3g}"
        # The backward is linear in d loss / d out5: what exchanging the assignment changes in the step's gradient must be what it
        # changes in the composition, to the same bound, wherever the change stands clear of fp32 summation noise (1e-3 >> 1e-6).
        if share > 1e-3:
            carried += 1
            ec = rel_err(got[n] - without[n], want[n] - without[n])
            print(f"{n}: relative error of the change against the fixed rule {ec:.3g}")
            assert ec < 5e-2, f"{n}: the assignment's contribution is off by {ec:.3g}"
    assert carried > 0
    assert any(not torch.equal(p.detach(), before[n]) for n, p in net.named_parameters() if n in head)      # the step was taken
    for k in ("loss", "cls_ls", "box_ls"):
        np.testing.assert_allclose(float(ls[k]), ref[k], rtol=1e-5, err_msg=k)


@pytest.mark.parametrize("extra", [dict(matcher="atss"),
                                   dict(matcher="atss", cls_quality="qfl", box_iou_loss="giou", group_trn_by_image=True,
                                        trn_queries_per_image=2)],
                         ids=["atss", "atss_qfl_giou_grouped"])
def test_learner_trains_two_epochs_and_validates(Z, tmp_path, extra):
    config = Z[0]
    from zsgnet_pytorch_amd.main_dist import learner_init
    cfg = config.get_cfg(resnet_arch="resnet18", bs=4, bsv=2, resize_img=[96, 96], steps_per_epoch=4, tmp_path=str(tmp_path),
                         synthetic=True, **extra)
    cfg.freeze()
    learn = learner_init("atss", cfg)
    keys = ["loss", "cls_ls", "box_ls"] + (["iou_ls", "pos_iou"] if "cls_quality" in extra else [])
    assert learn.loss_keys == keys
    w0 = learn.mdl.store.flat.clone()
    tr, va = learn.fit(2, 1e-4)
    assert learn.num_epoch == 2 and not torch.equal(learn.mdl.store.flat, w0)
    assert set(keys) <= set(tr) and all(np.isfinite(tr[k]) for k in keys), tr
    assert set(va) == set(learn.loss_keys) | set(learn.met_keys) and all(np.isfinite(v) for v in va.values()), va
    np.testing.assert_allclose(va["loss"], va["box_ls"] + va.get("iou_ls", 0.0) + va["cls_ls"], rtol=1e-4)
    lf = learn.loss_fn
    assert lf.matcher == "atss" and lf.pos_mask.dtype == torch.uint8 and int(lf.npos.min()) >= 1
    assert torch.equal(lf.pos_mask.sum(1).int(), lf.npos)
