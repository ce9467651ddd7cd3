"""CPU-only checks of the box IoU loss (cfg box_iou_loss): the fp64 reference of tests/boxiou_ref.py against closed forms and
gradcheck, the cfg keys and ZSGLoss's validation of them, and the binding of zsg_loss_fwd_bwd_iou."""
import pytest
import torch

import boxiou_ref as R


@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_identical_boxes_give_zero(kind):
    b = torch.tensor([[-0.3, -0.2, 0.4, 0.5], [0.0, 0.0, 1.0, 1.0]], dtype=torch.float64)
    L = R.box_iou_loss(b, b.clone(), kind)
    assert L.abs().max().item() < 1e-6                  # (eps / area: 1e-7 / 0.49 and 1e-7 / 1)


def test_reference_disjoint_unit_squares_closed_form():
    """[0,0,1,1] vs [0,2,1,3]: inter 0, union 2, enclosing box 1 x 3, centres 2 apart -> giou 1 + 1/3, diou 1 + 4/10"""
    p = torch.tensor([[0.0, 0.0, 1.0, 1.0]], dtype=torch.float64)
    g = torch.tensor([[0.0, 2.0, 1.0, 3.0]], dtype=torch.float64)
    assert abs(R.box_iou_loss(p, g, "giou").item() - 4.0 / 3.0) < 1e-7
    assert abs(R.box_iou_loss(p, g, "diou").item() - 1.4) < 1e-7


@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_gradcheck(kind):
    gen = torch.Generator().manual_seed(5)
    tl = torch.rand(3, 2, generator=gen, dtype=torch.float64) * 0.5 - 0.6
    p = torch.cat([tl, tl + 0.2 + torch.rand(3, 2, generator=gen, dtype=torch.float64) * 0.6], dim=1).requires_grad_()
    tl = torch.rand(3, 2, generator=gen, dtype=torch.float64) * 0.5 - 0.6
    g = torch.cat([tl, tl + 0.2 + torch.rand(3, 2, generator=gen, dtype=torch.float64) * 0.6], dim=1)
    assert torch.autograd.gradcheck(lambda x: R.box_iou_loss(x, g, kind), (p,))


@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_gradcheck_through_decode(kind):
    gen = torch.Generator().manual_seed(6)
    anc = torch.tensor([[-0.5, -0.4, 0.1, 0.3], [-0.2, -0.6, 0.6, 0.2], [0.0, -0.1, 0.7, 0.8]], dtype=torch.float64)
    annot = torch.tensor([[-0.35, -0.3, 0.3, 0.35]], dtype=torch.float64)
    reg = (0.3 * torch.randn(1, 3, 4, generator=gen, dtype=torch.float64)).requires_grad_()
    mask = torch.tensor([[True, False, True]])
    assert torch.autograd.gradcheck(lambda r: R.iou_ls(r, annot, anc, mask, kind), (reg,))
    _, g = R.iou_ls_and_grad(reg.detach(), annot, anc, mask, kind)
    assert g[0, 1].abs().max().item() == 0 and g[0, 0].abs().max().item() > 0


def test_config_keys_and_validation():
    from zsgnet_pytorch_amd import config, loss
    cfg = config.get_cfg()
    assert cfg["box_iou_loss"] == "none" and cfg["lamb_iou"] == 1.0
    cfg = config.get_cfg(box_iou_loss="giou", lamb_iou=2)
    assert cfg["box_iou_loss"] == "giou" and cfg["lamb_iou"] == 2.0 and isinstance(cfg["lamb_iou"], float)
    r, s = config.ratios_scales(cfg)
    lf = loss.get_default_loss(r, s, cfg)
    assert lf.loss_keys == ["loss", "cls_ls", "box_ls", "iou_ls"] and lf.iou_kind == 1 and lf.lamb_iou == 2.0
    assert loss.get_default_loss(r, s, config.get_cfg(box_iou_loss="diou")).iou_kind == 2
    off = loss.get_default_loss(r, s, config.get_cfg())
    assert off.loss_keys == ["loss", "cls_ls", "box_ls"] and off.iou_kind == 0
    for bad in ("ciou", "GIoU", ""):
        with pytest.raises(ValueError):
            loss.get_default_loss(r, s, config.get_cfg(box_iou_loss=bad))
    with pytest.raises(ValueError):
        loss.get_default_loss(r, s, config.get_cfg(box_iou_loss="giou", lamb_iou=-0.5))
    # a pure IoU criterion is a valid configuration
    assert loss.get_default_loss(r, s, config.get_cfg(box_iou_loss="giou", lamb_reg=0)).lamb_reg == 0


def test_cli_override_reaches_the_cfg():
    from zsgnet_pytorch_amd import config
    cfg = config.update_from_dict(config.get_cfg(), {"box_iou_loss": "diou", "lamb_iou": "0.5"})
    assert cfg["box_iou_loss"] == "diou" and cfg["lamb_iou"] == 0.5


def test_binding_resolves_the_new_entry():
    import ctypes
    from zsgnet_pytorch_amd import _lib
    assert "zsg_loss_fwd_bwd_iou" in _lib.SIGNATURES
    fn = _lib.lib.zsg_loss_fwd_bwd_iou
    assert fn.restype is ctypes.c_int32 or fn.restype is ctypes.c_int
    assert len(fn.argtypes) == len(_lib.SIGNATURES["zsg_loss_fwd_bwd"][1]) + 2
    # bad arguments are refused before any launch (no GPU is touched): null pointers
    assert fn(None, None, None, 1, 1, 0.25, 2.0, 1.0, 0.6, 3, 1.0, 1, 1.0, None, None, None, None, None, 0, None) == -1
    assert b"loss_fwd_bwd_iou" in _lib.lib.zsg_last_error()
