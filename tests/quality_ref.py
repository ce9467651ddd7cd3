"""Independent restatement of the IoU-aware classification losses (cfg cls_quality = "qfl" / "vfl") as differentiable torch code, for
the tests.  It imports nothing of the product: the definition is written out from INTEGRATION.md "IoU-aware scores".

x = the att logit, s = sigmoid(x), m = the positives mask, q = m ? iou(decoded box of the anchor, annotation) : 0 with
iou = inter / (union + 1e-7) (tests/boxiou_ref.py's), a constant: nothing is differentiated through q.
    BCE(x, q) = max(x, 0) - x q + log1p(exp(-|x|))
    qfl:  l = |q - s|^gamma BCE(x, q)                                   every anchor
    vfl:  l = q BCE(x, q)  at positives,   alpha s^gamma BCE(x, 0)  at negatives
    cls_ls = sum of l over samples and anchors / sum of m;   pos_iou = mean over samples of (sum of q over the positives / their number)
compose() puts the term into the whole criterion: the oracle (oracle.zsg_oracle.zsg_loss) supplies the mask, box_ls and the smooth-L1
gradient, tests/boxiou_ref.py the optional IoU loss."""
import numpy as np
import torch

import boxiou_ref as R

EPS = 1e-7
KINDS = ("qfl", "vfl")


def iou(p: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """p, g [..., 4] (y1, x1, y2, x2) -> inter / (union + eps)"""
    py1, px1, py2, px2 = p.unbind(-1)
    gy1, gx1, gy2, gx2 = g.unbind(-1)
    iy = (torch.minimum(py2, gy2) - torch.maximum(py1, gy1)).clamp(min=0)
    ix = (torch.minimum(px2, gx2) - torch.maximum(px1, gx1)).clamp(min=0)
    inter = iy * ix
    union = (py2 - py1) * (px2 - px1) + (gy2 - gy1) * (gx2 - gx1) - inter
    return inter / (union + EPS)


def quality_target(reg, annot, anchors, mask) -> torch.Tensor:
    """q [B, A] fp64: the IoU of every positive anchor's decoded box with its sample's annotation, 0 at the negatives; detached"""
    reg, annot, anchors = [torch.as_tensor(x).double().detach() for x in (reg, annot, anchors)]
    mask = torch.as_tensor(mask).bool()
    boxes = R.decode(anchors, reg)
    q = iou(boxes, annot[:, None, :].expand_as(boxes))
    return torch.where(mask, q, torch.zeros_like(q))


def bce(x: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    return x.clamp(min=0) - x * q + torch.log1p(torch.exp(-x.abs()))


def elementwise(x, q, mask, kind: str, alpha: float, gamma: float) -> torch.Tensor:
    """l [B, A] from the logits x (may require grad), the targets q and the bool mask"""
    assert kind in KINDS, kind
    s = torch.sigmoid(x)
    if kind == "qfl":
        return (q - s).abs().pow(gamma) * bce(x, q)
    return torch.where(mask, q * bce(x, q), alpha * s.pow(gamma) * bce(x, torch.zeros_like(q)))


def cls_ls(x, q, mask, kind: str, alpha: float, gamma: float) -> torch.Tensor:
    return elementwise(x, q, mask, kind, alpha, gamma).sum() / mask.sum()


def cls_ls_and_grad(att, q, mask, kind, alpha, gamma):
    """fp64 value and d cls_ls / d att [B, A]"""
    x = torch.as_tensor(att).double().clone().requires_grad_()
    v = cls_ls(x, torch.as_tensor(q).double(), torch.as_tensor(mask).bool(), kind, alpha, gamma)
    (g,) = torch.autograd.grad(v, x)
    return v.detach(), g


def pos_iou(q, mask) -> float:
    q, mask = torch.as_tensor(q).double(), torch.as_tensor(mask).bool()
    return float(((q * mask).sum(1) / mask.sum(1)).mean())


def compose(O, att, reg, annot, anc, kind, box_iou="none", use_multi=True, alpha=0.25, gamma=2.0, lamb_reg=1.0, lamb_iou=1.0):
    """fp64 loss scalars and gradients of the whole criterion with the quality term; O = oracle.zsg_oracle"""
    r = O.zsg_loss(att, reg, annot, anc, alpha=alpha, gamma=gamma, lamb_reg=lamb_reg, use_multi=use_multi)
    assert not r["nan"]
    mask = r["mask"]
    q = quality_target(reg, annot, anc, mask)
    v, g_att = cls_ls_and_grad(att, q, mask, kind, alpha, gamma)
    iou_v, g_reg = 0.0, r["g_reg"].astype(np.float64)
    if box_iou != "none":
        iv, gi = R.iou_ls_and_grad(reg, annot, anc, mask, box_iou)
        iou_v, g_reg = float(iv), g_reg + lamb_iou * gi.numpy()
    return dict(loss=lamb_reg * float(r["box_ls"]) + lamb_iou * iou_v + float(v), cls_ls=float(v), box_ls=float(r["box_ls"]),
                iou_ls=iou_v, pos_iou=pos_iou(q, mask), g_att=g_att.numpy(), g_reg=g_reg, q=q.numpy(), mask=mask, best=r["best"])
