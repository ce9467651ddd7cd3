"""Independent restatement of the box IoU loss (cfg box_iou_loss = "giou" / "diou") as differentiable torch code, for the tests.
It imports nothing of the product: the definition is written out from INTEGRATION.md "Box IoU loss".

Boxes are (y1, x1, y2, x2).  For a predicted box p and a target box g, eps = 1e-7:
    inter = max(min(p.y2, g.y2) - max(p.y1, g.y1), 0) * max(min(p.x2, g.x2) - max(p.x1, g.x1), 0)
    union = area(p) + area(g) - inter,   iou = inter / (union + eps)
    ey = max(p.y2, g.y2) - min(p.y1, g.y1),  ex likewise          (the enclosing box)
    giou:  L = 1 - iou + (ey ex - union) / (ey ex + eps)
    diou:  L = 1 - iou + rho2 / (ey^2 + ex^2 + eps),  rho2 = squared distance of the two centres
"""
import torch

EPS = 1e-7
KINDS = ("giou", "diou")


def box_iou_loss(p: torch.Tensor, g: torch.Tensor, kind: str) -> torch.Tensor:
    """p, g [..., 4] -> L [...]"""
    assert kind in KINDS, kind
    py1, px1, py2, px2 = p.unbind(-1)
    gy1, gx1, gy2, gx2 = g.unbind(-1)
    iy = (torch.minimum(py2, gy2) - torch.maximum(py1, gy1)).clamp(min=0)
    ix = (torch.minimum(px2, gx2) - torch.maximum(px1, gx1)).clamp(min=0)
    inter = iy * ix
    union = (py2 - py1) * (px2 - px1) + (gy2 - gy1) * (gx2 - gx1) - inter
    iou = inter / (union + EPS)
    ey = torch.maximum(py2, gy2) - torch.minimum(py1, gy1)
    ex = torch.maximum(px2, gx2) - torch.minimum(px1, gx1)
    if kind == "giou":
        return 1 - iou + (ey * ex - union) / (ey * ex + EPS)
    rho2 = ((py1 + py2) / 2 - (gy1 + gy2) / 2) ** 2 + ((px1 + px2) / 2 - (gx1 + gx2) / 2) ** 2
    return 1 - iou + rho2 / (ey ** 2 + ex ** 2 + EPS)


def decode(anchors: torch.Tensor, reg: torch.Tensor) -> torch.Tensor:
    """anchors [A, 4] tlbr, reg [B, A, 4] = (dy, dx, log h, log w) -> boxes [B, A, 4] tlbr (reference anchors.py:182-197)"""
    acy, acx = (anchors[:, 0] + anchors[:, 2]) / 2, (anchors[:, 1] + anchors[:, 3]) / 2
    ah, aw = anchors[:, 2] - anchors[:, 0], anchors[:, 3] - anchors[:, 1]
    cy, cx = ah * reg[..., 0] + acy, aw * reg[..., 1] + acx
    h, w = torch.exp(reg[..., 2]) * ah, torch.exp(reg[..., 3]) * aw
    return torch.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], dim=-1)


def iou_ls(reg: torch.Tensor, annot: torch.Tensor, anchors: torch.Tensor, mask: torch.Tensor, kind: str) -> torch.Tensor:
    """mean over samples of (sum of L over the sample's positive anchors / their number).  reg [B, A, 4] (may require grad),
    annot [B, 4], anchors [A, 4], mask [B, A] bool: the positives.  Only positives are evaluated: nothing of a negative anchor,
    not even a NaN, reaches the value or the gradient."""
    B = reg.shape[0]
    total = reg.new_zeros(())
    for b in range(B):
        idx = torch.nonzero(mask[b]).flatten()
        p = decode(anchors[idx], reg[b:b + 1, idx])[0]
        L = box_iou_loss(p, annot[b].expand_as(p), kind)
        total = total + L.sum() / idx.numel()
    return total / B


def iou_ls_and_grad(reg, annot, anchors, mask, kind):
    """fp64 value and d iou_ls / d reg [B, A, 4] (zero at negative anchors) from fp32 / fp64 numpy or torch inputs"""
    t = [torch.as_tensor(x).double() for x in (reg, annot, anchors)]
    r = t[0].clone().requires_grad_()
    v = iou_ls(r, t[1], t[2], torch.as_tensor(mask).bool(), kind)
    (g,) = torch.autograd.grad(v, r)
    return v.detach(), g
