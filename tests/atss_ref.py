"""Independent restatement of the ATSS anchor assignment (cfg matcher = "atss") in numpy, and of the criterion for an ARBITRARY positives
mask as differentiable fp64 torch code, for the tests.  It imports nothing of the product: the definition is written out from
INTEGRATION.md "Anchor assignment".

Anchors [A, 4] fp32 (y1, x1, y2, x2) in the flattened order of create_anchors; level l owns the indices [level_off[l], level_off[l + 1]).
One annotation g per sample, an integer k.  Every step in np.float32, in this order:
    acy = (a.y1 + a.y2) / 2, acx = (a.x1 + a.x2) / 2;  gcy, gcx likewise
    d(a) = (acy - gcy) (acy - gcy) + (acx - gcx) (acx - gcx)
    C = per level the min(k, n_l) anchors with the smallest key (d, index), lexicographic; ordered by level, then by rank
    v(a) = inter / (union + 1e-8), the matching IoU (the operation order of the reference's IoU_values)
    t = mean(v over C) + std(v over C): fp64 from the fp32 values, summed in the order of C, unbiased (0 for |C| = 1)
    positive: (a in C and (double)v(a) >= t and g.y1 < acy < g.y2 and g.x1 < acx < g.x2)  or  a == arg-max v (lowest index)
The criterion on a mask m (the reference's loss.py with its matching taken out): t = m as 0 / 1, s = sigmoid(x),
    box_ls = mean over samples of (sum over positives of smooth-L1(reg - target(anchor, g)) / #pos of the sample)
    cls_ls = sum of w BCE(x, t) / total #pos,  w = (t (1 - s) + (1 - t) s)^gamma ((1 - t) alpha + t (1 - alpha)), detached
compose() adds the optional IoU loss (tests/boxiou_ref.py) and quality term (tests/quality_ref.py), which already take a mask."""
import functools

import numpy as np
import torch

import boxiou_ref as R
import quality_ref as Q

F32 = np.float32
MAX_CAND = 8 * 16
# feature-map sizes of the test pyramids (9 anchors per cell): A = 126 (one block per sample in the loss kernels), 189 (chunked, ranges of
# 6: levels straddle ranges), 261 (non-square; a 9-anchor level = k, an 18-anchor level)
PYRAMIDS = {"P126": [(3, 3), (2, 2), (1, 1)], "P189": [(4, 4), (2, 2), (1, 1)], "P261": [(5, 4), (3, 2), (2, 1), (1, 1)]}
TOPKS = (4, 9, 12)
BATCHES = (1, 3)


def level_table(feat_sizes, n):
    return np.concatenate([[0], np.cumsum([int(h) * int(w) * n for h, w in feat_sizes])]).astype(np.int32)


def iou_f32(g, anc):
    """fp32 IoU [A] of one box g [4] with anchors [A, 4]"""
    g, a = g.astype(F32), anc.astype(F32)
    tly, tlx = np.maximum(g[0], a[:, 0]), np.maximum(g[1], a[:, 1])
    bry, brx = np.minimum(g[2], a[:, 2]), np.minimum(g[3], a[:, 3])
    sy, sx = np.maximum((bry - tly).astype(F32), F32(0)), np.maximum((brx - tlx).astype(F32), F32(0))
    inter = (sy * sx).astype(F32)
    garea = F32((g[2] - g[0]) * (g[3] - g[1]))
    aarea = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])).astype(F32)
    uni = ((garea + aarea).astype(F32) - inter).astype(F32)
    return (inter / (uni + F32(1e-8)).astype(F32)).astype(F32)


def centres(b):
    b = b.astype(F32)
    return ((b[..., 0] + b[..., 2]) / F32(2)).astype(F32), ((b[..., 1] + b[..., 3]) / F32(2)).astype(F32)


def atss_match(annot, anc, level_off, k):
    """-> dict: mask [B, A] bool (the positives), cand [B, 128] int32 (C in its order, -1 behind it), ncand [B], per_level [B, L] (the
    candidates of every level), thr [B] float64, best [B] int64, iou [B, A] fp32"""
    annot, anc = np.asarray(annot, F32), np.asarray(anc, F32)
    B, A, L = annot.shape[0], anc.shape[0], len(level_off) - 1
    assert level_off[0] == 0 and level_off[-1] == A
    acy, acx = centres(anc)
    mask = np.zeros((B, A), bool)
    cand = np.full((B, MAX_CAND), -1, np.int32)
    per_level = np.zeros((B, L), np.int64)
    thr, best, ious = np.zeros(B, np.float64), np.zeros(B, np.int64), np.zeros((B, A), F32)
    for b in range(B):
        g = annot[b]
        gcy, gcx = centres(g)
        dy, dx = (acy - gcy).astype(F32), (acx - gcx).astype(F32)
        d = ((dy * dy).astype(F32) + (dx * dx).astype(F32)).astype(F32)
        C = []
        for l in range(L):
            lo, hi = int(level_off[l]), int(level_off[l + 1])
            order = sorted(range(lo, hi), key=lambda a: (d[a], a))[:min(k, hi - lo)]
            per_level[b, l] = len(order)
            C += order
        v = iou_f32(g, anc)
        ious[b] = v
        s = 0.0
        for a in C:
            s += float(v[a])
        mean = s / len(C)
        ss = 0.0
        for a in C:
            ss += (float(v[a]) - mean) * (float(v[a]) - mean)
        thr[b] = mean + (np.sqrt(ss / (len(C) - 1)) if len(C) > 1 else 0.0)
        best[b] = int(np.argmax(v))                       # the first maximum: the lowest index
        for a in C:
            inside = g[0] < acy[a] < g[2] and g[1] < acx[a] < g[3]
            if float(v[a]) >= thr[b] and inside:
                mask[b, a] = True
        mask[b, best[b]] = True
        cand[b, :len(C)] = C
    return dict(mask=mask, cand=cand, ncand=(cand >= 0).sum(1), per_level=per_level, thr=thr, best=best, iou=ious)


def reg_targets(anc, annot):
    """fp64 [B, A, 4]: the regression targets of the reference's bbox_to_reg_params (the 1e-8 of its denominators included)"""
    a, g = torch.as_tensor(anc).double(), torch.as_tensor(annot).double()
    acy, acx, ah, aw = (a[:, 0] + a[:, 2]) / 2, (a[:, 1] + a[:, 3]) / 2, a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    gcy, gcx, gh, gw = (g[:, 0] + g[:, 2]) / 2, (g[:, 1] + g[:, 3]) / 2, g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
    dh, dw = ah + 1e-8, aw + 1e-8
    return torch.stack([(gcy[:, None] - acy[None]) / dh[None], (gcx[:, None] - acx[None]) / dw[None],
                        torch.log(gh[:, None] / dh[None]), torch.log(gw[:, None] / dw[None])], dim=-1)


def box_ls(reg, annot, anc, mask):
    """reg [B, A, 4] fp64 (may require grad), mask [B, A] bool"""
    d = reg - reg_targets(anc, annot)
    ad = d.abs()
    sl1 = torch.where(ad < 1, 0.5 * d * d, ad - 0.5).sum(-1)
    return (torch.where(mask, sl1, torch.zeros_like(sl1)).sum(1) / mask.sum(1)).mean()


def focal_cls_ls(x, mask, alpha, gamma, use_focal=True):
    t = mask.double()
    bce = x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    if use_focal:
        s = torch.sigmoid(x)
        w = ((t * (1 - s) + (1 - t) * s).pow(gamma) * ((1 - t) * alpha + t * (1 - alpha))).detach()
    else:
        w = torch.ones_like(x)
    return (w * bce).sum() / mask.sum()


def compose(att, reg, annot, anc, mask, best, kind="none", box_iou="none", alpha=0.25, gamma=2.0, lamb_reg=1.0, lamb_iou=1.0):
    """fp64 loss scalars and gradients of the whole criterion on the positives mask `mask`.  kind: "none" (focal) / "qfl" / "vfl";
    box_iou: "none" / "giou" / "diou"."""
    m = torch.as_tensor(mask).bool()
    x = torch.as_tensor(att).double().clone().requires_grad_()
    r = torch.as_tensor(reg).double().clone().requires_grad_()
    q = Q.quality_target(reg, annot, anc, mask)
    box = box_ls(r, annot, anc, m)
    cls = focal_cls_ls(x, m, alpha, gamma) if kind == "none" else Q.cls_ls(x, q, m, kind, alpha, gamma)
    total = lamb_reg * box + cls
    iou_v = 0.0
    if box_iou != "none":
        iou = R.iou_ls(r, torch.as_tensor(annot).double(), torch.as_tensor(anc).double(), m, box_iou)
        total = total + lamb_iou * iou
        iou_v = float(iou.detach())
    g_att, g_reg = torch.autograd.grad(total, (x, r))
    total, cls, box = total.detach(), cls.detach(), box.detach()
    return dict(loss=float(total), cls_ls=float(cls), box_ls=float(box), iou_ls=iou_v, pos_iou=Q.pos_iou(q, mask), g_att=g_att.numpy(),
                g_reg=g_reg.numpy(), mask=np.asarray(mask), best=np.asarray(best), q=q.numpy())


@functools.lru_cache(maxsize=None)
def pyramid_anchors(O, name):
    """(anchors [A, 4] fp32, level_off int32) of a test pyramid or of "full" (the 300 x 300 network's six levels, A = 17460)"""
    ratios, scales = O.default_ratios_scales()
    fs = O.feat_sizes_for(300, 300) if name == "full" else PYRAMIDS[name]
    anc = np.ascontiguousarray(O.create_anchors(fs, ratios, scales).astype(F32))
    off = level_table(fs, len(ratios) * len(scales))
    assert off[-1] == anc.shape[0]
    return anc, off


@functools.lru_cache(maxsize=None)
def inputs(O, name, B):
    """(att [B, A], reg [B, A, 4], annot [B, 4], anchors [A, 4], level_off) fp32: annot = a seeded anchor + U(-0.01, 0.01); reg and att
    drawn as tests/test_gpu_boxiou.py's inputs() draws them"""
    anc, off = pyramid_anchors(O, name)
    A = anc.shape[0]
    rs = np.random.RandomState(100 * A + B)
    ks = rs.choice(A, B, replace=False)
    annot = (anc[ks] + rs.uniform(-0.01, 0.01, (B, 4))).astype(F32)
    reg = (0.3 * rs.randn(B, A, 4)).astype(F32)
    att = (1.5 * rs.randn(B, A) - 2.0).astype(F32)
    return att, reg, annot, anc, off


@functools.lru_cache(maxsize=None)
def matched(O, name, B, k):
    att, reg, annot, anc, off = inputs(O, name, B)
    return atss_match(annot, anc, off, k)
