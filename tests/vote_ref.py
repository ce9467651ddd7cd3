"""The definition the box-voting tests measure against (not a test module): zsg_eval_vote (include/zsg.h) restated in numpy on top of
tests/topk_ref.py — the same ranking (topk_ref.rank_order), the oracle's decode (O.reg_params_to_bbox), pixels (topk_ref.to_pixels)
and IoU (O.iou_values, kept box first, as the NMS calls it) — with the weighted sums in fp64 from the fp32 scores and coordinates,
accumulated candidate by candidate in rank order.

A candidate is valid when its score is not NaN and its decoded coordinates (y1x1y2x2 and pixels) are finite.  The members of a kept
row are its own candidate and every other valid candidate whose IoU with the row's box is >= vote_thr, if the row's own candidate is
valid; nobody otherwise.  voted = (float32)(sum s_c box_c / sum s_c); with no member or a zero weight sum the row keeps its box.
hit_rank is zsg_eval_topk's rule on the voted boxes in the [-1, 1] coordinates (the same weighted mean of the y1x1y2x2 boxes)."""
import numpy as np

from oracle import zsg_oracle as O

import topk_ref

F32 = np.float32


def _seq_sum(x: np.ndarray) -> np.ndarray:
    """fp64 sum over axis 0, one addend after the other (np.sum adds pairwise)"""
    acc = np.zeros(x.shape[1:], np.float64)
    for row in x:
        acc = acc + row
    return acc


def vote(att, reg, annot, img_size, anchors_f32, pre_n, K, vote_thr, nms_thr=0.5, acc_thr=0.5):
    """att [B, A] logits, reg [B, A, 4], annot [B, 4] or None, img_size [B, 2] = (h, w).  -> topk_ref.topk's outputs (the unvoted rows)
    under their names plus vote_boxes [B, K, 4], vote_n [B, K] and, with annot, vote_hit_rank [B], vote_acc_at [K], vote_iou [B, K]
    (the voted rows' IoU with annot, NaN past topk_n: what hit_rank thresholds)."""
    assert 0 < vote_thr <= 1
    B, A = att.shape
    res = topk_ref.topk(att, reg, annot, img_size, anchors_f32, pre_n, K, nms_thr, acc_thr)
    score = O._sigmoid(att)
    reg = reg.astype(F32)
    vb = np.zeros((B, K, 4), F32)
    vn = np.zeros((B, K), np.int32)
    hit = np.full(B, K, np.int32)
    viou = np.full((B, K), np.nan, F32)
    for b in range(B):
        order = topk_ref.rank_order(score[b])[:min(pre_n, A)]
        s = score[b, order]
        cand = O.reg_params_to_bbox(anchors_f32[order], reg[b, order][None])[0]
        px = topk_ref.to_pixels(cand, np.broadcast_to(img_size[b], (len(order), 2)))
        valid = ~np.isnan(s) & np.isfinite(cand).all(axis=1) & np.isfinite(px).all(axis=1)
        for r in range(int(res["topk_n"][b])):
            own = int(np.nonzero(order == res["topk_idx"][b, r])[0][0])
            vb[b, r] = res["topk_boxes"][b, r]
            norm = cand[own]
            if valid[own]:
                with np.errstate(invalid="ignore"):
                    m = valid & (O.iou_values(cand[own:own + 1], cand)[0] >= F32(vote_thr))
                m[own] = True
                vn[b, r] = int(m.sum())
                w = s[m].astype(np.float64)
                sw = _seq_sum(w)
                if sw > 0:
                    vb[b, r] = (_seq_sum(w[:, None] * px[m].astype(np.float64)) / sw).astype(F32)
                    norm = (_seq_sum(w[:, None] * cand[m].astype(np.float64)) / sw).astype(F32)
            if annot is not None:
                with np.errstate(invalid="ignore"):
                    viou[b, r] = O.iou_values(norm[None], annot[b:b + 1].astype(F32))[0, 0]
                if hit[b] == K and viou[b, r] >= F32(acc_thr):
                    hit[b] = r
    res["vote_boxes"], res["vote_n"] = vb, vn
    if annot is not None:
        res["vote_hit_rank"] = hit
        res["vote_acc_at"] = np.array([F32((hit <= j).sum()) / F32(B) for j in range(K)], F32)
        res["vote_iou"] = viou
    return res
