"""The definition the Soft-NMS tests measure against (not a test module): zsg_eval_topk_soft (include/zsg.h) restated in numpy on top of
tests/topk_ref.py — the same ranking (topk_ref.rank_order), the oracle's decode (O.reg_params_to_bbox), pixels (topk_ref.to_pixels)
and IoU (O.iou_values, kept box first, as the NMS calls it) — with the weights in fp64, decayed pick by pick.

Row 0 is candidate 0 whatever its score.  Every further row is the unpicked candidate with a non-NaN score and the largest weight, ties
to the smaller position; the rows end when there is none or when that weight is < (double)(float32)min_score.  After picking m every
unpicked candidate c with u = IoU(box_m, box_c) has its weight multiplied by 1 - u where u > nms_thr ("soft_linear", fp32 compare) or
by exp(-u u / sigma) where u is not NaN ("soft_gauss").  topk_scores are the weights at pick time, rounded to fp32.

trace=True also returns, per query, what the GPU tests' input-safety check reads: every pick's (best weight, runner-up weight, whether
both are still the undecayed scores), every compared IoU, every weight the floor was compared with, the picked boxes' IoU with annot
and, per row, whether its candidate was never decayed."""
import numpy as np

from oracle import zsg_oracle as O

import topk_ref

F32 = np.float32
METHODS = ("soft_linear", "soft_gauss")


def soft_topk(att, reg, annot, img_size, anchors_f32, pre_n, K, method, nms_thr=0.5, sigma=0.5, min_score=0.001, acc_thr=0.5, trace=False):
    """att [B, A] logits, reg [B, A, 4], annot [B, 4] or None, img_size [B, 2] = (h, w).  -> the outputs of zsg_eval_topk_soft."""
    assert method in METHODS and 1 <= K <= pre_n
    B, A = att.shape
    score = O._sigmoid(att)
    reg = reg.astype(F32)
    thr, sig, floor = F32(nms_thr), float(F32(sigma)), float(F32(min_score))
    boxes = np.zeros((B, K, 4), F32)
    scores = np.zeros((B, K), F32)
    idx = np.full((B, K), -1, np.int32)
    n = np.zeros(B, np.int32)
    hit = np.full(B, K, np.int32)
    traces = []
    for b in range(B):
        order = topk_ref.rank_order(score[b])[:min(pre_n, A)]
        nc = len(order)
        s = score[b, order]
        cand = O.reg_params_to_bbox(anchors_f32[order], reg[b, order][None])[0]
        w = s.astype(np.float64)                        # a NaN score is never looked at after row 0
        clean = np.ones(nc, bool)                       # never decayed: the weight is still the fp32 score
        open_ = ~np.isnan(s)                            # not picked, a score that is a number
        picked, emitted = [], []
        tr = dict(picks=[], ious=[], floor=[], hit_iou=[], clean=[])
        for r in range(K):
            if r == 0:
                m, wm = 0, float(s[0])
            else:
                live = np.flatnonzero(open_)
                if live.size == 0:
                    break
                m = int(live[np.argmax(w[live])])       # the largest weight, ties to the smaller position (argmax takes the first)
                wm = float(w[m])
                tr["floor"].append(wm)                  # every weight the floor is compared with, the stopping one included
                if wm < floor:
                    break
                rest = live[live != m]
                if rest.size:
                    ru = int(rest[np.argmax(w[rest])])
                    tr["picks"].append((wm, float(w[ru]), bool(clean[m] and clean[ru])))
            open_[m] = False
            tr["clean"].append(bool(clean[m]))          # the emitted score is the candidate's own score
            picked.append(m)
            emitted.append(s[m] if r == 0 else F32(wm))
            with np.errstate(invalid="ignore"):
                u = O.iou_values(cand[m:m + 1], cand)[0].astype(F32)
                tr["ious"].append(u[open_])
                if method == "soft_linear":
                    hitc = open_ & (u > thr)
                    w[hitc] = w[hitc] * (1.0 - u[hitc].astype(np.float64))
                    clean[hitc] = False
                else:
                    hitc = open_ & (u == u)
                    ud = u[hitc].astype(np.float64)
                    w[hitc] = w[hitc] * np.exp(-(ud * ud) / sig)
                    clean[hitc & (u != 0)] = False      # (exp(-0) is exactly 1: the weight keeps its bits)
        k = len(picked)
        n[b] = k
        idx[b, :k] = order[picked]
        scores[b, :k] = np.array(emitted, F32)
        boxes[b, :k] = topk_ref.to_pixels(cand[picked], np.broadcast_to(img_size[b], (k, 2)))
        if annot is not None:
            with np.errstate(invalid="ignore"):
                iou = O.iou_values(cand[picked], annot[b:b + 1].astype(F32))[:, 0]
            tr["hit_iou"] = [float(x) for x in iou]
            ok = iou >= F32(acc_thr)
            if ok.any():
                hit[b] = int(np.argmax(ok))
        traces.append(tr)
    res = dict(topk_boxes=boxes, topk_scores=scores, topk_idx=idx, topk_n=n)
    if annot is not None:
        res["hit_rank"] = hit
        res["acc_at"] = np.array([F32((hit <= j).sum()) / F32(B) for j in range(K)], F32)
    if trace:
        res["trace"] = traces
    return res
