"""The reference the top-k grounding tests measure against (not a test module): the ordering contract of zsg_eval_topk restated in
numpy from the oracle's public pieces — O._sigmoid scores, a stable descending sort (ties to the lower anchor index, a NaN score below
every number), O.reg_params_to_bbox on the first min(pre_n, A) candidates, greedy NMS with O.iou_values(kept, candidate) > nms_thr,
hit_rank / acc_at with O.iou_values(box, annot) >= acc_thr.  Pinned to tests/golden/g17_topk.npz (made from the reference's own
functions by tests/golden/make_topk_fixture.py) by tests/test_cpu_topk.py."""
import numpy as np
import torch

from oracle import zsg_oracle as O

F32 = np.float32


def rank_order(score: np.ndarray) -> np.ndarray:
    """anchor indices of one query, best first: score descending, index ascending, NaN last"""
    key = np.where(np.isnan(score), F32(-1), score)
    return np.argsort(-key, kind="stable")


def to_pixels(boxes: np.ndarray, hw: np.ndarray) -> np.ndarray:
    """y1x1y2x2 in [-1, 1] -> pixels x1y1x2y2, as O.zsg_eval does for pred_boxes (evaluator.py:96-98)"""
    half = ((boxes.astype(F32) + F32(1)) / F32(2)).astype(F32)
    sz = hw.astype(F32)
    px = np.concatenate([sz * half[:, :2], sz * half[:, 2:]], axis=1).astype(F32)
    return px[:, [1, 0, 3, 2]]


def topk(att, reg, annot, img_size, anchors_f32, pre_n, K, nms_thr=0.5, acc_thr=0.5):
    """att [B, A] logits, reg [B, A, 4], annot [B, 4] or None, img_size [B, 2] = (h, w).  -> the outputs of zsg_eval_topk."""
    B, A = att.shape
    assert 1 <= K <= pre_n
    score = O._sigmoid(att)
    reg = reg.astype(F32)
    boxes = np.zeros((B, K, 4), F32)
    scores = np.zeros((B, K), F32)
    idx = np.full((B, K), -1, np.int32)
    n = np.zeros(B, np.int32)
    hit = np.full(B, K, np.int32)
    for b in range(B):
        order = rank_order(score[b])[:min(pre_n, A)]
        cand = O.reg_params_to_bbox(anchors_f32[order], reg[b, order][None])[0]
        kept = []
        for r in range(len(order)):
            if len(kept) == K:
                break
            if kept and np.any(O.iou_values(cand[kept], cand[r:r + 1])[:, 0] > F32(nms_thr)):
                continue
            kept.append(r)
        n[b] = len(kept)
        idx[b, :len(kept)] = order[kept]
        scores[b, :len(kept)] = score[b, order[kept]]
        boxes[b, :len(kept)] = to_pixels(cand[kept], np.broadcast_to(img_size[b], (len(kept), 2)))
        if annot is not None:
            ok = O.iou_values(cand[kept], annot[b:b + 1].astype(F32))[:, 0] >= F32(acc_thr)
            if ok.any():
                hit[b] = int(np.argmax(ok))
    res = dict(topk_boxes=boxes, topk_scores=scores, topk_idx=idx, topk_n=n)
    if annot is not None:
        res["hit_rank"] = hit
        res["acc_at"] = np.array([F32((hit <= j).sum()) / F32(B) for j in range(K)], F32)
    return res


def load_case(g, name):
    """one case of g17_topk.npz -> inputs (out5 [B, A, 5] = (reg, logit), annot, img_size, anchors, pre_n, K, nms_thr, acc_thr) and the
    expected outputs under 'want'.  The seed-only case regenerates its noise and applies the stored patches."""
    c = dict(pre_n=int(g[f"{name}_pre_n"][0]), K=int(g[f"{name}_K"][0]), nms_thr=float(g[f"{name}_nms_thr"]), acc_thr=float(g["acc_thr"]),
             annot=g[f"{name}_annot"], img_size=g[f"{name}_img_size"])
    if f"{name}_out5" in g.files:
        c["out5"], c["anchors"] = g[f"{name}_out5"], g[f"{name}_anchors"]
    else:
        ratios, scales = O.default_ratios_scales()
        c["anchors"] = O.create_anchors([tuple(x) for x in g[f"{name}_fs"].tolist()], ratios, scales).astype(F32)
        B, A = int(g[f"{name}_B"][0]), c["anchors"].shape[0]
        gen = torch.Generator().manual_seed(int(g[f"{name}_seed"][0]))
        att = torch.randn(B, A, 1, generator=gen) * 1.5 - 3.0
        bbx = torch.randn(B, A, 4, generator=gen) * 0.6
        out5 = torch.cat([bbx, att], dim=2).numpy()
        pi = g[f"{name}_patch_idx"]
        out5[pi[:, 0], pi[:, 1]] = g[f"{name}_patch_val"]
        c["out5"] = out5
    c["want"] = {k: g[f"{name}_{k}"] for k in ("topk_boxes", "topk_scores", "topk_idx", "topk_n", "hit_rank", "acc_at")}
    return c
