"""Evaluator on MI355X (reference `code/evaluator.py`): arg-max score anchor -> box decode -> IoU>=thr accuracy, one
HIP launch per batch (csrc/loss.hip: eval_kernel); only the two boxes per sample that are needed are decoded.

cfg eval_topk = K > 1 (an extension of this build): in eval mode the K best distinct boxes per query as well — score ranking,
greedy NMS at eval_nms_thr over the eval_pre_nms best candidates (csrc/loss.hip: zsg_eval_topk) — and Acc@K.

A multi-scale eval forward (ZSGNet.eval_scales) hands over `tta_att_bbx_out` [B, sum A_s, 5] and `tta_feat_sizes`: the same two entries
then run on that tensor against the passes' anchor tables back to back — the arg-max is the best box over all scales, the NMS removes
the object found at several of them.  cfg eval_box_vote = t in (0, 1] (eval mode only): every kept box becomes the score-weighted
mean of the candidates whose IoU with it is >= t (csrc/vote.hip: zsg_eval_vote; tests/vote_ref.py is the definition).

cfg eval_nms = "soft_linear" / "soft_gauss": the K rows are picked by Soft-NMS instead of the greedy NMS (csrc/softnms.hip:
zsg_eval_topk_soft; tests/softnms_ref.py is the definition) — a picked box decays the scores of its neighbours, topk_scores are the
decayed scores, the rows end at eval_soft_min_score; everything downstream (voting included) reads the rows as it reads the hard ones."""
from functools import partial
from typing import Dict

import torch
from torch import nn

from ._lib import lib, check, stream_ptr
from .anchors import create_anchors


class Evaluator(nn.Module):
    """To get the accuracy.  Operates at training time (reference evaluator.py:20-117)."""

    def __init__(self, ratios, scales, cfg):
        super().__init__()
        self.cfg = cfg
        self.ratios, self.scales = ratios, scales
        self.met_keys = ["Acc", "MaxPos"]
        self.anchs = None
        self.get_anchors = partial(create_anchors, ratios=self.ratios, scales=self.scales, flatten=True)
        self.acc_iou_threshold = cfg["acc_iou_threshold"]
        self.topk = int(cfg.get("eval_topk", 1))
        self.nms_thr = float(cfg.get("eval_nms_thr", 0.5))
        self.pre_nms = int(cfg.get("eval_pre_nms", 128))
        self.box_vote = check_box_vote(cfg.get("eval_box_vote", 0.0))
        self.nms, self.soft_sigma, self.soft_min_score = check_nms(cfg.get("eval_nms", "hard"), cfg.get("eval_soft_sigma", 0.5),
                                                                   cfg.get("eval_soft_min_score", 0.001))
        self._tta_anchs = {}                               # the per-pass size lists of a multi-scale output -> its concatenated anchor table
        if self.topk > 1:                                  # met_keys[0] stays Acc: checkpoint gating / the LR scheduler read it
            self.met_keys = self.met_keys + [f"Acc@{self.topk}"]

    def _out5_anchors(self, out):
        """-> (out5 [B, A, 5], the anchor table [A, 4] it is scored against); self.anchs is always the table of the batch's own resolution"""
        if "att_bbx_out" in out:
            out5 = out["att_bbx_out"].detach()
        else:
            out5 = torch.cat([out["bbx_out"], out["att_out"]], dim=2).detach()
        out5 = out5.contiguous()
        if self.anchs is None:
            fs = out["feat_sizes"]
            if "num_f_out" in out and out["num_f_out"].numel() > 1:
                fs = fs[:int(out["num_f_out"][0])]
            self.anchs = self.get_anchors(fs, device=out5.device)
        if "tta_att_bbx_out" not in out:
            return out5, self.anchs
        key = tuple(tuple((int(h), int(w)) for h, w in fs) for fs in out["tta_feat_sizes"])
        if key not in self._tta_anchs:
            self._tta_anchs[key] = torch.cat([self.get_anchors(list(fs), device=out5.device) for fs in key], dim=0).contiguous()
        return out["tta_att_bbx_out"].detach().contiguous(), self._tta_anchs[key]

    def _topk(self, out5, anchs, annot, img_size, K) -> Dict[str, torch.Tensor]:
        """one zsg_eval_topk call (zsg_eval_topk_soft under eval_nms soft_*); annot None: boxes only (no hit_rank / Acc@K)"""
        B, A, _ = out5.shape
        dev = out5.device
        boxes = torch.empty(B, K, 4, device=dev)
        scores = torch.empty(B, K, device=dev)
        self.topk_idx = torch.empty(B, K, dtype=torch.int32, device=dev)
        n = torch.empty(B, dtype=torch.int32, device=dev)
        hit = torch.empty(B, dtype=torch.int32, device=dev) if annot is not None else None
        acc = torch.empty(K, device=dev) if annot is not None else None
        if self.nms != "hard":
            nb = int(lib.zsg_eval_topk_soft_workspace_bytes(B, A, self.pre_nms, K))
            ws = torch.empty((nb + 7) // 8, dtype=torch.int64, device=dev)
            check(lib.zsg_eval_topk_soft(out5.data_ptr(), annot.data_ptr() if annot is not None else None, anchs.data_ptr(),
                                         img_size.data_ptr(), B, A, self.pre_nms, K, self.nms_thr, float(self.acc_iou_threshold),
                                         SOFT_METHODS[self.nms], self.soft_sigma, self.soft_min_score, boxes.data_ptr(),
                                         scores.data_ptr(), self.topk_idx.data_ptr(), n.data_ptr(),
                                         hit.data_ptr() if hit is not None else None, acc.data_ptr() if acc is not None else None,
                                         ws.data_ptr(), nb, stream_ptr()), "zsg_eval_topk_soft")
        else:
            ws = torch.empty((int(lib.zsg_eval_topk_workspace_bytes(B, A, self.pre_nms, K)) + 7) // 8, dtype=torch.int64, device=dev)
            check(lib.zsg_eval_topk(out5.data_ptr(), annot.data_ptr() if annot is not None else None, anchs.data_ptr(),
                                    img_size.data_ptr(), B, A, self.pre_nms, K, self.nms_thr, float(self.acc_iou_threshold),
                                    boxes.data_ptr(), scores.data_ptr(), self.topk_idx.data_ptr(), n.data_ptr(),
                                    hit.data_ptr() if hit is not None else None, acc.data_ptr() if acc is not None else None,
                                    ws.data_ptr(), stream_ptr()), "zsg_eval_topk")
        res = {"topk_boxes": boxes, "topk_scores": scores, "topk_n": n}
        if annot is not None:
            self.acc_at = acc
            res["hit_rank"] = hit
            res[f"Acc@{K}"] = acc[K - 1]
        return res

    def _vote(self, out5, anchs, annot, img_size, K, tk) -> Dict[str, torch.Tensor]:
        """one zsg_eval_vote call on the rows zsg_eval_topk kept (tk = _topk's result for the same K): the voted rows under _topk's names,
        topk_boxes_raw the rows as the NMS left them, vote_n the member counts; with annot hit_rank / Acc@K of the voted boxes"""
        B, A, _ = out5.shape
        dev = out5.device
        boxes = torch.empty(B, K, 4, device=dev)
        vn = torch.empty(B, K, dtype=torch.int32, device=dev)
        hit = torch.empty(B, dtype=torch.int32, device=dev) if annot is not None else None
        acc = torch.empty(K, device=dev) if annot is not None else None
        nb = int(lib.zsg_eval_vote_workspace_bytes(B, A, self.pre_nms, K))
        ws = torch.empty((nb + 7) // 8, dtype=torch.int64, device=dev)
        check(lib.zsg_eval_vote(out5.data_ptr(), annot.data_ptr() if annot is not None else None, anchs.data_ptr(), img_size.data_ptr(),
                                B, A, self.pre_nms, K, self.box_vote, float(self.acc_iou_threshold), tk["topk_boxes"].data_ptr(),
                                tk["topk_scores"].data_ptr(), self.topk_idx.data_ptr(), tk["topk_n"].data_ptr(), boxes.data_ptr(),
                                vn.data_ptr(), hit.data_ptr() if hit is not None else None, acc.data_ptr() if acc is not None else None,
                                ws.data_ptr(), nb, stream_ptr()), "zsg_eval_vote")
        res = dict(tk, topk_boxes=boxes, topk_boxes_raw=tk["topk_boxes"], vote_n=vn)
        if annot is not None:
            self.acc_at = acc
            res["hit_rank"] = hit
            res[f"Acc@{K}"] = acc[K - 1]
        return res

    @torch.no_grad()
    def forward(self, out: Dict[str, torch.Tensor], inp: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        annot = inp["annot"].contiguous().float()
        out5, anchs = self._out5_anchors(out)
        B, A, _ = out5.shape
        dev = out5.device
        img_size = inp["img_size"].contiguous().float()
        metrics = torch.empty(2, device=dev)
        pred_boxes = torch.empty(B, 4, device=dev)
        pred_scores = torch.empty(B, device=dev)
        self.pred_idx = torch.empty(B, dtype=torch.int32, device=dev)
        self.best_idx = torch.empty(B, dtype=torch.int32, device=dev)
        ws = torch.empty((int(lib.zsg_eval_workspace_bytes(B)) + 3) // 4, device=dev)
        check(lib.zsg_eval(out5.data_ptr(), annot.data_ptr(), anchs.data_ptr(), img_size.data_ptr(), B, A,
                           float(self.acc_iou_threshold), metrics.data_ptr(), pred_boxes.data_ptr(), pred_scores.data_ptr(),
                           self.pred_idx.data_ptr(), self.best_idx.data_ptr(), ws.data_ptr(), stream_ptr()), "zsg_eval")
        res = {"Acc": metrics[0], "MaxPos": metrics[1], "idxs": inp["idxs"], "pred_boxes": pred_boxes, "pred_scores": pred_scores}
        if self.training:                                  # nothing is added to the per-step path of training
            return res
        if self.box_vote > 0:
            K = max(1, self.topk)
            v = self._vote(out5, anchs, annot, img_size, K, self._topk(out5, anchs, annot, img_size, K))
            if self.topk == 1:
                del v["Acc@1"]                             # (K = 1 only carries the vote: Acc says the same)
            res.update(v, Acc=self.acc_at[0], pred_boxes=v["topk_boxes"][:, 0], pred_boxes_raw=pred_boxes)
        elif self.topk > 1:
            res.update(self._topk(out5, anchs, annot, img_size, self.topk))
        return res

    @torch.no_grad()
    def predict(self, out: Dict[str, torch.Tensor], inp: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """Pure inference: the eval_topk best boxes per query without ground truth (inp needs img_size only).
        -> topk_boxes [B, K, 4] pixels x1y1x2y2, topk_scores [B, K], topk_n [B]; rows past topk_n are zeros.  With eval_box_vote (in eval
        mode) the boxes are the voted ones, topk_boxes_raw the rows as the NMS left them and vote_n [B, K] the member counts."""
        out5, anchs = self._out5_anchors(out)
        img_size = inp["img_size"].contiguous().float()
        K = max(1, self.topk)
        tk = self._topk(out5, anchs, None, img_size, K)
        if self.box_vote > 0 and not self.training:
            return self._vote(out5, anchs, None, img_size, K, tk)
        return tk


def check_box_vote(v) -> float:
    """cfg eval_box_vote: 0 (off) or an IoU threshold in (0, 1]; ValueError otherwise"""
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not (v == 0 or 0 < v <= 1):
        raise ValueError(f"eval_box_vote={v!r}: expected 0 (off) or an IoU threshold in (0, 1]")
    return float(v)


SOFT_METHODS = {"soft_linear": 1, "soft_gauss": 2}      # zsg_eval_topk_soft's method argument


def check_nms(nms, sigma, min_score):
    """cfg eval_nms / eval_soft_sigma / eval_soft_min_score -> (nms, sigma, min_score); ValueError for anything zsg_eval_topk_soft refuses"""
    if not isinstance(nms, str) or (nms != "hard" and nms not in SOFT_METHODS):
        raise ValueError(f"eval_nms={nms!r}: expected 'hard', 'soft_linear' or 'soft_gauss'")
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not (0 < sigma < float("inf")):
        raise ValueError(f"eval_soft_sigma={sigma!r}: expected a finite number > 0")
    if isinstance(min_score, bool) or not isinstance(min_score, (int, float)) or not (0 <= min_score < 1):
        raise ValueError(f"eval_soft_min_score={min_score!r}: expected a number in [0, 1)")
    return nms, float(sigma), float(min_score)


def get_default_eval(ratios, scales, cfg):
    return Evaluator(ratios, scales, cfg)
