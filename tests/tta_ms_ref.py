"""The definition the multi-scale test-time-augmentation tests measure against (not a test module; numpy / Pillow, no GPU, no library):

* the size rule: entry s of eval_scales adds a pass at (round(s H), round(s W)), halves rounded up;
* the resampling: PIL.Image.resize (Pillow's default bicubic, what dat_loader's integer passes reproduce) of the batch's own pixels;
* the pooled output: the passes' [B, A_s, 5] outputs along the anchor axis, pass 0 first, scored against the passes' anchor tables
  (O.create_anchors of each pass's feature sizes) back to back — the oracle's evaluator, tests/topk_ref.py and tests/vote_ref.py on
  the concatenated arrays."""
import math

import numpy as np

from oracle import zsg_oracle as O

import topk_ref
import vote_ref

F32 = np.float32


def scale_sizes(H, W, scales):
    return [(int(math.floor(s * H + 0.5)), int(math.floor(s * W + 0.5))) for s in scales]


def resample(img_u8: np.ndarray, Hs: int, Ws: int) -> np.ndarray:
    """uint8 [B, H, W, 3] -> uint8 [B, Hs, Ws, 3], image by image"""
    from PIL import Image
    return np.stack([np.asarray(Image.fromarray(im).resize((Ws, Hs))) for im in img_u8])


def pooled_anchors(tta_feat_sizes, ratios, scales) -> np.ndarray:
    """float32 [sum A_s, 4]: one create_anchors table per pass, in pass order"""
    return np.concatenate([O.create_anchors([tuple(x) for x in fs], ratios, scales).astype(F32) for fs in tta_feat_sizes], axis=0)


def evaluate(out5, annot, img_size, anchors_f32, pre_n=128, K=1, nms_thr=0.5, acc_thr=0.5, vote_thr=0.0):
    """out5 [B, sum A_s, 5] = (reg, logit) -> the oracle's evaluator on the pooled arrays; K > 1 or vote_thr > 0 add topk_ref / vote_ref"""
    att, reg = out5[..., 4].astype(F32), out5[..., :4].astype(F32)
    res = dict(O.zsg_eval(att, reg, annot, img_size, anchors_f32, acc_thr))
    if vote_thr > 0:
        res.update(vote_ref.vote(att, reg, annot, img_size, anchors_f32, pre_n, K, vote_thr, nms_thr, acc_thr))
    elif K > 1:
        res.update(topk_ref.topk(att, reg, annot, img_size, anchors_f32, pre_n, K, nms_thr, acc_thr))
    return res
