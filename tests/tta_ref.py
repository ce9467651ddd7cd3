"""THE definition of flip test-time augmentation (cfg eval_tta = "flip", ZSGNet.eval_tta): numpy / torch-CPU only, no GPU, no library.

A batch of B queries runs as one eval forward of 2B rows — rows 0..B-1 as given, rows B..2B-1 with the image mirrored along W, the query
vectors of `qvec_flip` (else `qvec`), the same qlens and the same h0 | c0 (`tta_batch`) — and the [2B, A, 5] head output (channels ty, tx,
th, tw, att: anchors are y1x1y2x2) is merged per anchor with its mirror partner (`partner_map`, `merge_ref`): one fp32 add (tx: subtract)
and one fp32 multiply by 0.5 per output, which numpy reproduces bit for bit."""
from typing import Dict, Sequence, Tuple

import numpy as np
import torch


def level_table(feat_sizes: Sequence[Tuple[int, int]], n: int) -> np.ndarray:
    """int32 [L, 4] of (first anchor, h, w, anchors per cell) per pyramid level: anchor (y, x, k) of a level sits at first + (y*w + x)*n + k"""
    rows, off = [], 0
    for h, w in feat_sizes:
        rows.append((off, int(h), int(w), int(n)))
        off += int(h) * int(w) * int(n)
    return np.array(rows, dtype=np.int32).reshape(-1, 4)


def partner_map(feat_sizes: Sequence[Tuple[int, int]], n: int) -> np.ndarray:
    """int64 [A]: the index of each anchor's mirror image, anchor (y, w-1-x, k) of the same level"""
    out = []
    for off, h, w, n in level_table(feat_sizes, n).tolist():
        y, x, k = np.meshgrid(np.arange(h), np.arange(w), np.arange(n), indexing="ij")
        out.append((off + (y * w + (w - 1 - x)) * n + k).reshape(-1))
    return np.concatenate(out).astype(np.int64)


def merge_ref(out5_2b: np.ndarray, feat_sizes: Sequence[Tuple[int, int]], n: int) -> np.ndarray:
    """[2B, A, 5] float32 -> [B, A, 5] float32: out[b, a] = 0.5f * (u0 + v0, u1 - v1, u2 + v2, u3 + v3, u4 + v4) with u = out5_2b[b, a],
    v = out5_2b[B + b, partner(a)]; every operation a single fp32 rounding"""
    x = np.ascontiguousarray(out5_2b, dtype=np.float32)
    assert x.ndim == 3 and x.shape[0] % 2 == 0 and x.shape[2] == 5, x.shape
    B = x.shape[0] // 2
    p = partner_map(feat_sizes, n)
    assert p.shape[0] == x.shape[1], (p.shape, x.shape)
    u, v = x[:B], x[B:][:, p]
    sign = np.array([1, -1, 1, 1, 1], dtype=np.float32)
    half = np.float32(0.5)
    with np.errstate(all="ignore"):
        s = np.where(sign > 0, u + v, u - v).astype(np.float32)
        return (half * s).astype(np.float32)


def tta_batch(inp: Dict[str, torch.Tensor], h0: torch.Tensor, c0: torch.Tensor):
    """(batch of 2B rows, h0, c0) of the one forward a flip-TTA forward of `inp` stands for; img fp32 [B,3,H,W] or uint8 [B,H,W,3].  A batch
    with img_idx (Q queries over Bi images) becomes 2Bi images, the mirrors behind the originals, and 2Q queries, the mirrored ones
    pointing at the mirrors."""
    img = inp["img"]
    wdim = 2 if img.dtype == torch.uint8 else 3
    qf = inp["qvec_flip"] if inp.get("qvec_flip") is not None else inp["qvec"]
    out = {k: v for k, v in inp.items() if k not in ("qvec_flip", "h0", "c0")}
    for k, v in inp.items():
        if torch.is_tensor(v) and k not in ("img", "qvec", "qvec_flip", "img_idx", "h0", "c0") and v.dim() >= 1 and v.shape[0] == inp["qvec"].shape[0]:
            out[k] = torch.cat([v, v])                  # (qlens, and whatever else is per query: the mirrored rows keep it)
    out["img"] = torch.cat([img, torch.flip(img, [wdim])])
    out["qvec"] = torch.cat([inp["qvec"], qf])
    if inp.get("img_idx") is not None:
        out["img_idx"] = torch.cat([inp["img_idx"], inp["img_idx"] + img.shape[0]])
    return out, torch.cat([h0, h0], dim=1), torch.cat([c0, c0], dim=1)
