"""Batch producer for real datasets — counterpart of the reference's `code/dat_loader.py`.

Contract kept (dat_loader.py:98-146, 187-196): a CSV with columns `img_id, bbox, query` (bbox "[x1, y1, x2, y2]" in
pixels, query a string or a list literal of strings); one sample = the image resized to cfg.resize_img with PIL, the
query as `phrase_len` = 50 word vectors (the text is padded with ' PD' tokens; `qlens` = number of real tokens), the box
as y1x1y2x2 normalised to [-1, 1]; the collater stacks every field as float and cuts `qvec` to the longest query of the
batch.

What is different, and why:
  * word vectors come from a pluggable embedder: spaCy (`en_core_web_md`, as the reference) when it is installed, else a
    word-vector table file (cfg.word_vectors: .npz with `words` [V] and `vectors` [V, emb_dim]); spaCy is not available
    offline, so the table path is what the tests exercise;
  * with `gpu_normalise` the image travels as uint8 HWC (4x fewer PCIe bytes, pinned memory, copied on a side stream by
    `DevicePrefetcher`) and `/255` + the NHWC4 layout happen in one HIP kernel (`zsg_u8hwc_to_nhwc4`) — bit-identical to
    `pil2tensor(...).float().div_(255)` (dat_loader.py:26-33, 134);
  * dataset names other than the two the reference's `_read_annotations` knows (dat_loader.py:176-184 leaves `trn_df`
    undefined for flickr30k_c0/c1, vg_split_*) work: flickr30k* ids get the '.jpg' suffix, everything else is a path.
"""
import ast
import collections
import functools
import math
import re
from pathlib import Path
from typing import Dict, Iterator, List, Optional, Tuple

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset
from torch.utils.data.distributed import DistributedSampler

PHRASE_LEN = 50            # dat_loader.py:88
PAD_TOKEN = "PD"           # dat_loader.py:110


# ---------------------------------------------------------------------------------------------------------------------
# word vectors
# ---------------------------------------------------------------------------------------------------------------------
class SpacyEmbedder:
    """The reference's tokeniser + vectors (dat_loader.py:23, 105-115)."""

    def __init__(self, model: str = "en_core_web_md"):
        import spacy                    # raises ImportError when absent: the caller then needs cfg.word_vectors
        self.nlp = spacy.load(model)

    def tokens(self, text: str) -> List[str]:
        return [t.text for t in self.nlp(text)]

    def vectors(self, text: str) -> np.ndarray:
        return np.array([t.vector for t in self.nlp(text)], dtype=np.float32)


class TableEmbedder:
    """Word-vector table: tokens are runs of word characters or single punctuation marks; unknown words (and the pad
    token, unless the table has it) map to the zero vector, as spaCy does for out-of-vocabulary tokens."""
    _tok = re.compile(r"\w+|[^\w\s]", re.UNICODE)

    def __init__(self, path: str, emb_dim: int = 300):
        z = np.load(path, allow_pickle=False)
        self.index = {str(w): i for i, w in enumerate(z["words"])}
        self.table = np.asarray(z["vectors"], dtype=np.float32)
        assert self.table.ndim == 2 and self.table.shape[1] == emb_dim, f"{path}: vectors must be [V, {emb_dim}]"
        self.emb_dim = emb_dim

    def tokens(self, text: str) -> List[str]:
        return self._tok.findall(text)

    def vectors(self, text: str) -> np.ndarray:
        toks = self.tokens(text)
        out = np.zeros((len(toks), self.emb_dim), np.float32)
        for i, t in enumerate(toks):
            j = self.index.get(t, self.index.get(t.lower(), -1))
            if j >= 0:
                out[i] = self.table[j]
        return out


def get_embedder(cfg):
    path = cfg["word_vectors"] if "word_vectors" in cfg else ""
    if path:
        return TableEmbedder(path, int(cfg["emb_dim"]))
    try:
        return SpacyEmbedder()
    except ImportError as e:
        raise RuntimeError("no word vectors: spaCy is not installed and cfg.word_vectors (a .npz with `words`, `vectors`) is empty") from e


def embed_query(embedder, query: str, phrase_len: int = PHRASE_LEN) -> Tuple[np.ndarray, int]:
    """dat_loader.py:104-115: -> ([phrase_len, emb] float32, number of real tokens)."""
    query = query.strip()
    qlen = len(embedder.tokens(query))
    if qlen == 0:
        raise NotImplementedError("empty query")               # as the reference (dat_loader.py:106-108)
    vecs = embedder.vectors(query + (" " + PAD_TOKEN) * (phrase_len - qlen))[:phrase_len]
    assert vecs.shape[0] == phrase_len, "tokenisation of the padded query is not stable"
    return vecs, qlen


# ---------------------------------------------------------------------------------------------------------------------
# GPU-side resize: PIL.Image.resize's default filter reproduced bit for bit on uint8
# ---------------------------------------------------------------------------------------------------------------------
_RESIZE_PRECISION_BITS = 32 - 8 - 2          # Pillow's Resample.c: 8-bit channels are filtered in 22-bit fixed point


def _bicubic(x: float) -> float:
    """Pillow's bicubic kernel (a = -0.5), evaluated in double precision in ITS operation order"""
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@functools.lru_cache(maxsize=4096)
def resize_tables(in_size: int, out_size: int):
    """The per-axis tap tables `img.resize((W, H))` — the reference's only resampling call, dat_loader.py:121, PIL's default filter
    (bicubic for RGB) — uses for one axis: Pillow's precompute_coeffs + normalize_coeffs_8bpc restated (double-precision weights
    normalised to sum 1, then rounded to 22-bit fixed point).  Returns (bounds int32 [out, 2] = first tap, tap count; coefficients
    int32 [out, ksize]; ksize).  The HIP kernel zsg_resize_u8 accumulates these integers exactly as Pillow does, so its uint8 output
    is bit-identical to Pillow's (tests/test_cpu_loader.py pins the tables against Pillow itself, tests/test_gpu_trainer.py the kernel)."""
    scale = float(np.float32(in_size) - np.float32(0.0)) / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    # every output position at once; per element the SAME double-precision operations in the same order as Pillow's loops
    # (a random augmentation crop needs two new tables per image: a Python loop per output position cost the consumer thread ~1 ms each)
    center = 0.0 + (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)                      # (int): truncation
    cnt = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    taps = np.arange(ksize, dtype=np.int64)[None, :]
    x = np.abs(((taps + xmin[:, None]) - center[:, None] + 0.5) * ss)
    a = -0.5
    k = np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))      # _bicubic
    k = np.where(taps < cnt[:, None], k, 0.0)
    ww = np.zeros(out_size, np.float64)
    for t in range(ksize):                                                               # the sum in tap order, as Pillow adds it
        ww = ww + k[:, t]
    k = np.where((ww != 0.0)[:, None], k / np.where(ww != 0.0, ww, 1.0)[:, None], k)
    v = k * (1 << _RESIZE_PRECISION_BITS)
    coef = np.where(k < 0, (-0.5 + v).astype(np.int64), (0.5 + v).astype(np.int64)).astype(np.int32)
    bounds = np.stack([xmin, cnt], 1).astype(np.int32)
    return bounds, coef, ksize


def flatten_raw(imgs) -> Tuple[torch.Tensor, torch.Tensor]:
    """Raw uint8 [h, w, 3] images of different sizes -> (one flat uint8 tensor, int32 [B, 2] heights / widths): what the collater hands on
    in gpu_resize mode — the DataLoader's pin thread pins ONE tensor and the trainer uploads it with ONE copy (a list of B tensors cost
    the trainer thread a pin_memory() + a copy per image)."""
    hw = torch.tensor([[int(im.shape[0]), int(im.shape[1])] for im in imgs], dtype=torch.int32)
    return torch.cat([im.reshape(-1) for im in imgs]), hw


# ---------------------------------------------------------------------------------------------------------------------
# training augmentation: box-safe random crop + colour jitter, zoom-out onto a filled canvas, phrase-aware horizontal flip.  The host
# definition (exact to the byte); the HIP kernels of csrc/aug.hip (zsg_augment_u8_batched and, for flips and windows that leave the
# image, zsg_augment_geom_u8_batched, driven by GpuResizer.resize_flat) reproduce augment_host bit for bit.
# ---------------------------------------------------------------------------------------------------------------------
AUG_KEYS = {"aug_crop_min": 1.0, "aug_brightness": 0.0, "aug_contrast": 0.0, "aug_saturation": 0.0}      # the defaults: off


def aug_params(cfg) -> Tuple[float, float, float, float]:
    """the four aug_* keys of cfg (a cfg without them = the defaults), validated: ValueError outside their ranges"""
    cmin, vb, vc, vs = (float(cfg[k]) if k in cfg else d for k, d in AUG_KEYS.items())
    if not (0.0 < cmin <= 1.0):
        raise ValueError(f"aug_crop_min = {cmin}: must lie in (0, 1]")
    for k, v in (("aug_brightness", vb), ("aug_contrast", vc), ("aug_saturation", vs)):
        if not (0.0 <= v < math.inf):
            raise ValueError(f"{k} = {v}: must be >= 0 (and finite)")
    return cmin, vb, vc, vs


AUG_GEOM_KEYS = {"aug_flip": 0.0, "aug_expand_max": 1.0, "aug_fill": (124, 116, 104)}      # the defaults: off (aug_fill: the ImageNet mean)


def aug_geom_params(cfg) -> Tuple[float, float, Tuple[int, int, int]]:
    """aug_flip, aug_expand_max, aug_fill of cfg (a cfg without them = the defaults), validated: ValueError outside their ranges"""
    pflip = float(cfg["aug_flip"]) if "aug_flip" in cfg else AUG_GEOM_KEYS["aug_flip"]
    emax = float(cfg["aug_expand_max"]) if "aug_expand_max" in cfg else AUG_GEOM_KEYS["aug_expand_max"]
    fill = cfg["aug_fill"] if "aug_fill" in cfg else AUG_GEOM_KEYS["aug_fill"]
    if not (0.0 <= pflip <= 1.0):
        raise ValueError(f"aug_flip = {pflip}: a probability, must lie in [0, 1]")
    if not (1.0 <= emax <= 4.0):
        raise ValueError(f"aug_expand_max = {emax}: must lie in [1, 4]")
    return pflip, emax, _check_fill(fill, "aug_fill")


def _check_fill(fill, name: str) -> Tuple[int, int, int]:
    try:
        vals = [v for v in fill]
        ok = len(vals) == 3 and all(float(v) == int(v) and 0 <= int(v) <= 255 and not isinstance(v, bool) for v in vals)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{name} = {fill!r}: three integers 0..255 (RGB)")
    return tuple(int(v) for v in vals)


AUG_WARP_KEYS = {"aug_rotate": 0.0, "aug_shear": 0.0, "aug_warp_keep": 0.8, "aug_blur": 0.0, "aug_blur_p": 0.5}      # the defaults: off


def aug_warp_params(cfg) -> Tuple[float, float, float, float, float]:
    """aug_rotate, aug_shear, aug_warp_keep, aug_blur, aug_blur_p of cfg (a cfg without them = the defaults), validated: ValueError
    outside their ranges"""
    rot, shear, keep, blur, blur_p = (float(cfg[k]) if k in cfg else d for k, d in AUG_WARP_KEYS.items())
    if not (0.0 <= rot <= 30.0):
        raise ValueError(f"aug_rotate = {rot}: degrees, must lie in [0, 30]")
    if not (0.0 <= shear <= 20.0):
        raise ValueError(f"aug_shear = {shear}: degrees, must lie in [0, 20]")
    if not (0.0 < keep <= 1.0):
        raise ValueError(f"aug_warp_keep = {keep}: must lie in (0, 1]")
    if not (blur == 0.0 or BLUR_SIGMA_MIN <= blur <= 2.5):
        raise ValueError(f"aug_blur = {blur}: 0 (off), or a sigma in [{BLUR_SIGMA_MIN}, 2.5] output pixels")
    if not (0.0 <= blur_p <= 1.0):
        raise ValueError(f"aug_blur_p = {blur_p}: a probability, must lie in [0, 1]")
    return rot, shear, keep, blur, blur_p


def aug_warp_enabled(cfg) -> bool:
    rot, shear, _, blur, _ = aug_warp_params(cfg)
    return rot > 0.0 or shear > 0.0 or blur > 0.0


def aug_enabled(cfg) -> bool:
    pflip, emax, _ = aug_geom_params(cfg)
    return aug_params(cfg) != tuple(AUG_KEYS.values()) or pflip > 0.0 or emax > 1.0 or aug_warp_enabled(cfg)


def _draw_window(rng, h: int, w: int, boxes, cmin: float):
    """the box-safe random window of an h x w area: cw, ch, x0, y0 in this order"""
    cw = max(1, int(round(w * rng.uniform(cmin, 1.0))))
    ch = max(1, int(round(h * rng.uniform(cmin, 1.0))))
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    xs, ys = np.clip(b[:, [0, 2]], 0, w), np.clip(b[:, [1, 3]], 0, h)
    X1, X2, Y1, Y2 = int(math.floor(xs.min())), int(math.ceil(xs.max())), int(math.floor(ys.min())), int(math.ceil(ys.max()))
    cw, ch = min(w, max(cw, X2 - X1, 1)), min(h, max(ch, Y2 - Y1, 1))
    x0 = int(rng.randint(max(0, X2 - cw), min(X1, w - cw) + 1))           # never empty: cw >= X2 - X1, X2 <= w, cw <= w
    y0 = int(rng.randint(max(0, Y2 - ch), min(Y1, h - ch) + 1))
    return x0, y0, x0 + cw, y0 + ch


def _draw_factors(rng, vb: float, vc: float, vs: float) -> np.ndarray:
    f = [np.float32(rng.uniform(max(0.0, 1.0 - v), 1.0 + v)) if v > 0 else np.float32(1.0) for v in (vb, vc, vs)]
    return np.array(f, np.float32)


def draw_augment(rng, h: int, w: int, boxes, cfg):
    """One random augmentation of a decoded h x w image whose queries have the pixel boxes `boxes` ([x1, y1, x2, y2] each): None when
    the aug_* keys are at their defaults, else (crop, jitter) with crop = (x0, y0, x0 + cw, y0 + ch) integers — inside the image and
    holding every box (clipped to the image) — and jitter = float32 (brightness, contrast, saturation) factors.  rng: numpy's
    uniform / randint interface (np.random, a RandomState).  Draw order: cw, ch, x0, y0, then the three factors; a part that is off
    draws nothing.  (aug_flip / aug_expand_max are not read here: draw_augment_geom.)"""
    cmin, vb, vc, vs = aug_params(cfg)
    if (cmin, vb, vc, vs) == tuple(AUG_KEYS.values()):
        return None
    h, w = int(h), int(w)
    crop = _draw_window(rng, h, w, boxes, cmin) if cmin < 1.0 else (0, 0, w, h)
    return crop, _draw_factors(rng, vb, vc, vs)


def draw_augment_geom(rng, h: int, w: int, boxes, cfg):
    """draw_augment with the zoom-out and the flip: None when all seven aug_* keys are off, else (crop, jitter, flip).  Draw order — a part
    that is off draws nothing, so with aug_flip = 0 and aug_expand_max = 1 this consumes exactly draw_augment's random numbers and
    returns its (crop, jitter) plus False:
      1. aug_expand_max > 1: r = uniform(1, aug_expand_max); the image lies on a canvas W = max(w, round(w r)), H = max(h, round(h r)) at
         ox = randint(0, W - w + 1), oy = randint(0, H - h + 1);
      2. aug_crop_min < 1: draw_augment's box-safe window (cw, ch, x0, y0) on the canvas, the boxes shifted by (ox, oy); else the window
         is the whole canvas;
      3. the brightness, contrast and saturation factors;
      4. aug_flip > 0: flip = uniform() < aug_flip.
    crop is in IMAGE coordinates, (x0 - ox, y0 - oy, x1 - ox, y1 - oy): integers that may be negative or beyond the image — what lies
    outside is aug_fill (augment_host(..., fill=...))."""
    cmin, vb, vc, vs = aug_params(cfg)
    pflip, emax, _ = aug_geom_params(cfg)
    if (cmin, vb, vc, vs) == tuple(AUG_KEYS.values()) and pflip <= 0.0 and emax <= 1.0:
        return None
    return _draw_geom(rng, h, w, boxes, cmin, vb, vc, vs, pflip, emax)


def _draw_geom(rng, h: int, w: int, boxes, cmin, vb, vc, vs, pflip, emax):
    """steps 1-4 of draw_augment_geom, whatever is on"""
    h, w = int(h), int(w)
    W, H, ox, oy = w, h, 0, 0
    if emax > 1.0:
        r = rng.uniform(1.0, emax)
        W, H = max(w, int(round(w * r))), max(h, int(round(h * r)))
        ox, oy = int(rng.randint(0, W - w + 1)), int(rng.randint(0, H - h + 1))
    if cmin < 1.0:
        b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4) + np.array([ox, oy, ox, oy], np.float64)
        x0, y0, x1, y1 = _draw_window(rng, H, W, b, cmin)
    else:
        x0, y0, x1, y1 = 0, 0, W, H
    jitter = _draw_factors(rng, vb, vc, vs)
    flip = bool(rng.uniform() < pflip) if pflip > 0.0 else False
    return (x0 - ox, y0 - oy, x1 - ox, y1 - oy), jitter, flip


# ---- affine warp (rotation + shear about the centre of the OUTPUT) and Gaussian blur: steps 6 and 7 of augment_host ------------------
WARP_IDENTITY = (65536, 0, 0, 0, 65536, 0)
BLUR_SIGMA_MIN = 0.1
BLUR_MAX_RADIUS = 8


def _q16(v: float) -> int:
    return int(math.floor(v * 65536.0 + 0.5))


def _warp_forward(theta: float, shear: float):
    """M = R(theta) S(shear), degrees: R = [[cos, -sin], [sin, cos]] (x right, y down: a positive theta turns the picture clockwise on
    screen), S = [[1, tan], [0, 1]]; det M = 1"""
    t, s = math.radians(theta), math.radians(shear)
    c, sn, tn = math.cos(t), math.sin(t), math.tan(s)
    return (c, c * tn - sn), (sn, sn * tn + c)


def warp_matrix(theta: float, shear: float, out_hw) -> Tuple[int, int, int, int, int, int]:
    """The six 16.16 integers (a, b, c0, d, e, c1) of the warp p' = c + M (p - c), c = (Wo / 2, Ho / 2), M = R(theta) S(shear): output
    pixel (x, y) samples the source at SU = a x + b y + c0, SV = d x + e y + c1 — the inverse map through pixel centres,
    u = Mi (x + 0.5 - cx) + cx - 0.5 — computed in float64 and rounded with q(v) = floor(v 65536 + 0.5)."""
    Ho, Wo = int(out_hw[0]), int(out_hw[1])
    (m00, m01), (m10, m11) = _warp_forward(theta, shear)
    i00, i01, i10, i11 = m11, -m01, -m10, m00                                            # M^-1 (det M = 1)
    cx, cy = Wo / 2.0, Ho / 2.0
    c0 = cx - 0.5 + i00 * (0.5 - cx) + i01 * (0.5 - cy)
    c1 = cy - 0.5 + i10 * (0.5 - cx) + i11 * (0.5 - cy)
    return _q16(i00), _q16(i01), _q16(c0), _q16(i10), _q16(i11), _q16(c1)


def warp_box(box, theta: float, shear: float, out_hw, win_hw, keep: Optional[float] = None):
    """The box of a warped image.  box = (x1, y1, x2, y2) in WINDOW pixels (as query_item has it after crop and flip), win_hw = the window's
    (height, width): scaled to output pixels, its four corners mapped forward with M, their bounding box clipped to [0, Wo] x [0, Ho] and
    scaled back to window pixels.  keep: the draw is refused — None is returned — when the clipped bounding box has less than `keep`
    of the unclipped one's area (keep = None: never refused)."""
    Ho, Wo = float(out_hw[0]), float(out_hw[1])
    ch, cw = float(win_hw[0]), float(win_hw[1])
    sx, sy = Wo / cw, Ho / ch
    (m00, m01), (m10, m11) = _warp_forward(theta, shear)
    cx, cy = Wo / 2.0, Ho / 2.0
    pts = [(float(box[i]) * sx - cx, float(box[j]) * sy - cy) for i in (0, 2) for j in (1, 3)]
    xs, ys = [cx + m00 * x + m01 * y for x, y in pts], [cy + m10 * x + m11 * y for x, y in pts]
    x1, y1, x2, y2 = min(xs), min(ys), max(xs), max(ys)
    kx1, ky1 = min(max(x1, 0.0), Wo), min(max(y1, 0.0), Ho)
    kx2, ky2 = max(min(x2, Wo), kx1), max(min(y2, Ho), ky1)
    if keep is not None and (kx2 - kx1) * (ky2 - ky1) < keep * ((x2 - x1) * (y2 - y1)):
        return None
    return kx1 / sx, ky1 / sy, kx2 / sx, ky2 / sy


def settle_warp(theta: float, shear: float, boxes, out_hw, win_hw, keep: float):
    """The box rule: (theta, shear) is accepted when warp_box keeps every box; else both are halved and tested again, at most four
    halvings; then the warp is dropped (None).  No random numbers."""
    for _ in range(5):
        if all(warp_box(b, theta, shear, out_hw, win_hw, keep) is not None for b in boxes):
            return theta, shear
        theta, shear = theta / 2.0, shear / 2.0
    return None


def blur_taps(sigma: float):
    """(r, taps) of the separable Gaussian blur: r = min(8, ceil(3 sigma)), taps = int64 [2 r + 1], the float64 weights exp(-k^2 / 2 sigma^2)
    normalised over k = -r .. r, rounded to 16 bits (floor(w 65536 + 0.5)), the centre tap adjusted so that they sum to exactly 65536"""
    sigma = float(sigma)
    if not (0.0 < sigma < math.inf):
        raise ValueError(f"blur_taps: sigma = {sigma} must be positive")
    r = min(BLUR_MAX_RADIUS, int(math.ceil(3.0 * sigma)))
    w = np.exp(-(np.arange(-r, r + 1, dtype=np.float64) ** 2) / (2.0 * sigma * sigma))
    w /= w.sum()
    t = np.floor(w * 65536.0 + 0.5).astype(np.int64)
    t[r] += 65536 - int(t.sum())
    return r, t


def warp_host(img: np.ndarray, m, fill) -> np.ndarray:
    """step 6 of augment_host: uint8 [Ho, Wo, 3] warped by the six 16.16 integers m (warp_matrix), taps outside the image = fill"""
    Ho, Wo = img.shape[:2]
    a, b, c0, d, e, c1 = (np.int64(int(v)) for v in m)
    y, x = np.mgrid[0:Ho, 0:Wo].astype(np.int64)
    SU, SV = a * x + b * y + c0, d * x + e * y + c1
    ix, iy = SU >> 16, SV >> 16
    fx, fy = ((SU >> 8) & 255)[..., None], ((SV >> 8) & 255)[..., None]
    fillv = np.array(_check_fill(fill, "warp_host: fill"), np.int64)

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < Wo) & (yy >= 0) & (yy < Ho)
        return np.where(ok[..., None], img[np.clip(yy, 0, Ho - 1), np.clip(xx, 0, Wo - 1)].astype(np.int64), fillv)
    p00, p01, p10, p11 = tap(iy, ix), tap(iy, ix + 1), tap(iy + 1, ix), tap(iy + 1, ix + 1)
    return (((p00 * (256 - fx) + p01 * fx) * (256 - fy) + (p10 * (256 - fx) + p11 * fx) * fy + 32768) >> 16).astype(np.uint8)


def blur_host(img: np.ndarray, sigma: float) -> np.ndarray:
    """step 7 of augment_host: blur_taps(sigma) along x, then along y, the index clamped to the image"""
    r, t = blur_taps(sigma)
    out = img
    for axis in (1, 0):
        n = out.shape[axis]
        acc = np.full(out.shape, 32768, np.int64)
        for k in range(-r, r + 1):
            acc += t[k + r] * np.take(out, np.clip(np.arange(n) + k, 0, n - 1), axis=axis).astype(np.int64)
        out = (acc >> 16).astype(np.uint8)
    return out


def draw_augment_warp(rng, h: int, w: int, boxes, cfg, out_hw):
    """draw_augment_geom with the warp and the blur: None when every aug_* key is off, else (crop, jitter, flip, warp, sigma) — warp =
    the settled (theta, shear) in degrees or None (keys off, or the draw dropped by the box rule), sigma = the blur's or None.  Draw
    order: draw_augment_geom's steps 1-4, then
      5. aug_rotate > 0: theta = uniform(-aug_rotate, aug_rotate);  6. aug_shear > 0: shear = uniform(-aug_shear, aug_shear);
      7. aug_blur > 0: u = uniform(), sigma = uniform(0.1, aug_blur) rounded to float32 — both always drawn; the blur is applied when
         u < aug_blur_p.
    A part that is off draws nothing: with the new keys off this consumes exactly draw_augment_geom's random numbers.  The box rule
    (settle_warp over all `boxes`, taken to window pixels and mirrored as query_item does) costs no random numbers."""
    cmin, vb, vc, vs = aug_params(cfg)
    pflip, emax, _ = aug_geom_params(cfg)
    rot, shear, keep, blur, blur_p = aug_warp_params(cfg)
    if (cmin, vb, vc, vs) == tuple(AUG_KEYS.values()) and pflip <= 0.0 and emax <= 1.0 and not (rot > 0.0 or shear > 0.0 or blur > 0.0):
        return None
    crop, jitter, flip = _draw_geom(rng, h, w, boxes, cmin, vb, vc, vs, pflip, emax)
    warp = sigma = None
    if rot > 0.0 or shear > 0.0:
        theta = float(rng.uniform(-rot, rot)) if rot > 0.0 else 0.0
        phi = float(rng.uniform(-shear, shear)) if shear > 0.0 else 0.0
        x0, y0, x1, y1 = crop
        b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4) - np.array([x0, y0, x0, y0], np.float64)
        if flip:
            b[:, [0, 2]] = (x1 - x0) - b[:, [2, 0]]
        warp = settle_warp(theta, phi, b.tolist(), out_hw, (y1 - y0, x1 - x0), keep)
    if blur > 0.0:
        u, s = rng.uniform(), rng.uniform(BLUR_SIGMA_MIN, blur)
        sigma = float(np.float32(s)) if u < blur_p else None          # (float32: what the item's aug_blur field carries to the GPU path)
    return crop, jitter, flip, warp, sigma


_LR_WORDS = {"left": "right", "leftmost": "rightmost", "lefthand": "righthand"}
_LR_WORDS.update({v: k for k, v in list(_LR_WORDS.items())})
_LR_RE = re.compile(r"\b(" + "|".join(sorted(_LR_WORDS, key=len, reverse=True)) + r")\b", re.IGNORECASE)


def swap_left_right(text: str) -> str:
    """the query of a mirrored image: left <-> right, leftmost <-> rightmost, lefthand <-> righthand — whole words, any case, the token's
    capitalisation style kept (Left -> Right, LEFT -> RIGHT); everything else ("bright", "leftover") is left alone"""
    def sub(m):
        tok = m.group(0)
        new = _LR_WORDS[tok.lower()]
        return new.upper() if tok.isupper() else (new.capitalize() if tok[0].isupper() else new)
    return _LR_RE.sub(sub, text)


def _resize_pass_host(src: np.ndarray, n_out: int) -> np.ndarray:
    """one pass of Pillow's 8-bit resampler along axis 0 of uint8 [n_in, m, 3], with resize_tables' integers (an unchanged length:
    Pillow skips the pass)"""
    n_in = src.shape[0]
    if n_in == n_out:
        return src
    bounds, coef, ks = resize_tables(n_in, n_out)
    idx = np.minimum(bounds[:, :1] + np.arange(ks, dtype=np.int32)[None], n_in - 1)      # taps past the count have coefficient 0
    acc = np.int32(1 << 21) + (src[idx].astype(np.int32) * coef[:, :, None, None]).sum(axis=1, dtype=np.int32)
    return np.clip(acc >> 22, 0, 255).astype(np.uint8)


_GRAY = (np.float32(0.2989), np.float32(0.587), np.float32(0.114))


def _gray_host(p: np.ndarray) -> np.ndarray:
    """trunc((0.2989 r + 0.587 g) + 0.114 b) of float32 [..., 3], every product and sum rounded to fp32"""
    return np.trunc((_GRAY[0] * p[..., 0] + _GRAY[1] * p[..., 1]) + _GRAY[2] * p[..., 2])


def _blend_host(x: np.ndarray, m, f: np.float32) -> np.ndarray:
    """trunc(clamp(f * x + (1 - f) * m, 0, 255)) in fp32, no fused multiply-add (numpy rounds every operation)"""
    return np.trunc(np.clip(f * x + (np.float32(1.0) - f) * m, np.float32(0.0), np.float32(255.0)))


def augment_host(img_u8_hwc: np.ndarray, crop, jitter, out_hw, flip: bool = False, fill=None, warp=None, blur: float = 0.0) -> np.ndarray:
    """THE definition of the training augmentation: uint8 [h, w, 3] -> uint8 [Ho, Wo, 3].
    1. Pillow's `img.crop(crop).resize((Wo, Ho))`: the tap tables of the crop's side lengths applied to the window (taps stop at the
       window's edge, not the image's).  fill = (r, g, b): the window may reach outside the image on any side (x0 < x1, y0 < y1, any
       sign) — `canvas.crop(crop).resize((Wo, Ho))` with the image pasted on a `fill`-coloured canvas that covers the window: the same
       two passes over the window's pixels, of which those outside the image are `fill`.  fill = None: a window that is not inside the
       image is a ValueError;
    2. brightness: blend(x, 0, b);  3. contrast: blend(x, mean, c), mean = the exact integer sum of gray over the image after step 2,
       divided by Ho * Wo in double precision and rounded once to fp32;  4. saturation: blend(x, gray(pixel after step 3), s);
    with blend(x, m, f) = trunc(clamp(f * x + (1 - f) * m, 0, 255)) and gray = trunc((0.2989 r + 0.587 g) + 0.114 b), all in fp32 with
    every product and sum rounded separately.  A factor of exactly 1 is the identity.
    5. flip: the result mirrored left-right, out[:, ::-1] — last (steps 2 and 4 are per pixel and the mean of step 3 is an exact
       integer sum, so any earlier place gives the same bytes).
    6. warp = six 16.16 integers (warp_matrix; None or WARP_IDENTITY: nothing happens): the affine warp about the image centre, all in
       integers — for output pixel (x, y): SU = a x + b y + c0, SV = d x + e y + c1 (exact), ix = SU >> 16, fx = (SU >> 8) & 255,
       likewise iy, fy; the taps (iy, ix), (iy, ix + 1), (iy + 1, ix), (iy + 1, ix + 1) of the step-5 image, `fill` where a tap lies
       outside it (a warp needs fill); v = ((p00 (256 - fx) + p01 fx)(256 - fy) + (p10 (256 - fx) + p11 fx) fy + 32768) >> 16.
    7. blur = sigma in output pixels (0: nothing happens): blur_taps(sigma) along x, then along y, each pass
       (sum_k t_k p[clamp(i + k, 0, n - 1)] + 32768) >> 16."""
    Ho, Wo = int(out_hw[0]), int(out_hw[1])
    a = np.asarray(img_u8_hwc)
    assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3, "augment_host: uint8 [h, w, 3]"
    x0, y0, x1, y1 = (int(v) for v in crop)
    if fill is None:
        if not (0 <= x0 < x1 <= a.shape[1] and 0 <= y0 < y1 <= a.shape[0]):
            raise ValueError(f"augment_host: crop {(x0, y0, x1, y1)} is not inside the {a.shape[0]} x {a.shape[1]} image")
        win = a[y0:y1, x0:x1]
    else:
        if not (x0 < x1 and y0 < y1):
            raise ValueError(f"augment_host: crop {(x0, y0, x1, y1)} is empty")
        win = np.empty((y1 - y0, x1 - x0, 3), np.uint8)
        win[:] = np.array(_check_fill(fill, "augment_host: fill"), np.uint8)
        ix0, iy0, ix1, iy1 = max(x0, 0), max(y0, 0), min(x1, a.shape[1]), min(y1, a.shape[0])      # the window's part inside the image
        if ix0 < ix1 and iy0 < iy1:
            win[iy0 - y0:iy1 - y0, ix0 - x0:ix1 - x0] = a[iy0:iy1, ix0:ix1]
    win = _resize_pass_host(win.transpose(1, 0, 2), Wo).transpose(1, 0, 2)        # horizontal pass first, as Pillow
    p = _resize_pass_host(win, Ho).astype(np.float32)
    fb, fc, fs = (np.float32(v) for v in jitter)
    p = _blend_host(p, np.float32(0.0), fb)
    mean = np.float32(np.float64(int(_gray_host(p).astype(np.int64).sum())) / np.float64(Ho * Wo))
    p = _blend_host(p, mean, fc)
    p = _blend_host(p, _gray_host(p)[..., None], fs)
    out = p.astype(np.uint8)
    out = np.ascontiguousarray(out[:, ::-1]) if flip else out
    if warp is not None and tuple(int(v) for v in warp) != WARP_IDENTITY:
        if fill is None:
            raise ValueError("augment_host: a warp needs fill, the colour of the taps outside the image")
        out = warp_host(out, warp, fill)
    if blur:
        out = blur_host(out, blur)
    return out


class GpuResizer:
    """Resizes raw uint8 HWC images of ANY size to one [B, H, W, 3] uint8 batch on the GPU (Pillow's two-pass fixed-point bicubic, bit-
    identical to PIL.Image.resize's default filter, dat_loader.py:121).  The tap tables of an axis length are computed once on the host
    and kept on the device.  Round 5: the whole batch is resized by TWO launches (zsg_resize_u8_batched) from one job table — the
    per-image form (one call, two launches and one upload per image) capped the consumer at 3 680 img/s with sixteen workers."""

    def __init__(self, out_hw, device="cuda"):
        self.Ho, self.Wo, self.dev = int(out_hw[0]), int(out_hw[1]), device
        self._tab = collections.OrderedDict()          # (axis length in, out) -> device tap tables, least recently used first
        self._tmp = None
        self._gray = None
        self._jobs_host = None
        self.launches = {"augment_u8": 0, "augment_geom_u8": 0}      # calls of zsg_augment_u8_batched / zsg_augment_geom_u8_batched
        self._warp_src = self._warp_tmp = None         # scratch batches of the warp / blur launches: allocated by the first batch that has one
        self.warp_calls = 0                            # calls of zsg_augment_warp_u8_batched
        import PIL
        if tuple(int(v) for v in PIL.__version__.split(".")[:2]) < (7, 0):      # (Pillow < 7 resizes with NEAREST by default: the two paths would differ)
            raise RuntimeError("GpuResizer reproduces PIL.Image.resize's default filter of Pillow >= 7 (bicubic); found Pillow " + PIL.__version__)

    TABLE_CACHE = 4096          # device tap tables kept (as resize_tables' lru_cache): crop sides vary per sample

    def _tables(self, n_in, n_out, identity_ok=True):
        """device tap tables (bounds, coefficients, ksize) of one axis; an axis that keeps its length gets the identity table (one tap,
        2^22: the batched launches run both passes for every image, Pillow skips that pass — the same bytes)"""
        self._ensure_tables([(n_in, n_out)])
        return self._tab[(n_in, n_out)]

    def _ensure_tables(self, keys):
        """All tables of a batch that are not on the device yet travel in ONE pinned, asynchronous upload (random crops bring two new
        axis lengths per image).  The cache is bounded: the least recently used tables leave; kernels still queued keep theirs (the
        caching allocator reuses a freed block only for later work of the same stream)."""
        new = []
        for key in dict.fromkeys(keys):
            if key in self._tab:
                self._tab.move_to_end(key)
            else:
                new.append(key)
        if not new:
            return
        host, parts = [], []
        for n_in, n_out in new:
            if n_in == n_out:
                b = np.stack([np.arange(n_out, dtype=np.int32), np.ones(n_out, np.int32)], 1)
                c, ks = np.full((n_out, 1), 1 << _RESIZE_PRECISION_BITS, np.int32), 1
            else:
                b, c, ks = resize_tables(n_in, n_out)
            host += [b.reshape(-1), c.reshape(-1)]
            parts.append((n_out, ks))
        buf = torch.from_numpy(np.concatenate(host))
        dev = (buf.pin_memory() if torch.device(self.dev).type == "cuda" else buf).to(self.dev, non_blocking=True)
        off = 0
        for key, (n, ks) in zip(new, parts):
            while len(self._tab) >= max(self.TABLE_CACHE, 2 * len(keys)):
                self._tab.popitem(last=False)
            self._tab[key] = (dev[off:off + 2 * n].view(n, 2), dev[off + 2 * n:off + (2 + ks) * n].view(n, ks), ks)
            off += (2 + ks) * n

    def resize_flat(self, flat: torch.Tensor, hw, out: Optional[torch.Tensor] = None, crop=None, jitter=None, flip=None, fill=None,
                    warp=None, blur=None) -> torch.Tensor:
        """resize_geom's batch, then steps 6 and 7 of augment_host on the GPU (zsg_augment_warp_u8_batched): warp = [B, 6] host integers
        (warp_matrix; a WARP_IDENTITY row = that job is not warped; a warped job needs `fill`), blur = [B] host sigmas (0 = that job is not
        blurred).  With a job to warp or blur the batch is resized into a scratch batch and the new launches write `out`; a batch
        without one makes no new launch and allocates nothing new (`self.warp_calls` counts the calls of the new entry)."""
        B = len(hw)
        jobs = self._warp_jobs(B, warp, blur, fill)
        if jobs is None:
            return self.resize_geom(flat, hw, out, crop, jitter, flip, fill)
        if self._warp_src is None or self._warp_src.shape[0] < B:
            self._warp_src = torch.empty(B, self.Ho, self.Wo, 3, dtype=torch.uint8, device=self.dev)
        src = self.resize_geom(flat, hw, self._warp_src[:B], crop, jitter, flip, fill)
        if out is None:
            out = torch.empty(B, self.Ho, self.Wo, 3, dtype=torch.uint8, device=self.dev)
        return self._run_warp(src, out, jobs)

    def _warp_jobs(self, B, warp, blur, fill):
        """None when no job has a warp or a blur; else per job (six integers or None, (r, taps) or None, fill)"""
        if warp is None and blur is None:
            return None
        wr = [None] * B if warp is None else [tuple(int(v) for v in row) for row in (warp.tolist() if torch.is_tensor(warp) else warp)]
        sg = [0.0] * B if blur is None else [float(v) for v in (blur.tolist() if torch.is_tensor(blur) else blur)]
        if len(wr) != B or len(sg) != B or any(m is not None and len(m) != 6 for m in wr):
            raise ValueError(f"resize_flat: {B} images, warp must be [{B}, 6] and blur [{B}]")
        wr = [None if m is None or m == WARP_IDENTITY else m for m in wr]
        if any(m is not None and not all(-(1 << 31) <= v < 1 << 31 for v in m) for m in wr):
            raise ValueError("resize_flat: warp coefficients must fit 32 bits")
        if any(not (s == 0.0 or 0.0 < s < math.inf) for s in sg):
            raise ValueError("resize_flat: blur sigmas must be 0 (off) or positive and finite")
        if not any(m is not None for m in wr) and not any(sg):
            return None
        fills = [(0, 0, 0)] * B
        if any(m is not None for m in wr):
            if fill is None:
                raise ValueError("resize_flat: a warp needs fill, the colour of the taps outside the image")
            f = np.asarray(fill.cpu() if torch.is_tensor(fill) else fill)
            f = np.broadcast_to(f, (B, f.shape[0])) if f.ndim == 1 else f
            if f.shape != (B, 3):
                raise ValueError(f"resize_flat: fill must be (r, g, b) or [{B}, 3]")
            fills = [_check_fill(row.tolist(), "resize_flat: fill") for row in f]
        return [(m, blur_taps(s) if s else None, fl) for m, s, fl in zip(wr, sg, fills)]

    def _run_warp(self, src, out, jobs):
        """src -> out through zsg_augment_warp_u8_batched; the 128-byte job record of include/zsg.h, validated by the entry before it launches"""
        import struct
        from ._lib import check, lib, stream_ptr
        B, per = len(jobs), self.Ho * self.Wo * 3
        if tuple(out.shape) != (B, self.Ho, self.Wo, 3) or out.dtype != torch.uint8 or not out.is_contiguous():
            raise ValueError(f"resize_flat: out must be a contiguous uint8 [{B}, {self.Ho}, {self.Wo}, 3]")
        stages = int(any(m is not None for m, _, _ in jobs)) | 2 * int(any(t is not None for _, t, _ in jobs))
        tmp_ptr = 0
        if stages & 2:
            need = B * ((per + 3) // 4 * 4)
            if self._warp_tmp is None or self._warp_tmp.numel() < need:
                self._warp_tmp = torch.empty(need, dtype=torch.uint8, device=self.dev)
            tmp_ptr = self._warp_tmp.data_ptr()
        blob = b""
        for i, (m, bt, (r, g, b)) in enumerate(jobs):
            rad, taps = (bt[0], [int(v) for v in bt[1]]) if bt is not None else (0, [])
            blob += struct.pack("<qq6iIii17i2i", src.data_ptr() + i * per, out.data_ptr() + i * per, *(m if m is not None else WARP_IDENTITY),
                                r | g << 8 | b << 16, int(m is not None) | 2 * int(bt is not None), rad, *(taps + [0] * (17 - len(taps))), 0, 0)
        table = self._upload_jobs(blob, 128)
        check(lib.zsg_augment_warp_u8_batched(table.data_ptr(), blob, B, self.Ho, self.Wo, tmp_ptr, stages, stream_ptr()), "zsg_augment_warp_u8_batched")
        self.warp_calls += 1
        return out

    def resize_geom(self, flat: torch.Tensor, hw, out: Optional[torch.Tensor] = None, crop=None, jitter=None, flip=None, fill=None) -> torch.Tensor:
        """Steps 1-5 of augment_host (resize_flat without warp and blur is exactly this call).
        flat: uint8 DEVICE tensor holding the raw images back to back; hw: [B, 2] (host) heights / widths.  Returns uint8 [B, Ho, Wo, 3].
        crop ([B, 4] host integers x0, y0, x1, y1 inside each image) and / or jitter ([B, 3] host float32 brightness, contrast,
        saturation factors): the training augmentation augment_host defines, on the GPU (zsg_augment_u8_batched) — each image's
        window is resized instead of the whole image, then jittered; a missing one = the whole image / factors 1.
        flip ([B] host booleans): the job's result is mirrored left-right.  fill ((r, g, b), or [B, 3], host integers 0..255): windows
        may leave their images, what lies outside is that colour (without it such a window is a ValueError).  A batch with a flipped
        job or a window not inside its image runs zsg_augment_geom_u8_batched, every other batch the kernels it always ran
        (`self.launches` counts the calls of either entry)."""
        offs = self._offsets(hw)
        if crop is None and jitter is None and flip is None and fill is None:
            return self._run([(flat.data_ptr() + off, h, w) for off, h, w in offs], out, keep=flat)
        B = len(offs)
        crop = [[0, 0, w, h] for _, h, w in offs] if crop is None else (crop.tolist() if torch.is_tensor(crop) else [list(c) for c in crop])
        jit = np.ones((B, 3), np.float32) if jitter is None else np.asarray(jitter.cpu() if torch.is_tensor(jitter) else jitter, dtype=np.float32).reshape(-1, 3)
        flips = [False] * B if flip is None else [bool(v) for v in (flip.tolist() if torch.is_tensor(flip) else flip)]
        if len(crop) != B or jit.shape[0] != B or len(flips) != B:
            raise ValueError(f"resize_flat: {B} images, {len(crop)} crops, {jit.shape[0]} jitter triples, {len(flips)} flips")
        if not np.isfinite(jit).all() or (jit < 0).any():
            raise ValueError("resize_flat: jitter factors must be finite and >= 0")
        fills = None
        if fill is not None:
            f = np.asarray(fill.cpu() if torch.is_tensor(fill) else fill)
            if f.ndim == 1:
                f = np.broadcast_to(f, (B, f.shape[0]))
            if f.shape != (B, 3):
                raise ValueError(f"resize_flat: fill must be (r, g, b) or [{B}, 3]")
            fills = [_check_fill(row.tolist(), "resize_flat: fill") for row in f]
        items, geom = [], any(flips)
        for (off, h, w), c in zip(offs, crop):
            x0, y0, x1, y1 = (int(v) for v in c)
            inside = 0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h
            if not inside and fills is None:                           # checked HERE: zsg_augment_u8_batched reads the window unchecked
                raise ValueError(f"resize_flat: crop {(x0, y0, x1, y1)} is not inside the {h} x {w} image")
            if not (x0 < x1 and y0 < y1):
                raise ValueError(f"resize_flat: crop {(x0, y0, x1, y1)} is empty")
            geom = geom or not inside
            items.append((flat.data_ptr() + off, h, w, x0, y0, x1, y1))
        if geom:
            return self._run_aug_geom(items, jit, flips, fills if fills is not None else [(0, 0, 0)] * B, out)
        return self._run_aug([(ptr + (y0 * w + x0) * 3, y1 - y0, x1 - x0, w) for ptr, h, w, x0, y0, x1, y1 in items], jit, out)

    MAX_GEOM_SIDE = 1 << 15     # zsg_augment_geom_u8_batched: image and window sides

    @staticmethod
    def _offsets(hw):
        off, res = 0, []
        for h, w in (hw.tolist() if torch.is_tensor(hw) else hw):
            res.append((off, int(h), int(w)))
            off += int(h) * int(w) * 3
        return res

    def _run(self, items, out, keep=None):
        import struct
        from ._lib import check, lib, stream_ptr
        B = len(items)
        if out is None:
            out = torch.empty(B, self.Ho, self.Wo, 3, dtype=torch.uint8, device=self.dev)
        need = sum(h for _, h, _ in items) * self.Wo * 3
        if self._tmp is None or self._tmp.numel() < need:
            self._tmp = torch.empty(need, dtype=torch.uint8, device=self.dev)
        blob, tmp_off, bx, by = b"", 0, 0, 0
        per_out = self.Ho * self.Wo * 3
        self._ensure_tables([(w, self.Wo) for _, _, w in items] + [(h, self.Ho) for _, h, _ in items])
        for i, (ptr, h, w) in enumerate(items):
            tx, ty = self._tab[(w, self.Wo)], self._tab[(h, self.Ho)]
            blob += struct.pack("<qqqqqqqiiiiiiii", ptr, self._tmp.data_ptr() + tmp_off, out.data_ptr() + i * per_out,
                                tx[0].data_ptr(), tx[1].data_ptr(), ty[0].data_ptr(), ty[1].data_ptr(), h, w, tx[2], ty[2], bx, by, 0, 0)
            tmp_off += h * self.Wo * 3
            bx += (h * self.Wo * 3 + 1023) // 1024
            by += (per_out + 1023) // 1024
        jobs = self._upload_jobs(blob, 88)
        check(lib.zsg_resize_u8_batched(jobs.data_ptr(), B, 3, self.Ho, self.Wo, bx, by, stream_ptr()), "zsg_resize_u8_batched")
        return out

    def _upload_jobs(self, blob: bytes, stride: int):
        """job table: pinned host slot -> device, asynchronously; four slots in rotation, each guarded by the event of its last upload
        (a slot is rewritten only when that copy has completed: normally four batches ago).  Returns the device table."""
        if self._jobs_host is None or self._jobs_host[0].numel() < len(blob):
            n = max(len(blob), stride * 256)
            self._jobs_host = [torch.empty(n, dtype=torch.uint8).pin_memory() for _ in range(4)]
            self._jobs_dev = [torch.empty(n, dtype=torch.uint8, device=self.dev) for _ in range(4)]
            self._jobs_ev = [None] * 4
            self._slot = 0
        k = self._slot = (self._slot + 1) % 4
        if self._jobs_ev[k] is not None:
            self._jobs_ev[k].synchronize()
        self._jobs_host[k][:len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8)
        self._jobs_dev[k][:len(blob)].copy_(self._jobs_host[k][:len(blob)], non_blocking=True)
        self._jobs_ev[k] = torch.cuda.Event()
        self._jobs_ev[k].record()
        return self._jobs_dev[k]

    def _run_aug(self, items, jit, out):
        """items: (address of the window's first pixel, window height, window width, row pitch of its image in pixels) per image"""
        import struct
        from ._lib import check, lib, stream_ptr
        B = len(items)
        if out is None:
            out = torch.empty(B, self.Ho, self.Wo, 3, dtype=torch.uint8, device=self.dev)
        need = sum((h * self.Wo * 3 + 3) // 4 * 4 for _, h, _, _ in items)
        if self._tmp is None or self._tmp.numel() < need:
            self._tmp = torch.empty(need, dtype=torch.uint8, device=self.dev)
        if self._gray is None or self._gray.numel() < B:
            self._gray = torch.zeros(max(B, 64), dtype=torch.int32, device=self.dev)
        blob, tmp_off, bx, by = b"", 0, 0, 0
        per_out = self.Ho * self.Wo * 3
        self._ensure_tables([(w, self.Wo) for _, _, w, _ in items] + [(h, self.Ho) for _, h, _, _ in items])
        for i, (ptr, h, w, pitch) in enumerate(items):
            tx, ty = self._tab[(w, self.Wo)], self._tab[(h, self.Ho)]
            blob += struct.pack("<qqqqqqqiiiiiiiifffi", ptr, self._tmp.data_ptr() + tmp_off, out.data_ptr() + i * per_out,
                                tx[0].data_ptr(), tx[1].data_ptr(), ty[0].data_ptr(), ty[1].data_ptr(), h, w, pitch, tx[2], ty[2], bx, by, 0,
                                float(jit[i, 0]), float(jit[i, 1]), float(jit[i, 2]), 0)
            tmp_off += (h * self.Wo * 3 + 3) // 4 * 4          # every job's scratch starts dword aligned
            bx += (h * self.Wo + 255) // 256
            by += (self.Ho * self.Wo + 255) // 256
        jobs = self._upload_jobs(blob, 104)
        do_cs = int(bool((jit[:, 1:] != 1.0).any()))           # launch 3 (contrast, saturation) only when some job needs it
        check(lib.zsg_augment_u8_batched(jobs.data_ptr(), B, self.Ho, self.Wo, bx, by, self._gray.data_ptr(), do_cs, stream_ptr()),
              "zsg_augment_u8_batched")
        self.launches["augment_u8"] += 1
        return out

    def _run_aug_geom(self, items, jit, flips, fills, out):
        """items: (address of the image's pixel (0, 0), image height, width, window x0, y0, x1, y1) per image — the window may leave the
        image; the 120-byte job record of zsg_augment_geom_u8_batched (include/zsg.h), which validates the table before it launches"""
        import struct
        from ._lib import check, lib, stream_ptr
        B = len(items)
        for _, h, w, x0, y0, x1, y1 in items:                  # (the C entry checks the same; here the message names the window)
            if max(x1 - x0, y1 - y0, h, w) > self.MAX_GEOM_SIDE or max(abs(x0), abs(y0)) >= 1 << 24:
                raise ValueError(f"resize_flat: crop {(x0, y0, x1, y1)} of the {h} x {w} image: sides up to {self.MAX_GEOM_SIDE} with fill / flip")
        if out is None:
            out = torch.empty(B, self.Ho, self.Wo, 3, dtype=torch.uint8, device=self.dev)
        need = sum(((y1 - y0) * self.Wo * 3 + 3) // 4 * 4 for _, _, _, _, y0, _, y1 in items)
        if self._tmp is None or self._tmp.numel() < need:
            self._tmp = torch.empty(need, dtype=torch.uint8, device=self.dev)
        if self._gray is None or self._gray.numel() < B:
            self._gray = torch.zeros(max(B, 64), dtype=torch.int32, device=self.dev)
        blob, tmp_off, bx, by = b"", 0, 0, 0
        per_out = self.Ho * self.Wo * 3
        self._ensure_tables([(x1 - x0, self.Wo) for _, _, _, x0, _, x1, _ in items] + [(y1 - y0, self.Ho) for _, _, _, _, y0, _, y1 in items])
        for i, (ptr, h, w, x0, y0, x1, y1) in enumerate(items):
            wh, ww = y1 - y0, x1 - x0
            tx, ty = self._tab[(ww, self.Wo)], self._tab[(wh, self.Ho)]
            r, g, b = fills[i]
            blob += struct.pack("<qqqqqqqiiiiiiiiiiiIfffi", ptr, self._tmp.data_ptr() + tmp_off, out.data_ptr() + i * per_out,
                                tx[0].data_ptr(), tx[1].data_ptr(), ty[0].data_ptr(), ty[1].data_ptr(), h, w, x0, y0, wh, ww, tx[2], ty[2], bx, by,
                                int(flips[i]), r | g << 8 | b << 16, float(jit[i, 0]), float(jit[i, 1]), float(jit[i, 2]), 0)
            tmp_off += (wh * self.Wo * 3 + 3) // 4 * 4           # every job's scratch starts dword aligned
            bx += (wh * self.Wo + 255) // 256
            by += (self.Ho * self.Wo + 255) // 256
        jobs = self._upload_jobs(blob, 120)
        do_cs = int(bool((jit[:, 1:] != 1.0).any()))
        check(lib.zsg_augment_geom_u8_batched(jobs.data_ptr(), blob, B, self.Ho, self.Wo, bx, by, self._gray.data_ptr(), do_cs, stream_ptr()),
              "zsg_augment_geom_u8_batched")
        self.launches["augment_geom_u8"] += 1
        return out

    def __call__(self, imgs, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """imgs: list of uint8 [h, w, 3] DEVICE tensors; returns uint8 [B, Ho, Wo, 3]"""
        for im in imgs:
            assert im.is_cuda and im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3 and im.is_contiguous()
        return self._run([(im.data_ptr(), int(im.shape[0]), int(im.shape[1])) for im in imgs], out, keep=imgs)


# ---------------------------------------------------------------------------------------------------------------------
# dataset + collater
# ---------------------------------------------------------------------------------------------------------------------
class ImgQuDataset(Dataset):
    """Any grounding dataset given as a CSV of (img_id, bbox, query) rows; the same image may appear on many rows."""

    def __init__(self, cfg, csv_file, ds_name: str, split_type: str = "train", embedder=None, gpu_normalise: bool = False,
                 gpu_resize: bool = False):
        """gpu_normalise: the item's image stays uint8 HWC (converted on the GPU); gpu_resize (implies it): the image is NOT resized by
        the worker either — it travels at its decoded size and DevicePrefetcher resizes it on the GPU (GpuResizer: Pillow's filter
        bit for bit), which leaves a worker only the JPEG decode."""
        import pandas as pd
        gpu_normalise = gpu_normalise or gpu_resize
        self.cfg, self.ds_name, self.split_type, self.gpu_normalise, self.gpu_resize = cfg, ds_name, split_type, gpu_normalise, gpu_resize
        self.embedder = embedder if embedder is not None else get_embedder(cfg)
        self.augment = split_type == "train" and aug_enabled(cfg)      # training split only: draw_augment_geom per item / per image slot
        pflip, emax, fill = aug_geom_params(cfg)
        self.aug_warp = self.augment and aug_warp_enabled(cfg)         # aug_rotate / aug_shear / aug_blur on: the items carry aug_warp and aug_blur
        self.aug_fill = fill if self.augment and (pflip > 0.0 or emax > 1.0 or self.aug_warp) else None      # flips / windows that leave the image / warps
        tta = cfg["eval_tta"] if "eval_tta" in cfg else "none"
        if tta not in ("none", "flip"):
            raise ValueError(f"eval_tta={tta!r}: expected one of none, flip")
        self.tta_flip = split_type != "train" and tta == "flip"       # validation / test items also carry `qvec_flip` (ZSGNet.eval_tta)
        self.img_dir = Path(cfg["ds_info"][ds_name]["img_dir"])
        self.phrase_len = PHRASE_LEN
        df = pd.read_csv(csv_file)
        self.boxes = [ast.literal_eval(b) if isinstance(b, str) else list(b) for b in df["bbox"]]
        first = str(df["query"].iloc[0])
        self.queries = [ast.literal_eval(q) for q in df["query"]] if first[:1] == "[" else [str(q) for q in df["query"]]
        ids = [str(i) for i in df["img_id"]]
        self.files = [f"{i}.jpg" for i in ids] if ds_name.startswith("flickr30k") else ids        # dat_loader.py:176-184

    def __len__(self):
        return len(self.files)

    def load_image(self, idx: int, boxes=None):
        """the image of row idx as the batch carries it (decoded, resized unless gpu_resize) + its decoded height / width.
        boxes (a training dataset with augmentation on): the pixel boxes the crop must keep — one draw_augment_warp from np.random; a
        worker that resizes applies it (augment_host), with gpu_resize the raw image travels and DevicePrefetcher applies it on the GPU.
        Returns a fourth value then: the (crop, jitter, flip, warp, sigma) drawn."""
        import PIL.Image
        img = PIL.Image.open(self.img_dir / self.files[idx]).convert("RGB")
        h, w = img.height, img.width
        rs = self.cfg["resize_img"]
        aug = draw_augment_warp(np.random, h, w, boxes, self.cfg, (rs[1], rs[0])) if boxes is not None else None
        if not self.gpu_resize:
            if aug is not None:
                img = augment_host(np.asarray(img), aug[0], aug[1], (rs[1], rs[0]), flip=aug[2], fill=self.aug_fill,
                                   warp=warp_matrix(*aug[3], (rs[1], rs[0])) if aug[3] is not None else None, blur=aug[4] or 0.0)
            else:
                img = img.resize((rs[0], rs[1]))                  # PIL's default filter, as the reference (dat_loader.py:121)
        a = np.asarray(img)                                       # [H, W, 3] uint8
        if self.gpu_normalise:
            img_t = torch.from_numpy(a.copy())                    # normalised on the GPU (zsg_u8hwc_to_nhwc4)
        else:
            img_t = torch.from_numpy(a.transpose(2, 0, 1).astype(np.float64)).float().div_(255)     # pil2tensor(...).float().div_(255)
        return (img_t, h, w) if boxes is None else (img_t, h, w, aug)

    def query_item(self, idx: int, h: int, w: int, crop=None, flip: bool = False, warp=None) -> Dict[str, torch.Tensor]:
        """the per-query fields of row idx (everything but the image, whose decoded size h, w scales the box).  crop (x0, y0, x1, y1):
        the image was cropped to that window (which may leave the image: zoom-out) — the box is given relative to it (unclipped) and
        img_size is the window's, so the identities between annot, orig_annot and img_size the evaluator relies on keep holding.
        flip: the window was mirrored left-right — so is the box, in window pixels (x1' = cw - x2, x2' = cw - x1), and the query's
        direction words are swapped (swap_left_right) before it is embedded.
        warp (theta, shear): the resized window was warped (augment_host step 6) — the box becomes warp_box's: the bounding box of its
        warped corners, clipped to the window, in window pixels; img_size stays the window's."""
        q = self.queries[idx]
        if isinstance(q, list):
            q = str(np.random.choice(q))                          # dat_loader.py:153-154
        q = q.replace("_", " ")
        if flip:
            q = swap_left_right(q)
        qvec, qlen = embed_query(self.embedder, q, self.phrase_len)
        extra = {}
        if self.tta_flip:
            # the query of the mirrored image (cfg eval_tta = "flip"): left <-> right word for word, so the token count cannot change
            qvf, qlf = embed_query(self.embedder, swap_left_right(q), self.phrase_len)
            assert qlf == qlen, f"swap_left_right changed the token count of {q!r}: {qlen} -> {qlf}"
            extra["qvec_flip"] = torch.from_numpy(qvf)
        x1, y1, x2, y2 = self.boxes[idx]
        if crop is not None:
            x0, y0 = int(crop[0]), int(crop[1])
            h, w = int(crop[3]) - y0, int(crop[2]) - x0
            x1, y1, x2, y2 = x1 - x0, y1 - y0, x2 - x0, y2 - y0
        if flip:
            x1, x2 = w - x2, w - x1
        if warp is not None:
            rs = self.cfg["resize_img"]
            x1, y1, x2, y2 = warp_box((x1, y1, x2, y2), warp[0], warp[1], (rs[1], rs[0]), (h, w))
        target = 2 * np.array([y1 / h, x1 / w, y2 / h, x2 / w]) - 1          # y1x1y2x2 in [-1, 1] (anchors are row, column)
        return {"idxs": torch.tensor(idx).long(), "qvec": torch.from_numpy(qvec),
                "qlens": torch.tensor(min(qlen, self.phrase_len)), "annot": torch.from_numpy(target).float(),
                "orig_annot": torch.tensor([x1, y1, x2, y2]).float(), "img_size": torch.tensor([h, w]), **extra}

    def __getitem__(self, idx: int) -> Dict[str, torch.Tensor]:
        if self.augment:
            img_t, h, w, (crop, jitter, flip, warp, sigma) = self.load_image(idx, [self.boxes[idx]])
            item = {"img": img_t}
            item.update(self.query_item(idx, h, w, crop, flip, warp))
            if self.gpu_resize:                                   # applied by DevicePrefetcher (GpuResizer.resize_flat), dropped there
                item["aug_crop"], item["aug_jitter"] = torch.tensor(crop, dtype=torch.int32), torch.from_numpy(jitter)
                if self.aug_fill is not None:                     # only with aug_flip / aug_expand_max / a warp key on: (flip, fill r, g, b)
                    item["aug_geom"] = torch.tensor([int(flip), *self.aug_fill], dtype=torch.int32)
                if self.aug_warp:                                 # only with aug_rotate / aug_shear / aug_blur on
                    item["aug_warp"], item["aug_blur"] = self._warp_fields(warp, sigma)
            return item
        img_t, h, w = self.load_image(idx)
        item = {"img": img_t}
        item.update(self.query_item(idx, h, w))
        return item

    def _warp_fields(self, warp, sigma):
        """(aug_warp int32 [6], aug_blur float32 scalar) of one drawn (theta, shear) / sigma: the identity and 0 where none applies"""
        rs = self.cfg["resize_img"]
        m = warp_matrix(warp[0], warp[1], (rs[1], rs[0])) if warp is not None else WARP_IDENTITY
        return torch.tensor(m, dtype=torch.int32), torch.tensor(sigma or 0.0, dtype=torch.float32)

    def grouped_batch(self, rows: List[int]) -> Dict[str, torch.Tensor]:
        """One batch of the grouped validation loader (cfg group_val_by_image): every distinct image file among `rows` is decoded (and
        resized) ONCE; `img` holds the distinct images in order of first appearance and `img_idx` [Q] int64 names each query's image
        (ZSGNet.forward's shared-image contract).  The per-query fields are collater's, in the order of `rows`."""
        slot, imgs, sizes, items, idx = {}, [], [], [], []
        for r in rows:
            f = self.files[r]
            if f not in slot:
                img_t, h, w = self.load_image(r)
                slot[f] = len(imgs)
                imgs.append(img_t)
                sizes.append((h, w))
            k = slot[f]
            items.append(self.query_item(r, *sizes[k]))
            idx.append(k)
        return grouped_collater(items, imgs, idx)

    def grouped_train_batch(self, chunks: List[List[int]]) -> Dict[str, torch.Tensor]:
        """One batch of the grouped TRAINING loader (cfg group_trn_by_image): one image slot per chunk — the rows of a chunk share an image
        file, which is decoded (and resized) once, from the chunk's first row — even if two chunks of one file meet in a batch; the
        queries in chunk order.  Exactly len(chunks) slots, every one used (checked by the collater)."""
        imgs, items, idx, crops, jitters, geoms, warps = [], [], [], [], [], [], []
        for s, rows in enumerate(chunks):
            if len({self.files[r] for r in rows}) != 1:
                raise ValueError(f"grouped_train_batch: chunk {s} mixes image files")
            crop, flip, warp = None, False, None
            if self.augment:                                      # ONE draw per image slot, from the union of the chunk's boxes
                img_t, h, w, (crop, jitter, flip, warp, sigma) = self.load_image(rows[0], [self.boxes[r] for r in rows])
                crops.append(crop)
                jitters.append(jitter)
                if self.aug_fill is not None:
                    geoms.append([int(flip), *self.aug_fill])
                if self.aug_warp:
                    warps.append(self._warp_fields(warp, sigma))
            else:
                img_t, h, w = self.load_image(rows[0])
            imgs.append(img_t)
            for r in rows:                                        # every query of the slot: the slot's window, mirrored and swapped alike
                items.append(self.query_item(r, h, w, crop, flip, warp))
                idx.append(s)
        aug = ((crops, jitters, geoms, warps) if warps else (crops, jitters, geoms) if geoms else (crops, jitters)) if self.augment and self.gpu_resize else None
        return grouped_collater(items, imgs, idx, all_slots_used=True, aug=aug)


def collater(batch: List[Dict[str, torch.Tensor]]) -> Dict[str, torch.Tensor]:
    """dat_loader.py:187-196: every field stacked as float (uint8 images stay uint8: they become float on the GPU);
    qvec (and qvec_flip, the mirrored image's query of cfg eval_tta = "flip", where the items carry it) cut to the longest query of the batch."""
    max_qlen = int(max(int(b["qlens"]) for b in batch))
    out = {}
    for k in batch[0]:
        if k == "img" and batch[0][k].dtype == torch.uint8 and len({tuple(b[k].shape) for b in batch}) > 1:
            # raw images of different sizes (gpu_resize): ONE flat tensor + the sizes; DevicePrefetcher uploads it with one copy and
            # resizes the batch on the GPU with two launches
            out["img"], out["img_hw"] = flatten_raw([b[k] for b in batch])
            continue
        t = torch.stack([b[k] for b in batch])
        out[k] = t if ((k == "img" and t.dtype == torch.uint8) or k in ("aug_crop", "aug_geom", "aug_warp")) else t.float()       # (aug_crop, aug_geom, aug_warp: int32)
    out["qvec"] = out["qvec"][:, :max_qlen]
    if "qvec_flip" in out:
        out["qvec_flip"] = out["qvec_flip"][:, :max_qlen]
    if "img_hw" in out:
        out["img_hw"] = out["img_hw"].int()
    return out


def grouped_collater(items: List[Dict[str, torch.Tensor]], imgs: List[torch.Tensor], img_idx: List[int],
                     all_slots_used: bool = False, aug=None) -> Dict[str, torch.Tensor]:
    """collater for queries that share images: `items` carry no image; `imgs` are the distinct images, img_idx[q] the image of query q.
    This is where the index range is checked (on the host, once per batch): the forward reads img_idx on the device only.
    all_slots_used (training batches): every image slot must be named by some query — train-mode BatchNorm reduces over all slots.
    aug = (crops, jitters), one per image SLOT (gpu_resize training with augmentation): emitted as `aug_crop` int32 [slots, 4] and
    `aug_jitter` float32 [slots, 3] alongside `img`; a third member (aug_flip / aug_expand_max on) = (flip, fill r, g, b) per slot,
    emitted as `aug_geom` int32 [slots, 4]; a fourth (aug_rotate / aug_shear / aug_blur on) = (six warp integers, sigma) tensors per slot,
    emitted as `aug_warp` int32 [slots, 6] and `aug_blur` float32 [slots]."""
    if not imgs or len(img_idx) != len(items) or min(img_idx) < 0 or max(img_idx) >= len(imgs):
        raise ValueError(f"grouped_collater: img_idx out of range for {len(imgs)} images / {len(items)} queries")
    if all_slots_used and len(set(img_idx)) != len(imgs):
        raise ValueError(f"grouped_collater: {len(imgs) - len(set(img_idx))} of {len(imgs)} image slots are used by no query")
    out = collater(items)
    if imgs[0].dtype == torch.uint8 and len({tuple(im.shape) for im in imgs}) > 1:
        out["img"], out["img_hw"] = flatten_raw(imgs)            # raw images of different sizes (gpu_resize), as collater
        out["img_hw"] = out["img_hw"].int()
    else:
        t = torch.stack(imgs)
        out["img"] = t if t.dtype == torch.uint8 else t.float()
    out["img_idx"] = torch.tensor(img_idx, dtype=torch.long)
    if aug is not None:
        if len(aug[0]) != len(imgs) or len(aug[1]) != len(imgs):
            raise ValueError(f"grouped_collater: {len(imgs)} image slots but {len(aug[0])} crops / {len(aug[1])} jitter triples")
        out["aug_crop"] = torch.tensor([list(c) for c in aug[0]], dtype=torch.int32)
        out["aug_jitter"] = torch.from_numpy(np.stack(aug[1]).astype(np.float32))
        if len(aug) > 2:
            if len(aug[2]) != len(imgs):
                raise ValueError(f"grouped_collater: {len(imgs)} image slots but {len(aug[2])} flip / fill records")
            out["aug_geom"] = torch.tensor([list(g) for g in aug[2]], dtype=torch.int32)
        if len(aug) > 3:
            if len(aug[3]) != len(imgs):
                raise ValueError(f"grouped_collater: {len(imgs)} image slots but {len(aug[3])} warp / blur records")
            out["aug_warp"], out["aug_blur"] = torch.stack([m for m, _ in aug[3]]), torch.stack([s for _, s in aug[3]])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# samplers / loaders
# ---------------------------------------------------------------------------------------------------------------------
def group_rows_by_image(files: List[str], rank: int = 0, world: int = 1) -> List[int]:
    """Dataset rows ordered so that the rows of one image file are adjacent: files in order of first appearance, the rows of a file in
    dataset order (the documented reordering of the grouped validation loader).  world > 1: this rank's share of that order — whole
    image groups, contiguous, the same on every call (no shuffle, no padding), balanced by rows: the group that starts at position c of
    the n rows goes to rank floor(c * world / n).  Every row appears exactly once across the ranks."""
    first: Dict[str, int] = {}
    for i, f in enumerate(files):
        first.setdefault(f, i)
    order = sorted(range(len(files)), key=lambda i: (first[files[i]], i))
    if world <= 1:
        return order
    n, mine, owner = len(order), [], 0
    for c, i in enumerate(order):
        if c == 0 or files[i] != files[order[c - 1]]:
            owner = min(world - 1, c * world // n)
        if owner == rank:
            mine.append(i)
    return mine


class _GroupedBatches(Dataset):
    """item i = the i-th whole batch of the grouped order, built by ImgQuDataset.grouped_batch in a worker (DataLoader(batch_size=None))"""

    def __init__(self, dataset, batches: List[List[int]]):
        self.dataset, self.batches = dataset, batches

    def __len__(self):
        return len(self.batches)

    def __getitem__(self, i: int):
        return self.dataset.grouped_batch(self.batches[i])


def _identity(x):
    return x


def get_grouped_dataloader(cfg, dataset, rank: Optional[int] = None, world: Optional[int] = None) -> DataLoader:
    """Validation / test loader of cfg group_val_by_image: batches of bsv queries (the last one shorter) in group_rows_by_image's
    order, each distinct image of a batch decoded once and emitted once, with `img_idx`.  Under do_dist every rank reads its own share
    of whole image groups, in a fixed order (NewDistributedSampler would shuffle rows and tear the groups apart)."""
    if rank is None or world is None:
        rank, world = 0, 1
        if bool(cfg["do_dist"]) and torch.distributed.is_available() and torch.distributed.is_initialized():
            rank, world = torch.distributed.get_rank(), torch.distributed.get_world_size()
    rows = group_rows_by_image(dataset.files, rank, world)
    bs = cfg["bsv"] if "bsv" in cfg else cfg["bs"]
    nw = cfg["nwv"] if "nwv" in cfg else cfg["nw"]
    batches = [rows[i:i + bs] for i in range(0, len(rows), bs)]
    return DataLoader(_GroupedBatches(dataset, batches), batch_size=None, shuffle=False, num_workers=nw, collate_fn=_identity,
                      pin_memory=torch.cuda.is_available(), persistent_workers=nw > 0)


class GroupedTrainSampler(torch.utils.data.Sampler):
    """Batches of the grouped TRAINING loader (cfg group_trn_by_image), one per iteration step: a list of bs // k chunks, each k rows of
    ONE image file.  Per epoch: the rows of each file are shuffled and cut into chunks of k; a short last chunk is filled by re-drawing
    rows of the same file; the chunks are shuffled — seeded by the epoch, as NewDistributedSampler, so every rank sees the same
    list — and dealt to the ranks in equal numbers (rank r takes every world-th chunk from r); every batch is bs // k chunks, hence
    exactly bs // k image slots and bs queries on every rank; the last short batch is dropped, as drop_last does for the ungrouped
    training loader.  The number of batches does not depend on the epoch."""

    def __init__(self, files: List[str], bs: int, k: int, rank: int = 0, world: int = 1, seed: int = 0):
        if k < 1 or bs < k or bs % k != 0:
            raise ValueError(f"grouped training loader: bs={bs} must be a positive multiple of trn_queries_per_image={k}")
        self.bs, self.k, self.rank, self.world, self.seed, self.epoch = bs, k, rank, max(1, world), seed, 0
        self.by_file: Dict[str, List[int]] = {}
        for i, f in enumerate(files):
            self.by_file.setdefault(f, []).append(i)
        n_chunks = sum((len(r) + k - 1) // k for r in self.by_file.values())
        self.n_batches = n_chunks // (self.world * (bs // k))

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    def __len__(self):
        return self.n_batches

    def chunks(self, epoch: int) -> List[List[int]]:
        """every chunk of the epoch, in the shuffled order all ranks share"""
        g = torch.Generator()
        g.manual_seed(self.seed + epoch)
        out, k = [], self.k
        for rows in self.by_file.values():
            perm = [rows[i] for i in torch.randperm(len(rows), generator=g).tolist()]
            for c in range(0, len(perm), k):
                ch = perm[c:c + k]
                if len(ch) < k:
                    ch = ch + [rows[i] for i in torch.randint(0, len(rows), (k - len(ch),), generator=g).tolist()]
                out.append(ch)
        return [out[i] for i in torch.randperm(len(out), generator=g).tolist()]

    def batches(self, epoch: Optional[int] = None) -> List[List[List[int]]]:
        mine = self.chunks(self.epoch if epoch is None else epoch)[self.rank::self.world]
        cpb = self.bs // self.k
        return [mine[b * cpb:(b + 1) * cpb] for b in range(self.n_batches)]

    def __iter__(self):
        yield from self.batches()
        self.epoch += 1          # (a caller that never calls set_epoch still gets a new order every epoch)


class _GroupedTrainBatches(Dataset):
    """indexed by a batch of GroupedTrainSampler (DataLoader(batch_size=None) hands the sampler's item over as the index): the whole
    batch is built by ImgQuDataset.grouped_train_batch in ONE worker call"""

    def __init__(self, dataset):
        self.dataset = dataset

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, chunks):
        return self.dataset.grouped_train_batch(chunks)


def get_grouped_train_dataloader(cfg, dataset, rank: Optional[int] = None, world: Optional[int] = None) -> DataLoader:
    """Training loader of cfg group_trn_by_image: every batch is cfg.bs queries over cfg.bs // cfg.trn_queries_per_image image slots with
    `img_idx`, equal groups (GroupedTrainSampler), for ZSGNet.shared_training."""
    if rank is None or world is None:
        rank, world = 0, 1
        if bool(cfg["do_dist"]) and torch.distributed.is_available() and torch.distributed.is_initialized():
            rank, world = torch.distributed.get_rank(), torch.distributed.get_world_size()
    sampler = GroupedTrainSampler(dataset.files, int(cfg["bs"]), int(cfg["trn_queries_per_image"]), rank, world)
    nw = cfg["nw"]
    return DataLoader(_GroupedTrainBatches(dataset), batch_size=None, sampler=sampler, num_workers=nw, collate_fn=_identity,
                      pin_memory=torch.cuda.is_available(), persistent_workers=nw > 0)


class NewDistributedSampler(DistributedSampler):
    """DistributedSampler with a shuffle switch, so validation can be sharded too (dat_loader.py:36-65): deterministic
    per-epoch permutation, padded with the head of the list to a multiple of the world size, contiguous rank slices."""

    def __init__(self, dataset, num_replicas=None, rank=None, shuffle=True):
        super().__init__(dataset, num_replicas=num_replicas, rank=rank)
        self.shuffle = shuffle

    def __iter__(self):
        n = len(self.dataset)
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.epoch)
            indices = torch.randperm(n, generator=g).tolist()
        else:
            indices = list(range(n))
        indices += indices[: (self.total_size - len(indices))]
        off = self.num_samples * self.rank
        return iter(indices[off: off + self.num_samples])


def get_dataloader(cfg, dataset: Dataset, is_train: bool) -> DataLoader:
    """dat_loader.py:208-230 (one process per GPU: per-rank batch = cfg.bs; validation is sharded and shuffled under DDP)."""
    if not is_train and bool(cfg["group_val_by_image"] if "group_val_by_image" in cfg else False):
        return get_grouped_dataloader(cfg, dataset)
    if is_train and bool(cfg["group_trn_by_image"] if "group_trn_by_image" in cfg else False):
        return get_grouped_train_dataloader(cfg, dataset)
    dist_on = bool(cfg["do_dist"])
    if dist_on:
        sampler = NewDistributedSampler(dataset, shuffle=True)
    elif is_train:
        sampler = torch.utils.data.RandomSampler(dataset)
    else:
        sampler = torch.utils.data.SequentialSampler(dataset)
    bs = cfg["bs"] if is_train else (cfg["bsv"] if "bsv" in cfg else cfg["bs"])
    nw = cfg["nw"] if is_train else (cfg["nwv"] if "nwv" in cfg else cfg["nw"])
    return DataLoader(dataset, batch_size=bs, sampler=sampler, drop_last=is_train, num_workers=nw, collate_fn=collater,
                      pin_memory=torch.cuda.is_available(), persistent_workers=nw > 0)


class DevicePrefetcher:
    """Wraps a loader of pinned host batches: the next batch is copied to the GPU on a side stream while the current one
    is being consumed (HIP copy engine overlaps the training step), and handed over with an event wait."""

    _HOST_ONLY = ("img_hw", "aug_crop", "aug_jitter", "aug_geom", "aug_warp", "aug_blur")        # fields the resizer consumes on the host: not part of the device batch

    def __init__(self, loader, device="cuda", resize_hw=None):
        """resize_hw = (H, W): batches whose "img" is raw uint8 HWC (a list of differently sized images, or a stack at another size)
        are resized on the GPU, on the upload stream (GpuResizer)."""
        self.loader, self.device = loader, torch.device(device)
        self.stream = torch.cuda.Stream(self.device) if self.device.type == "cuda" else None
        self.resize_hw = tuple(resize_hw) if resize_hw is not None else None
        self._resizer = None

    def __len__(self):
        return len(self.loader)

    def _upload(self, batch):
        if self.stream is None:
            return batch, None
        with torch.cuda.stream(self.stream):
            dev = {k: v.to(self.device, non_blocking=True) for k, v in batch.items() if torch.is_tensor(v) and k not in self._HOST_ONLY}
            img = batch.get("img")
            hw = batch.get("img_hw")
            crop, jitter = batch.get("aug_crop"), batch.get("aug_jitter")      # training augmentation: applied by the resizer, not handed on
            if isinstance(img, list):              # (callers that still hand over a list of raw images: flattened here, on this thread)
                img, hw = flatten_raw(img)
                dev["img"] = img.pin_memory().to(self.device, non_blocking=True)
            elif hw is None and self.resize_hw and torch.is_tensor(img) and img.dtype == torch.uint8 and img.dim() == 4 \
                    and (tuple(img.shape[1:3]) != self.resize_hw or crop is not None):
                hw = torch.tensor([[img.shape[1], img.shape[2]]] * img.shape[0], dtype=torch.int32)      # a stack at another size
                dev["img"] = dev["img"].reshape(-1)
            if hw is not None:
                if self.resize_hw is None:
                    raise RuntimeError("DevicePrefetcher: raw images of mixed sizes need resize_hw")
                if self._resizer is None:
                    self._resizer = GpuResizer(self.resize_hw, self.device)
                geom = batch.get("aug_geom")                   # int32 [B, 4] = (flip, fill r, g, b): only with aug_flip / aug_expand_max on
                if geom is not None:               # (aug_warp / aug_blur: only with aug_rotate / aug_shear / aug_blur on, and then with aug_geom)
                    dev["img"] = self._resizer.resize_flat(dev["img"], hw, crop=crop, jitter=jitter, flip=geom[:, 0] != 0, fill=geom[:, 1:],
                                                           warp=batch.get("aug_warp"), blur=batch.get("aug_blur"))
                else:
                    dev["img"] = self._resizer.resize_flat(dev["img"], hw, crop=crop, jitter=jitter)
            elif crop is not None:
                raise RuntimeError("DevicePrefetcher: a batch with aug_crop / aug_jitter needs raw uint8 images and resize_hw")
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return dev, ev

    def __iter__(self) -> Iterator[Dict[str, torch.Tensor]]:
        sampler = getattr(self.loader, "sampler", None)
        if hasattr(sampler, "set_epoch"):
            self._epoch = getattr(self, "_epoch", -1) + 1
            sampler.set_epoch(self._epoch)
        nxt = None
        for batch in self.loader:
            cur, nxt = nxt, self._upload(batch)
            if cur is not None:
                yield self._hand_over(cur)
        if nxt is not None:
            yield self._hand_over(nxt)

    def _hand_over(self, item):
        dev, ev = item
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)
            for v in dev.values():
                v.record_stream(torch.cuda.current_stream())
        return dev


def get_data(cfg, embedder=None, prefetch: Optional[bool] = None):
    """dat_loader.py:233-257: train / valid / test loaders of cfg.ds_to_use (paths from cfg.ds_info)."""
    from .synth import DataWrap
    ds_name = cfg["ds_to_use"]
    info = cfg["ds_info"][ds_name]
    aug_params(cfg)                                          # ValueError for an aug_* key outside its range
    aug_geom_params(cfg)
    aug_warp_params(cfg)
    emb = embedder if embedder is not None else get_embedder(cfg)
    gpu = torch.cuda.is_available() and (cfg["gpu_img_normalise"] if "gpu_img_normalise" in cfg else True)
    prefetch = gpu if prefetch is None else prefetch
    gpu_rs = bool(gpu and prefetch and (cfg["gpu_img_resize"] if "gpu_img_resize" in cfg else True))      # resize on the GPU too (N2)
    rs = cfg["resize_img"]

    def make(csv_key, split, is_train):
        ds = ImgQuDataset(cfg, info[csv_key], ds_name, split, emb, gpu_normalise=gpu, gpu_resize=gpu_rs)
        dl = get_dataloader(cfg, ds, is_train)
        return DevicePrefetcher(dl, cfg["device"], resize_hw=(rs[1], rs[0]) if gpu_rs else None) if prefetch else dl
    return DataWrap(make("trn_csv_file", "train", True), make("val_csv_file", "valid", False),
                    {"test0": make("test_csv_file", "valid", False)}, cfg["tmp_path"])
