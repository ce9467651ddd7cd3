"""The inputs and the case grid the Soft-NMS tests share (not a test module): tests/test_cpu_softnms.py checks on the reference alone that
they are safe to compare exactly, tests/test_gpu_softnms.py runs them through the C ABI.

Table "pooled": the anchor table of a two-pass multi-scale forward (tests/test_gpu_vote.py's) — levels (4,4),(2,2),(1,1) plus
(5,5),(3,3),(2,2), nine anchors a cell, A = 531 — with regressions that are noise around zero, so that neighbouring anchors and the two
passes really overlap.  Sample 0 carries an isolated tiny box with the best score, sample 1 equal logits everywhere (ties go to the lower
position), sample 2 anchors with NaN logits and a finite best score on a box that does not decode.  Under "soft_gauss" sample 1 is left
out: every candidate of a tie is decayed a little by every pick, which turns bit-equal scores into near-equal weights whose order the
device's expf may not reproduce.
Table "cell": one cell, A = 9, run with pre_n = 16 > A.  Sample 0 is noise, sample 1 has six NaN logits (the rows end when the three
numbers are used up: a NaN score is never picked after row 0), sample 2 only NaN logits (row 0 alone, its score NaN).

A case is (table, method, pre_n, K, nms_thr, sigma, min_score); "soft_linear" does not read sigma and "soft_gauss" does not read nms_thr,
so each method's grid runs over the two parameters it reads."""
import itertools

import numpy as np
import torch

from oracle import zsg_oracle as O

import softnms_ref

F32 = np.float32
ACC_THR = 0.5
LEVELS = [(4, 4), (2, 2), (1, 1), (5, 5), (3, 3), (2, 2)]
LDS_PRE = 256                    # SN_LDS_PRE of csrc/softnms.hip: up to this pre_n the finishing block merges the lists from LDS
PRE_N = (1, 8, 64, LDS_PRE, LDS_PRE + 1, 512)
TOP_K = (1, 3, 5, 64)
NMS_THR = (0.3, 0.5)
SIGMA = (0.25, 0.5)
MIN_SCORE = (0.0, 0.001, 0.05)
SEED_POOLED, SEED_CELL = 26, 5      # chosen so that every case is safe to compare exactly (test_cpu_softnms.py asserts it)


def _grid(table, pre_ns):
    out = []
    for p, k, f in itertools.product(pre_ns, TOP_K, MIN_SCORE):
        if k > p:
            continue
        out += [(table, "soft_linear", p, k, t, SIGMA[1], f) for t in NMS_THR]
        out += [(table, "soft_gauss", p, k, NMS_THR[1], s, f) for s in SIGMA]
    return out


CASES = _grid("pooled", PRE_N) + _grid("cell", (16,))


def case_id(c):
    return f"{c[0]}-{c[1][5:]}-pre{c[2]}-K{c[3]}-thr{c[4]}-sig{c[5]}-min{c[6]}"


def _annot_from(px, img_size):
    """pixel boxes x1y1x2y2 -> y1x1y2x2 in [-1, 1], rounded to two digits (NaN rows become a fixed box)"""
    a = np.stack([px[:, 1] / img_size[:, 0], px[:, 0] / img_size[:, 1], px[:, 3] / img_size[:, 0], px[:, 2] / img_size[:, 1]], axis=1) * 2 - 1
    a = np.where(np.isfinite(a).all(axis=1, keepdims=True), a, np.array([[-0.5, -0.5, 0.5, 0.5]]))
    return np.round(a, 2).astype(F32)


def _pooled():
    ratios, scales = O.default_ratios_scales()
    anchors = O.create_anchors(LEVELS, ratios, scales).astype(F32)
    A = anchors.shape[0]
    assert A == 531
    g = torch.Generator().manual_seed(SEED_POOLED)
    att = (torch.randn(3, A, generator=g) * 1.5 - 3.0).numpy()
    reg = (torch.randn(3, A, 4, generator=g) * 0.08).numpy()
    att[0, 40], reg[0, 40] = 6.0, (0.3, -0.2, -3.0, -3.0)          # the best score of sample 0 on a box no other candidate overlaps
    att[1, :] = -1.25                                               # ties everywhere: candidates are anchors 0 .. pre_n - 1
    att[2, [3, 100, 317]] = np.nan
    att[2, 200], reg[2, 200, 2] = 5.0, np.nan                       # a finite best score on a box that does not decode
    img_size = np.array([[360, 480], [300, 300], [333, 500]], F32)
    # annotations that some rows hit: the boxes of rows 2 / 0 / 1 of one linear case, back in [-1, 1], rounded to 2 digits
    w = softnms_ref.soft_topk(att, reg, None, img_size, anchors, 64, 5, "soft_linear", 0.5, 0.5, 0.001, ACC_THR)["topk_boxes"]
    annot = _annot_from(np.stack([w[0, 2], w[1, 0], w[2, 1]]), img_size)
    return dict(out5=np.concatenate([reg, att[..., None]], axis=2).astype(F32), annot=annot, img_size=img_size, anchors=anchors)


def _cell():
    ratios, scales = O.default_ratios_scales()
    anchors = O.create_anchors([(1, 1)], ratios, scales).astype(F32)
    assert anchors.shape[0] == 9
    g = torch.Generator().manual_seed(SEED_CELL)
    att = (torch.randn(3, 9, generator=g) * 1.5 - 1.0).numpy()
    reg = (torch.randn(3, 9, 4, generator=g) * 0.3).numpy()
    att[1, [0, 2, 3, 5, 7, 8]] = np.nan
    att[2, :] = np.nan
    img_size = np.array([[200, 320], [128, 128], [240, 180]], F32)
    w = softnms_ref.soft_topk(att, reg, None, img_size, anchors, 16, 3, "soft_linear", 0.5, 0.5, 0.001, ACC_THR)["topk_boxes"]
    annot = _annot_from(np.stack([w[0, 1], w[1, 2], w[2, 0]]), img_size)
    return dict(out5=np.concatenate([reg, att[..., None]], axis=2).astype(F32), annot=annot, img_size=img_size, anchors=anchors)


_TABLES = {}


def inputs(table, method):
    """-> dict(out5 [B, A, 5], annot [B, 4], img_size [B, 2], anchors [A, 4]) of the samples listed for (table, method); built once"""
    if table not in _TABLES:
        _TABLES[table] = _pooled() if table == "pooled" else _cell()
    d = _TABLES[table]
    key = (table, method)
    if key not in _TABLES:
        rows = [0, 2] if (table == "pooled" and method == "soft_gauss") else [0, 1, 2]
        _TABLES[key] = dict(out5=np.ascontiguousarray(d["out5"][rows]), annot=np.ascontiguousarray(d["annot"][rows]),
                            img_size=np.ascontiguousarray(d["img_size"][rows]), anchors=d["anchors"], rows=rows)
    return _TABLES[key]


_REFS = {}


def reference(case):
    """softnms_ref.soft_topk on a case's inputs (with annot); with its trace; computed once per case and left unchanged"""
    if case not in _REFS:
        table, method, p, k, thr, sig, floor = case
        d = inputs(table, method)
        o = d["out5"]
        _REFS[case] = softnms_ref.soft_topk(o[..., 4], o[..., :4], d["annot"], d["img_size"], d["anchors"], p, k, method, thr, sig, floor,
                                            ACC_THR, trace=True)
    return _REFS[case]
