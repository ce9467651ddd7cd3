"""Independent restatement of the task-aligned anchor assignment (cfg matcher = "tal") in numpy, for the tests.  It imports nothing of the
product: the definition is written out from INTEGRATION.md "Anchor assignment".  (tests/atss_ref.py supplies the toy pyramids and
compose(), the fp64 criterion on an arbitrary mask.)

Per sample: one annotation g (y1, x1, y2, x2), anchors [A, 4] fp32 in create_anchors' flattened order, the network output rows
(dy, dx, dh, dw, att) fp32.  In fp64 from the fp32 inputs:
    s = 1 / (1 + exp(-att))
    p = the decoded box: cy = ah dy + acy, cx = aw dx + acx, h = exp(dh) ah, w = exp(dw) aw, p = (cy - h/2, cx - w/2, cy + h/2, cx + w/2)
    u = inter / (union + 1e-7) of p with g; the min / max inside drop a NaN operand (C's fmin / fmax), the differences do not
    t = s^alpha * u^beta;  NaN where any of the five values of the row is NaN or u is NaN, i.e. a decode that overflows to inf - inf
        (numpy's power(nan, 0) is 1, so said outright)
and in np.float32, with ATSS's expressions, acy = (a.y1 + a.y2) / 2, acx = (a.x1 + a.x2) / 2, inside = g.y1 < acy < g.y2 and g.x1 < acx < g.x2.
    candidate: inside and t > 0 (false for NaN)
    selected:  the min(topk, #candidates) candidates first in the order (t descending, index ascending)
    metric:    t where inside (NaN stays NaN), -1.0 elsewhere
The device evaluates s in fp32 and rounds u to fp32 before the powers (the q of the quality term): metric_tolerance() is the relative
distance that allows, and gaps() is what test_cpu_tal.py demands of the seeded inputs so that the masks can be compared exactly."""
import functools

import numpy as np

import atss_ref as T

F32 = np.float32
TOPKS = (4, 13)
EXPONENTS = ((1.0, 6.0), (0.5, 2.0))
CASES = [(name, B) for name in T.PYRAMIDS for B in T.BATCHES]
# relative error of the device's fp32 quantities against their fp64 values, from the formats: the sigmoid is expf (within 1 ulp = 2^-23
# relative), one add and one IEEE divide (2^-24 each); u is one rounding of an fp64 value to fp32 (2^-24), doubled for the last bits of the
# two fp64 exp implementations where min / max differences cancel
E_S, E_U = 2.0 ** -22, 2.0 ** -23
GAP_FACTOR = 100.0


def metric_tolerance(alpha, beta):
    """relative tolerance of t = s^alpha u^beta to first order in the relative errors of s and u"""
    return alpha * E_S + beta * E_U


def inside_mask(g, anc):
    acy, acx = T.centres(anc)
    g = g.astype(F32)
    return (g[0] < acy) & (acy < g[2]) & (g[1] < acx) & (acx < g[3])


def decode(anc, reg):
    """fp64 boxes [A, 4] of the fp32 anchors [A, 4] and regression rows [A, 4]"""
    a, r = anc.astype(np.float64), reg.astype(np.float64)
    acy, acx = (a[:, 0] + a[:, 2]) / 2, (a[:, 1] + a[:, 3]) / 2
    ah, aw = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    cy, cx = ah * r[:, 0] + acy, aw * r[:, 1] + acx
    h, w = np.exp(r[:, 2]) * ah, np.exp(r[:, 3]) * aw
    return np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], axis=1)


def iou_f64(p, g):
    g = g.astype(np.float64)
    with np.errstate(invalid="ignore"):
        iy = np.fmax(np.fmin(p[:, 2], g[2]) - np.fmax(p[:, 0], g[0]), 0.0)
        ix = np.fmax(np.fmin(p[:, 3], g[3]) - np.fmax(p[:, 1], g[1]), 0.0)
        inter = iy * ix
        union = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1]) + (g[2] - g[0]) * (g[3] - g[1]) - inter
        return inter / (union + 1e-7)


def select(metric_row, topk):
    """the selection from one sample's metric row alone -> sorted candidate list (best first), the selected indices"""
    cand = [a for a in range(metric_row.shape[0]) if metric_row[a] > 0]          # (False for NaN and for the -1 of an outside anchor)
    cand.sort(key=lambda a: (-metric_row[a], a))
    return cand, cand[:min(topk, len(cand))]


def tal_match(att, reg, annot, anc, topk, alpha, beta):
    """-> dict: mask [B, A] bool (the selected anchors, WITHOUT the arg-max anchor the loss adds), metric [B, A] float64, inside [B, A],
    order (per sample the candidates, best first), s, u [B, A] float64"""
    att, reg, annot, anc = np.asarray(att, F32), np.asarray(reg, F32), np.asarray(annot, F32), np.asarray(anc, F32)
    alpha, beta = float(F32(alpha)), float(F32(beta))
    B, A = att.shape
    mask, metric = np.zeros((B, A), bool), np.full((B, A), -1.0)
    ins, order = np.zeros((B, A), bool), []
    s_all, u_all = np.zeros((B, A)), np.zeros((B, A))
    for b in range(B):
        with np.errstate(over="ignore", invalid="ignore"):
            s = 1.0 / (1.0 + np.exp(-att[b].astype(np.float64)))
            u = iou_f64(decode(anc, reg[b]), annot[b])
            t = np.power(s, alpha) * np.power(u, beta)
        t[np.isnan(att[b]) | np.isnan(reg[b]).any(axis=1) | np.isnan(u)] = np.nan
        ins[b] = inside_mask(annot[b], anc)
        metric[b] = np.where(ins[b], t, -1.0)
        cand, sel = select(metric[b], topk)
        mask[b, sel] = True
        order.append(cand)
        s_all[b], u_all[b] = s, u
    return dict(mask=mask, metric=metric, inside=ins, order=order, s=s_all, u=u_all)


def with_best(mask, annot, anc):
    """the positives the loss sees: the mask plus every sample's arg-max IoU anchor (lowest index) -> (mask, best [B])"""
    m = np.array(mask, bool)
    best = np.array([int(np.argmax(T.iou_f32(np.asarray(annot, F32)[b], anc))) for b in range(m.shape[0])], np.int64)
    m[np.arange(m.shape[0]), best] = True
    return m, best


def gaps(match, topk):
    """what an exact comparison of masks relies on -> (the smallest relative gap between the last selected and the first unselected key
    over the samples that have more than topk candidates, inf if none has; the smallest t of any candidate)"""
    gap, low = np.inf, np.inf
    for b, cand in enumerate(match["order"]):
        t = match["metric"][b]
        if cand:
            low = min(low, float(t[cand[-1]]))
        if len(cand) > topk:
            last, nxt = t[cand[topk - 1]], t[cand[topk]]
            gap = min(gap, float((last - nxt) / last))
    return gap, low


# ---- seeded inputs -------------------------------------------------------------------------------------------------------------------
# "trained": the regression output is the target of the annotation plus noise, so every decoded box lies near the annotation and the
# metric of every anchor inside it is far from 0; the annotation is an anchor that holds at least MIN_INSIDE anchor centres, jittered.
# "wild" (atss_ref.inputs): regression and scores unrelated to the annotation, IoUs of every size; used where no exact mask is compared.
SEEDS = {("P126", 1): 1, ("P126", 3): 1, ("P189", 1): 1, ("P189", 3): 1, ("P261", 1): 1, ("P261", 3): 1, ("full", 2): 1}
NOISE = {"full": 0.05}
MIN_INSIDE = 20


@functools.lru_cache(maxsize=None)
def inputs(O, name, B):
    """(att [B, A], reg [B, A, 4], annot [B, 4], anchors [A, 4]) fp32 of the "trained" kind"""
    anc, _ = T.pyramid_anchors(O, name)
    A = anc.shape[0]
    rs = np.random.RandomState(7919 * SEEDS[(name, B)] + 100 * A + B)
    acy, acx = T.centres(anc)
    holds = np.array([int(((anc[k, 0] < acy) & (acy < anc[k, 2]) & (anc[k, 1] < acx) & (acx < anc[k, 3])).sum()) for k in range(A)])
    ks = rs.choice(np.nonzero(holds >= MIN_INSIDE)[0], B, replace=False)
    annot = (anc[ks] + rs.uniform(-0.01, 0.01, (B, 4))).astype(F32)
    a, g = anc.astype(np.float64)[None], annot.astype(np.float64)[:, None]
    ah, aw = a[..., 2] - a[..., 0], a[..., 3] - a[..., 1]
    gh, gw = g[..., 2] - g[..., 0], g[..., 3] - g[..., 1]
    n = NOISE.get(name, 0.08) * rs.randn(B, A, 4)          # every anchor predicts the annotation, shifted and resized by a few per cent of its size
    cy, cx = (g[..., 0] + g[..., 2]) / 2 + gh * n[..., 0], (g[..., 1] + g[..., 3]) / 2 + gw * n[..., 1]
    reg = np.stack([(cy - (a[..., 0] + a[..., 2]) / 2) / ah, (cx - (a[..., 1] + a[..., 3]) / 2) / aw,
                    np.log(gh / ah) + n[..., 2], np.log(gw / aw) + n[..., 3]], axis=-1).astype(F32)
    att = (0.8 * rs.randn(B, A) + 0.5).astype(F32)
    return att, reg, annot, anc


@functools.lru_cache(maxsize=None)
def matched(O, name, B, topk, alpha, beta):
    att, reg, annot, anc = inputs(O, name, B)
    return tal_match(att, reg, annot, anc, topk, alpha, beta)
