"""Fixture of the top-k grounding tests: tests/golden/g17_topk.npz (data only), made on the host from the REFERENCE's own functions.

    python tests/golden/make_topk_fixture.py

The reference has no NMS; the yardstick is composed from its pieces (code/anchors.py, imported here as make_golden.py imports it):
torch.sigmoid scores (evaluator.py:74), a stable descending sort (ties to the lower anchor index; a NaN score below every number),
reg_params_to_bbox on the first min(pre_n, A) candidates, greedy NMS in rank order — a candidate is kept unless
IoU_values(kept, candidate) > nms_thr for a box already kept, at most K boxes — and hit_rank / acc_at with
IoU_values(box, annot) >= acc_thr (evaluator.py:115-117).  Pixel boxes as evaluator.py:96-98.

Inputs are seeded noise plus planted entries ("patches"): a well-regressed anchor per query at a varying score rank, near-duplicates of it, exact logit ties
inside the top pre_n and across the cut, saturated scores, a query whose candidates collapse onto one box, NaN logits.  Small-A cases
are stored in full; the A = 17 460 case and the 600 x 600 case at the limits (pre_n = 512, K = 64) as seed + patches + expected outputs.

Device expf and the host's exp may differ in the last bit, so an input on a decision boundary would test the libm instead of the
kernel.  Every case must satisfy, on the reference (asserted below; seeds are searched until all hold, no case is ever dropped):
  1. among the top pre_n + 1 scores of a query, two neighbours come from bit-equal logits or differ by >= 4 ulp;
  2. every IoU of a candidate the greedy walk examines with a box kept before it is >= 1e-4 away from nms_thr;
  3. every IoU of a kept box with annot is >= 1e-4 away from acc_thr.
If torchvision is importable, the greedy NMS is also cross-checked against torchvision.ops.nms.
"""
import sys
sys.dont_write_bytecode = True   # never write __pycache__ into the reference tree
import os

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(REPO, "tests", "golden")
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REF, "code"))
from oracle import zsg_oracle as O   # noqa: E402  (seed-only batch generator, feature-map sizes)
import anchors as R                  # noqa: E402  (the reference's code/anchors.py)

try:
    from torchvision.ops import nms as tv_nms
except Exception:
    tv_nms = None

MARGIN = 1e-4
FS_SMALL = [(8, 8), (4, 4), (2, 2)]          # A = 756
FS_TINY = [(2, 2), (1, 1)]                   # A = 45
FS_FULL = O.feat_sizes_for(300, 300)         # A = 17 460
FS_600 = O.feat_sizes_for(600, 600)          # the 600 x 600 pyramid: an anchor range of a query no longer fits one LDS sort

# name, B, feature sizes, pre_n, K, nms_thr, plants, first seed tried
CASES = [
    dict(name="b16", B=16, fs=FS_SMALL, pre_n=128, K=5, nms_thr=0.5, plant=("good", "dups"), seed=100),
    dict(name="b1", B=1, fs=FS_SMALL, pre_n=128, K=5, nms_thr=0.5, plant=("good",), seed=200),
    dict(name="ties", B=2, fs=FS_SMALL, pre_n=32, K=5, nms_thr=0.5, plant=("good", "ties"), seed=300),
    dict(name="saturated", B=2, fs=FS_SMALL, pre_n=64, K=8, nms_thr=0.45, plant=("good", "saturated"), seed=400),
    dict(name="collapse", B=2, fs=FS_SMALL, pre_n=8, K=5, nms_thr=0.5, plant=("good", "collapse"), seed=500),
    dict(name="k1", B=3, fs=FS_SMALL, pre_n=16, K=1, nms_thr=0.5, plant=("good",), seed=600),
    dict(name="pre_gt_A", B=2, fs=FS_TINY, pre_n=64, K=4, nms_thr=0.3, plant=("nan",), seed=700),
    dict(name="nan", B=2, fs=FS_SMALL, pre_n=32, K=5, nms_thr=0.5, plant=("good", "nan"), seed=800),
    dict(name="limits", B=2, fs=FS_600, pre_n=512, K=64, nms_thr=0.5, plant=("good", "dups", "ties", "saturated"), seed=1000, seed_only=True),
    dict(name="full", B=4, fs=FS_FULL, pre_n=128, K=5, nms_thr=0.5, plant=("good", "dups", "ties", "saturated"), seed=900, seed_only=True),
]
ACC_THR = 0.5


def base_inputs(seed, B, A):
    """what the tests regenerate for a seed-only case: out5 [B, A, 5] = (reg, logit)"""
    g = torch.Generator().manual_seed(seed)
    att = torch.randn(B, A, 1, generator=g) * 1.5 - 3.0
    bbx = torch.randn(B, A, 4, generator=g) * 0.6
    return torch.cat([bbx, att], dim=2)


def build(case, seed, anchs):
    B, A, pre_n = case["B"], anchs.shape[0], case["pre_n"]
    out5 = base_inputs(seed, B, A)
    bt = O.synthetic_batch(B, 8, 8, seed=seed + 1)
    annot = bt["annot"].float()
    img_size = torch.tensor([[300.0 + 10 * b, 400.0 + 7 * b] for b in range(B)])        # (h, w)
    rng = np.random.default_rng(seed)
    patched = set()

    def patch(b, a, reg=None, logit=None):
        if reg is not None:
            out5[b, a, :4] = reg
        if logit is not None:
            out5[b, a, 4] = logit
        patched.add((b, int(a)))

    for b in range(B):
        srt = torch.sort(out5[b, :, 4], descending=True, stable=True)
        if "good" in case["plant"]:              # a well-regressed anchor at score rank ~ b % 7
            a = int(R.IoU_values(annot[b:b + 1], anchs)[0].argmax())
            reg = R.bbox_to_reg_params(anchs[a:a + 1], annot[b:b + 1])[0, 0]
            patch(b, a, reg=reg, logit=float(srt[0][min(b % 7, A - 1)]) + 0.01)
        if "dups" in case["plant"]:              # near-duplicates of the annotated box among the best scores: NMS has work to do
            cur = torch.sort(out5[b, :, 4], descending=True, stable=True)[1]
            for pos in (b % 7 + 1, b % 7 + 2, b % 7 + 4, b % 7 + 7):      # behind the well-regressed anchor
                a = int(cur[pos])
                jit = annot[b:b + 1] + torch.from_numpy(rng.uniform(-0.04, 0.04, (1, 4)).astype(np.float32))
                patch(b, a, reg=R.bbox_to_reg_params(anchs[a:a + 1], jit)[0, 0])
        if "saturated" in case["plant"]:         # sigmoid == 1.0f exactly
            for a in rng.choice(A, 3, replace=False):
                patch(b, int(a), logit=30.0)
        if "ties" in case["plant"]:              # bit-equal logits inside the top pre_n and across the cut (ranks after the plants above)
            srt = torch.sort(out5[b, :, 4], descending=True, stable=True)
            v = float(srt[0][pre_n - 1])
            for pos in (pre_n - 2, pre_n - 1, pre_n, pre_n + 1):
                patch(b, int(srt[1][pos]), logit=v)
            patch(b, int(srt[1][11]), logit=float(srt[0][10]))
        if "collapse" in case["plant"] and b == 0:      # every candidate decodes onto the annotated box: one box survives
            top = torch.sort(out5[b, :, 4], descending=True, stable=True)[1][:pre_n + 2]
            for a in top.tolist():
                patch(b, a, reg=R.bbox_to_reg_params(anchs[a:a + 1], annot[b:b + 1])[0, 0])
        if "nan" in case["plant"]:               # the would-be winner and one more anchor score NaN
            patch(b, int(out5[b, :, 4].argmax()), logit=float("nan"))
            patch(b, int(rng.integers(0, A)), logit=float("nan"))
    pidx = np.array(sorted(patched), np.int32).reshape(-1, 2)
    pval = np.stack([out5[b, a].numpy() for b, a in pidx]) if len(pidx) else np.zeros((0, 5), np.float32)
    return out5, annot, img_size, pidx, pval.astype(np.float32)


def ulps(hi, lo):
    return int(np.float32(hi).view(np.int32)) - int(np.float32(lo).view(np.int32))


def reference_topk(case, out5, annot, img_size, anchs):
    """-> (outputs, list of violated conditions)"""
    B, A, _ = out5.shape
    pre_n, K, nms_thr = case["pre_n"], case["K"], case["nms_thr"]
    att, reg = out5[..., 4], out5[..., :4]
    score = torch.sigmoid(att)
    key = torch.where(torch.isnan(score), torch.full_like(score, -1.0), score)
    order = torch.sort(key, dim=1, descending=True, stable=True)[1]
    boxes = torch.zeros(B, K, 4)
    scores = torch.zeros(B, K)
    idx = torch.full((B, K), -1, dtype=torch.int32)
    n = torch.zeros(B, dtype=torch.int32)
    hit = torch.full((B,), K, dtype=torch.int32)
    bad = []
    for b in range(B):
        top = order[b, :min(pre_n + 1, A)]
        s, x = score[b, top].numpy(), att[b, top].numpy()
        for i in range(len(top) - 1):                                  # condition 1
            if np.isnan(s[i]) or np.isnan(s[i + 1]):
                continue
            d = ulps(s[i], s[i + 1])
            if not (d >= 4 or (d == 0 and x[i].view(np.int32) == x[i + 1].view(np.int32))):
                bad.append(f"q{b}: scores at ranks {i},{i + 1} are {d} ulp apart")
        o = order[b, :min(pre_n, A)]
        cand = R.reg_params_to_bbox(anchs[o], reg[b, o][None])[0]
        kept = []
        for r in range(len(o)):
            if len(kept) == K:
                break
            if kept:
                ious = R.IoU_values(cand[kept], cand[r:r + 1])[:, 0]
                near = (ious - nms_thr).abs() < MARGIN                 # condition 2
                if bool(near.any()):
                    bad.append(f"q{b}: candidate {r} has an IoU within {MARGIN} of nms_thr")
                if bool((ious > nms_thr).any()):
                    continue
            kept.append(r)
        if tv_nms is not None and not bool(torch.isnan(cand).any() | torch.isnan(key[b, o]).any()):
            tv = tv_nms(cand[:, [1, 0, 3, 2]], torch.arange(len(o), 0, -1).float(), nms_thr)[:K].tolist()      # (scores: the rank order)
            assert tv == kept, (case["name"], b, tv, kept)
        kb = cand[kept]
        ia = R.IoU_values(kb, annot[b:b + 1])[:, 0]
        if bool(((ia - ACC_THR).abs() < MARGIN).any()):                # condition 3
            bad.append(f"q{b}: a kept box has an IoU within {MARGIN} of acc_thr")
        ok = ia >= ACC_THR
        if bool(ok.any()):
            hit[b] = int(ok.float().argmax())
        n[b] = len(kept)
        idx[b, :len(kept)] = o[kept].int()
        scores[b, :len(kept)] = score[b, o[kept]]
        # evaluator.py:96-98: (box + 1) / 2, times (h, w), then y1x1y2x2 -> x1y1x2y2
        half = (kb + 1) / 2
        px = torch.cat([img_size[b] * half[:, :2], img_size[b] * half[:, 2:]], dim=1)
        boxes[b, :len(kept)] = R.x1y1x2y2_to_y1x1y2x2(px)
    acc_at = torch.stack([(hit <= j).float().mean() for j in range(K)])
    res = dict(topk_boxes=boxes.numpy(), topk_scores=scores.numpy(), topk_idx=idx.numpy(), topk_n=n.numpy(), hit_rank=hit.numpy(),
               acc_at=acc_at.numpy())
    return res, bad


def main():
    ratios, scales = O.default_ratios_scales()
    arrs = {"cases": np.array([c["name"] for c in CASES]), "acc_thr": np.float32(ACC_THR)}
    anchor_sets = {}
    for case in CASES:
        key = str(case["fs"])
        if key not in anchor_sets:
            anchor_sets[key] = R.create_anchors(case["fs"], ratios, scales, device=torch.device("cpu")).float()
        anchs = anchor_sets[key]
        for seed in range(case["seed"], case["seed"] + 100):
            out5, annot, img_size, pidx, pval = build(case, seed, anchs)
            res, bad = reference_topk(case, out5, annot, img_size, anchs)
            if not bad:
                break
            print(f"{case['name']}: seed {seed} rejected ({bad[0]})")
        assert not bad, f"{case['name']}: no seed satisfies the input conditions"
        nm = case["name"]
        if case["name"] == "collapse":
            assert res["topk_n"][0] < case["K"]
        arrs.update({f"{nm}_seed": np.array([seed]), f"{nm}_pre_n": np.array([case["pre_n"]]), f"{nm}_K": np.array([case["K"]]),
                     f"{nm}_nms_thr": np.float32(case["nms_thr"]), f"{nm}_annot": annot.numpy(), f"{nm}_img_size": img_size.numpy(),
                     f"{nm}_patch_idx": pidx, f"{nm}_patch_val": pval})
        if case.get("seed_only"):               # the tests rebuild the anchors with the oracle: the same table, bit for bit
            assert np.array_equal(O.create_anchors(case["fs"], ratios, scales).astype(np.float32), anchs.numpy())
            arrs[f"{nm}_B"] = np.array([case["B"]])
            arrs[f"{nm}_fs"] = np.array(case["fs"], np.int32)
        else:
            arrs[f"{nm}_out5"] = out5.numpy()
            arrs[f"{nm}_anchors"] = anchs.numpy()
        arrs.update({f"{nm}_{k}": v for k, v in res.items()})
        sup = sum(int(res["topk_idx"][b, -1]) != int(torch.sort(torch.nan_to_num(torch.sigmoid(out5[b, :, 4]), nan=-1.0), descending=True, stable=True)[1][case["K"] - 1]) for b in range(case["B"]))
        print(f"{nm}: seed {seed}, A {anchs.shape[0]}, queries with a suppressed candidate among the best K: {sup}, topk_n {res['topk_n'].tolist()}, hit_rank {res['hit_rank'].tolist()}")
    path = os.path.join(OUT, "g17_topk.npz")
    np.savez_compressed(path, **arrs)
    print(f"g17_topk.npz  {os.path.getsize(path) / 1024:.1f} KB" + ("" if tv_nms else "  (torchvision not importable: no cross-check)"))


if __name__ == "__main__":
    main()
