"""Developer tool: device time of the ZSGLoss call (loss + gradient kernels) at B = 16, A = 17460 on a fixed head output, for
cfg box_iou_loss = none / giou / diou and (--cls) cfg cls_quality = qfl / vfl, alternating call by call with none.  Each call is bracketed by the library's own HIP events (zsg_prof_enable: recorded on
the stream right before the first and after the last launch of the entry point), so the figure is the kernels and the gaps between them,
not the Python around them; the median of --calls calls after --warmup, min and max next to it.  One JSON line (--json PATH also writes it).
--kinds none restricts the set (a tree from before the IoU loss has only that one); --cls qfl,vfl adds those variants (each with
box_iou_loss none; "qfl+giou" names a box IoU loss next to it); --matcher iou,atss,tal times every variant under each anchor assignment
(cfg matcher; the atss / tal rows are named "atss", "atss+giou", "tal+qfl+giou", ... and are the sum of the two bracketed entry points,
zsg_match_atss or zsg_match_tal and zsg_loss_fwd_bwd_m; the matcher's own share is reported next to it as "<row>_match_us")."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import zsg_oracle as O  # noqa: E402
from zsgnet_pytorch_amd import _lib as L, config, loss  # noqa: E402
from zsgnet_pytorch_amd.synth import synthetic_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--calls", type=int, default=60)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--kinds", default="none,giou,diou")
ap.add_argument("--cls", default="", help="comma list of cls_quality variants timed next to --kinds: qfl, vfl, qfl+giou, ...")
ap.add_argument("--matcher", default="iou", help="comma list of cfg matcher values every variant is timed under: iou, atss, tal")
ap.add_argument("--json", default=None)
args = ap.parse_args()
B, A = args.batch, 17460
base = args.kinds.split(",") + [k for k in args.cls.split(",") if k]
kinds = [k if m == "iou" else (m if k == "none" else m + "+" + k) for m in args.matcher.split(",") for k in base]

gen = torch.Generator().manual_seed(7)
out5 = torch.cat([torch.randn(B, A, 4, generator=gen) * 0.3, torch.randn(B, A, 1, generator=gen) * 1.5 - 3.0], dim=2).cuda().requires_grad_()
bt = synthetic_batch(B, 8, 8, seed=1)
out = dict(att_bbx_out=out5, feat_sizes=torch.tensor(O.feat_sizes_for(300, 300)), num_f_out=torch.tensor([6]))
inp = {"annot": bt["annot"].cuda()}
lfs = {}
for k in kinds:
    parts = k.split("+")
    kw = {}
    if parts[0] in ("atss", "tal"):
        kw["matcher"] = parts.pop(0)
    for p in parts:
        if p in ("qfl", "vfl"):
            kw["cls_quality"] = p
        elif p != "none":
            kw["box_iou_loss"] = p
    c = config.get_cfg(**kw)
    lfs[k] = loss.get_default_loss(*config.ratios_scales(c), c)


def one_call(lf):
    """device milliseconds of one call"""
    ents = (L.ProfEntry * 16)()
    L.lib.zsg_prof_collect(ents, 16)                 # (drop earlier records)
    lf(out, inp)
    n = L.lib.zsg_prof_collect(ents, 16)             # (waits for the recorded events)
    got = {ents[i].name.decode(): (ents[i].launches, ents[i].ms) for i in range(n)}
    mine = [v for k, v in got.items() if k.startswith(("loss_fwd_bwd", "match_"))]
    assert len(mine) == (1 if lf.matcher == "iou" else 2) and all(calls == 1 for calls, _ in mine), got
    return sum(ms for _, ms in mine), sum(ms for k, (_, ms) in got.items() if k.startswith("match_"))


ms = {k: [] for k in kinds}
ms_match = {k: [] for k in kinds}
L.lib.zsg_prof_enable(1)
try:
    for i in range(args.warmup + args.calls):
        for k in kinds:                              # alternating: every variant sees the same clock state
            t, tm = one_call(lfs[k])
            if i >= args.warmup:
                ms[k].append(t)
                ms_match[k].append(tm)
finally:
    L.lib.zsg_prof_enable(0)
npos = lfs[kinds[0]].npos.cpu().tolist()
npos_atss = [lf.npos.cpu().tolist() for k, lf in lfs.items() if lf.matcher == "atss"][:1]
res = {"what": "ZSGLoss call, HIP events around the entry point's launches, median of %d calls" % args.calls, "B": B, "A": A,
       "positives_per_sample_min_max": [min(npos), max(npos)], "stamp": L.lib.zsg_source_stamp().decode()}
if npos_atss:
    res["positives_per_sample_min_max_atss"] = [min(npos_atss[0]), max(npos_atss[0])]
npos_tal = [lf.npos.cpu().tolist() for k, lf in lfs.items() if lf.matcher == "tal"][:1]
if npos_tal:
    res["positives_per_sample_min_max_tal"] = [min(npos_tal[0]), max(npos_tal[0])]
for k in kinds:
    v = sorted(ms[k])
    res[k + "_us"] = round(1e3 * v[len(v) // 2], 2)
    res[k + "_min_max_us"] = [round(1e3 * v[0], 2), round(1e3 * v[-1], 2)]
    if lfs[k].matcher != "iou":
        res[k + "_match_us"] = round(1e3 * sorted(ms_match[k])[len(v) // 2], 2)
line = json.dumps(res)
print(line)
if args.json:
    with open(args.json, "w") as f:
        f.write(line + "\n")
