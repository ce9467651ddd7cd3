"""Developer tool: how far the bf16 and bf16_act eval plans (cfg eval_dtype, ZSGNet.eval_precision) land from the fp32 eval plan of the SAME
weights.  ResNet-50 FPN 300x300, B = 16 (--arch / --hw / --batch change it), oracle.seeded_state_dict(arch, 1), a synthetic batch.
Prints, for bf16 against fp32 (the keys it always had) and for bf16_act against fp32 (the same keys with the prefix "act_"): max and mean |delta| of the box channels and of the att channel relative to max|fp32| of those
channels, the share of queries whose evaluator pred_idx agrees, and both Acc values — one JSON line (--json PATH also writes it to a
file)."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--arch", default="resnet50")
ap.add_argument("--hw", type=int, default=300)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--json", default=None, help="also write the result line to this file")
args = ap.parse_args()

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import zsg_oracle as O
from zsgnet_pytorch_amd import config, evaluator, mdl
from zsgnet_pytorch_amd.synth import synthetic_batch

cfg = config.get_cfg(resnet_arch=args.arch)
net = mdl.get_default_net(9, cfg)
net.load_state_dict(O.seeded_state_dict(args.arch, args.seed))
net.to("cuda").eval()
bt = {k: v.cuda() for k, v in synthetic_batch(args.batch, args.hw, args.hw, seed=1).items()}
g = torch.Generator().manual_seed(0)
nd = 2 if cfg["use_bidirectional"] else 1
bt["h0"], bt["c0"] = torch.randn(nd, args.batch, cfg["lstm_dim"], generator=g), torch.randn(nd, args.batch, cfg["lstm_dim"], generator=g)
r, s = config.ratios_scales(cfg)
ev = evaluator.get_default_eval(r, s, cfg).eval()
res = {}
with torch.no_grad():
    for dtype in ("fp32", "bf16", "bf16_act"):
        out = net.eval_precision(dtype)(bt)
        em = ev(out, bt)
        torch.cuda.synchronize()
        res[dtype] = (out["att_bbx_out"].double().cpu(), ev.pred_idx.cpu().clone(), float(em["Acc"]))
a = res["fp32"][0]
sb, sa = float(a[..., :4].abs().max()), float(a[..., 4].abs().max())
rec = {"what": "bf16 / bf16_act (act_*) eval plans against the fp32 eval plan of the same weights, relative to max|fp32| per channel group",
       "arch": args.arch, "hw": args.hw, "B": args.batch, "acc_fp32": res["fp32"][2]}
for dtype, pre in (("bf16", ""), ("bf16_act", "act_")):
    b = res[dtype][0]
    box, att = (b[..., :4] - a[..., :4]).abs(), (b[..., 4] - a[..., 4]).abs()
    rec.update({pre + "box_max": float(box.max()) / sb, pre + "box_mean": float(box.mean()) / sb, pre + "att_max": float(att.max()) / sa,
                pre + "att_mean": float(att.mean()) / sa, pre + "pred_idx_agree": float((res["fp32"][1] == res[dtype][1]).float().mean()),
                "acc_" + dtype: res[dtype][2]})
line = json.dumps(rec)
print(line)
if args.json:
    with open(args.json, "w") as f:
        f.write(line + "\n")
