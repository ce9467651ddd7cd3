"""Developer tool: one training step = forward, loss, backward, FusedAdam.step, evaluator; ResNet-50 FPN 300x300, synthetic batch.
--images N [--queries Q]: the shared-image training plan (ZSGNet.shared_training): Q queries (default 16) over N image slots, equal
groups; without --images the one-image-per-query step of Q pairs.  Prints one JSON line (ms per step over --steps timed steps that
end in a device synchronise)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zsgnet_pytorch_amd import config, evaluator, loss, mdl, optim
from zsgnet_pytorch_amd.synth import synthetic_batch

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=None, help="image slots per batch (shared-image training plan); default: one image per query")
ap.add_argument("--queries", type=int, default=16, help="queries per batch")
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--warmup", type=int, default=10)
args = ap.parse_args()
Q = args.queries
cfg = config.get_cfg()
net = mdl.get_default_net(9, cfg).to("cuda").train()
if args.images is None:
    bt = synthetic_batch(Q, 300, 300, seed=1)
else:
    from zsgnet_pytorch_amd.synth import synthetic_shared_batch
    if Q % args.images:
        raise SystemExit("--queries must be a multiple of --images (equal groups)")
    net.shared_training(True)
    bt = synthetic_shared_batch(args.images, Q, 300, 300, seed=1)
    g = torch.Generator().manual_seed(2)
    bt["img_idx"] = torch.arange(args.images).repeat_interleave(Q // args.images)[torch.randperm(Q, generator=g)]
bt = {k: v.cuda() for k, v in bt.items()}
r, s = config.ratios_scales(cfg)
lf, ev = loss.get_default_loss(r, s, cfg), evaluator.get_default_eval(r, s, cfg)
opt = optim.FusedAdam(net, lr=1e-4, betas=(0.9, 0.99))


def step():
    opt.zero_grad()
    out = net(bt)
    lf(out, bt)["loss"].mean().backward()
    opt.step()
    ev(out, bt)


for _ in range(args.warmup):
    step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(args.steps):
    step()
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / args.steps
print(json.dumps(dict(mode="plain" if args.images is None else "shared", images=Q if args.images is None else args.images, queries=Q,
                      steps=args.steps, ms_per_step=round(1e3 * dt, 4), queries_per_s=round(Q / dt, 1))))
