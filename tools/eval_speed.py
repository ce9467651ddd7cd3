"""Developer tool: eval-mode (validation) forward + loss + evaluator throughput, ResNet-50 FPN 300x300, B=16.
--images N [--queries Q]: the shared-image eval plan instead (ZSGNet.forward with img_idx): Q queries (default 16) over N distinct
images per batch; without --images the one-image-per-query path, as before."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zsgnet_pytorch_amd import config, evaluator, loss, mdl
from zsgnet_pytorch_amd.synth import synthetic_batch, synthetic_shared_batch

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=None, help="distinct images per batch (shared-image plan); default: one image per query")
ap.add_argument("--queries", type=int, default=16, help="queries per batch")
args = ap.parse_args()
Q = args.queries
cfg = config.get_cfg()
net = mdl.get_default_net(9, cfg).to("cuda").eval()
if args.images is None:
    bt = synthetic_batch(Q, 300, 300, seed=1)
else:
    bt = synthetic_shared_batch(args.images, Q, 300, 300, seed=1)
bt = {k: v.cuda() for k, v in bt.items()}
r, s = config.ratios_scales(cfg)
lf, ev = loss.get_default_loss(r, s, cfg), evaluator.get_default_eval(r, s, cfg)
with torch.no_grad():
    for _ in range(5):
        out = net(bt); lf(out, bt); ev(out, bt)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):
        out = net(bt); lf(out, bt); ev(out, bt)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 50
if args.images is None:
    print(f"eval: {1e3 * dt:.3f} ms per batch of {Q} -> {Q / dt:.0f} img/s")
else:
    print(f"eval (shared): {1e3 * dt:.3f} ms per batch of {Q} queries over {args.images} images -> {Q / dt:.0f} queries/s")
