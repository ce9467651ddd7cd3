"""Developer tool (a report, not a test): what bf16 weight gradients (cfg wgrad_dtype / ZSGNet.wgrad_precision("bf16")) do to a short
training run.  N Adam steps on seeded synthetic batches, once with wgrad_dtype = fp32 and once with bf16, from the SAME initial weights
and the same batches; prints both loss curves and the relative L2 distance of the final weights.

    python tools/train_precision.py [--steps 30] [--arch resnet50] [--size 300] [--bs 16] [--lr 1e-4] [--batches 4]

ZSG_DETERMINISTIC=1 is set, so the fp32 run is reproducible and the distance is the bf16 rounding's alone."""
import argparse
import os
import sys

os.environ.setdefault("ZSG_DETERMINISTIC", "1")
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zsgnet_pytorch_amd import config, loss, mdl, optim  # noqa: E402
from zsgnet_pytorch_amd.synth import synthetic_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--arch", default="resnet50")
ap.add_argument("--size", type=int, default=300)
ap.add_argument("--bs", type=int, default=16)
ap.add_argument("--lr", type=float, default=1e-4)
ap.add_argument("--batches", type=int, default=4, help="distinct synthetic batches, visited round-robin")
a = ap.parse_args()

torch.cuda.set_device(0)
cfg = config.get_cfg(resnet_arch=a.arch, bs=a.bs, resize_img=[a.size, a.size])
r, s = config.ratios_scales(cfg)
lf = loss.get_default_loss(r, s, cfg)
batches = []
for i in range(a.batches):
    bt = {k: v.cuda() for k, v in synthetic_batch(a.bs, a.size, a.size, seed=100 + i).items()}
    bt["h0"], bt["c0"] = torch.zeros(2, a.bs, 128), torch.zeros(2, a.bs, 128)
    batches.append(bt)
sd, curves, final = None, {}, {}
w_init = None
for dtype in mdl.WGRAD_DTYPES:
    torch.manual_seed(1234)
    net = mdl.get_default_net(9, cfg)
    if sd is None:
        sd = {k: v.clone() for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    net.to("cuda").train().wgrad_precision(dtype)
    if w_init is None:
        w_init = net.store.flat.detach().double().cpu()
    opt = optim.FusedAdam(net, lr=a.lr, betas=(0.9, 0.99))
    curves[dtype] = []
    for it in range(a.steps):
        bt = batches[it % len(batches)]
        opt.zero_grad()
        ls = lf(net(bt), bt)["loss"].mean()
        ls.backward()
        opt.step()
        curves[dtype].append(float(ls))
    torch.cuda.synchronize()
    final[dtype] = net.store.flat.detach().double().cpu()
print(f"train_precision: {a.arch} {a.size}x{a.size} B={a.bs}, {a.steps} Adam steps (lr {a.lr:g}) over {a.batches} synthetic batches")
print("step   loss fp32     loss bf16-wgrad   difference")
for it, (x, y) in enumerate(zip(curves["fp32"], curves["bf16"])):
    print(f"{it:4d}   {x:.6f}    {y:.6f}        {y - x:+.2e}")
d = final["bf16"] - final["fp32"]
moved = float((final["fp32"] - w_init).norm())
print(f"distance travelled by the fp32 run: ||w_fp32 - w_init||_2 = {moved:.3e}; ||w_bf16 - w_fp32||_2 / that = {float(d.norm()) / moved:.3e}")
print(f"final weights: ||w_bf16 - w_fp32||_2 / ||w_fp32||_2 = {float(d.norm() / final['fp32'].norm()):.3e}, max |difference| = {float(d.abs().max()):.3e}")
