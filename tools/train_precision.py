"""Developer tool (a report, not a test): what the reduced-precision TRAINING switches do to a short training run — bf16 weight gradients
(cfg wgrad_dtype / ZSGNet.wgrad_precision("bf16")), the bf16 forward and data gradients of the pyramid and the heads (cfg train_dtype /
ZSGNet.train_precision("bf16_head")), both, the bf16 forward of the ResNet encoder (cfg enc_dtype / ZSGNet.encoder_precision("bf16_fwd"):
--switch enc), the bf16 data gradients of the ResNet encoder (cfg enc_bwd_dtype / ZSGNet.encoder_backward_precision("bf16"): --switch encb),
or all four (--switch all).  N Adam steps on seeded synthetic batches, once in fp32 and once with the switch, from the
SAME initial weights and the same batches; prints both loss curves, the distance of the first step's gradients (same weights, same batch:
the rounding's alone) and the relative L2 distance of the final weights.

    python tools/train_precision.py [--switch wgrad|train|both|enc|encb|all] [--steps 30] [--arch resnet50] [--size 300] [--bs 16] [--lr 1e-4] [--batches 4]

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
ap.add_argument("--switch", default="wgrad", choices=("wgrad", "train", "both", "enc", "encb", "all"))
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--arch", default="resnet50")
ap.add_argument("--size", type=int, default=300)
ap.add_argument("--bs", type=int, default=16)
ap.add_argument("--lr", type=float, default=1e-4)
ap.add_argument("--batches", type=int, default=4, help="distinct synthetic batches, visited round-robin")
a = ap.parse_args()

# (label, wgrad_dtype, train_dtype, enc_dtype, enc_bwd_dtype) of the two runs
ON = dict(wgrad=("bf16-wgrad", "bf16", "fp32", "fp32", "fp32"), train=("bf16_head", "fp32", "bf16_head", "fp32", "fp32"),
          both=("bf16_head+bf16-wgrad", "bf16", "bf16_head", "fp32", "fp32"), enc=("bf16_fwd-enc", "fp32", "fp32", "bf16_fwd", "fp32"),
          encb=("bf16-enc-dgrad", "fp32", "fp32", "fp32", "bf16"),
          all=("bf16-enc-dgrad+bf16_fwd-enc+bf16_head+bf16-wgrad", "bf16", "bf16_head", "bf16_fwd", "bf16"))[a.switch]
RUNS = (("fp32", "fp32", "fp32", "fp32", "fp32"), ON)

torch.cuda.set_device(0)
cfg = config.get_cfg(resnet_arch=a.arch, bs=a.bs, resize_img=[a.size, a.size])
r, s = config.ratios_scales(cfg)
lf = loss.get_default_loss(r, s, cfg)
batches = []
for i in range(a.batches):
    bt = {k: v.cuda() for k, v in synthetic_batch(a.bs, a.size, a.size, seed=100 + i).items()}
    bt["h0"], bt["c0"] = torch.zeros(2, a.bs, 128), torch.zeros(2, a.bs, 128)
    batches.append(bt)
sd, curves, final, g0, names, spans = None, {}, {}, {}, None, None
w_init = None
for label, wdt, tdt, edt, bdt in RUNS:
    torch.manual_seed(1234)
    net = mdl.get_default_net(9, cfg)
    if sd is None:
        sd = {k: v.clone() for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    net.to("cuda").train().wgrad_precision(wdt).train_precision(tdt).encoder_precision(edt).encoder_backward_precision(bdt)
    if w_init is None:
        w_init = net.store.flat.detach().double().cpu()
        names, spans = list(net._param_names), {n: (net.store.entries[n].offset, net.store.entries[n].size) for n in net._param_names}
    opt = optim.FusedAdam(net, lr=a.lr, betas=(0.9, 0.99))
    curves[label] = []
    for it in range(a.steps):
        bt = batches[it % len(batches)]
        opt.zero_grad()
        ls = lf(net(bt), bt)["loss"].mean()
        ls.backward()
        if it == 0:
            g0[label] = net.store.grad.detach().double().cpu()
        opt.step()
        curves[label].append(float(ls))
    torch.cuda.synchronize()
    final[label] = net.store.flat.detach().double().cpu()
on = ON[0]
print(f"train_precision: {a.arch} {a.size}x{a.size} B={a.bs}, {a.steps} Adam steps (lr {a.lr:g}) over {a.batches} synthetic batches; fp32 against {on}")
print(f"step   loss fp32     loss {on}   difference")
for it, (x, y) in enumerate(zip(curves["fp32"], curves[on])):
    print(f"{it:4d}   {x:.6f}    {y:.6f}        {y - x:+.2e}")
ga, gb = g0["fp32"], g0[on]
print(f"first step's gradient (same weights, same batch): ||g - g_fp32||_2 / ||g_fp32||_2 = {float((gb - ga).norm() / ga.norm()):.3e}, "
      f"cosine = {float((ga * gb).sum() / (ga.norm() * gb.norm())):.6f}")
per = sorted(((float((gb[o:o + n] - ga[o:o + n]).norm() / ga[o:o + n].norm()), nm) for nm, (o, n) in spans.items() if float(ga[o:o + n].norm()) > 0), reverse=True)
print("  largest per-parameter distances: " + ", ".join(f"{nm} {v:.2e}" for v, nm in per[:5]) + f"; median {per[len(per) // 2][0]:.2e}; bit-equal parameters: "
      f"{sum(1 for nm, (o, n) in spans.items() if torch.equal(ga[o:o + n], gb[o:o + n]))} of {len(spans)}")
d = final[on] - final["fp32"]
moved = float((final["fp32"] - w_init).norm())
print(f"distance travelled by the fp32 run: ||w_fp32 - w_init||_2 = {moved:.3e}; ||w - w_fp32||_2 / that = {float(d.norm()) / moved:.3e}")
print(f"final weights: ||w - w_fp32||_2 / ||w_fp32||_2 = {float(d.norm() / final['fp32'].norm()):.3e}, max |difference| = {float(d.abs().max()):.3e}")
