"""Developer tool: device time of one optimizer step over a flat buffer of the headline model's size (net.store.flat.numel() of BASELINE
configs[1]: ResNet-50 at 300 px), for every rule of csrc/optim.hip with and without the weight average riding, beside csrc/adam.hip's
zsg_adam_step / zsg_adam_step_ema.  HIP events on the stream around each launch; the variants alternate round by round (every variant
sees the same clock state); the median of --calls rounds after --warmup, min and max next to it; algorithmic bytes (include/zsg.h) over
the median = achieved TB/s.  zsg_adam_step is timed twice per round (adam_step, adam_step_again): the distance between the two medians is
the spread of one and the same program, the yard-stick for every other comparison in the table.

--ab-lib PATH: another build of libzsg.so (the parent commit's), whose zsg_adam_step joins the rounds on the same buffers as parent_adam_step.
For context torch.optim.AdamW / SGD(momentum, foreach=True) over the network's ~170 parameter views are timed the same way (--no-torch skips).
--rule lamb: csrc/lamb.hip instead — zsg_lamb_moments, zsg_lamb_apply and the two together over the headline network's own segment table (every
parameter tensor, the two groups cfg opt_fn "LAMB" builds), beside zsg_adam_step_segments over the same table (timed twice: the yard-stick; with
--ab-lib the parent's too).
One JSON line at the end (--json PATH also writes it)."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zsgnet_pytorch_amd import _lib as L, config, mdl  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=60)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--n", type=int, default=0, help="elements of the flat buffer (default: the headline network's)")
ap.add_argument("--ab-lib", default=None, help="another libzsg.so whose zsg_adam_step is timed in the same rounds")
ap.add_argument("--rule", default="all", choices=["all", "lamb"], help="lamb: zsg_lamb_moments / zsg_lamb_apply over the headline network's "
                "segment table beside zsg_adam_step_segments over the same table (instead of the flat-buffer variants)")
ap.add_argument("--no-torch", action="store_true")
ap.add_argument("--json", default=None)
args = ap.parse_args()
L.require_gpu()

net = None
if not args.n or not args.no_torch:
    net = mdl.get_default_net(9, config.get_cfg()).to("cuda")
n = args.n or net.store.flat.numel()
gen = torch.Generator(device="cuda").manual_seed(7)
p = torch.randn(n, device="cuda", generator=gen)
g = torch.randn(n, device="cuda", generator=gen) * 1e-3
s0, s1, s2, ema = (torch.zeros(n, device="cuda") for _ in range(4))
step2 = torch.zeros(2, dtype=torch.int32, device="cuda")
LR, B1, B2, EPS, WD = 1e-4, 0.9, 0.99, 1e-8, 1e-2


def adam_entry(lib):
    fn = lib.zsg_adam_step
    fn.restype, fn.argtypes = L.SIGNATURES["zsg_adam_step"]
    return lambda: fn(p.data_ptr(), g.data_ptr(), s0.data_ptr(), s1.data_ptr(), n, LR, B1, B2, EPS, WD, 1.0, step2.data_ptr(), L.stream_ptr())


def general(algo, flags, grp, with_ema):
    head = (algo, flags, p.data_ptr(), g.data_ptr(), s0.data_ptr(), s1.data_ptr(), s2.data_ptr(), n, grp, 1.0, step2.data_ptr())
    if with_ema:
        return lambda: L.lib.zsg_optim_step_ema(*head, ema.data_ptr(), 0.001, L.stream_ptr())
    return lambda: L.lib.zsg_optim_step(*head, L.stream_ptr())


adam_g = L.OptimGroup(LR, B1, B2, EPS, WD, 0.0, 0.0, 0)
# name -> (bytes per parameter, the call)
variants = {"adam_step": (28, adam_entry(L.lib)), "adam_step_again": (28, adam_entry(L.lib)),
            "adam_step_ema": (36, lambda: L.lib.zsg_adam_step_ema(p.data_ptr(), g.data_ptr(), s0.data_ptr(), s1.data_ptr(), n, LR, B1, B2, EPS, WD, 1.0,
                                                                  step2.data_ptr(), ema.data_ptr(), 0.001, L.stream_ptr()))}
if args.ab_lib:
    variants["parent_adam_step"] = (28, adam_entry(C.CDLL(args.ab_lib)))
for name, algo, flags, grp, per in (
        ("optim_adam", L.OPT_ADAM, 0, adam_g, 28), ("optim_adamw", L.OPT_ADAMW, 0, adam_g, 28),
        ("optim_adam_amsgrad", L.OPT_ADAM, L.OPT_AMSGRAD, adam_g, 36), ("optim_adamw_amsgrad", L.OPT_ADAMW, L.OPT_AMSGRAD, adam_g, 36),
        ("optim_sgd_momentum", L.OPT_SGD, 0, L.OptimGroup(LR, 0, 0, 0, WD, 0.9, 0.0, 0), 20),
        ("optim_sgd_nesterov", L.OPT_SGD, 0, L.OptimGroup(LR, 0, 0, 0, WD, 0.9, 0.0, 1), 20),
        ("optim_sgd_plain", L.OPT_SGD, 0, L.OptimGroup(LR, 0, 0, 0, WD, 0.0, 0.0, 0), 12)):
    variants[name] = (per, general(algo, flags, grp, False))
    variants[name + "_ema"] = (per + 8, general(algo, flags, grp, True))

if args.rule == "lamb":
    # LAMB steps parameter tensors, not a flat range: the headline network's own segment table (every parameter, two groups as cfg opt_fn
    # "LAMB" builds them), timed beside the segmented Adam step (zsg_adam_step_segments) over the same table — this build's twice, and with
    # --ab-lib the parent's.  Bytes: the listed elements (each parameter padded to 4 floats) times 28 (Adam), 24 + 16 (LAMB's launches).
    from zsgnet_pytorch_amd import optim  # noqa: E402
    net = net or mdl.get_default_net(9, config.get_cfg()).to("cuda")
    plist = net._ordered_params()
    key = tuple((i, 0 if q.dim() >= 2 else 1) for i, q in enumerate(plist))
    tab, nch = optim.segment_table(net, key)
    nseg, n = len(key), net.store.flat.numel()
    listed = sum((q.numel() + 3) // 4 * 4 for q in plist)
    p = net.store.flat.detach().clone()
    g = torch.randn(n, device="cuda", generator=gen) * 1e-3
    s0, s1 = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    cnt = torch.zeros(nseg + 1, dtype=torch.int32, device="cuda")
    part = torch.empty(2 * nch, dtype=torch.float64, device="cuda")
    stats = torch.ones(3, nseg, device="cuda")
    ag = (L.AdamGroup * 2)(L.AdamGroup(LR, B1, B2, EPS, WD), L.AdamGroup(LR, B1, B2, EPS, 0.0))
    lg = (L.LambGroup * 2)(L.LambGroup(LR, B1, B2, EPS, WD, 1), L.LambGroup(LR, B1, B2, EPS, 0.0, 0))

    def adam_segments(lib):
        fn = lib.zsg_adam_step_segments
        fn.restype, fn.argtypes = L.SIGNATURES["zsg_adam_step_segments"]
        return lambda: fn(p.data_ptr(), g.data_ptr(), s0.data_ptr(), s1.data_ptr(), tab.data_ptr(), nseg, nch, ag, 2, 1.0, cnt.data_ptr(),
                          cnt[nseg:].data_ptr(), L.stream_ptr())

    def lamb_moments():
        return L.lib.zsg_lamb_moments(p.data_ptr(), g.data_ptr(), s0.data_ptr(), s1.data_ptr(), tab.data_ptr(), nseg, nch, lg, 2, 1.0, cnt.data_ptr(),
                                      part.data_ptr(), cnt[nseg:].data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(), stats[2].data_ptr(),
                                      L.stream_ptr())

    def lamb_apply():
        return L.lib.zsg_lamb_apply(p.data_ptr(), s0.data_ptr(), s1.data_ptr(), tab.data_ptr(), nseg, nch, lg, 2, stats[0].data_ptr(), cnt.data_ptr(),
                                    cnt[nseg:].data_ptr(), L.stream_ptr())

    variants = {"adam_step_segments": (28, adam_segments(L.lib)), "adam_step_segments_again": (28, adam_segments(L.lib)),
                "lamb_moments": (24, lamb_moments), "lamb_apply": (16, lamb_apply), "lamb_step": (40, lambda: lamb_moments() or lamb_apply())}
    if args.ab_lib:
        variants["parent_adam_step_segments"] = (28, adam_segments(C.CDLL(args.ab_lib)))
    args.no_torch = True
    n_bytes = listed
    print(f"{nseg} parameter tensors, {listed} listed elements in {nch} work chunks")

if not args.no_torch:          # context: what a user without the fused step runs, one multi-tensor update over the parameter views
    params = list(net.parameters())
    for q in params:
        q.grad = torch.randn_like(q) * 1e-3
    for name, opt in (("torch_adamw_foreach", torch.optim.AdamW(params, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, foreach=True)),
                      ("torch_sgd_momentum_foreach", torch.optim.SGD(params, lr=LR, momentum=0.9, weight_decay=WD, foreach=True))):
        variants[name] = (0, opt.step)


def timed(fn):
    """device milliseconds between two events around the call on torch's current stream"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    rc = fn()
    b.record()
    b.synchronize()
    assert rc in (0, None), L.lib.zsg_last_error().decode()
    return a.elapsed_time(b)


ms = {k: [] for k in variants}
for i in range(args.warmup + args.calls):
    for k, (_, fn) in variants.items():
        t = timed(fn)
        if i >= args.warmup:
            ms[k].append(t)

if args.rule == "lamb":
    n, same = n_bytes, ("adam_step_segments", "adam_step_segments_again")
else:
    same = ("adam_step", "adam_step_again")
res = {"what": f"one optimizer step over {n} fp32 parameters, HIP events around the launch, median of {args.calls} alternating rounds "
               f"after {args.warmup}", "n": n, "stamp": L.lib.zsg_source_stamp().decode(), "variants": {}}
print(f"{'variant':30s} {'ms':>8s} {'min':>8s} {'max':>8s} {'B/param':>8s} {'TB/s':>7s}")
for k, (per, _) in variants.items():
    v = sorted(ms[k])
    med = v[len(v) // 2]
    r = {"ms": round(med, 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}
    if per:
        r["bytes"] = per * n
        r["tb_per_s"] = round(per * n / (med * 1e-3) / 1e12, 3)
    res["variants"][k] = r
    print(f"{k:30s} {med:8.4f} {v[0]:8.4f} {v[-1]:8.4f} {per if per else '-':>8} {r.get('tb_per_s', '-'):>7}")
a, b = res["variants"][same[0]]["ms"], res["variants"][same[1]]["ms"]
res["same_program_spread"] = round(abs(a - b) / min(a, b), 4)
print(f"spread of one program ({same[0]} vs {same[1]}): {100 * res['same_program_spread']:.2f} %")
line = json.dumps(res)
print(line)
if args.json:
    with open(args.json, "w") as f:
        f.write(line + "\n")
