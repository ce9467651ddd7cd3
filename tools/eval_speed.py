"""Developer tool: eval-mode (validation) forward + loss + evaluator throughput, ResNet-50 FPN 300x300, B=16.
--images N [--queries Q]: the shared-image eval plan instead (ZSGNet.forward with img_idx): Q queries (default 16) over N distinct
images per batch; without --images the one-image-per-query path, as before.
--topk K [--pre-nms N] [--queries Q]: the evaluator call alone, on a fixed [Q, 17460, 5] head output: eval_topk = 1 (zsg_eval only) against
eval_topk = K in eval mode (zsg_eval + zsg_eval_topk), alternating; device events around groups of calls, the median per call of each, one
JSON line (--json PATH also writes it to a file).  --nms soft_linear|soft_gauss (one or both): the same call with cfg eval_nms set
(zsg_eval + zsg_eval_topk_soft) joins the alternation, `<name>_us` per rule.
--dtype fp32|bf16|bf16_act: cfg eval_dtype of the network (the forward paths; --topk times no network).
--head-ctx none|gc: cfg head_ctx of the network (gc: the global-context block behind the heads' conv0, with drawn weights and a non-zero
last layer); composes with every forward path above.
--tta flip: flip test-time augmentation (cfg eval_tta): the eval FORWARD of the same network at the same B = --queries, three ways,
alternating — the plain batch, the plain batch at 2B, the TTA batch (2B rows in one forward + the staging and merge launches) — and the
two new launches alone; device events around groups of calls, the median per call of each, one JSON line (--json PATH also writes it to
a file).  Works with --dtype and --images / --queries.  The expectation to read it against: TTA ~ plain 2B + merge.
--scales 0.75,1.25 [--vote THR]: multi-scale test-time augmentation (cfg eval_scales) on a uint8 batch, alternating — the plain eval
forward, the multi-scale forward, every pass alone (the plain forward on the resampled batch) — the resample launches alone, and the
wall-clock time of the first multi-scale batch (the new geometries lower and tune there).  --vote THR (cfg eval_box_vote): the evaluator
call on that forward's output with and without the vote, and zsg_eval_vote alone (with --topk K as its K, else 1).  Composes with --tta flip
(every forward of the comparison then runs flip TTA), --dtype, --images / --queries.  One JSON line (--json PATH also writes it)."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", choices=("fp32", "bf16", "bf16_act"), default="fp32",
                help="eval_dtype: operand precision of the eval plan's convolutions (bf16_act: bf16 activation storage as well)")
ap.add_argument("--head-ctx", choices=("none", "gc"), default="none", help="head_ctx: the global-context block of the head towers")
ap.add_argument("--per-kernel", action="store_true", help="also print the per-launch device times of one forward and the plan's bytes")
ap.add_argument("--images", type=int, default=None, help="distinct images per batch (shared-image plan); default: one image per query")
ap.add_argument("--queries", type=int, default=16, help="queries per batch")
ap.add_argument("--topk", type=int, default=None, help="time the evaluator call with and without the top-k launch (K boxes per query)")
ap.add_argument("--pre-nms", type=int, default=128, help="with --topk: candidates per query that enter the NMS")
ap.add_argument("--nms", nargs="+", choices=("soft_linear", "soft_gauss"), default=[],
                help="with --topk: also time the evaluator call with eval_nms set to these Soft-NMS rules")
ap.add_argument("--tta", choices=("flip",), default=None, help="time the eval forward plain at B, plain at 2B and with eval_tta=flip at B, and the two TTA launches alone")
ap.add_argument("--scales", default=None, help="comma-separated eval_scales, e.g. 0.75,1.25: time the multi-scale eval forward against the plain one, pass by pass")
ap.add_argument("--vote", type=float, default=None, help="eval_box_vote threshold: time the evaluator with and without the vote and zsg_eval_vote alone (on the --scales output when given)")
ap.add_argument("--json", default=None, help="with --topk / --tta / --scales / --vote: also write the result line to this file")
args = ap.parse_args()          # (before the heavy imports: --help and a bad value answer at once)

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zsgnet_pytorch_amd import config, evaluator, loss, mdl
from zsgnet_pytorch_amd.synth import synthetic_batch, synthetic_shared_batch

Q = args.queries
cfg = config.get_cfg(eval_dtype=args.dtype, head_ctx=args.head_ctx)


def time_topk():
    from oracle import zsg_oracle as O
    A, groups, per_group = 17460, 41, 25
    gen = torch.Generator().manual_seed(7)
    out5 = torch.cat([torch.randn(Q, A, 4, generator=gen) * 0.6, torch.randn(Q, A, 1, generator=gen) * 1.5 - 3.0], dim=2).cuda()
    bt = synthetic_batch(Q, 8, 8, seed=1)
    out = dict(att_bbx_out=out5, feat_sizes=torch.tensor(O.feat_sizes_for(300, 300)), num_f_out=torch.tensor([6]))
    inp = {k: bt[k].cuda() for k in ("annot", "img_size", "idxs")}
    evs = {}
    for name, k, nms in [("plain", 1, "hard"), ("topk", args.topk, "hard")] + [(m, args.topk, m) for m in args.nms]:
        c = config.get_cfg(eval_topk=k, eval_pre_nms=args.pre_nms, eval_nms=nms)
        evs[name] = evaluator.get_default_eval(*config.ratios_scales(c), c).eval()
    ms = {name: [] for name in evs}
    for g in range(groups + 3):                      # the first 3 groups are warm-up
        for name, e in evs.items():                  # alternating: all see the same clock state
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(per_group):
                e(out, inp)
            t1.record()
            t1.synchronize()
            if g >= 3:
                ms[name].append(t0.elapsed_time(t1) / per_group)
    med = {name: sorted(v)[len(v) // 2] for name, v in ms.items()}
    res = {"what": "evaluator call, eval mode, device events, median of %d groups of %d calls" % (groups, per_group), "B": Q, "A": A,
           "K": args.topk, "pre_nms": args.pre_nms, "plain_us": round(1e3 * med["plain"], 2), "topk_us": round(1e3 * med["topk"], 2),
           "ratio": round(med["topk"] / med["plain"], 3), "plain_min_max_us": [round(1e3 * min(ms["plain"]), 2), round(1e3 * max(ms["plain"]), 2)],
           "topk_min_max_us": [round(1e3 * min(ms["topk"]), 2), round(1e3 * max(ms["topk"]), 2)]}
    for m in args.nms:
        c = evs[m].cfg
        res.update({m + "_us": round(1e3 * med[m], 2), m + "_over_topk": round(med[m] / med["topk"], 3),
                    m + "_min_max_us": [round(1e3 * min(ms[m]), 2), round(1e3 * max(ms[m]), 2)],
                    m + "_mean_rows": round(float(evs[m](out, inp)["topk_n"].float().mean()), 2)})
    if args.nms:
        res.update({"nms_thr": c["eval_nms_thr"], "soft_sigma": c["eval_soft_sigma"], "soft_min_score": c["eval_soft_min_score"]})
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if args.topk is not None and args.scales is None and args.vote is None:
    time_topk()
    sys.exit(0)
net = mdl.get_default_net(9, cfg)
if args.head_ctx == "gc":           # (drawn gc tensors: the fresh net's zero last layer would time the same launches on t = 0)
    g_ = torch.Generator().manual_seed(0)
    net.load_state_dict({k: (torch.randn(v.shape, generator=g_) * 0.05 + (1.0 if k.endswith("ln.weight") else 0.0)) for k, v in net.state_dict().items()
                         if ".gc." in k}, strict=False)
net = net.to("cuda").eval()


def _median_groups(fns, groups, per_group, warm=3):
    """{name: fn} -> {name: [ms per call of every group]}, the functions alternating group by group (all see the same clock state)"""
    ms = {k: [] for k in fns}
    for g in range(groups + warm):
        for name, fn in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(per_group):
                fn()
            t1.record()
            t1.synchronize()
            if g >= warm:
                ms[name].append(t0.elapsed_time(t1) / per_group)
    return ms


def time_scales():
    from zsgnet_pytorch_amd._lib import check, lib, stream_ptr
    scales = [float(v) for v in args.scales.split(",")] if args.scales else []
    K = args.topk or 1
    Bi = args.images
    b = synthetic_batch(Q, 300, 300, seed=1) if Bi is None else synthetic_shared_batch(Bi, Q, 300, 300, seed=1)
    b["img"] = (b["img"].permute(0, 2, 3, 1) * 255).round().to(torch.uint8).contiguous()
    b = {k: v.cuda() for k, v in b.items()}
    net.eval_tta(args.tta or "none")
    sizes = mdl.eval_scale_sizes(300, 300, scales)
    res = {"what": "eval forward on a uint8 batch, device events, median ms per batch; launches alone back to back, us", "dtype": args.dtype,
           "tta": args.tta or "none", "B": Q, "images": Bi, "scales": scales, "sizes": sizes}
    with torch.no_grad():
        net.eval_scales(())
        net(b)
        torch.cuda.synchronize()
        net.eval_scales(scales)
        t0 = time.perf_counter()
        out = net(b)
        torch.cuda.synchronize()
        res["first_multi_scale_batch_s"] = round(time.perf_counter() - t0, 2)
        if scales:
            passes = {f"pass_{h}x{w}": dict(b, img=net._resample(b["img"], h, w).clone()) for h, w in sizes}

            def plain(x):
                net.eval_scales(())
                net(x)

            def multi():
                net.eval_scales(scales)
                net(b)
            fns = {"plain": lambda: plain(b), "multi_scale": multi, **{k: (lambda x=x: plain(x)) for k, x in passes.items()}}
            ms = _median_groups(fns, 15, 5)
            med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
            res.update({k + "_ms": round(v, 4) for k, v in med.items()})
            res.update({k + "_min_max_ms": [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()})
            res["multi_over_plain"] = round(med["multi_scale"] / med["plain"], 4)
            res["sum_of_passes_ms"] = round(med["plain"] + sum(med[k] for k in passes), 4)
            rs = _median_groups({f"resample_{h}x{w}": (lambda h=h, w=w: net._resample(b["img"], h, w)) for h, w in sizes}, 15, 100)
            res.update({k + "_us": round(1e3 * sorted(v)[len(v) // 2], 2) for k, v in rs.items()})
            net.eval_scales(scales)
            out = net(b)
        if args.vote is not None:
            r, s = config.ratios_scales(cfg)
            evs = {name: evaluator.get_default_eval(r, s, config.get_cfg(eval_topk=K, eval_pre_nms=args.pre_nms, eval_box_vote=v)).eval()
                   for name, v in (("evaluator", 0.0), ("evaluator_vote", args.vote))}
            ev = evs["evaluator_vote"]
            em = ev(out, b)
            o5, anchs = ev._out5_anchors(out)
            A = o5.shape[1]
            annot, sz = b["annot"].contiguous().float(), b["img_size"].contiguous().float()
            tk = ev._topk(o5, anchs, annot, sz, K)
            fns = {name: (lambda e=e: e(out, b)) for name, e in evs.items()}
            fns["zsg_eval_vote"] = lambda: ev._vote(o5, anchs, annot, sz, K, tk)
            ms = _median_groups(fns, 21, 25)
            res.update({"A": A, "K": K, "pre_nms": args.pre_nms, "vote_thr": args.vote, "mean_members": round(float(em["vote_n"].float().mean()), 2)})
            res.update({k + "_us": round(1e3 * sorted(v)[len(v) // 2], 2) for k, v in ms.items()})
            res.update({k + "_min_max_us": [round(1e3 * min(v), 2), round(1e3 * max(v), 2)] for k, v in ms.items()})
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if args.scales is not None or args.vote is not None:
    time_scales()
    sys.exit(0)


def time_tta():
    from zsgnet_pytorch_amd._lib import check, lib, stream_ptr
    groups, per_group = 21, 10
    Bi = args.images

    def batch(q, bi, seed):
        b = synthetic_batch(q, 300, 300, seed=seed) if bi is None else synthetic_shared_batch(bi, q, 300, 300, seed=seed)
        return {k: v.cuda() for k, v in b.items()}
    b1, b2 = batch(Q, Bi, 1), batch(2 * Q, None if Bi is None else 2 * Bi, 2)
    runs = {"plain_B": ("none", b1), "plain_2B": ("none", b2), "tta_B": ("flip", b1)}
    ms = {k: [] for k in runs}
    with torch.no_grad():
        for g in range(groups + 3):                  # the first 3 groups are warm-up (they lower and tune the two plans)
            for name, (mode, b) in runs.items():     # alternating: all three see the same clock state
                net.eval_tta(mode)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(per_group):
                    net(b)
                t1.record()
                t1.synchronize()
                if g >= 3:
                    ms[name].append(t0.elapsed_time(t1) / per_group)
        net.eval_tta("flip")
        geo = net.plan_geometry(b1)                  # (B, H, W, T) or, for queries sharing images, (Bi, Q, H, W, T): the cached TTA plan
        plan = net._plan_for(*geo) if Bi is None else net._plan_for(geo[0], geo[2], geo[3], geo[4], Q=geo[1])
        A, lv = plan.A, plan._tta_levels()
        n_img = Q if Bi is None else Bi
        img = b1["img"].contiguous()
        x0 = torch.empty(2 * n_img, 300, 300, 4, device="cuda")
        o2, om = torch.randn(2 * Q, A, 5, device="cuda"), torch.empty(Q, A, 5, device="cuda")
        alone = {"stage_f32": lambda: check(lib.zsg_tta_flip_stage_f32(img.data_ptr(), n_img, 300, 300, x0.data_ptr(), stream_ptr()), "stage"),
                 "merge": lambda: check(lib.zsg_tta_flip_merge(o2.data_ptr(), Q, A, lv.ctypes.data, lv.shape[0], om.data_ptr(), stream_ptr()), "merge")}
        us = {}
        for name, fn in alone.items():
            v = []
            for g in range(groups + 3):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(100):
                    fn()
                t1.record()
                t1.synchronize()
                if g >= 3:
                    v.append(10.0 * t0.elapsed_time(t1))          # ms per 100 launches -> us per launch (back to back: includes the launch gap)
            us[name] = sorted(v)[len(v) // 2]
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    res = {"what": "eval forward, device events, median of %d groups of %d calls, ms per batch; launches alone back to back, us" % (groups, per_group),
           "dtype": args.dtype, "B": Q, "images": Bi, "A": A,
           **{k + "_ms": round(v, 4) for k, v in med.items()},
           **{k + "_min_max_ms": [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
           "tta_over_plain_2B": round(med["tta_B"] / med["plain_2B"], 4), "tta_over_plain_B": round(med["tta_B"] / med["plain_B"], 4),
           **{k + "_us": round(v, 2) for k, v in us.items()}}
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if args.tta is not None:
    time_tta()
    sys.exit(0)
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
plan = next(reversed(net._plans.values()))
print(f"plan bytes [{args.dtype}]: {plan.bytes} ({plan.bytes / 2**20:.1f} MiB), {len(plan.fwd.calls)} launches")
if args.per_kernel:
    from zsgnet_pytorch_amd._lib import stream_ptr
    torch.cuda.synchronize()
    rows = plan.fwd.profile(stream_ptr())
    for r_ in rows:
        print("  ", r_)
if args.images is None:
    print(f"eval [{args.dtype}]: {1e3 * dt:.3f} ms per batch of {Q} -> {Q / dt:.0f} img/s")
else:
    print(f"eval (shared) [{args.dtype}]: {1e3 * dt:.3f} ms per batch of {Q} queries over {args.images} images -> {Q / dt:.0f} queries/s")
