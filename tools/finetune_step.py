"""Developer tool: ms per training step at BASELINE configs[1] (ResNet-50 + FPN, 300x300, B = 16) with parts of the network frozen
(requires_grad=False), timed with device events in ONE process, the variants alternating round by round so that clock and thermal drift
fall on all of them alike.  Each variant has its own network (a change of the trainable set re-lowers the plan), the same weights and
batch.  Prints one JSON object: per variant the median ms per step over the rounds, all round medians, the backward program's launch
count and the number of stepped parameters.

    python tools/finetune_step.py [--rounds 5] [--steps 10] [--warmup 3] [--out profiles/finetune_step.json]
    python tools/finetune_step.py --frozen-bn [--out profiles/finetune_step_frozen_bn.json]

--frozen-bn measures every BatchNorm layer frozen (ZSGNet.freeze_batchnorm) against train-mode BatchNorm, with everything trainable
and with the encoder's parameters frozen.

    python tools/finetune_step.py --clip [--out profiles/finetune_step_clip.json]

--clip measures gradient-norm clipping between backward and step, everything trainable: no clipping, the fused optim.clip_grad_norm_
with a max_norm it never reaches (the scale pass reads its coefficient and exits), the fused clip engaged (every gradient scaled), and
torch.nn.utils.clip_grad_norm_ engaged on the same p.grad views.

    python tools/finetune_step.py --sync-bn [--out profiles/finetune_step_sync_bn.json]

--sync-bn measures synchronized BatchNorm in a 1-rank nccl group with forced collectives: the DistributedDataParallel wrapper
(force_collectives) against the same wrapper with dist.convert_sync_batchnorm(force=True) — one all-reduce per train-mode BatchNorm layer
and direction on top of the gradient buckets.

    python tools/finetune_step.py --ema [--out profiles/ema_step.json]

--ema measures the weight average (ema.ModelEma, decay 0.999), everything trainable: none, attached to FusedAdam (the update rides in the
Adam launch: zsg_adam_step_ema + the statistics' zsg_ema_update), update() after an unattached step (one zsg_ema_update over both
buffers), and the out-of-tree way, torch._foreach_lerp_ over clones of the ~170 strided parameter views.

    python tools/finetune_step.py --wgrad-bf16 [--out profiles/wgrad_bf16_step.json]

--wgrad-bf16 measures the convolution weight gradients on bf16 MFMA (ZSGNet.wgrad_precision("bf16"): zsg_conv_wgrad_bf16) against the
fp32 plan, everything trainable.  Each variant also reports its weight-gradient kernel class per kernel (zsg_prof_*: the library's
per-launch events over a few steps on one stream): wgrad_kernel / wino_wgrad_kernel / wgrad_bf16_kernel instantiations and
wgrad_reduce_kernel, with launches and ms per step, TFLOP/s and algorithmic bytes per launch.

    python tools/finetune_step.py --enc-bf16 [--train-bf16-head] [--wgrad-bf16] [--out profiles/enc_bf16_step.json]
    python tools/finetune_step.py --enc-bwd-bf16 [--enc-bf16] [--train-bf16-head] [--wgrad-bf16] [--out profiles/enc_bwd_bf16_step.json]

--enc-bwd-bf16 measures the encoder's data gradients on bf16 MFMA (ZSGNet.encoder_backward_precision("bf16"): zsg_conv_igemm_bf16_m /
zsg_conv_igemm_bf16_bnb) against the fp32 plan; with the other three flags three variants alternate: fp32, those switches, those switches +
the encoder's data gradients.  Each variant also reports its encoder data gradients launch by launch (serial replay) and the encoder's
BatchNorm-backward launches by entry.
--enc-bf16 measures the encoder's forward convolutions on bf16 MFMA (ZSGNet.encoder_precision("bf16_fwd"): zsg_conv_igemm_bf16_bn) against
the fp32 plan; with --train-bf16-head / --wgrad-bf16 four variants alternate: fp32, enc_bf16, those switches, those switches + enc_bf16.
Each variant also reports its encoder forward convolutions launch by launch (serial replay) and the "stats:" launches beside them.

    python tools/finetune_step.py --train-bf16-head [--wgrad-bf16] [--out profiles/train_bf16_head_step.json]

--train-bf16-head measures the forward convolutions and data gradients of the pyramid and the heads on bf16 MFMA
(ZSGNet.train_precision("bf16_head"): zsg_conv_igemm_bf16 / zsg_conv_igemm_bf16_m) against the fp32 plan, everything trainable; together
with --wgrad-bf16 four variants alternate: fp32, bf16_head, bf16_wgrad, both.  Each variant also reports, from per-launch events of its
four programs replayed on one stream (ops.Program.profile), the forward and data-gradient launches of those layers (the Winograd /
implicit-GEMM launches of the fp32 plan, the bf16 launches that replace them, the laterals' data gradients that stay fp32), the pack
launches and the Winograd filter transforms.

    python tools/finetune_step.py --lang-pool [--out profiles/lang_pool_step.json]

--lang-pool measures cfg lang_pool, everything trainable: last (the reference's vector), final, mean and attn alternate.  Each variant also
reports its query encoder launch by launch from per-launch events of the forward and backward programs replayed on one stream (every
launch alone on the GPU): the side-stream (lane 1) time the encoder's launches add up to, forward and backward.

    python tools/finetune_step.py --lang-fuse film [--out profiles/film_step.json]

--lang-fuse film measures cfg lang_fuse, everything trainable: concat (the reference's concatenation) and film alternate, film with drawn
film weights (gamma of a few tenths).  Each variant also reports the launches of head conv0's fusion point (the language / scale
launches, conv0's feature GEMM, the epilogue or film launch and their backward counterparts) from per-launch events of the forward and
backward programs replayed on one stream (every launch alone on the GPU).

    python tools/finetune_step.py --lang-fuse concat,film,words [--out profiles/words_step.json]

A comma-separated list names the modes to alternate (concat always runs).  words (word-level attention, drawn key / value weights) needs
the BiLSTM's per-token output and so runs with lang_pool = final, the full-sequence program whose vector is closest to the default's; its
difference to film therefore includes that encoder's (side-stream) cost.

    python tools/finetune_step.py --head-ctx none,gc [--out profiles/head_ctx_step.json]

cfg head_ctx: none and gc (the global-context block behind the heads' conv0, drawn weights with a non-zero last layer) alternate; each
variant also reports the block's launches (the gc forward and backward calls and the ReLU-mask commit of d(h1)) from the serial replay.

host_enqueue_ms_per_step: host time to enqueue a step (starting from an idle GPU; equal
to the GPU's ms_per_step when the host, not the GPU, sets the pace).  --only NAME[,NAME] runs the named variants alone (profiling).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zsgnet_pytorch_amd import config, dist as zdist, ema as zema, loss, mdl, ops, optim  # noqa: E402
from zsgnet_pytorch_amd.synth import synthetic_batch  # noqa: E402

ENC = "backbone.encoder."
VARIANTS = {
    "all_trainable": (),
    "stem_layer1_frozen": (ENC + "conv1.", ENC + "bn1.", ENC + "layer1."),
    "encoder_frozen": (ENC,),
    "encoder_lstm_frozen": (ENC, "lstm."),
}
# (frozen parameter prefixes, every BatchNorm layer in eval mode)
BN_VARIANTS = {
    "all_trainable": ((), False),
    "all_trainable_bn_frozen": ((), True),
    "encoder_frozen": ((ENC,), False),
    "encoder_frozen_bn_frozen": ((ENC,), True),
}
# (clip function, max_norm): 1e9 never engages, 1e-3 always does (the pre-clip 2-norm at configs[1] is far above it)
CLIP_VARIANTS = {
    "no_clip": None,
    "fused_clip_not_engaged": ("fused", 1e9),
    "fused_clip_engaged": ("fused", 1e-3),
    "torch_clip_engaged": ("torch", 1e-3),
}
# how the weight average is updated after every step
EMA_VARIANTS = {
    "no_ema": None,
    "ema_fused": "fused",
    "ema_separate": "separate",
    "torch_foreach_lerp": "foreach",
}
EMA_DECAY = 0.999
# (DistributedDataParallel with forced collectives, synchronized BatchNorm)
# cfg wgrad_dtype of the variant's network
WGRAD_VARIANTS = {
    "fp32": "fp32",
    "bf16_wgrad": "bf16",
}
# (cfg wgrad_dtype, cfg train_dtype) of the variant's network: --train-bf16-head alone runs the first two
TRAIN_VARIANTS = {
    "fp32": ("fp32", "fp32"),
    "bf16_head": ("fp32", "bf16_head"),
    "bf16_wgrad": ("bf16", "fp32"),
    "bf16_head_bf16_wgrad": ("bf16", "bf16_head"),
}
SYNC_VARIANTS = {
    "ddp_forced": False,
    "ddp_forced_sync_bn": True,
}


# cfg lang_pool of the variant's network
POOL_VARIANTS = ("last", "final", "mean", "attn")
# the query encoder's launches by their names in the plan (mdl._Plan._lower_lstm / _lower_lstm_seq)
POOL_WHATS = ("gather_last", "lstm", "lang_pool", "wgrad:w_ih", "wgrad:w_hh", "bgrad:lstm.", "wgrad:lang_pool")


def pool_class(v, nprof=3):
    """the query encoder's launches of one variant from per-launch events, as head_class takes them: the forward and backward programs
    replayed nprof times on one stream right after a step.  Per launch the name, the entry and the microseconds; the sums are the time
    the encoder occupies lane 1 (the side stream) in the forward and in the backward"""
    net = v["net"]
    plan = [p for k, p in net._plans.items() if k[-1]][0]
    st = torch.cuda.current_stream().cuda_stream
    acc = {}
    for _ in range(nprof):
        for tag, prog in (("fwd", plan.fwd), ("bwd", plan.bwd)):
            for i, (what, fname, ms) in enumerate(prog.profile(st)):
                acc[(tag, i, what, fname)] = acc.get((tag, i, what, fname), 0.0) + ms / nprof
    rows = [[tag, what, fname, round(ms * 1e3, 1)] for (tag, i, what, fname), ms in sorted(acc.items()) if what.startswith(POOL_WHATS)]
    tot = lambda t: round(sum(r[3] for r in rows if r[0] == t) / 1e3, 4)
    return dict(lang_pool=net.lang_pool_mode, encoder_fwd_ms=tot("fwd"), encoder_bwd_ms=tot("bwd"), encoder_launches=len(rows),
                fwd_program_ms=round(sum(ms for (tag, *_), ms in acc.items() if tag == "fwd"), 4),
                bwd_program_ms=round(sum(ms for (tag, *_), ms in acc.items() if tag == "bwd"), 4), encoder_rows=rows)


# cfg lang_fuse of the variant's network
FUSE_VARIANTS = ("concat", "film", "words")
# the launches of head conv0's fusion point by their names in the plan (mdl._Plan._head_stack)
FUSE_WHATS = ("att_reg_box0.", "att_reg_box.0.0", "lmap", "dgamma:", "dwe", "wgrad:att_reg_box.film", "bsum", "zero:head.Q", "wgrad:att_reg_box.words", "dhseq.",
              "transpose:att_reg_box")


def fuse_class(v, nprof=3):
    """the launches of head conv0's fusion point of one variant, taken as pool_class takes the query encoder's"""
    net = v["net"]
    plan = [p for k, p in net._plans.items() if k[-1]][0]
    st = torch.cuda.current_stream().cuda_stream
    acc = {}
    for _ in range(nprof):
        for tag, prog in (("fwd", plan.fwd), ("bwd", plan.bwd)):
            for i, (what, fname, ms) in enumerate(prog.profile(st)):
                acc[(tag, i, what, fname)] = acc.get((tag, i, what, fname), 0.0) + ms / nprof
    rows = [[tag, what, fname, round(ms * 1e3, 1)] for (tag, i, what, fname), ms in sorted(acc.items()) if any(k in what for k in FUSE_WHATS)]
    tot = lambda t: round(sum(r[3] for r in rows if r[0] == t) / 1e3, 4)
    return dict(lang_fuse=net.lang_fuse, fusion_fwd_ms=tot("fwd"), fusion_bwd_ms=tot("bwd"), fusion_launches=len(rows),
                fwd_program_ms=round(sum(ms for (tag, *_), ms in acc.items() if tag == "fwd"), 4),
                bwd_program_ms=round(sum(ms for (tag, *_), ms in acc.items() if tag == "bwd"), 4), fusion_rows=rows)


# cfg head_ctx of the variant's network
CTX_VARIANTS = ("none", "gc")
# the block's launches by their names in the plan (mdl._Plan._head_gc)
CTX_WHATS = (".gc", "mask+acc:att_reg_box.h1", "cast f32<-att_reg_box.h1", "cast bf16<-att_reg_box.h1g")


def ctx_class(v, nprof=3):
    """the launches of the heads' global-context block of one variant, taken as pool_class takes the query encoder's"""
    net = v["net"]
    plan = [p for k, p in net._plans.items() if k[-1]][0]
    st = torch.cuda.current_stream().cuda_stream
    acc = {}
    for _ in range(nprof):
        for tag, prog in (("fwd", plan.fwd), ("bwd", plan.bwd)):
            for i, (what, fname, ms) in enumerate(prog.profile(st)):
                acc[(tag, i, what, fname)] = acc.get((tag, i, what, fname), 0.0) + ms / nprof
    rows = [[tag, what, fname, round(ms * 1e3, 1)] for (tag, i, what, fname), ms in sorted(acc.items()) if any(k in what for k in CTX_WHATS)]
    tot = lambda t: round(sum(r[3] for r in rows if r[0] == t) / 1e3, 4)
    return dict(head_ctx=net.head_ctx, ctx_fwd_ms=tot("fwd"), ctx_bwd_ms=tot("bwd"), ctx_launches=len(rows),
                fwd_program_ms=round(sum(ms for (tag, *_), ms in acc.items() if tag == "fwd"), 4),
                bwd_program_ms=round(sum(ms for (tag, *_), ms in acc.items() if tag == "bwd"), 4), ctx_rows=rows)


WGRAD_KERNELS = ("wgrad_kernel", "wino_wgrad_kernel", "wgrad_bf16_kernel", "wgrad_reduce_kernel")


def wgrad_class(step_fn, nprof=4):
    """the weight-gradient kernel class of one variant, per kernel, taken with the library's own per-launch events (zsg_prof_*, as
    bench.py's roofline leg and tools/eval_speed.py --per-kernel do): nprof steps with every launch alone on the GPU (one stream), so a
    kernel's time is its own.  Rows are per kernel instantiation: launches and ms per step, TFLOP/s of the direct-form work, algorithmic
    bytes per launch and the rate they amount to; wgrad_reduce_kernel is listed on its own."""
    from zsgnet_pytorch_amd._lib import ProfEntry, lib
    keep = ops.SIDE_STREAM
    ops.SIDE_STREAM = False
    try:
        step_fn()
        torch.cuda.synchronize()
        lib.zsg_prof_enable(1)
        for _ in range(nprof):
            step_fn()
        torch.cuda.synchronize()
        lib.zsg_prof_enable(0)
    finally:
        ops.SIDE_STREAM = keep
    arr = (ProfEntry * 256)()
    n = lib.zsg_prof_collect(arr, 256)
    rows, total = [], 0.0
    for i in range(n):
        e = arr[i]
        name = e.name.decode()
        total += e.ms / nprof
        if name.split("<")[0] not in WGRAD_KERNELS:
            continue
        rows.append(dict(kernel=name, launches_per_step=e.launches / nprof, ms_per_step=round(e.ms / nprof, 4),
                         us_per_launch=round(1e3 * e.ms / e.launches, 2),
                         tflops=round(e.flops / (e.ms * 1e9), 1) if e.flops > 0 else None,
                         alg_mbytes_per_launch=round(e.bytes / e.launches / 2 ** 20, 2) if e.bytes > 0 else None,
                         alg_gbps=round(e.bytes / (e.ms * 1e6), 1) if e.bytes > 0 else None))
    rows.sort(key=lambda r: -r["ms_per_step"])
    return dict(wgrad_class_ms=round(sum(r["ms_per_step"] for r in rows), 4),
                wgrad_reduce_ms=round(sum(r["ms_per_step"] for r in rows if r["kernel"].startswith("wgrad_reduce")), 4),
                all_kernels_ms=round(total, 4), wgrad_kernels=rows)


def head_class(v, nprof=3):
    """the launches train_dtype = "bf16_head" replaces, of one variant, from per-launch events: the plan's four programs replayed nprof
    times on one stream (every launch alone on the GPU) right after a step, so every buffer holds that step's operands.  Per class the
    launch count and the ms per step; the rows name every launch."""
    net = v["net"]
    plan = [p for k, p in net._plans.items() if k[-1]][0]
    st = torch.cuda.current_stream().cuda_stream
    acc = {}
    for _ in range(nprof):
        for tag, prog in (("fwd-prep", plan.prep_u), ("fwd", plan.fwd), ("bwd-prep", plan.prep), ("bwd", plan.bwd)):
            for i, (what, fname, ms) in enumerate(prog.profile(st)):
                k = (tag, i, what, fname)
                acc[k] = acc.get(k, 0.0) + ms / nprof
    convs = ("zsg_conv_igemm", "zsg_conv_wino", "zsg_conv_igemm_bf16", "zsg_conv_igemm_bf16_m")
    cls = {}
    for (tag, i, what, fname), ms in acc.items():
        base = what[:-len("+bf16")] if what.endswith("+bf16") else what
        c = None
        if fname == "zsg_pack_w_bf16_batched":
            c = "pack_" + ("fwd" if tag == "fwd-prep" else "bwd")
        elif fname == "zsg_wino_weights":
            c = "wino_filter_transforms_" + ("fwd" if tag in ("fwd-prep", "fwd") else "bwd")
        elif tag == "fwd" and fname in convs and base.startswith(mdl.BF16_HEAD_PREFIXES):
            c = "head_fwd_" + ("bf16" if "bf16" in fname else ("wino" if "wino" in fname else "igemm"))
        elif tag == "bwd" and fname in convs and base.startswith("dgrad:") and base[6:].startswith(mdl.BF16_HEAD_PREFIXES):
            c = "head_dgrad_" + ("bf16" if "bf16" in fname else ("wino" if "wino" in fname else "igemm"))
        if c is not None:
            e = cls.setdefault(c, dict(launches=0, ms_per_step=0.0, rows=[]))
            e["launches"] += 1
            e["ms_per_step"] += ms
            e["rows"].append([what, fname, round(ms * 1e3, 1)])
    for e in cls.values():
        e["ms_per_step"] = round(e["ms_per_step"], 4)
    tot = lambda pre: round(sum(e["ms_per_step"] for c, e in cls.items() if c.startswith(pre)), 4)
    return dict(head_fwd_ms=tot("head_fwd_"), head_dgrad_ms=tot("head_dgrad_"), pack_ms=tot("pack_"), wino_filter_transforms_ms=tot("wino_filter"),
                fwd_program_ms=round(sum(ms for (tag, *_), ms in acc.items() if tag == "fwd"), 4),
                bwd_program_ms=round(sum(ms for (tag, *_), ms in acc.items() if tag == "bwd"), 4), head_classes=cls)


def enc_class(v, nprof=3):
    """the encoder's forward convolutions of one variant (what enc_dtype = "bf16_fwd" replaces), from per-launch events as head_class
    takes them: per launch the layer, the entry and the microseconds in serial replay; the "stats:" finalize launches of encoder
    BatchNorms are counted and timed beside them (a bf16 launch has no in-kernel finalize)"""
    net = v["net"]
    plan = [p for k, p in net._plans.items() if k[-1]][0]
    st = torch.cuda.current_stream().cuda_stream
    acc = {}
    for _ in range(nprof):
        for i, (what, fname, ms) in enumerate(plan.fwd.profile(st)):
            acc[(i, what, fname)] = acc.get((i, what, fname), 0.0) + ms / nprof
    rows, stats_n, stats_ms, apply_ms = [], 0, 0.0, 0.0
    for (i, what, fname), ms in sorted(acc.items()):
        if what.startswith(mdl.BF16_ENC_PREFIX) and fname.startswith("zsg_conv"):
            layer = what.split("+")[0]
            rows.append([layer, fname, what[len(layer):], round(ms * 1e3, 1)])
        elif what.startswith("stats:" + mdl.BF16_ENC_PREFIX):
            stats_n, stats_ms = stats_n + 1, stats_ms + ms
        elif what.startswith(mdl.BF16_ENC_PREFIX) and fname.startswith("zsg_bn_apply"):
            apply_ms += ms
    return dict(enc_fwd_conv_ms=round(sum(r[3] for r in rows) / 1e3, 4), enc_stats_launches=stats_n, enc_stats_ms=round(stats_ms, 4),
                enc_bn_apply_ms=round(apply_ms, 4), fwd_program_ms=round(sum(acc.values()), 4), enc_fwd_rows=rows)


def encb_class(v, nprof=3):
    """the encoder's data gradients of one variant (what enc_bwd_dtype = "bf16" replaces) and the BatchNorm backward launches behind
    them, from per-launch events of the backward program in serial replay: per launch the layer, the entry, its suffix and the
    microseconds; the encoder's "bnbwd" launches by entry (a bf16 data gradient has no in-kernel finalize: zsg_bn_bwd_apply becomes
    zsg_bn_backward_from_partials)"""
    net = v["net"]
    plan = [p for k, p in net._plans.items() if k[-1]][0]
    st = torch.cuda.current_stream().cuda_stream
    acc = {}
    for _ in range(nprof):
        for tag, prog in (("bwd-prep", plan.prep), ("bwd", plan.bwd)):
            for i, (what, fname, ms) in enumerate(prog.profile(st)):
                acc[(tag, i, what, fname)] = acc.get((tag, i, what, fname), 0.0) + ms / nprof
    rows, bnb, pack_ms = [], {}, 0.0
    for (tag, i, what, fname), ms in sorted(acc.items()):
        if tag == "bwd-prep":
            if fname == "zsg_pack_w_bf16_batched":
                pack_ms += ms
        elif what.startswith("dgrad:" + mdl.BF16_ENC_PREFIX):
            layer = what.split("+")[0]
            rows.append([layer[6:], fname, what[len(layer):], round(ms * 1e3, 1)])
        elif what.startswith(("bnbwd:" + mdl.BF16_ENC_PREFIX, "bnbwd(frozen):" + mdl.BF16_ENC_PREFIX)):
            e = bnb.setdefault(fname, dict(launches=0, ms_per_step=0.0))
            e["launches"] += 1
            e["ms_per_step"] = round(e["ms_per_step"] + ms, 4)
    return dict(enc_dgrad_ms=round(sum(r[3] for r in rows) / 1e3, 4), enc_dgrad_in_kernel_finalize=sum(r[2].endswith("+fin") for r in rows),
                enc_bnbwd=bnb, enc_bnbwd_ms=round(sum(e["ms_per_step"] for e in bnb.values()), 4), bwd_pack_ms=round(pack_ms, 4),
                bwd_program_ms=round(sum(ms for (tag, *_), ms in acc.items() if tag == "bwd"), 4), enc_dgrad_rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bs", type=int, default=16)
    ap.add_argument("--out", default="")
    ap.add_argument("--frozen-bn", action="store_true")
    ap.add_argument("--clip", action="store_true")
    ap.add_argument("--sync-bn", action="store_true")
    ap.add_argument("--ema", action="store_true")
    ap.add_argument("--wgrad-bf16", action="store_true")
    ap.add_argument("--train-bf16-head", action="store_true")
    ap.add_argument("--enc-bf16", action="store_true", help="fp32 against enc_dtype = bf16_fwd; with --train-bf16-head / --wgrad-bf16 "
                                                             "also those switches without and with the encoder's")
    ap.add_argument("--enc-bwd-bf16", action="store_true", help="fp32 against enc_bwd_dtype = bf16; with --enc-bf16 / --train-bf16-head / "
                                                                 "--wgrad-bf16 also those switches without and with the encoder's data gradients")
    ap.add_argument("--lang-pool", action="store_true", help="cfg lang_pool: last, final, mean and attn alternate")
    ap.add_argument("--lang-fuse", default="", help="cfg lang_fuse: concat and the named modes (film, words; comma-separated) alternate")
    ap.add_argument("--head-ctx", default="", help="cfg head_ctx: the named modes (none, gc; comma-separated) alternate")
    ap.add_argument("--only", default="", help="comma-separated variant names to run (e.g. one variant under rocprofv3)")
    a = ap.parse_args()
    modes = [f for f, on in (("--head-ctx", a.head_ctx), ("--lang-fuse", a.lang_fuse), ("--lang-pool", a.lang_pool), ("--enc-bwd-bf16", a.enc_bwd_bf16),
                             ("--enc-bf16", a.enc_bf16), ("--sync-bn", a.sync_bn), ("--train-bf16-head", a.train_bf16_head),
                             ("--wgrad-bf16", a.wgrad_bf16), ("--ema", a.ema), ("--clip", a.clip), ("--frozen-bn", a.frozen_bn)) if on]
    if a.head_ctx and len(modes) > 1:       # (the switches below it in the chain would be dropped without a word)
        ap.error(f"--head-ctx chooses the variants on its own: it does not combine with {', '.join(modes[1:])}")
    torch.cuda.set_device(0)
    if a.sync_bn:
        import socket
        import torch.distributed as dist
        sk = socket.socket()
        sk.bind(("127.0.0.1", 0))
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(sk.getsockname()[1]))
        sk.close()
        dist.init_process_group("nccl", rank=0, world_size=1)
    cfg = config.get_cfg()
    r, s = config.ratios_scales(cfg)
    lf = loss.get_default_loss(r, s, cfg)
    bt = {k: v.cuda() for k, v in synthetic_batch(a.bs, 300, 300, seed=1).items()}
    bt["h0"], bt["c0"] = torch.zeros(2, a.bs, 128), torch.zeros(2, a.bs, 128)
    sd = None
    runs = {}
    enc_of = {}                              # variant -> cfg enc_dtype (default fp32)
    encb_of = {}                             # variant -> cfg enc_bwd_dtype (default fp32)
    pool_of = {}                             # variant -> cfg lang_pool (default last)
    fuse_of = {}                             # variant -> cfg lang_fuse (default concat)
    ctx_of = {}                              # variant -> cfg head_ctx (default none)
    if a.head_ctx:
        asked = [m for m in a.head_ctx.split(",") if m]
        if not asked or [m for m in asked if m not in CTX_VARIANTS]:
            ap.error(f"--head-ctx: expected a comma-separated list of {', '.join(CTX_VARIANTS)}")
        variants = {k: ((), False, None, None, None, "fp32", "fp32") for k in CTX_VARIANTS if k in asked}
        ctx_of = {k: k for k in variants}
    elif a.lang_fuse:
        asked = [m for m in a.lang_fuse.split(",") if m]
        if [m for m in asked if m not in FUSE_VARIANTS]:
            ap.error(f"--lang-fuse: expected a comma-separated list of {', '.join(FUSE_VARIANTS)}")
        modes = [m for m in FUSE_VARIANTS if m == "concat" or m in asked]
        variants = {k: ((), False, None, None, None, "fp32", "fp32") for k in modes}
        fuse_of = {k: k for k in modes}
    elif a.lang_pool:
        variants = {k: ((), False, None, None, None, "fp32", "fp32") for k in POOL_VARIANTS}
        pool_of = {k: k for k in POOL_VARIANTS}
    elif a.enc_bwd_bf16:
        other = ("bf16" if a.wgrad_bf16 else "fp32", "bf16_head" if a.train_bf16_head else "fp32")
        oname = "+".join(n for n, on in (("enc_bf16", a.enc_bf16), ("bf16_head", a.train_bf16_head), ("bf16_wgrad", a.wgrad_bf16)) if on)
        variants = {"fp32": ((), False, None, None, None, "fp32", "fp32")}
        if oname:
            variants[oname] = ((), False, None, None, None) + other
            variants[oname + "+encb_bf16"] = ((), False, None, None, None) + other
            encb_of[oname + "+encb_bf16"] = "bf16"
            if a.enc_bf16:
                enc_of[oname] = enc_of[oname + "+encb_bf16"] = "bf16_fwd"
        else:
            variants["encb_bf16"] = ((), False, None, None, None, "fp32", "fp32")
            encb_of["encb_bf16"] = "bf16"
    elif a.enc_bf16:
        other = ("bf16" if a.wgrad_bf16 else "fp32", "bf16_head" if a.train_bf16_head else "fp32")
        oname = next(k for k, v in TRAIN_VARIANTS.items() if v == other)
        variants = {"fp32": ((), False, None, None, None, "fp32", "fp32"), "enc_bf16": ((), False, None, None, None, "fp32", "fp32")}
        enc_of["enc_bf16"] = "bf16_fwd"
        if oname != "fp32":
            variants[oname] = ((), False, None, None, None) + other
            variants["enc_bf16_" + oname] = ((), False, None, None, None) + other
            enc_of["enc_bf16_" + oname] = "bf16_fwd"
    elif a.sync_bn:
        variants = {k: ((), False, None, v, None, "fp32", "fp32") for k, v in SYNC_VARIANTS.items()}
    elif a.train_bf16_head:
        variants = {k: ((), False, None, None, None, v[0], v[1]) for k, v in TRAIN_VARIANTS.items() if a.wgrad_bf16 or v[0] == "fp32"}
    elif a.wgrad_bf16:
        variants = {k: ((), False, None, None, None, v, "fp32") for k, v in WGRAD_VARIANTS.items()}
    elif a.ema:
        variants = {k: ((), False, None, None, v, "fp32", "fp32") for k, v in EMA_VARIANTS.items()}
    elif a.clip:
        variants = {k: ((), False, c, None, None, "fp32", "fp32") for k, c in CLIP_VARIANTS.items()}
    elif a.frozen_bn:
        variants = {k: (v[0], v[1], None, None, None, "fp32", "fp32") for k, v in BN_VARIANTS.items()}
    else:
        variants = {k: (v, False, None, None, None, "fp32", "fp32") for k, v in VARIANTS.items()}
    if a.only:
        variants = {k: v for k, v in variants.items() if k in a.only.split(",")}
    for name, (prefixes, bn_frozen, clip, sync_bn, ema, wgrad_dtype, train_dtype) in variants.items():
        vcfg = config.get_cfg(head_ctx=ctx_of[name]) if name in ctx_of else config.get_cfg(lang_pool=pool_of[name]) if name in pool_of else (config.get_cfg(lang_fuse=fuse_of[name], **({"lang_pool": "final"} if fuse_of[name] == "words" else {})) if name in fuse_of else cfg)
        net = mdl.get_default_net(9, vcfg)
        net.wgrad_precision(wgrad_dtype).train_precision(train_dtype).encoder_precision(enc_of.get(name, "fp32"))
        net.encoder_backward_precision(encb_of.get(name, "fp32"))
        if sd is None:
            sd = {k: v.clone() for k, v in net.state_dict().items() if ".gc." not in k}
        if "lang_pool.weight" in net.state_dict():      # (attn: a drawn scorer beside the shared weights, so the attention is not uniform)
            g = torch.Generator().manual_seed(0)
            net.load_state_dict(dict(sd, **{"lang_pool.weight": torch.randn(1, net.lstm_out_dim, generator=g) * 0.25}))
        elif net.head_ctx == "gc":                      # (drawn gc tensors beside the shared weights: a non-zero last layer, so every launch works)
            g = torch.Generator().manual_seed(0)
            net.load_state_dict(dict(sd, **{k: torch.randn(v.shape, generator=g) * 0.05 + (1.0 if k.endswith("ln.weight") else 0.0)
                                            for k, v in net.state_dict().items() if ".gc." in k}))
        elif net.lang_fuse == "film":                   # (drawn film weights beside the shared weights, so the scale is not 1)
            g = torch.Generator().manual_seed(0)
            net.load_state_dict(dict(sd, **{"att_reg_box.film.weight": torch.randn(256, net.lstm_out_dim, generator=g) * 0.05}))
        elif net.lang_fuse == "words":                  # (drawn key / value weights: the attention is not uniform, the scale not 1)
            g = torch.Generator().manual_seed(0)
            net.load_state_dict(dict(sd, **{f"att_reg_box.words.{kv}.weight": torch.randn(256, net.lstm_out_dim, generator=g) * 0.05
                                            for kv in ("key", "value")}))
        else:
            net.load_state_dict(sd)
        net.to("cuda").train()
        for n, p in net.named_parameters():
            p.requires_grad_(not (prefixes and n.startswith(prefixes)))
        if bn_frozen:
            net.freeze_batchnorm()
        model = net
        if sync_bn is not None:              # (--sync-bn: the wrapper with forced collectives, converted or not)
            model = zdist.DistributedDataParallel(net, device_ids=[0], force_collectives=True)
            if sync_bn:
                zdist.convert_sync_batchnorm(model, force=True)
        runs[name] = dict(net=net, model=model, opt=optim.FusedAdam(net, lr=1e-4, betas=(0.9, 0.99)), ms=[], host_ms=[], clip=clip,
                          params=list(net.parameters()), ema=ema)
        if ema == "fused":
            runs[name]["avg"] = zema.ModelEma(net, decay=EMA_DECAY).attach(runs[name]["opt"])
        elif ema == "separate":
            runs[name]["avg"] = zema.ModelEma(net, decay=EMA_DECAY)
        elif ema == "foreach":
            runs[name]["src"] = [p.detach() for p in net.parameters()]
            runs[name]["shadow"] = [p.clone() for p in runs[name]["src"]]

    def step(v):
        v["opt"].zero_grad()
        v["out"] = v["model"](bt)            # (kept: the forward program's output slot points at it until the next forward)
        lf(v["out"], bt)["loss"].backward()
        if v["clip"] is not None:
            kind, max_norm = v["clip"]
            fn = optim.clip_grad_norm_ if kind == "fused" else torch.nn.utils.clip_grad_norm_
            v["norm"] = fn(v["params"], max_norm)
        v["opt"].step()
        if v["ema"] == "separate":
            v["avg"].update()
        elif v["ema"] == "foreach":
            torch._foreach_lerp_(v["shadow"], v["src"], 1.0 - EMA_DECAY)
    for v in runs.values():              # lowering (and any tuning) outside the timed rounds
        for _ in range(a.warmup):
            step(v)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, v in runs.items():
            for _ in range(a.warmup):
                step(v)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev[0].record()
            for i in range(a.steps):
                step(v)
                ev[i + 1].record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            v["ms"].append(statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(a.steps)))
            v["host_ms"].append((t1 - t0) * 1e3 / a.steps)
    res = dict(config="BASELINE configs[1] shape (ResNet-50 + FPN, 300x300, B=%d, 1 GPU)" % a.bs, rounds=a.rounds, steps=a.steps,
               tune_loaded=ops.TUNE_INFO.get("loaded", 0), stamp_match=ops.TUNE_INFO.get("table_stamp") == ops.TUNE_INFO.get("stamp"),
               variants={})
    for name, v in runs.items():
        net = v["net"]
        plan = [p for k, p in net._plans.items() if k[-1]][0]
        res["variants"][name] = dict(ms_per_step=round(statistics.median(v["ms"]), 4), round_medians=[round(x, 4) for x in v["ms"]],
                                     host_enqueue_ms_per_step=round(statistics.median(v["host_ms"]), 4),
                                     bwd_launches=len(plan.bwd.calls), prep_launches=len(plan.prep.calls),
                                     fwd_launches=len(plan.fwd.calls), fwd_prep_launches=len(plan.prep_u.calls),
                                     fwd_prep=[c[2] for c in plan.prep_u.calls],
                                     stepped_params=sum(p.numel() for p in net.parameters() if p.grad is not None),
                                     frozen_tensors=sum(1 for p in net.parameters() if not p.requires_grad),
                                     frozen_bn_layers=len(net._frozen_bn_key()),
                                     collectives_per_step=sum(c[0].__name__ == "host" for c in plan.fwd.calls + plan.bwd.calls),
                                     sync_bn_layers=len(plan.sync_bn))
        if v["clip"] is not None:
            res["variants"][name].update(clip=v["clip"][0], max_norm=v["clip"][1], last_grad_norm=round(float(v["norm"]), 6),
                                         engaged=float(v["norm"]) > v["clip"][1])
        if a.head_ctx:
            res["variants"][name].update(**ctx_class(v))
        elif a.lang_fuse:
            res["variants"][name].update(**fuse_class(v))
        elif a.lang_pool:
            res["variants"][name].update(**pool_class(v))
        elif a.enc_bwd_bf16:
            res["variants"][name].update(enc_bwd_dtype=net._enc_bwd_dtype, enc_dtype=net._enc_dtype, train_dtype=net._train_dtype,
                                         wgrad_dtype=net._wgrad_dtype, **encb_class(v))
        elif a.enc_bf16:
            res["variants"][name].update(enc_dtype=net._enc_dtype, train_dtype=net._train_dtype, wgrad_dtype=net._wgrad_dtype, **enc_class(v))
        elif a.train_bf16_head:
            res["variants"][name].update(train_dtype=net._train_dtype, wgrad_dtype=net._wgrad_dtype, **head_class(v))
        elif a.wgrad_bf16:
            res["variants"][name].update(wgrad_dtype=net._wgrad_dtype, **wgrad_class(lambda: step(v)))
        if v["ema"] is not None:
            res["variants"][name].update(ema=v["ema"], ema_decay=EMA_DECAY)
            if "avg" in v:
                res["variants"][name].update(ema_updates=v["avg"].n_averaged)
    js = json.dumps(res, indent=1)
    print(js)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(js + "\n")


if __name__ == "__main__":
    main()
