"""ZSGNet on MI355X: same module surface as the reference `code/mdl.py` (get_default_net / ZSGNet.forward), with
every device op a hand-written HIP kernel reached through the C ABI (include/zsg.h).

Reference behaviour mirrored here (file:line in /root/reference/code):
  * ZSGNet.forward mdl.py:338-403 — dict in (img [B,3,H,W], qvec [B,T,300], qlens [B]) -> dict out
    (att_out [B,A,1], bbx_out [B,A,4], feat_sizes [L,2] int64, num_f_out [1] int64).
  * RetinaBackBone.encode_feats mdl.py:148-159 (ResNet stem + layer1..4, Bottleneck fpn_resnet.py:61-100,
    BasicBlock :26-58) and FPN_backbone.forward fpn_resnet.py:154-178.
  * BackBone.concat_we mdl.py:69-104 (channel order [feat | language vector | grid y,x]).
    cfg lang_fuse = film (not in the reference) also scales conv0's feature part per query and channel by 1 + W_gamma . we
    (csrc/film.hip; definition in include/zsg.h, host twin tests/film_ref.py).
    cfg lang_fuse = words (not in the reference) makes that scale a function of the pixel: conv0's raw feature accumulator attends over
    the BiLSTM's per-token output (csrc/words.hip; definition in include/zsg.h, host twin tests/words_ref.py).
  * shared 6-conv head mdl.py:235-244 + permute_correctly :246-254 (free here: NHWC output == [B, h*w*9, 5]).
  * BiLSTM query encoder apply_lstm mdl.py:296-336, random initial state lstm_init_hidden :279-294.
    cfg lang_pool = final / mean / attn (not in the reference: its get_full_seq hook is unused) hands the head a vector of the whole
    phrase instead of the last token's output; definitions in include/zsg.h, host twin tests/langpool_ref.py.

Execution model: for a given input geometry the network is lowered ONCE into two static launch programs
(forward, backward) over preallocated NHWC buffers (`ops.Program`); a step replays them on torch's current stream.
The whole forward is a single autograd node, so the reference trainer's `loss.backward()` / `optimizer.step()`
keep working while no autograd graph is built per layer.
"""
import ctypes as _ct
import math
import os
import struct as _struct
import types
import weakref
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch
from torch import nn

from . import anchors as anchors_mod
from ._lib import check, lib, require_gpu, stream_ptr
from .ops import (Level, Program, TView, WinoJobs, apply_main_priority_env, autotune_conv, autotune_wgrad_batch, conv_out, ensure_stream_scratch, dgrad_desc, fwd_desc, igemm_partial_rows, marshal,
                  shared_side_stream, tile_hint, wino_mode, wino_ok)
from .params import ParamStore, pad4, register_named

VGG_BASE = [64, 64, "M", 128, 128, "M", 256, 256, 256, "C", 512, 512, 512, "M", 512, 512, 512]     # ssd_vgg.py:174-177
SSD_EXTRAS = [256, "S", 512, 128, "S", 256, 128, 256, 128, 256]                                          # ssd_vgg.py:179-182

WGRAD_DTYPES = ("fp32", "bf16")               # cfg wgrad_dtype / ZSGNet.wgrad_precision: operand precision of the training plans' convolution weight gradients
EVAL_TTAS = ("none", "flip")                   # cfg eval_tta / ZSGNet.eval_tta: test-time augmentation of the eval forwards
EVAL_DTYPES = ("fp32", "bf16", "bf16_act")    # cfg eval_dtype / ZSGNet.eval_precision: operand precision of the eval plans' convolutions (+ bf16 activation storage)
TRAIN_DTYPES = ("fp32", "bf16_head")         # cfg train_dtype / ZSGNet.train_precision: operand precision of the training plans' forward convolutions and data gradients ("bf16_head": the pyramid and the heads; "bf16" is left free for a whole-network version)
ENC_DTYPES = ("fp32", "bf16_fwd")             # cfg enc_dtype / ZSGNet.encoder_precision: operand precision of the training plans' forward convolutions of a ResNet encoder behind the stem (the backward stays what wgrad_dtype / fp32 make it)
ENC_BWD_DTYPES = ("fp32", "bf16")             # cfg enc_bwd_dtype / ZSGNet.encoder_backward_precision: operand precision of the training plans' data gradients of a ResNet encoder behind the stem (independent of enc_dtype, which keeps its two values)
BF16_ENC_PREFIX = "backbone.encoder."         # the layers enc_dtype = "bf16_fwd" covers (ResNet only; never the stem, never a convolution that applies a pending BatchNorm)
BF16_HEAD_PREFIXES = ("backbone.fpn.", "att_reg_box.", "att_box.", "reg_box.")     # the layers train_dtype = "bf16_head" covers: no BatchNorm among them
LSTM_DIMS = (32, 64, 128, 256)    # cfg lstm_dim: the widths csrc/lstm.hip instantiates zsg_lstm_fwd / zsg_lstm_bwd for
LANG_POOLS = ("last", "final", "mean", "attn")      # cfg lang_pool: the sentence vector the query encoder hands to the head (_lower_lstm)
LANG_FUSES = ("concat", "film", "words")                   # cfg lang_fuse: how that vector meets the image in the heads' conv0 (_head_stack)
HEAD_CTXS = ("none", "gc")                          # cfg head_ctx: a global-context block behind the heads' conv0 (_head_stack, csrc/gcblock.hip)
GC_STAT_LD = 388                                    # floats zsg_head_gc_fwd saves per (query, level): ZSG_GC_STAT_LD of include/zsg.h
GC_SUFFIXES = (".gc.key.weight", ".gc.fc1.weight", ".gc.fc1.bias", ".gc.ln.weight", ".gc.ln.bias", ".gc.fc2.weight", ".gc.fc2.bias")

LIVE_NETS = weakref.WeakSet()      # every ZSGNet alive: optim.clip_grad_norm_ finds a parameter's flat store here

ARCHS = {
    "resnet18": ("basic", (2, 2, 2, 2)),
    "resnet34": ("basic", (3, 4, 6, 3)),
    "resnet50": ("bottleneck", (3, 4, 6, 3)),
    "resnet101": ("bottleneck", (3, 4, 23, 3)),
}


@dataclass
class ConvL:
    name: str
    cin: int
    cout: int
    k: int
    stride: int = 1
    pad: int = 0
    dil: int = 1
    bias: bool = False
    merge_x: bool = False

    @property
    def cpad(self):
        return pad4(self.cin)


@dataclass
class BnL:
    name: str
    c: int
    index: int = 0      # slot in the flat running-stat buffers


BNB_FUSE = os.environ.get("ZSG_BNB_FUSE", "1") != "0"     # BatchNorm-backward sums in the epilogue of the data gradient that completes dout
# bn3 + residual + ReLU of a bottleneck applied by the NEXT block's conv1 (zsg_conv_igemm_bnpre) instead of a zsg_bn_apply launch, where the
# activation is at least this large (MB): the apply pass is HBM-bound there and the consumer would read its output again
BN_PRE_MIN_MB = 40
STAGE_INPUTS = True      # run_forward stages its inputs in one launch (tests/test_gpu_net.py compares it with the torch copies)
WG_BATCH = os.environ.get("ZSG_WG_BATCH", "1") != "0"      # identical-shape Winograd weight gradients of a stage in ONE launch (_Plan._batch_wgrads)


SHARED_PLANS_MAX = 12     # shared-image eval plans kept per network (least recently used goes first): two token buckets of a 32-query loader


EVAL_SCALES_MAX = 4       # cfg eval_scales / ZSGNet.eval_scales: extra eval passes per batch
EVAL_SCALE_RANGE = (0.5, 2.0)


def check_eval_scales(scales) -> Tuple[float, ...]:
    """cfg eval_scales as a tuple of floats; ValueError for anything but at most EVAL_SCALES_MAX finite numbers in EVAL_SCALE_RANGE"""
    if isinstance(scales, (str, bytes)) or not isinstance(scales, (list, tuple)):
        raise ValueError(f"eval_scales={scales!r}: expected a list of at most {EVAL_SCALES_MAX} numbers in [{EVAL_SCALE_RANGE[0]}, {EVAL_SCALE_RANGE[1]}]")
    if len(scales) > EVAL_SCALES_MAX:
        raise ValueError(f"eval_scales={list(scales)!r}: at most {EVAL_SCALES_MAX} entries")
    for s in scales:
        if isinstance(s, bool) or not isinstance(s, (int, float)) or not math.isfinite(s) or not EVAL_SCALE_RANGE[0] <= s <= EVAL_SCALE_RANGE[1]:
            raise ValueError(f"eval_scales={list(scales)!r}: entry {s!r} is not a finite number in [{EVAL_SCALE_RANGE[0]}, {EVAL_SCALE_RANGE[1]}]")
    return tuple(float(s) for s in scales)


def eval_scale_sizes(H: int, W: int, scales) -> List[Tuple[int, int]]:
    """The (height, width) of every extra pass of a multi-scale eval forward over an H x W batch: (round(s H), round(s W)) with halves
    rounded up.  ValueError when two entries give one size or an entry gives the batch's own size (pass 0 already runs it)."""
    sizes = [(int(math.floor(s * H + 0.5)), int(math.floor(s * W + 0.5))) for s in check_eval_scales(scales)]
    for i, (s, hw) in enumerate(zip(scales, sizes)):
        if hw == (H, W):
            raise ValueError(f"eval_scales={list(scales)!r}: entry {s!r} rounds to the batch's own size {H} x {W}")
        if hw in sizes[:i]:
            raise ValueError(f"eval_scales={list(scales)!r}: entries {scales[sizes.index(hw)]!r} and {s!r} both round to {hw[0]} x {hw[1]}")
    return sizes


def bucket_images(Bi: int, Q: int) -> int:
    """Image-batch bucket of the shared-image eval plan: the smallest power of two >= Bi, capped at Q.  A grouped loader yields another
    number of distinct images in almost every batch and each plan geometry costs a set of activation buffers and a tuner run, so for a
    given Q only {1, 2, 4, ..., Q} occur: at most ceil(log2 Q) + 1 values, each >= Bi."""
    if not 1 <= Bi <= Q:
        raise ValueError(f"shared images: {Bi} images for {Q} queries (need 1 <= images <= queries)")
    return min(Q, 1 << (Bi - 1).bit_length())


class Act(TView):
    """TView + autograd bookkeeping used while lowering (grad buffer, whether it already holds a partial sum, and
    whether the gradient stored there is w.r.t. the pre-ReLU value so producers must apply the ReLU mask)."""

    def __init__(self, buf, B, C, ld, levels, name=""):
        super().__init__(buf, B, C, ld, levels)
        self.name = name
        self.grad: Optional["Act"] = None
        self.gfilled = False
        self.needs_mask = False
        self.requires_grad = True

    @property
    def b16(self) -> bool:
        """stored as bf16 (a bf16_act eval plan); the layout is in ELEMENTS either way"""
        return self.buf.dtype == torch.bfloat16

    def lvl(self, i) -> "Act":
        a = Act(self.buf, self.B, self.C, self.ld, [self.levels[i]], f"{self.name}[{i}]")
        a.requires_grad = self.requires_grad
        return a


class ZSGNet(nn.Module):
    """The main model (reference mdl.py:171-403).  `backbone_kind` in {'retina', 'ssd_vgg'}."""

    def __init__(self, backbone_kind: str = "retina", n_anchors: int = 9, cfg: Any = None, arch: str = "resnet50"):
        super().__init__()
        self.cfg = cfg
        self.backbone_kind = backbone_kind
        self.arch = arch
        self.n_anchors = n_anchors
        self.emb_dim = int(cfg["emb_dim"])
        self.bid = bool(cfg["use_bidirectional"])
        self.lstm_dim = int(cfg["lstm_dim"])
        # (the reference takes any value; here the recurrence is compiled per width, csrc/lstm.hip, and the input projection is an
        # MFMA GEMM over 4-channel groups, zsg_conv_igemm: refuse before anything is allocated, not with -1 inside the first forward)
        if self.lstm_dim not in LSTM_DIMS:
            raise ValueError(f"lstm_dim={self.lstm_dim}: supported values are {', '.join(map(str, LSTM_DIMS))}")
        if self.emb_dim <= 0 or self.emb_dim % 4:
            raise ValueError(f"emb_dim={self.emb_dim}: supported values are the positive multiples of 4 "
                             "(zero-pad the word vectors, e.g. GloVe-50 to 52)")
        self.lstm_out_dim = self.lstm_dim * (self.bid + 1)
        # (fixed at construction: "attn" owns a parameter, lang_pool.weight, so the mode decides the state dict's keys)
        self.lang_pool_mode = str(cfg["lang_pool"]) if "lang_pool" in cfg else "last"
        if self.lang_pool_mode not in LANG_POOLS:
            raise ValueError(f"lang_pool={self.lang_pool_mode!r}: supported values are {', '.join(LANG_POOLS)}")
        if self.lang_pool_mode == "final" and not self.bid and not ("lang_fuse" in cfg and str(cfg["lang_fuse"]) == "words"):
            # one direction: h_n IS the forward state at len - 1, the same program (lang_fuse = "words" keeps the sequence program: it reads
            # the per-token output, which only that program writes; the vector is the same)
            self.lang_pool_mode = "last"
        self.use_lang = bool(cfg["use_lang"])
        self.use_img = bool(cfg["use_img"])
        self.same_atb = bool(cfg["use_same_atb"])
        if backbone_kind not in ("retina", "ssd_vgg"):
            raise ValueError(f"mdl_to_use={backbone_kind!r}: expected 'retina' or 'ssd_vgg' (mdl.py:410-414)")
        # (fixed at construction: "film" owns a parameter per head stack, <head>.film.weight, so the mode decides the state dict's keys)
        self.lang_fuse = str(cfg["lang_fuse"]) if "lang_fuse" in cfg else "concat"
        if self.lang_fuse not in LANG_FUSES:
            raise ValueError(f"lang_fuse={self.lang_fuse!r}: supported values are {', '.join(LANG_FUSES)}")
        if self.lang_fuse == "film" and not (self.use_lang and self.use_img):
            raise ValueError("lang_fuse='film' scales the image features by a function of the phrase: it needs use_lang=True and use_img=True")
        if self.lang_fuse == "words":
            if not (self.use_lang and self.use_img):
                raise ValueError("lang_fuse='words' lets every pixel attend over the phrase's words: it needs use_lang=True and use_img=True")
            if self.lang_pool_mode == "last":
                raise ValueError("lang_fuse='words' reads the BiLSTM's per-token output, which lang_pool='last' never forms (its reverse cell sees "
                                 "one token): set lang_pool to 'final', 'mean' or 'attn'")
        # (fixed at construction: "gc" owns seven parameters per head stack, so the mode decides the state dict's keys)
        self.head_ctx = str(cfg["head_ctx"]) if "head_ctx" in cfg else "none"
        if self.head_ctx not in HEAD_CTXS:
            raise ValueError(f"head_ctx={self.head_ctx!r}: supported values are {', '.join(HEAD_CTXS)}")
        self.do_norm = bool(cfg["do_norm"])
        # fpn_resnet.py:173 tests resize_img == [600,600]; ssd_vgg.py:98 tests resize_img[0] >= 600
        self.six_hundred = (list(cfg["resize_img"]) == [600, 600]) if backbone_kind == "retina" else (cfg["resize_img"][0] >= 600)
        self.cf = 256 if self.use_img else 0
        self.cw = self.lstm_out_dim if self.use_lang else 0
        self.use_grid = (self.use_img and self.use_lang) or (not self.use_img and not self.use_lang)
        self.start_dim_head = self.cf + self.cw + (2 if self.use_grid else 0)       # mdl.py:196-209
        self.lstm_state = "randn"          # 'randn' (reference) | 'zeros'

        self.store = ParamStore()
        self.convs: Dict[str, ConvL] = {}
        self.bns: Dict[str, BnL] = {}
        self._declare()
        self.store.allocate(torch.device("cpu"))
        nb = sum(b.c for b in self.bns.values())
        self._rmv = torch.cat([torch.zeros(nb), torch.ones(nb)])      # running means | running variances: ONE buffer, so the
        self._rm, self._rv = self._rmv[:nb], self._rmv[nb:]            # per-forward DDP buffer sync (C2) is one broadcast
        self._nbt = torch.zeros(len(self.bns), dtype=torch.long)
        self._register()
        self.reset_parameters()
        self._plans: Dict[Tuple, "_Plan"] = {}
        self._anchor = None
        self._bn_eval = set()          # BatchNorm layers freeze_batchnorm() keeps in eval mode across train()
        self._sync_bn_group = None     # process group of the synchronized BatchNorm collectives (sync_batchnorm), None: per-rank statistics
        self._sync_bn_conf = None      # (process group it was made for, force) of that group
        self.debug = False
        self._eval_dtype = "fp32"      # operand precision of the eval plans' convolutions (eval_precision)
        self._eval_tta = "none"        # test-time augmentation of the eval forwards (eval_tta)
        self._eval_scales = ()         # extra scales of the eval forwards (eval_scales)
        self._ms_resize = {}           # (B, H, W, Hs, Ws) -> (GpuResizer of Hs x Ws, its uint8 output batch): the resampler of one extra pass
        self._wgrad_dtype = "fp32"     # operand precision of the training plans' convolution weight gradients (wgrad_precision)
        self._train_dtype = "fp32"     # operand precision of the training plans' forward convolutions / data gradients (train_precision)
        self._enc_dtype = "fp32"       # operand precision of the training plans' encoder forward convolutions (encoder_precision)
        self._enc_bwd_dtype = "fp32"   # operand precision of the training plans' encoder data gradients (encoder_backward_precision)
        LIVE_NETS.add(self)

    # ------------------------------------------------------------------------------------------------------
    # declaration (names == reference state_dict keys)
    # ------------------------------------------------------------------------------------------------------
    def _conv(self, name, cin, cout, k, stride=1, pad=0, dil=1, bias=False, merge_x=False) -> ConvL:
        L = ConvL(name, cin, cout, k, stride, pad, dil, bias, merge_x)
        self.convs[name] = L
        self.store.add_conv(name + ".weight", cout, cin, k)
        if bias:
            self.store.add_vec(name + ".bias", cout)
        return L

    def _bn(self, name, c) -> BnL:
        off = sum(b.c for b in self.bns.values())
        L = BnL(name, c, off)
        self.bns[name] = L
        self.store.add_vec(name + ".weight", c)
        self.store.add_vec(name + ".bias", c)
        return L

    def _declare(self):
        if self.backbone_kind == "ssd_vgg":
            self._declare_ssd()
        else:
            self._declare_resnet_fpn()
        self._declare_head_lstm()

    def _declare_ssd(self):
        """SSD300-VGG16 trunk (ssd_vgg.py:117-171): registration order vgg, fproj1-3, extras, loc, conf.  The loc/conf
        multibox heads are created but never used by SSD.forward; they are kept so reference checkpoints load."""
        e = "backbone.encoder."
        self.block_kind, self.nblocks, self.blocks = "vgg", (), []
        self.vgg_layers = []
        cin, idx = 3, 0
        for v in VGG_BASE:
            if v in ("M", "C"):
                self.vgg_layers.append(("pool", idx, 2, 2, 0, v == "C"))
                idx += 1
            else:
                self._conv(f"{e}vgg.{idx}", cin, v, 3, 1, 1, bias=True, merge_x=(cin == 3))
                self.vgg_layers.append(("conv", idx))
                idx += 2
                cin = v
        self.vgg_layers.append(("pool", idx, 3, 1, 1, False))
        idx += 1
        self._conv(f"{e}vgg.{idx}", 512, 1024, 3, 1, 6, 6, bias=True)
        self.vgg_layers.append(("conv", idx))
        idx += 2
        self._conv(f"{e}vgg.{idx}", 1024, 1024, 1, 1, 0, bias=True)
        self.vgg_layers.append(("conv", idx))
        self._conv(e + "fproj1", 512, 256, 1, bias=True)
        self._conv(e + "fproj2", 1024, 256, 1, bias=True)
        self._conv(e + "fproj3", 512, 256, 1, bias=True)
        cin, flag, k = 1024, False, 0
        for i, v in enumerate(SSD_EXTRAS):
            if cin != "S":
                if v == "S":
                    self._conv(f"{e}extras.{k}", cin, SSD_EXTRAS[i + 1], (1, 3)[flag], 2, 1, bias=True)
                else:
                    self._conv(f"{e}extras.{k}", cin, v, (1, 3)[flag], 1, 0, bias=True)
                k += 1
                flag = not flag
            cin = v
        self.n_extras = k
        for nm, mult in (("loc", 4), ("conf", 21)):
            for i, (c, nb) in enumerate(zip((512, 1024, 512, 256, 256, 256), (4, 6, 6, 6, 4, 4))):
                self._conv(f"{e}{nm}.{i}", c, nb * mult, 3, 1, 1, bias=True)

    def _declare_resnet_fpn(self):
        kind, nblocks = ARCHS[self.arch]
        self.block_kind, self.nblocks = kind, nblocks
        exp = 4 if kind == "bottleneck" else 1
        e = "backbone.encoder."
        self._conv(e + "conv1", 3, 64, 7, 2, 3, merge_x=True)
        self._bn(e + "bn1", 64)
        inpl = 64
        self.blocks = []
        for li, (planes, nb) in enumerate(zip((64, 128, 256, 512), nblocks), start=1):
            for bi in range(nb):
                stride = 2 if (bi == 0 and li > 1) else 1
                q = f"{e}layer{li}.{bi}."
                blk = dict(prefix=q, stride=stride, layer=li, last=(bi == nb - 1), ds=False)
                if kind == "bottleneck":       # stride on the 3x3 (torchvision v1.5 == fpn_resnet.py:73-74)
                    self._conv(q + "conv1", inpl, planes, 1)
                    self._bn(q + "bn1", planes)
                    self._conv(q + "conv2", planes, planes, 3, stride, 1)
                    self._bn(q + "bn2", planes)
                    self._conv(q + "conv3", planes, planes * 4, 1)
                    self._bn(q + "bn3", planes * 4)
                else:
                    self._conv(q + "conv1", inpl, planes, 3, stride, 1)
                    self._bn(q + "bn1", planes)
                    self._conv(q + "conv2", planes, planes, 3, 1, 1)
                    self._bn(q + "bn2", planes)
                if bi == 0 and (stride != 1 or inpl != planes * exp):
                    self._conv(q + "downsample.0", inpl, planes * exp, 1, stride, 0)
                    self._bn(q + "downsample.1", planes * exp)
                    blk["ds"] = True
                inpl = planes * exp
                self.blocks.append(blk)
        c3, c4, c5 = 128 * exp, 256 * exp, 512 * exp
        f = "backbone.fpn."          # registration order of FPN_backbone.__init__, fpn_resnet.py:123-152
        self._conv(f + "P7_2", 256, 256, 3, 2, 1, bias=True)
        self._conv(f + "P6", c5, 256, 3, 2, 1, bias=True)
        self._conv(f + "P5_1", c5, 256, 1, 1, 0, bias=True)
        self._conv(f + "P5_2", 256, 256, 3, 1, 1, bias=True)
        self._conv(f + "P4_1", c4, 256, 1, 1, 0, bias=True)
        self._conv(f + "P4_2", 256, 256, 3, 1, 1, bias=True)
        self._conv(f + "P3_1", c3, 256, 1, 1, 0, bias=True)
        self._conv(f + "P3_2", 256, 256, 3, 1, 1, bias=True)

    def _declare_head_lstm(self):
        # shared head (the paper's configuration) or separate attention / box heads (mdl.py:211-225)
        heads = [("att_reg_box", 5)] if self.same_atb else [("att_box", 1), ("reg_box", 4)]
        for prefix, ncls in heads:
            self._conv(prefix + ".0.0", self.start_dim_head, 256, 3, 1, 1, bias=True)
            for i in range(1, 5):
                self._conv(f"{prefix}.{i}.0", 256, 256, 3, 1, 1, bias=True)
            self._conv(prefix + ".5", 256, ncls * self.n_anchors, 3, 1, 1, bias=True)
        H4 = 4 * self.lstm_dim
        for suf in ([""] + (["_reverse"] if self.bid else [])):       # nn.LSTM parameter order
            self.store.add_mat("lstm.weight_ih_l0" + suf, H4, self.emb_dim)
            self.store.add_mat("lstm.weight_hh_l0" + suf, H4, self.lstm_dim)
            self.store.add_vec("lstm.bias_ih_l0" + suf, H4)
            self.store.add_vec("lstm.bias_hh_l0" + suf, H4)
        if self.lang_pool_mode == "attn":       # the attention scorer s_t = w . o_t (no bias: softmax is shift-invariant); last in the flat buffer
            self.store.add_mat("lang_pool.weight", 1, self.lstm_out_dim)
        if self.lang_fuse == "film":            # gamma = W_gamma . we per head stack; behind every other entry: no existing offset moves
            for prefix, _ in heads:
                self.store.add_mat(prefix + ".film.weight", 256, self.lstm_out_dim)
        if self.lang_fuse == "words":           # Kw = W_key . o_t, Vw = W_value . o_t per head stack; behind every other entry, key then value
            for prefix, _ in heads:
                self.store.add_mat(prefix + ".words.key.weight", 256, self.lstm_out_dim)
                self.store.add_mat(prefix + ".words.value.weight", 256, self.lstm_out_dim)
        if self.head_ctx == "gc":               # the global-context block behind conv0 (N = 256, M = 64); behind every other entry
            for prefix, _ in heads:
                self.store.add_mat(prefix + ".gc.key.weight", 1, 256)
                self.store.add_mat(prefix + ".gc.fc1.weight", 64, 256)
                self.store.add_vec(prefix + ".gc.fc1.bias", 64)
                self.store.add_vec(prefix + ".gc.ln.weight", 64)
                self.store.add_vec(prefix + ".gc.ln.bias", 64)
                self.store.add_mat(prefix + ".gc.fc2.weight", 256, 64)
                self.store.add_vec(prefix + ".gc.fc2.bias", 256)

    def _register(self):
        self._param_names = list(self.store.order)
        for name in self._param_names:
            register_named(self, name, self.store.view(name))
        for i, (name, L) in enumerate(self.bns.items()):
            register_named(self, name + ".running_mean", self._rm[L.index:L.index + L.c], buffer=True)
            register_named(self, name + ".running_var", self._rv[L.index:L.index + L.c], buffer=True)
            register_named(self, name + ".num_batches_tracked", self._nbt[i], buffer=True)

    def _rebind(self):
        """Re-point every Parameter / buffer at the (possibly moved) flat storages."""
        mods = dict(self.named_modules())
        for name in self._param_names:
            path, leaf = name.rsplit(".", 1)
            p = mods[path]._parameters[leaf]
            p.data = self.store.view(name)
            p.grad = None
        for i, (name, L) in enumerate(self.bns.items()):
            m = mods[name]
            m._buffers["running_mean"] = self._rm[L.index:L.index + L.c]
            m._buffers["running_var"] = self._rv[L.index:L.index + L.c]
            m._buffers["num_batches_tracked"] = self._nbt[i]
        self._plans = {}

    def _apply(self, fn, recurse=True):
        flat = fn(self.store.flat)
        if flat.dtype != torch.float32:
            raise TypeError("zsgnet-pytorch_amd keeps its parameters and activations in fp32; dtype conversion is not supported "
                            "(reduced-precision inference: ZSGNet.eval_precision('bf16') / cfg eval_dtype)")
        self.store.flat = flat
        self.store.grad = torch.zeros_like(flat)
        self._rmv = fn(self._rmv)
        nb = self._rmv.numel() // 2
        self._rm, self._rv = self._rmv[:nb], self._rmv[nb:]
        self._nbt = self._nbt.to(flat.device)
        self._rebind()
        return self

    @property
    def device(self):
        return self.store.flat.device

    @torch.no_grad()
    def reset_parameters(self, seed: Optional[int] = None):
        """Random init (no network access for torchvision's ImageNet weights, mdl.py:411): He-normal encoder convs
        (fpn_resnet.py:266-272), PyTorch-default FPN/head convs, U(+-1/sqrt(H)) LSTM, head bias [0,0,0,0,-4]*A
        (mdl.py:214-219)."""
        g = torch.Generator().manual_seed(seed) if seed is not None else None
        for name in self._param_names:
            p = self.store.view(name)
            e = self.store.entries[name]
            if e.kind == "conv":
                co, ci, k, _ = e.shape
                if name.startswith("backbone.encoder."):
                    p.copy_(torch.randn(e.shape, generator=g) * math.sqrt(2.0 / (k * k * co)))
                else:
                    bound = 1.0 / math.sqrt(ci * k * k)
                    p.copy_((torch.rand(e.shape, generator=g) * 2 - 1) * bound)
            elif name.startswith("lstm."):
                bound = 1.0 / math.sqrt(self.lstm_dim)
                p.copy_((torch.rand(e.shape, generator=g) * 2 - 1) * bound)
            elif name == "lang_pool.weight":     # uniform attention: a fresh "attn" net computes "mean"
                p.zero_()
            elif name.endswith(".film.weight"):  # gamma = 0: a fresh "film" net computes "concat"
                p.zero_()
            elif name.endswith(".words.value.weight"):       # gamma = 0 whatever the attention: a fresh "words" net computes "concat"
                p.zero_()
            elif name.endswith(".words.key.weight"):         # (declared last: no existing net's draws change)
                bound = 1.0 / math.sqrt(self.lstm_out_dim)
                p.copy_((torch.rand(e.shape, generator=g) * 2 - 1) * bound)
            elif name.endswith((".gc.key.weight", ".gc.fc1.weight", ".gc.fc1.bias")):      # U(+-1/sqrt(N)) (declared last: no existing net's draws change)
                p.copy_((torch.rand(e.shape, generator=g) * 2 - 1) * (1.0 / math.sqrt(256.0)))
            elif name.endswith((".gc.fc2.weight", ".gc.fc2.bias", ".gc.ln.bias")):        # t = 0: a fresh "gc" net computes "none"
                p.zero_()
            elif name.endswith(".gc.ln.weight"):
                p.fill_(1.0)
            elif name.endswith(".bias") and name[:-5] in self.convs:
                L = self.convs[name[:-5]]
                bound = 1.0 / math.sqrt(L.cin * L.k * L.k)
                p.copy_((torch.rand(e.shape, generator=g) * 2 - 1) * bound)
            elif name.endswith(".weight"):       # BN gamma
                p.fill_(1.0)
            else:                                # BN beta
                p.zero_()
        if self.same_atb:                        # final biases, mdl.py:214-225
            hb = torch.zeros(5 * self.n_anchors)
            hb[4::5] = -4.0
            self.store.view("att_reg_box.5.bias").copy_(hb)
        else:
            self.store.view("att_box.5.bias").fill_(-4.0)
            self.store.view("reg_box.5.bias").zero_()

    def join_weight_readers(self):
        """Called before anything WRITES the flat weight buffer on the current stream (optimizer step, load_state_dict):
        a training forward that was never back-propagated (metrics-only forward, discarded loss) leaves its backward weight
        preparation running on the side stream, reading the weights — make the current stream wait for it."""
        for plan in self._plans.values():
            if plan._prep_pending:
                torch.cuda.current_stream().wait_event(plan._prep_ev)
                plan._prep_pending = False

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """Accepts reference checkpoints: strips DDP's 'module.' prefix (utils.py:489) and tolerates torchvision's
        unused `backbone.encoder.fc.*`."""
        if self.device.type == "cuda":
            self.join_weight_readers()
        sd = {}
        for k, v in state_dict.items():
            k = k[7:] if k.startswith("module.") else k
            if k.startswith("backbone.encoder.fc.") or k.startswith("backbone.encoder.fpn."):
                continue
            sd[k] = v
        return super().load_state_dict(sd, strict=strict, **kw)

    # ------------------------------------------------------------------------------------------------------
    # forward / backward
    # ------------------------------------------------------------------------------------------------------
    def refine_tuning(self, inp: Dict[str, Any], steps: int = 9, log=None) -> dict:
        """In-step refinement of the autotuner's near-ties for the training plan of `inp`'s geometry (ops.refine_in_step): alternatives
        the tuner timed within a few percent of its winner ALONE on the GPU are tried in the real step — forward + backward of the
        lowered plan on both streams, a fixed incoming gradient, no optimizer — and kept when the step gets faster.  Only shapes this
        process tuned itself have alternatives (a stamp-matched shipped table has none: nothing happens).  Not under DDP (rank 0's
        choices are broadcast before any rank lowers, dist._sync_tuning).  Returns ops.TUNE_INFO['refined']."""
        from . import ops as _ops
        assert self.training, "refine_tuning measures the training step"
        out = self(inp)                                   # lowers (and tunes) the plan if it is new
        plan = self._plan_for(*self.plan_geometry(inp))
        g = torch.randn(out["att_bbx_out"].shape, device=out["att_bbx_out"].device) * 1e-3
        out["att_bbx_out"].backward(g)

        def measure():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
            o = self(inp)
            o["att_bbx_out"].backward(g)
            ev[0].record()
            for i in range(steps):
                o = self(inp)
                o["att_bbx_out"].backward(g)
                ev[i + 1].record()
            torch.cuda.synchronize()
            t = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(steps))
            return t[len(t) // 2]
        res = _ops.refine_in_step(plan._tunables, measure, log=log)
        for p in self.parameters():
            p.grad = None
        return res

    def lstm_init_hidden(self, bs: int):
        """Reference mdl.py:279-294: two CPU draws (hidden_a then hidden_b) per forward, train and eval."""
        n = 2 if self.bid else 1
        if self.lstm_state == "zeros":
            return torch.zeros(n, bs, self.lstm_dim), torch.zeros(n, bs, self.lstm_dim)
        return torch.randn(n, bs, self.lstm_dim), torch.randn(n, bs, self.lstm_dim)

    def _ordered_params(self) -> List[nn.Parameter]:
        """Parameters in flat-storage order (== the order run_backward returns gradients in)."""
        if getattr(self, "_plist", None) is None:
            mods = dict(self.named_modules())
            self._plist = [mods[n.rsplit(".", 1)[0]]._parameters[n.rsplit(".", 1)[1]] for n in self._param_names]
        return self._plist

    def _param_index(self) -> Dict[int, int]:
        """id(parameter) -> its index in _ordered_params() (flat-storage order)"""
        if getattr(self, "_pindex", None) is None:
            self._pindex = {id(p): i for i, p in enumerate(self._ordered_params())}
        return self._pindex

    def plan_geometry(self, inp: Dict[str, Any]) -> Tuple[int, int, int, int]:
        """(B, H, W, T_plan) of the launch plan forward(inp) will use (T is bucketed: see forward).  An eval forward with
        eval_tta("flip") uses the plan of twice the rows (image slots and queries): the mirrored pass rides in the same forward."""
        img = inp["img"]
        if img.dtype == torch.uint8:
            B, H, W, _ = img.shape
        else:
            B, _, H, W = img.shape
        T = inp["qvec"].shape[1]
        Tp = 20 if T <= 20 else (50 if T <= 50 else T)
        m = 2 if self._tta_on() else 1          # (flip TTA: the mirrors behind the batch's own images, the mirrored queries behind its queries)
        if inp.get("img_idx") is not None:
            # queries sharing images: (Bi_plan, Q, H, W, T_plan), the image count bucketed as T is (bucket_images); the blind variants
            # gather the images into the plain plan of Q pairs.  A shared TRAINING plan has exactly the batch's image slots (train-mode
            # BatchNorm reduces across slots: no padding)
            Q = m * inp["qvec"].shape[0]
            if not (self.use_img and self.use_lang):
                return Q, H, W, Tp
            return (B if self.training else bucket_images(m * B, Q), Q, H, W, Tp)
        return m * B, H, W, Tp

    def _frozen_key(self) -> Tuple[int, ...]:
        """flat-order indices of the parameters with requires_grad=False (the training plans are lowered for one trainable set)"""
        return tuple(i for i, p in enumerate(self._ordered_params()) if not p.requires_grad)

    def batchnorm_modules(self):
        """(name, module) of every BatchNorm layer, in running-statistics order.  The layers are plain NamedTree nodes that carry the
        reference's names and parameters (isinstance(m, nn.BatchNorm2d) does not find them); their `.training` flag decides, inside a
        training network, whether the layer normalises with batch statistics or is frozen (see _frozen_bn_key)."""
        if getattr(self, "_bn_mods", None) is None:
            mods = dict(self.named_modules())
            self._bn_mods = [(name, mods[name]) for name in self.bns]
        return iter(self._bn_mods)

    def freeze_batchnorm(self, prefixes=("",), freeze: bool = True) -> List[str]:
        """Puts the BatchNorm layers whose names start with one of `prefixes` in eval mode (freeze=True) and remembers them, so that
        train() keeps them there (mmdet's norm_eval); freeze=False returns them to the root's mode and forgets them.  A frozen layer of a
        training network normalises with its running statistics, leaves them and num_batches_tracked unchanged and back-propagates
        F.batch_norm(training=False)'s gradient.  Returns the names that matched."""
        if isinstance(prefixes, str):
            prefixes = (prefixes,)
        names = []
        for name, m in self.batchnorm_modules():
            if any(name.startswith(p) for p in prefixes):
                names.append(name)
                if freeze:
                    self._bn_eval.add(name)
                    m.train(False)
                else:
                    self._bn_eval.discard(name)
                    m.train(self.training)
        return names

    def train(self, mode: bool = True):
        super().train(mode)
        if mode and self._bn_eval:
            for name, m in self.batchnorm_modules():
                if name in self._bn_eval:
                    m.train(False)
        return self

    def _frozen_bn_key(self) -> Tuple[int, ...]:
        """running-statistics order indices of the BatchNorm layers in eval mode (frozen inside a training network)"""
        return tuple(i for i, (_, m) in enumerate(self.batchnorm_modules()) if not m.training)

    def sync_batchnorm(self, process_group=None, enable: bool = True, force: bool = False) -> "ZSGNet":
        """torch.nn.SyncBatchNorm for this network's BatchNorm layers (they are NamedTree nodes: torch's convert_sync_batchnorm finds none).
        enable=True: every train-mode layer of a training forward normalises with the mean / variance of the union of the batches of
        `process_group`'s ranks (default: the whole world) and back-propagates through them; its d(gamma) / d(beta) stay the rank's own
        sums, which the gradient reducer averages.  Eval-mode layers (freeze_batchnorm) and eval forwards are not synced.  A collective call:
        every rank of the default group makes it with the SAME process_group (dist.new_group over its ranks, which new_group requires of
        every rank: the BatchNorm collectives get a group of their own, never the gradient reducer's).  Per-node subgroups — each rank
        passing its own subgroup, as torch.nn.SyncBatchNorm allows — are not supported: a rank outside process_group raises.  A group of
        one rank syncs only with force=True; without an initialised process group the network keeps per-rank statistics (torch's
        SyncBatchNorm falls back to batch_norm there).  enable=False returns to per-rank statistics."""
        import torch.distributed as dist
        group = None
        if enable and dist.is_available() and dist.is_initialized():
            pg = process_group if process_group is not None else dist.group.WORLD
            if pg is not dist.group.WORLD and dist.get_rank(pg) < 0:
                raise ValueError("sync_batchnorm: this rank is not in process_group (every rank must pass the same group that contains it)")
            ranks = dist.get_process_group_ranks(pg)
            if len(ranks) > 1 or force:
                if self._sync_bn_group is not None and self._sync_bn_conf == (pg, force):
                    group = self._sync_bn_group
                else:
                    group = dist.new_group(ranks=ranks)
        elif enable and force:
            raise RuntimeError("sync_batchnorm(force=True) needs an initialised torch.distributed process group")
        self._sync_bn_group = group
        self._sync_bn_conf = (process_group if process_group is not None else dist.group.WORLD, force) if group is not None else None
        return self

    def _sync_bn_key(self) -> Tuple[int, ...]:
        """running-statistics order indices of the BatchNorm layers a training forward synchronizes across ranks (sync_batchnorm)"""
        if self._sync_bn_group is None:
            return ()
        return tuple(i for i, (_, m) in enumerate(self.batchnorm_modules()) if m.training)

    def shared_training(self, enable: bool = True) -> "ZSGNet":
        """Opt-in: a TRAIN-mode batch with `img_idx` (Q queries over Bi distinct images) runs the image trunk and head conv0's feature GEMM
        once per image, forward and backward, instead of raising "eval-only".  The result is the gradient of
        sum_q loss(net(img[img_idx[q]], query q)) with the trunk evaluated once per distinct image; train-mode BatchNorm statistics are
        taken over the Bi distinct images, each counted once — equal to plain training on the expanded batch img[img_idx] when every image
        has the same number of queries (or BatchNorm is frozen / absent), a different function otherwise (INTEGRATION, "Many phrases per
        image").  Every image slot must be used by some query (the batch builder's business).  Not together with sync_batchnorm."""
        self._shared_train = bool(enable)
        return self

    def eval_precision(self, dtype: str = "fp32") -> "ZSGNet":
        """Operand precision of the convolutions of the EVAL plans: "fp32" (default: what every plan lowered before) or "bf16" — every
        convolution behind the stem runs on bf16 MFMA (zsg_conv_igemm_bf16: fp32 activations rounded by the operand loader, weights packed
        once per forward, fp32 accumulation and epilogue); the stem, the query encoder, the language map, pooling, upsampling and
        l2norm stay fp32 — or "bf16_act": "bf16", and the activations between the stem's max-pool and the heads' last convolution are STORED
        as bf16 (half the activation bytes of the plan; each value rounded once where it is stored, all arithmetic fp32: include/zsg.h), the
        stem's output, the query encoder, the language maps, the shared plan's accumulator and the outputs stay fp32.  Train-mode plans are
        untouched.  The eval plan cache is keyed by the dtype, so switching back and forth reuses plans."""
        if dtype not in EVAL_DTYPES:
            raise ValueError(f"eval_dtype={dtype!r}: expected one of {', '.join(EVAL_DTYPES)}")
        self._eval_dtype = dtype
        return self

    def eval_tta(self, mode: str = "none") -> "ZSGNet":
        """Test-time augmentation of the EVAL forwards: "none" (default: one pass over the batch as given) or "flip" — the batch of B
        queries runs as ONE eval forward of 2B rows: rows 0..B-1 as given, rows B..2B-1 with the image mirrored along W and the query
        vectors of inp["qvec_flip"] (the embedding of dat_loader.swap_left_right(query); without that key the mirrored rows read
        inp["qvec"]: an image-only flip), the same qlens and the same h0 | c0.  The two halves are merged per anchor in regression-parameter
        space (anchor (y, x, k) of a level with anchor (y, w-1-x, k) of the mirrored row; tx changes sign; zsg_tta_flip_merge, include/zsg.h)
        into a fresh [B, A, 5] output: the caller cannot tell it from a plain one by its shape.  tests/tta_ref.py is the definition.
        Training-mode forwards ignore the switch.  The forward uses the plain eval plan of 2B rows (for a batch with img_idx: 2Bi image
        slots, 2Q queries), so it composes with eval_precision and switching back and forth reuses plans."""
        if mode not in EVAL_TTAS:
            raise ValueError(f"eval_tta={mode!r}: expected one of {', '.join(EVAL_TTAS)}")
        self._eval_tta = mode
        return self

    def _tta_on(self) -> bool:
        return self._eval_tta == "flip" and not self.training

    def eval_scales(self, scales=()) -> "ZSGNet":
        """Multi-scale test-time augmentation of the EVAL forwards: () (default: one pass) or up to four factors in [0.5, 2].  Pass 0 is
        the batch as given, H x W; every entry s adds one pass over the batch resampled ON THE DEVICE to (round(s H), round(s W)) with
        Pillow's bicubic (zsg_resize_u8_batched, byte-identical to PIL.Image.resize of the batch's own pixels — not of the raw file: for
        real detail at the large scales set resize_img to the largest one).  Every pass is the plain eval forward of its geometry, with
        the same queries and LSTM state and, under eval_tta("flip"), its own mirrored rows and merge.  The returned dict is pass 0's,
        plus tta_att_bbx_out [B, sum A_s, 5] (the passes' outputs along the anchor axis, pass 0 first, a fresh tensor) and tta_feat_sizes
        (a host list of one [(h, w), ...] per pass): anchors are normalised image coordinates, so the pooled output is one more head
        output over the concatenated anchor tables (Evaluator reads the two keys).  Needs the uint8 [B, H, W, 3] batch.  Training-mode
        forwards ignore the switch.  Sizes that collide (with each other or with H x W) are a ValueError at the forward."""
        self._eval_scales = check_eval_scales(scales)
        return self

    def _forward_scales(self, inp: Dict[str, Any]) -> Dict[str, Any]:
        """the eval forward under eval_scales: pass 0 on the batch as given, then one plain eval forward per extra size"""
        img = inp["img"]
        if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[3] != 3:
            raise ValueError("eval_scales needs the uint8 [B, H, W, 3] image batch (cfg gpu_img_normalise, the default); an fp32 NCHW img "
                             "is not resampled")
        B, H, W, _ = img.shape
        sizes = eval_scale_sizes(H, W, self._eval_scales)
        geo = self.plan_geometry(inp)
        Q = geo[1] if len(geo) == 5 else None
        plans = [self._plan_for(geo[0], H, W, geo[-1], Q=Q)]
        for s, (Hs, Ws) in zip(self._eval_scales, sizes):      # every pass must lower before any pass runs
            try:
                plans.append(self._plan_for(geo[0], Hs, Ws, geo[-1], Q=Q))
            except Exception as e:
                raise ValueError(f"eval_scales: scale {s!r} ({Hs} x {Ws} from {H} x {W}) cannot be lowered: {e}") from e
        img = img.contiguous()
        res = dict(self._forward_one(inp))
        outs = [res["att_bbx_out"].detach()]
        for Hs, Ws in sizes:
            outs.append(self._forward_one(dict(inp, img=self._resample(img, Hs, Ws)))["att_bbx_out"].detach())
        res["tta_att_bbx_out"] = torch.cat(outs, dim=1)
        res["tta_feat_sizes"] = [[(int(h), int(w)) for h, w in p.feat_sizes] for p in plans]
        return res

    def _resample(self, img: torch.Tensor, Hs: int, Ws: int) -> torch.Tensor:
        """img uint8 [B, H, W, 3] on the device -> uint8 [B, Hs, Ws, 3], dat_loader.GpuResizer's two launches; one resizer and one output
        batch per geometry, made by its first batch (imported here: the model does not need the loader to be imported)"""
        B, H, W, _ = img.shape
        key = (B, H, W, Hs, Ws)
        if key not in self._ms_resize:
            from .dat_loader import GpuResizer
            self._ms_resize[key] = (GpuResizer((Hs, Ws), device=img.device), torch.empty(B, Hs, Ws, 3, dtype=torch.uint8, device=img.device))
        rz, out = self._ms_resize[key]
        return rz.resize_flat(img.view(-1), [(H, W)] * B, out=out)

    def _tta_inputs(self, inp: Dict[str, Any], h0, c0):
        """(qvec, qlens, h0, c0) of the 2B rows of a flip-TTA forward: the mirrored rows behind the rows as given"""
        qvec, qlens = inp["qvec"], inp["qlens"]
        qf = inp.get("qvec_flip")
        if qf is None:
            qf = qvec
        elif not isinstance(qf, torch.Tensor) or qf.shape != qvec.shape or qf.device != qvec.device or qf.dtype != qvec.dtype:
            raise ValueError("qvec_flip must have the shape, dtype and device of qvec")
        ql = qlens.reshape(-1)
        return torch.cat([qvec, qf]), torch.cat([ql, ql]), torch.cat([h0, h0], dim=1), torch.cat([c0, c0], dim=1)

    def wgrad_precision(self, dtype: str = "fp32") -> "ZSGNet":
        """Operand precision of the convolution weight gradients of the TRAINING plans: "fp32" (default: what every plan lowered before,
        launch for launch) or "bf16" — every weight gradient that goes through _Plan.wgrad and that zsg_conv_wgrad_bf16 accepts runs on
        bf16 MFMA (src and dy rounded by the operand loader, fp32 accumulation, the fp32 slab reduction; include/zsg.h).  The forward, the
        loss, every data gradient, the stem's weight gradient and the directly lowered small ones (LSTM projections, head conv0's language
        / grid columns) stay fp32: everything but those weight gradients keeps the fp32 plan's bits.  Eval plans ignore the switch.  The
        precision is part of a training plan's identity: switching drops the training plans of the other precision."""
        if dtype not in WGRAD_DTYPES:
            raise ValueError(f"wgrad_dtype={dtype!r}: expected one of {', '.join(WGRAD_DTYPES)}")
        self._wgrad_dtype = dtype
        return self

    def train_precision(self, dtype: str = "fp32") -> "ZSGNet":
        """Operand precision of the forward convolutions and data gradients of the TRAINING plans: "fp32" (default: what every plan
        lowered before, launch for launch) or "bf16_head" — the convolutions of the pyramid (backbone.fpn.*) and of the head stacks, which
        contain no BatchNorm, run on bf16 MFMA in the forward (zsg_conv_igemm_bf16: fp32 activations rounded by the operand loader, the
        weights packed by one launch per forward, fp32 accumulation, bias / add / ReLU epilogue) and in the data gradient
        (zsg_conv_igemm_bf16_m: the same with the ReLU-mask epilogue, on the packed transposed filter), except where the data gradient
        lands in a BatchNorm output (the laterals P*_1 and P6: it may carry that BatchNorm's backward sums, which are fp32 only).  The
        encoder, the query encoder, the language / grid maps, every weight gradient (wgrad_precision decides those) and every activation
        in memory stay fp32.  Eval plans ignore the switch.  The precision is part of a training plan's identity: switching drops the
        training plans of the other precision."""
        if dtype not in TRAIN_DTYPES:
            raise ValueError(f"train_dtype={dtype!r}: expected one of {', '.join(TRAIN_DTYPES)}")
        self._train_dtype = dtype
        return self

    def encoder_precision(self, dtype: str = "fp32") -> "ZSGNet":
        """Operand precision of the forward convolutions of the ENCODER in the TRAINING plans: "fp32" (default: what every plan lowered
        before, launch for launch) or "bf16_fwd" — every forward convolution named backbone.encoder.* of a ResNet encoder (basic blocks and
        bottlenecks, projection shortcuts included) runs on bf16 MFMA: in front of a live train-mode BatchNorm zsg_conv_igemm_bf16_bn,
        whose epilogue writes the BatchNorm's partial rows as the fp32 launch does (fp32 activations rounded by the operand loader, the
        weights packed by the forward's one pack launch, fp32 accumulation; include/zsg.h), in front of a frozen BatchNorm the plain
        zsg_conv_igemm_bf16.  Not covered: the stem, and a convolution whose source carries a PENDING BatchNorm (it applies that
        BatchNorm in its operand loader: zsg_conv_igemm_bnpre, fp32 with all its fusions).  The whole backward is the fp32 plan's
        lowering — fp32 data gradients with their BatchNorm-backward epilogues, weight gradients as wgrad_precision says — and every
        activation in memory stays fp32.  The SSD-VGG encoder is not covered: there the switch changes nothing.  Eval plans ignore the
        switch.  Independent of train_precision, wgrad_precision and eval_precision.  The precision is part of a training plan's
        identity: switching drops the training plans of the other precision."""
        if dtype not in ENC_DTYPES:
            raise ValueError(f"enc_dtype={dtype!r}: expected one of {', '.join(ENC_DTYPES)}")
        self._enc_dtype = dtype
        return self

    def encoder_backward_precision(self, dtype: str = "fp32") -> "ZSGNet":
        """Operand precision of the DATA GRADIENTS of the encoder in the TRAINING plans: "fp32" (default: what every plan lowered before,
        launch for launch) or "bf16" — every data gradient of a convolution named backbone.encoder.* of a ResNet encoder (never the
        stem's) that zsg_conv_igemm_bf16_m accepts runs on bf16 MFMA (dy rounded by the operand loader, the transposed filter packed by
        one launch with the other weight-only work, fp32 accumulation, no Winograd, no split-K).  Where such a launch completes the
        dout of a BatchNorm (live, frozen or synchronized) it is re-issued as zsg_conv_igemm_bf16_bnb, whose epilogue writes that
        BatchNorm's backward partial rows as the fp32 launch does (include/zsg.h); there is no in-kernel finalize on this path:
        zsg_bn_backward_from_partials reduces the rows.  The whole forward, the stem, the pyramid's data gradients into C3-C5, every
        weight gradient (wgrad_precision decides those) and every activation in memory stay fp32.  The SSD-VGG encoder is not covered:
        there the switch changes nothing.  Eval plans ignore the switch.  Independent of encoder_precision, train_precision,
        wgrad_precision and eval_precision.  The precision is part of a training plan's identity: switching drops the training plans of
        the other precision."""
        if dtype not in ENC_BWD_DTYPES:
            raise ValueError(f"enc_bwd_dtype={dtype!r}: expected one of {', '.join(ENC_BWD_DTYPES)}")
        self._enc_bwd_dtype = dtype
        return self

    def _enc_key(self) -> Tuple:
        """what encoder_precision and encoder_backward_precision add to a training plan's key (as _train_key: nothing for fp32, whose
        key stays what it always was; ("encb", ...) stands behind ("enc", ...))"""
        return (() if self._enc_dtype == "fp32" else (("enc", self._enc_dtype),)) + (() if self._enc_bwd_dtype == "fp32" else (("encb", self._enc_bwd_dtype),))

    @staticmethod
    def _key_encb(k: Tuple) -> str:
        """the encoder data-gradient precision of a training plan's key"""
        return next((e[1] for e in k[7:-1] if isinstance(e, tuple) and e[0] == "encb"), "fp32")

    @staticmethod
    def _key_enc(k: Tuple) -> str:
        """the encoder-forward precision of a training plan's key"""
        return next((e[1] for e in k[7:-1] if isinstance(e, tuple) and e[0] == "enc"), "fp32")

    def _enc_kw(self) -> Dict[str, str]:
        """the _Plan keyword of the switch: none with the default, so that a plan of the default is constructed exactly as before"""
        kw = {} if self._enc_dtype == "fp32" else {"enc_dtype": self._enc_dtype}
        if self._enc_bwd_dtype != "fp32":
            kw["enc_bwd_dtype"] = self._enc_bwd_dtype
        return kw

    def _train_key(self) -> Tuple:
        """what train_precision adds to a training plan's key (as _wgrad_key: nothing for fp32, whose key stays what it always was)"""
        return () if self._train_dtype == "fp32" else (("train", self._train_dtype),)

    @staticmethod
    def _key_train(k: Tuple) -> str:
        """the forward / data-gradient precision of a training plan's key"""
        return next((e[1] for e in k[7:-1] if isinstance(e, tuple) and e[0] == "train"), "fp32")

    def _wgrad_key(self) -> Tuple:
        """what the weight-gradient precision adds to a training plan's key, in front of its trailing fields (_plan_for reads those by
        position from the end and the leading ones by index): nothing for fp32, whose key stays what it always was"""
        return () if self._wgrad_dtype == "fp32" else (("wgrad", self._wgrad_dtype),)

    @staticmethod
    def _key_wgrad(k: Tuple) -> str:
        """the weight-gradient precision of a training plan's key"""
        return next((e[1] for e in k[7:-1] if isinstance(e, tuple) and e[0] == "wgrad"), "fp32")

    @staticmethod
    def _key_shared(k: Tuple):
        """("shared", Q) of a shared-image training plan's key, else None"""
        return next((e for e in k[7:-1] if isinstance(e, tuple) and e[0] == "shared"), None)

    def _eval_key(self, B, H, W, T, Q: Optional[int] = None) -> Tuple:
        """plan-cache key of an eval plan; the default dtype keeps the key it always had"""
        dt = () if self._eval_dtype == "fp32" else (self._eval_dtype,)
        if Q is not None:
            return (B, Q, H, W, T, "shared") + dt + (False,)
        return (B, H, W, T) + dt + (False,)

    def _refuse_sync_shared(self, inp) -> None:
        """sync_batchnorm + a shared training batch is out of scope: refused before any collective of the forward is issued (the
        data-parallel wrapper calls this ahead of its buffer broadcast)"""
        if (inp.get("img_idx") is not None and self.training and getattr(self, "_shared_train", False) and self.use_img and self.use_lang
                and self._sync_bn_key()):
            raise RuntimeError("ZSGNet.forward: sync_batchnorm together with shared_training (a training batch with img_idx) is not "
                               "supported; use per-rank BatchNorm statistics (sync_batchnorm(enable=False)) or freeze_batchnorm()")

    def _plan_for(self, B, H, W, T, Q: Optional[int] = None) -> "_Plan":
        if Q is not None and self.training:
            # shared-image training plan: exactly B image slots and Q queries.  One (B, Q) at a time: a new one, like a new trainable set,
            # drops the shared training plans of the old (activation buffers must not pile up)
            fz, fb, sb = self._frozen_key(), self._frozen_bn_key(), self._sync_bn_key()
            key = (B, H, W, T, fz, fb, sb, ("shared", Q)) + self._wgrad_key() + self._train_key() + self._enc_key() + (True,)
            if key not in self._plans:
                for k in [k for k in self._plans if k[-1] and ((k[4], k[5], k[6]) != (fz, fb, sb) or self._key_wgrad(k) != self._wgrad_dtype
                                                               or self._key_train(k) != self._train_dtype or self._key_enc(k) != self._enc_dtype or self._key_encb(k) != self._enc_bwd_dtype
                                                               or (self._key_shared(k) is not None and (k[0], self._key_shared(k)[1]) != (B, Q)))]:
                    old = self._plans.pop(k)
                    if old._prep_pending:
                        torch.cuda.current_stream().wait_event(old._prep_ev)
                bn_names = list(self.bns)
                self._plans[key] = _Plan(self, B, H, W, T, True, frozen={self._param_names[i] for i in fz},
                                         frozen_bn={bn_names[i] for i in fb}, Q=Q, wgrad_dtype=self._wgrad_dtype, train_dtype=self._train_dtype,
                                         **self._enc_kw())
            return self._plans[key]
        if Q is not None:
            # eval-only plan of Q queries over B (bucketed) images; the cache of these is bounded: least recently used first out
            assert not self.training
            key = self._eval_key(B, H, W, T, Q)
            if key in self._plans:
                self._plans[key] = self._plans.pop(key)         # (most recently used last)
            else:
                old = [k for k in self._plans if len(k) in (7, 8) and k[5] == "shared"]      # (of every eval dtype: one bound)
                # (a multi-scale set is one plan per pass: the bound grows with the passes, so that a set never evicts its own members)
                for k in old[:max(0, len(old) + 1 - SHARED_PLANS_MAX * (1 + len(self._eval_scales)))]:
                    del self._plans[k]
                self._plans[key] = _Plan(self, B, H, W, T, False, Q=Q, dtype=self._eval_dtype)
            return self._plans[key]
        if not self.training:
            key = self._eval_key(B, H, W, T)
            if key not in self._plans:
                self._plans[key] = _Plan(self, B, H, W, T, False, dtype=self._eval_dtype)
            return self._plans[key]
        fz, fb, sb = self._frozen_key(), self._frozen_bn_key(), self._sync_bn_key()
        key = (B, H, W, T, fz, fb, sb) + self._wgrad_key() + self._train_key() + self._enc_key() + (True,)
        if key not in self._plans:
            # a new trainable set, frozen-BatchNorm set or synchronized-BatchNorm set: the training plans of the old one go (gradual
            # unfreezing must not pile up activation buffers)
            for k in [k for k in self._plans if k[-1] and ((k[4], k[5], k[6]) != (fz, fb, sb) or self._key_wgrad(k) != self._wgrad_dtype
                                                           or self._key_train(k) != self._train_dtype or self._key_enc(k) != self._enc_dtype
                                                           or self._key_encb(k) != self._enc_bwd_dtype)]:
                old = self._plans.pop(k)
                if old._prep_pending:           # (its side-stream weight preparation may still be reading the weights)
                    torch.cuda.current_stream().wait_event(old._prep_ev)
            bn_names = list(self.bns)
            self._plans[key] = _Plan(self, B, H, W, T, True, frozen={self._param_names[i] for i in fz},
                                     frozen_bn={bn_names[i] for i in fb}, sync_bn={bn_names[i] for i in sb}, wgrad_dtype=self._wgrad_dtype,
                                     train_dtype=self._train_dtype, **self._enc_kw())
        return self._plans[key]

    def _forward_shared(self, inp: Dict[str, Any]) -> Dict[str, Any]:
        """forward for `img` [Bi, ...] shared by Q >= Bi queries, img_idx [Q] (device integers in [0, Bi)) naming each query's image: row
        q of the result is what forward returns for the pair (img[img_idx[q]], query q).  Eval-only, forward-only.  The image trunk and
        head conv0's feature GEMM run once per image, everything that depends on the phrase once per query; img_idx is read by the
        kernel (zsg_head_shared_conv0), never by the host: its range is the batch builder's business (dat_loader's grouped collater)."""
        img, qvec, idx = inp["img"], inp["qvec"], inp["img_idx"]
        train = self.training and getattr(self, "_shared_train", False)
        self._refuse_sync_shared(inp)
        if self.training and not train:
            raise RuntimeError("ZSGNet.forward: a batch with img_idx (queries sharing images) is eval-only; call net.eval() (gradients "
                               "through shared images are not supported)")
        if not isinstance(idx, torch.Tensor) or idx.device != img.device or idx.dim() != 1 or idx.dtype not in (torch.int64, torch.int32):
            raise ValueError("img_idx must be a 1-d int64 / int32 tensor on the device of img")
        Q = qvec.shape[0]
        if idx.numel() != Q or inp["qlens"].numel() != Q:
            raise ValueError(f"img_idx / qlens must have one entry per query ({Q})")
        if not (self.use_img and self.use_lang):
            # blind variants: no image path or no phrase path to share; the plain plan on the gathered images (a device gather)
            sub = {k: v for k, v in inp.items() if k != "img_idx"}
            sub["img"] = img.index_select(0, idx.long())
            return self._forward_one(sub)
        tta = self._tta_on()
        Bp, Qp, H, W, Tp = self.plan_geometry(inp)
        plan = self._plan_for(Bp, H, W, Tp, Q=Qp)
        if "h0" in inp:
            h0, c0 = inp["h0"], inp["c0"]
        else:
            h0, c0 = self.lstm_init_hidden(Q)
        plan.tta = tta
        if tta:
            # 2Bi image slots (the mirrors behind the originals) and 2Q queries; a mirrored query points at its image's mirror
            qvec, qlens, h0, c0 = self._tta_inputs(inp, h0, c0)
            idx = torch.cat([idx, idx + img.shape[0]])
            inp = dict(inp, qlens=qlens)
        if self._anchor is None or self._anchor.device != img.device:
            self._anchor = torch.zeros(1, device=img.device, requires_grad=True)
        if train:
            # the shared-image TRAINING plan (shared_training): exactly img.shape[0] image slots; the loss / evaluator / optimizer see
            # Q rows and the flat gradient buffer, as with the plain plan
            plan.expect_backward = torch.is_grad_enabled()
            out5 = _SharedTrainFn.apply(self, plan, img, qvec, inp["qlens"], h0, c0, idx, self._anchor)
            out5._zsg_g5 = plan.g5_in
            out5._zsg_plan = plan
            return dict(att_out=out5[..., 4:5], bbx_out=out5[..., :4], feat_sizes=plan.feat_sizes_t,
                        num_f_out=plan.num_f_out_t, att_bbx_out=out5)
        plan.expect_backward = False
        out5 = _SharedFn.apply(plan, img, qvec, inp["qlens"], h0, c0, idx, self._anchor)
        return dict(att_out=out5[..., 4:5], bbx_out=out5[..., :4], feat_sizes=plan.feat_sizes_t,
                    num_f_out=plan.num_f_out_t, att_bbx_out=out5)

    def forward(self, inp: Dict[str, Any]) -> Dict[str, Any]:
        require_gpu()
        img = inp["img"]
        if img.device.type != "cuda" or self.device.type != "cuda":
            raise RuntimeError("ZSGNet.forward needs the model and the batch on the MI355X (no CPU fallback)")
        if self._eval_scales and not self.training:
            return self._forward_scales(inp)
        return self._forward_one(inp)

    def _forward_one(self, inp: Dict[str, Any]) -> Dict[str, Any]:
        """one forward of the batch as given (under eval_scales: one pass)"""
        img, qvec, qlens = inp["img"], inp["qvec"], inp["qlens"]
        if inp.get("img_idx") is not None:
            return self._forward_shared(inp)
        # (img may be uint8 [B, H, W, 3] as PIL decodes (dat_loader gpu_normalise): /255 then happens on the GPU.)
        # The collater cuts qvec to the longest query of the batch (dat_loader.py:187-196), so T changes from batch to batch;
        # a launch plan (and its buffers) is built per geometry, so T is bucketed: the plan processes T_plan >= T tokens of
        # zero-padded input — the LSTM kernels stop at each query's own length, so the result does not depend on T_plan.
        tta = self._tta_on()
        B, H, W, Tp = self.plan_geometry(inp)
        plan = self._plan_for(B, H, W, Tp)
        if "h0" in inp:
            h0, c0 = inp["h0"], inp["c0"]
        else:
            h0, c0 = self.lstm_init_hidden(B // 2 if tta else B)
        plan.tta = tta
        if tta:
            qvec, qlens, h0, c0 = self._tta_inputs(inp, h0, c0)
        # ONE differentiable input ties the custom Function into autograd: run_backward writes the parameter gradients
        # straight into the flat gradient buffer that every p.grad views, so autograd has nothing to accumulate per
        # parameter (161 AccumulateGrad nodes cost the host ~0.5 ms per step with the GPU idle at the end of backward)
        if self._anchor is None or self._anchor.device != img.device:
            self._anchor = torch.zeros(1, device=img.device, requires_grad=True)
        plan.expect_backward = torch.is_grad_enabled()      # (grad mode is off inside autograd.Function.forward: decide here)
        out5 = _NetFn.apply(self, plan, img, qvec, qlens, h0, c0, self._anchor)
        if plan.training:
            out5._zsg_g5 = plan.g5_in           # where the loss may write d(loss)/d(out5) directly (loss._LossFn.forward): no copy, no multiply
            out5._zsg_plan = plan
        return dict(att_out=out5[..., 4:5], bbx_out=out5[..., :4], feat_sizes=plan.feat_sizes_t,
                    num_f_out=plan.num_f_out_t, att_bbx_out=out5)


class _SharedFn(torch.autograd.Function):
    """forward of the shared-image eval plan; it has no backward"""
    @staticmethod
    def forward(ctx, plan, img, qvec, qlens, h0, c0, img_idx, anchor):
        return plan.run_forward(img, qvec, qlens, h0, c0, img_idx=img_idx)

    @staticmethod
    def backward(ctx, g5):
        raise RuntimeError("ZSGNet: a batch with img_idx (queries sharing images) is eval-only and forward-only: there are no gradients "
                           "through the shared-image path")


class _SharedTrainFn(torch.autograd.Function):
    """forward / backward of the shared-image training plan (ZSGNet.shared_training)"""
    @staticmethod
    def forward(ctx, net, plan, img, qvec, qlens, h0, c0, img_idx, anchor):
        ctx.plan = plan
        out = plan.run_forward(img, qvec, qlens, h0, c0, img_idx=img_idx)
        ctx.fwd_id = plan.fwd_id
        return out

    @staticmethod
    def backward(ctx, g5):
        if ctx.fwd_id != ctx.plan.fwd_id:
            raise RuntimeError("backward of a forward whose activations were overwritten: this geometry's plan ran another "
                               "forward since (one backward per forward per input geometry)")
        ctx.plan.run_backward(g5)
        return (None,) * 9


class _NetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, plan, img, qvec, qlens, h0, c0, anchor):
        ctx.net, ctx.plan = net, plan
        out = plan.run_forward(img, qvec, qlens, h0, c0)
        ctx.fwd_id = plan.fwd_id
        return out

    @staticmethod
    def backward(ctx, g5):
        # a plan owns ONE set of activation buffers: the backward must belong to the plan's latest forward
        if ctx.fwd_id != ctx.plan.fwd_id:
            raise RuntimeError("backward of a forward whose activations were overwritten: this geometry's plan ran another "
                               "forward since (one backward per forward per input geometry)")
        ctx.plan.run_backward(g5)
        return (None,) * 8


class _Plan:
    """Static lowering of ZSGNet for one (B, H, W, T, training) geometry."""

    def __init__(self, net: ZSGNet, B: int, H: int, W: int, T: int, training: bool, frozen=frozenset(), frozen_bn=frozenset(),
                 sync_bn=frozenset(), Q: Optional[int] = None, dtype: str = "fp32", wgrad_dtype: str = "fp32", train_dtype: str = "fp32", enc_dtype: str = "fp32",
                 enc_bwd_dtype: str = "fp32"):
        self.net, self.B, self.H, self.W, self.T, self.training = net, B, H, W, T, training
        self.tta = False            # set per forward by ZSGNet.forward (eval_tta "flip", eval plans only): see run_forward
        # training plans only (ZSGNet.wgrad_precision): the weight gradients that go through wgrad() are lowered to zsg_conv_wgrad_bf16
        assert wgrad_dtype in WGRAD_DTYPES
        self.wgrad_bf16 = training and wgrad_dtype == "bf16"
        # training plans only (ZSGNet.train_precision): the forward convolutions of the pyramid and the heads are lowered to
        # zsg_conv_igemm_bf16 (their packed weights refreshed by ONE pack launch per forward, on the side stream with the other weight-only
        # work: prep_u), their data gradients to zsg_conv_igemm_bf16_m (the packed transposed filters by one more pack launch in prep)
        assert train_dtype in TRAIN_DTYPES
        self.train_bf16 = training and train_dtype == "bf16_head"
        self.dpack_jobs, self.dpack_blocks, self.dpack_jobs_dev, self._dpack = [], 0, None, {}
        # training plans only (ZSGNet.encoder_precision): the forward convolutions of a ResNet encoder behind the stem are lowered to
        # zsg_conv_igemm_bf16_bn (fused BatchNorm partial rows) / zsg_conv_igemm_bf16 (frozen BatchNorm); their packed weights join the
        # forward's one pack launch; the backward is the fp32 lowering's.  _b16_log entries of kind "enc_fwd" (see below) also hold
        # bn (the BatchNorm's name), frozen and mean / invstd (the statistics buffers it normalises with), filled by bn()
        assert enc_dtype in ENC_DTYPES
        self.enc_bf16 = training and enc_dtype == "bf16_fwd" and net.backbone_kind == "retina"
        # enc_bwd_dtype = "bf16": the data gradients of the encoder behind the stem on bf16 MFMA (dgrad, _bnb_reissue); _b16_log entries of
        # kind "enc_dgrad" hold d, src (dy), out (dx), add, window, pname and, where the launch was re-issued with a BatchNorm's backward
        # sums, bn, x, mean, invstd, rmask, part, chunks and epi_flags
        assert enc_bwd_dtype in ENC_BWD_DTYPES
        self.encb_bf16 = training and enc_bwd_dtype == "bf16" and net.backbone_kind == "retina"
        # every launch train_dtype = "bf16_head" put on bf16 MFMA, in lowering order: dict(kind "fwd" | "dgrad", what, idx (launch index in
        # fwd / bwd), d (descriptor copy), src (src / dy), out (out / dx), add (Act | None), mask (Act | None), pname (weight), window
        # ((wc0, C) of the weight's channels, forward; (row0, n) of its input channels, data gradient)).  No plan buffer is recycled, so
        # after a step the operands still hold that step's values (the tests recompute each layer from them)
        self._b16_log = []
        # eval plans only (ZSGNet.eval_precision): every convolution zsg_conv_igemm_bf16 supports is lowered to it; their weights are
        # packed to bf16 by ONE zsg_pack_w_bf16_batched launch per forward (behind the BatchNorm fold, whose output it reads)
        assert dtype in EVAL_DTYPES and not (training and dtype != "fp32")
        self.bf16 = dtype in ("bf16", "bf16_act")
        # bf16_act: the activations behind the stem are 16-bit buffers (adt), the convolutions go through zsg_conv_igemm_bf16_io with the
        # flags their operands' dtypes imply, the element-wise launches through csrc/bf16_act.hip; an operation without a bf16 form is
        # wrapped in casts (_f32 / _via_f32)
        self.act16 = dtype == "bf16_act"
        self.adt = torch.bfloat16 if self.act16 else torch.float32
        self.pack_jobs, self.pack_blocks, self.pack_keep, self.pack_jobs_dev = [], 0, [], None
        # Q: a shared-image plan (ZSGNet._forward_shared) — the image trunk up to conv0's feature GEMM is lowered at batch B (image
        # slots), the query encoder and everything behind zsg_head_shared_conv0 at batch Q; every other plan has one batch, Q == B.  A
        # shared TRAINING plan (ZSGNet.shared_training) has exactly B slots, all used; its backward turns the gradient of h1 [Q] into
        # the gradient of conv0's per-image accumulator with zsg_head_shared_conv0_bwd and runs conv0's feature weight / data gradients
        # and the whole trunk backward at batch B
        self.shared = Q is not None
        self.Q = Q if Q is not None else B
        assert not (self.shared and training and sync_bn), "shared training does not synchronize BatchNorm across ranks"
        # BatchNorm layers in eval mode inside this training network: running statistics in the forward (one zsg_bn_eval_stats launch),
        # no statistics update, F.batch_norm(training=False)'s backward (zsg_bn_frozen_backward / zsg_bn_frozen_relu_maxpool_bwd)
        self.frozen_bn = frozenset(frozen_bn) if training else frozenset()
        self._ev_stats = None
        # BatchNorm layers synchronized across the ranks of net._sync_bn_group (ZSGNet.sync_batchnorm): every statistics pass stops at
        # rank-local fp64 sums (zsg_bn_sync_*), a host op of the program all-reduces them on the stream of its lane, and the finalize /
        # apply restarts from the global sums.  sync_bn_paths records the forms each layer took: forward 'partials' (the producing
        # convolution's epilogue rows) or 'x' (a pass over the input), '+bnpre' (applied by the next convolution's loader); backward
        # 'bnb' (the data gradient's epilogue rows), 'plain' (a pass over dout / x) or 'stem'; '+alias' when the residual's gradient
        # aliases dout
        self.sync_bn = (frozenset(sync_bn) - self.frozen_bn) if training else frozenset()
        self.sync_bn_paths: Dict[str, str] = {}
        self._sync_sums: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
        # which backward form each frozen layer got (_bn_frozen_back): 'bnb+fin' / 'bnb' (sums from the data gradient's epilogue, with or
        # without its in-kernel finalize), 'onepass' (zsg_bn_frozen_backward reduces them), 'scale' (no sums: frozen affine); '+alias' when
        # the residual's gradient aliases dout
        self.frozen_bn_paths: Dict[str, str] = {}
        # parameters with requires_grad=False when the plan was lowered: no weight / bias gradient, no data gradient into an activation
        # that no trainable parameter lies upstream of (Act.requires_grad), no p.grad view, no DDP bucket
        self.frozen = frozenset(frozen) if training else frozenset()
        self.dev = net.device
        apply_main_priority_env()
        self.fwd = Program("fwd")
        self.prep = Program("bwd-prep")
        self._prep_stream, self._prep_ev, self._prep_fwd, self._prep_pending = None, None, -1, False
        self._bwd_fwd = -2               # fwd_id of the forward whose backward ran last (a second backward re-runs the preparation)
        self._rel_ev = torch.cuda.Event()
        self._hc_pin, self._hc_ev = None, None      # pinned ring of host-drawn LSTM states (run_forward)
        self._prep_idx_v = False
        self._out_slots_v = False
        self.expect_backward = False
        self._tunables = []              # convolution descriptors of this plan, as lowered (ops.refine_in_step)
        self._wg_log = []                # (launch index, descriptor, src, dy, gradient view, parameter, name) of every convolution weight gradient
        self.g5_from_loss = None         # (fwd_id, scale): the loss kernel wrote d(loss)/d(out5) x scale into g5_in for that forward
        self.bwd = Program("bwd")
        self.bwd.side_batch = 3 if B * H * W <= (4 << 20) else 1      # (ops.SIDE_BATCH: markers vs overlap, measured)
        self.bwd.side_defer = 1      # (ops.SIDE_DEFER; round 5, with the main chain at wave priority 3: 1 wins at every size)
        self.tape = []
        self.acts: Dict[str, Act] = {}
        self.bytes = 0
        self.wt: Dict[str, torch.Tensor] = {}
        self.grad_ready: Dict[str, int] = {}
        self.reducer = None
        self.fwd_id = 0
        self.wt_jobs, self.wt_arena_used = [], 0
        self.wt_arena = self._buf(net.store.total + 4096 * len(net.convs)) if training else None
        self.fold_jobs, self.fold_used, self.fold_rows = [], 0, 0          # eval: BatchNorm folded into the convolutions
        self.fold_arena = self._buf(net.store.total + 8 * len(net.convs)) if (not training and net.bns) else None
        self.wino_jobs = {"fwd": WinoJobs(), "bwd": WinoJobs()}     # filter transforms of the Winograd convolutions (one launch each)
        # work that depends on the weights only / touches buffers nobody reads yet: runs on the side stream at the start of a training
        # forward (Winograd filter transforms, zero-fills of split-K outputs); the main stream waits for it right before the first
        # launch that needs any of it (_wait_idx): an event WAIT, no marker of its own
        self.prep_u, self._u_ev, self._wait_idx = Program("fwd-prep"), None, 1 << 30
        self._side_prep = training
        self._zero_calls = []
        self._lower()
        for i, c in enumerate(self.fwd.calls):          # (positions after the hoisting of the language maps)
            if any(c is z for z in self._zero_calls):
                self._wait_idx = min(self._wait_idx, i)
                break
        wj = self.wino_jobs["fwd"]
        if wj.jobs and self._side_prep:
            # U = G g G^T of every Winograd forward convolution depends on the weights only: in training it runs on the side stream
            # while the main stream converts the image and runs the stem (it was 47 us at the head of the forward's dependent chain)
            self.prep_u.add(lib.zsg_wino_weights, wj.finish(self.dev), len(wj.jobs), wj.blocks, what="wino filter transforms")
            self.prep_u.calls.insert(0, self.prep_u.calls.pop())          # (needed first)
            self.prep_u.lanes.insert(0, self.prep_u.lanes.pop())
            wfns = (lib.zsg_conv_wino, lib.zsg_conv_wino_bnstat)
            self._wait_idx = min(self._wait_idx, next(i for i, c in enumerate(self.fwd.calls) if c[0] in wfns))
        elif wj.jobs:        # eval (after the BatchNorm fold): first launch after the image conversion
            self.fwd.add(lib.zsg_wino_weights, wj.finish(self.dev), len(wj.jobs), wj.blocks, what="wino filter transforms")
            self.fwd.calls.insert(1, self.fwd.calls.pop())
            self.fwd.lanes.insert(1, self.fwd.lanes.pop())
        if training:
            self._finish_prep()
        elif self.fold_jobs:
            import struct
            blob = b"".join(struct.pack("<qqqqqiiii", *j) for j in self.fold_jobs)
            self.fold_jobs_dev = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(self.dev)
        if self.pack_jobs:
            blob = b"".join(_struct.pack("<qqiiiiiiii", *j) for j in self.pack_jobs)
            self.pack_jobs_dev = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(self.dev)
            if training:
                # train_dtype = "bf16_head": the weights change every step — ONE pack launch per forward with the other weight-only work
                # on the side stream (prep_u: released behind the optimizer step's write of the weights by _rel_ev); the main stream waits
                # for it in front of the first launch that reads an image, a side-stream reader is behind it in its own stream
                self.prep_u.add(lib.zsg_pack_w_bf16_batched, self.pack_jobs_dev, len(self.pack_jobs), self.pack_blocks, what="pack bf16 weight images")
                self._wait_idx = min(self._wait_idx, next(i for i, c in enumerate(self.fwd.calls)
                                                          if c[0] in (lib.zsg_conv_igemm_bf16, lib.zsg_conv_igemm_bf16_bn)))
        for e in self._b16_log:          # (launch indices after the reordering of the programs: hoisting, _batch_wgrads)
            prog = self.fwd if e["kind"] in ("fwd", "enc_fwd") else self.bwd
            call = e.pop("call")
            e["idx"] = next(i for i, c in enumerate(prog.calls) if c is call)

    # ---- allocation helpers --------------------------------------------------------------------------------
    def _buf(self, n, dtype=torch.float32):
        t = torch.zeros(int(n), dtype=dtype, device=self.dev)
        self.bytes += t.numel() * t.element_size()
        return t

    def act(self, name, B, H, W, C, ld=None, requires_grad=True, dtype=torch.float32) -> Act:
        ld = ld or C
        a = Act(self._buf(B * H * W * ld, dtype=dtype), B, C, ld, [Level(0, H, W, H * W * ld)], name)
        a.requires_grad = requires_grad
        self.acts[name] = a
        return a

    def packed(self, name, B, sizes, C, ld=None, dtype=torch.float32) -> Act:
        """pyramid levels packed level-major in one buffer"""
        ld = ld or C
        lv, off = [], 0
        for (h, w) in sizes:
            lv.append(Level(off, h, w, h * w * ld))
            off += B * h * w * ld
        a = Act(self._buf(off, dtype=dtype), B, C, ld, lv, name)
        self.acts[name] = a
        return a

    # ---- bf16_act: casts around an operation that has no bf16 form ------------------------------------------------------------
    @staticmethod
    def _span(a: Act) -> Tuple[int, int]:
        """(first element, element count) of the buffer region an activation owns: one level of a packed buffer, or all of it"""
        if len(a.levels) == 1:
            return a.levels[0].off, a.B * a.levels[0].bstride
        return 0, a.buf.numel()

    def _twin32(self, a: Act) -> Act:
        """an fp32 buffer with the element layout of the bf16 activation `a` (same offsets: descriptors built on `a` stay valid)"""
        t = Act(self._buf(a.buf.numel()), a.B, a.C, a.ld, a.levels, a.name + ".f32")
        t.requires_grad = a.requires_grad
        return t

    def _f32(self, a: Optional[Act], lane: int = 0) -> Optional[Act]:
        """`a` itself when it is fp32, else its fp32 copy (one zsg_cast_bf16_f32 launch)"""
        if a is None or not a.b16:
            return a
        t = self._twin32(a)
        o, n = self._span(a)
        self.fwd.add(lib.zsg_cast_bf16_f32, a.buf[o:], n, t.buf[o:], what="cast f32<-" + a.name, lane=lane)
        return t

    def _via_f32(self, src: Optional[Act], out: Act, add: Optional[Act] = None, lane: int = 0):
        """(src, out, add) as fp32 Acts for an fp32-only launch + finish(): the launch that rounds the fp32 result into the bf16 `out`.
        Identities when nothing is bf16."""
        s32, a32 = self._f32(src, lane), self._f32(add, lane)
        if not out.b16:
            return s32, out, a32, lambda: None
        o32 = self._twin32(out)

        def finish():
            o, n = self._span(out)
            self.fwd.add(lib.zsg_cast_f32_bf16, o32.buf[o:], n, out.buf[o:], what="cast bf16<-" + out.name, lane=lane)
        return s32, o32, a32, finish

    def like(self, a: Act, name=None) -> Act:
        if len(a.levels) == 1:           # a level of a packed buffer gets a compact twin, not a copy of the whole pack
            l = a.levels[0]
            return Act(self._buf(a.B * l.bstride), a.B, a.C, a.ld, [Level(0, l.H, l.W, l.bstride)], name or (a.name + ".grad"))
        g = Act(self._buf(a.buf.numel()), a.B, a.C, a.ld, a.levels, name or (a.name + ".grad"))
        return g

    def grad_of(self, a: Act) -> Act:
        if a.grad is None:
            a.grad = self.like(a)
        return a.grad

    @staticmethod
    def base(a: Act) -> torch.Tensor:
        """flat tensor starting at the first element of a (single-level or packed) activation"""
        return a.buf[a.levels[0].off:]

    def trains(self, name) -> bool:
        """the parameter `name` gets a gradient (it is not frozen)"""
        return name not in self.frozen

    def bn_frozen(self, L: Optional[BnL]) -> bool:
        """the BatchNorm layer L is in eval mode inside this training plan"""
        return L is not None and L.name in self.frozen_bn

    def _eval_stats(self, L: BnL):
        """(mean, invstd) of a frozen BatchNorm layer from its running statistics.  ONE zsg_bn_eval_stats launch over the span of every
        frozen layer's slots, issued on the main stream where the first frozen layer needs it (a side-stream user waits for it: lane 1
        waits for everything enqueued on the main stream before it).  The span may include train-mode layers' slots, whose running
        statistics another launch of this forward may be updating at the same time: the values computed for those slots are never read."""
        if self._ev_stats is None:
            bns = [self.net.bns[n] for n in self.frozen_bn]
            lo, hi = min(b.index for b in bns), max(b.index + b.c for b in bns)
            self._ev_stats = (self._buf(self.net._rm.numel()), self._buf(self.net._rm.numel()))
            m, s = self._ev_stats
            self.fwd.add(lib.zsg_bn_eval_stats, self.net._rm[lo:hi], self.net._rv[lo:hi], hi - lo, 1e-5, m[lo:hi], s[lo:hi],
                         what="eval stats: frozen BatchNorm", lane=0)
        m, s = self._ev_stats
        return m[L.index:L.index + L.c], s[L.index:L.index + L.c]

    def bn_synced(self, L: Optional[BnL]) -> bool:
        """the BatchNorm layer L normalises with statistics all-reduced over the ranks (ZSGNet.sync_batchnorm)"""
        return L is not None and L.name in self.sync_bn

    def _sync_bufs(self, L: BnL) -> Tuple[torch.Tensor, torch.Tensor]:
        """the layer's fp64 sums, allocated with the plan: forward [sum x | sum x^2 | n] (kept for the backward's N), backward
        [sum g | sum g * xhat]"""
        if L.name not in self._sync_sums:
            f = torch.zeros(2 * L.c + 1, dtype=torch.float64, device=self.dev)
            b = torch.zeros(2 * L.c, dtype=torch.float64, device=self.dev)
            self.bytes += (f.numel() + b.numel()) * 8
            self._sync_sums[L.name] = (f, b)
        return self._sync_sums[L.name]

    def _allreduce(self, prog: Program, buf: torch.Tensor, what: str, lane: int):
        """a host op of `prog`: SUM-all-reduce of `buf` over the BatchNorm group, issued from the stream of `lane` (nccl: stream-ordered,
        work.wait() makes that stream wait; gloo blocks the host)"""
        import torch.distributed as dist
        net = self.net

        def allreduce():
            # (the group is read when the op runs: a later conversion with another process group over the same layers keeps this plan)
            dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=net._sync_bn_group, async_op=True).wait()
        prog.add_host(allreduce, what=what, lane=lane)

    def _sync_fwd_stats(self, L: BnL, x: Optional[torch.Tensor], rows: int, partials, chunks: int, mean, invstd, lane: int, ws=None):
        """synchronized statistics: local sums (from the partial rows, else one pass over x) -> all-reduce -> finalize (mean, invstd,
        running statistics from the global sums)"""
        fs, _ = self._sync_bufs(L)
        rm, rv = self.net._rm[L.index:L.index + L.c], self.net._rv[L.index:L.index + L.c]
        if partials is not None:
            self.fwd.add(lib.zsg_bn_sync_fwd_sums, None, rows, L.c, partials, chunks, fs, None, 0, what="bnsums:" + L.name, lane=lane)
        else:
            self.fwd.add(lib.zsg_bn_sync_fwd_sums, x, rows, L.c, None, 0, fs, ws, self.ws_bytes, what="bnsums:" + L.name, lane=lane)
        self._allreduce(self.fwd, fs, "allreduce:" + L.name, lane)
        self.fwd.add(lib.zsg_bn_sync_fwd_finalize, fs, L.c, mean, invstd, rm, rv, 0.1, 1e-5, what="stats:" + L.name, lane=lane)

    def P(self, name):      # raw parameter storage
        return self.net.store.raw(name)

    def G(self, name):
        """gradient storage of a parameter; remembers the last backward launch that writes it (bucket readiness)"""
        self.grad_ready[name] = len(self.bwd.calls)
        return self.net.store.raw(name, self.net.store.grad)

    # ---- op lowering ---------------------------------------------------------------------------------------------
    def _tune(self, kind, fn, d, *a, **k):
        """autotune_conv + remember the descriptor: ops.refine_in_step may later switch its tile hint in place (ZSGNet.refine_tuning)"""
        r = autotune_conv(kind, fn, d, *a, **k)
        self._tunables.append(d)
        return r

    def _bf16_conv(self, d, src_buf, w_src: torch.Tensor, wC: int, wc0: int, out_buf, bias, add_src, what: str, lane: int = 0) -> bool:
        """Lower the convolution `d` to zsg_conv_igemm_bf16 when this is a bf16 eval plan and the library takes the descriptor (else
        False: the caller lowers the fp32 launch).  w_src: the fp32 OHWI weight (raw parameter storage or a folded copy) whose channel
        window [wc0, wc0 + d.C) of wC is packed to uint16 [N][taps][C8]; the job joins the plan's one pack launch and the image is
        filled once now, so that the tuner times real data."""
        if not self.bf16 or self.training:
            return False
        b16 = lambda t: t is not None and t.dtype == torch.bfloat16
        io = (1 if b16(src_buf) else 0) | (2 if b16(out_buf) else 0) | (4 if b16(add_src) else 0)      # SRC_BF16 | OUT_BF16 | ADD_BF16
        if self.act16:
            if not lib.zsg_conv_igemm_bf16_io_supported(_ct.byref(d), io):
                return False
        elif not lib.zsg_conv_igemm_bf16_supported(_ct.byref(d)):
            return False
        wp = self._fwd_image(d, w_src, wC, wc0)
        args = (src_buf, wp, out_buf, bias, add_src)
        if self.act16:
            self._tune("igemm", lib.zsg_conv_igemm_bf16_io, d, args + (io,), stream_ptr())
            self.fwd.add(lib.zsg_conv_igemm_bf16_io, d, *args, io, what=what + f"+bf16io{io}", lane=lane)
            return True
        self._tune("igemm", lib.zsg_conv_igemm_bf16, d, args, stream_ptr())
        self.fwd.add(lib.zsg_conv_igemm_bf16, d, *args, what=what + "+bf16", lane=lane)
        return True

    def _pack_image(self, src_ptr: int, N: int, T: int, wC: int, wc0: int, C: int):
        """A packed bf16 weight image uint16 [N][T][C8] of the channel window [wc0, wc0 + C) of the fp32 image [N][T][wC] at src_ptr,
        filled once now so that the tuner times real data.  Returns (image, its zsg_pack_w_bf16_batched job without blk0, its blocks)."""
        c8 = (C + 7) // 8 * 8
        wp = self._buf(N * T * c8, dtype=torch.int16)
        job = (src_ptr, wp.data_ptr(), N, T, wC, wc0, C, c8)
        one = torch.frombuffer(bytearray(_struct.pack("<qqiiiiiiii", *job, 0, 0)), dtype=torch.uint8).to(self.dev)
        nblk = (N * T * c8 // 8 + 255) // 256
        check(lib.zsg_pack_w_bf16_batched(one.data_ptr(), 1, nblk, stream_ptr()), "pack_w_bf16")
        torch.cuda.current_stream().synchronize()          # (`one` is freed on return)
        return wp, job, nblk

    def _fwd_image(self, d, w_src: torch.Tensor, wC: int, wc0: int) -> torch.Tensor:
        """the packed image of a forward convolution's weight; its job joins the plan's one forward pack launch"""
        T = d.wR * d.wS
        assert wc0 + d.C <= wC and w_src.numel() >= d.N * T * wC
        wp, job, nblk = self._pack_image(w_src.data_ptr(), d.N, T, wC, wc0, d.C)
        self.pack_jobs.append(job + (self.pack_blocks, 0))
        self.pack_blocks += nblk
        self.pack_keep.append(w_src)
        return wp

    def _b16_eligible(self, lname: str) -> bool:
        """train_dtype = "bf16_head" covers the layer, forward AND data gradient: a convolution of the pyramid or of a head stack (never
        backbone.encoder.*)"""
        return self.train_bf16 and lname.startswith(BF16_HEAD_PREFIXES)

    def _enc_eligible(self, L: ConvL) -> bool:
        """enc_dtype = "bf16_fwd" covers the layer, FORWARD only (the data gradient asks _b16_eligible): an encoder convolution behind
        the stem"""
        return self.enc_bf16 and L.name.startswith(BF16_ENC_PREFIX) and not L.merge_x

    def _encb_eligible(self, L: ConvL) -> bool:
        """enc_bwd_dtype = "bf16" covers the layer's DATA GRADIENT: an encoder convolution behind the stem"""
        return self.encb_bf16 and L.name.startswith(BF16_ENC_PREFIX) and not L.merge_x

    def _enc_fwd(self, L: ConvL, d, src: Act, out: Act, wt: torch.Tensor, bias, relu: bool, bn_fuse: Optional[BnL]):
        """Lower the forward convolution of a covered encoder layer on bf16 MFMA.  Returns (launched, partials): (False, None) where the
        layer is not covered or the library refuses (the caller lowers fp32); (True, None) behind a plain zsg_conv_igemm_bf16 launch (no
        batch statistics needed); (True, the partial-row buffer) behind a zsg_conv_igemm_bf16_bn launch, with out.bn_chunks set (the
        caller continues with _conv_after).  Never raises: whatever does not fit falls back."""
        no = (False, None)
        if not self._enc_eligible(L):
            return no
        stats = bn_fuse is not None and not L.bias and not relu
        if bn_fuse is not None and not stats:
            return no                    # (a BatchNorm behind a bias or a ReLU: no such layer in a ResNet; fp32 serves it)
        if stats:
            rows = sum(src.B * d.seg[i].rows_y * d.seg[i].rows_x for i in range(d.nseg))
            rows64 = sum((src.B * d.seg[i].rows_y * d.seg[i].rows_x + 63) // 64 for i in range(d.nseg))
            if not lib.zsg_conv_igemm_bf16_bn_supported(_ct.byref(d)) or rows64 * 2 * L.cout * 4 > self.ws_bytes:
                return no                # (statistics needed and no room / no kernel for them: the fp32 lowering)
            wp = self._fwd_image(d, wt, L.cpad, 0)
            partials = self._ws_now()    # (the tuner's trials write at most the BM = 64 rows)
            # autotune_conv, NOT self._tune: this descriptor must stay out of _tunables — ops.refine_in_step switches tile hints in place,
            # and another BM would leave out.bn_chunks (and the bn_inline / stats: choice made from it below) stale
            autotune_conv("igemm", lib.zsg_conv_igemm_bf16_bn, d, (src.buf, wp, out.buf, partials), stream_ptr())
            chunks = int(lib.zsg_conv_igemm_bf16_partial_rows(_ct.byref(d)))
            assert 0 < chunks <= rows64 and rows > 0
            out.bn_chunks = chunks
            self.fwd.add(lib.zsg_conv_igemm_bf16_bn, d, src.buf, wp, out.buf, partials, what=L.name + "+bf16bn", lane=self._lane)
            res = (True, partials)
        else:
            if not lib.zsg_conv_igemm_bf16_supported(_ct.byref(d)):
                return no
            wp = self._fwd_image(d, wt, L.cpad, 0)
            args = (src.buf, wp, out.buf, bias, None)
            self._tune("igemm", lib.zsg_conv_igemm_bf16, d, args, stream_ptr())
            self.fwd.add(lib.zsg_conv_igemm_bf16, d, *args, what=L.name + "+bf16", lane=self._lane)
            out.bn_chunks = 0
            res = (True, None)
        self._b16_log.append(dict(kind="enc_fwd", what=L.name, idx=-1, call=self.fwd.calls[-1], d=type(d).from_buffer_copy(d), src=src,
                                  out=out, add=None, mask=None, pname=L.name + ".weight", window=(0, d.C),
                                  bn=None, frozen=None, mean=None, invstd=None))
        out._enc_log = self._b16_log[-1]
        return res

    def _bf16_train_fwd(self, lname: str, d, src: Act, w_src: torch.Tensor, wC: int, wc0: int, out: Act, bias, add: Optional[Act], what: str,
                        lane: int = 0) -> bool:
        """Lower the forward convolution `d` of layer `lname` to zsg_conv_igemm_bf16 when this is a bf16_head training plan, the layer
        is covered and the library takes the descriptor (else False: the caller lowers the fp32 launch, Winograd candidates included).
        The weight is the RAW parameter (training has no BatchNorm fold); activations stay fp32 in memory."""
        if not self._b16_eligible(lname) or not lib.zsg_conv_igemm_bf16_supported(_ct.byref(d)):
            return False
        wp = self._fwd_image(d, w_src, wC, wc0)
        args = (src.buf, wp, out.buf, bias, add.buf if add is not None else None)
        self._tune("igemm", lib.zsg_conv_igemm_bf16, d, args, stream_ptr())
        self.fwd.add(lib.zsg_conv_igemm_bf16, d, *args, what=what + "+bf16", lane=lane)
        self._b16_log.append(dict(kind="fwd", what=what, idx=-1, call=self.fwd.calls[-1], d=type(d).from_buffer_copy(d), src=src, out=out,
                                  add=add, mask=None, pname=lname + ".weight", window=(wc0, d.C)))
        return True

    def _wino_u(self, src_ptr: int, N: int, Cred: int, row_ld: int, tap_ld: int, flip: int):
        """Transformed filter image of one 3x3 convolution (+ a one-off transform so that the tuner times real data);
        the job joins the program's batched transform only if the Winograd kernel wins the tuning."""
        # (not a plan buffer: when the direct kernel wins the tuning nobody keeps a reference and the image is freed; a Winograd
        # launch keeps it alive through its program's argument list.  The transform writes every element, padding included.)
        U = torch.empty(int(lib.zsg_wino_u_elems(Cred, N)), dtype=torch.float32, device=self.dev)
        job = (src_ptr, U.data_ptr(), N, Cred, row_ld, tap_ld, flip)
        one = WinoJobs()
        one.add(*job)
        one.finish(self.dev)
        one.launch(stream_ptr())
        return U, job

    def _ws_now(self):
        """BatchNorm / statistics workspace of the lane being lowered (forward launches on the side stream run concurrently
        with the main stream's, so they get their own)"""
        return self.ws if self._lane == 0 else self.ws_side

    def _join_side(self):
        """the main stream waits for everything lowered on the side stream so far (an empty lane-2 launch)"""
        if self.training:
            self.fwd.add(lib.zsg_memset_f32, self.ws, 0, 0.0, what="join side stream", lane=2)

    def on_side_stream(self):
        """context: forward launches lowered inside go to the side HIP stream (lane 1: each waits for everything enqueued
        on the main stream before it); the consumer of their results must be lowered with join=True (lane 2)."""
        import contextlib

        @contextlib.contextmanager
        def cm():
            if not self.training:          # (eval plans are short chains of folded convolutions: keep one stream)
                yield
                return
            keep, self._lane = self._lane, 1
            try:
                yield
            finally:
                self._lane = keep
        return cm()

    @staticmethod
    def _wino_chunks(d, B: int) -> int:
        tb = d.tile_hint & 0xff
        return sum((B * ((d.seg[i].src_H + 1) // 2) * ((d.seg[i].src_W + 1) // 2) + tb - 1) // tb for i in range(d.nseg))

    def conv(self, L: ConvL, src: Act, relu=False, out: Optional[Act] = None, name=None, bn_fuse: Optional[BnL] = None) -> Act:
        """bn_fuse: the output feeds a train-mode BatchNorm — let the epilogue emit the per-tile (sum, sum^2) partials
        (no extra pass over the activation) unless the autotuner chose split-K for this layer."""
        if out is None:
            lv = src.levels
            assert len(lv) == 1
            out = self.act(name or L.name, src.B, conv_out(lv[0].H, L.k, L.stride, L.pad, L.dil),
                           conv_out(lv[0].W, L.k, L.stride, L.pad, L.dil), L.cout, dtype=torch.float32 if L.merge_x else self.adt)
        d = fwd_desc(src, out, L.cpad, L.cout, L.k, L.stride, L.pad, L.dil, wC=L.cpad, relu=relu, merge_x=L.merge_x)
        bias = self.P(L.name + ".bias") if L.bias else None
        rd = src
        ig_fn, wn_fn = lib.zsg_conv_igemm, lib.zsg_conv_wino
        pend = getattr(src, "pending", None)
        if self.bn_frozen(bn_fuse) and pend is None:
            bn_fuse = None                 # a frozen BatchNorm normalises with its running statistics: no fused batch statistics
        # a split-K choice would cost this layer its fused BatchNorm statistics: a statistics pass over the output at
        # ~4 TB/s plus two more dependent launches
        pen = 0.0
        if bn_fuse is not None and self.training and not L.bias and not relu:
            pen = 0.008 + out.rows() * L.cout * 4 / 4e9
        wt = self.P(L.name + ".weight")
        if pend is not None:
            return self._conv_bnpre(L, src, out, d, wt, pend, bn_fuse)
        if self._bf16_train_fwd(L.name, d, src, wt, L.cpad, 0, out, bias, None, L.name, lane=self._lane):
            # (train_dtype = "bf16_head": the tape entry, needs_mask, requires_grad and the lane are the fp32 lowering's below)
            assert bn_fuse is None, "a convolution in front of a BatchNorm is not a bf16_head layer"
            out.bn_chunks, out.bn_inline, out.needs_mask, out.requires_grad = 0, None, relu, self._conv_rg(L, src)
            completes = getattr(src, "bn_out", False) and not getattr(src, "_consumed", False)
            src._consumed = True
            self.tape.append(lambda: self._conv_bwd(L, src, out, completes_bn=completes))
            return out
        if self._bf16_conv(d, rd.buf, wt, L.cpad, 0, out.buf, bias, None, L.name, lane=self._lane):
            # (an eval plan has no backward: the tape entry only keeps the callers' bookkeeping — _head_stack pops it — in step)
            out.bn_chunks, out.bn_inline, out.needs_mask, out.requires_grad = 0, None, relu, self._conv_rg(L, src)
            src._consumed = True
            self.tape.append(lambda: None)
            return out
        if src.b16 or out.b16:
            # bf16_act, a convolution the bf16 entry refuses: the fp32 lowering between casts
            s32, o32, _, finish = self._via_f32(src, out, lane=self._lane)
            self.conv(L, s32, relu=relu, out=o32, bn_fuse=bn_fuse)
            finish()
            out.bn_chunks, out.bn_inline, out.needs_mask, out.requires_grad = 0, None, relu, o32.requires_grad
            return out
        # enc_dtype = "bf16_fwd": a covered encoder convolution on bf16 MFMA; what follows the launch (the statistics branches, the tape
        # entry: the fp32 lowering's backward) is _conv_after, shared with the fp32 launch below
        launched, partials = self._enc_fwd(L, d, src, out, wt, bias, relu, bn_fuse)
        if launched:
            return self._conv_after(L, d, src, out, relu, bn_fuse, partials)
        wargs = None
        if wino_ok(L.k, L.stride, L.pad, L.dil) and not L.merge_x and wino_mode() != "0":
            U, job = self._wino_u(wt.data_ptr(), L.cout, L.cpad, L.k * L.k * L.cpad, L.cpad, 0)
            wargs = (rd.buf, U, out.buf, bias, None, None, None)
        self._tune("igemm", ig_fn, d, (rd.buf, wt, out.buf, bias, None, None, None), stream_ptr(),
                      split_penalty_ms=pen, wino_args=wargs, wino_fn=wn_fn)
        fn = ig_fn
        if d.use_wino:
            fn, wt = wn_fn, U
            self.wino_jobs["fwd"].add(*job)
        partials = None
        out.bn_chunks = 0
        if bn_fuse is not None and self.training and d.tile_hint and ((d.tile_hint >> 16) & 0xff) <= 1 and not L.bias and not relu:
            if d.use_wino:
                chunks = self._wino_chunks(d, src.B)
            else:
                chunks = igemm_partial_rows(d)
            if chunks * 2 * L.cout * 4 <= self.ws_bytes:
                partials, out.bn_chunks = self._ws_now(), chunks
        pre_zero = None
        if self._side_prep and ((d.tile_hint >> 16) & 0xff) > 1 and len(out.levels) == 1:
            # split-K: the K slices are added with atomics to a ZEROED output.  The zero-fill (a dependent ~6 us launch in front of the
            # convolution when the library issues it) goes to the side-stream preparation instead — nobody reads this buffer between
            # the previous step's backward and this launch — and the convolution is told to accumulate onto its own output.
            lv0 = out.levels[0]
            self.prep_u.add(lib.zsg_memset_f32, out.buf[lv0.off:], out.B * lv0.bstride, 0.0, what="zero:" + L.name)
            pre_zero = out.buf
        tail_n = -1
        if partials is not None and not self.bn_synced(bn_fuse):
            # BatchNorm statistics FINALISED by the last-arriving tile of the convolution (csrc/bn_tail.h, round 5): no finalize launch, no
            # re-reduction in the apply pass, wherever the launch has <= 128 partial rows per column block (tail_n > 0)
            tail_n = int(lib.zsg_conv_bn_tail_tickets(_ct.byref(d), 1 if d.use_wino else 0))
        if tail_n > 0:
            # the convolution's last tile per column block finalises the statistics itself (mean / invstd / running statistics are ready
            # when the launch ends): the plain apply launch follows, nothing in between
            Lb = bn_fuse
            tk = self._buf(tail_n, dtype=torch.int32)
            out.bn_mean, out.bn_invstd = self._buf(Lb.c), self._buf(Lb.c)
            rm, rv = self.net._rm[Lb.index:Lb.index + Lb.c], self.net._rv[Lb.index:Lb.index + Lb.c]
            self.fwd.add(lib.zsg_conv_wino_bnstat if d.use_wino else lib.zsg_conv_igemm_bnstat, d, rd.buf, wt, out.buf, partials, tk,
                         out.bn_mean, out.bn_invstd, rm, rv, 0.1, 1e-5, what=L.name + "+bnstat", lane=self._lane)
        else:
            self.fwd.add(fn, d, rd.buf, wt, out.buf, bias, pre_zero, None, partials, what=L.name, lane=self._lane)
        if pre_zero is not None:
            self._zero_calls.append(self.fwd.calls[-1])
        return self._conv_after(L, d, src, out, relu, bn_fuse, None if tail_n > 0 else partials)

    def _conv_after(self, L: ConvL, d, src: Act, out: Act, relu: bool, bn_fuse: Optional[BnL], partials) -> Act:
        """What conv() lowers behind its launch.  partials: the rows (out.bn_chunks of them) the launch wrote for bn_fuse WITHOUT finalising
        them, or None (no fused statistics, or finalised in the kernel).  Then the bookkeeping and the tape entry."""
        out.bn_inline = None
        if partials is None:
            pass
        elif self.bn_synced(bn_fuse):
            # synchronized statistics from the partial rows, at once (the shared workspace is reused by the next launch)
            rows = sum(src.B * d.seg[i].rows_y * d.seg[i].rows_x for i in range(d.nseg))
            out.bn_mean, out.bn_invstd = self._buf(bn_fuse.c), self._buf(bn_fuse.c)
            self._sync_fwd_stats(bn_fuse, None, rows, partials, out.bn_chunks, out.bn_mean, out.bn_invstd, self._lane)
        elif out.bn_chunks <= lib.zsg_bn_inline_max_chunks():
            # few partial rows: the BatchNorm apply launch (the very next launch on this stream: the workspace is still intact)
            # reduces them itself — no finalize launch
            out.bn_inline = partials
            out.bn_mean, out.bn_invstd = self._buf(bn_fuse.c), self._buf(bn_fuse.c)
        else:                              # finalize at once: the shared workspace is reused by the next launch
            Lb = bn_fuse
            rows = sum(src.B * d.seg[i].rows_y * d.seg[i].rows_x for i in range(d.nseg))
            out.bn_mean, out.bn_invstd = self._buf(Lb.c), self._buf(Lb.c)
            rm, rv = self.net._rm[Lb.index:Lb.index + Lb.c], self.net._rv[Lb.index:Lb.index + Lb.c]
            self.fwd.add(lib.zsg_bn_stats_from_partials, partials, out.bn_chunks, rows, Lb.c, out.bn_mean, out.bn_invstd, rm, rv, 0.1, 1e-5,
                         what="stats:" + Lb.name, lane=self._lane)
        out.needs_mask = relu
        out.requires_grad = self._conv_rg(L, src)
        # the first consumer lowered is the LAST to add to src's gradient in the backward: if src is a train-mode BatchNorm's
        # output, that data gradient completes the BatchNorm's dout and can carry its backward sums (see bn())
        completes = self.training and getattr(src, "bn_out", False) and not getattr(src, "_consumed", False)
        src._consumed = True
        self.tape.append(lambda: self._conv_bwd(L, src, out, completes_bn=completes))
        return out

    def _conv_bnpre(self, L: ConvL, src: Act, out: Act, d, wt, pend, bn_fuse: Optional[BnL]) -> Act:
        """conv() for a source whose closing BatchNorm + residual + ReLU is still pending (bn(defer=True)): this 1x1 convolution applies
        it in its operand loader and writes the activation (src.buf) and its ReLU bits itself — zsg_conv_igemm_bnpre.  Everything
        behind the launch (this convolution's own fused statistics, the tape) is conv()'s."""
        assert self.training and L.k == 1 and L.stride == 1 and L.pad == 0 and not L.bias and bn_fuse is not None and len(src.levels) == 1, \
            "a deferred BatchNorm apply needs a plain 1x1 consumer in front of a BatchNorm"
        x = pend["x"]
        fn = lib.zsg_conv_igemm_bnpre
        pre = (pend["mean"], pend["invstd"], pend["gam"], pend["bet"], pend["residual"].buf, src.buf, pend["rmask"])
        self._tune("igemm", fn, d, (x.buf, wt, out.buf, None, None, None, None, None, None, 0.1, 1e-5) + pre, stream_ptr())
        h = d.tile_hint
        admissible = (h and ((h >> 16) & 0xff) <= 1 and (h & 0xff) in (64, 128) and not (h >> 27) & 1 and not (h >> 28) & 3
                      and not ((h & 0xffff) == 0x8080 and not (h >> 24) & 1))
        if not admissible:
            # no tuner (ZSG_AUTOTUNE=0, heuristic hint 0) or a cached / shipped entry the BatchNorm-applying loader has no variant for
            # (split-K, 64-deep K tiles, stream-K, the streaming 1x1 kernel, the 4-wave 128x128 tile): the 64x64 tile always applies —
            # lowering must not crash on a table it did not make
            d.tile_hint = tile_hint(64, 64, 1)
        lane = 2 if pend["join"] else self._lane
        Lb = bn_fuse
        out.bn_inline = None
        what = L.name + "+bnpre(" + pend["name"] + ")"
        if self.bn_frozen(Lb):
            # (the BatchNorm behind this convolution is frozen: no statistics of the output, the loader still applies the pending one)
            out.bn_chunks = 0
            self.fwd.add(fn, d, x.buf, wt, out.buf, None, None, None, None, None, None, 0.1, 1e-5, *pre, what=what, lane=lane)
            src.pending = None
            out.needs_mask = False
            out.requires_grad = self._conv_rg(L, src)
            completes = self.training and getattr(src, "bn_out", False) and not getattr(src, "_consumed", False)
            src._consumed = True
            self.tape.append(lambda: self._conv_bwd(L, src, out, completes_bn=completes))
            return out
        chunks = igemm_partial_rows(d)
        assert chunks * 2 * L.cout * 4 <= self.ws_bytes
        partials, out.bn_chunks = self._ws_now(), chunks
        sync = self.bn_synced(Lb)
        tail_n = int(lib.zsg_conv_bn_tail_tickets(_ct.byref(d), 0)) if not sync else 0
        rm, rv = self.net._rm[Lb.index:Lb.index + Lb.c], self.net._rv[Lb.index:Lb.index + Lb.c]
        if sync:
            # (no tickets: the partial rows stop at the rank-local sums, finalised from the all-reduced ones)
            self.fwd.add(fn, d, x.buf, wt, out.buf, partials, None, None, None, None, None, 0.1, 1e-5, *pre, what=what, lane=lane)
            out.bn_mean, out.bn_invstd = self._buf(Lb.c), self._buf(Lb.c)
            self._sync_fwd_stats(Lb, None, src.B * d.seg[0].rows_y * d.seg[0].rows_x, partials, out.bn_chunks, out.bn_mean, out.bn_invstd,
                                 self._lane)
        elif tail_n > 0:
            tk = self._buf(tail_n, dtype=torch.int32)
            out.bn_mean, out.bn_invstd = self._buf(Lb.c), self._buf(Lb.c)
            self.fwd.add(fn, d, x.buf, wt, out.buf, partials, tk, out.bn_mean, out.bn_invstd, rm, rv, 0.1, 1e-5, *pre, what=what + "+bnstat", lane=lane)
        else:
            self.fwd.add(fn, d, x.buf, wt, out.buf, partials, None, None, None, None, None, 0.1, 1e-5, *pre, what=what, lane=lane)
            out.bn_mean, out.bn_invstd = self._buf(Lb.c), self._buf(Lb.c)
            if out.bn_chunks <= lib.zsg_bn_inline_max_chunks():
                out.bn_inline = partials
            else:
                rows = src.B * d.seg[0].rows_y * d.seg[0].rows_x
                self.fwd.add(lib.zsg_bn_stats_from_partials, partials, out.bn_chunks, rows, Lb.c, out.bn_mean, out.bn_invstd, rm, rv, 0.1, 1e-5,
                             what="stats:" + Lb.name, lane=self._lane)
        src.pending = None
        out.needs_mask = False
        out.requires_grad = self._conv_rg(L, src)
        completes = self.training and getattr(src, "bn_out", False) and not getattr(src, "_consumed", False)
        src._consumed = True
        self.tape.append(lambda: self._conv_bwd(L, src, out, completes_bn=completes))
        return out

    def conv_bn(self, L: ConvL, Lb: BnL, x: Act, relu: bool, residual: Optional[Act] = None, name=None, yname=None) -> Act:
        """conv -> BatchNorm [-> + residual] [-> ReLU].  Training: the two lowered ops (batch statistics from the conv
        epilogue).  Eval: ONE convolution with the BatchNorm folded into its weights / bias (zsg_bn_fold refreshes the
        folded copies at the start of every eval forward), residual add and ReLU in its epilogue."""
        if self.training:
            y = self.conv(L, x, name=yname or (L.name + ".y"), bn_fuse=Lb)
            return self.bn(Lb, y, relu, residual=residual, name=name)
        net = self.net
        n_w = L.cout * L.k * L.k * L.cpad
        w_off = self.fold_used
        b_off = w_off + (n_w + 3) // 4 * 4
        self.fold_used = b_off + (L.cout + 3) // 4 * 4
        assert self.fold_used <= self.fold_arena.numel(), "BN-fold arena too small"
        ents = net.store.entries
        self.fold_jobs.append((ents[L.name + ".weight"].offset, w_off, ents[Lb.name + ".weight"].offset, ents[Lb.name + ".bias"].offset,
                               b_off, self.fold_rows, L.cout, L.k * L.k * L.cpad, Lb.index))
        self.fold_rows += L.cout
        lv = x.levels[0]
        out = self.act(name or Lb.name, x.B, conv_out(lv.H, L.k, L.stride, L.pad, L.dil), conv_out(lv.W, L.k, L.stride, L.pad, L.dil), L.cout,
                       dtype=torch.float32 if L.merge_x else self.adt)       # (the stem convolution's output stays fp32)
        d = fwd_desc(x, out, L.cpad, L.cout, L.k, L.stride, L.pad, L.dil, wC=L.cpad, relu=relu, merge_x=L.merge_x)
        wt, bias = self.fold_arena[w_off:w_off + n_w], self.fold_arena[b_off:b_off + L.cout]
        args = (x.buf, wt, out.buf, bias, residual.buf if residual is not None else None, None, None)
        if self._bf16_conv(d, x.buf, wt, L.cpad, 0, out.buf, bias, args[4], L.name + "+bn"):
            return out
        if x.b16 or out.b16 or (residual is not None and residual.b16):
            # bf16_act, a convolution the bf16 entry refuses: the fp32 launch below between casts
            x32, o32, r32, finish = self._via_f32(x, out, residual)
            args = (x32.buf, wt, o32.buf, bias, r32.buf if r32 is not None else None, None, None)
            x, real_out, out = x32, out, o32
        else:
            real_out, finish = out, (lambda: None)
        wargs = None
        if wino_ok(L.k, L.stride, L.pad, L.dil) and not L.merge_x and wino_mode() != "0":
            U, job = self._wino_u(wt.data_ptr(), L.cout, L.cpad, L.k * L.k * L.cpad, L.cpad, 0)
            wargs = (x.buf, U) + args[2:]
        self._tune("igemm", lib.zsg_conv_igemm, d, args, stream_ptr(), wino_args=wargs)
        if d.use_wino:
            self.wino_jobs["fwd"].add(*job)
            self.fwd.add(lib.zsg_conv_wino, d, *wargs, what=L.name + "+bn")
        else:
            self.fwd.add(lib.zsg_conv_igemm, d, *args, what=L.name + "+bn")
        finish()
        return real_out

    def _wt(self, L: ConvL, cred: int) -> torch.Tensor:
        """transposed weight image [cpad][k*k][cred] for the data gradient (a slice of one arena); all images are
        refreshed by ONE batched transpose launch at the start of backward (built in _finish_prep)"""
        if L.name not in self.wt:
            n = L.cpad * L.k * L.k * cred
            off = self.wt_arena_used
            self.wt_arena_used += (n + 3) // 4 * 4
            assert self.wt_arena_used <= self.wt_arena.numel(), "dgrad weight arena too small"
            self.wt[L.name] = self.wt_arena[off:off + n]
            e = self.net.store.entries[L.name + ".weight"]
            self.wt_jobs.append((e.offset, off, L.cout, L.k * L.k, L.cpad, cred))
            # fill the image once now: the autotuner that follows times the data gradient (and the Winograd filter transform) on real
            # weights, not on the arena's zeros (zero operands clock ~20 % higher: MI355X_MICROARCH.md, DVFS)
            check(lib.zsg_transpose_w(self.net.store.flat.data_ptr() + 4 * e.offset, self.wt[L.name].data_ptr(), L.cout, L.k * L.k, L.cpad, cred,
                                      stream_ptr()), "transpose_w")
        return self.wt[L.name]

    def _finish_prep(self):
        import struct
        if not self.wt_jobs:
            return
        blob, tile0 = b"", 0
        for (so, do, N, T, Cc, ld) in self.wt_jobs:
            tc, tn = (Cc + 63) // 64, (ld + 63) // 64          # 64 x 64 tiles (csrc/misc.hip transpose_w_batched_kernel)
            assert Cc % 4 == 0 and ld % 4 == 0 and so % 4 == 0 and do % 4 == 0
            blob += struct.pack("<qqiiiiiiii", so, do, N, T, Cc, ld, tile0, tc, tn, 0)
            tile0 += T * tc * tn
        self.wt_jobs_dev = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(self.dev)
        self.prep.add(lib.zsg_transpose_w_batched, self.net.store.flat, self.wt_arena, self.wt_jobs_dev, len(self.wt_jobs), tile0,
                      what="transpose all dgrad weight images")
        if self.dpack_jobs:      # train_dtype = "bf16_head": the packed bf16 copies of the transposed images the bf16 data gradients read
            blob = b"".join(_struct.pack("<qqiiiiiiii", *j) for j in self.dpack_jobs)
            self.dpack_jobs_dev = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(self.dev)
            self.prep.add(lib.zsg_pack_w_bf16_batched, self.dpack_jobs_dev, len(self.dpack_jobs), self.dpack_blocks,
                          what="pack bf16 dgrad weight images")
        wj = self.wino_jobs["bwd"]
        if wj.jobs:          # rotated filter transforms of the Winograd data gradients, from the transposed images
            self.prep.add(lib.zsg_wino_weights, wj.finish(self.dev), len(wj.jobs), wj.blocks, what="wino dgrad filter transforms")

    def _conv_rg(self, L: ConvL, src: Act) -> bool:
        """a convolution's output needs a gradient when its input does or one of its own parameters trains"""
        return src.requires_grad or self.trains(L.name + ".weight") or (L.bias and self.trains(L.name + ".bias"))

    def _conv_bwd(self, L: ConvL, src: Act, out: Act, dy: Optional[Act] = None, completes_bn: bool = False):
        dy = dy or out.grad
        if dy is None:
            return
        if self.trains(L.name + ".weight"):
            dw = fwd_desc(src, dy, L.cpad, L.cout, L.k, L.stride, L.pad, L.dil, wC=L.cpad)
            self.wgrad(dw, src, dy, L.name + ".weight", "wgrad:" + L.name, merge_x=L.merge_x)
        if L.bias and self.trains(L.name + ".bias"):
            base = dy.levels[0].off
            self.bwd.add(lib.zsg_colsum, dy.buf[base:], 1, 0, dy.rows(), dy.ld, 0, L.cout, self.G(L.name + ".bias"), 1,
                         what="bgrad:" + L.name, lane=1)
        if src.requires_grad:
            self.dgrad(L, dy, src, n=L.cpad, completes_bn=completes_bn)

    def wgrad(self, d, src: Act, dy: Act, pname: str, what: str, merge_x: bool = False):
        """weight gradient of one parameter, accumulated into the flat gradient buffer (every parameter has exactly one
        wgrad launch per backward; the shared head's pyramid levels are segments of that one launch).  The autotuner's
        trial launches write a scratch image, never the gradient buffer.  merge_x: the layer's forward descriptor is a merge_x one (the
        network's first convolution, C = 4) — the weight-gradient descriptor does not carry the flag, the bf16 entry is asked with it."""
        gw = self.G(pname)
        args = (src.buf, dy.buf, gw, 1, self.wg_ws, self.wg_ws_bytes)
        targs = (src.buf, dy.buf, self.tune_dw, 0, self.wg_ws, self.wg_ws_bytes)
        s0 = d.seg[0]
        wino = (d.wR == 3 and d.wS == 3 and s0.sy == 1 and s0.ty.d0 == -1 and s0.ty.dstep == 1 and not d.merge_x
                and dy.ld % 4 == 0 and wino_mode() != "0")       # 3x3 / stride 1 / pad 1: Winograd F(3x3,2x2) candidates
        if self.wgrad_bf16 and self._wgrad_bf16_ok(d, merge_x):
            # wgrad_dtype = "bf16": the same launch on bf16 MFMA (one direct kernel for 1x1 and 3x3: no Winograd candidates)
            self._tune("wgrad", lib.zsg_conv_wgrad_bf16, d, targs, stream_ptr(), self.wg_ws_bytes)
            self.bwd.add(lib.zsg_conv_wgrad_bf16, d, *args, what=what + "+bf16", lane=1)
            self._wg_log.append((len(self.bwd.calls) - 1, d, src, dy, gw, pname, what + "+bf16"))
            return
        self._tune("wgrad", lib.zsg_conv_wgrad, d, targs, stream_ptr(), self.wg_ws_bytes, wino_args=targs if wino else None)
        self.bwd.add(lib.zsg_conv_wgrad_wino if d.use_wino else lib.zsg_conv_wgrad, d, *args, what=what, lane=1)
        self._wg_log.append((len(self.bwd.calls) - 1, d, src, dy, gw, pname, what))

    @staticmethod
    def _wgrad_bf16_ok(d, merge_x: bool = False) -> bool:
        """zsg_conv_wgrad_bf16_supported on the convolution's descriptor with the forward descriptor's merge_x flag"""
        dq = type(d).from_buffer_copy(d)
        dq.merge_x = int(bool(merge_x))
        return bool(lib.zsg_conv_wgrad_bf16_supported(_ct.byref(dq)))

    def dgrad(self, L: ConvL, dy: Act, src: Act, n: int, row0: int = 0, dx: Optional[Act] = None, completes_bn: bool = False):
        """dx (+)= dgrad(dy) for input channels [row0, row0+n) of L; applies src's ReLU mask when required."""
        cred = dy.ld
        assert cred % 4 == 0
        wt = self._wt(L, cred)
        dx = dx or self.grad_of(src)
        d = dgrad_desc(dy, dx, cred, n, L.k, L.stride, L.pad, L.dil)
        wt_off = row0 * L.k * L.k * cred
        if d.zero_fill and not dx.gfilled:      # stride-parity classes without taps get no launch: clear them
            # (a gradient buffer is idle from the previous step's optimizer update until this backward: with the side-stream
            # preparation on, the fill runs there during the forward instead of on the backward's dependent chain)
            (self.prep if self._side_prep else self.bwd).add(lib.zsg_memset_f32, self.base(dx), sum(dx.B * l.H * l.W * dx.ld for l in dx.levels), 0.0,
                                                             what="zero:" + L.name)
            dx.gfilled = True
        mask = None
        if src.needs_mask:
            # the epilogue indexes the mask with the OUTPUT offsets; dx may be a level of a packed buffer while src has
            # its own: rebase the pointer so that mask[o] == src[o - (dx_off - src_off)]
            deltas = {sl.off - dl.off for sl, dl in zip(src.levels, dx.levels)}
            assert len(deltas) == 1 and src.ld == dx.ld, "ReLU mask needs one common offset between src and its gradient"
            mask = src.buf.data_ptr() + 4 * deltas.pop()
            self.bwd.keep.append(src.buf)
        if self._b16_eligible(L.name) and not getattr(src, "bn_out", False) and lib.zsg_conv_igemm_bf16_m_supported(_ct.byref(d)):
            # train_dtype = "bf16_head": the same launch on bf16 MFMA, on the packed copy of the transposed image (one more pack launch in
            # prep, behind the transpose).  Not into a BatchNorm output (the laterals, P6): that data gradient completes the BatchNorm's
            # dout and may be re-issued with its backward sums in the epilogue, which the bf16 entry does not have.  No Winograd
            # candidates, no split-K (so no zero-fill beyond the one above)
            key = (L.name, row0, n)
            if key not in self._dpack:
                self._dpack[key], job, nblk = self._pack_image(wt.data_ptr() + 4 * wt_off, n, L.k * L.k, cred, 0, cred)
                self.dpack_jobs.append(job + (self.dpack_blocks, 0))
                self.dpack_blocks += nblk
            add = dx if dx.gfilled else None
            args = (dy.buf, self._dpack[key], dx.buf, None, dx.buf if dx.gfilled else None, mask)
            self._tune("igemm", lib.zsg_conv_igemm_bf16_m, d, args, stream_ptr())
            self.bwd.add(lib.zsg_conv_igemm_bf16_m, d, *args, what="dgrad:" + L.name + "+bf16")
            self._b16_log.append(dict(kind="dgrad", what="dgrad:" + L.name, idx=-1, call=self.bwd.calls[-1], d=type(d).from_buffer_copy(d),
                                      src=dy, out=dx, add=add, mask=src if mask is not None else None, pname=L.name + ".weight",
                                      window=(row0, n)))
            dx.gfilled = True
            dx.last_writer = None
            return
        if self._encb_eligible(L) and lib.zsg_conv_igemm_bf16_m_supported(_ct.byref(d)):
            # enc_bwd_dtype = "bf16": the same launch on bf16 MFMA, on the packed copy of the transposed image (the one extra pack launch in
            # prep that train_dtype has).  The strided (zero-filled) and the accumulating data gradients never carry a BatchNorm's sums; one
            # that completes a BatchNorm's dout is re-issued by _bnb_reissue as zsg_conv_igemm_bf16_bnb.  No Winograd candidates, no split-K.
            # autotune_conv, NOT self._tune: the partial-row count of the re-issued launch is baked into the BatchNorm backward behind it,
            # so ops.refine_in_step must not move this descriptor's tile hint afterwards (as in _enc_fwd)
            key = (L.name, row0, n)
            if key not in self._dpack:
                self._dpack[key], job, nblk = self._pack_image(wt.data_ptr() + 4 * wt_off, n, L.k * L.k, cred, 0, cred)
                self.dpack_jobs.append(job + (self.dpack_blocks, 0))
                self.dpack_blocks += nblk
            add = dx if dx.gfilled else None
            args = (dy.buf, self._dpack[key], dx.buf, None, dx.buf if dx.gfilled else None, mask)
            autotune_conv("igemm", lib.zsg_conv_igemm_bf16_m, d, args, stream_ptr())
            self.bwd.add(lib.zsg_conv_igemm_bf16_m, d, *args, what="dgrad:" + L.name + "+bf16")
            self._b16_log.append(dict(kind="enc_dgrad", what="dgrad:" + L.name, idx=-1, call=self.bwd.calls[-1], d=type(d).from_buffer_copy(d),
                                      src=dy, out=dx, add=add, mask=src if mask is not None else None, pname=L.name + ".weight",
                                      window=(row0, n), bn=None))
            dx.gfilled = True
            covers_all = not d.zero_fill and mask is None and d.tile_hint and dx.ld == n and n % 4 == 0
            # (the fifth field marks a bf16 launch: its _b16_log entry, which a re-issue completes)
            dx.last_writer = (len(self.bwd.calls) - 1, d, args, "dgrad:" + L.name + "+bf16", self._b16_log[-1]) if covers_all else None
            return
        args = (dy.buf, wt[wt_off:], dx.buf, None, dx.buf if dx.gfilled else None, mask, None)
        wargs = None
        if wino_ok(L.k, L.stride, L.pad, L.dil) and wino_mode() != "0":
            U, job = self._wino_u(wt.data_ptr() + 4 * wt_off, n, cred, L.k * L.k * cred, cred, 1)
            wargs = (dy.buf, U) + args[2:]
        # a split-K choice would cost the BatchNorm below its fused backward sums: a pass over dout and x plus a launch
        pen = (0.006 + 2 * dx.rows() * n * 4 / 4e9) if (completes_bn and BNB_FUSE and not d.zero_fill and mask is None) else 0.0
        self._tune("igemm", lib.zsg_conv_igemm, d, args, stream_ptr(), split_penalty_ms=pen, wino_args=wargs, allow_sk=False)
        if self._side_prep and ((d.tile_hint >> 16) & 0xff) > 1 and args[4] is None and len(dx.levels) == 1:
            # split-K into a gradient buffer nothing has written yet: its zero-fill moves to the side-stream preparation (see conv())
            lv0 = dx.levels[0]
            self.prep.add(lib.zsg_memset_f32, dx.buf[lv0.off:], dx.B * lv0.bstride, 0.0, what="zero:dgrad:" + L.name)
            args = args[:4] + (dx.buf,) + args[5:]
            if wargs is not None:
                wargs = wargs[:4] + (dx.buf,) + wargs[5:]
        if d.use_wino:
            self.wino_jobs["bwd"].add(*job)
            self.bwd.add(lib.zsg_conv_wino, d, *wargs, what="dgrad:" + L.name)
        else:
            self.bwd.add(lib.zsg_conv_igemm, d, *args, what="dgrad:" + L.name)
        dx.gfilled = True
        # If this launch turns out to be the one that COMPLETES a BatchNorm's dout (the BatchNorm's backward is lowered right
        # after it), its epilogue can also produce that BatchNorm's backward sums: remember how to re-issue it (see bn()).
        covers_all = not d.zero_fill and mask is None and ((d.tile_hint >> 16) & 0xff) <= 1 and d.tile_hint and dx.ld == n and n % 4 == 0
        dx.last_writer = (len(self.bwd.calls) - 1, d, wargs if d.use_wino else args, "dgrad:" + L.name) if covers_all else None

    def bn(self, L: BnL, x: Act, relu: bool, residual: Optional[Act] = None, name=None, join: bool = False, defer: bool = False) -> Act:
        """join: an operand (the residual) was produced on the side stream — the apply launch first joins it (lane 2).
        defer: no apply launch — the one consumer lowered next (a 1x1 convolution, conv()) applies this BatchNorm in its operand loader
        and materialises the activation (out.pending describes it)."""
        net = self.net
        lv = x.levels[0]
        out = self.act(name or L.name, x.B, lv.H, lv.W, L.c)
        # (frozen gamma / beta with an input that needs a gradient: the backward still writes d(gamma) / d(beta) into the flat gradient
        # buffer as a by-product of the fused kernels; those ranges are never exposed as p.grad, reduced or stepped)
        out.requires_grad = (x.requires_grad or self.trains(L.name + ".weight") or self.trains(L.name + ".bias")
                             or (residual is not None and residual.requires_grad))
        rows = x.B * lv.H * lv.W
        frozen = self.bn_frozen(L)
        fused = self.training and getattr(x, "bn_chunks", 0) > 0
        assert not (frozen and fused), "a frozen BatchNorm's producer must not compute batch statistics"
        if frozen:
            mean, invstd = self._eval_stats(L)
        else:
            mean, invstd = (x.bn_mean, x.bn_invstd) if fused else (self._buf(L.c), self._buf(L.c))
        if getattr(x, "_enc_log", None) is not None:       # (enc_dtype = "bf16_fwd": the statistics this convolution's output is normalised with)
            x._enc_log.update(bn=L.name, frozen=frozen, mean=mean, invstd=invstd)
        rm, rv = net._rm[L.index:L.index + L.c], net._rv[L.index:L.index + L.c]
        self.ws_need = max(getattr(self, "ws_need", 0), lib.zsg_bn_workspace_bytes(rows, L.c))
        gam, bet = self.P(L.name + ".weight"), self.P(L.name + ".bias")
        sync = self.bn_synced(L)
        if fused or frozen:
            pass                          # statistics were finalized right after the producing convolution / are the running ones
        elif sync:
            self._sync_fwd_stats(L, x.buf, rows, None, 0, mean, invstd, self._lane, ws=self._ws_now())
        elif self.training:
            self.fwd.add(lib.zsg_bn_stats, x.buf, rows, L.c, mean, invstd, rm, rv, 0.1, 1e-5, self._ws_now(), self.ws_bytes, what=L.name, lane=self._lane)
        else:
            self.fwd.add(lib.zsg_bn_eval_stats, rm, rv, L.c, 1e-5, mean, invstd, what=L.name, lane=self._lane)
        rmask = self._buf((rows * L.c // 4 + 3) // 4) if (relu and self.training) else None     # 4 mask bits per byte
        lane = 2 if (join and self.training) else self._lane
        inl = getattr(x, "bn_inline", None) if fused else None
        defer = defer and self.training and relu and residual is not None and rmask is not None and rows * L.c * 4 >= BN_PRE_MIN_MB * 1e6
        if defer:
            if inl is not None:       # the statistics were left to the apply launch: finalise them now (the very next launch: workspace intact)
                self.fwd.add(lib.zsg_bn_stats_from_partials, inl, x.bn_chunks, rows, L.c, mean, invstd, rm, rv, 0.1, 1e-5, what="stats:" + L.name, lane=lane)
            out.pending = dict(x=x, mean=mean, invstd=invstd, gam=gam, bet=bet, residual=residual, rmask=rmask, join=join, name=L.name)
        elif inl is not None:
            self.fwd.add(lib.zsg_bn_apply_from_partials, x.buf, rows, L.c, inl, x.bn_chunks, gam, bet, residual.buf if residual is not None else None,
                         int(relu), out.buf, rmask, mean, invstd, rm, rv, 0.1, 1e-5, what=L.name, lane=lane)
        else:
            self.fwd.add(lib.zsg_bn_apply, x.buf, rows, L.c, mean, invstd, gam, bet, residual.buf if residual is not None else None,
                         int(relu), out.buf, rmask, what=L.name, lane=lane)

        out.bn_out = self.training
        if sync:
            self.sync_bn_paths[L.name] = ("partials" if fused else "x") + ("+bnpre" if defer else "")

        def back():
            if out.grad is None:
                return
            if frozen:
                self._bn_frozen_back(L, x, out, residual, relu, rmask, rows, mean, invstd, gam)
                return
            if sync:
                self._bn_sync_back(L, x, out, residual, relu, rmask, rows, mean, invstd, gam)
                return
            dx = self.grad_of(x)
            # re-issue the data gradient that has just completed dout with the BatchNorm-backward sums in its epilogue
            # (per-tile partial rows, reduced in a fixed order by the finalize launch: deterministic)
            lw, chunks = self._bnb_chunks(L, x, out)
            fuse = lw is not None
            g_out, bits = None, rmask
            if residual is not None and residual.requires_grad:
                # Round 6: where the data gradient that completes dout carries this BatchNorm's backward sums anyway, it also STORES the
                # ReLU-masked gradient (zsg_conv_desc.epi_flags bit 0) — which IS the residual branch's gradient (out = relu(bn(x) +
                # residual)): the residual's gradient buffer becomes an alias of dout, and the apply pass below neither reads the mask nor
                # writes a second output (16 -> 12 bytes per element on the step's sixteen bn3 passes, 645 MB per step at configs[1]).
                alias = (fuse and relu and rmask is not None and residual.grad is None and len(residual.levels) == 1
                         and residual.levels[0].off == 0 and residual.ld == L.c and residual.C == L.c and residual.buf.numel() == out.grad.buf.numel())
                if alias:
                    residual.grad = out.grad
                    lw[1].epi_flags |= 1
                    bits = None
                else:
                    rg = self.grad_of(residual)
                    assert not rg.gfilled, "residual gradient must be produced first (tape order)"
                    g_out = rg.buf
                    rg.gfilled = True
            if fuse:
                part = self.ws[2 * L.c:]              # (the first 2C floats of the workspace: the finalize launch's coefficients)
                tail_n = self._bnb_tail_tickets(lw)
                if tail_n > 0:
                    # the data gradient's last tile per column block finalises the coefficients and d(gamma) / d(beta): the apply pass
                    # is all that is left of this BatchNorm's backward
                    tk = self._buf(tail_n, dtype=torch.int32)
                    coef = self._buf(2 * L.c)
                    self._bnb_reissue(lw, L, x, mean, invstd, rmask, part, chunks, fin=(tk, coef, self.G(L.name + ".weight"), self.G(L.name + ".bias")))
                    self.bwd.add(lib.zsg_bn_bwd_apply, self.base(out.grad), bits, x.buf, rows, L.c, mean, invstd, gam, coef, dx.buf, g_out,
                                 what="bnbwd:" + L.name)
                else:
                    self._bnb_reissue(lw, L, x, mean, invstd, rmask, part, chunks)
                    self.bwd.add(lib.zsg_bn_backward_from_partials, self.base(out.grad), bits, x.buf, rows, L.c, mean, invstd, gam,
                                 dx.buf, g_out, self.G(L.name + ".weight"), self.G(L.name + ".bias"), 1, part, chunks, self.ws, self.ws_bytes,
                                 what="bnbwd:" + L.name)
            else:
                self.bwd.add(lib.zsg_bn_backward, self.base(out.grad), None, rmask, x.buf, rows, L.c, mean, invstd, gam,
                             dx.buf, g_out, self.G(L.name + ".weight"), self.G(L.name + ".bias"), 1, self.ws, self.ws_bytes,
                             what="bnbwd:" + L.name)
            dx.gfilled = True
        self.tape.append(back)
        return out

    def _bnb_chunks(self, L: BnL, x: Act, out: Act):
        """(last_writer, partial rows) when the launch that has just completed out's gradient can be re-issued with this BatchNorm's
        backward sums in its epilogue (_bnb_reissue) and its partial rows fit the workspace, else (None, 0): the BatchNorm then takes
        its plain backward.  Never raises."""
        lw = getattr(out.grad, "last_writer", None)
        fuse = (BNB_FUSE and lw is not None and lw[0] == len(self.bwd.calls) - 1 and self.bwd.lanes[lw[0]] == 0
                and len(out.grad.levels) == 1 and out.grad.levels[0].off == 0 and x.levels[0].off == 0 and out.grad.ld == L.c and x.ld == L.c)
        if not fuse:
            return None, 0
        d = lw[1]
        if len(lw) > 4:                  # a bf16 data gradient (enc_bwd_dtype): zsg_conv_igemm_bf16_bnb, or nothing
            if not lib.zsg_conv_igemm_bf16_bnb_supported(_ct.byref(d)):
                return None, 0
            chunks = int(lib.zsg_conv_igemm_bf16_partial_rows(_ct.byref(d)))
            if chunks <= 0:
                return None, 0
        elif d.use_wino:
            chunks = self._wino_chunks(d, x.B)
        else:
            chunks = igemm_partial_rows(d)
        if chunks * 2 * L.c * 4 + 2 * L.c * 4 > self.ws_bytes:
            return None, 0
        return lw, chunks

    @staticmethod
    def _bnb_tail_tickets(lw) -> int:
        """tickets of the in-kernel finalize the re-issued launch can carry (0: none — every bf16 launch, which has no such form)"""
        if len(lw) > 4:
            return 0
        return int(lib.zsg_conv_bn_tail_tickets(_ct.byref(lw[1]), 1 if lw[1].use_wino else 0))

    def _bnb_reissue(self, lw, L: BnL, x: Act, mean, invstd, rmask, part, chunks: int, fin=None):
        """Re-issue the data gradient lw, which has just completed the dout of BatchNorm L, with that BatchNorm's backward sums in its
        epilogue: per-tile partial rows in `part`, reduced in a fixed order by the launch the caller adds behind it.  fin = (tickets,
        coef, d(gamma), d(beta)): the fp32 launch whose last tile per column block also finalises the sums (never a bf16 launch)."""
        idx, d, a, what = lw[:4]
        if len(lw) > 4:
            # a = (dy, packed transposed filter, out, bias=None, add_src, mask=None)
            assert a[3] is None and a[5] is None and fin is None
            fn = lib.zsg_conv_igemm_bf16_bnb
            self.bwd.calls[idx] = (fn, marshal(fn, (d, a[0], a[1], a[2], a[4], x.buf, mean, invstd, rmask, part), self.bwd.keep), what + "+bnb")
            lw[4].update(call=self.bwd.calls[idx], d=type(d).from_buffer_copy(d), bn=L.name, x=x, mean=mean, invstd=invstd, rmask=rmask,
                         part=part, chunks=chunks, epi_flags=int(d.epi_flags))
            return
        # a = (src, wt|U, out, bias=None, add_src, mask=None, partials=None)
        assert a[3] is None and a[5] is None and a[6] is None
        if fin is not None:
            tk, coef, dg, db = fin
            fn = lib.zsg_conv_wino_bnb_tail if d.use_wino else lib.zsg_conv_igemm_bnb_tail
            self.bwd.calls[idx] = (fn, marshal(fn, (d, a[0], a[1], a[2], a[4], x.buf, mean, invstd, rmask, part, tk, coef, dg, db, 1),
                                               self.bwd.keep), what + "+bnb+fin")
        else:
            fn = lib.zsg_conv_wino_bnb if d.use_wino else lib.zsg_conv_igemm_bnb
            self.bwd.calls[idx] = (fn, marshal(fn, (d, a[0], a[1], a[2], a[4], x.buf, mean, invstd, rmask, part), self.bwd.keep), what + "+bnb")

    def _bn_sync_back(self, L: BnL, x: Act, out: Act, residual: Optional[Act], relu: bool, rmask, rows: int, mean, invstd, gam):
        """Backward of a synchronized BatchNorm [+ residual] [+ ReLU] (torch's SyncBatchNorm): the rank-local (sum g, sum g * xhat) — from
        the epilogue of the data gradient that completed dout (zsg_conv_*_bnb, never the in-kernel finalize: the sums are not final
        here) or from one pass over dout / x — with the rank's own d(gamma) / d(beta); an all-reduce; the apply from the global sums and
        the forward's global N.  The residual gradient may alias dout exactly as in bn()'s back."""
        dx = self.grad_of(x)
        fs, bs = self._sync_bufs(L)
        lw, chunks = self._bnb_chunks(L, x, out)
        fuse = lw is not None
        g_out, bits = None, rmask
        if residual is not None and residual.requires_grad:
            alias = (fuse and relu and rmask is not None and residual.grad is None and len(residual.levels) == 1
                     and residual.levels[0].off == 0 and residual.ld == L.c and residual.C == L.c and residual.buf.numel() == out.grad.buf.numel())
            if alias:
                residual.grad = out.grad
                lw[1].epi_flags |= 1
                bits = None
            else:
                rg = self.grad_of(residual)
                assert not rg.gfilled, "residual gradient must be produced first (tape order)"
                g_out = rg.buf
                rg.gfilled = True
        dg, db = self.G(L.name + ".weight"), self.G(L.name + ".bias")
        if fuse:
            part = self.ws[2 * L.c:]
            self._bnb_reissue(lw, L, x, mean, invstd, rmask, part, chunks)
            self.bwd.add(lib.zsg_bn_sync_bwd_sums, None, None, None, rows, L.c, None, None, part, chunks, bs, dg, db, 1, None, 0,
                         what="bnsums:" + L.name)
        else:
            self.bwd.add(lib.zsg_bn_sync_bwd_sums, self.base(out.grad), rmask, x.buf, rows, L.c, mean, invstd, None, 0, bs, dg, db, 1,
                         self.ws, self.ws_bytes, what="bnsums:" + L.name)
        self._allreduce(self.bwd, bs, "allreduce:bnbwd:" + L.name, 0)
        self.bwd.add(lib.zsg_bn_sync_bwd_apply, self.base(out.grad), bits, x.buf, rows, L.c, mean, invstd, gam, bs, fs, dx.buf, g_out,
                     what="bnbwd:" + L.name)
        self.sync_bn_paths[L.name] += "/" + ("bnb" if fuse else "plain") + ("+alias" if bits is None and rmask is not None else "")
        dx.gfilled = True

    def _bn_frozen_back(self, L: BnL, x: Act, out: Act, residual: Optional[Act], relu: bool, rmask, rows: int, mean, invstd, gam):
        """Backward of a frozen BatchNorm [+ residual] [+ ReLU]: dx = gamma * invstd * g with g = dout * relu-bit, d(gamma) / d(beta) for
        the trainable ones only.  Where they are wanted and the data gradient that completed dout can carry the sums in its epilogue (as in
        bn()'s back), it does so for the eval statistics, and the residual gradient may alias dout exactly as there."""
        dx = self.grad_of(x) if x.requires_grad else None
        dg = self.G(L.name + ".weight") if self.trains(L.name + ".weight") else None
        db = self.G(L.name + ".bias") if self.trains(L.name + ".bias") else None
        lw, chunks = self._bnb_chunks(L, x, out) if (dg is not None or db is not None) else (None, 0)
        fuse = lw is not None
        g_out, bits = None, rmask
        if residual is not None and residual.requires_grad:
            alias = (fuse and relu and rmask is not None and residual.grad is None and len(residual.levels) == 1
                     and residual.levels[0].off == 0 and residual.ld == L.c and residual.C == L.c and residual.buf.numel() == out.grad.buf.numel())
            if alias:
                residual.grad = out.grad
                lw[1].epi_flags |= 1
                bits = None
            else:
                rg = self.grad_of(residual)
                assert not rg.gfilled, "residual gradient must be produced first (tape order)"
                g_out = rg.buf
                rg.gfilled = True
        dout = self.base(out.grad)
        dxb = dx.buf if dx is not None else None
        what_b = "bnbwd(frozen):" + L.name
        path = "onepass" if (dg is not None or db is not None) else "scale"
        if fuse:
            part = self.ws[2 * L.c:]
            tail_n = self._bnb_tail_tickets(lw)
            path = "bnb+fin" if tail_n > 0 else "bnb"
            if tail_n > 0:
                # the data gradient's last tile per column block writes d(gamma) / d(beta) for the eval statistics: a pure scale is left
                tk, coef = self._buf(tail_n, dtype=torch.int32), self._buf(2 * L.c)
                self._bnb_reissue(lw, L, x, mean, invstd, rmask, part, chunks, fin=(tk, coef, dg, db))
                if dxb is not None or g_out is not None:
                    self.bwd.add(lib.zsg_bn_frozen_backward, dout, bits, None, rows, L.c, None, invstd, gam, dxb, g_out, None, None, 0,
                                 None, 0, None, 0, what=what_b)
            else:
                self._bnb_reissue(lw, L, x, mean, invstd, rmask, part, chunks)
                self.bwd.add(lib.zsg_bn_frozen_backward, dout, bits, x.buf, rows, L.c, mean, invstd, gam, dxb, g_out, dg, db, 1, part, chunks,
                             self.ws, self.ws_bytes, what=what_b)
        elif dxb is not None or g_out is not None or dg is not None or db is not None:
            self.bwd.add(lib.zsg_bn_frozen_backward, dout, rmask, x.buf, rows, L.c, mean, invstd, gam, dxb, g_out, dg, db, 1, None, 0,
                         self.ws, self.ws_bytes, what=what_b)
        self.frozen_bn_paths[L.name] = path + ("+alias" if bits is None and rmask is not None else "")
        if dx is not None:
            dx.gfilled = True

    # ---- the network ---------------------------------------------------------------------------------------------------
    def _lower(self):
        net, B, H, W, T = self.net, self.B, self.H, self.W, self.T
        C = net.convs
        BN = net.bns
        e = "backbone.encoder."
        # shared BN workspace: sized generously up-front (largest rows*C is the stem's conv output)
        H1, W1 = conv_out(H, 7, 2, 3), conv_out(W, 7, 2, 3)
        self.ws_bytes = 32 << 20         # BN partials: >= zsg_bn_workspace_bytes for every layer, and the conv-epilogue partials
        self.ws = self._buf(self.ws_bytes // 4)
        self.ws_side = self._buf(self.ws_bytes // 4)     # the same for forward launches on the side stream (they run concurrently)
        self._lane = 0
        self.wg_ws_bytes = 256 << 20     # split-K slabs of the weight-gradient kernel (largest: 64 splits x 1.2 M weights)
        self.wg_ws = self._buf(self.wg_ws_bytes // 4)
        self.tune_dw = self._buf(max(e.size for e in net.store.entries.values()) + 64)

        # ---- static inputs ------------------------------------------------------------------------------------------
        Qn = self.Q                      # queries (== B unless images are shared)
        self.in_qvec = self._buf(Qn * T * net.emb_dim)
        self.in_qlens = self._buf(Qn)
        self.in_idx = self._buf(Qn, dtype=torch.int64) if self.shared else None      # img_idx of the forward being replayed
        nd = 2 if net.bid else 1
        self.in_hc = self._buf(2 * nd * Qn * net.lstm_dim)            # (h0 | c0: ONE host-to-device copy per step when both come from the host)
        self.in_h0, self.in_c0 = self.in_hc[:nd * Qn * net.lstm_dim], self.in_hc[nd * Qn * net.lstm_dim:]
        self.img_slot = len(self.fwd.calls)
        x0 = self.act("img_nhwc4", B, H, W, 4, requires_grad=False)
        self.fwd.add(lib.zsg_nchw_to_nhwc4, self.in_qvec, B, 3, H, W, x0.buf, what="img")     # src pointer patched per call

        # ---- query encoder ----------------------------------------------------------------------------------------------
        # The query encoder is independent of the image encoder: its launches go to the side stream (joined where the head
        # first reads `we`), and its backward is replayed right after the head's — not at the very end of the step.
        we, lstm_tape = None, []
        self._hoist = []
        if net.use_lang:
            t0 = len(self.tape)
            we = self._lower_lstm()
            lstm_tape = self.tape[t0:]
            del self.tape[t0:]
        hoist_to = len(self.fwd.calls)            # right behind the query encoder

        # ---- encoder ------------------------------------------------------------------------------------------------------
        # (the image-blind variants still run the encoder, as the reference does, mdl.py:363-375: the pyramid sizes and the
        # train-mode BatchNorm running statistics come from it; no gradient reaches it, so its backward emits nothing)
        feats: List[Act] = []
        if net.backbone_kind == "ssd_vgg":
            feats = self._lower_ssd(x0)
        else:
            H2, W2 = conv_out(H1, 3, 2, 1), conv_out(W1, 3, 2, 1)
            if self.training:
                x = self._lower_stem_fused(C[e + "conv1"], BN[e + "bn1"], x0, H1, W1, H2, W2)
            else:
                a = self.conv_bn(C[e + "conv1"], BN[e + "bn1"], x0, True, name="stem.a", yname="stem.y")
                x = self.act("pool", B, H2, W2, 64, dtype=self.adt)
                if self.act16:                                    # fp32 stem output -> bf16 (no indices: nothing runs backward)
                    idx = None
                    self.fwd.add(lib.zsg_maxpool_fwd_bf16, a.buf, int(a.b16), B, H1, W1, 64, 3, 2, 1, H2, W2, x.buf, what="maxpool")
                else:
                    idx = self._buf((B * H2 * W2 * 64 + 3) // 4)      # uint8 indices, stored in a float-sized buffer
                    self.fwd.add(lib.zsg_maxpool_fwd, a.buf, B, H1, W1, 64, 3, 2, 1, H2, W2, x.buf, idx, what="maxpool")
                pool_in, pool_out = a, x

                def pool_back():
                    if pool_out.grad is None:
                        return
                    dx = self.grad_of(pool_in)
                    self.bwd.add(lib.zsg_maxpool_bwd, self.base(pool_out.grad), idx, B, H1, W1, 64, 3, 2, 1, H2, W2, dx.buf, what="maxpool_bwd")
                    dx.gfilled = True
                self.tape.append(pool_back)
            taps, lat = {}, {}
            for blk in net.blocks:
                # (a block that is not the last of its stage has ONE first reader, the next block's conv1: that convolution applies this block's
                # closing BatchNorm + residual + ReLU itself where the activation is large, see BN_PRE_MIN_MB)
                big = net.block_kind == "bottleneck" and self.training and not blk["last"]
                x = self._lower_block(blk, x, defer_out=big)
                if blk["last"]:
                    taps[blk["layer"]] = x
                    if self.training and blk["layer"] in (2, 3):
                        # the pyramid's lateral 1x1 convolutions P3_1 / P4_1 only read C3 / C4: on the side stream as soon as their
                        # input exists, under layer3 / layer4 (whose 19^2 / 10^2 launches leave a quarter of the CUs idle), instead
                        # of in the main stream's chain between layer4 and the head
                        with self.on_side_stream():
                            nm = "P3_1" if blk["layer"] == 2 else "P4_1"
                            lat[blk["layer"]] = self.conv(C["backbone.fpn." + nm], x, name="t3" if blk["layer"] == 2 else "t4")
            feats = self._lower_fpn(taps[2], taps[3], taps[4], lat.get(2), lat.get(3))
        self.feat_sizes = [(f.levels[0].H, f.levels[0].W) for f in feats]
        self.feat_sizes_t = torch.tensor(self.feat_sizes, dtype=torch.long, device=self.dev)
        self.num_f_out_t = torch.tensor([len(feats)], dtype=torch.long, device=self.dev)
        self.tape.extend(lstm_tape)
        self._lower_head(feats, we)
        # image-independent head launches (language / grid maps of conv0) go to the side stream BEHIND the query encoder: a
        # side-stream launch waits for the main-stream work enqueued before it, so its place in the program decides what
        # it can overlap — here the whole image encoder
        moved_c, moved_l = [], []
        for (i0, i1) in reversed(self._hoist):          # cut from the back so the earlier spans' indices stay valid ...
            moved_c[0:0] = self.fwd.calls[i0:i1]
            moved_l[0:0] = self.fwd.lanes[i0:i1]
            del self.fwd.calls[i0:i1], self.fwd.lanes[i0:i1]
        self.fwd.calls[hoist_to:hoist_to] = moved_c      # ... and re-insert in their original order
        self.fwd.lanes[hoist_to:hoist_to] = moved_l
        if self.training:
            # the head-of-program side-stream block (query encoder, language maps; ~0.25 ms, read by the head ~4 ms later) is released
            # behind the 3rd join of the main stream with the side stream (a join waits for the WHOLE side stream, so in front of the
            # first one the block delays layer1.0's residual add)
            ln = self.fwd.lanes
            j = next((i for i in range(1, len(ln)) if ln[i] == 0), None)
            if j is not None and j > 1 and all(l == 1 for l in ln[1:j]):
                joins = [i for i in range(j, len(ln)) if ln[i] == 2]
                if len(joins) >= 5:          # (never behind the joins in front of the head itself; a network without residual
                    k = joins[2] + 1         #  joins — SSD-VGG — keeps the block at the head of the program)
                    blk_c, blk_l = self.fwd.calls[1:j], ln[1:j]
                    self.fwd.calls[1:k] = self.fwd.calls[j:k] + blk_c
                    self.fwd.lanes[1:k] = ln[j:k] + blk_l

        # ---- backward program: replay the tape in reverse ----------------------------------------------------------
        if self.training:
            for emit in reversed(self.tape):
                emit()
            if WG_BATCH:
                self._batch_wgrads()
            # (a frozen BatchNorm's d(gamma) / d(beta) written as a by-product is not a gradient anyone waits for)
            self.grad_ready = {k: v for k, v in self.grad_ready.items() if k not in self.frozen}
        self.tape = []

    def _batch_wgrads(self):
        """Round 6: the Winograd weight gradients of a stage's IDENTICAL convolutions (layerN.1 .. layerN.k conv2: fpn_resnet.py:86-100)
        become ONE launch (zsg_conv_wgrad_wino_batched) at the position of the last of them in the backward program.  Weight gradients
        are leaves of the backward graph and every activation / gradient buffer of a plan lives until the next forward, so holding the
        earlier ones back changes nothing but the order in which the side stream does its work: a job batch has njobs x the (n, c)
        blocks, i.e. a fraction of the split-K slabs and a longer stage loop per block (l3_conv2 x 5: 268 -> 205 us,
        profiles/r06_wgrad_batching.txt).  The launch indices recorded for DDP's buckets (grad_ready) are re-based."""
        import ctypes as C_
        groups = {}
        for rec in self._wg_log:
            idx, d, src, dy, gw, pname, what = rec
            # (Winograd launches only: batching the direct 1x1 weight gradients as well was built and measured — 13.07 -> 13.08 ms, the
            # later release of 24 launches costs what their shorter kernels save — and removed again, profiles/r06_wgrad_batching.txt)
            if d.nseg != 1 or not d.use_wino or self.bwd.calls[idx][0] is not lib.zsg_conv_wgrad_wino:
                continue
            # one geometry = one descriptor, byte for byte, the tile hint aside (the jobs of a launch share everything but their pointers)
            dz = type(d).from_buffer_copy(d)
            dz.tile_hint = 0
            sig = (bool(d.use_wino), bytes(dz))
            groups.setdefault(sig, []).append(rec)
        drop, put = set(), {}
        for sig, recs in groups.items():
            recs.sort(key=lambda r: r[0])
            for k in range(0, len(recs), 8):              # (at most ZSG_WG_MAX_JOBS per launch)
                part = recs[k:k + 8]
                if len(part) < 2:
                    continue
                n = len(part)
                d0 = part[0][1]
                db = type(d0).from_buffer_copy(d0)
                srcs, dys, gws = [r[2].buf for r in part], [r[3].buf for r in part], [r[4] for r in part]
                wino = bool(d0.use_wino)
                autotune_wgrad_batch(db, n, wino, srcs, dys, self.tune_dw, self.wg_ws, self.wg_ws_bytes, stream_ptr())
                VP = C_.c_void_p * n
                a_src, a_dy, a_dw = VP(*[t.data_ptr() for t in srcs]), VP(*[t.data_ptr() for t in dys]), VP(*[t.data_ptr() for t in gws])
                self.bwd.keep += [db, a_src, a_dy, a_dw] + srcs + dys + gws
                conv = (C_.byref(db), C_.c_int32(n), C_.cast(a_src, C_.c_void_p), C_.cast(a_dy, C_.c_void_p), C_.cast(a_dw, C_.c_void_p),
                        C_.c_int32(1), C_.c_void_p(self.wg_ws.data_ptr()), C_.c_size_t(self.wg_ws_bytes))
                last = part[-1][0]
                put[last] = (lib.zsg_conv_wgrad_wino_batched, conv, "wgrad x%d:" % n + part[-1][6].split(":", 1)[1] + " .. " + part[0][6].split(":", 1)[1])
                drop.update(r[0] for r in part[:-1])
                for r in part:
                    self.grad_ready[r[5]] = last
                    if r[1] in self._tunables:
                        self._tunables.remove(r[1])
        if not put:
            return
        remap, calls, lanes = {}, [], []
        for i, (c, l) in enumerate(zip(self.bwd.calls, self.bwd.lanes)):
            if i in drop:
                continue
            remap[i] = len(calls)
            calls.append(put.get(i, c))
            lanes.append(l)
        # a dropped launch's index maps to the next kept one (its gradient is complete no earlier than the batch, re-based above)
        nxt = len(calls)
        for i in range(len(self.bwd.calls), -1, -1):
            if i in remap:
                nxt = remap[i]
            else:
                remap[i] = nxt
        self.bwd.calls, self.bwd.lanes = calls, lanes
        self.grad_ready = {k: remap[v] for k, v in self.grad_ready.items()}
        self.n_wgrad_batches = len(put)
        # release policy with batches (ops.SIDE_BATCH): a bottleneck stage now releases ONE large Winograd launch per stage plus its 1x1
        # weight gradients; releasing every second main-stream convolution instead of every third gets the batch going earlier —
        # configs[1] 13.08 -> 13.03 / 13.14 -> 13.05 ms on two boxes (1 and 4 are slower; ResNet-18's basic blocks and SSD-VGG keep 3:
        # profiles/r06_ab_release_final.txt)
        if self.bwd.side_batch == 3 and getattr(self.net, "block_kind", "") == "bottleneck":
            self.bwd.side_batch = 2

    def _lower_stem_fused(self, L: ConvL, Lb: BnL, x0: Act, H1: int, W1: int, H2: int, W2: int) -> Act:
        """conv1 -> bn1 -> relu -> maxpool (mdl.py:149-152) in training: the BatchNorm + ReLU + max-pool are ONE pass over the stem
        activation (zsg_bn_relu_maxpool_fwd / _bwd) — the normalised 150x150x64 map, its ReLU mask and the dense pool gradient
        never exist (the stem activation is 92 MB at B=16: 311 -> 121 MB forward, 552 -> 236 MB backward)."""
        net, B = self.net, self.B
        y = self.conv(L, x0, name="stem.y", bn_fuse=Lb)
        rows = B * H1 * W1
        rm, rv = net._rm[Lb.index:Lb.index + Lb.c], net._rv[Lb.index:Lb.index + Lb.c]
        gam, bet = self.P(Lb.name + ".weight"), self.P(Lb.name + ".bias")
        self.ws_need = max(getattr(self, "ws_need", 0), lib.zsg_bn_workspace_bytes(rows, Lb.c))
        frozen = self.bn_frozen(Lb)
        sync = self.bn_synced(Lb)
        if frozen:
            mean, invstd = self._eval_stats(Lb)         # (conv() computed no statistics: the forward pass runs on the running ones)
        elif sync:
            if getattr(y, "bn_chunks", 0) > 0:          # (conv() synchronized them from its partial rows)
                mean, invstd = y.bn_mean, y.bn_invstd
            else:
                mean, invstd = self._buf(Lb.c), self._buf(Lb.c)
                self._sync_fwd_stats(Lb, y.buf, rows, None, 0, mean, invstd, 0, ws=self.ws)
            self.sync_bn_paths[Lb.name] = "partials" if getattr(y, "bn_chunks", 0) > 0 else "x"
        elif getattr(y, "bn_chunks", 0) > 0:
            mean, invstd = y.bn_mean, y.bn_invstd
            if y.bn_inline is not None:          # few partial rows (small inputs): nobody else will finalize them
                self.fwd.add(lib.zsg_bn_stats_from_partials, y.bn_inline, y.bn_chunks, rows, Lb.c, mean, invstd, rm, rv, 0.1, 1e-5, what="stats:" + Lb.name)
        else:
            mean, invstd = self._buf(Lb.c), self._buf(Lb.c)
            self.fwd.add(lib.zsg_bn_stats, y.buf, rows, Lb.c, mean, invstd, rm, rv, 0.1, 1e-5, self.ws, self.ws_bytes, what=Lb.name)
        x = self.act("pool", B, H2, W2, Lb.c)
        x.requires_grad = y.requires_grad or self.trains(Lb.name + ".weight") or self.trains(Lb.name + ".bias")
        idx = self._buf((B * H2 * W2 * Lb.c + 3) // 4)      # uint8 indices, stored in a float-sized buffer
        self.fwd.add(lib.zsg_bn_relu_maxpool_fwd, y.buf, B, H1, W1, Lb.c, mean, invstd, gam, bet, 3, 2, 1, H2, W2, x.buf, idx, what="bn1+relu+maxpool")

        def back():
            if x.grad is None:
                return
            if frozen:
                dy = self.grad_of(y) if y.requires_grad else None
                dg = self.G(Lb.name + ".weight") if self.trains(Lb.name + ".weight") else None
                db = self.G(Lb.name + ".bias") if self.trains(Lb.name + ".bias") else None
                if dy is None and dg is None and db is None:
                    return
                self.bwd.add(lib.zsg_bn_frozen_relu_maxpool_bwd, self.base(x.grad), idx, y.buf, B, H1, W1, Lb.c, mean, invstd, gam, bet, 3, 2, 1,
                             H2, W2, dy.buf if dy is not None else None, dg, db, 1, self.ws, self.ws_bytes, what="bnbwd(frozen)+maxpool_bwd:" + Lb.name)
                self.frozen_bn_paths[Lb.name] = "stem" + ("" if dg is None and db is None else "+sums")
                if dy is not None:
                    dy.gfilled = True
                return
            dy = self.grad_of(y)
            if sync:
                # zsg_bn_relu_maxpool_bwd split at the collective: rank-local sums over the pooled gradient, all-reduce, apply per input pixel
                fs, bs = self._sync_bufs(Lb)
                self.bwd.add(lib.zsg_bn_sync_relu_maxpool_bwd_sums, self.base(x.grad), idx, y.buf, B, H1, W1, Lb.c, mean, invstd, gam, bet, 3, 2,
                             1, H2, W2, bs, self.G(Lb.name + ".weight"), self.G(Lb.name + ".bias"), 1, self.ws, self.ws_bytes,
                             what="bnsums+maxpool_bwd:" + Lb.name)
                self._allreduce(self.bwd, bs, "allreduce:bnbwd:" + Lb.name, 0)
                self.bwd.add(lib.zsg_bn_sync_relu_maxpool_bwd_apply, self.base(x.grad), idx, y.buf, B, H1, W1, Lb.c, mean, invstd, gam, bet, 3, 2,
                             1, H2, W2, bs, fs, dy.buf, what="bnbwd+maxpool_bwd:" + Lb.name)
                self.sync_bn_paths[Lb.name] += "/stem"
                dy.gfilled = True
                return
            self.bwd.add(lib.zsg_bn_relu_maxpool_bwd, self.base(x.grad), idx, y.buf, B, H1, W1, Lb.c, mean, invstd, gam, bet, 3, 2, 1, H2, W2, dy.buf,
                         self.G(Lb.name + ".weight"), self.G(Lb.name + ".bias"), 1, self.ws, self.ws_bytes, what="bnbwd+maxpool_bwd:" + Lb.name)
            dy.gfilled = True
        self.tape.append(back)
        return x

    # ---- generic pooling / normalisation lowering (SSD-VGG trunk) -------------------------------------------------
    def _grad_sink(self, a: Act):
        """Where a non-conv producer may write d(a): straight into a.grad when nothing is there yet and no ReLU mask is
        due, else a scratch buffer that `_grad_commit` folds in with the mask (dx (+)= scratch * (a > 0))."""
        g = self.grad_of(a)
        if not g.gfilled and not a.needs_mask:
            return g, None
        return g, self.like(a, a.name + ".gtmp")

    def _grad_commit(self, a: Act, g: Act, tmp: Optional[Act]):
        if tmp is not None:
            n = sum(a.B * l.H * l.W * a.ld for l in a.levels)
            if a.needs_mask:
                self.bwd.add(lib.zsg_relu_bwd, self.base(tmp), self.base(a), n, self.base(g), int(g.gfilled), what="mask+acc:" + a.name)
            else:
                raise AssertionError("accumulation without mask is not needed by any lowered model")
        g.gfilled = True

    def maxpool(self, x: Act, k: int, s: int, p: int, ceil: bool, name: str) -> Act:
        l = x.levels[0]

        def osz(n):
            o = (n + 2 * p - k + (s - 1 if ceil else 0)) // s + 1
            if ceil and (o - 1) * s >= n + p:
                o -= 1
            return o
        Ho, Wo = osz(l.H), osz(l.W)
        out = self.act(name, x.B, Ho, Wo, x.C, dtype=self.adt)
        out.requires_grad = x.requires_grad
        if self.act16:
            idx = None
            self.fwd.add(lib.zsg_maxpool_fwd_bf16, x.buf, int(x.b16), x.B, l.H, l.W, x.C, k, s, p, Ho, Wo, out.buf, what=name)
        else:
            idx = self._buf((x.B * Ho * Wo * x.C + 3) // 4)
            self.fwd.add(lib.zsg_maxpool_fwd, x.buf, x.B, l.H, l.W, x.C, k, s, p, Ho, Wo, out.buf, idx, what=name)

        def back():
            if out.grad is None:
                return
            g, tmp = self._grad_sink(x)
            self.bwd.add(lib.zsg_maxpool_bwd, self.base(out.grad), idx, x.B, l.H, l.W, x.C, k, s, p, Ho, Wo, (tmp or g).buf, what=name + "_bwd")
            self._grad_commit(x, g, tmp)
        self.tape.append(back)
        return out

    def l2norm(self, x: Act, name: str, out: Optional[Act] = None, lane: int = 0) -> Act:
        """x / ||x||_2 over channels, no epsilon (ssd_vgg.py:80, mdl.py:118-130); x / out may be levels of packed buffers"""
        l = x.levels[0]
        rows = x.B * l.H * l.W
        if out is None:
            out = self.act(name, x.B, l.H, l.W, x.C, dtype=x.buf.dtype)
        out.requires_grad = x.requires_grad
        nrm = self._buf(rows)
        # (bf16_act: no bf16 form — the fp32 kernel between casts; identities in every other plan)
        x32, o32, _, finish = self._via_f32(x, out, lane=lane)
        self.fwd.add(lib.zsg_l2norm_fwd, self.base(x32), rows, x.C, self.base(o32), nrm, what=name, lane=lane)
        finish()

        def back():
            if out.grad is None:
                return
            g, tmp = self._grad_sink(x)
            self.bwd.add(lib.zsg_l2norm_bwd, self.base(out.grad), self.base(out), nrm, rows, x.C, self.base(tmp or g), what=name + "_bwd")
            self._grad_commit(x, g, tmp)
        self.tape.append(back)
        return out

    def _lower_ssd(self, x0: Act) -> List[Act]:
        """SSD.forward, ssd_vgg.py:54-102 (ReLU fused into every conv epilogue)."""
        net = self.net
        C = net.convs
        e = "backbone.encoder."
        # pyramid sizes of the 300-style trunk: conv4_3, conv7, then the four extras taps
        l0 = x0.levels[0]

        def trunk(n):
            n = (n // 2) // 2                       # two floor-mode 2x2 pools
            c43 = -(-n // 2)                        # ceil-mode pool ('C')
            c7 = c43 // 2
            e1 = conv_out(c7, 3, 2, 1)
            e3 = conv_out(e1, 3, 2, 1)
            e5 = conv_out(e3, 3, 1, 0)
            e7 = conv_out(e5, 3, 1, 0)
            return [c43, c7, e1, e3, e5, e7]
        all_sizes = list(zip(trunk(l0.H), trunk(l0.W)))
        fl = self._pyramid(all_sizes[1:] if net.six_hundred else all_sizes)
        dest = ([None] + fl) if net.six_hundred else fl          # destination of out_sources[i]
        x = x0
        sources = []
        for layer in net.vgg_layers:
            if layer[0] == "conv":
                x = self.conv(C[f"{e}vgg.{layer[1]}"], x, relu=True, name=f"vgg.{layer[1]}")
                if layer[1] == 21:                      # conv4_3 + ReLU == vgg[0:23]
                    sources.append(self.l2norm(x, "conv4_3.norm"))
            else:
                _, idx, k, s, p, ceil = layer
                x = self.maxpool(x, k, s, p, ceil, f"vgg.{idx}")
        sources.append(x)
        for k in range(net.n_extras):
            tap = (k % 2 == 1)
            x = self.conv(C[f"{e}extras.{k}"], x, relu=True, name=f"extras.{k}", out=dest[2 + (k - 1) // 2] if (tap and k > 1) else None)
            if tap:
                sources.append(x)
        outs = [self.conv(C[f"{e}fproj{i + 1}"], sources[i], name=f"fproj{i + 1}", out=dest[i]) for i in range(3)] + sources[3:]
        return outs[1:] if net.six_hundred else outs

    def _lower_block(self, blk, x: Act, defer_out: bool = False) -> Act:
        """fpn_resnet.py:26-58 (BasicBlock), :61-100 (Bottleneck).  Training: a projection shortcut (downsample conv +
        BatchNorm) only depends on the block input, so it is lowered FIRST, on the side stream, and runs concurrently with
        the block's main branch; the last BatchNorm (which adds it) joins."""
        net = self.net
        C, BN, q = net.convs, net.bns, blk["prefix"]
        rd = x
        if blk["ds"]:
            with self.on_side_stream():
                rd = self.conv_bn(C[q + "downsample.0"], BN[q + "downsample.1"], x, False, name=q + "rd", yname=q + "yd")
        join = blk["ds"]
        if net.block_kind == "bottleneck":
            a1 = self.conv_bn(C[q + "conv1"], BN[q + "bn1"], x, True, name=q + "a1", yname=q + "y1")
            a2 = self.conv_bn(C[q + "conv2"], BN[q + "bn2"], a1, True, name=q + "a2", yname=q + "y2")
            if self.training:
                y3 = self.conv(C[q + "conv3"], a2, name=q + "y3", bn_fuse=BN[q + "bn3"])
                return self.bn(BN[q + "bn3"], y3, True, residual=rd, name=q + "out", join=join, defer=defer_out)
            return self.conv_bn(C[q + "conv3"], BN[q + "bn3"], a2, True, residual=rd, name=q + "out", yname=q + "y3")
        a1 = self.conv_bn(C[q + "conv1"], BN[q + "bn1"], x, True, name=q + "a1", yname=q + "y1")
        if self.training:
            y2 = self.conv(C[q + "conv2"], a1, name=q + "y2", bn_fuse=BN[q + "bn2"])
            return self.bn(BN[q + "bn2"], y2, True, residual=rd, name=q + "out", join=join)
        return self.conv_bn(C[q + "conv2"], BN[q + "bn2"], a1, True, residual=rd, name=q + "out", yname=q + "y2")

    def _pyramid(self, sizes) -> List[Act]:
        """The head's input features: all pyramid levels packed level-major in ONE buffer (so every head convolution is
        one grouped launch); the producers write their level in place."""
        self.Fpack = self.packed("head.feat_raw" if self.net.do_norm else "head.feat", self.B, sizes, 256, dtype=self.adt)
        lv = [self.Fpack.lvl(i) for i in range(len(sizes))]
        for i, a in enumerate(lv):
            a.name = f"feat{i}"
        return lv

    def _lower_fpn(self, c3: Act, c4: Act, c5: Act, t3: Optional[Act] = None, t4: Optional[Act] = None) -> List[Act]:
        """fpn_resnet.py:154-178"""
        net, B = self.net, self.B
        C = net.convs
        f = "backbone.fpn."
        hw = lambda a: (a.levels[0].H, a.levels[0].W)
        s6 = tuple(conv_out(v, 3, 2, 1) for v in hw(c5))
        s7 = tuple(conv_out(v, 3, 2, 1) for v in s6)
        if net.six_hundred:
            fl = self._pyramid([hw(c4), hw(c5), s6, s7])
            o3, o8, (o4, o5, o6, o7) = None, None, fl
        else:
            fl = self._pyramid([hw(c3), hw(c4), hw(c5), s6, s7, (1, 1)])
            o3, o4, o5, o6, o7, o8 = fl
        # The pyramid's output convolutions P5_2 / P4_2 and the whole P6 -> P7 (-> P8) chain are leaves that only the head reads:
        # in training they run on the side stream, concurrently with the lateral / top-down path and the large P3_2.
        if t3 is not None or t4 is not None:
            # the laterals lowered early on the side stream (P3_1 under layer3, P4_1 under layer4) are joined HERE, in front of the pyramid's
            # own side-stream launches: a join waits for the whole side stream
            self._join_side()
        # Training (round 5; rocprofv3 showed the head's first convolution waiting 56 us for the side stream's chain P5_2 -> P4_2 -> P6 ->
        # ReLU -> P7 -> pool, which only started behind P5_1): the P6 chain (it reads C5 only) is released BEFORE P5_1, and P4_2 runs on
        # the main stream.  Eval and 600^2: the chain is lowered behind P4_2 and in front of P3_1 / the top-down add / the large P3_2 — a
        # side-stream launch waits for the main-stream work enqueued before it, so in program order behind P3_2 the chain only started when
        # P3_2 had finished and the head's first convolution waited ~90 us for it; here it runs under P3_1 / P3_2.
        p6_early = self.training and not net.six_hundred
        if p6_early:
            # (P5_1 stays the consumer whose data gradient completes layer4's last BatchNorm dout — it carries that BatchNorm's backward
            # sums, which the strided P6 cannot — so the chain's backward entries go BEHIND P5_1's on the tape: the tape is replayed in reverse)
            keep, n0 = getattr(c5, "_consumed", False), len(self.tape)
            c5._consumed = True
            p6, p7, p8 = self._lower_p6_chain(c5, o6, o7, o8)
            p6_tape = self.tape[n0:]
            del self.tape[n0:]
            c5._consumed = keep
        p51 = self.conv(C[f + "P5_1"], c5, name="p51")
        if p6_early:
            self.tape.extend(p6_tape)
        with self.on_side_stream():
            p5 = self.conv(C[f + "P5_2"], p51, out=o5)
        if t4 is None:
            t4 = self.conv(C[f + "P4_1"], c4, name="t4")
        p41 = self._upsample_add(t4, p51, "p41")
        if p6_early:
            p4 = self.conv(C[f + "P4_2"], p41, out=o4)
        else:
            with self.on_side_stream():
                p4 = self.conv(C[f + "P4_2"], p41, out=o4)
            p6, p7, p8 = self._lower_p6_chain(c5, o6, o7, o8)
        if t3 is None:
            t3 = self.conv(C[f + "P3_1"], c3, name="t3")
        p31 = self._upsample_add(t3, p41, "p31")
        p3 = self.conv(C[f + "P3_2"], p31, out=o3, name="p3")
        self._join_side()
        if net.six_hundred:
            return [p4, p5, p6, p7]           # p3 is computed and dropped, as the reference does (fpn_resnet.py:173-174)
        return [p3, p4, p5, p6, p7, p8]

    def _lower_p6_chain(self, c5: Act, o6: Act, o7: Act, o8: Optional[Act]):
        """P6 -> ReLU -> P7_2 (-> global average pool: fpn_resnet.py:175-178 + mdl.py's P8; o8=None at 600^2, which stops at P7)
        on the side stream"""
        net, B = self.net, self.B
        C = net.convs
        f = "backbone.fpn."
        with self.on_side_stream():
            p6 = self.conv(C[f + "P6"], c5, out=o6)
            r6 = self.act("r6", B, p6.levels[0].H, p6.levels[0].W, 256, dtype=self.adt)
            r6.requires_grad = p6.requires_grad
            n6 = r6.buf.numel()
            self.fwd.add(lib.zsg_relu_fwd_bf16 if self.act16 else lib.zsg_relu_fwd, self.base(p6), n6, r6.buf, what="relu(p6)", lane=self._lane)

            def relu_back():
                if r6.grad is None:
                    return
                g = self.grad_of(p6)
                self.bwd.add(lib.zsg_relu_bwd, self.base(r6.grad), self.base(p6), n6, self.base(g), int(g.gfilled), what="relu_bwd(p6)")
                g.gfilled = True
            self.tape.append(relu_back)
            p7 = self.conv(C[f + "P7_2"], r6, out=o7)
            if o8 is None:
                return p6, p7, None
            l7 = p7.levels[0]
            p8 = o8
            p8.requires_grad = p7.requires_grad
            self.fwd.add(lib.zsg_avgpool_fwd_bf16 if self.act16 else lib.zsg_avgpool_fwd, self.base(p7), B, l7.H * l7.W, 256, self.base(p8),
                         what="avgpool", lane=self._lane)

            def avg_back():
                if p8.grad is None:
                    return
                g = self.grad_of(p7)
                self.bwd.add(lib.zsg_avgpool_bwd, self.base(p8.grad), B, l7.H * l7.W, 256, self.base(g), int(g.gfilled), what="avgpool_bwd")
                g.gfilled = True
            self.tape.append(avg_back)
        return p6, p7, p8

    def _upsample_add(self, a: Act, p: Act, name: str, join: bool = False) -> Act:
        la, lp = a.levels[0], p.levels[0]
        out = self.act(name, a.B, la.H, la.W, a.C, dtype=self.adt)
        out.requires_grad = a.requires_grad or p.requires_grad
        assert a.b16 == p.b16 == out.b16
        self.fwd.add(lib.zsg_upsample_add_fwd_bf16 if self.act16 else lib.zsg_upsample_add_fwd, a.buf, p.buf, a.B, lp.H, lp.W, la.H, la.W, a.C,
                     out.buf, what=name, lane=2 if (join and self.training) else 0)

        def back():
            if out.grad is None:
                return
            assert a.grad is None
            a.grad = out.grad                     # identity branch: share the buffer
            g = self.grad_of(p)
            self.bwd.add(lib.zsg_upsample_add_bwd, self.base(out.grad), a.B, lp.H, lp.W, la.H, la.W, a.C, self.base(g), int(g.gfilled),
                         what=name + "_bwd")
            g.gfilled = True
        self.tape.append(back)
        return out

    def _lower_lstm(self) -> Act:
        """mdl.py:296-336.  we [B, 2H] = [h_fwd(len-1) | reverse-cell(x[len-1])]  (cfg lang_pool = last; the other modes: _lower_lstm_seq)"""
        net, B, T = self.net, self.Q, self.T
        E, Hd = net.emb_dim, net.lstm_dim
        H4 = 4 * Hd
        if net.lang_pool_mode != "last":
            return self._lower_lstm_seq()
        we = self.act("we", B, 1, 1, net.lstm_out_dim)
        dirs = [("", 0)] + ([("_reverse", 1)] if net.bid else [])
        we.requires_grad = any(self.trains(f"lstm.{k}_l0{suf}") for suf, _ in dirs for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
        x_all = Act(self.in_qvec, B, E, E, [Level(0, 1, T, T * E)], "qvec")
        x_all.requires_grad = False
        xlast = self.act("xlast", B, 1, 1, E, requires_grad=False)
        for suf, di in dirs:
            Tn = T if di == 0 else 1
            xin = x_all if di == 0 else xlast
            if di == 1:
                self.fwd.add(lib.zsg_lstm_gather_last, self.in_qvec, self.in_qlens, B, T, E, xlast.buf, what="gather_last", lane=1)
            gin = self.act("gin" + suf, B, 1, Tn, H4)
            d = fwd_desc(xin, gin, E, H4, 1, 1, 0, 1, wC=E)
            self.fwd.add(lib.zsg_conv_igemm, d, xin.buf, self.P("lstm.weight_ih_l0" + suf), gin.buf, self.P("lstm.bias_ih_l0" + suf),
                         None, None, None, what="lstm_in" + suf, lane=1)
            gates, cst, hprev = self._buf(B * Tn * H4), self._buf(B * Tn * Hd), self._buf(B * Tn * Hd)
            h0 = self.in_h0[di * B * Hd:(di + 1) * B * Hd]
            c0 = self.in_c0[di * B * Hd:(di + 1) * B * Hd]
            lens = self.in_qlens if di == 0 else None
            self.fwd.add(lib.zsg_lstm_fwd, gin.buf, self.P("lstm.weight_hh_l0" + suf), self.P("lstm.bias_hh_l0" + suf), h0, c0,
                         self.in_qlens, lens, B, Tn, Hd, gates, cst, hprev, we.buf, net.lstm_out_dim, di * Hd, what="lstm" + suf, lane=1)

            def back(suf=suf, di=di, Tn=Tn, xin=xin, gates=gates, cst=cst, hprev=hprev, c0=c0, lens=lens):
                if we.grad is None:
                    return
                dg = Act(self._buf(B * Tn * H4), B, H4, H4, [Level(0, 1, Tn, Tn * H4)], "dgates" + suf)
                self.bwd.add(lib.zsg_lstm_bwd, we.grad.buf, net.lstm_out_dim, di * Hd, self.P("lstm.weight_hh_l0" + suf), gates, cst, c0,
                             self.in_qlens, lens, B, Tn, Hd, dg.buf, what="lstm_bwd" + suf, lane=1)
                if self.trains("lstm.weight_ih_l0" + suf):
                    d_ih = fwd_desc(xin, dg, E, H4, 1, 1, 0, 1, wC=E)
                    self.bwd.add(lib.zsg_conv_wgrad, d_ih, xin.buf, dg.buf, self.G("lstm.weight_ih_l0" + suf), 1, self.wg_ws, self.wg_ws_bytes,
                                 what="wgrad:w_ih" + suf, lane=1)
                if self.trains("lstm.weight_hh_l0" + suf):
                    hp = Act(hprev, B, Hd, Hd, [Level(0, 1, Tn, Tn * Hd)], "hprev" + suf)
                    d_hh = fwd_desc(hp, dg, Hd, H4, 1, 1, 0, 1, wC=Hd)
                    self.bwd.add(lib.zsg_conv_wgrad, d_hh, hp.buf, dg.buf, self.G("lstm.weight_hh_l0" + suf), 1, self.wg_ws, self.wg_ws_bytes,
                                 what="wgrad:w_hh" + suf, lane=1)
                for bname in ("lstm.bias_ih_l0", "lstm.bias_hh_l0"):
                    if not self.trains(bname + suf):
                        continue
                    self.bwd.add(lib.zsg_colsum, dg.buf, 1, 0, B * Tn, H4, 0, H4, self.G(bname + suf), 1, what="bgrad:" + bname + suf, lane=1)
            self.tape.append(back)
        return we

    def _lower_lstm_seq(self) -> Act:
        """cfg lang_pool = final / mean / attn (csrc/lstm_seq.hip; definitions in include/zsg.h).  Both directions run over all T tokens:
        the reverse direction's input projection has the forward direction's geometry (no gather_last), zsg_lstm_seq_fwd walks it from
        x[len-1] down to x[0].  final: we [B, 2H] = [f_{len-1} | r_0], the two end states.  mean / attn: the directions write the padded
        output o [B, T, 2H] and zsg_lang_pool_fwd reduces it over each query's valid tokens; on the tape the pool's backward comes first and
        hands d(o) to the two BPTT sweeps.  Everything the steps save is token-aligned, so the weight / bias gradients are the GEMMs and
        column sums of the `last` program over [B * T] rows.  All on the side stream (lane 1).
        cfg lang_fuse = "words": o is written in every mode (final: beside the end states, by the same launches) and kept as self._hseq
        for the heads' key / value projections; the heads leave their d(o) = dKw . W_key + dVw . W_value as deferred launches in
        self._words_dhseq, which a tape entry replays BEHIND the pool's backward (that launch writes its d(o) everywhere; in final mode
        the heads' is the only one) and ahead of the two sweeps, accumulating into the one buffer the sweeps read."""
        net, B, T = self.net, self.Q, self.T
        E, Hd, D = net.emb_dim, net.lstm_dim, net.lstm_out_dim
        H4 = 4 * Hd
        mode = net.lang_pool_mode
        pooled = mode in ("mean", "attn")
        attn = mode == "attn"
        pmode = 1 if attn else 0           # ZSG_LANG_POOL_ATTN / ZSG_LANG_POOL_MEAN
        we = self.act("we", B, 1, 1, D)
        dirs = [("", 0)] + ([("_reverse", 1)] if net.bid else [])

        def dir_trains(suf):
            return any(self.trains(f"lstm.{k}_l0{suf}") for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
        pw_trains = attn and self.trains("lang_pool.weight")
        we.requires_grad = any(dir_trains(suf) for suf, _ in dirs) or pw_trains
        x_all = Act(self.in_qvec, B, E, E, [Level(0, 1, T, T * E)], "qvec")
        x_all.requires_grad = False
        words = net.lang_fuse == "words"
        hseq = self._buf(B * T * D) if (pooled or words) else None
        alpha = self._buf(B * T) if attn else None
        pw = self.P("lang_pool.weight") if attn else None
        lens = self.in_qlens
        grads = {}                         # d(o) of the pool's backward, read by the two sweeps emitted behind it
        if words:
            if not 1 <= T <= 64:           # (zsg_head_words_conv0's contract: one lane of the wave per token)
                raise ValueError(f"lang_fuse='words' attends over at most 64 token positions per query; this batch has qvec of {T}")
            self._hseq = Act(hseq, B, D, D, [Level(0, 1, T, T * D)], "hseq")
            self._hseq.requires_grad = any(dir_trains(suf) for suf, _ in dirs)      # (the heads form d(o) only when a direction trains)
            self._words_dhseq = []         # emit(dst, filled) of every head stack, filled in by _head_stack's backward
        for suf, di in dirs:
            gin = self.act("gin" + suf, B, 1, T, H4)
            d = fwd_desc(x_all, gin, E, H4, 1, 1, 0, 1, wC=E)
            self.fwd.add(lib.zsg_conv_igemm, d, x_all.buf, self.P("lstm.weight_ih_l0" + suf), gin.buf, self.P("lstm.bias_ih_l0" + suf),
                         None, None, None, what="lstm_in" + suf, lane=1)
            gates, cst, hprev = self._buf(B * T * H4), self._buf(B * T * Hd), self._buf(B * T * Hd)
            h0 = self.in_h0[di * B * Hd:(di + 1) * B * Hd]
            c0 = self.in_c0[di * B * Hd:(di + 1) * B * Hd]
            self.fwd.add(lib.zsg_lstm_seq_fwd, gin.buf, self.P("lstm.weight_hh_l0" + suf), self.P("lstm.bias_hh_l0" + suf), h0, c0,
                         self.in_qlens, lens, B, T, Hd, di, gates, cst, hprev, hseq, D, di * Hd, None if pooled else we.buf, D, di * Hd,
                         what="lstm_seq" + suf, lane=1)

            def back(suf=suf, di=di, gates=gates, cst=cst, hprev=hprev, c0=c0):
                if we.grad is None or not dir_trains(suf):
                    return
                dg = Act(self._buf(B * T * H4), B, H4, H4, [Level(0, 1, T, T * H4)], "dgates" + suf)
                self.bwd.add(lib.zsg_lstm_seq_bwd, None if pooled else we.grad.buf, D, di * Hd, grads.get("dhseq"), D, di * Hd,
                             self.P("lstm.weight_hh_l0" + suf), gates, cst, c0, self.in_qlens, lens, B, T, Hd, di, dg.buf,
                             what="lstm_seq_bwd" + suf, lane=1)
                if self.trains("lstm.weight_ih_l0" + suf):
                    d_ih = fwd_desc(x_all, dg, E, H4, 1, 1, 0, 1, wC=E)
                    self.bwd.add(lib.zsg_conv_wgrad, d_ih, x_all.buf, dg.buf, self.G("lstm.weight_ih_l0" + suf), 1, self.wg_ws, self.wg_ws_bytes,
                                 what="wgrad:w_ih" + suf, lane=1)
                if self.trains("lstm.weight_hh_l0" + suf):
                    hp = Act(hprev, B, Hd, Hd, [Level(0, 1, T, T * Hd)], "hprev" + suf)
                    d_hh = fwd_desc(hp, dg, Hd, H4, 1, 1, 0, 1, wC=Hd)
                    self.bwd.add(lib.zsg_conv_wgrad, d_hh, hp.buf, dg.buf, self.G("lstm.weight_hh_l0" + suf), 1, self.wg_ws, self.wg_ws_bytes,
                                 what="wgrad:w_hh" + suf, lane=1)
                for bname in ("lstm.bias_ih_l0", "lstm.bias_hh_l0"):
                    if not self.trains(bname + suf):
                        continue
                    self.bwd.add(lib.zsg_colsum, dg.buf, 1, 0, B * T, H4, 0, H4, self.G(bname + suf), 1, what="bgrad:" + bname + suf, lane=1)
            self.tape.append(back)
        if words:
            def words_back():              # (replayed behind pool_back, ahead of the two sweeps)
                for emit in self._words_dhseq:
                    if "dhseq" not in grads:
                        grads["dhseq"] = self._buf(B * T * D)
                        emit(grads["dhseq"], False)
                    else:
                        emit(grads["dhseq"], True)
            self.tape.append(words_back)
        if pooled:
            self.fwd.add(lib.zsg_lang_pool_fwd, hseq, lens, pw, pmode, B, T, D, we.buf, alpha, what="lang_pool", lane=1)

            def pool_back():               # (last on the tape: replayed ahead of the two sweeps)
                if we.grad is None:
                    return
                grads["dhseq"] = self._buf(B * T * D)
                ds = self._buf(B * T) if attn else None
                self.bwd.add(lib.zsg_lang_pool_bwd, we.grad.buf, hseq, lens, pw, alpha, pmode, B, T, D, grads["dhseq"], ds,
                             what="lang_pool_bwd", lane=1)
                if pw_trains:
                    self.bwd.add(lib.zsg_lang_pool_wgrad, ds, hseq, B, T, D, self.G("lang_pool.weight"), 1, what="wgrad:lang_pool", lane=1)
            self.tape.append(pool_back)
        return we

    def _lower_head(self, feats: List[Act], we: Optional[Act]):
        """concat_we (mdl.py:69-104, blind variants :363-375, do_norm :118-130) + the head(s) (mdl.py:211-244, 377-389)
        over all pyramid levels in grouped launches."""
        net, B = self.net, self.Q          # (the head's batch is the queries'; the features keep the images': self.B)
        sizes = self.feat_sizes
        Cf, Cw, Cg = net.cf, net.cw, (4 if net.use_grid else 0)
        assert [(f.levels[0].H, f.levels[0].W) for f in feats] == sizes
        hc = types.SimpleNamespace(Cf=Cf, Cw=Cw, Cg=Cg, we=we, gridmap=None)
        # do_norm: per-pixel channel L2 normalisation of the maps and of the language vector
        hc.Fp = self.Fpack if Cf else None
        feat_rg = any(f.requires_grad for f in feats)
        if Cf:
            self.Fpack.requires_grad = feat_rg
        heads_in = feats                         # the Acts whose .grad conv0's data gradient fills
        if net.do_norm and Cf:
            hc.Fp = self.packed("head.feat", self.B, sizes, 256, dtype=self.adt)
            hc.Fp.requires_grad = feat_rg
            heads_in = [self.l2norm(f, f"featnorm{i}", out=hc.Fp.lvl(i)) for i, f in enumerate(feats)]
        if net.do_norm and Cw:
            # (side stream, behind the query encoder that produces `we`; hoisted together with the language maps that read it)
            hoist = self.training and Cf
            i0 = len(self.fwd.calls)
            hc.we = self.l2norm(we, "we.norm", lane=(1 if hoist else 2))
            if hoist:
                self._hoist.append((i0, len(self.fwd.calls)))
        if Cg:
            gm = np.zeros((sum(h * w for h, w in sizes), 4), np.float32)
            o = 0
            for (h, w) in sizes:
                gm[o:o + h * w, :2] = anchors_mod.create_grid_np(h, w).reshape(h * w, 2)
                o += h * w
            hc.gridmap = self.packed("head.grid", 1, sizes, 4)
            hc.gridmap.buf.copy_(torch.from_numpy(gm.reshape(-1)))
            hc.gridmap.requires_grad = False
        P = sum(hh * ww for hh, ww in sizes)
        self.A = P * net.n_anchors
        nA = net.n_anchors

        def out_view(buf, nout):                 # [B][P][nout]: the levels concatenated along the anchor axis
            lv, off = [], 0
            for (hh, ww) in sizes:
                lv.append(Level(off * nout, hh, ww, P * nout))
                off += hh * ww
            return Act(buf, B, nout, nout, lv, "head.out")

        if Cf and self.training:                 # runs after every head's conv0 data gradient (reverse tape order)
            def feats_back():
                dF = hc.Fp.grad
                if dF is None:
                    return
                for i, f in enumerate(heads_in):
                    assert f.grad is None
                    f.grad = dF.lvl(i)
                    f.grad.gfilled = True
                    if f.needs_mask:             # SSD extras feed the head post-ReLU: turn d(relu(y)) into d(y) in place
                        n = f.B * f.levels[0].H * f.levels[0].W * f.ld
                        self.bwd.add(lib.zsg_relu_bwd, self.base(f.grad), self.base(f), n, self.base(f.grad), 0, what=f"mask:feat{i}")
            self.tape.append(feats_back)

        self.out5 = out_view(self._buf(B * P * 5 * nA), 5 * nA)
        self.g5_in = self._buf(B * P * 5 * nA) if self.training else None
        if net.same_atb:
            self._head_stack("att_reg_box", 5 * nA, hc, self.out5, self.g5_in)
            return
        # separate heads (mdl.py:220-225, 383-389): their outputs are interleaved into the [B, A, (4 box | 1 att)] tensor the
        # loss / evaluator kernels read, and the incoming gradient is split the same way
        o_att, o_reg = out_view(self._buf(B * P * nA), nA), out_view(self._buf(B * P * 4 * nA), 4 * nA)
        g_att = self._buf(B * P * nA) if self.training else None
        g_reg = self._buf(B * P * 4 * nA) if self.training else None
        self._head_stack("att_box", nA, hc, o_att, g_att)
        self._head_stack("reg_box", 4 * nA, hc, o_reg, g_reg)
        self.fwd.add(lib.zsg_interleave, o_reg.buf, B * P, nA, 4, self.out5.buf, 5, 0, 0, what="out5<-reg")
        self.fwd.add(lib.zsg_interleave, o_att.buf, B * P, nA, 1, self.out5.buf, 5, 4, 0, what="out5<-att")
        if self.training and (self._head_rg["att_box"] or self._head_rg["reg_box"]):
            def split_back():
                self.bwd.add(lib.zsg_interleave, g_reg, B * P, nA, 4, self.g5_in, 5, 0, 1, what="g5->reg")
                self.bwd.add(lib.zsg_interleave, g_att, B * P, nA, 1, self.g5_in, 5, 4, 1, what="g5->att")
            self.tape.append(split_back)

    def _head_stack(self, prefix: str, nout: int, hc, out: Act, g_in: Optional[torch.Tensor]):
        """One 6-convolution head `prefix`.{0..4}.0 / .5 (mdl.py:235-244) on the shared input described by hc; writes
        `out` [B][P][nout]; its backward starts from g_in (same layout)."""
        net, B = self.net, self.Q
        C = net.convs
        sizes = self.feat_sizes
        Cf, Cw, Cg, we, Fp, gridmap = hc.Cf, hc.Cw, hc.Cg, hc.we, hc.Fp, hc.gridmap
        L0 = C[prefix + ".0.0"]
        W0n = L0.name + ".weight"
        cp = L0.cpad
        assert cp == Cf + Cw + Cg
        h1 = self.packed(prefix + ".h1", B, sizes, 256, dtype=self.adt)
        # conv0 sees [features | language vector (constant over the image) | grid (constant over the batch)] (or a subset,
        # mdl.py:363-375): only the features go through the big implicit GEMM; the rest enters as an additive map
        #   lmap[b][p][n] = G[p][n] + sum_{tap valid at p} V[b][n*9+tap],  V = W0[:, :, :, lang] . we[b],  G = conv(grid, W0[..., grid])
        lmap = None
        # cfg lang_fuse = "film": EVERY plan takes the shared plans' form — the feature GEMM leaves the raw accumulator Y and one launch
        # (zsg_head_film_conv0) writes h1 = relu((1 + gamma[q]) * Y[img_idx[q]] + bias + G + taps of V[q]), gamma = W_gamma . we from one
        # more 1x1 launch beside V's.  A plain plan passes no index (the identity, Bi == Q).  Y is kept for the backward (d(gamma) reads
        # it; no plan buffer is recycled).  In a plain training plan V, gamma and G sit on the side stream and are hoisted behind the
        # query encoder, as the language maps of a "concat" plan are.
        # cfg lang_fuse = "words": film's form with a scale per PIXEL — Kw = W_key . o_t, Vw = W_value . o_t from two 1x1 launches over the
        # [Q * T] rows of the BiLSTM's output (beside V on the side stream, hoisted with it), and zsg_head_words_conv0 in place of the film
        # launch: every pixel's Y row attends over its phrase's tokens.  Training plans keep alpha [Q][P][T] and Y for the backward.
        film = net.lang_fuse == "film"
        words = net.lang_fuse == "words"
        mod = film or words
        Wfn = prefix + ".film.weight"
        Wkn, Wvn = prefix + ".words.key.weight", prefix + ".words.value.weight"
        wscale = 1.0 / math.sqrt(256.0)
        gam = Y = Kw = Vw = walpha = None
        if self.shared or mod:
            # Queries sharing images: the feature GEMM runs once per IMAGE SLOT and leaves its raw accumulator Y (no bias, no ReLU, no
            # additive map); ONE zsg_head_shared_conv0 launch then writes every query's h1 = relu(Y[img_idx[q]] + bias + G + taps of V[q]),
            # which takes the place of the language map launch and of conv0's epilogue.  Nothing here reduces across image slots, so a
            # slot no query points to (the padding of the image bucket) never reaches an output row.
            # In a training plan the same launches run (Y is not kept for the backward: the ReLU mask is h1's own); train-mode BatchNorm
            # upstream DOES reduce across slots, which is why such a plan has no padding slots.
            assert Cf
            V = G = None
            side = 1 if (mod and self.training and not self.shared) else 0
            i0 = len(self.fwd.calls)
            if Cw:
                V = self.act(prefix + ".V", B, 1, 1, 9 * 256, requires_grad=False)
                dv = fwd_desc(we, V, Cw, 9 * 256, 1, 1, 0, 1, wC=cp, wt_ld=cp, wc0=Cf)
                self.fwd.add(lib.zsg_conv_igemm, dv, we.buf, self.P(W0n), V.buf, None, None, None, None, what=prefix + "0.V", lane=(1 if side else 2))
            if film:
                gam = self.act(prefix + ".gamma", B, 1, 1, 256, requires_grad=False)
                dgm = fwd_desc(we, gam, Cw, 256, 1, 1, 0, 1, wC=Cw)
                self.fwd.add(lib.zsg_conv_igemm, dgm, we.buf, self.P(Wfn), gam.buf, None, None, None, None, what=prefix + "0.gamma",
                             lane=(1 if side else 2))
            if words:
                hs = self._hseq
                Dh = net.lstm_out_dim
                Kw, Vw = (self.act(prefix + nm, B, 1, self.T, 256, requires_grad=False) for nm in (".Kw", ".Vw"))
                for dst, wn, nm in ((Kw, Wkn, "0.Kw"), (Vw, Wvn, "0.Vw")):
                    dkv = fwd_desc(hs, dst, Dh, 256, 1, 1, 0, 1, wC=Dh)
                    self.fwd.add(lib.zsg_conv_igemm, dkv, hs.buf, self.P(wn), dst.buf, None, None, None, None, what=prefix + nm,
                                 lane=(1 if side else 2))
                if self.training:
                    walpha = self._buf(B * sum(hh * ww for hh, ww in sizes) * self.T)
            if Cg:
                G = self.packed(prefix + ".G", 1, sizes, 256)
                dg = fwd_desc(gridmap, G, 4, 256, 3, 1, 1, 1, wC=cp, wc0=Cf + Cw)
                self.fwd.add(lib.zsg_conv_igemm, dg, gridmap.buf, self.P(W0n), G.buf, None, None, None, None, what=prefix + "0.G", lane=side)
            if side:
                self._hoist.append((i0, len(self.fwd.calls)))
                self._join_side()
            Y = self.packed(prefix + ".Y", self.B, sizes, 256)
            d0 = fwd_desc(Fp, Y, Cf, 256, 3, 1, 1, 1, wC=cp, wc0=0, relu=False)
            a0 = (Fp.buf, self.P(W0n), Y.buf, None, None, None, None)
            wargs = None
            bf0 = (self._bf16_conv(d0, Fp.buf, self.P(W0n), cp, 0, Y.buf, None, None, L0.name + ".feat")
                   or self._bf16_train_fwd(L0.name, d0, Fp, self.P(W0n), cp, 0, Y, None, None, L0.name + ".feat"))
            if not bf0 and Fp.b16:           # (bf16_act and the bf16 entry refuses: the fp32 launch on a cast copy of the features)
                a0 = (self._f32(Fp).buf,) + a0[1:]
            if not bf0 and wino_mode() != "0":
                U0, job0 = self._wino_u(self.P(W0n).data_ptr(), 256, Cf, 9 * cp, cp, 0)
                wargs = (a0[0], U0) + a0[2:]
            if not bf0:
                self._tune("igemm", lib.zsg_conv_igemm, d0, a0, stream_ptr(), wino_args=wargs)
                if d0.use_wino:
                    self.wino_jobs["fwd"].add(*job0)
                    self.fwd.add(lib.zsg_conv_wino, d0, *wargs, what=L0.name + ".feat")
                else:
                    self.fwd.add(lib.zsg_conv_igemm, d0, *a0, what=L0.name + ".feat")
            hw = torch.tensor([v for hw_ in sizes for v in hw_], dtype=torch.int32)
            if film:
                self.fwd.add(lib.zsg_head_film_conv0, Y.buf, self.in_idx, 1, self.P(L0.name + ".bias"), G.buf if G is not None else None,
                             V.buf if V is not None else None, gam.buf, self.B, B, len(sizes), hw, 256, h1.buf, int(h1.b16), what=L0.name + ".film")
            elif words:
                self.fwd.add(lib.zsg_head_words_conv0, Y.buf, self.in_idx, 1, self.P(L0.name + ".bias"), G.buf if G is not None else None,
                             V.buf if V is not None else None, Kw.buf, Vw.buf, self.in_qlens, wscale, self.B, B, self.T, len(sizes), hw, 256, h1.buf,
                             int(h1.b16), walpha, what=L0.name + ".words")
            else:
                self.fwd.add(lib.zsg_head_shared_conv0_bf16 if h1.b16 else lib.zsg_head_shared_conv0, Y.buf, self.in_idx, 1, self.P(L0.name + ".bias"), G.buf if G is not None else None,
                             V.buf if V is not None else None, self.B, B, len(sizes), hw, 256, h1.buf, what=L0.name + ".shared")
        elif Cw or Cg:
            # None of this depends on the image: in training it runs on the side stream right behind the query encoder (the
            # launches are moved there after lowering, see _hoist_language_maps) and conv0 joins.
            side = 1 if (self.training and Cf) else 0
            i0 = len(self.fwd.calls)
            V = self.act(prefix + ".V", B, 1, 1, 9 * 256, requires_grad=False)          # stays zero without language
            if Cw:
                dv = fwd_desc(we, V, Cw, 9 * 256, 1, 1, 0, 1, wC=cp, wt_ld=cp, wc0=Cf)
                self.fwd.add(lib.zsg_conv_igemm, dv, we.buf, self.P(W0n), V.buf, None, None, None, None, what=prefix + "0.V", lane=(1 if side else 2))
            G = None
            if Cg:
                G = self.packed(prefix + ".G", 1, sizes, 256)
                dg = fwd_desc(gridmap, G, 4, 256, 3, 1, 1, 1, wC=cp, wc0=Cf + Cw)
                self.fwd.add(lib.zsg_conv_igemm, dg, gridmap.buf, self.P(W0n), G.buf, None, None, None, None, what=prefix + "0.G", lane=side)
            lmap = self.packed(prefix + ".lmap", B, sizes, 256)
            # every level in one launch (G and lmap are packed level-major with the same level list)
            hw = torch.tensor([v for hw_ in sizes for v in hw_], dtype=torch.int32)
            self.fwd.add(lib.zsg_head_lang_map_packed, V.buf, G.buf if G is not None else None, B, len(sizes), hw, 256, lmap.buf,
                         what="lmap", lane=side)
            if side:
                self._hoist.append((i0, len(self.fwd.calls)))
                self._join_side()
        if self.shared or mod:
            pass                          # (h1 is written by zsg_head_shared_conv0 / zsg_head_film_conv0 / zsg_head_words_conv0 above)
        elif Cf:
            d0 = fwd_desc(Fp, h1, Cf, 256, 3, 1, 1, 1, wC=cp, wc0=0, relu=True)
            a0 = (Fp.buf, self.P(W0n), h1.buf, self.P(L0.name + ".bias"), lmap.buf if lmap is not None else None, None, None)
            wargs = None
            bf0 = (self._bf16_conv(d0, Fp.buf, self.P(W0n), cp, 0, h1.buf, a0[3], a0[4], L0.name)
                   or self._bf16_train_fwd(L0.name, d0, Fp, self.P(W0n), cp, 0, h1, a0[3], lmap, L0.name))
            finish0 = lambda: None
            if not bf0 and (Fp.b16 or h1.b16):      # (bf16_act and the bf16 entry refuses: the fp32 launch between casts)
                f32_, h32, _, finish0 = self._via_f32(Fp, h1)
                a0 = (f32_.buf, a0[1], h32.buf) + a0[3:]
            if not bf0 and wino_mode() != "0":
                U0, job0 = self._wino_u(self.P(W0n).data_ptr(), 256, Cf, 9 * cp, cp, 0)
                wargs = (a0[0], U0) + a0[2:]
            if not bf0:
                self._tune("igemm", lib.zsg_conv_igemm, d0, a0, stream_ptr(), wino_args=wargs)
                if d0.use_wino:
                    self.wino_jobs["fwd"].add(*job0)
                    self.fwd.add(lib.zsg_conv_wino, d0, *wargs, what=L0.name)
                else:
                    self.fwd.add(lib.zsg_conv_igemm, d0, *a0, what=L0.name)
                finish0()
        else:                             # image-blind: h1 = relu(lmap + bias), an affine map with scale 1
            one, zero = self._buf(256) + 1.0, self._buf(256)
            _, h32, _, finish0 = self._via_f32(None, h1)          # (bf16_act: zsg_bn_apply writes fp32; rounded into h1 by a cast)
            self.fwd.add(lib.zsg_bn_apply, lmap.buf, h1.rows(), 256, zero, one, one, self.P(L0.name + ".bias"), None, 1, h32.buf, None,
                         what=L0.name)
            finish0()
        h1.needs_mask = True
        w0t, b0t = self.trains(W0n), self.trains(L0.name + ".bias")
        we_rg = bool(Cw) and we.requires_grad
        wft = film and self.trains(Wfn)
        wkt, wvt = words and self.trains(Wkn), words and self.trains(Wvn)
        hs_rg = words and self._hseq.requires_grad
        h1.requires_grad = bool(Cf and Fp.requires_grad) or we_rg or w0t or b0t or wft or wkt or wvt or hs_rg

        def head0_back():
            dy = h1.grad
            if dy is None:
                return
            gW0 = self.G(W0n) if w0t else None
            if not Cw and b0t:       # (with language the bias gradient falls out of the border sums below)
                self.bwd.add(lib.zsg_colsum, dy.buf, 1, 0, dy.rows(), 256, 0, 256, self.G(L0.name + ".bias"), 1, what="bgrad:" + L0.name, lane=1)
            if Cf:
                dyf = dy                 # the gradient of conv0's feature GEMM output, at the batch of the features
                dKw_ = dVw_ = None
                if words and (w0t or Fp.requires_grad or wkt or wvt or hs_rg):
                    # words: ONE call gives d(Y) per query, dYq = (1 + gamma) dy + c sum_t ds_t Kw_t, and the fp64 fixed-order sums
                    # dKw / dVw over the pixels (the forward's Y and alpha are still in place); each output only where someone reads it.
                    # Queries sharing images: the plain segmented sum of the shared plans folds dYq into the per-image accumulator.
                    need_dy = w0t or Fp.requires_grad
                    hwb = torch.tensor([v for hw_ in sizes for v in hw_], dtype=torch.int32)
                    nws = int(lib.zsg_head_words_bwd_ws_bytes(B, self.T, len(sizes), hwb.data_ptr(), 256))
                    assert nws > 0
                    wws = self._buf((nws + 7) // 8, dtype=torch.float64)
                    dYq = self.packed(prefix + ".dYq", B, sizes, 256) if need_dy else None
                    if wkt or hs_rg:
                        dKw_ = self.act(prefix + ".dKw", B, 1, self.T, 256, requires_grad=False)
                    if wvt or hs_rg:
                        dVw_ = self.act(prefix + ".dVw", B, 1, self.T, 256, requires_grad=False)
                    self.bwd.add(lib.zsg_head_words_conv0_bwd, dy.buf, Y.buf, self.in_idx, 1, Kw.buf, Vw.buf, walpha, self.in_qlens, wscale, self.B, B,
                                 self.T, len(sizes), hwb, 256, dYq.buf if need_dy else None, dKw_.buf if dKw_ is not None else None,
                                 dVw_.buf if dVw_ is not None else None, wws, nws, what=L0.name + ".words_bwd")
                    if need_dy and self.shared:
                        dyf = self.packed(prefix + ".dY", self.B, sizes, 256)
                        self.bwd.add(lib.zsg_head_shared_conv0_bwd, dYq.buf, self.in_idx, 1, self.B, B, len(sizes), hwb, 256, dyf.buf,
                                     what=L0.name + ".shared_bwd")
                    elif need_dy:
                        dyf = dYq
                elif film and (w0t or Fp.requires_grad):
                    # FiLM: d(Y)[i] = sum_{q: idx q == i} (1 + gamma[q]) * dy[q] — the segmented sum below with each query's row scaled
                    # (a plain plan: the identity index, one query per slot)
                    dyf = self.packed(prefix + ".dY", self.B, sizes, 256)
                    hwb = torch.tensor([v for hw_ in sizes for v in hw_], dtype=torch.int32)
                    self.bwd.add(lib.zsg_head_film_conv0_bwd, dy.buf, self.in_idx, 1, gam.buf, self.B, B, len(sizes), hwb, 256, dyf.buf,
                                 what=L0.name + ".film_bwd")
                elif self.shared and (w0t or Fp.requires_grad):
                    # queries sharing images: sum_q X[idx q]^T dy[q] = sum_i X[i]^T dY[i], so the feature columns of dW0 and d(Fp) take
                    # the segmented sum dY[i] = sum_{q: idx q == i} dy[q] (dy is already ReLU-masked) at batch self.B; img_idx is the
                    # forward's copy in in_idx, read by the kernel
                    dyf = self.packed(prefix + ".dY", self.B, sizes, 256)
                    hwb = torch.tensor([v for hw_ in sizes for v in hw_], dtype=torch.int32)
                    self.bwd.add(lib.zsg_head_shared_conv0_bwd, dy.buf, self.in_idx, 1, self.B, B, len(sizes), hwb, 256, dyf.buf,
                                 what=L0.name + ".shared_bwd")
                if w0t:
                    dwf = fwd_desc(Fp, dyf, Cf, 256, 3, 1, 1, 1, wC=cp, wc0=0)
                    self.wgrad(dwf, Fp, dyf, W0n, "wgrad:" + L0.name)
                if Fp.requires_grad:
                    self.dgrad(L0, dyf, Fp, n=Cf, row0=0, dx=self.grad_of(Fp))
            # The language / grid columns of dW0, the bias gradient and d(we) hang off dy only and feed nothing but the query encoder's
            # backward (itself on the side stream): with features present they are leaves of the main chain and go to the side stream,
            # so that the pyramid's backward starts right behind conv0's data gradient.
            # (not with do_norm: the language vector's normalisation has its backward on the main stream, right behind d(we))
            ln = 1 if (Cf and not (net.do_norm and Cw)) else 0
            hws_bytes = 16 << 20           # (a workspace of their own: on the main stream they ran concurrently with the side stream's slabs)
            hws = self._buf(hws_bytes // 4) if (Cw or Cg) else None
            if Cw and (w0t or b0t or we_rg):
                # (a frozen bias still receives the border sums' column total: a by-product in the flat gradient buffer, never exposed)
                # language columns of dW0 and d(we) from validity-masked sums of dy, themselves nine plain per-image sums
                S = self._buf(2 * B * 9 * 256)
                Q = self._buf(9 * B * 256)
                S1 = Act(S, B, 9 * 256, 9 * 256, [Level(0, 1, 1, 9 * 256)], "head.S1")
                S2 = Act(S, 1, B, B, [Level(B * 9 * 256, 1, 9 * 256, 9 * 256 * B)], "head.S2")
                self.bwd.add(lib.zsg_memset_f32, Q, Q.numel(), 0.0, what="zero:head.Q", lane=ln)
                for i, (h, w) in enumerate(sizes):
                    self.bwd.add(lib.zsg_head_border_sums, self.base(dy.lvl(i)), B, h, w, 256, Q, what=f"bsum{i}", lane=ln)
                self.bwd.add(lib.zsg_head_border_finalize, Q, B, 256, S, self.base(S2), self.G(L0.name + ".bias"), what="bsum.finalize", lane=ln)
                if w0t:
                    dwl = fwd_desc(we, S1, Cw, 9 * 256, 1, 1, 0, 1, wC=cp, wt_ld=cp, wc0=Cf)
                    self.bwd.add(lib.zsg_conv_wgrad, dwl, we.buf, S, gW0, 1, hws, hws_bytes, what="wgrad:" + L0.name + ".lang", lane=ln)
                if we_rg:
                    ent = net.store.entries[W0n]
                    Wrows = Act(net.store.flat, 1, Cw, cp, [Level(ent.offset + Cf, 1, 9 * 256, 9 * 256 * cp)], "head.W0rows")
                    gwe = self.grad_of(we)
                    dwe = fwd_desc(Wrows, S2, Cw, B, 1, 1, 0, 1, wC=Cw, wt_ld=Cw)
                    self.bwd.add(lib.zsg_conv_wgrad, dwe, Wrows.buf, S, self.base(gwe), int(gwe.gfilled), hws, hws_bytes, what="dwe:" + prefix, lane=ln)
                    gwe.gfilled = True
            if film and (wft or we_rg):
                # FiLM: d(gamma)[q][n] = sum_p dy[q][p][n] * Y[idx q][p][n] (fp64, fixed order; the forward's Y is still in place), then the
                # two small GEMMs d(W_gamma) += d(gamma)^T . we and d(we) += d(gamma) . W_gamma through the entries of the launches above
                hwg = torch.tensor([v for hw_ in sizes for v in hw_], dtype=torch.int32)
                nws = int(lib.zsg_head_film_dgamma_ws_bytes(B, len(sizes), hwg.data_ptr(), 256))
                assert nws > 0
                gws = self._buf(nws // 8, dtype=torch.float64)
                dgm_ = self.act(prefix + ".dgamma", B, 1, 1, 256, requires_grad=False)
                dgt = Act(self._buf(256 * B), 1, B, B, [Level(0, 1, 256, 256 * B)], prefix + ".dgamma_t")
                self.bwd.add(lib.zsg_head_film_dgamma, dy.buf, Y.buf, self.in_idx, 1, self.B, B, len(sizes), hwg, 256, dgm_.buf,
                             dgt.buf if we_rg else None, gws, nws, what="dgamma:" + prefix, lane=ln)
                if wft:
                    dwf_ = fwd_desc(we, dgm_, Cw, 256, 1, 1, 0, 1, wC=Cw)
                    self.bwd.add(lib.zsg_conv_wgrad, dwf_, we.buf, dgm_.buf, self.G(Wfn), 1, hws, hws_bytes, what="wgrad:" + prefix + ".film", lane=ln)
                    self.grad_ready[Wfn] = len(self.bwd.calls)
                if we_rg:
                    entf = net.store.entries[Wfn]
                    Wg = Act(net.store.flat, 1, Cw, Cw, [Level(entf.offset, 1, 256, 256 * Cw)], "head.Wgamma")
                    gwe = self.grad_of(we)
                    dwe2 = fwd_desc(Wg, dgt, Cw, B, 1, 1, 0, 1, wC=Cw, wt_ld=Cw)
                    self.bwd.add(lib.zsg_conv_wgrad, dwe2, Wg.buf, dgt.buf, self.base(gwe), int(gwe.gfilled), hws, hws_bytes, what="dwe.film:" + prefix,
                                 lane=ln)
                    gwe.gfilled = True
            if words and (dKw_ is not None or dVw_ is not None):
                # words: d(W_key) += dKw^T . o and d(W_value) += dVw^T . o over the [Q * T] token rows through the small-GEMM entry above;
                # d(o) = dKw . W_key + dVw . W_value through the same entry on the transposed gradients [256][Q * T] — DEFERRED: the query
                # encoder's tape replays these launches behind the pool's backward (_lower_lstm_seq), on its side stream
                hs, Dh, QT = self._hseq, net.lstm_out_dim, B * self.T
                for dkv_, wn, trn, nm in ((dKw_, Wkn, wkt, "key"), (dVw_, Wvn, wvt, "value")):
                    if trn:
                        dwk = fwd_desc(hs, dkv_, Dh, 256, 1, 1, 0, 1, wC=Dh)
                        self.bwd.add(lib.zsg_conv_wgrad, dwk, hs.buf, dkv_.buf, self.G(wn), 1, hws, hws_bytes, what=f"wgrad:{prefix}.words.{nm}", lane=ln)
                        self.grad_ready[wn] = len(self.bwd.calls)
                if hs_rg:
                    def emit_dhseq(dst, filled):
                        for dkv_, wn, nm in ((dKw_, Wkn, "key"), (dVw_, Wvn, "value")):
                            ent = net.store.entries[wn]
                            Wm = Act(net.store.flat, 1, Dh, Dh, [Level(ent.offset, 1, 256, 256 * Dh)], "head.W" + nm)
                            dt = Act(self._buf(256 * QT), 1, QT, QT, [Level(0, 1, 256, 256 * QT)], f"{prefix}.d{nm}_t")
                            self.bwd.add(lib.zsg_transpose_w, dkv_.buf, dt.buf, QT, 1, 256, QT, what=f"transpose:{prefix}.d{nm}", lane=1)
                            dho = fwd_desc(Wm, dt, Dh, QT, 1, 1, 0, 1, wC=Dh, wt_ld=Dh)
                            self.bwd.add(lib.zsg_conv_wgrad, dho, Wm.buf, dt.buf, dst, int(filled), self.wg_ws, self.wg_ws_bytes,
                                         what=f"dhseq.{nm}:{prefix}", lane=1)
                            filled = True
                    self._words_dhseq.append(emit_dhseq)
            if Cg and w0t:
                dys = self.packed(prefix + ".dysum", 1, sizes, 256)
                for i, (h, w) in enumerate(sizes):
                    self.bwd.add(lib.zsg_batch_sum, self.base(dy.lvl(i)), B, h * w * 256, self.base(dys.lvl(i)), what=f"dysum{i}", lane=ln)
                dwg = fwd_desc(gridmap, dys, 4, 256, 3, 1, 1, 1, wC=cp, wc0=Cf + Cw)
                self.bwd.add(lib.zsg_conv_wgrad, dwg, gridmap.buf, dys.buf, gW0, 1, hws, hws_bytes, what="wgrad:" + L0.name + ".grid", lane=ln)
            if w0t:
                self.grad_ready[W0n] = len(self.bwd.calls)
        self.tape.append(head0_back)
        hs = [self._head_gc(prefix, h1) if net.head_ctx == "gc" else h1]
        for i in range(1, 5):
            nxt = self.packed(f"{prefix}.h{i + 1}", B, sizes, 256, dtype=self.adt)
            self.conv(C[f"{prefix}.{i}.0"], hs[-1], relu=True, out=nxt)      # backward via the tape
            hs.append(nxt)
        L5 = C[prefix + ".5"]
        assert L5.cout == nout
        self.conv(L5, hs[-1], relu=False, out=out)
        self.tape.pop()
        if not self.training:
            return
        # ---- last conv backward: the incoming gradient is re-packed to a multiple of 4 channels (16-byte GEMM rows) -----
        npad = pad4(nout)
        P = sum(hh * ww for hh, ww in sizes)
        lvp, off = [], 0
        for (hh, ww) in sizes:
            lvp.append(Level(off * npad, hh, ww, P * npad))
            off += hh * ww
        g5p = Act(self._buf(B * P * npad), B, npad, npad, lvp, prefix + ".g5p")
        h5 = hs[-1]
        w5t, b5t = self.trains(L5.name + ".weight"), self.trains(L5.name + ".bias")
        self._head_rg = getattr(self, "_head_rg", {})
        self._head_rg[prefix] = w5t or b5t or h5.requires_grad

        def head5_back():
            if not self._head_rg[prefix]:
                return                   # (everything of this head and upstream of it is frozen)
            self.bwd.add(lib.zsg_pad_rows, g_in, B * P, nout, nout, g5p.buf, npad, what="pad g5")
            if b5t:
                # column sums of the PADDED copy (16-byte loads; its pad columns are zero and land in the 4-float storage padding)
                self.bwd.add(lib.zsg_colsum, g5p.buf, 1, 0, B * P, npad, 0, npad, self.G(L5.name + ".bias"), 1, what="bgrad:" + L5.name, lane=1)
            if w5t:
                dw = fwd_desc(h5, g5p, L5.cpad, nout, 3, 1, 1, 1, wC=L5.cpad)
                self.wgrad(dw, h5, g5p, L5.name + ".weight", "wgrad:" + L5.name)
            if h5.requires_grad:
                self.dgrad(L5, g5p, h5, n=256)
        self.tape.append(head5_back)

    def _head_gc(self, prefix: str, h1: Act) -> Act:
        """cfg head_ctx = "gc": the global-context block between h1 and `prefix`.1.0 (csrc/gcblock.hip; definition in include/zsg.h, host
        twin tests/gc_ref.py).  Per query and level, y_p = x_p + W2 relu(LN(W1 sum_p softmax_p(k . x_p) x_p + b1)) + b2 over the rows
        of the post-ReLU h1, whatever wrote it (plain, shared-image, film, words, image- or language-blind): ONE zsg_head_gc_fwd call
        (three launches) writes y, which takes h1's place as conv1's input.  fp32 under every dtype switch: a bf16_act eval plan casts
        around it (_via_f32).  A training plan keeps the logits and the per-(q, l) statistics; ONE zsg_head_gc_bwd call gives d(h1) —
        through h1's ReLU mask (_grad_sink / _grad_commit) — and the gradients of the parameters that train; it is left out when
        neither h1 nor any of the seven needs a gradient (then conv1 forms no d(y))."""
        B, sizes = self.Q, self.feat_sizes
        names = [prefix + suf for suf in GC_SUFFIXES]
        nlev, rows = len(sizes), B * sum(hh * ww for hh, ww in sizes)
        hw = torch.tensor([v for hw_ in sizes for v in hw_], dtype=torch.int32)
        y = self.packed(prefix + ".h1g", B, sizes, 256, dtype=self.adt)
        x32, y32, _, finish = self._via_f32(h1, y)
        nws = int(lib.zsg_head_gc_fwd_ws_bytes(B, nlev, hw.data_ptr(), 256))
        assert nws > 0
        ws = self._buf((nws + 3) // 4)
        s = self._buf(rows) if self.training else None
        stat = self._buf(B * nlev * GC_STAT_LD) if self.training else None
        self.fwd.add(lib.zsg_head_gc_fwd, x32.buf, *[self.P(n) for n in names], B, nlev, hw, 256, y32.buf, s, stat, ws, nws, what=prefix + ".gc")
        finish()
        trains = [self.trains(n) for n in names]
        y.needs_mask = False
        y.requires_grad = h1.requires_grad or any(trains)
        if not self.training:
            return y
        Pk, Pw1, _, Plw, _, Pw2, _ = [self.P(n) for n in names]

        def gc_back():
            g = y.grad
            if g is None:
                return
            gh, tmp = self._grad_sink(h1) if h1.requires_grad else (None, None)
            dx = None if gh is None else (tmp if tmp is not None else gh)
            nwb = int(lib.zsg_head_gc_bwd_ws_bytes(B, nlev, hw.data_ptr(), 256))
            assert nwb > 0
            wsb = self._buf((nwb + 7) // 8, dtype=torch.float64)
            grads = [self.G(n) if t else None for n, t in zip(names, trains)]
            self.bwd.add(lib.zsg_head_gc_bwd, g.buf, h1.buf, s, stat, Pk, Pw1, Plw, Pw2, B, nlev, hw, 256, dx.buf if dx is not None else None, *grads, 1,
                         wsb, nwb, what=prefix + ".gc_bwd")
            for n, t in zip(names, trains):
                if t:
                    self.grad_ready[n] = len(self.bwd.calls)
            if gh is not None:
                self._grad_commit(h1, gh, tmp)
        self.tape.append(gc_back)
        return y

    # ---- execution -------------------------------------------------------------------------------------------------------
    def run_forward(self, img, qvec, qlens, h0, c0, img_idx=None) -> torch.Tensor:
        net = self.net
        B = self.Q                               # the staged inputs and the output are per query
        n_img = self.B
        tta = self.tta and not self.training     # flip TTA: img holds half the image rows, the staging launch writes the mirrors behind them
        if tta and (B % 2 or (not self.shared and 2 * img.shape[0] != self.B)):
            raise ValueError("flip TTA: img / qvec do not fit the plan's geometry (twice the batch's rows)")
        if self.shared:
            # the batch's own image count (<= the plan's slots; the slots behind it keep what they hold and no query points to them)
            n_img = img.shape[0] * (2 if tta else 1)
            if img_idx is None or not 1 <= n_img <= self.B or qvec.shape[0] != B or (self.training and n_img != self.B):
                raise ValueError("shared-image plan: img / qvec / img_idx do not fit the plan's geometry")
            self.in_idx.copy_(img_idx, non_blocking=True)          # (device to device: no host synchronisation)
        ensure_stream_scratch(stream_ptr())      # (stream-K launches take their scratch from the stream they run on)
        do_prep = self.training and self.expect_backward and len(self.prep)
        if do_prep or len(self.prep_u):
            # the side stream's weight preparation may start now (behind the optimizer step), not behind the input copies below
            if self._prep_stream is None:
                self._prep_stream, self._prep_ev, self._u_ev = shared_side_stream(), torch.cuda.Event(), torch.cuda.Event()
            self._rel_ev.record(torch.cuda.current_stream())
        img = img.contiguous()
        u8 = img.dtype == torch.uint8
        if not u8 and img.dtype != torch.float32:
            img = img.float()
        T = qvec.shape[1]
        nd = 2 if net.bid else 1
        host_hc = h0.device.type == "cpu" and c0.device.type == "cpu"
        staged = (STAGE_INPUTS and host_hc and qvec.is_cuda and qvec.dtype == torch.float32 and qlens.is_cuda
                  and qlens.dtype in (torch.int64, torch.float32) and qlens.numel() == B)
        if staged:
            # ONE launch for the whole input staging (qvec into the zero-padded token bucket, qlens, the host-drawn h0 | c0 read straight
            # from a pinned ring slot, the BatchNorm counters): five torch operations with 5-20 us between them before (rocprofv3: 45 us
            # at the head of every forward).  A ring slot is rewritten only after the launch that read it has finished.
            if self._hc_pin is None:
                self._hc_pin = torch.empty(8, 2, nd, B, net.lstm_dim).pin_memory()
                self._hc_ev = [None] * 8
            k = self.fwd_id % 8
            if self._hc_ev[k] is not None:
                self._hc_ev[k].synchronize()
            torch.stack([h0.float(), c0.float()], out=self._hc_pin[k])
            qv, ql = qvec.contiguous(), qlens.reshape(B).contiguous()
            n_nbt = net._nbt.numel() if (self.training and not self.frozen_bn) else 0
            check(lib.zsg_stage_inputs(qv.data_ptr(), B, T, net.emb_dim, self.T, self.in_qvec.data_ptr(), ql.data_ptr(),
                                       int(ql.dtype == torch.float32), self.in_qlens.data_ptr(),
                                       self._hc_pin[k].data_ptr(), self.in_hc.numel(), self.in_hc.data_ptr(),
                                       net._nbt.data_ptr() if n_nbt else None, n_nbt, stream_ptr()), "stage_inputs")
            if self._hc_ev[k] is None:
                self._hc_ev[k] = torch.cuda.Event()
            self._hc_ev[k].record(torch.cuda.current_stream())
            self._in_keepalive = (qv, ql)
        else:
            qbuf = self.in_qvec.view(B, self.T, net.emb_dim)
            qbuf[:, :T].copy_(qvec, non_blocking=True)
            if T < self.T:
                qbuf[:, T:].zero_()
            self.in_qlens.copy_(qlens.reshape(B), non_blocking=True)
            if host_hc:     # lstm_init_hidden's two host draws: one transfer
                self.in_hc.view(2, nd, B, net.lstm_dim).copy_(torch.stack([h0.float(), c0.float()]), non_blocking=True)
            else:
                self.in_h0.view(nd, B, net.lstm_dim).copy_(h0, non_blocking=True)
                self.in_c0.view(nd, B, net.lstm_dim).copy_(c0, non_blocking=True)
        # patch the one dynamic pointer (the caller's image tensor); a flip-TTA forward does not run that launch (img holds half its rows)
        fn, args, what = self.fwd.calls[self.img_slot]
        import ctypes as C_
        if not tta:
            self.fwd.calls[self.img_slot] = (fn, (C_.c_void_p(img.data_ptr()), C_.c_int32(n_img)) + args[2:], what)
        self._img_keepalive = img
        self.fwd_id += 1
        if self.training and self.frozen_bn:
            # frozen BatchNorm layers keep num_batches_tracked: the train-mode counters only (one add; the default program stages them all)
            if getattr(self, "_nbt_inc", None) is None or self._nbt_inc.device != net._nbt.device:
                fz = set(self.frozen_bn)
                self._nbt_inc = torch.tensor([0 if n in fz else 1 for n in net.bns], dtype=net._nbt.dtype, device=net._nbt.device)
            net._nbt.add_(self._nbt_inc)
        elif self.training and not staged:
            net._nbt.add_(1)
        assert self.img_slot == 0
        if not self.training and self.fold_jobs:       # the weights may have changed since the last eval forward: refold (one launch)
            check(lib.zsg_bn_fold(net.store.flat.data_ptr(), net._rm.data_ptr(), net._rv.data_ptr(), 1e-5, self.fold_jobs_dev.data_ptr(),
                                  len(self.fold_jobs), self.fold_rows, self.fold_arena.data_ptr(), stream_ptr()), "bn_fold")
        if self.pack_jobs and not self.training:       # bf16 eval plan: the packed weight images, from the parameters and the fold just made (one launch)
            check(lib.zsg_pack_w_bf16_batched(self.pack_jobs_dev.data_ptr(), len(self.pack_jobs), self.pack_blocks, stream_ptr()), "pack_w_bf16")
        if tta:
            # the image conversion and its mirror in one launch: rows [0, n) as given, rows [n, 2n) mirrored along W
            stage = lib.zsg_tta_flip_stage_u8 if u8 else lib.zsg_tta_flip_stage_f32
            check(stage(img.data_ptr(), n_img // 2, self.H, self.W, self.fwd.calls[self.img_slot][1][5], stream_ptr()), "tta_flip_stage")
        elif u8:
            check(lib.zsg_u8hwc_to_nhwc4(img.data_ptr(), n_img * self.H * self.W, self.fwd.calls[self.img_slot][1][5], stream_ptr()), "u8hwc_to_nhwc4")
        else:
            self.fwd.run(stream_ptr(), 0, 1)          # the one launch with a per-call pointer (the caller's image)
        if do_prep or len(self.prep_u):
            # the forward's Winograd filter transforms and the backward's weight images (transposed filters of the data gradients,
            # their Winograd transforms) depend on the weights only: produced here on the side stream, under the forward
            self._prep_stream.wait_event(self._rel_ev)
            if len(self.prep_u):
                self.prep_u.run(self._prep_stream.cuda_stream)
                self._u_ev.record(self._prep_stream)

        def run_prep():
            if do_prep:
                self.prep.run(self._prep_stream.cuda_stream)
                self._prep_ev.record(self._prep_stream)
                self._prep_fwd, self._prep_pending = self.fwd_id, True
        # cut points of the forward program: (launch index, action enqueued in front of that launch)
        cuts = []
        if len(self.prep_u):
            cuts.append((self._wait_idx, lambda: torch.cuda.current_stream().wait_event(self._u_ev)))
        k_prep = self._prep_index() if do_prep else None
        if do_prep and k_prep is None:
            run_prep()             # at the head of the side stream's work
        elif do_prep:
            cuts.append((k_prep, run_prep))
        cuts.sort(key=lambda c: c[0])
        slots, out = self._out_slots(), None
        if slots:
            # the [B, A, 5] output is written straight into a FRESH tensor (the launches that produce it take its address per call), so
            # the caller owns it as with the reference's module — the copy out of the plan's static buffer (a dependent 6 us launch
            # between the head's last convolution and the loss kernels) is gone.  The slots are patched BEFORE any launch range of this
            # forward is replayed: they still hold the previous step's tensor, which may have been freed since.
            out = torch.empty(B, self.A, 5, device=self.out5.buf.device, dtype=torch.float32)
            for a in slots:
                a.value = out.data_ptr()
        pos = 1
        for idx, action in cuts:
            if idx > pos:
                self.fwd.run(stream_ptr(), pos, idx, join=False)
                pos = idx
            action()
        self.fwd.run(stream_ptr(), pos)
        if tta:
            # rows [B/2, B) are the mirrored pass: merged per anchor into the rows as given (zsg_tta_flip_merge), a fresh [B/2, A, 5]
            src = out if out is not None else self.out5.buf
            merged = torch.empty(B // 2, self.A, 5, device=src.device, dtype=torch.float32)
            lv = self._tta_levels()
            check(lib.zsg_tta_flip_merge(src.data_ptr(), B // 2, self.A, lv.ctypes.data, lv.shape[0], merged.data_ptr(), stream_ptr()),
                  "tta_flip_merge")
            return merged
        if out is not None:
            return out
        return self.out5.buf.view(B, self.A, 5).clone()

    def _tta_levels(self) -> np.ndarray:
        """the level table of zsg_tta_flip_merge, int32 [L][4] of (first anchor, h, w, anchors per cell): built once per plan"""
        if getattr(self, "_tta_lv", None) is None:
            n, rows, off = self.net.n_anchors, [], 0
            for h, w in self.feat_sizes:
                rows.append((off, h, w, n))
                off += h * w * n
            assert off == self.A, (off, self.A)
            self._tta_lv = np.ascontiguousarray(rows, dtype=np.int32)
        return self._tta_lv

    def _out_slots(self):
        """The pointer arguments of the forward program that hold the address of the [B, A, 5] output buffer (the last head convolution, or
        the two interleave launches of separate heads) — None when the address is also baked into another program of the plan: run_forward
        then copies out of the static buffer."""
        if self._out_slots_v is not False:
            return self._out_slots_v
        import ctypes as C_
        ptr, nbytes = self.out5.buf.data_ptr(), self.out5.buf.numel() * 4

        def holders(prog):
            # every pointer argument that points INTO the buffer; one at an offset cannot be re-based by value and disables the path
            return [a for _, args, _ in prog.calls for a in args if isinstance(a, C_.c_void_p) and a.value is not None and ptr <= a.value < ptr + nbytes]
        mine = holders(self.fwd)
        others = sum(len(holders(pr)) for pr in (self.bwd, self.prep, self.prep_u) if pr is not None)
        ok = (bool(mine) and all(a.value == ptr for a in mine) and not others and os.environ.get("ZSG_FRESH_OUT", "1") != "0")
        self._out_slots_v = mine if ok else None
        return self._out_slots_v

    def _prep_index(self):
        """Where in the forward program the backward's weight images (transposed / Winograd-transformed filters: ~0.2 ms of HBM-bound
        launches the backward needs, nothing in the forward does) are enqueued on the side stream: the launch index behind the 2nd join
        of the main stream with the side stream (the residual blocks' downsample branches), so that they do not sit in front of
        side-stream work the main stream waits for sooner; None = in front of everything (a network with too few joins: SSD-VGG)."""
        if self._prep_idx_v is not False:
            return self._prep_idx_v
        joins = [i for i, l in enumerate(self.fwd.lanes) if l == 2]
        self._prep_idx_v = joins[1] + 1 if len(joins) >= 4 else None       # (never behind the joins in front of the head)
        return self._prep_idx_v

    def run_backward(self, g5: torch.Tensor):
        ensure_stream_scratch(stream_ptr())
        net = self.net
        if not self.training:
            raise RuntimeError("backward through an eval-mode plan")
        # Gradients are ACCUMULATED (+=) into the flat gradient buffer, as autograd does into p.grad: the buffer is zeroed by
        # FusedAdam.zero_grad() (one memset, the p.grad views stay), or here when the p.grad were set to None.
        params = net._ordered_params()
        st = stream_ptr()
        if self.frozen:
            # p.grad views for the trainable parameters only: a frozen one keeps p.grad None (as autograd leaves it), so the
            # optimizer does not step it
            names = net._param_names
            params = [p for n, p in zip(names, params) if n not in self.frozen]
            for n, p in zip(names, net._ordered_params()):
                if n in self.frozen:
                    p.grad = None
        if any(p.grad is None for p in params):
            net._grad_reduced = False
            lib.zsg_memset_f32(net.store.grad.data_ptr(), net.store.grad.numel(), 0.0, st)
            for n, p in zip(net._param_names, net._ordered_params()):
                if n not in self.frozen:
                    p.grad = net.store.view(n, net.store.grad)
        if g5.data_ptr() != self.g5_in.data_ptr():        # (the loss wrote it in place: see ZSGNet.forward)
            self.g5_in.view_as(g5).copy_(g5)
        ddp = getattr(net, "_ddp", None)
        if self._prep_fwd == self.fwd_id and self._bwd_fwd != self.fwd_id:
            torch.cuda.current_stream().wait_event(self._prep_ev)
            self._prep_pending = False
        else:
            # no side-stream preparation for this forward, or a SECOND backward of it (retain_graph): the split-K / strided
            # data-gradient targets the first one accumulated into must be zeroed again — the preparation is idempotent
            if self._prep_fwd == self.fwd_id and self._prep_pending:
                torch.cuda.current_stream().wait_event(self._prep_ev)
                self._prep_pending = False
            self.prep.run(st)
        self._bwd_fwd = self.fwd_id
        if ddp is not None and ddp.active:
            # The reducer SUM-all-reduces the whole (accumulating) gradient buffer: a second backward before zero_grad would
            # reduce the first one's gradients again.  FusedAdam.zero_grad / dropping the p.grad clears the flag.
            if getattr(net, "_grad_reduced", False):
                raise RuntimeError("DDP: second backward without zero_grad() — gradient accumulation is not supported by the "
                                   "flat-buffer reducer (reduced gradients would be all-reduced again)")
            net._grad_reduced = True
            # average over ranks: pre-scale the incoming gradient (backward is linear), then SUM-all-reduce buckets as
            # soon as the launches that fill them are enqueued; the optimizer waits through wait_gradients().
            if not (g5.data_ptr() == self.g5_in.data_ptr() and self.g5_from_loss == (self.fwd_id, 1.0 / ddp.world)):
                self.g5_in.mul_(1.0 / ddp.world)       # (the loss kernel writes the gradient pre-scaled when it can: loss._LossFn.forward)
            self.g5_from_loss = None
            if self.reducer is None:
                from .dist import grad_spans
                self.reducer = ddp.make_reducer(grad_spans(net.store.entries, net._param_names, self.grad_ready, self.frozen))
            # (join=False: a range that ends at a bucket boundary leaves the side stream's weight gradients running; the
            # bucket's collective waits for both streams, the main stream only joins at the very end)
            nb = len(self.bwd.calls)
            self.reducer.run(nb, lambda i, j: self.bwd.run(st, i, j, join=(j == nb)), side_stream=lambda: self.bwd._side)
            self.reducer.wait()
        else:
            self.bwd.run(st)


def map_pretrained_keys(net: "ZSGNet", sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Key mapping of the two encoder initialisations of the reference's get_default_net (mdl.py:406-422):
      * 'retina'  (mdl.py:411 `tvm.resnet50(True)`): a torchvision ResNet state dict — `conv1.weight`, `bn1.*`,
        `layer1.0.conv1.weight`, ..., `fc.*` — becomes `backbone.encoder.<key>` (the unused `fc.*` is dropped);
      * 'ssd_vgg' (mdl.py:415-416 `encoder.vgg.load_state_dict(torch.load('./weights/vgg16_reducedfc.pth'))`): the
        reduced-fc VGG16 trunk — `0.weight`, `0.bias`, `2.weight`, ..., `33.bias` — becomes `backbone.encoder.vgg.<key>`.
    Full ZSGNet checkpoints (keys already `backbone.` / `att_reg_box.` / `lstm.`-prefixed, optionally under DDP's
    `module.`) pass through unchanged."""
    own = set(net.state_dict().keys())
    keys = [k[7:] if k.startswith("module.") else k for k in sd]
    if any(k in own for k in keys):
        return {k2: v for k2, v in zip(keys, sd.values())}
    prefix = "backbone.encoder.vgg." if net.backbone_kind == "ssd_vgg" else "backbone.encoder."
    return {prefix + k: v for k, v in zip(keys, sd.values()) if not k.startswith("fc.")}


def load_pretrained_encoder(net: "ZSGNet", path: str) -> int:
    """Loads an encoder / full-model checkpoint into `net`; returns the number of tensors taken.  Raises when the file
    matches NOTHING of the model (a silent no-op here would train from random weights while the log says 'pretrained')
    or when a matched tensor has the wrong shape."""
    sd = torch.load(path, map_location="cpu")
    if isinstance(sd, dict) and "model_state_dict" in sd:
        sd = sd["model_state_dict"]
    mapped = map_pretrained_keys(net, sd)
    own = net.state_dict()
    hit = {k: v for k, v in mapped.items() if k in own}
    if not hit:
        raise ValueError(f"pretrained_path={path!r}: none of its {len(sd)} tensors matches a parameter of the "
                         f"{net.backbone_kind} model (first keys: {list(sd)[:4]})")
    for k, v in hit.items():
        if tuple(v.shape) != tuple(own[k].shape):
            raise ValueError(f"pretrained_path={path!r}: {k} has shape {tuple(v.shape)}, the model expects {tuple(own[k].shape)}")
    net.load_state_dict(hit, strict=False)
    return len(hit)


def get_default_net(num_anchors=1, cfg=None):
    """Constructs the network based on the config (reference mdl.py:406-422).  'retina' = ResNet + FPN; the encoder
    depth comes from the optional cfg key `resnet_arch` (default resnet50, the reference's hard-coded choice).
    The reference initialises the encoder from torchvision's ImageNet ResNet-50 (mdl.py:411) / `vgg16_reducedfc.pth`
    (mdl.py:415-416); with no network access the same files are taken from cfg `pretrained_path` (torchvision / SSD key
    layouts are mapped by map_pretrained_keys), else the encoder is randomly initialised."""
    kind = cfg["mdl_to_use"]
    arch = cfg["resnet_arch"] if "resnet_arch" in cfg else "resnet50"
    net = ZSGNet(kind, num_anchors, cfg=cfg, arch=arch)
    net.eval_precision(cfg["eval_dtype"] if "eval_dtype" in cfg else "fp32")          # (raises on anything but fp32 / bf16 / bf16_act)
    net.eval_tta(cfg["eval_tta"] if "eval_tta" in cfg else "none")                    # (raises on anything but none / flip)
    net.eval_scales(cfg["eval_scales"] if "eval_scales" in cfg else ())               # (raises on more than 4 entries or one outside [0.5, 2])
    net.wgrad_precision(cfg["wgrad_dtype"] if "wgrad_dtype" in cfg else "fp32")       # (raises on anything but fp32 / bf16)
    net.train_precision(cfg["train_dtype"] if "train_dtype" in cfg else "fp32")       # (raises on anything but fp32 / bf16_head)
    net.encoder_precision(cfg["enc_dtype"] if "enc_dtype" in cfg else "fp32")         # (raises on anything but fp32 / bf16_fwd)
    net.encoder_backward_precision(cfg["enc_bwd_dtype"] if "enc_bwd_dtype" in cfg else "fp32")     # (raises on anything but fp32 / bf16)
    path = cfg["pretrained_path"] if "pretrained_path" in cfg else ""
    if path:
        n = load_pretrained_encoder(net, path)
        print(f"loaded {n} pretrained tensors from {path}")
    return net
