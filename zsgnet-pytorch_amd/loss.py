"""ZSGLoss on MI355X (reference `code/loss.py`): anchor matching + focal BCE + smooth-L1, forward and backward fused
into two HIP launches (csrc/loss.hip) — no 17460^2 identity matrix, no host synchronisation, NaN branch on device."""
from functools import partial
from typing import Dict

import torch
from torch import nn

from ._lib import lib, check, stream_ptr
from .anchors import create_anchors


_ONES = {}


def _one(device) -> torch.Tensor:
    """the constant 1.0 on `device` (never written): the default upstream gradient of a scalar loss, created once instead of by a fill
    launch per backward — and recognisable in _LossFn.backward by its address"""
    key = (device.type, device.index)
    if key not in _ONES:
        _ONES[key] = torch.ones((), device=device)
    return _ONES[key]


class _LossScalar(torch.Tensor):
    """The 0-dim loss ZSGLoss returns.  The reference's trainer calls `loss.mean().backward()` on it (utils.py:412); on a 0-dim tensor
    that is a reduce launch, a fill launch for the implicit upstream gradient and a multiply — three dependent ~6 us launches between
    the loss kernels and the network's backward.  Here `.mean()` / `.sum()` of the scalar are the scalar itself and `.backward()`
    passes the cached constant 1 as the upstream gradient, which _LossFn.backward recognises: the gradient the loss kernel has
    already written into the network's incoming-gradient buffer is used as it stands — no launch at all.  Any other use (scaling the
    loss, adding losses, an explicit gradient) takes autograd's general path."""

    def mean(self, *a, **k):
        return self if (self.dim() == 0 and not a and not k) else super().mean(*a, **k)

    def sum(self, *a, **k):
        return self if (self.dim() == 0 and not a and not k) else super().sum(*a, **k)

    def __reduce_ex__(self, proto):
        return self.as_subclass(torch.Tensor).__reduce_ex__(proto)      # (pickles / torch.save as the plain tensor it is)

    def backward(self, gradient=None, retain_graph=None, create_graph=False, inputs=None):
        if gradient is None and self.dim() == 0 and not create_graph:
            gradient = _one(self.device)
        return torch.Tensor.backward(self, gradient, retain_graph, create_graph, inputs=inputs)


class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out5, mod, annot):
        B, A, _ = out5.shape
        dev = out5.device
        kind = mod.iou_kind                 # 0: the reference's criterion; 1 / 2: + lamb_iou * GIoU / DIoU loss (zsg_loss_fwd_bwd_iou)
        cls_kind = mod.cls_kind             # 0: the reference's classification term; 1 / 2: QFL / VFL on the IoU target (zsg_loss_fwd_bwd_q)
        atss = mod.matcher == "atss"        # the positives come from zsg_match_atss's mask (zsg_loss_fwd_bwd_m) instead of the fixed IoU rule
        tal = mod.matcher == "tal"          # ... from zsg_match_tal's mask: chosen from this forward's out5, a constant of the backward
        losses = torch.empty(5 if (cls_kind or atss or tal) else (4 if kind else 3), device=dev)
        # Where d(loss)/d(out5) goes: straight into the incoming-gradient buffer of the network plan that produced out5 (ZSGNet.forward
        # attaches it), already scaled by 1 / world under data parallelism (the reducer SUMs) — the backward then needs no launch of
        # its own when the upstream gradient is the constant 1.  Only the FIRST loss applied to an output may take the buffer.
        plan = getattr(out5, "_zsg_plan", None)
        buf = getattr(out5, "_zsg_g5", None)
        fast = (plan is not None and buf is not None and buf.numel() == out5.numel() and buf.device == dev and not getattr(out5, "_zsg_g5_taken", False))
        scale = 1.0
        if fast:
            out5._zsg_g5_taken = True
            grad5 = buf.view_as(out5)
            ddp = getattr(plan.net, "_ddp", None)
            if ddp is not None and ddp.active:
                scale = 1.0 / ddp.world
            plan.g5_from_loss = (plan.fwd_id, scale)
        else:
            grad5 = torch.empty_like(out5)
        mod.match_idx = torch.empty(B, dtype=torch.int32, device=dev)
        mod.npos = torch.empty(B, dtype=torch.int32, device=dev)
        wsb = lib.zsg_loss_workspace_bytes(B, A)
        ws = torch.empty((wsb + 7) // 8, dtype=torch.float64, device=dev)
        flags = (1 if mod.use_focal else 0) | (2 if mod.use_multi else 0) | (4 if mod.use_softmax else 0)
        if tal:
            mod.pos_mask = torch.empty((B, A), dtype=torch.uint8, device=dev)
            mod.tal_metric = torch.empty((B, A), dtype=torch.float64, device=dev)
            # (the keys the selection reads are the metric itself: with the metric asked for, the workspace is not touched and may be it)
            check(lib.zsg_match_tal(out5.data_ptr(), annot.data_ptr(), mod.anchs.data_ptr(), B, A, int(mod.tal_topk), float(mod.tal_alpha),
                                    float(mod.tal_beta), mod.pos_mask.data_ptr(), mod.tal_metric.data_ptr(), mod.tal_metric.data_ptr(),
                                    lib.zsg_match_tal_workspace_bytes(B, A), stream_ptr()), "zsg_match_tal")
        if atss:
            assert mod.level_off is not None and int(mod.level_off[-1]) == A, "matcher='atss' needs the level table of these anchors (set_anchors)"
            L = mod.level_off.numel() - 1
            mod.pos_mask = torch.empty((B, A), dtype=torch.uint8, device=dev)
            mod.atss_thr = torch.empty(B, dtype=torch.float64, device=dev)
            mwsb = lib.zsg_match_atss_workspace_bytes(B, L)
            mws = torch.empty((mwsb + 7) // 8, dtype=torch.float64, device=dev)
            check(lib.zsg_match_atss(annot.data_ptr(), mod.anchs.data_ptr(), mod.level_off.data_ptr(), L, B, A, int(mod.atss_topk),
                                     mod.pos_mask.data_ptr(), mod.atss_thr.data_ptr(), None, mws.data_ptr(), mwsb, stream_ptr()),
                  "zsg_match_atss")
        if atss or tal:
            check(lib.zsg_loss_fwd_bwd_m(out5.data_ptr(), annot.data_ptr(), mod.anchs.data_ptr(), B, A, mod.alpha, float(mod.gamma),
                                         float(mod.lamb_reg), float(mod.cfg["matching_threshold"]), flags, scale, kind,
                                         float(mod.lamb_iou), cls_kind, mod.pos_mask.data_ptr(), losses.data_ptr(), grad5.data_ptr(),
                                         mod.match_idx.data_ptr(), mod.npos.data_ptr(), ws.data_ptr(), wsb, stream_ptr()),
                  "zsg_loss_fwd_bwd_m")
        elif cls_kind:
            check(lib.zsg_loss_fwd_bwd_q(out5.data_ptr(), annot.data_ptr(), mod.anchs.data_ptr(), B, A, mod.alpha, float(mod.gamma),
                                         float(mod.lamb_reg), float(mod.cfg["matching_threshold"]), flags, scale, kind,
                                         float(mod.lamb_iou), cls_kind, losses.data_ptr(), grad5.data_ptr(), mod.match_idx.data_ptr(),
                                         mod.npos.data_ptr(), ws.data_ptr(), wsb, stream_ptr()), "zsg_loss_fwd_bwd_q")
        elif kind:
            check(lib.zsg_loss_fwd_bwd_iou(out5.data_ptr(), annot.data_ptr(), mod.anchs.data_ptr(), B, A, mod.alpha, float(mod.gamma),
                                           float(mod.lamb_reg), float(mod.cfg["matching_threshold"]), flags, scale, kind,
                                           float(mod.lamb_iou), losses.data_ptr(), grad5.data_ptr(), mod.match_idx.data_ptr(),
                                           mod.npos.data_ptr(), ws.data_ptr(), wsb, stream_ptr()), "zsg_loss_fwd_bwd_iou")
        else:
            check(lib.zsg_loss_fwd_bwd(out5.data_ptr(), annot.data_ptr(), mod.anchs.data_ptr(), B, A, mod.alpha, float(mod.gamma),
                                       float(mod.lamb_reg), float(mod.cfg["matching_threshold"]), flags, scale, losses.data_ptr(),
                                       grad5.data_ptr(), mod.match_idx.data_ptr(), mod.npos.data_ptr(), ws.data_ptr(), wsb,
                                       stream_ptr()), "zsg_loss_fwd_bwd")
        ctx.fast, ctx.scale, ctx.plan = fast, scale, plan
        if fast:
            ctx.grad5 = grad5                 # (the plan's own buffer: not a saved tensor — the plan enforces one backward per forward)
        else:
            ctx.save_for_backward(grad5)
        mod._last_losses = losses
        # (a view of the 3- to 5-float result, not a copy: one dependent launch less between the loss kernels and the backward)
        return losses.narrow(0, 0, 1).view(())

    @staticmethod
    def backward(ctx, g):
        if ctx.fast:
            grad5 = ctx.grad5
            if g.data_ptr() != _one(g.device).data_ptr():      # a scaled / combined loss: one in-place multiply, as before
                grad5.mul_(g)
            return grad5, None, None
        (grad5,) = ctx.saved_tensors
        return grad5 * g, None, None


class ZSGLoss(nn.Module):
    """Criterion to be minimised (reference loss.py:11-143).  forward(out, inp) -> {'loss','cls_ls','box_ls'}.
    cfg box_iou_loss = "giou" / "diou" adds lamb_iou * (that IoU loss of the decoded boxes of the positive anchors) and the key 'iou_ls'.
    cfg cls_quality = "qfl" / "vfl" trains the att logit towards the IoU of the anchor's decoded box with the annotation (Quality Focal /
    Varifocal loss in the place of the focal term) and adds the key 'pos_iou', the mean of that target over the positives (no gradient).
    cfg matcher = "atss" exchanges the fixed IoU rule for the positives with ATSS (zsg_match_atss, INTEGRATION.md "Anchor assignment");
    the mask of the last call stays in .pos_mask [B, A] uint8 and the per-sample thresholds in .atss_thr [B] float64.
    cfg matcher = "tal" exchanges it for the task-aligned assignment (zsg_match_tal on the forward's own output: the tal_topk anchors with the
    largest sigmoid(att)^tal_alpha * IoU(decoded box, annotation)^tal_beta whose centre lies inside the annotation); the mask stays in
    .pos_mask and the metric in .tal_metric [B, A] float64 (-1 where the centre lies outside)."""

    IOU_KINDS = {"none": 0, "giou": 1, "diou": 2}
    CLS_KINDS = {"none": 0, "qfl": 1, "vfl": 2}
    MATCHERS = ("iou", "atss", "tal")
    MAX_LEVELS, MAX_TOPK = 8, 16            # zsg_match_atss's limits
    TAL_MAX_TOPK = 32                       # zsg_match_tal's limit

    def __init__(self, ratios, scales, cfg):
        super().__init__()
        self.cfg = cfg
        self.ratios, self.scales = ratios, scales
        self.alpha, self.gamma = cfg["alpha"], cfg["gamma"]
        self.use_focal, self.use_softmax, self.use_multi = cfg["use_focal"], cfg["use_softmax"], cfg["use_multi"]
        self.lamb_reg = cfg["lamb_reg"]
        kind, self.lamb_iou = cfg.get("box_iou_loss", "none"), cfg.get("lamb_iou", 1.0)
        if kind not in self.IOU_KINDS:
            raise ValueError(f"box_iou_loss={kind!r}: expected one of {sorted(self.IOU_KINDS)}")
        if not self.lamb_iou >= 0:
            raise ValueError(f"lamb_iou={self.lamb_iou}: must not be negative")
        self.iou_kind = self.IOU_KINDS[kind]
        quality = cfg.get("cls_quality", "none")
        if quality not in self.CLS_KINDS:
            raise ValueError(f"cls_quality={quality!r}: expected one of {sorted(self.CLS_KINDS)}")
        self.cls_kind = self.CLS_KINDS[quality]
        if self.cls_kind:
            if self.use_softmax:
                raise ValueError(f"cls_quality={quality!r} is defined on the sigmoid branch: use_softmax must be False")
            if not self.use_focal:
                raise ValueError(f"cls_quality={quality!r} replaces the focal term: use_focal must be True")
            if not self.gamma >= 1:
                raise ValueError(f"cls_quality={quality!r} needs gamma >= 1 (gamma={self.gamma}: the derivative is singular where sigmoid = target)")
        self.matcher, self.atss_topk = cfg.get("matcher", "iou"), cfg.get("atss_topk", 9)
        if self.matcher not in self.MATCHERS:
            raise ValueError(f"matcher={self.matcher!r}: expected one of {sorted(self.MATCHERS)}")
        self.tal_topk, self.tal_alpha, self.tal_beta = cfg.get("tal_topk", 13), cfg.get("tal_alpha", 1.0), cfg.get("tal_beta", 6.0)
        if self.matcher in ("atss", "tal"):
            if not self.use_multi:
                raise ValueError(f"matcher={self.matcher!r} selects several positives per sample: use_multi must be True")
            if self.use_softmax:
                raise ValueError(f"matcher={self.matcher!r} is defined on the sigmoid branch: use_softmax must be False")
        if self.matcher == "tal":
            if not (isinstance(self.tal_topk, int) and not isinstance(self.tal_topk, bool) and 1 <= self.tal_topk <= self.TAL_MAX_TOPK):
                raise ValueError(f"tal_topk={self.tal_topk!r}: expected an integer in 1 .. {self.TAL_MAX_TOPK}")
            for key, v in (("tal_alpha", self.tal_alpha), ("tal_beta", self.tal_beta)):
                if not (isinstance(v, (int, float)) and not isinstance(v, bool) and 0 <= v < float("inf")):
                    raise ValueError(f"{key}={v!r}: expected a finite number >= 0")
        if self.matcher == "atss":
            if not (isinstance(self.atss_topk, int) and 1 <= self.atss_topk <= self.MAX_TOPK):
                raise ValueError(f"atss_topk={self.atss_topk!r}: expected an integer in 1 .. {self.MAX_TOPK}")
        self.loss_keys = ["loss", "cls_ls", "box_ls"] + (["iou_ls"] if self.iou_kind else []) + (["pos_iou"] if self.cls_kind else [])
        self.anchs = None
        self.level_off = None                    # int32 [levels + 1] in host memory: the anchor index ranges of the pyramid levels (set_anchors)
        self.get_anchors = partial(create_anchors, ratios=self.ratios, scales=self.scales, flatten=True)

    def set_anchors(self, anchs: torch.Tensor, feat_sizes) -> None:
        """the anchors [A, 4] (device, fp32, create_anchors' flattened order) together with the level table of the pyramid they were
        built from: feat_sizes = the (h, w) of every level, each level holding h * w * len(ratios) * len(scales) anchors"""
        n = len(self.ratios) * len(self.scales)
        sizes = [int(h) * int(w) * n for h, w in (feat_sizes.tolist() if torch.is_tensor(feat_sizes) else feat_sizes)]
        if not 1 <= len(sizes) <= self.MAX_LEVELS:
            raise ValueError(f"feat_sizes: {len(sizes)} pyramid levels, expected 1 .. {self.MAX_LEVELS}")
        if min(sizes) < 1 or sum(sizes) != anchs.shape[0]:
            raise ValueError(f"feat_sizes: the levels hold {sizes} = {sum(sizes)} anchors, the anchor list has {anchs.shape[0]}")
        self.anchs = anchs
        self.level_off = torch.tensor([0] + sizes, dtype=torch.int64).cumsum(0).to(torch.int32)

    def forward(self, out: Dict[str, torch.Tensor], inp: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        annot = inp["annot"].contiguous().float()
        if "att_bbx_out" in out:
            out5 = out["att_bbx_out"]
        else:                                    # a foreign model: rebuild the interleaved [B,A,5] layout
            out5 = torch.cat([out["bbx_out"], out["att_out"]], dim=2)
        out5 = out5.contiguous()
        if self.anchs is None:                   # computed once: sizes are fixed (loss.py:64-72); no .item() sync
            fs = out["feat_sizes"]
            if "num_f_out" in out and out["num_f_out"].numel() > 1:
                fs = fs[:int(out["num_f_out"][0])]
            self.set_anchors(self.get_anchors(fs, device=out5.device), fs)
        assert self.anchs.shape[0] == out5.shape[1], "anchor count does not match the network output"
        loss = _LossFn.apply(out5, self, annot)
        if loss.requires_grad:
            loss = loss.as_subclass(_LossScalar)      # (stays attached to the autograd graph; see _LossScalar)
        ls = self._last_losses
        res = {"loss": loss, "cls_ls": ls[1], "box_ls": ls[2]}
        if self.iou_kind:
            res["iou_ls"] = ls[3]
        if self.cls_kind:
            res["pos_iou"] = ls[4]
        return res


def get_default_loss(ratios, scales, cfg):
    return ZSGLoss(ratios, scales, cfg)
