"""Fused Adam over the model's flat parameter buffer (reference: torch.optim.Adam(betas=(0.9,0.99)), main_dist.py:50,
stepped at utils.py:413).  One HIP launch updates all 37.6 M parameters (28 B/param of HBM traffic) instead of ~170
per-tensor updates; the step counter lives on the device.

Fine-tuning (torch.optim semantics): `params=` takes the model's parameters or a list of group dicts with their own lr / betas /
eps / weight_decay (add_param_group too).  A parameter is stepped only when it is in some group AND its p.grad is not None — a
frozen parameter (requires_grad=False: the backward leaves its p.grad at None) keeps its value and moments bit for bit.  With one
group and every parameter stepped, the step is the single zsg_adam_step launch; otherwise zsg_adam_step_segments updates the
listed parameters only, with per-group hyperparameters and per-parameter step counters (torch's state['step']).

clip_grad_norm_ is torch.nn.utils.clip_grad_norm_ over the same flat gradient buffer: two HIP launches (zsg_grad_norm, zsg_grad_scale)
through the segment table the segmented Adam step uses, with no host round trip.

A weight average (ema.ModelEma.attach) rides in the step: inside the single launch (zsg_adam_step_ema), or as one zsg_ema_update over the
whole flat buffer behind the segmented step.  Which one follows from the path the step takes; nothing else selects it."""
import ctypes as C
import math

import torch

from . import mdl
from ._lib import ADAM_CHUNK, ADAM_MAX_GROUPS, AdamGroup, AdamSeg, check, lib, stream_ptr


def segment_table(net, key):
    """(device table, work chunks) of the segments `key` = ((parameter index, group index), ...) in flat order: the table of
    zsg_adam_step_segments, which zsg_grad_norm / zsg_grad_scale read too (group and counter unused).  Table None for an empty key."""
    ents, names = net.store.entries, net._param_names
    segs = (AdamSeg * max(1, len(key)))()
    chunk = 0
    for k, (i, gi) in enumerate(key):
        e = ents[names[i]]
        n = (e.size + 3) // 4 * 4                   # the store pads every parameter to 4 floats: step the padding as the full launch does
        assert e.offset % 4 == 0 and e.offset + n <= net.store.flat.numel()
        segs[k] = AdamSeg(e.offset, n, gi, i, chunk, 0)
        chunk += (n + ADAM_CHUNK - 1) // ADAM_CHUNK
    blob = bytes(segs)[:C.sizeof(AdamSeg) * len(key)]
    tab = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(net.store.flat.device) if key else None
    return tab, chunk


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, model, lr=1e-4, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.0, grad_scale=1.0, params=None):
        net = model.module if hasattr(model, "module") else model
        self.net = net
        plist = net._ordered_params()
        self._index = {id(p): i for i, p in enumerate(plist)}
        super().__init__(plist if params is None else params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        flat = net.store.flat
        self.m = torch.zeros_like(flat)
        self.v = torch.zeros_like(flat)
        self._step2 = torch.zeros(2, dtype=torch.int32, device=flat.device)      # [steps taken, the update kernel's completion ticket]
        self.step_count = self._step2[:1]
        self.grad_scale = grad_scale
        # per-parameter step counters of the segmented path [n params | its completion ticket].  While _seg is False every parameter has
        # taken step_count steps (the single-launch path counts for all); once a step leaves some parameter out, the counts move here.
        self._pcount = torch.zeros(len(plist) + 1, dtype=torch.int32, device=flat.device)
        self._seg, self._uniform = False, True
        self._seg_key, self._seg_tab, self._nchunks = None, None, 0
        self._ema = None          # ema.ModelEma.attach: step() updates this weight average

    def add_param_group(self, param_group):
        """torch's add_param_group, restricted to parameters of the model's flat store (the kernels address them by offset)."""
        ps = param_group["params"]
        ps = [ps] if isinstance(ps, torch.Tensor) else list(ps)
        param_group = dict(param_group, params=ps)          # (an iterator is consumed here once)
        index = self.__dict__.get("_index", {})
        for p in ps:
            if id(p) not in index:
                shape = tuple(p.shape) if isinstance(p, torch.Tensor) else type(p).__name__
                raise ValueError(f"FusedAdam: a tensor of shape {shape} is not a parameter of the model's flat parameter store; "
                                 "only the model's own parameters (model.parameters() or a subset) can be optimised")
        if len(self.param_groups) >= ADAM_MAX_GROUPS:
            raise ValueError(f"FusedAdam: at most {ADAM_MAX_GROUPS} parameter groups are supported")
        super().add_param_group(param_group)

    def zero_grad(self, set_to_none: bool = False):
        """One memset of the flat gradient buffer; the p.grad views stay (backward accumulates into them).  With
        set_to_none=True the views are dropped instead and the next backward re-creates them."""
        if set_to_none:
            for p in self.net._ordered_params():
                p.grad = None
            return
        st = self.net.store
        self.net._grad_reduced = False          # (DDP: one reduced backward per zero_grad, see _Plan.run_backward)
        if st.grad is not None and st.grad.is_cuda:
            check(lib.zsg_memset_f32(st.grad.data_ptr(), st.grad.numel(), 0.0, stream_ptr()), "zero_grad")

    # ---- which parameters a step updates ------------------------------------------------------------------------------
    def _stepped(self):
        """(parameter index, group index) of every parameter this step updates, in flat order, or None when that is ALL of them in one
        group (the single-launch path)."""
        groups = self.param_groups
        if len(groups) == 1 and len(groups[0]["params"]) == len(self._index):
            if all(p.grad is not None for p in groups[0]["params"]):
                return None
        idx = self._index
        return tuple(sorted((idx[id(p)], gi) for gi, g in enumerate(groups) for p in g["params"] if p.grad is not None))

    def _segment_table(self, key):
        """device segment table of zsg_adam_step_segments for `key` (rebuilt only when the stepped set or the groups change)"""
        if key == self._seg_key:
            return
        self._seg_tab, self._nchunks = segment_table(self.net, key)
        self._seg_key = key

    @torch.no_grad()
    def step(self, closure=None):
        if self.net.__dict__.get("_ema_applied") is not None:
            raise RuntimeError("FusedAdam.step inside ModelEma.applied(): the network holds the averaged weights, not the trained ones")
        ema = self._ema
        if ema is None:
            self._step(None, 0.0)
            return
        ema._check_launch("attach: step")
        w = ema._next_weight()
        if self._step(ema, w):
            ema._update(w, stats_only=True)       # the parameters' average rode in the Adam launch: the BatchNorm statistics remain
        else:
            ema._update(w)                        # segmented step: the whole flat buffer, frozen parameters included

    def _step(self, ema, ema_w):
        """the Adam update; True when the single launch took the weight average `ema` along (zsg_adam_step_ema)"""
        st = self.net.store
        self.net.join_weight_readers()          # (a forward without backward may still be reading the weights on the side stream)
        sel = self._stepped()
        if sel is None and self._seg and self._uniform:
            # every parameter has taken the same number of steps again: back to the single counter
            self._step2[0].copy_(self._pcount[0])
            self._pcount.zero_()
            self._seg = False
        if sel is None and not self._seg:
            g = self.param_groups[0]
            hp = (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]), float(self.grad_scale))
            if ema is not None:
                check(lib.zsg_adam_step_ema(st.flat.data_ptr(), st.grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), st.flat.numel(), *hp,
                                            self.step_count.data_ptr(), ema.flat.data_ptr(), ema_w, stream_ptr()), "zsg_adam_step_ema")
                return True
            check(lib.zsg_adam_step(st.flat.data_ptr(), st.grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), st.flat.numel(), *hp,
                                    self.step_count.data_ptr(), stream_ptr()), "zsg_adam_step")
            return False
        if sel is None:
            sel = tuple((i, 0) for i in range(len(self._index)))
        if not self._seg:                        # the counts move to the per-parameter counters
            n = len(self._index)
            self._pcount[:n].copy_(self._step2[:1].expand(n))
            self._step2[0].zero_()
            self._seg, self._uniform = True, True
        if len(sel) < len(self._index):
            self._uniform = False
        self._segment_table(sel)
        if not sel:
            return False
        gt = (AdamGroup * len(self.param_groups))(*[AdamGroup(float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                                                              float(g["weight_decay"])) for g in self.param_groups])
        n = len(self._index)
        check(lib.zsg_adam_step_segments(st.flat.data_ptr(), st.grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self._seg_tab.data_ptr(),
                                         len(sel), self._nchunks, gt, len(self.param_groups), float(self.grad_scale),
                                         self._pcount.data_ptr(), self._pcount[n:].data_ptr(), stream_ptr()), "zsg_adam_step_segments")
        return False

    def param_steps(self) -> torch.Tensor:
        """steps taken by every parameter, in flat order (torch.optim.Adam's state[p]['step'])"""
        n = len(self._index)
        return (self._pcount[:n] if self._seg else self._step2[:1].expand(n)).clone()

    def state_dict(self):
        d = super().state_dict()
        d["zsg"] = dict(m=self.m, v=self.v, step=self.step_count, steps=self.param_steps())
        return d

    def load_state_dict(self, sd):
        """Restores the moments / step counters AND the param_groups (lr as left by the scheduler, betas, eps, weight decay).
        A state saved before per-parameter counters existed (one 'step') gives its count to every parameter.
        A plain torch.optim.Adam state dict (a reference checkpoint) has per-parameter OIHW moments that do not map onto
        the flat OHWI buffer: refuse it loudly instead of silently restarting the moments."""
        z = sd.get("zsg")
        if z is None:
            raise ValueError("FusedAdam.load_state_dict: no 'zsg' entry — this is not a FusedAdam state (a torch.optim.Adam "
                             "state of the reference cannot be mapped onto the flat parameter buffer); resume with load_opt=False")
        self.m.copy_(z["m"])
        self.v.copy_(z["v"])
        steps = z.get("steps")
        n = len(self._index)
        self._pcount.zero_()
        if steps is not None and steps.numel() == n and bool((steps != steps.reshape(-1)[0]).any()):
            self._pcount[:n].copy_(steps.to(self._pcount.dtype))
            self._step2.zero_()
            self._seg, self._uniform = True, False
        else:
            cnt = z["step"] if steps is None or steps.numel() != n else steps.reshape(-1)[:1]
            self.step_count.copy_(cnt.to(self.step_count.dtype))
            self._seg, self._uniform = False, True
        saved = sd.get("param_groups", [])
        for g, gs in zip(self.param_groups, saved):
            for k in ("lr", "betas", "eps", "weight_decay"):
                if k in gs:
                    g[k] = gs[k]


# ---- gradient-norm clipping ---------------------------------------------------------------------------------------------------------
def _flat_owner(tensors):
    """(the ZSGNet whose flat store holds every tensor, its {id(parameter): flat index}); (None, None) for no tensors.  Any other tensor
    is a ValueError, as FusedAdam.add_param_group rejects it (the kernels address gradients by their offset in the flat buffer)."""
    net = index = None
    for p in tensors:
        if index is not None and id(p) in index:
            continue
        owner = next((n for n in list(mdl.LIVE_NETS) if id(p) in n._param_index()), None)
        if owner is None or (net is not None and owner is not net):
            shape = tuple(p.shape) if isinstance(p, torch.Tensor) else type(p).__name__
            raise ValueError(f"clip_grad_norm_: a tensor of shape {shape} is not a parameter of " +
                             ("a ZSGNet's flat parameter store" if owner is None else "the same ZSGNet as the others") +
                             "; only one model's own parameters (model.parameters() or a subset) can be clipped")
        net, index = owner, owner._param_index()
    return net, index


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm: float, norm_type: float = 2.0, error_if_nonfinite: bool = False, foreach=None) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_ for the parameters of a ZSGNet (any subset, e.g. net.lstm.parameters()): the total norm of the
    gradients of the given parameters whose p.grad is not None (a parameter listed twice counts once), and those gradients scaled in place
    by clamp(max_norm / (total_norm + 1e-6), max=1.0).  Frozen parameters (p.grad None) and the flat buffer's by-products that are never a
    p.grad (a frozen BatchNorm's d(gamma) / d(beta)) are neither counted nor scaled.

    Two launches on torch's current stream: zsg_grad_norm (fp64 sums of squares, a fixed reduction order: the same bits on every run and
    every rank given the same gradients) writes the norm and the coefficient to the device; zsg_grad_scale reads the coefficient there and
    writes nothing when it is 1.  No host synchronisation unless error_if_nonfinite=True.  No extra stream wait is needed: run_backward
    returns with the main stream joined to the side stream's weight gradients (ops.Program.run, join at the end of the range) and, under
    DDP, behind every bucket's all-reduce (the reducer's wait() runs inside run_backward).

    norm_type: 2 or inf (ValueError otherwise).  foreach: accepted for torch's signature; the fused kernels serve every value.
    Returns the total norm, a 0-dim fp32 tensor on the model's device allocated for this call (tensor(0.) when no gradient is listed:
    nothing is launched)."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    else:
        parameters = list(parameters)
    norm_type = float(norm_type)
    if norm_type not in (2.0, math.inf):
        raise ValueError(f"clip_grad_norm_: norm_type {norm_type} is not supported (2.0 or inf)")
    net, index = _flat_owner(parameters)
    sel = tuple(sorted({index[id(p)] for p in parameters if p.grad is not None}))
    if not sel:
        return torch.tensor(0.0)
    st = net.store
    cache = net.__dict__.get("_clip_scratch")
    if cache is None or cache[0] != (sel, st.grad.data_ptr()):
        if not st.grad.is_cuda:
            raise RuntimeError("clip_grad_norm_: the model's gradients are not on the MI355X (no CPU fallback)")
        plist, base = net._ordered_params(), st.grad.untyped_storage().data_ptr()
        for i in sel:
            if plist[i].grad.untyped_storage().data_ptr() != base:
                raise ValueError(f"clip_grad_norm_: the p.grad of {net._param_names[i]} is not a view of the model's flat gradient buffer")
        tab, nch = segment_table(net, tuple((i, 0) for i in sel))
        # the segment table, one fp64 partial per work chunk and the completion ticket (zero between launches): built once per set of
        # parameters with gradients, reused while it does not change
        cache = ((sel, st.grad.data_ptr()), tab, nch, torch.empty(nch, dtype=torch.float64, device=st.grad.device),
                 torch.zeros(1, dtype=torch.int32, device=st.grad.device))
        net._clip_scratch = cache
    _, tab, nch, partials, ticket = cache
    res = torch.empty(2, dtype=torch.float32, device=st.grad.device)          # [total_norm, clip_coef]
    check(lib.zsg_grad_norm(st.grad.data_ptr(), tab.data_ptr(), len(sel), nch, 1 if norm_type == math.inf else 0, float(max_norm),
                            partials.data_ptr(), ticket.data_ptr(), res.data_ptr(), stream_ptr()), "zsg_grad_norm")
    total = res[0]
    if error_if_nonfinite and not bool(torch.isfinite(total)):
        raise RuntimeError(f"The total norm of order {norm_type} for gradients from `parameters` is non-finite, so it cannot be clipped. "
                           "To disable this error and scale the gradients by the non-finite norm anyway, set `error_if_nonfinite=False`")
    check(lib.zsg_grad_scale(st.grad.data_ptr(), tab.data_ptr(), len(sel), nch, res.data_ptr() + 4, stream_ptr()), "zsg_grad_scale")
    return total
