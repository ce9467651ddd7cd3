"""Fused optimizers over the model's flat parameter buffer: FusedAdam (reference: torch.optim.Adam(betas=(0.9,0.99)), main_dist.py:50,
stepped at utils.py:413), FusedAdamW and FusedSGD (torch.optim.AdamW / SGD).  One HIP launch updates all 37.6 M parameters (Adam: 28 B/param
of HBM traffic) instead of ~170 per-tensor updates; the step counter lives on the device.  make_opt_fn(cfg) builds the one cfg opt_fn /
opt_fn_params name.  FusedOptimizer is what they share; the rule is the only thing a subclass adds.

Fine-tuning (torch.optim semantics): `params=` takes the model's parameters or a list of group dicts with their own hyperparameters (the
per-group keys torch takes for that optimizer; add_param_group too).  A parameter is stepped only when it is in some group AND its p.grad is
not None — a frozen parameter (requires_grad=False: the backward leaves its p.grad at None) keeps its value and state bit for bit.  With one
group and every parameter stepped, the step is the single launch (zsg_adam_step for plain FusedAdam, zsg_optim_step for every other rule);
otherwise zsg_adam_step_segments / zsg_optim_step_segments updates the listed parameters only, with per-group hyperparameters and
per-parameter step counters (torch's state['step']; a parameter's first step starts SGD's momentum buffer from its gradient).

State: FusedAdam / FusedAdamW m, v (+ vmax with amsgrad=True); FusedSGD momentum_buffer once some group has momentum != 0, else nothing.
state_dict()['zsg'] holds them with the counters and — for everything but plain FusedAdam, whose keys are m, v, step, steps — the rule's
name 'algo'; load_state_dict refuses another rule's state.  (A momentum switched on after a parameter's first step starts from a zero
buffer, where torch would start from the gradient: the two differ only with dampening != 0.)

clip_grad_norm_ is torch.nn.utils.clip_grad_norm_ over the same flat gradient buffer: two HIP launches (zsg_grad_norm, zsg_grad_scale)
through the segment table the segmented step uses, with no host round trip.

A weight average (ema.ModelEma.attach) rides in the step: inside the single launch (zsg_adam_step_ema / zsg_optim_step_ema), or as one
zsg_ema_update over the whole flat buffer behind the segmented step.  Which one follows from the path the step takes; nothing else selects it.

FusedLAMB (cfg opt_fn "LAMB") is the large-batch rule: Adam's moments with every parameter tensor's update rescaled by its trust ratio
|w| / |u| (zsg_lamb_moments + zsg_lamb_apply, always over the segment table: the rule needs the tensors' boundaries).  State m, v."""
import ctypes as C
import math

import torch

from . import mdl
from ._lib import (ADAM_CHUNK, ADAM_MAX_GROUPS, OPT_ADAM, OPT_ADAMW, OPT_AMSGRAD, OPT_SGD, AdamGroup, AdamSeg, LambGroup, OptimGroup, check,
                   lib, stream_ptr)


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


class FusedOptimizer(torch.optim.Optimizer):
    """What the fused optimizers share: the parameter index into the flat store, parameter groups, zero_grad, which parameters a step
    updates and their segment table, the step counters (one while every step updates every parameter, one per parameter once a step
    leaves some out), the weight average's hook in step(), the checkpoint's frame.  A subclass names its rule (NAME, ALGO), the group
    keys it takes (HYPER), its state buffers (_buffers) and one hyperparameter set of the C ABI (_group)."""
    NAME = None            # the rule's name in checkpoints and cfg opt_fn: 'Adam' / 'AdamW' / 'SGD' / 'LAMB'
    ALGO = None            # ZSG_OPT_*
    HYPER = ()             # group keys load_state_dict restores

    def __init__(self, model, defaults, grad_scale=1.0, params=None):
        net = model.module if hasattr(model, "module") else model
        self.net = net
        plist = net._ordered_params()
        self._index = {id(p): i for i, p in enumerate(plist)}
        super().__init__(plist if params is None else params, defaults)
        flat = net.store.flat
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
        name = type(self).__name__
        for p in ps:
            if id(p) not in index:
                shape = tuple(p.shape) if isinstance(p, torch.Tensor) else type(p).__name__
                raise ValueError(f"{name}: a tensor of shape {shape} is not a parameter of the model's flat parameter store; "
                                 "only the model's own parameters (model.parameters() or a subset) can be optimised")
        if len(self.param_groups) >= ADAM_MAX_GROUPS:
            raise ValueError(f"{name}: at most {ADAM_MAX_GROUPS} parameter groups are supported")
        self._check_group(param_group)
        super().add_param_group(param_group)

    def _check_group(self, group):
        """a ValueError for a group dict this rule cannot honour (its keys not in the dict take the defaults)"""

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
        """device segment table of the segmented step for `key` (rebuilt only when the stepped set or the groups change)"""
        if key == self._seg_key:
            return
        self._seg_tab, self._nchunks = segment_table(self.net, key)
        self._seg_key = key

    @torch.no_grad()
    def step(self, closure=None):
        if self.net.__dict__.get("_ema_applied") is not None:
            raise RuntimeError(f"{type(self).__name__}.step inside ModelEma.applied(): the network holds the averaged weights, not the "
                               "trained ones")
        ema = self._ema
        if ema is None:
            self._step(None, 0.0)
            return
        ema._check_launch("attach: step")
        w = ema._next_weight()
        if self._step(ema, w):
            ema._update(w, stats_only=True)       # the parameters' average rode in the step's launch: the BatchNorm statistics remain
        else:
            ema._update(w)                        # segmented step: the whole flat buffer, frozen parameters included

    def _step(self, ema, ema_w):
        """the update; True when the single launch took the weight average `ema` along"""
        self.net.join_weight_readers()          # (a forward without backward may still be reading the weights on the side stream)
        sel = self._stepped()
        if sel is None and self._seg and self._uniform:
            # every parameter has taken the same number of steps again: back to the single counter
            self._step2[0].copy_(self._pcount[0])
            self._pcount.zero_()
            self._seg = False
        if sel is None and not self._seg:
            self._launch_flat(self.param_groups[0], ema, ema_w)
            return ema is not None
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
        if sel:
            self._launch_segments(len(sel))
        return False

    # ---- the launches (zsg_optim_step / _ema / _segments with this rule) -----------------------------------------------------------
    def _flags(self) -> int:
        return 0

    def _buffers(self):
        """{checkpoint key: state buffer} in the C ABI's order s0, s1, s2 (allocated ones only)"""
        return {}

    def _group(self, g) -> OptimGroup:
        raise NotImplementedError

    def _state_ptrs(self):
        ptrs = [b.data_ptr() for b in self._buffers().values()]
        return ptrs + [None] * (3 - len(ptrs))

    def _launch_flat(self, g, ema, ema_w):
        st = self.net.store
        head = (self.ALGO, self._flags(), st.flat.data_ptr(), st.grad.data_ptr(), *self._state_ptrs(), st.flat.numel(), C.byref(self._group(g)),
                float(self.grad_scale), self.step_count.data_ptr())
        if ema is not None:
            check(lib.zsg_optim_step_ema(*head, ema.flat.data_ptr(), ema_w, stream_ptr()), "zsg_optim_step_ema")
        else:
            check(lib.zsg_optim_step(*head, stream_ptr()), "zsg_optim_step")

    def _launch_segments(self, nseg):
        st, n, groups = self.net.store, len(self._index), self.param_groups
        gt = (OptimGroup * len(groups))(*[self._group(g) for g in groups])
        check(lib.zsg_optim_step_segments(self.ALGO, self._flags(), st.flat.data_ptr(), st.grad.data_ptr(), *self._state_ptrs(),
                                          self._seg_tab.data_ptr(), nseg, self._nchunks, gt, len(groups), float(self.grad_scale),
                                          self._pcount.data_ptr(), self._pcount[n:].data_ptr(), stream_ptr()), "zsg_optim_step_segments")

    def param_steps(self) -> torch.Tensor:
        """steps taken by every parameter, in flat order (torch.optim's state[p]['step'])"""
        n = len(self._index)
        return (self._pcount[:n] if self._seg else self._step2[:1].expand(n)).clone()

    # ---- checkpoints ----------------------------------------------------------------------------------------------------------------
    def _describe(self) -> str:
        return self.NAME

    def _saved_meta(self):
        """what state_dict()['zsg'] holds beside the buffers and counters"""
        return dict(algo=self._describe())

    def state_dict(self):
        d = super().state_dict()
        d["zsg"] = dict(self._saved_meta(), **self._buffers(), step=self.step_count, steps=self.param_steps())
        return d

    def _load_buffers(self, z, saved):
        """copies the saved buffers in; a ValueError when one this rule needs is missing"""
        for k, b in self._buffers().items():
            if k not in z:
                raise ValueError(f"{type(self).__name__}.load_state_dict: the saved {saved} state has no '{k}' buffer, which "
                                 f"{self._describe()} needs")
            b.copy_(z[k])

    def load_state_dict(self, sd):
        """Restores the state buffers / step counters AND the param_groups' hyperparameters (lr as left by the scheduler, ...).
        A state saved before per-parameter counters existed (one 'step') gives its count to every parameter.  The state of another rule
        (or one without a buffer this rule needs) is a ValueError naming both.  A plain torch.optim state dict (a reference checkpoint)
        has per-parameter OIHW tensors that do not map onto the flat OHWI buffer: refuse it loudly instead of silently restarting."""
        name = type(self).__name__
        z = sd.get("zsg")
        if z is None:
            raise ValueError(f"{name}.load_state_dict: no 'zsg' entry — this is not a {name} state (a torch.optim.{self.NAME} "
                             "state of the reference cannot be mapped onto the flat parameter buffer); resume with load_opt=False")
        saved = z.get("algo", "Adam")          # (a state from before the rule was recorded is FusedAdam's)
        if saved != self._describe():
            raise ValueError(f"{name}.load_state_dict: the saved state belongs to {saved}, this optimizer is {self._describe()}; "
                             "resume with load_opt=False, or build the optimizer the checkpoint was written by (cfg opt_fn / opt_fn_params)")
        groups = self.param_groups
        for g, gs in zip(groups, sd.get("param_groups", [])):
            for k in self.HYPER:
                if k in gs:
                    g[k] = gs[k]
        self._load_buffers(z, saved)
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


class FusedAdam(FusedOptimizer):
    """torch.optim.Adam.  Without amsgrad it launches zsg_adam_step / zsg_adam_step_ema / zsg_adam_step_segments (csrc/adam.hip), with it
    the general entry points (csrc/optim.hip) and a third state buffer `vmax`."""
    NAME, ALGO, HYPER = "Adam", OPT_ADAM, ("lr", "betas", "eps", "weight_decay")

    def __init__(self, model, lr=1e-4, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.0, grad_scale=1.0, params=None, amsgrad=False):
        self.amsgrad = bool(amsgrad)
        super().__init__(model, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), grad_scale, params)
        flat = self.net.store.flat
        self.m = torch.zeros_like(flat)
        self.v = torch.zeros_like(flat)
        self.vmax = torch.zeros_like(flat) if self.amsgrad else None

    def _check_group(self, group):
        if "amsgrad" in group and bool(group["amsgrad"]) != self.amsgrad:
            raise ValueError(f"{type(self).__name__}: amsgrad is a property of the optimizer (amsgrad={self.amsgrad}), not of a parameter "
                             "group: one optimizer uses one update rule")

    def _flags(self):
        return OPT_AMSGRAD if self.amsgrad else 0

    def _describe(self):
        return self.NAME + (" with amsgrad" if self.amsgrad else "")

    def _buffers(self):
        return dict(m=self.m, v=self.v, vmax=self.vmax) if self.amsgrad else dict(m=self.m, v=self.v)

    def _group(self, g):
        return OptimGroup(float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]), 0.0, 0.0, 0)

    def _legacy(self):
        """the launches of csrc/adam.hip: plain Adam (what this class was before it had a base)"""
        return type(self) is FusedAdam and not self.amsgrad

    def _saved_meta(self):
        return {} if self._legacy() else super()._saved_meta()

    def _launch_flat(self, g, ema, ema_w):
        if not self._legacy():
            return super()._launch_flat(g, ema, ema_w)
        st = self.net.store
        hp = (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]), float(self.grad_scale))
        if ema is not None:
            check(lib.zsg_adam_step_ema(st.flat.data_ptr(), st.grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), st.flat.numel(), *hp,
                                        self.step_count.data_ptr(), ema.flat.data_ptr(), ema_w, stream_ptr()), "zsg_adam_step_ema")
        else:
            check(lib.zsg_adam_step(st.flat.data_ptr(), st.grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), st.flat.numel(), *hp,
                                    self.step_count.data_ptr(), stream_ptr()), "zsg_adam_step")

    def _launch_segments(self, nseg):
        if not self._legacy():
            return super()._launch_segments(nseg)
        st, n = self.net.store, len(self._index)
        gt = (AdamGroup * len(self.param_groups))(*[AdamGroup(float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                                                              float(g["weight_decay"])) for g in self.param_groups])
        check(lib.zsg_adam_step_segments(st.flat.data_ptr(), st.grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self._seg_tab.data_ptr(),
                                         nseg, self._nchunks, gt, len(self.param_groups), float(self.grad_scale),
                                         self._pcount.data_ptr(), self._pcount[n:].data_ptr(), stream_ptr()), "zsg_adam_step_segments")


class FusedAdamW(FusedAdam):
    """torch.optim.AdamW: the decay is p *= 1 - lr * weight_decay ahead of the Adam update of the unmodified gradient."""
    NAME, ALGO = "AdamW", OPT_ADAMW

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, grad_scale=1.0, params=None):
        super().__init__(model, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, grad_scale=grad_scale, params=params, amsgrad=amsgrad)


def _check_nesterov(nesterov, momentum, dampening):
    if nesterov and (momentum <= 0 or dampening != 0):
        raise ValueError("Nesterov momentum requires a momentum and zero dampening")          # (torch.optim.SGD's message)


class FusedSGD(FusedOptimizer):
    """torch.optim.SGD with momentum, dampening, weight decay and Nesterov momentum.  The momentum buffer exists once some group has
    momentum != 0 (plain SGD allocates nothing); a parameter's first step sets its part to the gradient, as torch creates it."""
    NAME, ALGO, HYPER = "SGD", OPT_SGD, ("lr", "momentum", "dampening", "weight_decay", "nesterov")

    def __init__(self, model, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, grad_scale=1.0, params=None):
        self.momentum_buffer = None
        super().__init__(model, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov), grad_scale,
                         params)
        self._ensure_buffer()

    def _check_group(self, group):
        d = self.defaults
        _check_nesterov(group.get("nesterov", d["nesterov"]), group.get("momentum", d["momentum"]), group.get("dampening", d["dampening"]))

    def _ensure_buffer(self):
        if self.momentum_buffer is None and any(float(g["momentum"]) != 0 for g in self.param_groups):
            self.momentum_buffer = torch.zeros_like(self.net.store.flat)

    def _buffers(self):
        self._ensure_buffer()          # (a group added, or a momentum set, after construction)
        return {} if self.momentum_buffer is None else dict(momentum_buffer=self.momentum_buffer)

    def _group(self, g):
        return OptimGroup(float(g["lr"]), 0.0, 0.0, 0.0, float(g["weight_decay"]), float(g["momentum"]), float(g["dampening"]),
                          1 if g["nesterov"] else 0)


class FusedLAMB(FusedOptimizer):
    """LAMB (You et al., "Large Batch Optimization for Deep Learning"; the definition in include/zsg.h, "Fused LAMB"): Adam's moments,
    and the update of every parameter tensor rescaled by its trust ratio |w| / |u|.  The rule needs the parameters' boundaries, so every
    step takes the segmented path — two launches, zsg_lamb_moments and zsg_lamb_apply (csrc/lamb.hip), over the segment table of the
    stepped parameters — and the step counts live in the per-parameter counters from the first step.  Group key `adapt` (default True):
    False gives the group's tensors the ratio 1, i.e. Adam with a coupled weight decay (biases, normalisation scales).  Frozen
    parameters, parameter groups, grad_scale, add_param_group and clip_grad_norm_ in front work as for the other rules; an attached
    weight average updates through the segmented path's zsg_ema_update.  Under DDP the norms are taken from the reduced gradients
    (run_backward returns behind reducer.wait()), in a fixed order: every rank computes the same ratios, bit for bit."""
    NAME, ALGO, HYPER = "LAMB", None, ("lr", "betas", "eps", "weight_decay", "adapt")

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, adapt=True, grad_scale=1.0, params=None):
        super().__init__(model, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, adapt=adapt), grad_scale, params)
        flat = self.net.store.flat
        self.m = torch.zeros_like(flat)
        self.v = torch.zeros_like(flat)
        self._lamb_key = None          # the stepped set the scratch below was sized for
        self._partials = self._stats = self._stepped_idx = None

    def _buffers(self):
        return dict(m=self.m, v=self.v)

    def _group(self, g):
        return LambGroup(float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                         1 if g["adapt"] else 0)

    def _stepped(self):
        """never None: LAMB has no single-launch path"""
        idx = self._index
        return tuple(sorted((idx[id(p)], gi) for gi, g in enumerate(self.param_groups) for p in g["params"] if p.grad is not None))

    def _launch_flat(self, g, ema, ema_w):
        raise RuntimeError("FusedLAMB has no single-launch path")

    def _launch_segments(self, nseg):
        st, n, groups = self.net.store, len(self._index), self.param_groups
        if self._lamb_key != self._seg_key:
            # scratch of this stepped set: the chunks' fp64 partial sums [2 * nchunks] and [ratio | |w| | |u|] per segment
            dev = st.flat.device
            self._partials = torch.empty(2 * self._nchunks, dtype=torch.float64, device=dev)
            self._stats = torch.ones(3, nseg, dtype=torch.float32, device=dev)
            self._stepped_idx = torch.tensor([i for i, _ in self._seg_key], dtype=torch.int64, device=dev)
            self._lamb_key = self._seg_key
        gt = (LambGroup * len(groups))(*[self._group(g) for g in groups])
        tab, cnt, ticket, stats = self._seg_tab.data_ptr(), self._pcount.data_ptr(), self._pcount[n:].data_ptr(), self._stats
        check(lib.zsg_lamb_moments(st.flat.data_ptr(), st.grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), tab, nseg, self._nchunks,
                                   gt, len(groups), float(self.grad_scale), cnt, self._partials.data_ptr(), ticket, stats[0].data_ptr(),
                                   stats[1].data_ptr(), stats[2].data_ptr(), stream_ptr()), "zsg_lamb_moments")
        check(lib.zsg_lamb_apply(st.flat.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), tab, nseg, self._nchunks, gt, len(groups),
                                 stats[0].data_ptr(), cnt, ticket, stream_ptr()), "zsg_lamb_apply")

    def _per_param(self, row, fill):
        out = torch.full((len(self._index),), fill, dtype=torch.float32, device=self.net.store.flat.device)
        if self._stats is not None and self._lamb_key == self._seg_key:
            out[self._stepped_idx] = self._stats[row]
        return out

    def trust_ratios(self) -> torch.Tensor:
        """the last step's trust ratio of every parameter, in flat order (1 for a parameter that step left out, and before the first
        step): a device tensor, no host synchronisation"""
        return self._per_param(0, 1.0)

    def norms(self):
        """(|w|, |u|) of the last step per parameter, in flat order (0 where trust_ratios() has its filler)"""
        return self._per_param(1, 0.0), self._per_param(2, 0.0)


OPT_FNS = {"Adam": FusedAdam, "AdamW": FusedAdamW, "SGD": FusedSGD, "LAMB": FusedLAMB}          # cfg opt_fn
OPT_FN_PARAMS = dict(betas=[0.9, 0.99], eps=1e-8, weight_decay=0.0, amsgrad=False, momentum=0.0, dampening=0.0, nesterov=False)


def lamb_param_groups(params, adapt_1d=False):
    """The groups cfg opt_fn "LAMB" trains with when the trainer names no parameters: tensors of two or more dimensions (convolution,
    linear, LSTM and embedding weights) get the trust ratio; one-dimensional ones (biases, BatchNorm scales and shifts) get adapt=False
    and no weight decay — their norms say little about a sensible step (the usual LAMB / LARS exclusion).  adapt_1d (cfg lamb_adapt_1d):
    one adaptive group of everything instead."""
    params = list(params)
    if adapt_1d:
        return [dict(params=params)]
    groups = [dict(params=[p for p in params if p.dim() >= 2]), dict(params=[p for p in params if p.dim() < 2], adapt=False, weight_decay=0.0)]
    return [g for g in groups if g["params"]]


def _make_lamb(model, lr=1e-3, params=None, grad_scale=1.0, adapt_1d=False, **hp):
    if params is None:
        net = model.module if hasattr(model, "module") else model
        params = lamb_param_groups(net._ordered_params(), adapt_1d)
    return FusedLAMB(model, lr=lr, params=params, grad_scale=grad_scale, **hp)


def make_opt_fn(cfg):
    """The optimizer factory of cfg opt_fn / opt_fn_params (reference main_dist.py:50: partial(torch.optim.Adam, betas=(0.9, 0.99))): a
    callable (model, lr=..., params=...) as trainer.Learner expects.  Keys of opt_fn_params that the chosen rule does not have are
    ignored, except that amsgrad or non-default betas with SGD are a ValueError (who sets them expects an effect).  "LAMB" reads betas,
    eps and weight_decay, and without params= builds lamb_param_groups (cfg lamb_adapt_1d)."""
    from functools import partial
    name = cfg["opt_fn"]
    if name not in OPT_FNS:
        raise ValueError(f"opt_fn {name!r} is not supported: one of {', '.join(OPT_FNS)}")
    hp = dict(OPT_FN_PARAMS, **cfg.get("opt_fn_params", {}))
    if name == "LAMB":
        return partial(_make_lamb, betas=tuple(float(b) for b in hp["betas"]), eps=float(hp["eps"]), weight_decay=float(hp["weight_decay"]),
                       adapt_1d=bool(cfg.get("lamb_adapt_1d", False)))
    if name == "SGD":
        if hp["amsgrad"] or [float(b) for b in hp["betas"]] != OPT_FN_PARAMS["betas"]:
            raise ValueError("opt_fn SGD has no amsgrad and no betas (opt_fn_params.amsgrad / opt_fn_params.betas are set): choose Adam or "
                             "AdamW, or leave them at their defaults")
        _check_nesterov(hp["nesterov"], float(hp["momentum"]), float(hp["dampening"]))
        return partial(FusedSGD, momentum=float(hp["momentum"]), dampening=float(hp["dampening"]), weight_decay=float(hp["weight_decay"]),
                       nesterov=bool(hp["nesterov"]))
    return partial(OPT_FNS[name], betas=tuple(float(b) for b in hp["betas"]), eps=float(hp["eps"]), weight_decay=float(hp["weight_decay"]),
                   amsgrad=bool(hp["amsgrad"]))


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
