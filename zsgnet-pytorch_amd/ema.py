"""Exponential moving average of a ZSGNet's weights: torch.optim.swa_utils.AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(decay),
use_buffers=True) for a network whose parameters are views into one flat buffer (a deep copy of the module is not an option: the launch
plans hold raw pointers into params.ParamStore.flat and net._rmv).

The average is three buffers of the network's own layouts: `flat` (store.flat), `rmv` (the BatchNorm running means | variances) and `nbt`
(num_batches_tracked, copied, not averaged).  Every element follows include/zsg.h's rule  ema <- fmaf(w, p - ema, ema),  w = 1 - decay_t
in fp32; the first update after construction / reset() is a copy (w = 1).  The update count is a host integer and w travels by value: no
device read-back, no synchronisation.

update() is one zsg_ema_update launch over both float buffers.  attach(optimizer) — any optim.FusedOptimizer: FusedAdam, FusedAdamW,
FusedSGD — makes optimizer.step() do it: inside the single step launch (zsg_adam_step_ema / zsg_optim_step_ema, + one small launch for
the statistics), or — when the step goes through the segmented launch (zsg_adam_step_segments / zsg_optim_step_segments: frozen
parameters, parameter groups) — as update() over the WHOLE flat buffer after the step, so that a parameter that was trained and later
frozen keeps converging to its value.  applied() exchanges the buffers' contents with the network's (zsg_swap_f32): inside, the network
is the averaged model for every plan (the eval plans refold BatchNorm from store.flat on each forward); on exit everything is restored
bit for bit.  There is no CPU fallback: a call that would launch raises RuntimeError when the buffers are not on the GPU."""
from collections import OrderedDict
from contextlib import contextmanager

import torch

from ._lib import check, lib, stream_ptr

META_KEY = "_ema"          # state_dict()'s one extra key: {'n_averaged', 'decay', 'warmup'}


def decay_at(decay: float, warmup: bool, n: int) -> float:
    """decay of the update after n earlier ones: `decay`, or with warm-up min(decay, (1 + n) / (10 + n))"""
    return min(decay, (1.0 + n) / (10.0 + n)) if warmup else decay


class ModelEma:
    def __init__(self, model, decay: float = 0.999, warmup: bool = False):
        net = model.module if hasattr(model, "module") else model
        if not hasattr(net, "store") or not hasattr(net, "_rmv"):
            raise ValueError(f"ModelEma: {type(net).__name__} is not a ZSGNet (or its DistributedDataParallel wrapper)")
        decay = float(decay)
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"ModelEma: decay {decay} outside [0, 1]")
        self.net, self.decay, self.warmup = net, decay, bool(warmup)
        self._opt = None
        self.reset()

    @torch.no_grad()
    def reset(self):
        """Re-copies the average from the network (its current buffers, wherever they live now); the next update is a copy again."""
        net = self.net
        if net.__dict__.get("_ema_applied") is not None:
            raise RuntimeError("ModelEma.reset inside applied(): the network holds the average, not its weights")
        self.flat, self.rmv, self.nbt = net.store.flat.clone(), net._rmv.clone(), net._nbt.clone()
        self.n_averaged = 0
        self._bound = self._store_id()

    # ---- checks -----------------------------------------------------------------------------------------------------------
    def _store_id(self):
        f = self.net.store.flat
        return (f.device, f.numel(), f.data_ptr())

    def _check_launch(self, what):
        if not (self.flat.is_cuda and self.net.store.flat.is_cuda):
            raise RuntimeError(f"ModelEma.{what}: the buffers are not on the MI355X (no CPU fallback)")
        if self._store_id() != self._bound:
            raise RuntimeError(f"ModelEma.{what}: the network's parameter store was moved or reallocated after the average was taken "
                               "(model.to(...)): build the ModelEma after the move, or call reset()")
        if self.net.__dict__.get("_ema_applied") is not None:
            raise RuntimeError(f"ModelEma.{what} inside applied(): the network holds the average, not its weights")

    def _next_weight(self) -> float:
        """w of the update about to be launched (counts it)"""
        n = self.n_averaged
        self.n_averaged = n + 1
        return 1.0 if n == 0 else 1.0 - decay_at(self.decay, self.warmup, n)

    # ---- updates ----------------------------------------------------------------------------------------------------------
    def _update(self, w: float, stats_only: bool = False):
        net = self.net
        if stats_only:
            check(lib.zsg_ema_update(self.rmv.data_ptr(), net._rmv.data_ptr(), self.rmv.numel(), None, None, 0, w, stream_ptr()), "zsg_ema_update")
        else:
            check(lib.zsg_ema_update(self.flat.data_ptr(), net.store.flat.data_ptr(), self.flat.numel(), self.rmv.data_ptr(),
                                     net._rmv.data_ptr(), self.rmv.numel(), w, stream_ptr()), "zsg_ema_update")
        self.nbt.copy_(net._nbt)

    @torch.no_grad()
    def update(self):
        """One update from the network's current weights and BatchNorm statistics (call it after the optimizer's step; any optimizer)."""
        if self._opt is not None:
            raise RuntimeError("ModelEma.update: attached to an optimizer whose step() updates the average; a second update would count "
                               "the step twice (detach() first)")
        self._check_launch("update")
        self._update(self._next_weight())

    def attach(self, optimizer):
        """From now on optimizer.step() (a FusedAdam / FusedAdamW / FusedSGD of the same network) updates the average itself."""
        from .optim import FusedOptimizer
        if not isinstance(optimizer, FusedOptimizer) or optimizer.net is not self.net:
            raise ValueError("ModelEma.attach: the optimizer is not a FusedAdam of this ModelEma's network, nor another optim.FusedOptimizer "
                             "(FusedAdamW, FusedSGD) of it")
        if optimizer._ema not in (None, self):
            raise ValueError("ModelEma.attach: the optimizer already updates another average")
        self.detach()
        optimizer._ema, self._opt = self, optimizer
        return self

    def detach(self):
        if self._opt is not None:
            self._opt._ema = None
            self._opt = None

    # ---- evaluation with the average --------------------------------------------------------------------------------------
    def _swap(self):
        net = self.net
        net.join_weight_readers()          # (a forward may still be reading the weights on the side stream)
        check(lib.zsg_swap_f32(net.store.flat.data_ptr(), self.flat.data_ptr(), self.flat.numel(), stream_ptr()), "zsg_swap_f32")
        check(lib.zsg_swap_f32(net._rmv.data_ptr(), self.rmv.data_ptr(), self.rmv.numel(), stream_ptr()), "zsg_swap_f32")
        t = net._nbt.clone()
        net._nbt.copy_(self.nbt)
        self.nbt.copy_(t)

    @contextmanager
    def applied(self):
        """Inside, the network IS the averaged model (weights, BatchNorm statistics, num_batches_tracked exchanged in place: every launch
        plan keeps its pointers); on exit the raw weights and the average are back, bit for bit.  The optimizer's step, update() and a nested
        applied() raise RuntimeError inside."""
        self._check_launch("applied")
        with torch.no_grad():
            self._swap()
        self.net._ema_applied = self
        try:
            yield self
        finally:
            self.net._ema_applied = None
            with torch.no_grad():
                self._swap()

    # ---- checkpoints ------------------------------------------------------------------------------------------------------
    def _views(self):
        """the network's state_dict keys -> views of the average's buffers (the reference's names and shapes)"""
        net = self.net
        nb = self.rmv.numel() // 2
        v = {name: net.store.view(name, self.flat) for name in net._param_names}
        for i, (name, L) in enumerate(net.bns.items()):
            v[name + ".running_mean"] = self.rmv[L.index:L.index + L.c]
            v[name + ".running_var"] = self.rmv[nb + L.index:nb + L.index + L.c]
            v[name + ".num_batches_tracked"] = self.nbt[i]
        return v

    def state_dict(self):
        """The averaged model under the network's own keys (loadable into the network, or with strict=False into the reference model) plus
        META_KEY: the update count and the schedule."""
        v = self._views()
        sd = OrderedDict((k, v[k]) for k in self.net.state_dict().keys())
        sd[META_KEY] = dict(n_averaged=self.n_averaged, decay=self.decay, warmup=self.warmup)
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd):
        """Takes state_dict()'s dict, or a plain model state dict (no META_KEY: the schedule is kept, and the average counts as one update
        so that the next one averages instead of copying)."""
        sd = {(k[7:] if k.startswith("module.") else k): t for k, t in sd.items()}
        v = self._views()
        missing = [k for k in v if k not in sd]
        if missing:
            raise ValueError(f"ModelEma.load_state_dict: {len(missing)} missing keys, e.g. {missing[:3]}")
        for k, dst in v.items():
            if tuple(sd[k].shape) != tuple(dst.shape):
                raise ValueError(f"ModelEma.load_state_dict: {k} has shape {tuple(sd[k].shape)}, expected {tuple(dst.shape)}")
        for k, dst in v.items():
            dst.copy_(sd[k])
        meta = sd.get(META_KEY)
        if meta is None:
            self.n_averaged = max(self.n_averaged, 1)
        else:
            decay = float(meta["decay"])
            if not 0.0 <= decay <= 1.0:
                raise ValueError(f"ModelEma.load_state_dict: decay {decay} outside [0, 1]")
            self.n_averaged, self.decay, self.warmup = int(meta["n_averaged"]), decay, bool(meta["warmup"])
