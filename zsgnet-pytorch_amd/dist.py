"""Data parallelism for the MI355X ZSGNet step: one process per GPU, gradients all-reduced with RCCL over xGMI.

Reference: main_dist.py:36-40 wraps the model in torch DistributedDataParallel (NCCL, broadcast_buffers=True); the
collectives are C1-C3 of SURVEY.md §2.2.  Here the gradients already live in ONE flat buffer in parameter order, so the
reducer is a handful of large in-place all-reduces on contiguous slices ("buckets", a few tens of MB each: xGMI is
point-to-point, ring collectives are per-link bound, so few large messages beat many small ones).  A bucket is launched
as soon as the last backward launch that writes into it has been enqueued, on RCCL's own stream (torch.distributed
fences it against the compute stream with events), so communication overlaps the rest of backward; the optimizer waits
on all of them.  The same code runs on CPU tensors over gloo, which is how it is tested without GPUs.
"""
import os
from dataclasses import dataclass
from typing import Any, Callable, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist
from torch import nn


def get_world_size() -> int:
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def get_rank() -> int:
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def is_main_process() -> bool:
    return get_rank() == 0


def synchronize():
    """utils.py:47-59"""
    if get_world_size() > 1:
        dist.barrier()


def init_process_group_from_env(backend: Optional[str] = None):
    """env:// rendezvous (torchrun / torch.distributed.launch): RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT, LOCAL_RANK."""
    if dist.is_initialized() or int(os.environ.get("WORLD_SIZE", "1")) <= 1:
        return
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if backend is None:
        backend = "nccl" if torch.cuda.is_available() else "gloo"
    if backend == "nccl":
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count()))
    dist.init_process_group(backend=backend, init_method="env://")


@dataclass
class Bucket:
    start: int          # element range [start, end) of the flat gradient buffer
    end: int
    ready: int          # index of the last backward launch that writes into the range (-1: nothing writes)


def plan_buckets(spans: Sequence[Tuple[int, int, int]], target_elems: int, tail_elems: Optional[int] = None) -> List[Bucket]:
    """spans: (offset, size, ready_index) per parameter in flat order.  Adjacent parameters are merged up to
    ~target_elems; the result covers the flat buffer exactly once and is sorted by readiness so buckets are launched in
    completion order.  tail_elems: the bucket that completes LAST (it holds the first layers of the network, whose
    gradients are written at the very end of backward) cannot overlap with anything, so its latest part is split off
    into a small bucket of ~tail_elems and only that small all-reduce is exposed."""
    groups: List[List[Tuple[int, int, int]]] = []
    for sp in sorted(spans):
        if groups and groups[-1][-1][0] + groups[-1][-1][1] == sp[0] and sum(x[1] for x in groups[-1]) < target_elems:
            groups[-1].append(sp)
        else:
            groups.append([sp])
    if tail_elems and groups:
        gi = max(range(len(groups)), key=lambda i: max(x[2] for x in groups[i]))
        g = groups[gi]
        if sum(x[1] for x in g) > 2 * tail_elems and len(g) > 1:
            k = max(range(len(g)), key=lambda i: g[i][2])           # the parameter written last
            j, acc = k, 0
            while j < len(g) and acc < tail_elems:
                acc += g[j][1]
                j += 1
            pieces = [p for p in (g[:k], g[k:j], g[j:]) if p]
            groups[gi:gi + 1] = pieces
    buckets = [Bucket(g[0][0], g[-1][0] + g[-1][1], max(x[2] for x in g)) for g in groups]
    return sorted(buckets, key=lambda b: (b.ready, b.start))


def grad_spans(entries, names: Sequence[str], grad_ready, frozen=()) -> List[Tuple[int, int, int]]:
    """(offset, padded size, ready index) of every parameter whose gradient the reducer all-reduces, in flat order: the trainable
    ones only — no bucket covers a frozen span (torch DDP skips requires_grad=False parameters).  entries: ParamStore.entries;
    grad_ready: the last backward launch that writes each gradient (-1 / missing: none)."""
    return [(entries[n].offset, (entries[n].size + 3) // 4 * 4, grad_ready.get(n, -1)) for n in names if n not in frozen]


class NativeComm:
    """The C-ABI communicator (include/zsg.h zsg_comm_*): RCCL bound inside libzsg.so, its own HIP stream and events.
    Rank 0 creates the ncclUniqueId; it travels over the already-initialised torch.distributed group (the rendezvous
    store of torchrun), then every rank calls ncclCommInitRank on its own device."""

    def __init__(self, group=None):
        import ctypes as C
        from ._lib import check, lib
        self._lib, self._check, self._C = lib, check, C
        world, rank = get_world_size(), get_rank()
        ident = C.create_string_buffer(128)
        if rank == 0:
            check(lib.zsg_comm_unique_id(ident), "zsg_comm_unique_id")
        ids = [ident.raw]
        if world > 1:
            dist.broadcast_object_list(ids, src=0, group=group)
        self.handle = C.c_void_p()
        check(lib.zsg_comm_init(C.byref(self.handle), ids[0], world, rank), "zsg_comm_init")

    @staticmethod
    def _stream() -> int:
        return torch.cuda.current_stream().cuda_stream

    def all_reduce(self, t: torch.Tensor):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        self._check(self._lib.zsg_comm_allreduce_bucket(self.handle, t.data_ptr(), t.numel(), self._C.c_void_p(self._stream())), "zsg_comm_allreduce_bucket")

    def broadcast(self, t: torch.Tensor, src: int = 0):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        self._check(self._lib.zsg_comm_broadcast(self.handle, t.data_ptr(), t.numel(), src, self._C.c_void_p(self._stream())), "zsg_comm_broadcast")

    def wait(self):
        self._check(self._lib.zsg_comm_wait(self.handle, self._C.c_void_p(self._stream())), "zsg_comm_wait")

    def close(self):
        if self.handle:
            self._check(self._lib.zsg_comm_destroy(self.handle), "zsg_comm_destroy")
            self.handle = None


class BucketReducer:
    """Sum-all-reduce of a flat buffer in buckets, interleaved with a list of launches.  comm: a NativeComm (RCCL
    through the C ABI) or None (torch.distributed.all_reduce on `group`: nccl = RCCL on GPUs, gloo in the CPU tests)."""

    def __init__(self, flat: torch.Tensor, buckets: List[Bucket], group=None, comm: Optional["NativeComm"] = None):
        self.flat, self.buckets, self.group, self.comm = flat, buckets, group, comm
        self.pending = []
        self.time_wait = False          # bench.py: bracket wait() with events — how long the compute stream stands behind the last bucket
        self.wait_events = []

    def run(self, n_launches: int, launch_range: Callable[[int, int], None], side_stream: Optional[Callable[[], Any]] = None):
        """launch_range(i, j) enqueues launches [i, j).  After the launch with index b.ready, bucket b is reduced.
        side_stream() (optional): a second compute stream that launch_range also enqueues on (the weight-gradient kernels) and
        does NOT join at the end of a range — the collective is then issued from that stream once it has caught up with the
        main stream, and the critical chain on the main stream never waits for the weight gradients at a bucket boundary (the join cost 0.67 ms of a
        15.5 ms step in a 1-rank group)."""
        done = 0
        for b in self.buckets:
            upto = min(max(b.ready + 1, done), n_launches)
            if upto > done:
                launch_range(done, upto)
                done = upto
            t = self.flat[b.start:b.end]
            side = side_stream() if side_stream is not None else None
            if side is not None and t.is_cuda:
                # issued from the side stream after it has caught up with the main stream: the collective is then ordered after
                # BOTH (no third stream: HIP streams share 4 hardware queues, see ops.shared_side_stream)
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    self._reduce(t)
            else:
                self._reduce(t)
        if done < n_launches:
            launch_range(done, n_launches)

    def _reduce(self, t: torch.Tensor):
        if self.comm is not None:
            self.comm.all_reduce(t)
        else:
            self.pending.append(dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group, async_op=True))

    def wait(self):
        ev = None
        if self.time_wait and self.flat.is_cuda:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()              # completes with the backward's last launch on the compute stream
        if self.comm is not None:
            self.comm.wait()
        for w in self.pending:
            w.wait()
        self.pending = []
        if ev is not None:
            ev[1].record()              # completes once the stream has passed the waits: the difference is the EXPOSED all-reduce time
            self.wait_events.append(ev)

    def exposed_ms(self) -> Optional[float]:
        """mean time the compute stream waited for the collectives per backward, over the brackets collected while time_wait was set"""
        if not self.wait_events:
            return None
        torch.cuda.synchronize()
        v = [a.elapsed_time(b) for a, b in self.wait_events]
        self.wait_events = []
        return sum(v) / len(v)


class DistributedDataParallel(nn.Module):
    """Drop-in for torch.nn.parallel.DistributedDataParallel(mdl, device_ids=[local_rank], broadcast_buffers=True) at
    main_dist.py:36-40, specialised to the flat-buffer ZSGNet: parameters are broadcast from rank 0 at construction
    (C3), BatchNorm running statistics before every training forward (C2), gradients are averaged by the bucketed
    reducer during backward (C1)."""

    def __init__(self, module: nn.Module, device_ids=None, output_device=None, broadcast_buffers: bool = True,
                 find_unused_parameters: bool = False, bucket_mb: float = 32.0, process_group=None, tail_bucket_mb: float = 4.0,
                 comm: Optional[str] = None, force_collectives: bool = False):
        """comm: 'torch' (torch.distributed.all_reduce / broadcast on the process group: ProcessGroupNCCL = RCCL) or
        'native' (zsg_comm_* of the C ABI: RCCL bound inside libzsg.so on its own stream); default from ZSG_COMM, else
        'torch'.  force_collectives: issue every collective even in a 1-rank group (tests / smoke runs of the RCCL path)."""
        super().__init__()
        self.module = module
        self.broadcast_buffers = broadcast_buffers
        self.group = process_group
        self.bucket_elems = int(bucket_mb * (1 << 20) / 4)
        self.tail_elems = int(tail_bucket_mb * (1 << 20) / 4)
        self.world = get_world_size()
        self.active = self.world > 1 or force_collectives
        kind = comm if comm is not None else os.environ.get("ZSG_COMM", "torch")
        if not isinstance(kind, str):      # a communicator object with NativeComm's interface (all_reduce / broadcast / wait / close): tests
            self.comm = kind if self.active else None
        else:
            if kind not in ("torch", "native"):
                raise ValueError(f"comm={kind!r}: expected 'torch' or 'native'")
            self.comm = NativeComm(process_group) if (kind == "native" and self.active) else None
        self._tuned = set()
        object.__setattr__(module, "_ddp", self)      # plain attribute: registering it as a sub-module would create a cycle
        if self.active:
            self._bcast(module.store.flat)
            self._sync_buffers(counters=True)

    def _bcast(self, t: torch.Tensor):
        if self.comm is not None and t.dtype == torch.float32:
            self.comm.broadcast(t, 0)
        else:
            dist.broadcast(t, src=0, group=self.group)

    def _sync_buffers(self, counters: bool = False):
        """C2 of the reference's DDP (broadcast_buffers=True): rank 0's BatchNorm running statistics before every training
        forward — all 53 layers' means and variances live in one buffer, so this is ONE broadcast (~0.2 MB).  The
        num_batches_tracked counters advance identically on every rank; they are sent once, at wrap time."""
        m = self.module
        self._bcast(m._rmv)
        if counters:
            dist.broadcast(m._nbt, src=0, group=self.group)

    def _sync_tuning(self, inp):
        """Rank 0 lowers (and autotunes) the launch plan of a new input geometry first and broadcasts its tile choices; the other
        ranks lower from that table.  Every rank then runs the SAME kernel variant for the same layer (each rank tuning on its own
        would pick by its own timing noise — harmless for the all-reduced gradients, but not reproducible, and 8x the tuning time).

        The decision to run the broadcast must be the same on every rank, so it is keyed on what all ranks share at a given step —
        (B, H, W, training): equal-sized shards (DistributedSampler pads), one mode — and NOT on the query-length bucket: the collater
        cuts qvec to the batch's longest query (dat_loader.py, as the reference's), so T_plan (20 / 50) differs from rank to rank
        and step to step.  (Keyed on T, a rank that met a bucket earlier than its peers skipped the broadcast they were waiting
        in: mismatched collectives.)  Rank 0 lowers the plan of ITS current bucket; the image branch — everything the autotuner
        touches — does not depend on T.  The T-dependent launches (the query encoder's input projections and their weight gradients,
        mdl._Plan._lower_lstm) are lowered with tile_hint 0, i.e. the library's deterministic shape heuristic, never the tuner: a rank
        that later meets the other bucket lowers exactly the launches its peers lower for it, so the promise above holds for every
        launch of the step (ADVICE r04 item 4 asked for rank 0 to lower both buckets: nothing of the second bucket is tuned)."""
        if not hasattr(self.module, "plan_geometry"):
            return
        from . import ops
        geo = self.module.plan_geometry(inp)
        shared = inp.get("img_idx") is not None
        if shared and not (self.module.training and getattr(self.module, "_shared_train", False) and len(geo) == 5
                           and not (hasattr(self.module, "_sync_bn_key") and self.module._sync_bn_key())):
            # queries sharing images in eval mode: the number of distinct images, hence the plan, differs from rank to rank and batch to
            # batch, so no decision about a collective can be keyed on it; every rank tunes its own plans.  (Nor for the blind variants,
            # which gather into the plain plan, or a training batch the forward is about to refuse.)
            return
        if shared:
            # a shared TRAINING batch: the grouped training loader gives every rank the same (Bi, Q), so the broadcast is keyed on
            # (Bi, Q, H, W, training, ...) — again not on the query-length bucket; rank 0 lowers the shared plan of ITS bucket
            key = ("shared",) + tuple(geo[:4]) + (True,)
        else:
            key = tuple(geo[:3]) + (self.module.training,)
        if self.module.training and hasattr(self.module, "_frozen_bn_key"):
            key += (self.module._frozen_bn_key(),)       # (frozen BatchNorm layers lower other launches: tuned anew, broadcast anew)
        if self.module.training and hasattr(self.module, "_sync_bn_key"):
            key += (self.module._sync_bn_key(),)         # (so do synchronized ones: no in-kernel statistics finalize)
        if self.module.training and getattr(self.module, "_wgrad_dtype", "fp32") != "fp32":
            key += (("wgrad", self.module._wgrad_dtype),)    # (bf16 weight gradients are tuned under their own entries)
        if self.module.training and getattr(self.module, "_train_dtype", "fp32") != "fp32":
            key += (("train", self.module._train_dtype),)    # (so are the bf16 forward convolutions / data gradients of the pyramid and the heads)
        if self.module.training and getattr(self.module, "_enc_dtype", "fp32") != "fp32":
            key += (("enc", self.module._enc_dtype),)        # (and the encoder's bf16 forward convolutions)
        if self.module.training and getattr(self.module, "_enc_bwd_dtype", "fp32") != "fp32":
            key += (("encb", self.module._enc_bwd_dtype),)   # (and the encoder's bf16 data gradients)
        if key in self._tuned:
            return
        self._tuned.add(key)
        if shared:
            if get_rank() == 0:
                Bi, Q, H, W, Tp = geo
                self.module._plan_for(Bi, H, W, Tp, Q=Q)          # (cached: lowers only when this (Bi, Q) / bucket is new)
        elif get_rank() == 0 and (self.module._eval_key(*geo[:4]) if (not self.module.training and hasattr(self.module, "_eval_key"))
                                  else tuple(geo) + (self.module.training,)) not in self.module._plans:
            self.module._plan_for(*geo[:4])
        payload = [dict(ops._TUNE_CACHE) if get_rank() == 0 else None]
        dist.broadcast_object_list(payload, src=0, group=self.group)
        if get_rank() != 0:
            ops._TUNE_CACHE.update(payload[0])

    def forward(self, inp):
        if hasattr(self.module, "_refuse_sync_shared"):
            self.module._refuse_sync_shared(inp)       # (raises before any collective of this forward)
        if self.world > 1:
            self._sync_tuning(inp)
        if self.active and self.broadcast_buffers and self.module.training:
            self._sync_buffers()
        return self.module(inp)

    def eval_precision(self, dtype: str = "fp32"):
        """ZSGNet.eval_precision of the wrapped network ("fp32" | "bf16" | "bf16_act"): eval plans are per rank, nothing is communicated"""
        self.module.eval_precision(dtype)
        return self

    def eval_tta(self, mode: str = "none"):
        """ZSGNet.eval_tta of the wrapped network ("none" | "flip"): eval plans are per rank, nothing is communicated"""
        self.module.eval_tta(mode)
        return self

    def eval_scales(self, scales=()):
        """ZSGNet.eval_scales of the wrapped network (extra eval passes at other resolutions): eval plans are per rank, nothing is communicated"""
        self.module.eval_scales(scales)
        return self

    def wgrad_precision(self, dtype: str = "fp32"):
        """ZSGNet.wgrad_precision of the wrapped network ("fp32" | "bf16"): the gradients stay fp32, so buckets and collectives are unchanged"""
        self.module.wgrad_precision(dtype)
        return self

    def train_precision(self, dtype: str = "fp32"):
        """ZSGNet.train_precision of the wrapped network ("fp32" | "bf16_head"): activations and gradients stay fp32 in memory, so buckets
        and collectives are unchanged"""
        self.module.train_precision(dtype)
        return self

    def encoder_precision(self, dtype: str = "fp32"):
        """ZSGNet.encoder_precision of the wrapped network ("fp32" | "bf16_fwd"): activations and gradients stay fp32 in memory, so buckets
        and collectives are unchanged (a synchronized BatchNorm reads the bf16 launch's partial rows as it reads the fp32 launch's)"""
        self.module.encoder_precision(dtype)
        return self

    def encoder_backward_precision(self, dtype: str = "fp32"):
        """ZSGNet.encoder_backward_precision of the wrapped network ("fp32" | "bf16"): activations and gradients stay fp32 in memory, so
        buckets and collectives are unchanged (a synchronized BatchNorm reads the bf16 data gradient's partial rows as it reads the fp32
        launch's)"""
        self.module.encoder_backward_precision(dtype)
        return self

    def close(self):
        """Releases the native communicator (its RCCL communicator, stream and events); the wrapper is unusable afterwards."""
        if self.comm is not None:
            self.comm.close()
            self.comm = None
            self.active = False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def make_reducer(self, spans) -> BucketReducer:
        return BucketReducer(self.module.store.grad, plan_buckets(spans, self.bucket_elems, self.tail_elems), self.group, self.comm)


def convert_sync_batchnorm(module, process_group=None, force: bool = False):
    """torch.nn.SyncBatchNorm.convert_sync_batchnorm for ZSGNet (whose BatchNorm layers torch's converter does not find): the train-mode
    BatchNorm layers of `module` — a ZSGNet or its DistributedDataParallel wrapper — normalise with the statistics of the union of the
    batches of `process_group`'s ranks (ZSGNet.sync_batchnorm).  A collective call: every rank of the default group makes it with the
    same process_group (per-node subgroups are not supported), and it creates the BatchNorm collectives' own group.  force=True syncs in a 1-rank group too (tests, measurements).  Returns `module`."""
    net = module.module if isinstance(module, DistributedDataParallel) else module
    net.sync_batchnorm(process_group=process_group, enable=True, force=force)
    return module


def reduce_dict(input_dict, average=False, all_ranks: bool = True):
    """utils.py:62-91: stack the scalar values and reduce them (C4).  The reference reduces to rank 0 only
    (dist.reduce(dst=0)) and then lets EVERY rank step ReduceLROnPlateau / gate checkpoints on its own buffer, so the
    learning rates of the replicas can drift apart; here every rank receives the global sums (all_reduce) unless
    all_ranks=False asks for the reference's rank-0-only behaviour."""
    world = get_world_size()
    if world < 2:
        return input_dict
    with torch.no_grad():
        names = sorted(input_dict.keys())
        values = torch.stack([input_dict[k].detach().float().reshape(()) for k in names], dim=0)
        if all_ranks:
            dist.all_reduce(values, op=dist.ReduceOp.SUM)
        else:
            dist.reduce(values, dst=0)
        if average and (all_ranks or dist.get_rank() == 0):
            values /= world
        return {k: v for k, v in zip(names, values)}
