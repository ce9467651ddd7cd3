"""Oracle fixture for frozen (eval-mode) BatchNorm at the configs[1] shape (ResNet-50 + FPN, 300x300, B = 16): the oracle's side of
tests/test_gpu_frozen_bn.py::test_configs1_all_frozen_vs_oracle_fixture, made on the host (~1-2 min) so that the GPU suite only reads it.

    python tests/golden/make_frozen_bn_fixture.py      # writes tests/golden/o3_r50_300_b16_frozen_bn.npz

Weights: O.seeded_state_dict("resnet50", SEED).  Running statistics: the batch statistics (mean, unbiased variance) of every
BatchNorm input in a train-mode forward of ANOTHER synthetic batch (with the seeded 0 / 1 statistics a frozen trunk would not
normalise).  Then every BatchNorm layer is frozen — F.batch_norm(training=False) inside a training forward, gamma / beta trainable —
and the fp32 CPU oracle and its fp64 twin run forward + backward on the test batch.  Stored, as tests/golden/make_oracle_fixtures.py
does for o2: the running statistics, the fp64 outputs on every 53rd anchor, the CPU-fp32 forward distance from fp64, the losses, and per
parameter the fp64 gradient norm, the CPU-fp32 distance from it and sampled entries (<= 128, fixed stride) of both gradients.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import zsg_oracle as O  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
NS = 128          # sampled gradient entries per parameter (the fixture stays well under 1 MiB)
SEED, STATS_SEED, BATCH_SEED, HC_SEED = 7, 33, 21, 4
B, HW, ARCH = 16, 300, "resnet50"


def sample_idx(n: int) -> np.ndarray:
    return np.arange(0, n, max(1, n // NS))[:NS]


def hc(seed, B):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, B, 128, generator=g), torch.randn(2, B, 128, generator=g)


class Frozen(O.BNState):
    """every BatchNorm layer in eval mode inside the training forward"""

    def __call__(self, x, name):
        sd = self.sd
        return F.batch_norm(x, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"], sd[name + ".bias"], False, 0.1, 1e-5)


def batch_statistics(sd):
    rec = {}

    class Rec(O.BNState):
        def __call__(self, x, name):
            rec[name] = (x.mean((0, 2, 3)).detach().float(), x.var((0, 2, 3)).detach().float())
            return super().__call__(x, name)
    bt = O.synthetic_batch(B, HW, HW, seed=STATS_SEED)
    h0, c0 = hc(HC_SEED + 1, B)
    keep, O.BNState = O.BNState, Rec
    try:
        with torch.no_grad():
            O.zsgnet_forward({k: v.clone() for k, v in sd.items()}, bt, h0, c0, arch=ARCH)
    finally:
        O.BNState = keep
    return rec


def main():
    sd = O.seeded_state_dict(ARCH, SEED)
    stats = batch_statistics(sd)
    names_bn = list(stats)
    for n in names_bn:
        sd[n + ".running_mean"], sd[n + ".running_var"] = stats[n][0].clone(), stats[n][1].clone()
    rm = np.concatenate([stats[n][0].numpy() for n in names_bn])
    rv = np.concatenate([stats[n][1].numpy() for n in names_bn])
    bt = O.synthetic_batch(B, HW, HW, seed=BATCH_SEED)
    h0, c0 = hc(HC_SEED, B)
    for k, v in sd.items():
        if v.is_floating_point() and "running" not in k:
            v.requires_grad_()
    r, s = O.default_ratios_scales()
    keep, O.BNState = O.BNState, Frozen
    try:
        ref = O.zsgnet_forward(sd, bt, h0, c0, arch=ARCH)
        anc = torch.from_numpy(O.create_anchors([tuple(x) for x in ref["feat_sizes"].tolist()], r, s).astype(np.float32))
        l32 = O.torch_loss(ref, bt["annot"], anc)
        l32["loss"].backward()
        print(f"fp32 oracle: loss {float(l32['loss'].detach()):.6f}", flush=True)
        sd64 = {k: (v.detach().double().requires_grad_(v.requires_grad) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
        ref64 = O.zsgnet_forward(sd64, {k: v.double() for k, v in bt.items()}, h0.double(), c0.double(), arch=ARCH, rank=O.sort_rank(bt["qlens"]))
        l64 = O.torch_loss(ref64, bt["annot"], anc)
        l64["loss"].backward()
        print(f"fp64 oracle: loss {float(l64['loss'].detach()):.9f}", flush=True)
    finally:
        O.BNState = keep
    o64 = torch.cat([ref64["bbx_out"], ref64["att_out"]], 2).detach()
    o32 = torch.cat([ref["bbx_out"], ref["att_out"]], 2).detach()
    arrs = dict(seed=np.array([SEED]), stats_seed=np.array([STATS_SEED]), batch_seed=np.array([BATCH_SEED]), hc_seed=np.array([HC_SEED]),
                bn_names=np.array(names_bn), running_mean=rm, running_var=rv, out64_s=o64[:, ::53].numpy(), out_stride=np.array([53]),
                fwd_err_cpu=np.array([float((o32.double() - o64).abs().max())]), loss32=np.array([float(l32["loss"].detach())]),
                loss64=np.array([float(l64["loss"].detach())]))
    names, n64, e32, g64s, g32s = [], [], [], [], []
    for n, v in sd64.items():
        if not (v.is_floating_point() and v.grad is not None):
            continue
        g64_, g32_ = v.grad.reshape(-1), sd[n].grad.reshape(-1).double()
        idx = sample_idx(g64_.numel())
        names.append(n)
        n64.append(float(g64_.norm()))
        e32.append(float((g32_ - g64_).norm()))
        a, b = np.zeros(NS), np.zeros(NS)
        a[:len(idx)] = g64_.numpy()[idx]
        b[:len(idx)] = g32_.numpy()[idx]
        g64s.append(a)
        g32s.append(b)
    arrs.update(names=np.array(names), norm64=np.array(n64), err32=np.array(e32), g64_s=np.stack(g64s), g32_s=np.stack(g32s).astype(np.float32))
    path = os.path.join(OUT, "o3_r50_300_b16_frozen_bn.npz")
    np.savez_compressed(path, **arrs)
    print(f"o3_r50_300_b16_frozen_bn.npz  {os.path.getsize(path) / 1024:.1f} KB, {len(names)} parameters", flush=True)


if __name__ == "__main__":
    torch.manual_seed(0)
    main()
