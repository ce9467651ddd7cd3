"""Developer tool (CPU): what enc_dtype = "bf16_fwd" should cost in accuracy, from the oracle alone.  The set-up of
tests/test_gpu_net_enc_bf16.py (ResNet-18, 128 px, B = 2, seeded weights, one forward + loss + backward) is run twice in the oracle
(torch-CPU autograd), once as it is and once with every encoder convolution behind the stem computing its FORWARD value from operands
rounded to bf16 (round-to-nearest-even) while its backward stays the unrounded convolution's (a straight-through value:
y = conv(x, w) + (conv(bf16 x, bf16 w) - conv(x, w)).detach() — the plan's backward reads the fp32 activations and weights).  Printed: the
metrics of the test's rounded part.  usage: python tools/enc_bf16_emul.py [--dtype float64|float32] [--arch resnet18]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import zsg_oracle as O  # noqa: E402


class _RoundedF:
    """oracle.F with conv2d rounding its operands in the forward (the stem, C = 3, apart)"""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, k):
        return getattr(self._real, k)

    def conv2d(self, x, w, *a, **k):
        y = self._real.conv2d(x, w, *a, **k)
        if w.shape[1] == 3:
            return y
        with torch.no_grad():
            yb = self._real.conv2d(x.to(torch.bfloat16).to(x.dtype), w.to(torch.bfloat16).to(w.dtype), *a, **k)
        return y + (yb - y).detach()


def run(arch, dtype, rounded):
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in O.seeded_state_dict(arch, 1).items()}
    params = [k for k, v in sd.items() if v.is_floating_point() and "running_" not in k]
    for k in params:
        sd[k] = sd[k].clone().requires_grad_(True)
    bt = O.synthetic_batch(2, 128, 128, seed=3)
    g = torch.Generator().manual_seed(0)
    h0, c0 = torch.randn(2, 2, 128, generator=g).to(dtype), torch.randn(2, 2, 128, generator=g).to(dtype)
    bt = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in bt.items()}
    real_enc, real_F = O.encoder_forward, O.F

    def enc(*a, **k):
        O.F = _RoundedF(real_F)
        try:
            return real_enc(*a, **k)
        finally:
            O.F = real_F
    if rounded:
        O.encoder_forward = enc
    try:
        out = O.zsgnet_forward(sd, bt, h0, c0, arch=arch, training=True)
    finally:
        O.encoder_forward = real_enc
    r, s = O.default_ratios_scales()
    anc = torch.from_numpy(O.create_anchors([tuple(x) for x in out["feat_sizes"].tolist()], r, s).astype(np.float32))
    ls = O.torch_loss(out, bt["annot"].float(), anc)
    ls["loss"].backward()
    flat = torch.cat([sd[k].grad.reshape(-1).double() for k in params])
    return out["bbx_out"].detach().double(), out["att_out"].detach().double(), float(ls["loss"].detach()), flat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="float64", choices=("float64", "float32"))
    ap.add_argument("--arch", default="resnet18")
    a = ap.parse_args()
    dtype = getattr(torch, a.dtype)
    b0, a0, l0, g0 = run(a.arch, dtype, False)
    b1, a1, l1, g1 = run(a.arch, dtype, True)
    box = float((b1 - b0).abs().max() / b0.abs().max())
    att = float((a1 - a0).abs().max() / a0.abs().max())
    l2 = float((g1 - g0).norm() / g0.norm())
    cos = float((g1 * g0).sum() / (g1.norm() * g0.norm()))
    print(f"enc_bf16 emulation ({a.arch}, {a.dtype}): box {box:.3e} att {att:.3e} loss {abs(l1 - l0) / abs(l0):.3e} ({l0:.6f} -> {l1:.6f}) "
          f"flat l2 {l2:.3e} 1-cos {1 - cos:.3e}")


if __name__ == "__main__":
    main()
