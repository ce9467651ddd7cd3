"""Developer tool (CPU): what enc_bwd_dtype = "bf16" should cost in accuracy, from the oracle alone.  The set-up of
tests/test_gpu_net_enc_bwd_bf16.py (ResNet-18, 128 px, B = 2, seeded weights, one forward + loss + backward) is run twice in the oracle
(torch-CPU autograd), once as it is and once with every encoder convolution behind the stem computing its DATA gradient from operands
rounded to bf16 (round-to-nearest-even: dy and the filter, as zsg_conv_igemm_bf16_m / _bnb round them) while its forward value and its
weight gradient stay the unrounded convolution's.  Printed: the flat-gradient metrics of the test's rounded part; emulate() returns them
(the test multiplies them by its margin).  usage: python tools/enc_bwd_bf16_emul.py [--dtype float64|float32] [--arch resnet18]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import zsg_oracle as O  # noqa: E402


class _ConvRoundedDgrad(torch.autograd.Function):
    """y = conv2d(x, w) (no bias, no groups); dx from bf16(dy) and bf16(w), dw from the unrounded operands"""

    @staticmethod
    def forward(ctx, x, w, stride, padding, dilation):
        ctx.save_for_backward(x, w)
        ctx.geo = (stride, padding, dilation)
        return torch.nn.functional.conv2d(x, w, None, stride, padding, dilation)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        stride, padding, dilation = ctx.geo
        rb = lambda t: t.to(torch.bfloat16).to(t.dtype)
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = torch.nn.grad.conv2d_input(x.shape, rb(w), rb(gy), stride, padding, dilation)
        if ctx.needs_input_grad[1]:
            gw = torch.nn.grad.conv2d_weight(x, w.shape, gy, stride, padding, dilation)
        return gx, gw, None, None, None


class _RoundedF:
    """oracle.F with conv2d rounding the operands of its data gradient (the stem, C = 3, apart)"""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, k):
        return getattr(self._real, k)

    def conv2d(self, x, w, bias=None, stride=1, padding=0, dilation=1, groups=1):
        if w.shape[1] == 3 or bias is not None or groups != 1:
            return self._real.conv2d(x, w, bias, stride, padding, dilation, groups)
        return _ConvRoundedDgrad.apply(x, w, stride, padding, dilation)


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
    return float(ls["loss"].detach()), flat


def emulate(arch="resnet18", dtype=torch.float64):
    """(relative L2, 1 - cosine) of the flat gradient with rounded encoder data gradients against the unrounded run; the loss is the same"""
    l0, g0 = run(arch, dtype, False)
    l1, g1 = run(arch, dtype, True)
    assert l0 == l1, "the forward is untouched"
    l2 = float((g1 - g0).norm() / g0.norm())
    cos = float((g1 * g0).sum() / (g1.norm() * g0.norm()))
    return l2, 1.0 - cos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="float64", choices=("float64", "float32"))
    ap.add_argument("--arch", default="resnet18")
    a = ap.parse_args()
    l2, omc = emulate(a.arch, getattr(torch, a.dtype))
    print(f"enc_bwd_bf16 emulation ({a.arch}, {a.dtype}): flat l2 {l2:.3e} 1-cos {omc:.3e}")


if __name__ == "__main__":
    main()
