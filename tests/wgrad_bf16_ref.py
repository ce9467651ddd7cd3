"""Host reference of the convolution weight gradient (tests/test_gpu_wgrad_bf16.py, tests/test_cpu_wgrad_bf16.py): the GEMM of
csrc/wgrad_bf16.hip written tap by tap in the operands' own dtype (int64: exact; float64: the reference of the rounded operands)."""
import torch


def conv_out(n, k, s, p, d):
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


def wgrad_ref(src, dy, k, s, p, d):
    """src [B, H, W, C], dy [B, Ho, Wo, N] of one dtype (int64 or float64) -> dw [N, k, k, C]:
    dw[n, ty, tx, c] = sum_{b, y, x} dy[b, y, x, n] * src[b, y*s + ty*d - p, x*s + tx*d - p, c]   (zero outside the image)"""
    B, H, W, Cc = src.shape
    _, Ho, Wo, N = dy.shape
    assert Ho == conv_out(H, k, s, p, d) and Wo == conv_out(W, k, s, p, d)
    pad = torch.zeros(B, H + 2 * p, W + 2 * p, Cc, dtype=src.dtype)
    pad[:, p:p + H, p:p + W] = src
    dw = torch.zeros(dy.shape[-1], k, k, Cc, dtype=src.dtype)
    g = dy.reshape(-1, N).t().contiguous()
    for ty in range(k):
        for tx in range(k):
            win = pad[:, ty * d: ty * d + (Ho - 1) * s + 1: s, tx * d: tx * d + (Wo - 1) * s + 1: s]
            dw[:, ty, tx] = torch.matmul(g, win.reshape(-1, Cc))
    return dw


def wgrad_ref_levels(srcs, dys, k, s, p, d):
    """the pyramid levels of a shared convolution are segments of one launch: their gradients add"""
    out = None
    for x, g in zip(srcs, dys):
        r = wgrad_ref(x, g, k, s, p, d)
        out = r if out is None else out + r
    return out


def bf16_round(x):
    """fp32 -> bf16 -> fp64, round-to-nearest-even: the rule of Tensor.to(torch.bfloat16) the kernel's operand loader follows"""
    return x.to(torch.bfloat16).double()
