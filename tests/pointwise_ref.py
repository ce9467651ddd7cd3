"""Plain numpy / torch-CPU definitions of the element-wise kernels (csrc/misc.hip) and of the BatchNorm finalize (csrc/bn.hip) that
tests/test_gpu_pointwise_edges.py and tests/test_gpu_bn_finalize.py compare against.  Nothing here imports the product.

torch CPU is the definition wherever torch has the operation (F.max_pool2d and its autograd, F.interpolate(size=), x / x.norm() and its
autograd, .float().div_(255)); the pure index shuffles (interleave, pad_rows, nchw_to_nhwc4) and the sums (batch_sum, colsum, the
BatchNorm finalize) are written out, sums in fp64.  Activations are NHWC, as the kernels take them; tests/test_cpu_pointwise_ref.py checks
the hand-written parts against torch on small inputs."""
import numpy as np
import torch
import torch.nn.functional as F


def nchw(x_nhwc):
    return x_nhwc.permute(0, 3, 1, 2).contiguous()


def nhwc(x_nchw):
    return x_nchw.permute(0, 2, 3, 1).contiguous()


# ---- max pool ----------------------------------------------------------------------------------------------------------------------
def maxpool(x_nhwc, k, s, p, ceil=False, dout_nhwc=None):
    """F.max_pool2d on an NHWC tensor -> (out NHWC, tap codes NHWC uint8, dx NHWC or None).  The tap code of a window is r * k + q of
    torch's arg-max element (r, q: row / column of the element inside the window, padding included), the encoding zsg_maxpool_fwd
    writes; dx is torch's autograd gradient for dout."""
    xr = nchw(x_nhwc).requires_grad_(dout_nhwc is not None)
    y, flat = F.max_pool2d(xr, k, s, p, ceil_mode=ceil, return_indices=True)
    W = x_nhwc.shape[2]
    Ho, Wo = y.shape[2:]
    ih, iw = flat // W, flat % W
    r = ih - (torch.arange(Ho).view(1, 1, Ho, 1) * s - p)
    q = iw - (torch.arange(Wo).view(1, 1, 1, Wo) * s - p)
    assert int(r.min()) >= 0 and int(r.max()) < k and int(q.min()) >= 0 and int(q.max()) < k
    codes = nhwc((r * k + q).to(torch.uint8))
    dx = None
    if dout_nhwc is not None:
        y.backward(nchw(dout_nhwc))
        dx = nhwc(xr.grad)
    return nhwc(y.detach()), codes, dx


def maxpool_bwd_ordered(dout_nhwc, codes_nhwc, H, W, k, s, p):
    """fp32 max-pool gradient with the additions of one input pixel made in the order maxpool_bwd_kernel states: window rows ho
    descending, then window columns wo descending.  (A window sends each (b, c) to ONE pixel, so adding window after window in that
    order gives every pixel its contributions in exactly that order.)"""
    g = dout_nhwc.numpy().astype(np.float32)
    codes = codes_nhwc.numpy().astype(np.int64)
    B, Ho, Wo, C = g.shape
    dx = np.zeros((B, H, W, C), np.float32)
    bb, cc = np.meshgrid(np.arange(B), np.arange(C), indexing="ij")
    for ho in range(Ho - 1, -1, -1):
        for wo in range(Wo - 1, -1, -1):
            code = codes[:, ho, wo, :]
            hi, wi = ho * s - p + code // k, wo * s - p + code % k
            ok = (hi >= 0) & (hi < H) & (wi >= 0) & (wi < W)
            dx[bb[ok], hi[ok], wi[ok], cc[ok]] += g[:, ho, wo, :][ok]
    return torch.from_numpy(dx)


def maxpool_rule(x_nhwc, k, s, p, Ho, Wo):
    """The forward's selection rule written out (loops; small inputs only): taps in row-major order, out-of-bounds taps skipped, the
    index starts at the first in-bounds tap, a tap takes over when it is greater than the running maximum or is NaN.
    -> (out, codes) as maxpool()."""
    x = x_nhwc.numpy()
    B, H, W, C = x.shape
    out = np.full((B, Ho, Wo, C), -np.inf, np.float32)
    codes = np.zeros((B, Ho, Wo, C), np.uint8)
    for b in range(B):
        for ho in range(Ho):
            for wo in range(Wo):
                for c in range(C):
                    best, bi, seen = -np.inf, 0, False
                    for r in range(k):
                        hi = ho * s - p + r
                        if hi < 0 or hi >= H:
                            continue
                        for q in range(k):
                            wi = wo * s - p + q
                            if wi < 0 or wi >= W:
                                continue
                            v = x[b, hi, wi, c]
                            if not seen:
                                seen, bi = True, r * k + q
                            if v > best or v != v:
                                best, bi = v, r * k + q
                    out[b, ho, wo, c], codes[b, ho, wo, c] = best, bi
    return torch.from_numpy(out), torch.from_numpy(codes)


# ---- nearest upsample + add -----------------------------------------------------------------------------------------------------------
def nearest_src_f32(n_src, n_dst):
    """source index of every destination index 0 .. n_dst - 1 by the kernels' fp32 rule min(int(floorf(f32(dst) * (f32(n_src) / f32(n_dst)))),
    n_src - 1), every operation rounded to fp32"""
    scale = np.float32(n_src) / np.float32(n_dst)
    src = np.floor(np.arange(n_dst, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(src, n_src - 1)


def nearest_src_torch(n_src, n_dst):
    """the same map read off F.interpolate(size=) ('nearest')"""
    return F.interpolate(torch.arange(n_src, dtype=torch.float32).view(1, 1, n_src, 1), size=(n_dst, 1)).view(-1).long().numpy()


def upsample_scan_range(ys, n_src, n_dst):
    """the candidate destination range upsample_add_bwd_kernel scans for source index ys: floorf(ys / sh) - 1 .. ceilf((ys + 1) / sh) + 1
    in fp32, clamped to the image"""
    sh = np.float32(n_src) / np.float32(n_dst)
    lo = max(0, int(np.floor(np.float32(ys) / sh)) - 1)
    hi = min(n_dst - 1, int(np.ceil(np.float32(ys + 1) / sh)) + 1)
    return lo, hi


def upsample_add(a_nhwc, p_nhwc, dout_nhwc=None):
    """a + F.interpolate(p, size=a's) -> (out NHWC, d(p) NHWC or None)"""
    pr = nchw(p_nhwc).requires_grad_(dout_nhwc is not None)
    out = nchw(a_nhwc) + F.interpolate(pr, size=tuple(a_nhwc.shape[1:3]))
    dp = None
    if dout_nhwc is not None:
        out.backward(nchw(dout_nhwc))
        dp = nhwc(pr.grad)
    return nhwc(out.detach()), dp


# ---- channel L2 norm ------------------------------------------------------------------------------------------------------------------
def l2norm(x, dout=None):
    """x / x.norm(dim=1, keepdim=True) on [rows, C] -> (out, norm [rows], dx or None); a zero row is NaN throughout, as torch has it"""
    xr = x.clone().requires_grad_(dout is not None)
    nrm = xr.norm(dim=1, keepdim=True)
    y = xr / nrm
    dx = None
    if dout is not None:
        y.backward(dout)
        dx = xr.grad
    return y.detach(), nrm.detach().view(-1), dx


# ---- index shuffles ---------------------------------------------------------------------------------------------------------------------
def interleave_to_strided(compact, strided, rows, groups, k, gs, off):
    """direction 0 of zsg_interleave: strided[r][a][off + e] = compact[r][a][e]; every other element of `strided` is kept"""
    out = strided.clone().view(rows, groups, gs)
    out[:, :, off:off + k] = compact.view(rows, groups, k)
    return out.view(-1)


def interleave_to_compact(strided, rows, groups, k, gs, off):
    """direction 1: compact[r][a][e] = strided[r][a][off + e]"""
    return strided.view(rows, groups, gs)[:, :, off:off + k].contiguous().view(-1)


def pad_rows(src, rows, C, src_ld, dst_ld):
    """dst[r][0:dst_ld] = [src[r][0:C] | +0]"""
    out = torch.zeros(rows, dst_ld, dtype=src.dtype)
    out[:, :C] = src.view(rows, src_ld)[:, :C]
    return out


def nchw_to_nhwc4(img):
    """[B, C <= 4, H, W] -> [B, H, W, 4], the missing channels +0"""
    B, C, H, W = img.shape
    out = torch.zeros(B, H, W, 4, dtype=img.dtype)
    out[..., :C] = img.permute(0, 2, 3, 1)
    return out


def u8hwc_to_nhwc4(img_u8):
    """[pixels, 3] uint8 -> [pixels, 4] float: .float().div_(255), fourth channel +0"""
    out = torch.zeros(img_u8.shape[0], 4)
    out[:, :3] = img_u8.float().div_(255)
    return out


# ---- sums (fp64) ------------------------------------------------------------------------------------------------------------------------
def batch_sum(x, B, stride):
    """out[i] = sum_b x[b * stride + i], fp64"""
    return x.view(-1)[:B * stride].view(B, stride).double().sum(0)


def colsum(x_flat, groups, gstride, rows, ld, c0, C):
    """out[g][c] = sum_r x[g * gstride + r * ld + c0 + c], fp64 -> [groups, C]"""
    out = torch.empty(groups, C, dtype=torch.float64)
    for g in range(groups):
        blk = x_flat[g * gstride:g * gstride + rows * ld].view(rows, ld)
        out[g] = blk[:, c0:c0 + C].double().sum(0)
    return out


# ---- BatchNorm finalize (fp64) ------------------------------------------------------------------------------------------------------------
def bn_partial_sums(partials):
    """[chunks][2][C] fp32 partial rows -> (sum e, sum e^2) per channel in fp64"""
    p = partials.double()
    return p[:, 0].sum(0), p[:, 1].sum(0)


def bn_finalize(se, sse, n, eps, running_mean=None, running_var=None, momentum=0.1):
    """Training-mode BatchNorm statistics from fp64 channel sums:
    mean = f32(se / n); var = max(sse / n - m * m, 0) (biased); invstd = f32(1 / sqrt(var + f64(f32(eps))));
    running statistics by torch's rule, new = (1 - momentum) * old + momentum * stat with the UNBIASED variance var * n / (n - 1)
    (in fp64 from the fp32 inputs: the caller allows for the kernel's fp32 roundings).
    -> dict(mean f32, invstd f32, invstd64, var, running_mean f64, running_var f64, rm_terms, rv_terms); *_terms are the two
    products of each running update, for the caller's rounding bound."""
    se, sse = se.double(), sse.double()
    n = float(n)
    m = se / n
    var = (sse / n - m * m).clamp_min(0)
    eps64 = float(np.float32(eps))
    inv64 = 1.0 / torch.sqrt(var + eps64)
    res = {"mean": m.float(), "invstd": inv64.float(), "invstd64": inv64, "var": var}
    mom = float(np.float32(momentum))
    keep = float(np.float32(1) - np.float32(momentum))
    if running_mean is not None:
        a, b = keep * running_mean.double(), mom * m.float().double()
        res["running_mean"], res["rm_terms"] = a + b, (a, b)
    if running_var is not None:
        unb = (var * n / (n - 1) if n > 1 else var).float().double()
        a, b = keep * running_var.double(), mom * unb
        res["running_var"], res["rv_terms"] = a + b, (a, b)
    return res


def conditioning_data(ratio_cycle=(0.0, 8.0, 64.0), rows=4096, C=64, seed=11):
    """fp32 [rows, C] data whose channel c has std 1 and mean ratio_cycle[c % 3]; -> (x, ratio per channel, fp64 invstd of that data)"""
    g = torch.Generator().manual_seed(seed)
    ratio = torch.tensor([ratio_cycle[c % len(ratio_cycle)] for c in range(C)])
    x = (torch.randn(rows, C, generator=g) + ratio).float()
    xd = x.double()
    var = (xd * xd).mean(0) - xd.mean(0) ** 2
    return x, ratio, 1.0 / torch.sqrt(var + float(np.float32(1e-5)))


def ulp_distance(a, b):
    """distance in units of the last place between two fp32 tensors of equal sign (finite, non-zero)"""
    ia = a.contiguous().view(torch.int32).long()
    ib = b.contiguous().view(torch.int32).long()
    return (ia - ib).abs()
