// loss.hip — anchor matching + focal / smooth-L1 loss (forward AND backward in one call) and the evaluator.
// Index contract: IoU is evaluated with the reference's exact fp32 operation order (no FMA contraction, IEEE divide),
// arg-max ties go to the lowest anchor index, so match indices / positive masks are bit-exact against the oracle.
// Reductions: per-thread fp32 -> wavefront shuffle -> LDS across waves, accumulated in fp64.
#include "common.h"
#pragma clang fp contract(off)

#define LS_THREADS 512

__device__ __forceinline__ float iou_exact(const f32x4 b, const f32x4 a) {   // b = first argument ("anchors" of IoU_values)
    const float tly = fmaxf(b[0], a[0]), tlx = fmaxf(b[1], a[1]);
    const float bry = fminf(b[2], a[2]), brx = fminf(b[3], a[3]);
    const float sy = fmaxf(bry - tly, 0.f), sx = fmaxf(brx - tlx, 0.f);
    const float inter = sy * sx;
    const float barea = (b[2] - b[0]) * (b[3] - b[1]);
    const float aarea = (a[2] - a[0]) * (a[3] - a[1]);
    const float uni = (barea + aarea) - inter;
    return inter / (uni + 1e-8f);
}

__device__ __forceinline__ float focal_pow(float x, float gamma) {   // torch.pow(x, 2) is x*x exactly (loss.py:117)
    return gamma == 2.f ? x * x : (gamma == 1.f ? x : powf(x, gamma));
}

struct ArgMax {
    float v;
    int i;
};
__device__ __forceinline__ ArgMax argmax_merge(ArgMax x, ArgMax y) {   // larger value, then lower index; NaN never wins
    const bool take = (y.v > x.v) || (y.v == x.v && y.i < x.i);
    return take ? y : x;
}
__device__ ArgMax block_argmax(ArgMax m, ArgMax* sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ArgMax y;
        y.v = __shfl_xor(m.v, o, 64);
        y.i = __shfl_xor(m.i, o, 64);
        m = argmax_merge(m, y);
    }
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[wave] = m;
    __syncthreads();
    ArgMax r = sm[0];
    for (int w = 1; w < nw; ++w) r = argmax_merge(r, sm[w]);
    __syncthreads();
    return r;
}
__device__ double block_sum_d(double v, double* sm) {
    v = wave_sum_d(v);
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[wave] = v;
    __syncthreads();
    double r = 0;
    for (int w = 0; w < nw; ++w) r += sm[w];
    __syncthreads();
    return r;
}

// smooth-L1 (beta = 1) of (reg - target(anchor, box)); returns the 4-sum and the four derivatives.
__device__ __forceinline__ float box_terms(const float* __restrict__ o5, const f32x4 an, const f32x4 bx, float d[4]) {
    const float acy = (an[0] + an[2]) / 2.f, acx = (an[1] + an[3]) / 2.f;
    const float ah = an[2] - an[0], aw = an[3] - an[1];
    const float bcy = (bx[0] + bx[2]) / 2.f, bcx = (bx[1] + bx[3]) / 2.f;
    const float bh = bx[2] - bx[0], bw = bx[3] - bx[1];
    const float dh = ah + 1e-8f, dw = aw + 1e-8f;
    float gt[4];
    gt[0] = (bcy - acy) / dh;
    gt[1] = (bcx - acx) / dw;
    gt[2] = logf(bh / dh);
    gt[3] = logf(bw / dw);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float df = o5[k] - gt[k];
        const float ad = fabsf(df);
        s += ad < 1.f ? 0.5f * df * df : ad - 0.5f;
        d[k] = ad < 1.f ? df : (df > 0.f ? 1.f : (df < 0.f ? -1.f : df));
    }
    return s;
}

struct LossWs {          // per-sample records in the workspace (doubles first for alignment)
    double box_sum, cls_sum, row_max, row_lse;
    int best, npos, pad0, pad1;
};

// pass 1: one block per sample — arg-max IoU, positive count, loss sums.
__global__ __launch_bounds__(LS_THREADS) void loss_stats_kernel(const float* __restrict__ out5, const float* __restrict__ annot,
                                                                const float* __restrict__ anchors, int A, float alpha, float gamma,
                                                                float thr, int flags, LossWs* __restrict__ ws) {
    __shared__ ArgMax sm_a[LS_THREADS / 64];
    __shared__ double sm_d[LS_THREADS / 64];
    const int b = blockIdx.x;
    const bool use_focal = flags & 1, use_multi = flags & 2, use_softmax = flags & 4;
    const f32x4 bx = *(const f32x4*)(annot + 4 * b);
    const float* o = out5 + (size_t)b * A * 5;

    ArgMax m = {-INFINITY, 0x7fffffff};
    for (int a = threadIdx.x; a < A; a += LS_THREADS) {
        const float v = iou_exact(bx, *(const f32x4*)(anchors + 4 * a));
        if (v > m.v) { m.v = v; m.i = a; }
    }
    m = block_argmax(m, sm_a);
    const int best = m.i == 0x7fffffff ? 0 : m.i;     // all-NaN row: torch returns the first NaN's index; degenerate

    double row_max = 0, row_lse = 0;
    if (use_softmax) {
        float mx = -INFINITY;
        for (int a = threadIdx.x; a < A; a += LS_THREADS) mx = fmaxf(mx, o[a * 5 + 4]);
        ArgMax t = {mx, 0};
        t = block_argmax(t, sm_a);
        double se = 0;
        for (int a = threadIdx.x; a < A; a += LS_THREADS) se += exp((double)o[a * 5 + 4] - (double)t.v);
        se = block_sum_d(se, sm_d);
        row_max = t.v;
        row_lse = (double)t.v + log(se);
    }

    double box = 0, cls = 0;
    int cnt = 0;
    for (int a = threadIdx.x; a < A; a += LS_THREADS) {
        const f32x4 an = *(const f32x4*)(anchors + 4 * a);
        const float v = iou_exact(bx, an);
        const bool pos = (use_multi && v > thr) || a == best;
        const float t = pos ? 1.f : 0.f;
        cnt += pos;
        float d[4];
        const float s = box_terms(o + a * 5, an, bx, d);
        box += (double)(s * t);                         // multiply (not select): inf * 0 = NaN, as the reference
        const float x = o[a * 5 + 4];
        if (!use_softmax) {
            const float bce = fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
            float w = 1.f;
            if (use_focal) {
                const float p = 1.0f / (1.0f + expf(-x));
                w = focal_pow(t * (1.f - p) + (1.f - t) * p, gamma) * ((1.f - t) * alpha + t * (1.f - alpha));
            }
            cls += (double)(w * bce);
        }
    }
    box = block_sum_d(box, sm_d);
    cls = block_sum_d(cls, sm_d);
    const int npos = (int)(block_sum_d((double)cnt, sm_d) + 0.5);
    if (threadIdx.x == 0) {
        if (use_softmax) cls = row_lse - (double)o[best * 5 + 4];
        LossWs r;
        r.box_sum = box; r.cls_sum = cls; r.row_max = row_max; r.row_lse = row_lse; r.best = best; r.npos = npos; r.pad0 = r.pad1 = 0;
        ws[b] = r;
    }
}

// Chunked pass 1 (sigmoid / focal classification, the default): the anchors of a sample are cut into LS_CHUNKS ranges so that
// B x LS_CHUNKS blocks work instead of B (16 blocks on 256 CUs took 62 us of the step's critical path):
//   1a  arg-max IoU of every range;  1b  every block merges the sample's range maxima (lowest index wins ties, as before),
//   then sums its own range.  The per-range records are merged in range order (fixed order: deterministic) by pass 2.
#define LS_CHUNKS 32
struct LossPart {
    double box_sum, cls_sum;
    int npos, pad;
};
__global__ __launch_bounds__(256) void loss_argmax_kernel(const float* __restrict__ annot, const float* __restrict__ anchors, int A,
                                                          ArgMax* __restrict__ amax) {
    __shared__ ArgMax sm_a[4];
    const int b = blockIdx.y, per = (A + LS_CHUNKS - 1) / LS_CHUNKS;
    const int a0 = blockIdx.x * per, a1 = min(A, a0 + per);
    const f32x4 bx = *(const f32x4*)(annot + 4 * b);
    ArgMax m = {-INFINITY, 0x7fffffff};
    for (int a = a0 + threadIdx.x; a < a1; a += 256) {
        const float v = iou_exact(bx, *(const f32x4*)(anchors + 4 * a));
        if (v > m.v) { m.v = v; m.i = a; }
    }
    m = block_argmax(m, sm_a);
    if (threadIdx.x == 0) amax[b * LS_CHUNKS + blockIdx.x] = m;
}
__global__ __launch_bounds__(256) void loss_part_kernel(const float* __restrict__ out5, const float* __restrict__ annot,
                                                        const float* __restrict__ anchors, int A, float alpha, float gamma, float thr,
                                                        int flags, const ArgMax* __restrict__ amax, LossPart* __restrict__ parts) {
    __shared__ double sm_d[4];
    const bool use_focal = flags & 1, use_multi = flags & 2;
    const int b = blockIdx.y, per = (A + LS_CHUNKS - 1) / LS_CHUNKS;
    const int a0 = blockIdx.x * per, a1 = min(A, a0 + per);
    const f32x4 bx = *(const f32x4*)(annot + 4 * b);
    const float* o = out5 + (size_t)b * A * 5;
    ArgMax m = amax[b * LS_CHUNKS];
    for (int c = 1; c < LS_CHUNKS; ++c) m = argmax_merge(m, amax[b * LS_CHUNKS + c]);
    const int best = m.i == 0x7fffffff ? 0 : m.i;
    double box = 0, cls = 0;
    int cnt = 0;
    for (int a = a0 + threadIdx.x; a < a1; a += 256) {
        const f32x4 an = *(const f32x4*)(anchors + 4 * a);
        const float v = iou_exact(bx, an);
        const bool pos = (use_multi && v > thr) || a == best;
        const float t = pos ? 1.f : 0.f;
        cnt += pos;
        float d[4];
        const float s = box_terms(o + a * 5, an, bx, d);
        box += (double)(s * t);                         // multiply (not select): inf * 0 = NaN, as the reference
        const float x = o[a * 5 + 4];
        const float bce = fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
        float w = 1.f;
        if (use_focal) {
            const float p = 1.0f / (1.0f + expf(-x));
            w = focal_pow(t * (1.f - p) + (1.f - t) * p, gamma) * ((1.f - t) * alpha + t * (1.f - alpha));
        }
        cls += (double)(w * bce);
    }
    box = block_sum_d(box, sm_d);
    cls = block_sum_d(cls, sm_d);
    const int npos = (int)(block_sum_d((double)cnt, sm_d) + 0.5);
    if (threadIdx.x == 0) {
        LossPart r;
        r.box_sum = box; r.cls_sum = cls; r.npos = npos; r.pad = best;       // (pad carries the sample's arg-max for pass 2)
        parts[b * LS_CHUNKS + blockIdx.x] = r;
    }
}

// pass 2: totals (every block recomputes them from the B records), loss scalars, gradients.
#define LS_MAX_B 512
__global__ __launch_bounds__(256) void loss_grad_kernel(const float* __restrict__ out5, const float* __restrict__ annot,
                                                        const float* __restrict__ anchors, int B, int A, float alpha, float gamma,
                                                        float lamb, float thr, int flags, float grad_scale,
                                                        const LossWs* __restrict__ ws_in, const LossPart* __restrict__ parts,
                                                        float* __restrict__ losses,
                                                        float* __restrict__ grad5, int* __restrict__ match_idx, int* __restrict__ npos_out) {
    const bool use_focal = flags & 1, use_multi = flags & 2, use_softmax = flags & 4;
    const int b = blockIdx.y;
    __shared__ LossWs ws[LS_MAX_B];
    for (int k = threadIdx.x; k < B; k += blockDim.x) {
        LossWs r;
        if (parts) {                                     // merge the sample's range records in range order
            r.box_sum = r.cls_sum = r.row_max = r.row_lse = 0;
            r.npos = 0;
            for (int c = 0; c < LS_CHUNKS; ++c) {
                const LossPart q = parts[k * LS_CHUNKS + c];
                r.box_sum += q.box_sum;
                r.cls_sum += q.cls_sum;
                r.npos += q.npos;
            }
            r.best = parts[k * LS_CHUNKS].pad;
            r.pad0 = r.pad1 = 0;
        } else {
            r = ws_in[k];
        }
        ws[k] = r;
    }
    __syncthreads();
    double box = 0, cls = 0;
    long long npos_all = 0;
    for (int k = 0; k < B; ++k) {
        box += ws[k].box_sum / (double)ws[k].npos;
        cls += ws[k].cls_sum;
        npos_all += ws[k].npos;
    }
    box /= (double)B;
    cls /= (double)npos_all;
    const bool bad = (box != box) || (cls != cls);       // loss.py:128-133: constants, no gradient reaches the network
    if (blockIdx.x == 0 && b == 0 && threadIdx.x == 0) {
        const double bl = bad ? 0.01 : box, cl = bad ? 1.0 : cls;
        losses[0] = (float)(lamb * bl + cl);
        losses[1] = (float)cl;
        losses[2] = (float)bl;
    }
    const LossWs me = ws[b];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        match_idx[b] = me.best;
        if (npos_out) npos_out[b] = me.npos;
    }
    if (!grad5) return;
    const f32x4 bx = *(const f32x4*)(annot + 4 * b);
    const float* o = out5 + (size_t)b * A * 5;
    float* g = grad5 + (size_t)b * A * 5;
    const float kbox = bad ? 0.f : grad_scale * lamb / ((float)B * (float)me.npos);
    const float kcls = bad ? 0.f : grad_scale / (float)npos_all;
    for (int a = blockIdx.x * blockDim.x + threadIdx.x; a < A; a += gridDim.x * blockDim.x) {
        const f32x4 an = *(const f32x4*)(anchors + 4 * a);
        const float v = iou_exact(bx, an);
        const bool pos = (use_multi && v > thr) || a == me.best;
        const float t = pos ? 1.f : 0.f;
        float d[4];
        box_terms(o + a * 5, an, bx, d);
#pragma unroll
        for (int k = 0; k < 4; ++k) g[a * 5 + k] = pos ? kbox * d[k] : 0.f;
        const float x = o[a * 5 + 4];
        float ga;
        if (use_softmax) {
            ga = (float)exp((double)x - me.row_lse) - (a == me.best ? 1.f : 0.f);
        } else {
            const float p = 1.0f / (1.0f + expf(-x));
            float w = 1.f;
            if (use_focal) w = focal_pow(t * (1.f - p) + (1.f - t) * p, gamma) * ((1.f - t) * alpha + t * (1.f - alpha));
            ga = w * (p - t);
        }
        g[a * 5 + 4] = kcls * ga;
    }
}

struct LossWsIou {       // LossWs + the sample's box-IoU loss sum (zsg_loss_fwd_bwd_iou); the same 48 bytes
    double box_sum, cls_sum, iou_sum, row_max, row_lse;
    int best, npos;
};
struct LossPartIou {     // LossPart + the range's box-IoU loss sum
    double box_sum, cls_sum, iou_sum;
    int npos, best;
};

struct LossWsQ {         // LossWsIou with the sum of the positives' quality targets in the place of row_max (which pass 2 never reads)
    double box_sum, cls_sum, iou_sum, q_sum, row_lse;
    int best, npos;
};
struct LossPartQ {       // LossPartIou + the range's sum of quality targets: the largest range record
    double box_sum, cls_sum, iou_sum, q_sum;
    int npos, best;
};

extern "C" size_t zsg_loss_workspace_bytes(int32_t B, int32_t A) {   // covers the three entry points (the records of the quality one are the largest)
    (void)A;
    static_assert(sizeof(LossWsIou) == sizeof(LossWs) && sizeof(LossWsQ) == sizeof(LossWs), "workspace records");
    static_assert(sizeof(LossPartQ) >= sizeof(LossPartIou) && sizeof(LossPartIou) >= sizeof(LossPart), "workspace records");
    return (size_t)B * (sizeof(LossWsQ) + LS_CHUNKS * (sizeof(ArgMax) + sizeof(LossPartQ)));
}

extern "C" int zsg_loss_fwd_bwd(const float* out5, const float* annot, const float* anchors, int32_t B, int32_t A, float alpha, float gamma,
                                float lamb_reg, float match_thr, int32_t flags, float grad_scale, float* losses, float* grad5,
                                int32_t* match_idx, int32_t* npos, void* ws, size_t ws_bytes, void* stream) {
    ZSG_REQUIRE(out5 && annot && anchors && losses && match_idx && ws && B > 0 && A > 0, "loss_fwd_bwd: bad argument");
    ZSG_REQUIRE(!((flags & 4) && (flags & 2)), "loss_fwd_bwd: use_softmax requires use_multi == False (loss.py:107)");
    if (ws_bytes < zsg_loss_workspace_bytes(B, A)) ZSG_FAIL(-2, "loss_fwd_bwd: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("loss_fwd_bwd", st, 0, (double)B * A * 5 * 4 * 3);
    ZSG_REQUIRE(B <= LS_MAX_B, "loss_fwd_bwd: B=%d exceeds %d", B, LS_MAX_B);
    LossWs* rec = (LossWs*)ws;
    LossPart* parts = (LossPart*)(rec + B);
    ArgMax* amax = (ArgMax*)(parts + (size_t)B * LS_CHUNKS);
    const bool chunked = !(flags & 4) && A >= 4 * LS_CHUNKS;      // softmax needs row-wide max / sum passes: one block per sample
    if (chunked) {
        ZSG_LAUNCH(loss_argmax_kernel, dim3(LS_CHUNKS, B), dim3(256), 0, st, annot, anchors, A, amax);
        ZSG_LAUNCH(loss_part_kernel, dim3(LS_CHUNKS, B), dim3(256), 0, st, out5, annot, anchors, A, alpha, gamma, match_thr, flags,
                           (const ArgMax*)amax, parts);
    } else {
        ZSG_LAUNCH(loss_stats_kernel, dim3(B), dim3(LS_THREADS), 0, st, out5, annot, anchors, A, alpha, gamma, match_thr, flags, rec);
    }
    const int chunks = min(32, cdiv(A, 256));
    ZSG_LAUNCH(loss_grad_kernel, dim3(chunks, B), dim3(256), 0, st, out5, annot, anchors, B, A, alpha, gamma, lamb_reg, match_thr,
                       flags, grad_scale, (const LossWs*)rec, chunked ? (const LossPart*)parts : (const LossPart*)nullptr, losses, grad5,
                       match_idx, npos);
    ZSG_CHECK_LAUNCH("loss_fwd_bwd");
    return 0;
}

// ---- box IoU loss: a GIoU / DIoU term next to the smooth-L1 term (zsg_loss_fwd_bwd_iou) ----------------------------------
// The kernels below are loss_stats_kernel / loss_part_kernel / loss_grad_kernel with that term added inside their anchor loops (the
// same launches, loss_argmax_kernel is shared); the kernels above are what ZSGLoss runs when the term is off, and are not touched.
// For a positive anchor: p = the decoded box (decode_box's expressions), g = the annotation,
//   inter = max(min(p.y2, g.y2) - max(p.y1, g.y1), 0) * (same in x),  union = area(p) + area(g) - inter,  iou = inter / (union + eps),
//   ey, ex = the sides of the smallest box enclosing both,
//   giou:  L = 1 - iou + (ey ex - union) / (ey ex + eps)          diou:  L = 1 - iou + |centre(p) - centre(g)|^2 / (ey^2 + ex^2 + eps)
// iou_loss_terms returns L and dL / d(r0..r3): the derivative with respect to (y1, x1, y2, x2) written out by hand, then through the
// decode (d/dr0 = ah (dy1 + dy2), d/dr2 = h / 2 (dy2 - dy1), likewise in x).  At an exact tie of a min / max the zero side is taken.
// It is evaluated in fp64 from the fp32 inputs: the derivative of inter / union is a difference of near-equal products, and only the
// few positive anchors of a sample come here, so the extra cost does not show.  Negative anchors never enter the sum (a select, not
// the multiply of the smooth-L1 term): a NaN in a negative anchor's regression output reaches box_ls only.
#define IOU_EPS 1e-7
__device__ __forceinline__ double iou_loss_terms(const float* __restrict__ o5, const f32x4 an, const f32x4 bx, int kind, double d[4]) {
    const double acy = ((double)an[0] + (double)an[2]) / 2., acx = ((double)an[1] + (double)an[3]) / 2.;
    const double ah = (double)an[2] - (double)an[0], aw = (double)an[3] - (double)an[1];
    const double cy = ah * (double)o5[0] + acy, cx = aw * (double)o5[1] + acx;
    const double h = exp((double)o5[2]) * ah, w = exp((double)o5[3]) * aw;
    const double y1 = cy - h / 2., x1 = cx - w / 2., y2 = cy + h / 2., x2 = cx + w / 2.;
    const double g0 = bx[0], g1 = bx[1], g2 = bx[2], g3 = bx[3];
    const double ry = fmin(y2, g2) - fmax(y1, g0), rx = fmin(x2, g3) - fmax(x1, g1);
    const double iy = fmax(ry, 0.), ix = fmax(rx, 0.);
    const double inter = iy * ix;
    const double ph = y2 - y1, pw = x2 - x1;
    const double uni = ph * pw + (g2 - g0) * (g3 - g1) - inter;
    const double ue = uni + IOU_EPS;
    const double iou = inter / ue;
    const double ey = fmax(y2, g2) - fmin(y1, g0), ex = fmax(x2, g3) - fmin(x1, g1);
    // per coordinate k of (y1, x1, y2, x2): d inter, d area(p), d ey, d ex
    const double di[4] = {(ry > 0. && y1 > g0) ? -ix : 0., (rx > 0. && x1 > g1) ? -iy : 0.,
                          (ry > 0. && y2 < g2) ? ix : 0., (rx > 0. && x2 < g3) ? iy : 0.};
    const double da[4] = {-pw, -ph, pw, ph};
    const double dey[4] = {y1 < g0 ? -1. : 0., 0., y2 > g2 ? 1. : 0., 0.};
    const double dex[4] = {0., x1 < g1 ? -1. : 0., 0., x2 > g3 ? 1. : 0.};
    double L, dp[4];
    if (kind == 1) {
        const double C = ey * ex, ce = C + IOU_EPS;
        L = 1. - iou + (C - uni) / ce;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double dU = da[k] - di[k], dC = dey[k] * ex + dex[k] * ey;
            dp[k] = ((dC - dU) * ce - (C - uni) * dC) / (ce * ce) - (di[k] * ue - inter * dU) / (ue * ue);
        }
    } else {
        const double qy = (y1 + y2) / 2. - (g0 + g2) / 2., qx = (x1 + x2) / 2. - (g1 + g3) / 2.;
        const double rho2 = qy * qy + qx * qx, D = ey * ey + ex * ex + IOU_EPS;
        L = 1. - iou + rho2 / D;
        const double dq[4] = {qy, qx, qy, qx};                      // d rho2: 2 q * (1 / 2)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double dU = da[k] - di[k], dD = 2. * (ey * dey[k] + ex * dex[k]);
            dp[k] = (dq[k] * D - rho2 * dD) / (D * D) - (di[k] * ue - inter * dU) / (ue * ue);
        }
    }
    d[0] = ah * (dp[0] + dp[2]);
    d[1] = aw * (dp[1] + dp[3]);
    d[2] = (h / 2.) * (dp[2] - dp[0]);
    d[3] = (w / 2.) * (dp[3] - dp[1]);
    return L;
}

// pass 1, one block per sample (loss_stats_kernel + the IoU sum)
__global__ __launch_bounds__(LS_THREADS) void loss_stats_iou_kernel(const float* __restrict__ out5, const float* __restrict__ annot,
                                                                    const float* __restrict__ anchors, int A, float alpha, float gamma,
                                                                    float thr, int flags, int iou_kind, LossWsIou* __restrict__ ws) {
    __shared__ ArgMax sm_a[LS_THREADS / 64];
    __shared__ double sm_d[LS_THREADS / 64];
    const int b = blockIdx.x;
    const bool use_focal = flags & 1, use_multi = flags & 2, use_softmax = flags & 4;
    const f32x4 bx = *(const f32x4*)(annot + 4 * b);
    const float* o = out5 + (size_t)b * A * 5;

    ArgMax m = {-INFINITY, 0x7fffffff};
    for (int a = threadIdx.x; a < A; a += LS_THREADS) {
        const float v = iou_exact(bx, *(const f32x4*)(anchors + 4 * a));
        if (v > m.v) { m.v = v; m.i = a; }
    }
    m = block_argmax(m, sm_a);
    const int best = m.i == 0x7fffffff ? 0 : m.i;

    double row_max = 0, row_lse = 0;
    if (use_softmax) {
        float mx = -INFINITY;
        for (int a = threadIdx.x; a < A; a += LS_THREADS) mx = fmaxf(mx, o[a * 5 + 4]);
        ArgMax t = {mx, 0};
        t = block_argmax(t, sm_a);
        double se = 0;
        for (int a = threadIdx.x; a < A; a += LS_THREADS) se += exp((double)o[a * 5 + 4] - (double)t.v);
        se = block_sum_d(se, sm_d);
        row_max = t.v;
        row_lse = (double)t.v + log(se);
    }

    double box = 0, cls = 0, iou = 0;
    int cnt = 0;
    for (int a = threadIdx.x; a < A; a += LS_THREADS) {
        const f32x4 an = *(const f32x4*)(anchors + 4 * a);
        const float v = iou_exact(bx, an);
        const bool pos = (use_multi && v > thr) || a == best;
        const float t = pos ? 1.f : 0.f;
        cnt += pos;
        float d[4];
        const float s = box_terms(o + a * 5, an, bx, d);
        box += (double)(s * t);
        if (pos) {
            double di[4];
            iou += iou_loss_terms(o + a * 5, an, bx, iou_kind, di);
        }
        const float x = o[a * 5 + 4];
        if (!use_softmax) {
            const float bce = fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
            float w = 1.f;
            if (use_focal) {
                const float p = 1.0f / (1.0f + expf(-x));
                w = focal_pow(t * (1.f - p) + (1.f - t) * p, gamma) * ((1.f - t) * alpha + t * (1.f - alpha));
            }
            cls += (double)(w * bce);
        }
    }
    box = block_sum_d(box, sm_d);
    cls = block_sum_d(cls, sm_d);
    iou = block_sum_d(iou, sm_d);
    const int npos = (int)(block_sum_d((double)cnt, sm_d) + 0.5);
    if (threadIdx.x == 0) {
        if (use_softmax) cls = row_lse - (double)o[best * 5 + 4];
        LossWsIou r;
        r.box_sum = box; r.cls_sum = cls; r.iou_sum = iou; r.row_max = row_max; r.row_lse = row_lse; r.best = best; r.npos = npos;
        ws[b] = r;
    }
}

// chunked pass 1b (loss_part_kernel + the IoU sum); pass 1a is loss_argmax_kernel itself
__global__ __launch_bounds__(256) void loss_part_iou_kernel(const float* __restrict__ out5, const float* __restrict__ annot,
                                                            const float* __restrict__ anchors, int A, float alpha, float gamma, float thr,
                                                            int flags, int iou_kind, const ArgMax* __restrict__ amax,
                                                            LossPartIou* __restrict__ parts) {
    __shared__ double sm_d[4];
    const bool use_focal = flags & 1, use_multi = flags & 2;
    const int b = blockIdx.y, per = (A + LS_CHUNKS - 1) / LS_CHUNKS;
    const int a0 = blockIdx.x * per, a1 = min(A, a0 + per);
    const f32x4 bx = *(const f32x4*)(annot + 4 * b);
    const float* o = out5 + (size_t)b * A * 5;
    ArgMax m = amax[b * LS_CHUNKS];
    for (int c = 1; c < LS_CHUNKS; ++c) m = argmax_merge(m, amax[b * LS_CHUNKS + c]);
    const int best = m.i == 0x7fffffff ? 0 : m.i;
    double box = 0, cls = 0, iou = 0;
    int cnt = 0;
    for (int a = a0 + threadIdx.x; a < a1; a += 256) {
        const f32x4 an = *(const f32x4*)(anchors + 4 * a);
        const float v = iou_exact(bx, an);
        const bool pos = (use_multi && v > thr) || a == best;
        const float t = pos ? 1.f : 0.f;
        cnt += pos;
        float d[4];
        const float s = box_terms(o + a * 5, an, bx, d);
        box += (double)(s * t);
        if (pos) {
            double di[4];
            iou += iou_loss_terms(o + a * 5, an, bx, iou_kind, di);
        }
        const float x = o[a * 5 + 4];
        const float bce = fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
        float w = 1.f;
        if (use_focal) {
            const float p = 1.0f / (1.0f + expf(-x));
            w = focal_pow(t * (1.f - p) + (1.f - t) * p, gamma) * ((1.f - t) * alpha + t * (1.f - alpha));
        }
        cls += (double)(w * bce);
    }
    box = block_sum_d(box, sm_d);
    cls = block_sum_d(cls, sm_d);
    iou = block_sum_d(iou, sm_d);
    const int npos = (int)(block_sum_d((double)cnt, sm_d) + 0.5);
    if (threadIdx.x == 0) {
        LossPartIou r;
        r.box_sum = box; r.cls_sum = cls; r.iou_sum = iou; r.npos = npos; r.best = best;
        parts[b * LS_CHUNKS + blockIdx.x] = r;
    }
}

// pass 2 (loss_grad_kernel + the IoU term): losses[4] = (loss, cls_ls, box_ls, iou_ls); a NaN in any of the three parts gives the
// constants, iou_ls = 0 and an exactly zero gradient (also at the anchor that holds the NaN).
__global__ __launch_bounds__(256) void loss_grad_iou_kernel(const float* __restrict__ out5, const float* __restrict__ annot,
                                                            const float* __restrict__ anchors, int B, int A, float alpha, float gamma,
                                                            float lamb, float thr, int flags, float grad_scale, int iou_kind, float lamb_iou,
                                                            const LossWsIou* __restrict__ ws_in, const LossPartIou* __restrict__ parts,
                                                            float* __restrict__ losses, float* __restrict__ grad5,
                                                            int* __restrict__ match_idx, int* __restrict__ npos_out) {
    const bool use_focal = flags & 1, use_multi = flags & 2, use_softmax = flags & 4;
    const int b = blockIdx.y;
    __shared__ LossWsIou ws[LS_MAX_B];
    for (int k = threadIdx.x; k < B; k += blockDim.x) {
        LossWsIou r;
        if (parts) {                                     // merge the sample's range records in range order
            r.box_sum = r.cls_sum = r.iou_sum = r.row_max = r.row_lse = 0;
            r.npos = 0;
            for (int c = 0; c < LS_CHUNKS; ++c) {
                const LossPartIou q = parts[k * LS_CHUNKS + c];
                r.box_sum += q.box_sum;
                r.cls_sum += q.cls_sum;
                r.iou_sum += q.iou_sum;
                r.npos += q.npos;
            }
            r.best = parts[k * LS_CHUNKS].best;
        } else {
            r = ws_in[k];
        }
        ws[k] = r;
    }
    __syncthreads();
    double box = 0, cls = 0, iou = 0;
    long long npos_all = 0;
    for (int k = 0; k < B; ++k) {
        box += ws[k].box_sum / (double)ws[k].npos;
        iou += ws[k].iou_sum / (double)ws[k].npos;
        cls += ws[k].cls_sum;
        npos_all += ws[k].npos;
    }
    box /= (double)B;
    iou /= (double)B;
    cls /= (double)npos_all;
    const bool bad = (box != box) || (cls != cls) || (iou != iou);
    if (blockIdx.x == 0 && b == 0 && threadIdx.x == 0) {
        const double bl = bad ? 0.01 : box, cl = bad ? 1.0 : cls, il = bad ? 0.0 : iou;
        losses[0] = (float)(lamb * bl + lamb_iou * il + cl);
        losses[1] = (float)cl;
        losses[2] = (float)bl;
        losses[3] = (float)il;
    }
    const LossWsIou me = ws[b];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        match_idx[b] = me.best;
        if (npos_out) npos_out[b] = me.npos;
    }
    if (!grad5) return;
    const f32x4 bx = *(const f32x4*)(annot + 4 * b);
    const float* o = out5 + (size_t)b * A * 5;
    float* g = grad5 + (size_t)b * A * 5;
    const float kbox = bad ? 0.f : grad_scale * lamb / ((float)B * (float)me.npos);
    const float kiou = bad ? 0.f : grad_scale * lamb_iou / ((float)B * (float)me.npos);
    const float kcls = bad ? 0.f : grad_scale / (float)npos_all;
    for (int a = blockIdx.x * blockDim.x + threadIdx.x; a < A; a += gridDim.x * blockDim.x) {
        const f32x4 an = *(const f32x4*)(anchors + 4 * a);
        const float v = iou_exact(bx, an);
        const bool pos = (use_multi && v > thr) || a == me.best;
        const float t = pos ? 1.f : 0.f;
        float d[4];
        box_terms(o + a * 5, an, bx, d);
        if (pos && !bad) {                               // (bad: zeros, not 0 * NaN — the NaN may sit in this very anchor)
            double di[4];
            iou_loss_terms(o + a * 5, an, bx, iou_kind, di);
#pragma unroll
            for (int k = 0; k < 4; ++k) g[a * 5 + k] = kbox * d[k] + kiou * (float)di[k];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) g[a * 5 + k] = 0.f;
        }
        const float x = o[a * 5 + 4];
        float ga;
        if (use_softmax) {
            ga = (float)exp((double)x - me.row_lse) - (a == me.best ? 1.f : 0.f);
        } else {
            const float p = 1.0f / (1.0f + expf(-x));
            float w = 1.f;
            if (use_focal) w = focal_pow(t * (1.f - p) + (1.f - t) * p, gamma) * ((1.f - t) * alpha + t * (1.f - alpha));
            ga = w * (p - t);
        }
        g[a * 5 + 4] = bad ? 0.f : kcls * ga;
    }
}

extern "C" int zsg_loss_fwd_bwd_iou(const float* out5, const float* annot, const float* anchors, int32_t B, int32_t A, float alpha,
                                    float gamma, float lamb_reg, float match_thr, int32_t flags, float grad_scale, int32_t iou_kind,
                                    float lamb_iou, float* losses, float* grad5, int32_t* match_idx, int32_t* npos, void* ws,
                                    size_t ws_bytes, void* stream) {
    ZSG_REQUIRE(out5 && annot && anchors && losses && match_idx && ws && B > 0 && A > 0, "loss_fwd_bwd_iou: bad argument");
    ZSG_REQUIRE(!((flags & 4) && (flags & 2)), "loss_fwd_bwd_iou: use_softmax requires use_multi == False (loss.py:107)");
    ZSG_REQUIRE(iou_kind == 1 || iou_kind == 2, "loss_fwd_bwd_iou: iou_kind=%d is neither 1 (giou) nor 2 (diou)", iou_kind);
    ZSG_REQUIRE(lamb_iou >= 0.f, "loss_fwd_bwd_iou: lamb_iou must not be negative");
    if (ws_bytes < zsg_loss_workspace_bytes(B, A)) ZSG_FAIL(-2, "loss_fwd_bwd_iou: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("loss_fwd_bwd_iou", st, 0, (double)B * A * 5 * 4 * 3);
    ZSG_REQUIRE(B <= LS_MAX_B, "loss_fwd_bwd_iou: B=%d exceeds %d", B, LS_MAX_B);
    LossWsIou* rec = (LossWsIou*)ws;
    LossPartIou* parts = (LossPartIou*)(rec + B);
    ArgMax* amax = (ArgMax*)(parts + (size_t)B * LS_CHUNKS);
    const bool chunked = !(flags & 4) && A >= 4 * LS_CHUNKS;      // as zsg_loss_fwd_bwd
    if (chunked) {
        ZSG_LAUNCH(loss_argmax_kernel, dim3(LS_CHUNKS, B), dim3(256), 0, st, annot, anchors, A, amax);
        ZSG_LAUNCH(loss_part_iou_kernel, dim3(LS_CHUNKS, B), dim3(256), 0, st, out5, annot, anchors, A, alpha, gamma, match_thr, flags,
                           iou_kind, (const ArgMax*)amax, parts);
    } else {
        ZSG_LAUNCH(loss_stats_iou_kernel, dim3(B), dim3(LS_THREADS), 0, st, out5, annot, anchors, A, alpha, gamma, match_thr, flags,
                           iou_kind, rec);
    }
    const int chunks = min(32, cdiv(A, 256));
    ZSG_LAUNCH(loss_grad_iou_kernel, dim3(chunks, B), dim3(256), 0, st, out5, annot, anchors, B, A, alpha, gamma, lamb_reg, match_thr,
                       flags, grad_scale, iou_kind, lamb_iou, (const LossWsIou*)rec,
                       chunked ? (const LossPartIou*)parts : (const LossPartIou*)nullptr, losses, grad5, match_idx, npos);
    ZSG_CHECK_LAUNCH("loss_fwd_bwd_iou");
    return 0;
}

// ---- IoU-aware classification targets: Quality Focal / Varifocal loss (zsg_loss_fwd_bwd_q) ----------------------------------
// The three kernels below are the IoU-loss kernels above with the classification term exchanged (the same launches, loss_argmax_kernel
// is shared); the kernels above are what the two older entry points run and are not touched.  With x the att logit, s = sigmoid(x),
// m the positives mask and q = m ? iou(decoded box, annotation) : 0 (the iou of iou_loss_terms, the same fp64 expressions in the same
// order: bit-equal to it), a constant for the derivative, BCE(x, q) = max(x, 0) - x q + log1p(exp(-|x|)):
//   cls_kind 1 (qfl):  l = |q - s|^gamma BCE(x, q)                                      every anchor
//   cls_kind 2 (vfl):  l = q BCE(x, q)  (positives),   alpha s^gamma BCE(x, 0)  (negatives)
// and dl/dx is the true derivative, through the modulating factor (d BCE / dx = s - q, ds/dx = s (1 - s)):
//   d/dx |q - s|^gamma BCE = sign(s - q) |s - q|^(gamma - 1) (gamma s (1 - s) BCE + (s - q)^2)
// Both summands inside the bracket are >= 0: nothing cancels except in s - q itself, where the derivative is small; fp32 as the
// focal term.  cls_kind 0 is the focal / plain / softmax term of the kernels above, expression for expression; iou_kind 0 leaves
// the IoU loss out (iou_ls = 0).  q is evaluated for every positive in all cases: its per-sample mean is losses[4] (pos_iou).
__device__ __forceinline__ double decoded_iou(const float* __restrict__ o5, const f32x4 an, const f32x4 bx) {
    const double acy = ((double)an[0] + (double)an[2]) / 2., acx = ((double)an[1] + (double)an[3]) / 2.;
    const double ah = (double)an[2] - (double)an[0], aw = (double)an[3] - (double)an[1];
    const double cy = ah * (double)o5[0] + acy, cx = aw * (double)o5[1] + acx;
    const double h = exp((double)o5[2]) * ah, w = exp((double)o5[3]) * aw;
    const double y1 = cy - h / 2., x1 = cx - w / 2., y2 = cy + h / 2., x2 = cx + w / 2.;
    const double g0 = bx[0], g1 = bx[1], g2 = bx[2], g3 = bx[3];
    const double ry = fmin(y2, g2) - fmax(y1, g0), rx = fmin(x2, g3) - fmax(x1, g1);
    const double iy = fmax(ry, 0.), ix = fmax(rx, 0.);
    const double inter = iy * ix;
    const double ph = y2 - y1, pw = x2 - x1;
    const double uni = ph * pw + (g2 - g0) * (g3 - g1) - inter;
    return inter / (uni + IOU_EPS);
}

// the fp32 score of an att logit: what the quality term trains towards q, and what zsg_match_tal ranks by
__device__ __forceinline__ float att_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// l and dl/dx of one anchor for cls_kind 1 / 2 (q = 0 at a negative anchor)
__device__ __forceinline__ float quality_terms(float x, float q, bool pos, int cls_kind, float alpha, float gamma, float* dx) {
    const float p = att_sigmoid(x);
    const float bce = fmaxf(x, 0.f) - x * q + log1pf(expf(-fabsf(x)));
    if (cls_kind == 2 && pos) {
        *dx = q * (p - q);
        return q * bce;
    }
    const float d = p - q, ad = fabsf(d);
    const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    const float w = cls_kind == 2 ? alpha : 1.f;
    *dx = w * sg * focal_pow(ad, gamma - 1.f) * (gamma * p * (1.f - p) * bce + d * d);
    return w * focal_pow(ad, gamma) * bce;
}

struct QSums {
    double box, cls, iou, q;
    int cnt;
};
// one anchor of pass 1: the loop body of loss_stats_iou_kernel / loss_part_iou_kernel with q and the exchanged classification term.
// MASK = false: the reference's fixed rule for the positives, the expression of the kernels above.  MASK = true (zsg_loss_fwd_bwd_m): pm,
// the sample's row of a positives mask made beforehand (zsg_match_atss), decides; use_multi and thr are not consulted.
template <bool MASK>
__device__ __forceinline__ void q_pass1_anchor(QSums& s, const float* __restrict__ o, const float* __restrict__ anchors, const f32x4 bx,
                                               int a, int best, float alpha, float gamma, float thr, int flags, int iou_kind, int cls_kind,
                                               const uint8_t* __restrict__ pm) {
    const bool use_focal = flags & 1, use_multi = flags & 2, use_softmax = flags & 4;
    const f32x4 an = *(const f32x4*)(anchors + 4 * a);
    const float v = iou_exact(bx, an);                   // (unused with a mask)
    const bool pos = MASK ? (pm[a] != 0 || a == best) : ((use_multi && v > thr) || a == best);
    const float t = pos ? 1.f : 0.f;
    s.cnt += pos;
    float d[4];
    const float sl1 = box_terms(o + a * 5, an, bx, d);
    s.box += (double)(sl1 * t);
    float q = 0.f;
    if (pos) {
        double di[4];
        if (iou_kind) s.iou += iou_loss_terms(o + a * 5, an, bx, iou_kind, di);
        const double qd = decoded_iou(o + a * 5, an, bx);
        s.q += qd;
        q = (float)qd;
    }
    const float x = o[a * 5 + 4];
    if (cls_kind) {
        float dx;
        s.cls += (double)quality_terms(x, q, pos, cls_kind, alpha, gamma, &dx);
    } else if (!use_softmax) {
        const float bce = fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
        float w = 1.f;
        if (use_focal) {
            const float p = 1.0f / (1.0f + expf(-x));
            w = focal_pow(t * (1.f - p) + (1.f - t) * p, gamma) * ((1.f - t) * alpha + t * (1.f - alpha));
        }
        s.cls += (double)(w * bce);
    }
}

// pass 1, one block per sample (loss_stats_iou_kernel + q).  The three kernels end in a parameter pack that is either empty
// (zsg_loss_fwd_bwd_q: the kernel's arguments and its code are what they were without the pack) or one const uint8_t* pos_mask [B][A]
// (zsg_loss_fwd_bwd_m).
__device__ __forceinline__ const uint8_t* mask_arg() { return nullptr; }
__device__ __forceinline__ const uint8_t* mask_arg(const uint8_t* p) { return p; }
template <typename... M>
__global__ __launch_bounds__(LS_THREADS) void loss_stats_q_kernel(const float* __restrict__ out5, const float* __restrict__ annot,
                                                                  const float* __restrict__ anchors, int A, float alpha, float gamma,
                                                                  float thr, int flags, int iou_kind, int cls_kind,
                                                                  LossWsQ* __restrict__ ws, M... pos_mask) {
    constexpr bool MASK = sizeof...(M) != 0;
    __shared__ ArgMax sm_a[LS_THREADS / 64];
    __shared__ double sm_d[LS_THREADS / 64];
    const int b = blockIdx.x;
    const bool use_softmax = flags & 4;
    const f32x4 bx = *(const f32x4*)(annot + 4 * b);
    const float* o = out5 + (size_t)b * A * 5;

    ArgMax m = {-INFINITY, 0x7fffffff};
    for (int a = threadIdx.x; a < A; a += LS_THREADS) {
        const float v = iou_exact(bx, *(const f32x4*)(anchors + 4 * a));
        if (v > m.v) { m.v = v; m.i = a; }
    }
    m = block_argmax(m, sm_a);
    const int best = m.i == 0x7fffffff ? 0 : m.i;

    double row_lse = 0;
    if (use_softmax) {
        float mx = -INFINITY;
        for (int a = threadIdx.x; a < A; a += LS_THREADS) mx = fmaxf(mx, o[a * 5 + 4]);
        ArgMax t = {mx, 0};
        t = block_argmax(t, sm_a);
        double se = 0;
        for (int a = threadIdx.x; a < A; a += LS_THREADS) se += exp((double)o[a * 5 + 4] - (double)t.v);
        se = block_sum_d(se, sm_d);
        row_lse = (double)t.v + log(se);
    }

    const uint8_t* pm = MASK ? mask_arg(pos_mask...) + (size_t)b * A : nullptr;
    QSums s = {0, 0, 0, 0, 0};
    for (int a = threadIdx.x; a < A; a += LS_THREADS)
        q_pass1_anchor<MASK>(s, o, anchors, bx, a, best, alpha, gamma, thr, flags, iou_kind, cls_kind, pm);
    const double box = block_sum_d(s.box, sm_d);
    double cls = block_sum_d(s.cls, sm_d);
    const double iou = block_sum_d(s.iou, sm_d);
    const double qs = block_sum_d(s.q, sm_d);
    const int npos = (int)(block_sum_d((double)s.cnt, sm_d) + 0.5);
    if (threadIdx.x == 0) {
        if (use_softmax) cls = row_lse - (double)o[best * 5 + 4];
        LossWsQ r;
        r.box_sum = box; r.cls_sum = cls; r.iou_sum = iou; r.q_sum = qs; r.row_lse = row_lse; r.best = best; r.npos = npos;
        ws[b] = r;
    }
}

// chunked pass 1b (loss_part_iou_kernel + q); pass 1a is loss_argmax_kernel itself
template <typename... M>
__global__ __launch_bounds__(256) void loss_part_q_kernel(const float* __restrict__ out5, const float* __restrict__ annot,
                                                          const float* __restrict__ anchors, int A, float alpha, float gamma, float thr,
                                                          int flags, int iou_kind, int cls_kind, const ArgMax* __restrict__ amax,
                                                          LossPartQ* __restrict__ parts, M... pos_mask) {
    constexpr bool MASK = sizeof...(M) != 0;
    __shared__ double sm_d[4];
    const int b = blockIdx.y, per = (A + LS_CHUNKS - 1) / LS_CHUNKS;
    const int a0 = blockIdx.x * per, a1 = min(A, a0 + per);
    const f32x4 bx = *(const f32x4*)(annot + 4 * b);
    const float* o = out5 + (size_t)b * A * 5;
    ArgMax m = amax[b * LS_CHUNKS];
    for (int c = 1; c < LS_CHUNKS; ++c) m = argmax_merge(m, amax[b * LS_CHUNKS + c]);
    const int best = m.i == 0x7fffffff ? 0 : m.i;
    const uint8_t* pm = MASK ? mask_arg(pos_mask...) + (size_t)b * A : nullptr;
    QSums s = {0, 0, 0, 0, 0};
    for (int a = a0 + threadIdx.x; a < a1; a += 256)
        q_pass1_anchor<MASK>(s, o, anchors, bx, a, best, alpha, gamma, thr, flags, iou_kind, cls_kind, pm);
    const double box = block_sum_d(s.box, sm_d);
    const double cls = block_sum_d(s.cls, sm_d);
    const double iou = block_sum_d(s.iou, sm_d);
    const double qs = block_sum_d(s.q, sm_d);
    const int npos = (int)(block_sum_d((double)s.cnt, sm_d) + 0.5);
    if (threadIdx.x == 0) {
        LossPartQ r;
        r.box_sum = box; r.cls_sum = cls; r.iou_sum = iou; r.q_sum = qs; r.npos = npos; r.best = best;
        parts[b * LS_CHUNKS + blockIdx.x] = r;
    }
}

// pass 2 (loss_grad_iou_kernel + q): losses[5] = (loss, cls_ls, box_ls, iou_ls, pos_iou); a NaN in any of the three loss parts gives
// the constants, iou_ls = pos_iou = 0 and an exactly zero gradient (also at the anchor that holds the NaN).
template <typename... M>
__global__ __launch_bounds__(256) void loss_grad_q_kernel(const float* __restrict__ out5, const float* __restrict__ annot,
                                                          const float* __restrict__ anchors, int B, int A, float alpha, float gamma,
                                                          float lamb, float thr, int flags, float grad_scale, int iou_kind, float lamb_iou,
                                                          int cls_kind, const LossWsQ* __restrict__ ws_in,
                                                          const LossPartQ* __restrict__ parts, float* __restrict__ losses,
                                                          float* __restrict__ grad5, int* __restrict__ match_idx,
                                                          int* __restrict__ npos_out, M... pos_mask) {
    constexpr bool MASK = sizeof...(M) != 0;
    const bool use_focal = flags & 1, use_multi = flags & 2, use_softmax = flags & 4;
    const int b = blockIdx.y;
    __shared__ LossWsQ ws[LS_MAX_B];
    for (int k = threadIdx.x; k < B; k += blockDim.x) {
        LossWsQ r;
        if (parts) {                                     // merge the sample's range records in range order
            r.box_sum = r.cls_sum = r.iou_sum = r.q_sum = r.row_lse = 0;
            r.npos = 0;
            for (int c = 0; c < LS_CHUNKS; ++c) {
                const LossPartQ q = parts[k * LS_CHUNKS + c];
                r.box_sum += q.box_sum;
                r.cls_sum += q.cls_sum;
                r.iou_sum += q.iou_sum;
                r.q_sum += q.q_sum;
                r.npos += q.npos;
            }
            r.best = parts[k * LS_CHUNKS].best;
        } else {
            r = ws_in[k];
        }
        ws[k] = r;
    }
    __syncthreads();
    double box = 0, cls = 0, iou = 0, qm = 0;
    long long npos_all = 0;
    for (int k = 0; k < B; ++k) {
        box += ws[k].box_sum / (double)ws[k].npos;
        iou += ws[k].iou_sum / (double)ws[k].npos;
        qm += ws[k].q_sum / (double)ws[k].npos;
        cls += ws[k].cls_sum;
        npos_all += ws[k].npos;
    }
    box /= (double)B;
    iou /= (double)B;
    qm /= (double)B;
    cls /= (double)npos_all;
    const bool bad = (box != box) || (cls != cls) || (iou != iou);
    if (blockIdx.x == 0 && b == 0 && threadIdx.x == 0) {
        const double bl = bad ? 0.01 : box, cl = bad ? 1.0 : cls, il = bad ? 0.0 : iou;
        losses[0] = (float)(lamb * bl + lamb_iou * il + cl);
        losses[1] = (float)cl;
        losses[2] = (float)bl;
        losses[3] = (float)il;
        losses[4] = (float)(bad ? 0.0 : qm);
    }
    const LossWsQ me = ws[b];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        match_idx[b] = me.best;
        if (npos_out) npos_out[b] = me.npos;
    }
    if (!grad5) return;
    const f32x4 bx = *(const f32x4*)(annot + 4 * b);
    const float* o = out5 + (size_t)b * A * 5;
    float* g = grad5 + (size_t)b * A * 5;
    const float kbox = bad ? 0.f : grad_scale * lamb / ((float)B * (float)me.npos);
    const float kiou = bad ? 0.f : grad_scale * lamb_iou / ((float)B * (float)me.npos);
    const float kcls = bad ? 0.f : grad_scale / (float)npos_all;
    const uint8_t* pm = MASK ? mask_arg(pos_mask...) + (size_t)b * A : nullptr;
    for (int a = blockIdx.x * blockDim.x + threadIdx.x; a < A; a += gridDim.x * blockDim.x) {
        const f32x4 an = *(const f32x4*)(anchors + 4 * a);
        const float v = iou_exact(bx, an);               // (unused with a mask)
        const bool pos = MASK ? (pm[a] != 0 || a == me.best) : ((use_multi && v > thr) || a == me.best);
        const float t = pos ? 1.f : 0.f;
        float d[4];
        box_terms(o + a * 5, an, bx, d);
        float q = 0.f;
        if (pos && !bad) {                               // (bad: zeros, not 0 * NaN — the NaN may sit in this very anchor)
            if (iou_kind) {
                double di[4];
                iou_loss_terms(o + a * 5, an, bx, iou_kind, di);
#pragma unroll
                for (int k = 0; k < 4; ++k) g[a * 5 + k] = kbox * d[k] + kiou * (float)di[k];
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) g[a * 5 + k] = kbox * d[k];
            }
            if (cls_kind) q = (float)decoded_iou(o + a * 5, an, bx);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) g[a * 5 + k] = 0.f;
        }
        const float x = o[a * 5 + 4];
        float ga;
        if (cls_kind) {
            quality_terms(x, q, pos, cls_kind, alpha, gamma, &ga);
        } else if (use_softmax) {
            ga = (float)exp((double)x - me.row_lse) - (a == me.best ? 1.f : 0.f);
        } else {
            const float p = 1.0f / (1.0f + expf(-x));
            float w = 1.f;
            if (use_focal) w = focal_pow(t * (1.f - p) + (1.f - t) * p, gamma) * ((1.f - t) * alpha + t * (1.f - alpha));
            ga = w * (p - t);
        }
        g[a * 5 + 4] = bad ? 0.f : kcls * ga;
    }
}

// the launches of zsg_loss_fwd_bwd_q (no mask argument) and zsg_loss_fwd_bwd_m (M = const uint8_t*) after their argument checks
template <typename... M>
static void loss_q_launch(const float* out5, const float* annot, const float* anchors, int32_t B, int32_t A, float alpha, float gamma,
                          float lamb_reg, float match_thr, int32_t flags, float grad_scale, int32_t iou_kind, float lamb_iou,
                          int32_t cls_kind, float* losses, float* grad5, int32_t* match_idx, int32_t* npos, void* ws, hipStream_t st,
                          M... pos_mask) {
    LossWsQ* rec = (LossWsQ*)ws;
    LossPartQ* parts = (LossPartQ*)(rec + B);
    ArgMax* amax = (ArgMax*)(parts + (size_t)B * LS_CHUNKS);
    const bool chunked = !(flags & 4) && A >= 4 * LS_CHUNKS;      // as zsg_loss_fwd_bwd
    if (chunked) {
        ZSG_LAUNCH(loss_argmax_kernel, dim3(LS_CHUNKS, B), dim3(256), 0, st, annot, anchors, A, amax);
        ZSG_LAUNCH(loss_part_q_kernel<M...>, dim3(LS_CHUNKS, B), dim3(256), 0, st, out5, annot, anchors, A, alpha, gamma, match_thr, flags,
                           iou_kind, cls_kind, (const ArgMax*)amax, parts, pos_mask...);
    } else {
        ZSG_LAUNCH(loss_stats_q_kernel<M...>, dim3(B), dim3(LS_THREADS), 0, st, out5, annot, anchors, A, alpha, gamma, match_thr, flags,
                           iou_kind, cls_kind, rec, pos_mask...);
    }
    const int chunks = min(32, cdiv(A, 256));
    ZSG_LAUNCH(loss_grad_q_kernel<M...>, dim3(chunks, B), dim3(256), 0, st, out5, annot, anchors, B, A, alpha, gamma, lamb_reg, match_thr,
                       flags, grad_scale, iou_kind, lamb_iou, cls_kind, (const LossWsQ*)rec,
                       chunked ? (const LossPartQ*)parts : (const LossPartQ*)nullptr, losses, grad5, match_idx, npos, pos_mask...);
}

extern "C" int zsg_loss_fwd_bwd_q(const float* out5, const float* annot, const float* anchors, int32_t B, int32_t A, float alpha,
                                  float gamma, float lamb_reg, float match_thr, int32_t flags, float grad_scale, int32_t iou_kind,
                                  float lamb_iou, int32_t cls_kind, float* losses, float* grad5, int32_t* match_idx, int32_t* npos,
                                  void* ws, size_t ws_bytes, void* stream) {
    ZSG_REQUIRE(out5 && annot && anchors && losses && match_idx && ws && B > 0 && A > 0, "loss_fwd_bwd_q: bad argument");
    ZSG_REQUIRE(!((flags & 4) && (flags & 2)), "loss_fwd_bwd_q: use_softmax requires use_multi == False (loss.py:107)");
    ZSG_REQUIRE(iou_kind >= 0 && iou_kind <= 2, "loss_fwd_bwd_q: iou_kind=%d is none of 0 (none), 1 (giou), 2 (diou)", iou_kind);
    ZSG_REQUIRE(lamb_iou >= 0.f, "loss_fwd_bwd_q: lamb_iou must not be negative");
    ZSG_REQUIRE(cls_kind >= 0 && cls_kind <= 2, "loss_fwd_bwd_q: cls_kind=%d is none of 0 (none), 1 (qfl), 2 (vfl)", cls_kind);
    ZSG_REQUIRE(!cls_kind || ((flags & 1) && !(flags & 4)), "loss_fwd_bwd_q: cls_kind=%d needs use_focal and no use_softmax", cls_kind);
    ZSG_REQUIRE(!cls_kind || gamma >= 1.f, "loss_fwd_bwd_q: cls_kind=%d needs gamma >= 1 (the derivative is singular at sigmoid = q below)", cls_kind);
    if (ws_bytes < zsg_loss_workspace_bytes(B, A)) ZSG_FAIL(-2, "loss_fwd_bwd_q: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("loss_fwd_bwd_q", st, 0, (double)B * A * 5 * 4 * 3);
    ZSG_REQUIRE(B <= LS_MAX_B, "loss_fwd_bwd_q: B=%d exceeds %d", B, LS_MAX_B);
    loss_q_launch(out5, annot, anchors, B, A, alpha, gamma, lamb_reg, match_thr, flags, grad_scale, iou_kind, lamb_iou, cls_kind, losses,
                  grad5, match_idx, npos, ws, st);
    ZSG_CHECK_LAUNCH("loss_fwd_bwd_q");
    return 0;
}

// zsg_loss_fwd_bwd_q on a positives mask made beforehand (zsg_match_atss): the instantiations of its three kernels that take the mask, the same
// launches on both paths.  An anchor is positive where pos_mask[b][a] != 0 or it is the sample's arg-max IoU anchor; flags bit1
// (use_multi) and match_thr are not consulted.  The sums, the NaN rule, grad_scale, losses[5], match_idx and npos are those of _q.
extern "C" int zsg_loss_fwd_bwd_m(const float* out5, const float* annot, const float* anchors, int32_t B, int32_t A, float alpha,
                                  float gamma, float lamb_reg, float match_thr, int32_t flags, float grad_scale, int32_t iou_kind,
                                  float lamb_iou, int32_t cls_kind, const uint8_t* pos_mask, float* losses, float* grad5,
                                  int32_t* match_idx, int32_t* npos, void* ws, size_t ws_bytes, void* stream) {
    ZSG_REQUIRE(out5 && annot && anchors && pos_mask && losses && match_idx && ws && B > 0 && A > 0, "loss_fwd_bwd_m: bad argument");
    ZSG_REQUIRE(!((flags & 4) && (flags & 2)), "loss_fwd_bwd_m: use_softmax requires use_multi == False (loss.py:107)");
    ZSG_REQUIRE(iou_kind >= 0 && iou_kind <= 2, "loss_fwd_bwd_m: iou_kind=%d is none of 0 (none), 1 (giou), 2 (diou)", iou_kind);
    ZSG_REQUIRE(lamb_iou >= 0.f, "loss_fwd_bwd_m: lamb_iou must not be negative");
    ZSG_REQUIRE(cls_kind >= 0 && cls_kind <= 2, "loss_fwd_bwd_m: cls_kind=%d is none of 0 (none), 1 (qfl), 2 (vfl)", cls_kind);
    ZSG_REQUIRE(!cls_kind || ((flags & 1) && !(flags & 4)), "loss_fwd_bwd_m: cls_kind=%d needs use_focal and no use_softmax", cls_kind);
    ZSG_REQUIRE(!cls_kind || gamma >= 1.f, "loss_fwd_bwd_m: cls_kind=%d needs gamma >= 1 (the derivative is singular at sigmoid = q below)", cls_kind);
    if (ws_bytes < zsg_loss_workspace_bytes(B, A)) ZSG_FAIL(-2, "loss_fwd_bwd_m: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("loss_fwd_bwd_m", st, 0, (double)B * A * 5 * 4 * 3);
    ZSG_REQUIRE(B <= LS_MAX_B, "loss_fwd_bwd_m: B=%d exceeds %d", B, LS_MAX_B);
    loss_q_launch(out5, annot, anchors, B, A, alpha, gamma, lamb_reg, match_thr, flags, grad_scale, iou_kind, lamb_iou, cls_kind, losses,
                  grad5, match_idx, npos, ws, st, pos_mask);
    ZSG_CHECK_LAUNCH("loss_fwd_bwd_m");
    return 0;
}

// ---- ATSS anchor assignment (zsg_match_atss): the positives mask that zsg_loss_fwd_bwd_m consumes ------------------------------------
// Adaptive Training Sample Selection (Zhang et al. 2020) for one annotation g per sample, over the L pyramid levels of the anchor list
// (level l owns the indices [level_off[l], level_off[l + 1])); every step fp32 in this order (the file is compiled without contraction):
//   acy = (a.y1 + a.y2) / 2, acx likewise; gcy, gcx likewise;  d(a) = (acy - gcy)(acy - gcy) + (acx - gcx)(acx - gcx)
//   candidates C: per level the min(topk, n_l) anchors with the smallest key (d, index), lexicographic (the n anchors of a cell share
//                 their centre: the lower index wins), ordered by level, then by rank
//   v(a) = iou_exact(g, a);  t = mean(v over C) + std(v over C), fp64 from the fp32 values, summed in the order of C, the unbiased
//                 std (0 for one candidate): mean = sum v / |C|,  std = sqrt(sum (v - mean)^2 / (|C| - 1))
//   positive: (a in C and (double)v(a) >= t and g.y1 < acy < g.y2 and g.x1 < acx < g.x2)  or  a == the arg-max IoU anchor (lowest index)
// Two launches, no atomics, fixed orders: the same bits on every run.
//   atss_select_kernel, (L, B) blocks: the arg-max IoU of the level, then up to topk block-wide arg-min passes over the level, each taking
//     the smallest key greater than the winner before it (no marks), and records (index, v) per slot; unused slots get index -1.
//   atss_mask_kernel, (ranges of ATSS_TILE anchors, B) blocks: the <= 128 records of the sample into LDS, t by one thread, the range's
//     flags in LDS (one thread per candidate tests and sets its own), then EVERY byte of the range of pos_mask is written, 0 or 1.
#define ATSS_MAX_L 8
#define ATSS_MAX_K 16
#define ATSS_TILE 1024
struct AtssCand {
    int idx;
    float v;
};
struct AtssLevels {      // the level table, by value: level_off is a host array, checked before anything is launched
    int off[ATSS_MAX_L + 1];
};

extern "C" size_t zsg_match_atss_workspace_bytes(int32_t B, int32_t L) {   // per (sample, level): ATSS_MAX_K slot records + the level's arg-max
    return (size_t)B * L * (ATSS_MAX_K * sizeof(AtssCand) + sizeof(ArgMax));
}

__global__ __launch_bounds__(LS_THREADS) void atss_select_kernel(const float* __restrict__ annot, const float* __restrict__ anchors,
                                                                 AtssLevels lv, int topk, AtssCand* __restrict__ cand,
                                                                 ArgMax* __restrict__ lmax) {
    __shared__ ArgMax sm_a[LS_THREADS / 64];
    const int l = blockIdx.x, b = blockIdx.y, L = gridDim.x;
    const int lo = lv.off[l], hi = lv.off[l + 1];
    const f32x4 bx = *(const f32x4*)(annot + 4 * b);
    const float gcy = (bx[0] + bx[2]) / 2.f, gcx = (bx[1] + bx[3]) / 2.f;

    ArgMax m = {-INFINITY, 0x7fffffff};
    for (int a = lo + threadIdx.x; a < hi; a += LS_THREADS) {
        const float v = iou_exact(bx, *(const f32x4*)(anchors + 4 * a));
        if (v > m.v) { m.v = v; m.i = a; }
    }
    m = block_argmax(m, sm_a);
    if (threadIdx.x == 0) lmax[b * L + l] = m;

    AtssCand* out = cand + ((size_t)b * L + l) * ATSS_MAX_K;
    float pd = -INFINITY;                                // the winner before: every key (d, a) is greater than (-inf, -1)
    int pi = -1;
    bool more = true;
    for (int r = 0; r < ATSS_MAX_K; ++r) {
        AtssCand rec = {-1, 0.f};
        if (more && r < topk) {                          // (block-uniform)
            ArgMax w = {-INFINITY, 0x7fffffff};          // the arg-max of -d with the lowest index = the lexicographic minimum of (d, a)
            for (int a = lo + threadIdx.x; a < hi; a += LS_THREADS) {
                const f32x4 an = *(const f32x4*)(anchors + 4 * a);
                const float acy = (an[0] + an[2]) / 2.f, acx = (an[1] + an[3]) / 2.f;
                const float dy = acy - gcy, dx = acx - gcx;
                const float d = dy * dy + dx * dx;
                if ((d > pd || (d == pd && a > pi)) && -d > w.v) { w.v = -d; w.i = a; }
            }
            w = block_argmax(w, sm_a);
            more = w.i != 0x7fffffff;                    // the level is used up (n_l < topk)
            if (more) {
                pd = -w.v;
                pi = w.i;
                rec.idx = w.i;
                rec.v = iou_exact(bx, *(const f32x4*)(anchors + 4 * w.i));
            }
        }
        if (threadIdx.x == 0) out[r] = rec;
    }
}

__global__ __launch_bounds__(256) void atss_mask_kernel(const float* __restrict__ annot, const float* __restrict__ anchors, int A, int L,
                                                        const AtssCand* __restrict__ cand, const ArgMax* __restrict__ lmax,
                                                        uint8_t* __restrict__ pos_mask, double* __restrict__ thr_out,
                                                        int* __restrict__ cand_out) {
    __shared__ AtssCand sc[ATSS_MAX_L * ATSS_MAX_K];
    __shared__ uint8_t flag[ATSS_TILE];
    __shared__ double s_thr;
    __shared__ int s_best;
    const int b = blockIdx.y, t = threadIdx.x;
    const int a0 = blockIdx.x * ATSS_TILE, a1 = min(A, a0 + ATSS_TILE);
    const int nrec = L * ATSS_MAX_K;
    if (t < nrec) sc[t] = cand[(size_t)b * nrec + t];
    for (int i = t; i < ATSS_TILE; i += 256) flag[i] = 0;
    __syncthreads();
    if (t == 0) {
        int n = 0;
        double sum = 0;
        for (int k = 0; k < nrec; ++k)
            if (sc[k].idx >= 0) { sum += (double)sc[k].v; ++n; }
        const double mean = sum / (double)n;
        double ss = 0;
        for (int k = 0; k < nrec; ++k)
            if (sc[k].idx >= 0) { const double e = (double)sc[k].v - mean; ss += e * e; }
        s_thr = mean + (n > 1 ? sqrt(ss / (double)(n - 1)) : 0.0);
        ArgMax m = lmax[b * L];
        for (int l = 1; l < L; ++l) m = argmax_merge(m, lmax[b * L + l]);
        s_best = m.i == 0x7fffffff ? 0 : m.i;            // as the loss kernels
        if (blockIdx.x == 0) {
            if (thr_out) thr_out[b] = s_thr;
            if (cand_out) {                              // C in its order, -1 behind it
                int c = 0;
                for (int k = 0; k < nrec; ++k)
                    if (sc[k].idx >= 0) cand_out[b * (ATSS_MAX_L * ATSS_MAX_K) + c++] = sc[k].idx;
                for (; c < ATSS_MAX_L * ATSS_MAX_K; ++c) cand_out[b * (ATSS_MAX_L * ATSS_MAX_K) + c] = -1;
            }
        }
    }
    __syncthreads();
    if (t < nrec) {
        const int a = sc[t].idx;
        if (a >= a0 && a < a1) {
            const f32x4 bx = *(const f32x4*)(annot + 4 * b);
            const f32x4 an = *(const f32x4*)(anchors + 4 * a);
            const float acy = (an[0] + an[2]) / 2.f, acx = (an[1] + an[3]) / 2.f;
            const bool inside = bx[0] < acy && acy < bx[2] && bx[1] < acx && acx < bx[3];
            if (inside && (double)sc[t].v >= s_thr) flag[a - a0] = 1;
        }
    }
    if (t == 0 && s_best >= a0 && s_best < a1) flag[s_best - a0] = 1;     // (may meet a candidate's own write of the same 1)
    __syncthreads();
    for (int i = t; a0 + i < a1; i += 256) pos_mask[(size_t)b * A + a0 + i] = flag[i];
}

extern "C" int zsg_match_atss(const float* annot, const float* anchors, const int32_t* level_off, int32_t L, int32_t B, int32_t A,
                              int32_t topk, uint8_t* pos_mask, double* thr, int32_t* cand, void* ws, size_t ws_bytes, void* stream) {
    ZSG_REQUIRE(annot && anchors && level_off && pos_mask && ws && B > 0 && A > 0, "match_atss: bad argument");
    ZSG_REQUIRE(L >= 1 && L <= ATSS_MAX_L, "match_atss: L=%d levels, expected 1..%d", L, ATSS_MAX_L);
    ZSG_REQUIRE(topk >= 1 && topk <= ATSS_MAX_K, "match_atss: topk=%d, expected 1..%d", topk, ATSS_MAX_K);
    ZSG_REQUIRE(B <= LS_MAX_B, "match_atss: B=%d exceeds %d", B, LS_MAX_B);
    AtssLevels lv;
    ZSG_REQUIRE(level_off[0] == 0, "match_atss: level_off[0]=%d, expected 0", level_off[0]);
    for (int l = 0; l <= ATSS_MAX_L; ++l) lv.off[l] = level_off[l < L ? l : L];
    for (int l = 0; l < L; ++l)
        ZSG_REQUIRE(level_off[l + 1] > level_off[l], "match_atss: level_off[%d]=%d is not above level_off[%d]=%d", l + 1, level_off[l + 1], l,
                    level_off[l]);
    ZSG_REQUIRE(level_off[L] == A, "match_atss: level_off[%d]=%d, expected A=%d", L, level_off[L], A);
    if (ws_bytes < zsg_match_atss_workspace_bytes(B, L)) ZSG_FAIL(-2, "match_atss: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("match_atss", st, 0, (double)B * A * 16 * (topk + 1));
    AtssCand* recs = (AtssCand*)ws;
    ArgMax* lmax = (ArgMax*)(recs + (size_t)B * L * ATSS_MAX_K);
    ZSG_LAUNCH(atss_select_kernel, dim3(L, B), dim3(LS_THREADS), 0, st, annot, anchors, lv, topk, recs, lmax);
    ZSG_LAUNCH(atss_mask_kernel, dim3(cdiv(A, ATSS_TILE), B), dim3(256), 0, st, annot, anchors, A, L, (const AtssCand*)recs,
                       (const ArgMax*)lmax, pos_mask, thr, cand);
    ZSG_CHECK_LAUNCH("match_atss");
    return 0;
}

// ---- task-aligned anchor assignment (zsg_match_tal): a positives mask from what the network predicts --------------------------------
// TOOD's Task-Aligned Assigner (Feng et al. 2021) for one annotation g per sample.  Per anchor a with the row (dy, dx, dh, dw, att) of out5:
//   s = att_sigmoid(att) (fp32, the score of the quality term);  u = (float)decoded_iou(row, a, g): the q of zsg_loss_fwd_bwd_q, here for
//   EVERY anchor;  acy = (a.y1 + a.y2) / 2, acx likewise (fp32, zsg_match_atss's expressions);  inside = g.y1 < acy < g.y2 and g.x1 < acx < g.x2
//   t = pow((double)s, alpha) * pow((double)u, beta) in fp64; NaN where any of the row's five values is NaN or u is NaN (a decode that
//   overflows to inf - inf); said outright because pow(NaN, 0) is 1
//   candidate: inside and t > 0 (false for NaN);  selected: the min(topk, #candidates) candidates first in the order (t descending, index ascending)
// Two launches, no atomics, fixed orders: the same bits on every run.
//   tal_key_kernel, (ranges of 256 anchors, B) blocks: key[b][a] = inside ? t : -1.0 (a candidate is exactly a key > 0) and 0 into EVERY
//     byte of pos_mask.  The keys ARE the optional metric output: they are written into metric where it is given, else into ws.
//   tal_select_kernel, one block per sample: up to topk block-wide arg-max rounds over the sample's keys, which stay in global memory (L2:
//     A fp64 keys do not fit in LDS at A = 17460).  A thread keeps the best of its own keys that has not won; the winner's byte is set and
//     only the thread that owned it reads its keys again, for its largest key behind that winner (no marks).  A round is latency: the
//     fewer dependent L2 loads stand between two reductions, the shorter it is (the timings are in DESIGN section 7).
#define TAL_MAX_K 32
#define TAL_BATCH 8
struct ArgMaxD {
    double v;
    int i;
};
__device__ __forceinline__ ArgMaxD argmax_merge_d(ArgMaxD x, ArgMaxD y) {   // larger value, then lower index; NaN never wins
    const bool take = (y.v > x.v) || (y.v == x.v && y.i < x.i);
    return take ? y : x;
}
__device__ ArgMaxD block_argmax_d(ArgMaxD m, ArgMaxD* sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ArgMaxD y;
        y.v = __shfl_xor(m.v, o, 64);
        y.i = __shfl_xor(m.i, o, 64);
        m = argmax_merge_d(m, y);
    }
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[wave] = m;
    __syncthreads();
    ArgMaxD r = sm[0];
    for (int w = 1; w < nw; ++w) r = argmax_merge_d(r, sm[w]);
    __syncthreads();
    return r;
}

extern "C" size_t zsg_match_tal_workspace_bytes(int32_t B, int32_t A) {   // the fp64 keys [B][A] (where no metric output holds them)
    if (B <= 0 || A <= 0) return 0;
    return (size_t)B * (size_t)A * sizeof(double);
}

__global__ __launch_bounds__(256) void tal_key_kernel(const float* __restrict__ out5, const float* __restrict__ annot,
                                                      const float* __restrict__ anchors, int A, double alpha, double beta,
                                                      double* __restrict__ key, uint8_t* __restrict__ pos_mask) {
    const int b = blockIdx.y, a = blockIdx.x * 256 + threadIdx.x;
    if (a >= A) return;
    const f32x4 bx = *(const f32x4*)(annot + 4 * b);
    const f32x4 an = *(const f32x4*)(anchors + 4 * a);
    const size_t e = (size_t)b * A + a;
    const float* o = out5 + e * 5;
    const float acy = (an[0] + an[2]) / 2.f, acx = (an[1] + an[3]) / 2.f;
    const bool inside = bx[0] < acy && acy < bx[2] && bx[1] < acx && acx < bx[3];
    double t = -1.0;
    if (inside) {
        const float s = att_sigmoid(o[4]);
        const float u = (float)decoded_iou(o, an, bx);
        t = pow((double)s, alpha) * pow((double)u, beta);
        if (o[0] != o[0] || o[1] != o[1] || o[2] != o[2] || o[3] != o[3] || o[4] != o[4] || u != u) t = __longlong_as_double(0x7ff8000000000000ll);
    }
    key[e] = t;
    pos_mask[e] = 0;
}

__global__ __launch_bounds__(LS_THREADS) void tal_select_kernel(const double* __restrict__ key, int A, int topk,
                                                                uint8_t* __restrict__ pos_mask) {
    __shared__ ArgMaxD sm_a[LS_THREADS / 64];
    const int b = blockIdx.x;
    const double* k = key + (size_t)b * A;
    // every thread holds the best of ITS keys (a = threadIdx.x + j LS_THREADS) that has not won yet; after a round only the winner's
    // owner looks for its next one: the largest of its keys behind the winner in the order.  Every key (t, a) comes behind (+inf, -1).
    double pt = INFINITY;
    int pi = -1;
    bool rescan = true;
    ArgMaxD mine;
    for (int r = 0; r < topk; ++r) {
        if (rescan) {
            mine.v = 0.0;                                // only keys > 0 are candidates (never NaN, never the -1.0 of an outside anchor)
            mine.i = 0x7fffffff;
            // TAL_BATCH independent loads in flight, then the compares in index order: the scan costs latencies, not bytes
            for (int a0 = threadIdx.x; a0 < A; a0 += TAL_BATCH * LS_THREADS) {
                double v[TAL_BATCH];
#pragma unroll
                for (int j = 0; j < TAL_BATCH; ++j) {
                    const int a = a0 + j * LS_THREADS;
                    v[j] = j * LS_THREADS < A - a0 ? k[a] : -1.0;      // (a < A, written so that a cannot wrap)
                }
#pragma unroll
                for (int j = 0; j < TAL_BATCH; ++j) {
                    const int a = a0 + j * LS_THREADS;
                    if ((v[j] < pt || (v[j] == pt && a > pi)) && v[j] > mine.v) { mine.v = v[j]; mine.i = a; }
                }
            }
        }
        const ArgMaxD w = block_argmax_d(mine, sm_a);
        if (w.i == 0x7fffffff) break;                    // the candidates are used up (block-uniform)
        rescan = (w.i % LS_THREADS) == (int)threadIdx.x;
        if (rescan) {
            pt = w.v;
            pi = w.i;
            pos_mask[(size_t)b * A + w.i] = 1;
        }
    }
}

extern "C" int zsg_match_tal(const float* out5, const float* annot, const float* anchors, int32_t B, int32_t A, int32_t topk, float alpha,
                             float beta, uint8_t* pos_mask, double* metric, void* ws, size_t ws_bytes, void* stream) {
    ZSG_REQUIRE(out5 && annot && anchors && pos_mask && ws && B > 0 && A > 0, "match_tal: bad argument (a null pointer, B=%d or A=%d)", B, A);
    ZSG_REQUIRE(topk >= 1 && topk <= TAL_MAX_K, "match_tal: topk=%d, expected 1..%d", topk, TAL_MAX_K);
    ZSG_REQUIRE(B <= LS_MAX_B, "match_tal: B=%d exceeds %d", B, LS_MAX_B);
    ZSG_REQUIRE(alpha >= 0.f && alpha <= 3.402823466e38f, "match_tal: alpha=%g, expected a finite value >= 0", (double)alpha);
    ZSG_REQUIRE(beta >= 0.f && beta <= 3.402823466e38f, "match_tal: beta=%g, expected a finite value >= 0", (double)beta);
    ZSG_REQUIRE(ws_bytes >= zsg_match_tal_workspace_bytes(B, A), "match_tal: ws_bytes=%zu, expected at least %zu", ws_bytes,
                zsg_match_tal_workspace_bytes(B, A));
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("match_tal", st, 0, (double)B * A * (20 + 16 + 1 + 8 * (topk + 1)));
    double* key = metric ? metric : (double*)ws;        // (with metric given ws is not touched: the caller may pass one buffer as both)
    ZSG_LAUNCH(tal_key_kernel, dim3(cdiv(A, 256), B), dim3(256), 0, st, out5, annot, anchors, A, (double)alpha, (double)beta, key, pos_mask);
    ZSG_LAUNCH(tal_select_kernel, dim3(B), dim3(LS_THREADS), 0, st, (const double*)key, A, topk, pos_mask);
    ZSG_CHECK_LAUNCH("match_tal");
    return 0;
}

// ---- evaluator ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x4 decode_box(const f32x4 an, const float* __restrict__ r) {   // anchors.py:182-197
    const float acy = (an[0] + an[2]) / 2.f, acx = (an[1] + an[3]) / 2.f;
    const float ah = an[2] - an[0], aw = an[3] - an[1];
    const float cy = ah * r[0] + acy, cx = aw * r[1] + acx;
    const float h = expf(r[2]) * ah, w = expf(r[3]) * aw;
    f32x4 o = {cy - h / 2.f, cx - w / 2.f, cy + h / 2.f, cx + w / 2.f};
    return o;
}

// Two launches: (EV_CHUNKS x B) blocks find, per anchor range, the arg-max sigmoid score and the arg-max IoU anchor (lowest index
// wins, as torch.max); ONE block then merges the range records of every sample in range order (deterministic), decodes the two
// boxes per sample, scores them and averages.  (One block per sample walking all 17 460 anchors took 30 us at the end of every
// training step, where nothing else runs.)
#define EV_CHUNKS 16
__global__ __launch_bounds__(256) void eval_chunk_kernel(const float* __restrict__ out5, const float* __restrict__ annot,
                                                         const float* __restrict__ anchors, int A, ArgMax* __restrict__ rec) {
    __shared__ ArgMax sm_a[4];
    const int b = blockIdx.y, c = blockIdx.x;
    const int per = (A + EV_CHUNKS - 1) / EV_CHUNKS;
    const int a0 = c * per, a1 = min(A, a0 + per);
    const f32x4 bx = *(const f32x4*)(annot + 4 * b);
    const float* o = out5 + (size_t)b * A * 5;
    ArgMax ms = {-INFINITY, 0x7fffffff}, mi = {-INFINITY, 0x7fffffff};
    for (int a = a0 + threadIdx.x; a < a1; a += 256) {
        const float p = 1.0f / (1.0f + expf(-o[a * 5 + 4]));          // arg-max over sigmoid scores, evaluator.py:74-75
        if (p > ms.v) { ms.v = p; ms.i = a; }
        const float v = iou_exact(bx, *(const f32x4*)(anchors + 4 * a));
        if (v > mi.v) { mi.v = v; mi.i = a; }
    }
    ms = block_argmax(ms, sm_a);
    mi = block_argmax(mi, sm_a);
    if (threadIdx.x == 0) {
        rec[((size_t)b * EV_CHUNKS + c) * 2] = ms;
        rec[((size_t)b * EV_CHUNKS + c) * 2 + 1] = mi;
    }
}

__global__ __launch_bounds__(256) void eval_finish_kernel(const float* __restrict__ out5, const float* __restrict__ annot,
                                                          const float* __restrict__ anchors, const float* __restrict__ img_size, int B, int A,
                                                          float acc_thr, const ArgMax* __restrict__ rec, float* __restrict__ metrics,
                                                          float* __restrict__ pred_boxes, float* __restrict__ pred_scores,
                                                          int* __restrict__ pred_idx, int* __restrict__ best_idx) {
    __shared__ double sm_d[4];
    double ok_s = 0, ok_b = 0;
    for (int b = threadIdx.x; b < B; b += 256) {
        ArgMax ms = rec[(size_t)b * EV_CHUNKS * 2], mi = rec[(size_t)b * EV_CHUNKS * 2 + 1];
        for (int c = 1; c < EV_CHUNKS; ++c) {
            ms = argmax_merge(ms, rec[((size_t)b * EV_CHUNKS + c) * 2]);
            mi = argmax_merge(mi, rec[((size_t)b * EV_CHUNKS + c) * 2 + 1]);
        }
        const f32x4 bx = *(const f32x4*)(annot + 4 * b);
        const float* o = out5 + (size_t)b * A * 5;
        const int ps = ms.i == 0x7fffffff ? 0 : ms.i, pb = mi.i == 0x7fffffff ? 0 : mi.i;
        const f32x4 box_s = decode_box(*(const f32x4*)(anchors + 4 * ps), o + ps * 5);
        const f32x4 box_b = decode_box(*(const f32x4*)(anchors + 4 * pb), o + pb * 5);
        ok_s += iou_exact(box_s, bx) >= acc_thr ? 1.0 : 0.0;
        ok_b += iou_exact(box_b, bx) >= acc_thr ? 1.0 : 0.0;
        const float hh = img_size[2 * b], ww = img_size[2 * b + 1];
        // (box+1)/2 * (h,w) then y1x1y2x2 -> x1y1x2y2  (evaluator.py:96-98, reshape :10-17)
        pred_boxes[4 * b + 0] = ww * ((box_s[1] + 1.f) / 2.f);
        pred_boxes[4 * b + 1] = hh * ((box_s[0] + 1.f) / 2.f);
        pred_boxes[4 * b + 2] = ww * ((box_s[3] + 1.f) / 2.f);
        pred_boxes[4 * b + 3] = hh * ((box_s[2] + 1.f) / 2.f);
        pred_scores[b] = ms.v;
        if (pred_idx) pred_idx[b] = ps;
        if (best_idx) best_idx[b] = pb;
    }
    ok_s = block_sum_d(ok_s, sm_d);                 // (counts of 0 / 1: exact in any order)
    ok_b = block_sum_d(ok_b, sm_d);
    if (threadIdx.x == 0) {
        metrics[0] = (float)ok_s / (float)B;
        metrics[1] = (float)ok_b / (float)B;
    }
}

extern "C" size_t zsg_eval_workspace_bytes(int32_t B) { return (size_t)B * EV_CHUNKS * 2 * sizeof(ArgMax); }

extern "C" int zsg_eval(const float* out5, const float* annot, const float* anchors, const float* img_size, int32_t B, int32_t A,
                        float acc_thr, float* metrics, float* pred_boxes, float* pred_scores, int32_t* pred_idx, int32_t* best_idx,
                        float* ws_ok, void* stream) {
    ZSG_REQUIRE(out5 && annot && anchors && img_size && metrics && pred_boxes && pred_scores && ws_ok && B > 0 && A > 0, "eval: bad argument");
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("eval", st, 0, (double)B * A * 5 * 4);
    ArgMax* rec = (ArgMax*)ws_ok;                    // [B][EV_CHUNKS][2]
    ZSG_LAUNCH(eval_chunk_kernel, dim3(EV_CHUNKS, B), dim3(256), 0, st, out5, annot, anchors, A, rec);
    ZSG_LAUNCH(eval_finish_kernel, dim3(1), dim3(256), 0, st, out5, annot, anchors, img_size, B, A, acc_thr, (const ArgMax*)rec, metrics,
                       pred_boxes, pred_scores, pred_idx, best_idx);
    ZSG_CHECK_LAUNCH("eval");
    return 0;
}

// ---- top-k grounding: score ranking + greedy NMS per query -----------------------------------------------------------
// Ordering contract: candidates are ranked by (sigmoid score descending, anchor index ascending); a NaN score ranks below every
// number.  One 64-bit composite carries it: the high word is the score's bit pattern + 1 (scores are in [0, 1], so the pattern is
// monotone; 0 is left for NaN), the low word is ~index, and a larger composite is a better rank.  Composite 0 (index 0xffffffff) is
// padding.  Rank 0 is therefore the anchor eval_chunk_kernel / argmax_merge pick, saturated scores and all-NaN rows included.
// Three launches, the evaluator's two-stage pattern: (EV_CHUNKS x B) blocks each sort their anchor range in LDS and leave its best
// pre_n composites, sorted, in the workspace; one block per query merges the EV_CHUNKS lists by rank counting (composites are unique,
// so the rank of one is the number of larger ones: a binary search per list, no barriers), decodes the pre_n boxes into LDS and
// runs K rounds of "the first candidate still alive is kept; every later one is tested against it"; one tiny block averages.
typedef unsigned long long u64;
#define TK_SORT 2048            // LDS sort buffer of a range block (composites)
#define TK_MAX_PRE 512
#define TK_MAX_K 64
#define TK_LDS_PRE 256          // the finishing block keeps the lists in LDS up to this pre_n (32 KB), beyond it it reads them from L2

__device__ __forceinline__ u64 tk_pack(float p, int a) {
    const unsigned key = (p != p) ? 0u : __float_as_uint(p) + 1u;
    return ((u64)key << 32) | (unsigned)~a;
}
__device__ __forceinline__ float tk_score(u64 c) {
    const unsigned key = (unsigned)(c >> 32);
    return key ? __uint_as_float(key - 1u) : __uint_as_float(0x7fc00000u);
}
__device__ __forceinline__ int tk_index(u64 c) { return (int)~(unsigned)c; }

__global__ __launch_bounds__(256) void topk_chunk_kernel(const float* __restrict__ out5, int A, int pre_n, u64* __restrict__ lists) {
    __shared__ u64 sm[TK_SORT];
    const int b = blockIdx.y, c = blockIdx.x;
    const int per = (A + EV_CHUNKS - 1) / EV_CHUNKS;
    const int a0 = min(A, c * per), a1 = min(A, a0 + per);
    const float* o = out5 + (size_t)b * A * 5;
    u64* dst = lists + ((size_t)b * EV_CHUNKS + c) * pre_n;
    if (a0 >= a1) {                                                // an empty range (A < EV_CHUNKS ranges): padding only
        for (int i = threadIdx.x; i < pre_n; i += 256) dst[i] = 0;
        return;
    }
    int N = 64;                                                   // sort width: the carried list + one tile of the range
    while (N < pre_n + (a1 - a0) && N < TK_SORT) N <<= 1;       // (N > pre_n: the range is not empty and pre_n <= 512 < TK_SORT)
    const int tile = N - pre_n;
    for (int i = threadIdx.x; i < pre_n; i += 256) sm[i] = 0;
    int base = a0;
    do {
        for (int i = threadIdx.x; i < tile; i += 256) {
            const int a = base + i;
            u64 v = 0;
            if (a < a1) v = tk_pack(1.0f / (1.0f + expf(-o[a * 5 + 4])), a);     // the score expression of eval_chunk_kernel
            sm[pre_n + i] = v;
        }
        __syncthreads();
        for (int k = 2; k <= N; k <<= 1) {                         // bitonic sort, descending
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = threadIdx.x; i < (N >> 1); i += 256) {
                    const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                    const u64 x = sm[lo], y = sm[hi];
                    const bool desc = (lo & k) == 0;
                    if (desc ? (x < y) : (x > y)) { sm[lo] = y; sm[hi] = x; }
                }
                __syncthreads();
            }
        }
        base += tile;
    } while (base < a1);
    for (int i = threadIdx.x; i < pre_n; i += 256) dst[i] = sm[i];
}

__device__ __forceinline__ int tk_count_greater(const u64* l, int n, u64 x) {     // l sorted descending
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (l[mid] > x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void topk_finish_kernel(const float* __restrict__ out5, const float* __restrict__ annot,
                                                          const float* __restrict__ anchors, const float* __restrict__ img_size, int A,
                                                          int pre_n, int K, float nms_thr, float acc_thr, const u64* __restrict__ lists,
                                                          float* __restrict__ topk_boxes, float* __restrict__ topk_scores,
                                                          int* __restrict__ topk_idx, int* __restrict__ topk_n, int* __restrict__ hit_rank) {
    __shared__ u64 sm_lists[EV_CHUNKS * TK_LDS_PRE];
    __shared__ u64 sm_cand[TK_MAX_PRE];
    __shared__ f32x4 sm_box[TK_MAX_PRE];
    __shared__ u64 sm_alive[2][2 * 4];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    const float* o = out5 + (size_t)b * A * 5;
    const u64* L = lists + (size_t)b * EV_CHUNKS * pre_n;
    const int nl = EV_CHUNKS * pre_n;
    for (int r = tid; r < TK_MAX_PRE; r += 256) sm_cand[r] = 0;
    if (pre_n <= TK_LDS_PRE) {
        for (int e = tid; e < nl; e += 256) sm_lists[e] = L[e];
        L = sm_lists;
    }
    __syncthreads();
    for (int e = tid; e < nl; e += 256) {                          // merge: a composite's rank is the number of larger ones
        const u64 x = L[e];
        if (x == 0) continue;
        int r = 0;
        for (int c = 0; c < EV_CHUNKS; ++c) r += tk_count_greater(L + c * pre_n, pre_n, x);
        if (r < pre_n) sm_cand[r] = x;
    }
    __syncthreads();
    const int nc = min(pre_n, A);
    bool alive[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {                                  // candidate r = tid + 256 s
        const int r = tid + 256 * s;
        const int a = r < nc ? tk_index(sm_cand[r]) : -1;
        alive[s] = (unsigned)a < (unsigned)A;                      // (every rank below nc is filled; the test keeps a stray index off memory)
        if (alive[s]) sm_box[r] = decode_box(*(const f32x4*)(anchors + 4 * a), o + a * 5);
    }
    f32x4 gt = {0.f, 0.f, 0.f, 0.f};
    if (annot) gt = *(const f32x4*)(annot + 4 * b);
    const float hh = img_size[2 * b], ww = img_size[2 * b + 1];
    int kept = 0, hit = K;
    for (; kept < K; ++kept) {
        u64* al = sm_alive[kept & 1];
        const u64 m0 = __ballot(alive[0]), m1 = __ballot(alive[1]);
        if ((tid & 63) == 0) { al[wave] = m0; al[4 + wave] = m1; }
        __syncthreads();                                           // (also orders sm_box before the first round's reads)
        int first = -1;
        for (int q = 7; q >= 0; --q) {
            const u64 m = al[q];
            if (m) first = 64 * q + __builtin_ctzll(m);
        }
        if (first < 0) break;                                      // block-uniform
        const f32x4 kb = sm_box[first];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int r = tid + 256 * s;
            if (alive[s] && (r == first || iou_exact(kb, sm_box[r]) > nms_thr)) alive[s] = false;
        }
        if (tid == 0) {
            const u64 cd = sm_cand[first];
            float* pb = topk_boxes + ((size_t)b * K + kept) * 4;
            // (box+1)/2 * (h,w) then y1x1y2x2 -> x1y1x2y2, the expressions of eval_finish_kernel
            pb[0] = ww * ((kb[1] + 1.f) / 2.f);
            pb[1] = hh * ((kb[0] + 1.f) / 2.f);
            pb[2] = ww * ((kb[3] + 1.f) / 2.f);
            pb[3] = hh * ((kb[2] + 1.f) / 2.f);
            topk_scores[(size_t)b * K + kept] = tk_score(cd);
            topk_idx[(size_t)b * K + kept] = tk_index(cd);
            if (annot && hit == K && iou_exact(kb, gt) >= acc_thr) hit = kept;
        }
    }
    for (int k = kept + tid; k < K; k += 256) {                    // rows past topk_n
        float* pb = topk_boxes + ((size_t)b * K + k) * 4;
        pb[0] = pb[1] = pb[2] = pb[3] = 0.f;
        topk_scores[(size_t)b * K + k] = 0.f;
        topk_idx[(size_t)b * K + k] = -1;
    }
    if (tid == 0) {
        topk_n[b] = kept;
        if (hit_rank) hit_rank[b] = hit;
    }
}

__global__ __launch_bounds__(64) void topk_acc_kernel(const int* __restrict__ hit_rank, int B, int K, float* __restrict__ acc_at) {
    const int j = threadIdx.x;
    if (j >= K) return;
    double ok = 0;                                                 // (counts of 0 / 1: exact in any order)
    for (int b = 0; b < B; ++b) ok += hit_rank[b] <= j ? 1.0 : 0.0;
    acc_at[j] = (float)ok / (float)B;
}

extern "C" size_t zsg_eval_topk_workspace_bytes(int32_t B, int32_t A, int32_t pre_n, int32_t K) {
    (void)A; (void)K;
    if (B <= 0 || pre_n <= 0) return 0;
    return (size_t)B * EV_CHUNKS * (size_t)pre_n * sizeof(u64);
}

extern "C" int zsg_eval_topk(const float* out5, const float* annot, const float* anchors, const float* img_size, int32_t B, int32_t A,
                             int32_t pre_n, int32_t K, float nms_thr, float acc_thr, float* topk_boxes, float* topk_scores,
                             int32_t* topk_idx, int32_t* topk_n, int32_t* hit_rank, float* acc_at, void* ws, void* stream) {
    ZSG_REQUIRE(out5 && anchors && img_size && topk_boxes && topk_scores && topk_idx && topk_n && ws, "eval_topk: null pointer argument");
    ZSG_REQUIRE(B > 0 && B <= 65535 && A > 0, "eval_topk: bad shape B=%d A=%d", B, A);
    ZSG_REQUIRE(pre_n >= 1 && pre_n <= TK_MAX_PRE, "eval_topk: pre_n=%d outside 1..%d", pre_n, TK_MAX_PRE);
    ZSG_REQUIRE(K >= 1 && K <= TK_MAX_K, "eval_topk: K=%d outside 1..%d", K, TK_MAX_K);
    ZSG_REQUIRE(K <= pre_n, "eval_topk: K=%d exceeds pre_n=%d", K, pre_n);
    ZSG_REQUIRE(!hit_rank || annot, "eval_topk: hit_rank needs annot");
    ZSG_REQUIRE(!acc_at || hit_rank, "eval_topk: acc_at needs hit_rank");
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("eval_topk", st, 0, (double)B * A * 4);
    u64* lists = (u64*)ws;                           // [B][EV_CHUNKS][pre_n]
    ZSG_LAUNCH(topk_chunk_kernel, dim3(EV_CHUNKS, B), dim3(256), 0, st, out5, A, pre_n, lists);
    ZSG_LAUNCH(topk_finish_kernel, dim3(B), dim3(256), 0, st, out5, annot, anchors, img_size, A, pre_n, K, nms_thr, acc_thr,
                       (const u64*)lists, topk_boxes, topk_scores, topk_idx, topk_n, hit_rank);
    if (acc_at) ZSG_LAUNCH(topk_acc_kernel, dim3(1), dim3(64), 0, st, (const int*)hit_rank, B, K, acc_at);
    ZSG_CHECK_LAUNCH("eval_topk");
    return 0;
}

__global__ void iou_kernel(const float* __restrict__ boxes, const float* __restrict__ anchors, int B, int A, float* __restrict__ iou) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * A) return;
    const int b = (int)(i / A), a = (int)(i % A);
    iou[i] = iou_exact(*(const f32x4*)(boxes + 4 * b), *(const f32x4*)(anchors + 4 * a));
}
extern "C" int zsg_iou(const float* boxes, const float* anchors, int32_t B, int32_t A, float* iou, void* stream) {
    ZSG_REQUIRE(boxes && anchors && iou && B > 0 && A > 0, "iou: bad argument");
    ZSG_LAUNCH(iou_kernel, dim3(cdiv((int64_t)B * A, 256)), dim3(256), 0, (hipStream_t)stream, boxes, anchors, B, A, iou);
    ZSG_CHECK_LAUNCH("iou");
    return 0;
}
