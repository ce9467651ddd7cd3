// adam.hip — fused Adam over one flat fp32 parameter buffer (torch.optim.Adam semantics, amsgrad off).  HBM-bound:
// reads p,g,m,v and writes p,m,v once: 28 B per parameter.  With the weight average riding in the launch (adam_kernel<true>,
// zsg_adam_step_ema) it reads and writes ema too: 36 B per parameter, against 28 + 12 for the step followed by zsg_ema_update.
#include "common.h"
#include "ema.h"

// The step counter lives on the device (the launch is hipGraph-capturable): step[0] = steps taken, step[1] = the ticket of the launch
// in flight — both belong to ONE optimizer (two optimizers stepping on different streams never share a ticket).  Every block reads
// step[0] when it starts and uses t = count + 1; the block that FINISHES last (ticket) publishes t and clears the ticket — by then
// every block has read the old value.  (A separate one-thread "tick" launch ahead of the update was 8 us of dependent launch at the
// end of every step.)

// EMA: the weight average takes the freshly updated p before it is stored (ema.h's rule: the bits zsg_ema_update gives on the stored p).
template <bool EMA>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t n4, int64_t n, float lr, float b1, float b2, float eps,
                                                   float wd, float gs, int* step, int tick, float* __restrict__ ema, float ema_w) {
    const int t = __hip_atomic_load(step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
    const float bc1 = 1.f - powf(b1, (float)t);
    const float bc2s = sqrtf(1.f - powf(b2, (float)t));
    const float step_size = lr / bc1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 pp = *(const f32x4*)(p + 4 * i);
        f32x4 gg = *(const f32x4*)(g + 4 * i) * gs;
        f32x4 mm = *(const f32x4*)(m + 4 * i);
        f32x4 vv = *(const f32x4*)(v + 4 * i);
        if (wd != 0.f) gg += pp * wd;
        mm = mm * b1 + gg * (1.f - b1);
        vv = vv * b2 + gg * gg * (1.f - b2);
#pragma unroll
        for (int e = 0; e < 4; ++e) pp[e] -= step_size * (mm[e] / (sqrtf(vv[e]) / bc2s + eps));
        *(f32x4*)(p + 4 * i) = pp;
        *(f32x4*)(m + 4 * i) = mm;
        *(f32x4*)(v + 4 * i) = vv;
        if (EMA) {
            f32x4 ee = *(const f32x4*)(ema + 4 * i);
#pragma unroll
            for (int e = 0; e < 4; ++e) ee[e] = zsg_ema_rule(ee[e], pp[e], ema_w);
            *(f32x4*)(ema + 4 * i) = ee;
        }
    }
    // tail (n not a multiple of 4)
    if (blockIdx.x == 0 && threadIdx.x < (int)(n - 4 * n4)) {
        const int64_t i = 4 * n4 + threadIdx.x;
        float gg = g[i] * gs;
        if (wd != 0.f) gg += p[i] * wd;
        const float mm = m[i] * b1 + gg * (1.f - b1);
        const float vv = v[i] * b2 + gg * gg * (1.f - b2);
        p[i] -= step_size * (mm / (sqrtf(vv) / bc2s + eps));
        m[i] = mm;
        v[i] = vv;
        if (EMA) ema[i] = zsg_ema_rule(ema[i], p[i], ema_w);
    }
    if (!tick) return;          // (a partial update of the step: the launch that covers the rest publishes the counter)
    __syncthreads();
    if (threadIdx.x == 0 && __hip_atomic_fetch_add(step + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1) {
        __hip_atomic_store(step + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(step, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

static int adam_launch(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                       float weight_decay, float grad_scale, int32_t* step_count, int tick, float* ema, float ema_w, void* stream) {
    ZSG_REQUIRE(p && g && m && v && step_count && n > 0, "adam_step: bad argument");
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF(ema ? "adam_step_ema" : "adam_step", st, 0, (double)n * (ema ? 36 : 28));
    const int64_t n4 = n / 4;
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > ZSG_NUM_CU * 8) blocks = ZSG_NUM_CU * 8;
    if (blocks < 1) blocks = 1;
    if (ema)
        ZSG_LAUNCH(adam_kernel<true>, dim3((int)blocks), dim3(256), 0, st, p, g, m, v, n4, n, lr, beta1, beta2, eps, weight_decay, grad_scale,
                   step_count, tick, ema, ema_w);
    else
        ZSG_LAUNCH(adam_kernel<false>, dim3((int)blocks), dim3(256), 0, st, p, g, m, v, n4, n, lr, beta1, beta2, eps, weight_decay, grad_scale,
                   step_count, tick, ema, ema_w);
    ZSG_CHECK_LAUNCH("adam_step");
    return 0;
}

extern "C" int zsg_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                             float weight_decay, float grad_scale, int32_t* step_count, void* stream) {
    return adam_launch(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, grad_scale, step_count, 1, nullptr, 0.f, stream);
}

// The same step with the weight average updated in the launch: ema <- ema.h's rule on the p this step stores.
extern "C" int zsg_adam_step_ema(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                                 float weight_decay, float grad_scale, int32_t* step_count, float* ema, float ema_w, void* stream) {
    ZSG_REQUIRE(ema, "adam_step_ema: null average buffer");
    ZSG_REQUIRE(ema_w >= 0.f && ema_w <= 1.f, "adam_step_ema: weight %g outside [0, 1]", (double)ema_w);
    ZSG_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) == 0, "adam_step_ema: buffers must be 16-byte aligned");
    return adam_launch(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, grad_scale, step_count, 1, ema, ema_w, stream);
}

// One optimizer step as several launches over disjoint ranges of the flat buffer (so that the part whose gradients are complete can
// be updated while the last weight gradients are still being computed): every launch of the step computes with t = counter + 1;
// exactly the LAST one passes publish = 1 and advances the counter.
extern "C" int zsg_adam_step_range(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                                   float weight_decay, float grad_scale, int32_t* step_count, int32_t publish, void* stream) {
    return adam_launch(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, grad_scale, step_count, publish ? 1 : 0, nullptr, 0.f, stream);
}

// ---- Adam over listed segments (fine-tuning: frozen parameters, parameter groups) -----------------------------------------------------
// One block per work chunk of <= ZSG_ADAM_CHUNK elements of one segment (the segment table gives each segment's first chunk), so the
// loop body is adam_kernel's, vectorised, with the segment's own hyperparameters and bias correction.  Nothing outside the listed
// ranges is read or written.  The counters follow adam_kernel's ticket scheme: every block reads the counter of its segment when it
// starts; the block that finishes last (by then every block has read) advances the counters of all listed segments.

struct AdamGroups {
    zsg_adam_group g[ZSG_ADAM_MAX_GROUPS];
};

__global__ __launch_bounds__(256) void adam_segments_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, const zsg_adam_seg* __restrict__ segs, int nseg,
                                                            AdamGroups hp, float gs, int* counters, int* ticket) {
    // the segment of this chunk: the last one whose chunk0 <= blockIdx.x (block-uniform binary search)
    const int c = blockIdx.x;
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].chunk0 <= c) lo = mid;
        else hi = mid - 1;
    }
    const zsg_adam_seg sg = segs[lo];
    const zsg_adam_group h = hp.g[sg.group];
    const float lr = h.lr, b1 = h.beta1, b2 = h.beta2, eps = h.eps, wd = h.weight_decay;
    const int t = __hip_atomic_load(counters + sg.counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
    const float bc1 = 1.f - powf(b1, (float)t);
    const float bc2s = sqrtf(1.f - powf(b2, (float)t));
    const float step_size = lr / bc1;
    const int64_t start = (int64_t)(c - sg.chunk0) * ZSG_ADAM_CHUNK;
    const int64_t rem = sg.len - start;
    const int cnt = rem < ZSG_ADAM_CHUNK ? (int)rem : ZSG_ADAM_CHUNK;
    const int n4 = cnt >> 2;
    float* pb = p + sg.off + start;
    const float* gb = g + sg.off + start;
    float* mb = m + sg.off + start;
    float* vb = v + sg.off + start;
    for (int i = threadIdx.x; i < n4; i += blockDim.x) {
        f32x4 pp = *(const f32x4*)(pb + 4 * i);
        f32x4 gg = *(const f32x4*)(gb + 4 * i) * gs;
        f32x4 mm = *(const f32x4*)(mb + 4 * i);
        f32x4 vv = *(const f32x4*)(vb + 4 * i);
        if (wd != 0.f) gg += pp * wd;
        mm = mm * b1 + gg * (1.f - b1);
        vv = vv * b2 + gg * gg * (1.f - b2);
#pragma unroll
        for (int e = 0; e < 4; ++e) pp[e] -= step_size * (mm[e] / (sqrtf(vv[e]) / bc2s + eps));
        *(f32x4*)(pb + 4 * i) = pp;
        *(f32x4*)(mb + 4 * i) = mm;
        *(f32x4*)(vb + 4 * i) = vv;
    }
    // tail of a segment whose length is not a multiple of 4 (its last chunk only)
    if ((int)threadIdx.x < cnt - 4 * n4) {
        const int i = 4 * n4 + threadIdx.x;
        float gg = gb[i] * gs;
        if (wd != 0.f) gg += pb[i] * wd;
        const float mm = mb[i] * b1 + gg * (1.f - b1);
        const float vv = vb[i] * b2 + gg * gg * (1.f - b2);
        pb[i] -= step_size * (mm / (sqrtf(vv) / bc2s + eps));
        mb[i] = mm;
        vb[i] = vv;
    }
    __shared__ int last;
    __syncthreads();
    if (threadIdx.x == 0) last = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
    __syncthreads();
    if (!last) return;
    for (int s = threadIdx.x; s < nseg; s += blockDim.x) {
        const int k = segs[s].counter;
        const int old = __hip_atomic_load(counters + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(counters + k, old + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

extern "C" int zsg_adam_step_segments(float* p, const float* g, float* m, float* v, const zsg_adam_seg* segs, int32_t nseg,
                                      int32_t nchunks, const zsg_adam_group* groups, int32_t ngroups, float grad_scale,
                                      int32_t* counters, int32_t* ticket, void* stream) {
    ZSG_REQUIRE(p && g && m && v && segs && groups && counters && ticket, "adam_step_segments: null pointer");
    ZSG_REQUIRE(ngroups >= 1 && ngroups <= ZSG_ADAM_MAX_GROUPS, "adam_step_segments: %d parameter groups (1..%d supported)", ngroups,
                ZSG_ADAM_MAX_GROUPS);
    ZSG_REQUIRE(nseg >= 0 && nchunks >= nseg, "adam_step_segments: %d segments in %d chunks", nseg, nchunks);
    ZSG_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "adam_step_segments: buffers must be 16-byte aligned");
    if (nseg == 0) return 0;          // nothing is stepped: no launch, no counter moves
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("adam_step_segments", st, 0, (double)nchunks * ZSG_ADAM_CHUNK * 28);      // (bytes: an upper bound)
    AdamGroups hp = {};
    for (int i = 0; i < ngroups; ++i) hp.g[i] = groups[i];
    ZSG_LAUNCH(adam_segments_kernel, dim3(nchunks), dim3(256), 0, st, p, g, m, v, segs, (int)nseg, hp, grad_scale, counters, ticket);
    ZSG_CHECK_LAUNCH("adam_step_segments");
    return 0;
}
