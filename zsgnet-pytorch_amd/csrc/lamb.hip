// lamb.hip — fused LAMB (You et al., "Large Batch Optimization for Deep Learning") over listed segments of the flat fp32 parameter buffer:
// Adam's moments, and the update of every parameter tensor rescaled by its trust ratio |w| / |u|.  The definition is include/zsg.h's
// ("Fused LAMB"); tests/lamb_ref.py is its host twin.  Two launches through zsg_adam_step_segments' segment table (one block of 256
// threads per work chunk of <= ZSG_ADAM_CHUNK elements of one segment, 16-byte accesses plus a tail), no host round trip:
//     zsg_lamb_moments   reads p, g, m, v, stores m, v, forms u in registers and the chunk's fp64 sums of w^2 and u^2; the block that
//                        arrives last reduces them per segment and writes ratio / |w| / |u|                       24 B per parameter
//     zsg_lamb_apply     reads p, m, v and the segment's ratio, forms the same u again, stores p -= lr * ratio * u;  the block that
//                        finishes last advances the listed counters                                               16 B per parameter
// HBM-bound: 24 + 16 = 40 B per parameter (Adam's single pass: 28).  u is not stored between the launches (that would be 28 + 20 B).
//
// This file is compiled with -ffp-contract=off (Makefile) and both kernels form u with the one function lamb_u from the stored m, v:
// every operation rounds on its own, so the u whose norm sets the ratio and the u that is applied are the same bits.  No float atomics:
// the per-segment sums are combined in an order fixed by the chunk index (lane l of a wave takes chunks l, l + 64, ... of the segment in
// index order, then xor-shuffles), with grad_norm_kernel's ticket hand-off (clip.hip) — the same bits from run to run.
#include "common.h"

struct LambGroups {
    zsg_lamb_group g[ZSG_ADAM_MAX_GROUPS];
};

// What the rule needs of one hyperparameter set at step t (uniform over a block).  The bias corrections 1 - beta^t are formed in fp64
// and rounded once to fp32 (tests/lamb_ref.py does the same): exact whenever 1 - beta^t is a float.
struct LambCoef {
    float b1, b2, omb1, omb2, bc1, bc2, eps, wd;
};

__device__ __forceinline__ LambCoef lamb_coef(const zsg_lamb_group& h, int t) {
    LambCoef c;
    c.b1 = h.beta1;
    c.b2 = h.beta2;
    c.omb1 = 1.f - h.beta1;
    c.omb2 = 1.f - h.beta2;
    c.bc1 = (float)(1.0 - pow((double)h.beta1, (double)t));
    c.bc2 = (float)(1.0 - pow((double)h.beta2, (double)t));
    c.eps = h.eps;
    c.wd = h.weight_decay;
    return c;
}

// u of one element from its stored moments and its weight (fp32, every operation rounded on its own)
__device__ __forceinline__ float lamb_u(float m, float v, float w, const LambCoef& c) {
    return (m / c.bc1) / (sqrtf(v / c.bc2) + c.eps) + c.wd * w;
}

__device__ __forceinline__ void lamb_moments(float& m, float& v, float g, const LambCoef& c) {
    m = c.b1 * m + c.omb1 * g;
    v = c.b2 * v + c.omb2 * (g * g);
}

// the segment index of work chunk ch: the last one whose chunk0 <= ch (block-uniform binary search, as adam_segments_kernel)
__device__ __forceinline__ int lamb_segment_of(const zsg_adam_seg* __restrict__ segs, int nseg, int ch) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].chunk0 <= ch) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// elements of chunk ch of segment sg (0 for a chunk behind the segment's end: a table whose nchunks overstates it touches nothing)
__device__ __forceinline__ int lamb_chunk_count(const zsg_adam_seg& sg, int ch, int64_t* base) {
    const int64_t start = (int64_t)(ch - sg.chunk0) * ZSG_ADAM_CHUNK;
    const int64_t rem = sg.len - start;
    *base = sg.off + start;
    return rem <= 0 ? 0 : rem < ZSG_ADAM_CHUNK ? (int)rem : ZSG_ADAM_CHUNK;
}

__device__ __forceinline__ double lamb_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- launch 1: the moments and the norms ----------------------------------------------------------------------------------------------
// partials[2 * chunk] = the chunk's sum of w^2, [2 * chunk + 1] = of u^2 (fp64).  Hand-off as grad_norm_kernel (cdna_hip_programming.md
// Guideline 16, counter form): thread 0 stores both write-through (agent-scope atomic stores: sc1), drains them (s_waitcnt vmcnt(0))
// before its ticket add; the last arriver — told by the value its add returns — acquires at agent scope and reads the partials with
// agent-scope atomic loads.  It then takes the segments a wave at a time, four segments' loads in flight per wave.
__global__ __launch_bounds__(256) void lamb_moments_kernel(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, const zsg_adam_seg* __restrict__ segs, int nseg,
                                                           LambGroups hp, float gs, const int* counters, double* partials, int* ticket,
                                                           float* ratio, float* norm_w, float* norm_u) {
    __shared__ double sh[8];
    __shared__ int last;
    const int ch = blockIdx.x;
    const zsg_adam_seg sg = segs[lamb_segment_of(segs, nseg, ch)];
    const int t = __hip_atomic_load(counters + sg.counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
    const LambCoef c = lamb_coef(hp.g[sg.group], t);
    int64_t base;
    const int cnt = lamb_chunk_count(sg, ch, &base);
    const int n4 = cnt >> 2;
    const float* pb = p + base;
    const float* gb = g + base;
    float* mb = m + base;
    float* vb = v + base;
    double sw = 0.0, su = 0.0;
    for (int i = threadIdx.x; i < n4; i += 256) {
        const f32x4 pp = *(const f32x4*)(pb + 4 * i);
        const f32x4 gg = *(const f32x4*)(gb + 4 * i) * gs;
        f32x4 mm = *(const f32x4*)(mb + 4 * i);
        f32x4 vv = *(const f32x4*)(vb + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float me = mm[e], ve = vv[e];
            lamb_moments(me, ve, gg[e], c);
            mm[e] = me, vv[e] = ve;
            const float u = lamb_u(me, ve, pp[e], c);
            sw += (double)pp[e] * (double)pp[e];
            su += (double)u * (double)u;
        }
        *(f32x4*)(mb + 4 * i) = mm;
        *(f32x4*)(vb + 4 * i) = vv;
    }
    // tail of a segment whose length is not a multiple of 4 (its last chunk only)
    if ((int)threadIdx.x < cnt - 4 * n4) {
        const int i = 4 * n4 + threadIdx.x;
        const float w = pb[i];
        float me = mb[i], ve = vb[i];
        lamb_moments(me, ve, gb[i] * gs, c);
        mb[i] = me, vb[i] = ve;
        const float u = lamb_u(me, ve, w, c);
        sw += (double)w * (double)w;
        su += (double)u * (double)u;
    }
    // fixed-shape block reduction: xor-shuffles inside each wave, then the 4 wave results in wave order
    sw = lamb_wave_sum(sw);
    su = lamb_wave_sum(su);
    if ((threadIdx.x & 63) == 0) {
        sh[threadIdx.x >> 6] = sw;
        sh[4 + (threadIdx.x >> 6)] = su;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double pw = ((sh[0] + sh[1]) + sh[2]) + sh[3];
        const double pu = ((sh[4] + sh[5]) + sh[6]) + sh[7];
        __hip_atomic_store(partials + 2 * ch, pw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(partials + 2 * ch + 1, pu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        last = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    // wave w: segments w, w + 4, ..., US of them at a time; lane l: the segment's chunks l, l + 64, ... in index order.  A lane without
    // a chunk adds +0.0, which leaves the order of the sum unchanged.
    constexpr int US = 4;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nchunks = (int)gridDim.x;
    for (int s0 = wave; s0 < nseg; s0 += 4 * US) {
        double aw[US], au[US];
#pragma unroll
        for (int k = 0; k < US; ++k) {
            aw[k] = 0.0, au[k] = 0.0;
            const int s = s0 + 4 * k;
            if (s >= nseg) continue;
            const int c0 = segs[s].chunk0;
            const int c1 = s + 1 < nseg ? segs[s + 1].chunk0 : nchunks;
            for (int q = c0 + lane; q < c1; q += 64) {
                aw[k] += __hip_atomic_load(partials + 2 * q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                au[k] += __hip_atomic_load(partials + 2 * q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
#pragma unroll
        for (int k = 0; k < US; ++k) {
            const int s = s0 + 4 * k;
            if (s >= nseg) continue;          // (wave-uniform)
            const double tw = lamb_wave_sum(aw[k]), tu = lamb_wave_sum(au[k]);
            if (lane == 0) {
                const float nw = (float)sqrt(tw), nu = (float)sqrt(tu);
                float r = 1.0f;
                if (hp.g[segs[s].group].adapt) {
                    if (nw != nw || nu != nu) r = __builtin_nanf("");
                    else if (nw > 0.f && nu > 0.f) r = nw / nu;
                }
                ratio[s] = r;
                norm_w[s] = nw;
                norm_u[s] = nu;
            }
        }
    }
    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- launch 2: the update ---------------------------------------------------------------------------------------------------------------
// p -= (lr * ratio[segment]) * u, u formed again from the m, v launch 1 stored.  The counters are read here as in launch 1 (it does not
// move them); the block that finishes last advances every listed one, as optim_segments_kernel.
__global__ __launch_bounds__(256) void lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v,
                                                         const zsg_adam_seg* __restrict__ segs, int nseg, LambGroups hp,
                                                         const float* __restrict__ ratio, int* counters, int* ticket) {
    const int ch = blockIdx.x;
    const int si = lamb_segment_of(segs, nseg, ch);
    const zsg_adam_seg sg = segs[si];
    const int t = __hip_atomic_load(counters + sg.counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
    const LambCoef c = lamb_coef(hp.g[sg.group], t);
    const float step = hp.g[sg.group].lr * ratio[si];
    int64_t base;
    const int cnt = lamb_chunk_count(sg, ch, &base);
    const int n4 = cnt >> 2;
    float* pb = p + base;
    const float* mb = m + base;
    const float* vb = v + base;
    for (int i = threadIdx.x; i < n4; i += 256) {
        f32x4 pp = *(const f32x4*)(pb + 4 * i);
        const f32x4 mm = *(const f32x4*)(mb + 4 * i);
        const f32x4 vv = *(const f32x4*)(vb + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) pp[e] = pp[e] - step * lamb_u(mm[e], vv[e], pp[e], c);
        *(f32x4*)(pb + 4 * i) = pp;
    }
    if ((int)threadIdx.x < cnt - 4 * n4) {
        const int i = 4 * n4 + threadIdx.x;
        const float w = pb[i];
        pb[i] = w - step * lamb_u(mb[i], vb[i], w, c);
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

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
static int lamb_check_table(const char* what, const zsg_adam_seg* segs, int32_t nseg, int32_t nchunks, const zsg_lamb_group* groups,
                            int32_t ngroups, const int32_t* counters, const int32_t* ticket) {
    ZSG_REQUIRE(segs, "%s: null segs", what);
    ZSG_REQUIRE(groups, "%s: null groups", what);
    ZSG_REQUIRE(counters, "%s: null counters", what);
    ZSG_REQUIRE(ticket, "%s: null ticket", what);
    ZSG_REQUIRE(ngroups >= 1 && ngroups <= ZSG_ADAM_MAX_GROUPS, "%s: ngroups: %d parameter groups (1..%d supported)", what, ngroups,
                ZSG_ADAM_MAX_GROUPS);
    ZSG_REQUIRE(nseg >= 0 && nchunks >= nseg, "%s: nseg / nchunks: %d segments in %d chunks", what, nseg, nchunks);
    return 0;
}

extern "C" int zsg_lamb_moments(const float* p, const float* g, float* m, float* v, const zsg_adam_seg* segs, int32_t nseg, int32_t nchunks,
                                const zsg_lamb_group* groups, int32_t ngroups, float grad_scale, const int32_t* counters, double* partials,
                                int32_t* ticket, float* ratio, float* norm_w, float* norm_u, void* stream) {
    const char* what = "lamb_moments";
    ZSG_REQUIRE(p, "%s: null p", what);
    ZSG_REQUIRE(g, "%s: null g", what);
    ZSG_REQUIRE(m, "%s: null m", what);
    ZSG_REQUIRE(v, "%s: null v", what);
    if (int rc = lamb_check_table(what, segs, nseg, nchunks, groups, ngroups, counters, ticket)) return rc;
    ZSG_REQUIRE(partials, "%s: null partials", what);
    ZSG_REQUIRE(ratio && norm_w && norm_u, "%s: null ratio, norm_w or norm_u", what);
    ZSG_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "%s: p, g, m and v must be 16-byte aligned", what);
    ZSG_REQUIRE(((uintptr_t)partials & 7) == 0, "%s: partials must be 8-byte aligned", what);
    if (nseg == 0) return 0;          // nothing listed: no launch, nothing written
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("lamb_moments", st, 0, (double)nchunks * ZSG_ADAM_CHUNK * 24);      // (bytes: an upper bound)
    LambGroups hp = {};
    for (int i = 0; i < ngroups; ++i) hp.g[i] = groups[i];
    ZSG_LAUNCH(lamb_moments_kernel, dim3(nchunks), dim3(256), 0, st, p, g, m, v, segs, (int)nseg, hp, grad_scale, counters, partials, ticket,
               ratio, norm_w, norm_u);
    ZSG_CHECK_LAUNCH(what);
    return 0;
}

extern "C" int zsg_lamb_apply(float* p, const float* m, const float* v, const zsg_adam_seg* segs, int32_t nseg, int32_t nchunks,
                              const zsg_lamb_group* groups, int32_t ngroups, const float* ratio, int32_t* counters, int32_t* ticket,
                              void* stream) {
    const char* what = "lamb_apply";
    ZSG_REQUIRE(p, "%s: null p", what);
    ZSG_REQUIRE(m, "%s: null m", what);
    ZSG_REQUIRE(v, "%s: null v", what);
    if (int rc = lamb_check_table(what, segs, nseg, nchunks, groups, ngroups, counters, ticket)) return rc;
    ZSG_REQUIRE(ratio, "%s: null ratio", what);
    ZSG_REQUIRE((((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "%s: p, m and v must be 16-byte aligned", what);
    if (nseg == 0) return 0;          // nothing is stepped: no launch, no counter moves
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("lamb_apply", st, 0, (double)nchunks * ZSG_ADAM_CHUNK * 16);        // (bytes: an upper bound)
    LambGroups hp = {};
    for (int i = 0; i < ngroups; ++i) hp.g[i] = groups[i];
    ZSG_LAUNCH(lamb_apply_kernel, dim3(nchunks), dim3(256), 0, st, p, m, v, segs, (int)nseg, hp, ratio, counters, ticket);
    ZSG_CHECK_LAUNCH(what);
    return 0;
}
