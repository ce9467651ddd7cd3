// optim.hip — the fused optimizer steps beside adam.hip's: Adam with amsgrad, AdamW (with and without amsgrad) and SGD with (Nesterov)
// momentum over one flat fp32 parameter buffer, each following torch's single-tensor implementation (torch/optim/adam.py, adamw.py,
// sgd.py).  HBM-bound streaming kernels in adam.hip's three launch shapes — the whole buffer, the whole buffer with the weight average
// riding (ema.h's rule on the p about to be stored), listed segments with per-group hyperparameters and per-segment counters — and with
// its counter schemes.  Bytes per parameter (p and g read, p written, every state buffer read and written; + 8 with the average):
//     Adam / AdamW 28,  with amsgrad 36,  SGD with momentum 20,  plain SGD 12.
// The arithmetic of a rule is written ONCE (optim_rule) and the loop over a span once (optim_span); the kernels only place spans.
//
// This file is compiled with -ffp-contract=off (Makefile): every fused multiply-add below is an explicit fmaf.  The Adam rule spells out
// the contractions adam.hip's kernels compile to, so rule Adam here and zsg_adam_step give the same bits: in the 16-byte body g += wd * p
// and both moments are fused, in the < 4 element tail they round product by product (there the compiler packs the two products of a
// moment into one v_pk_mul_f32 and adds: profiles/optim_text_identity.txt) — optim_rule's FUSE.  AdamW's decay p *= 1 - lr * wd stays a
// product of its own (fused into the update it would round differently, and AdamW at wd = 0 would leave Adam's bits).
#include "common.h"
#include "ema.h"

// What a rule needs of one hyperparameter set at step t (uniform over a block).
struct OptCoef {
    float wd;
    float b1, b2, omb1, omb2, eps, neg_step, bc2s, decay;          // Adam / AdamW
    float neg_lr, mom, omd;                                        // SGD
    bool first, nesterov;
};

template <int ALG>
__device__ __forceinline__ OptCoef optim_coef(const zsg_optim_group& h, int t) {
    OptCoef c = {};
    c.wd = h.weight_decay;
    if (ALG == ZSG_OPT_SGD) {
        c.neg_lr = -h.lr;
        c.mom = h.momentum;
        c.omd = 1.f - h.dampening;
        c.first = t == 1;          // the parameter's first step: buf = g (torch creates the buffer as a clone of the gradient)
        c.nesterov = h.nesterov != 0;
    } else {
        c.b1 = h.beta1;
        c.b2 = h.beta2;
        c.omb1 = 1.f - h.beta1;
        c.omb2 = 1.f - h.beta2;
        c.eps = h.eps;
        c.neg_step = -(h.lr / (1.f - powf(h.beta1, (float)t)));
        c.bc2s = sqrtf(1.f - powf(h.beta2, (float)t));
        c.decay = 1.f - h.lr * h.weight_decay;
    }
    return c;
}

template <bool FUSE>
__device__ __forceinline__ float mul_add(float a, float b, float c) {
    return FUSE ? fmaf(a, b, c) : a * b + c;
}

// One element.  X: amsgrad (Adam / AdamW), a momentum buffer exists (SGD).  State: s0 = m, s1 = v, s2 = vmax | s0 = the momentum buffer.
// FUSE: the Adam family's g += wd * p and moments as the body (true) or the tail (false) of adam_kernel rounds them.
template <int ALG, bool X, bool FUSE>
__device__ __forceinline__ void optim_rule(float& p, float g, float& s0, float& s1, float& s2, const OptCoef& c) {
    if (ALG == ZSG_OPT_SGD) {
        if (c.wd != 0.f) g = fmaf(c.wd, p, g);
        float d = g;
        if (X && c.mom != 0.f) {          // (a group without momentum beside one with it: its part of the buffer is not touched)
            s0 = c.first ? g : fmaf(c.omd, g, s0 * c.mom);
            d = c.nesterov ? fmaf(c.mom, s0, g) : s0;
        }
        p = fmaf(c.neg_lr, d, p);
    } else {
        if (c.wd != 0.f) {
            if (ALG == ZSG_OPT_ADAMW) p = p * c.decay;
            else g = mul_add<FUSE>(c.wd, p, g);
        }
        s0 = mul_add<FUSE>(c.b1, s0, c.omb1 * g);
        s1 = mul_add<FUSE>(c.b2, s1, c.omb2 * (g * g));
        float den = s1;
        if (X) {
            s2 = (s1 > s2 || s1 != s1) ? s1 : s2;          // torch.maximum: a NaN propagates
            den = s2;
        }
        p = fmaf(c.neg_step, s0 / (sqrtf(den) / c.bc2s + c.eps), p);
    }
}

template <int ALG, bool X>
struct OptState {
    static constexpr int N = ALG == ZSG_OPT_SGD ? (X ? 1 : 0) : (X ? 3 : 2);          // state buffers of the rule
};

// The 16-byte groups i0, i0 + stride, ... < n4 of the span at p / g / s0..2 / ema, and its `tail` < 4 last elements (behind 4 * n4) on the
// first threads of the block (tail = 0: another block has them).  A momentum-free group of an SGD launch that has a buffer skips it.
template <int ALG, bool X, bool EMA>
__device__ __forceinline__ void optim_span(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s0, float* __restrict__ s1,
                                           float* __restrict__ s2, float* __restrict__ ema, int64_t i0, int64_t stride, int64_t n4, int tail,
                                           const OptCoef& c, float gs, float ema_w) {
    constexpr int NS = OptState<ALG, X>::N;
    const bool use0 = NS >= 1 && (ALG != ZSG_OPT_SGD || c.mom != 0.f);
    for (int64_t i = i0; i < n4; i += stride) {
        f32x4 pp = *(const f32x4*)(p + 4 * i);
        const f32x4 gg = *(const f32x4*)(g + 4 * i) * gs;
        f32x4 a = {}, b = {}, d = {};
        if (use0) a = *(const f32x4*)(s0 + 4 * i);
        if (NS >= 2) b = *(const f32x4*)(s1 + 4 * i);
        if (NS >= 3) d = *(const f32x4*)(s2 + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = pp[e], ae = a[e], be = b[e], de = d[e];
            optim_rule<ALG, X, true>(pe, gg[e], ae, be, de, c);
            pp[e] = pe, a[e] = ae, b[e] = be, d[e] = de;
        }
        *(f32x4*)(p + 4 * i) = pp;
        if (use0) *(f32x4*)(s0 + 4 * i) = a;
        if (NS >= 2) *(f32x4*)(s1 + 4 * i) = b;
        if (NS >= 3) *(f32x4*)(s2 + 4 * i) = d;
        if (EMA) {
            f32x4 ee = *(const f32x4*)(ema + 4 * i);
#pragma unroll
            for (int e = 0; e < 4; ++e) ee[e] = zsg_ema_rule(ee[e], pp[e], ema_w);
            *(f32x4*)(ema + 4 * i) = ee;
        }
    }
    if ((int)threadIdx.x < tail) {
        const int64_t i = 4 * n4 + threadIdx.x;
        float pp = p[i], a = 0.f, b = 0.f, d = 0.f;
        if (use0) a = s0[i];
        if (NS >= 2) b = s1[i];
        if (NS >= 3) d = s2[i];
        optim_rule<ALG, X, false>(pp, g[i] * gs, a, b, d, c);
        p[i] = pp;
        if (use0) s0[i] = a;
        if (NS >= 2) s1[i] = b;
        if (NS >= 3) s2[i] = d;
        if (EMA) ema[i] = zsg_ema_rule(ema[i], pp, ema_w);
    }
}

// ---- the whole flat buffer in one launch ------------------------------------------------------------------------------------------------
// step[0] = steps taken, step[1] = the completion ticket: adam_kernel's scheme (adam.hip) — every block computes with t = step[0] + 1, the
// block that finishes last publishes t and clears the ticket.
template <int ALG, bool X, bool EMA>
__global__ __launch_bounds__(256) void optim_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s0,
                                                    float* __restrict__ s1, float* __restrict__ s2, int64_t n4, int64_t n, zsg_optim_group h,
                                                    float gs, int* step, float* __restrict__ ema, float ema_w) {
    const int t = __hip_atomic_load(step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
    const OptCoef c = optim_coef<ALG>(h, t);
    optim_span<ALG, X, EMA>(p, g, s0, s1, s2, ema, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x, n4,
                            blockIdx.x == 0 ? (int)(n - 4 * n4) : 0, c, gs, ema_w);
    __syncthreads();
    if (threadIdx.x == 0 && __hip_atomic_fetch_add(step + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1) {
        __hip_atomic_store(step + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(step, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- listed segments ----------------------------------------------------------------------------------------------------------------------
// adam_segments_kernel's shape (adam.hip): one block per work chunk of <= ZSG_ADAM_CHUNK elements of one segment, the segment's group and
// its own counter (t == 1 is the segment's first step, whenever it joins); the block that finishes last advances every listed counter.
struct OptGroups {
    zsg_optim_group g[ZSG_ADAM_MAX_GROUPS];
};

template <int ALG, bool X>
__global__ __launch_bounds__(256) void optim_segments_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s0,
                                                             float* __restrict__ s1, float* __restrict__ s2,
                                                             const zsg_adam_seg* __restrict__ segs, int nseg, OptGroups hp, float gs,
                                                             int* counters, int* ticket) {
    // the segment of this chunk: the last one whose chunk0 <= blockIdx.x (block-uniform binary search)
    const int ch = blockIdx.x;
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].chunk0 <= ch) lo = mid;
        else hi = mid - 1;
    }
    const zsg_adam_seg sg = segs[lo];
    const int t = __hip_atomic_load(counters + sg.counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
    const OptCoef c = optim_coef<ALG>(hp.g[sg.group], t);
    const int64_t start = (int64_t)(ch - sg.chunk0) * ZSG_ADAM_CHUNK;
    const int64_t rem = sg.len - start;
    const int cnt = rem < ZSG_ADAM_CHUNK ? (int)rem : ZSG_ADAM_CHUNK;
    const int64_t base = sg.off + start;
    constexpr int NS = OptState<ALG, X>::N;
    optim_span<ALG, X, false>(p + base, g + base, NS >= 1 ? s0 + base : nullptr, NS >= 2 ? s1 + base : nullptr, NS >= 3 ? s2 + base : nullptr,
                              nullptr, threadIdx.x, blockDim.x, cnt >> 2, cnt & 3, c, gs, 0.f);
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
// The checks every entry point makes on the rule, the hyperparameter sets and the buffers the rule needs.  *x = the kernels' X.
static int optim_check(const char* what, int32_t algo, int32_t flags, const float* p, const float* g, const float* s0, const float* s1,
                       const float* s2, const zsg_optim_group* groups, int32_t ngroups, bool* x) {
    ZSG_REQUIRE(algo == ZSG_OPT_ADAM || algo == ZSG_OPT_ADAMW || algo == ZSG_OPT_SGD, "%s: unknown algorithm %d (ZSG_OPT_ADAM, _ADAMW, _SGD)", what,
                algo);
    ZSG_REQUIRE((flags & ~ZSG_OPT_AMSGRAD) == 0, "%s: unknown flags 0x%x", what, flags);
    ZSG_REQUIRE(!(flags & ZSG_OPT_AMSGRAD) || algo != ZSG_OPT_SGD, "%s: flags: amsgrad is not a property of SGD", what);
    ZSG_REQUIRE(p && g, "%s: null p or g", what);
    ZSG_REQUIRE(groups, "%s: null hyperparameters", what);
    ZSG_REQUIRE(ngroups >= 1 && ngroups <= ZSG_ADAM_MAX_GROUPS, "%s: %d parameter groups (1..%d supported)", what, ngroups, ZSG_ADAM_MAX_GROUPS);
    uintptr_t bits = (uintptr_t)p | (uintptr_t)g;
    if (algo == ZSG_OPT_SGD) {
        bool mom = false;
        for (int i = 0; i < ngroups; ++i) {
            const zsg_optim_group& h = groups[i];
            ZSG_REQUIRE(!h.nesterov || (h.momentum > 0.f && h.dampening == 0.f), "%s: nesterov momentum requires a momentum and zero dampening", what);
            mom = mom || h.momentum != 0.f;
        }
        ZSG_REQUIRE(!mom || s0, "%s: null momentum buffer (s0) with momentum != 0", what);
        *x = mom;
        if (mom) bits |= (uintptr_t)s0;
    } else {
        ZSG_REQUIRE(s0 && s1, "%s: null m (s0) or v (s1)", what);
        *x = (flags & ZSG_OPT_AMSGRAD) != 0;
        ZSG_REQUIRE(!*x || s2, "%s: null vmax (s2) with amsgrad", what);
        bits |= (uintptr_t)s0 | (uintptr_t)s1 | (*x ? (uintptr_t)s2 : 0);
    }
    ZSG_REQUIRE((bits & 15) == 0, "%s: buffers must be 16-byte aligned", what);
    return 0;
}

static double optim_bytes(int32_t algo, bool x, bool ema) {
    return (algo == ZSG_OPT_SGD ? (x ? 20 : 12) : (x ? 36 : 28)) + (ema ? 8 : 0);
}

template <int ALG, bool X>
static void optim_launch_flat(int blocks, hipStream_t st, float* p, const float* g, float* s0, float* s1, float* s2, int64_t n,
                              const zsg_optim_group& h, float gs, int32_t* step, float* ema, float ema_w) {
    const auto kern = ema ? optim_kernel<ALG, X, true> : optim_kernel<ALG, X, false>;
    ZSG_LAUNCH(kern, dim3(blocks), dim3(256), 0, st, p, g, s0, s1, s2, n / 4, n, h, gs, step, ema, ema_w);
}

static int optim_flat(const char* what, int32_t algo, int32_t flags, float* p, const float* g, float* s0, float* s1, float* s2, int64_t n,
                      const zsg_optim_group* hp, float gs, int32_t* step, float* ema, float ema_w, void* stream) {
    bool x = false;
    if (int rc = optim_check(what, algo, flags, p, g, s0, s1, s2, hp, 1, &x)) return rc;
    ZSG_REQUIRE(step, "%s: null step_count", what);
    ZSG_REQUIRE(n > 0, "%s: n = %lld", what, (long long)n);
    hipStream_t st = (hipStream_t)stream;
    static const char* const names[2][3] = {{"optim_adam_step", "optim_adamw_step", "optim_sgd_step"},
                                            {"optim_adam_step_ema", "optim_adamw_step_ema", "optim_sgd_step_ema"}};
    ZSG_PROF(names[ema ? 1 : 0][algo], st, 0, (double)n * optim_bytes(algo, x, ema != nullptr));
    int64_t blocks = (n / 4 + 255) / 256;          // the grid of adam_launch
    if (blocks > ZSG_NUM_CU * 8) blocks = ZSG_NUM_CU * 8;
    if (blocks < 1) blocks = 1;
    const int b = (int)blocks;
    if (algo == ZSG_OPT_ADAM) {
        if (x) optim_launch_flat<ZSG_OPT_ADAM, true>(b, st, p, g, s0, s1, s2, n, *hp, gs, step, ema, ema_w);
        else optim_launch_flat<ZSG_OPT_ADAM, false>(b, st, p, g, s0, s1, s2, n, *hp, gs, step, ema, ema_w);
    } else if (algo == ZSG_OPT_ADAMW) {
        if (x) optim_launch_flat<ZSG_OPT_ADAMW, true>(b, st, p, g, s0, s1, s2, n, *hp, gs, step, ema, ema_w);
        else optim_launch_flat<ZSG_OPT_ADAMW, false>(b, st, p, g, s0, s1, s2, n, *hp, gs, step, ema, ema_w);
    } else {
        if (x) optim_launch_flat<ZSG_OPT_SGD, true>(b, st, p, g, s0, s1, s2, n, *hp, gs, step, ema, ema_w);
        else optim_launch_flat<ZSG_OPT_SGD, false>(b, st, p, g, s0, s1, s2, n, *hp, gs, step, ema, ema_w);
    }
    ZSG_CHECK_LAUNCH(what);
    return 0;
}

extern "C" int zsg_optim_step(int32_t algo, int32_t flags, float* p, const float* g, float* s0, float* s1, float* s2, int64_t n,
                              const zsg_optim_group* hp, float grad_scale, int32_t* step_count, void* stream) {
    return optim_flat("optim_step", algo, flags, p, g, s0, s1, s2, n, hp, grad_scale, step_count, nullptr, 0.f, stream);
}

extern "C" int zsg_optim_step_ema(int32_t algo, int32_t flags, float* p, const float* g, float* s0, float* s1, float* s2, int64_t n,
                                  const zsg_optim_group* hp, float grad_scale, int32_t* step_count, float* ema, float ema_w, void* stream) {
    ZSG_REQUIRE(ema, "optim_step_ema: null average buffer (ema)");
    ZSG_REQUIRE(ema_w >= 0.f && ema_w <= 1.f, "optim_step_ema: ema_w %g outside [0, 1]", (double)ema_w);
    ZSG_REQUIRE(((uintptr_t)ema & 15) == 0, "optim_step_ema: buffers must be 16-byte aligned (ema)");
    return optim_flat("optim_step_ema", algo, flags, p, g, s0, s1, s2, n, hp, grad_scale, step_count, ema, ema_w, stream);
}

template <int ALG, bool X>
static void optim_launch_segments(int nchunks, hipStream_t st, float* p, const float* g, float* s0, float* s1, float* s2, const zsg_adam_seg* segs,
                                  int nseg, const OptGroups& hp, float gs, int32_t* counters, int32_t* ticket) {
    const auto kern = optim_segments_kernel<ALG, X>;
    ZSG_LAUNCH(kern, dim3(nchunks), dim3(256), 0, st, p, g, s0, s1, s2, segs, nseg, hp, gs, counters, ticket);
}

extern "C" int zsg_optim_step_segments(int32_t algo, int32_t flags, float* p, const float* g, float* s0, float* s1, float* s2,
                                       const zsg_adam_seg* segs, int32_t nseg, int32_t nchunks, const zsg_optim_group* groups, int32_t ngroups,
                                       float grad_scale, int32_t* counters, int32_t* ticket, void* stream) {
    const char* what = "optim_step_segments";
    bool x = false;
    if (int rc = optim_check(what, algo, flags, p, g, s0, s1, s2, groups, ngroups, &x)) return rc;
    ZSG_REQUIRE(segs && counters && ticket, "%s: null segs, counters or ticket", what);
    ZSG_REQUIRE(nseg >= 0 && nchunks >= nseg, "%s: %d segments in %d chunks", what, nseg, nchunks);
    if (nseg == 0) return 0;          // nothing is stepped: no launch, no counter moves
    hipStream_t st = (hipStream_t)stream;
    static const char* const names[3] = {"optim_adam_step_segments", "optim_adamw_step_segments", "optim_sgd_step_segments"};
    ZSG_PROF(names[algo], st, 0, (double)nchunks * ZSG_ADAM_CHUNK * optim_bytes(algo, x, false));      // (bytes: an upper bound)
    OptGroups hp = {};
    for (int i = 0; i < ngroups; ++i) hp.g[i] = groups[i];
    if (algo == ZSG_OPT_ADAM) {
        if (x) optim_launch_segments<ZSG_OPT_ADAM, true>(nchunks, st, p, g, s0, s1, s2, segs, nseg, hp, grad_scale, counters, ticket);
        else optim_launch_segments<ZSG_OPT_ADAM, false>(nchunks, st, p, g, s0, s1, s2, segs, nseg, hp, grad_scale, counters, ticket);
    } else if (algo == ZSG_OPT_ADAMW) {
        if (x) optim_launch_segments<ZSG_OPT_ADAMW, true>(nchunks, st, p, g, s0, s1, s2, segs, nseg, hp, grad_scale, counters, ticket);
        else optim_launch_segments<ZSG_OPT_ADAMW, false>(nchunks, st, p, g, s0, s1, s2, segs, nseg, hp, grad_scale, counters, ticket);
    } else {
        if (x) optim_launch_segments<ZSG_OPT_SGD, true>(nchunks, st, p, g, s0, s1, s2, segs, nseg, hp, grad_scale, counters, ticket);
        else optim_launch_segments<ZSG_OPT_SGD, false>(nchunks, st, p, g, s0, s1, s2, segs, nseg, hp, grad_scale, counters, ticket);
    }
    ZSG_CHECK_LAUNCH(what);
    return 0;
}
