// clip.hip — gradient-norm clipping over listed segments of the flat gradient buffer (torch.nn.utils.clip_grad_norm_, 2- and inf-norm).
// Two launches, no host round trip: zsg_grad_norm writes [total_norm, clip_coef] to device memory, zsg_grad_scale reads the coefficient
// from there.  Both address the buffer through zsg_adam_step_segments' segment table (one block per work chunk of <= ZSG_ADAM_CHUNK
// elements of one segment) and touch nothing outside the listed ranges.  HBM-bound: the norm reads 4 B per element, an engaged scale
// reads and writes it again.
#include "common.h"

// the segment of work chunk c: the last one whose chunk0 <= c (block-uniform binary search, as adam_segments_kernel)
__device__ __forceinline__ zsg_adam_seg clip_segment_of(const zsg_adam_seg* __restrict__ segs, int nseg, int c) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].chunk0 <= c) lo = mid;
        else hi = mid - 1;
    }
    return segs[lo];
}

// max that keeps a NaN (fmaxf drops it; torch's inf-norm propagates it)
__device__ __forceinline__ double nan_max(double a, double b) {
    return (b > a || b != b) ? b : a;
}

// Fixed-shape block reduction of one double per thread (256 threads): xor-shuffles inside each wave, then the 4 wave results in wave
// order.  The combination order depends on nothing but the thread index.
template <bool INF>
__device__ __forceinline__ double clip_block_reduce(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o, 64);
        v = INF ? nan_max(v, w) : v + w;
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = sh[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) r = INF ? nan_max(r, sh[k]) : r + sh[k];
    return r;
}

// One block per work chunk: the chunk's sum of squares (fp64) or max |g| becomes partials[chunk].  The block that finishes last reduces
// the partials in a fixed order (thread t takes chunks t, t + 256, ... in index order, then clip_block_reduce), so the result is the same
// bits whatever the arrival order.  Hand-off (cdna_hip_programming.md Guideline 16, counter form as bn_tail.h): each block stores its
// partial write-through (an agent-scope atomic store: sc1), drains it (s_waitcnt vmcnt(0)) before its ticket add, and the last arriver
// — told by the value its add returns — acquires at agent scope and reads the partials with sc1 loads.  No float atomics.
template <bool INF>
__global__ __launch_bounds__(256) void grad_norm_kernel(const float* __restrict__ g, const zsg_adam_seg* __restrict__ segs, int nseg,
                                                        float max_norm, double* partials, int* ticket, float* out) {
    __shared__ double sh[4];
    __shared__ int last;
    const int c = blockIdx.x;
    const zsg_adam_seg sg = clip_segment_of(segs, nseg, c);
    const int64_t start = (int64_t)(c - sg.chunk0) * ZSG_ADAM_CHUNK;
    const int64_t rem = sg.len - start;
    const int cnt = rem < ZSG_ADAM_CHUNK ? (int)rem : ZSG_ADAM_CHUNK;
    const int n4 = cnt >> 2;
    const float* gb = g + sg.off + start;
    double acc = 0.0;
#pragma unroll 4
    for (int i = threadIdx.x; i < n4; i += blockDim.x) {
        const f32x4 v = *(const f32x4*)(gb + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = INF ? nan_max(acc, (double)fabsf(v[e])) : acc + (double)v[e] * (double)v[e];
    }
    // tail of a segment whose length is not a multiple of 4 (its last chunk only)
    if ((int)threadIdx.x < cnt - 4 * n4) {
        const float x = gb[4 * n4 + threadIdx.x];
        acc = INF ? nan_max(acc, (double)fabsf(x)) : acc + (double)x * (double)x;
    }
    const double part = clip_block_reduce<INF>(acc, sh);
    if (threadIdx.x == 0) {
        __hip_atomic_store(partials + c, part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
    // thread t: partials t, t + 256, ... in index order, 8 loads in flight at a time (one at a time, each sc1 load's round trip was
    // exposed); a missing index adds +0.0 (or maxes 0 into norms >= 0), which leaves the order of the sum unchanged
    constexpr int UL = 8;
    double tot = 0.0;
    for (int k0 = threadIdx.x; k0 < (int)gridDim.x; k0 += UL * 256) {
        double p[UL];
#pragma unroll
        for (int u = 0; u < UL; ++u) {
            const int k = k0 + u * 256;
            p[u] = k < (int)gridDim.x ? __hip_atomic_load(partials + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < UL; ++u) tot = INF ? nan_max(tot, p[u]) : tot + p[u];
    }
    __syncthreads();          // (sh is reused)
    tot = clip_block_reduce<INF>(tot, sh);
    if (threadIdx.x == 0) {
        // torch: total_norm is fp32; clip_coef = clamp(max_norm / (total_norm + 1e-6), max=1.0), where a Python scalar divided by a
        // tensor is reciprocal(tensor) * scalar (Tensor.__rdiv__) and clamp keeps a NaN
        const float tn = INF ? (float)tot : (float)sqrt(tot);
        const float q = (1.0f / (tn + 1e-6f)) * max_norm;
        out[0] = tn;
        out[1] = q > 1.0f ? 1.0f : q;
        __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// g *= coef over the listed segments; every block reads the coefficient first and leaves memory alone when it is 1 (g * 1.0f == g:
// bit-identical to torch's unconditional _foreach_mul_, and the unclipped step costs one read of 4 bytes per block).
__global__ __launch_bounds__(256) void grad_scale_kernel(float* __restrict__ g, const zsg_adam_seg* __restrict__ segs, int nseg,
                                                         const float* __restrict__ coef) {
    const float s = *coef;
    if (s == 1.0f) return;
    const int c = blockIdx.x;
    const zsg_adam_seg sg = clip_segment_of(segs, nseg, c);
    const int64_t start = (int64_t)(c - sg.chunk0) * ZSG_ADAM_CHUNK;
    const int64_t rem = sg.len - start;
    const int cnt = rem < ZSG_ADAM_CHUNK ? (int)rem : ZSG_ADAM_CHUNK;
    const int n4 = cnt >> 2;
    float* gb = g + sg.off + start;
    // four loads in flight before the first store (the compiler does not hoist a load above a store to the same buffer)
    constexpr int U = 4;
    int i = threadIdx.x;
    for (; i + (U - 1) * 256 < n4; i += U * 256) {
        f32x4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = *(const f32x4*)(gb + 4 * (i + u * 256));
#pragma unroll
        for (int u = 0; u < U; ++u) *(f32x4*)(gb + 4 * (i + u * 256)) = v[u] * s;
    }
    for (; i < n4; i += 256) *(f32x4*)(gb + 4 * i) = *(const f32x4*)(gb + 4 * i) * s;
    if ((int)threadIdx.x < cnt - 4 * n4) gb[4 * n4 + threadIdx.x] *= s;
}

extern "C" int zsg_grad_norm(const float* g, const zsg_adam_seg* segs, int32_t nseg, int32_t nchunks, int32_t inf_norm, float max_norm,
                             double* partials, int32_t* ticket, float* out, void* stream) {
    ZSG_REQUIRE(g && segs && partials && ticket && out, "grad_norm: null pointer");
    ZSG_REQUIRE(nseg >= 0 && nchunks >= nseg, "grad_norm: %d segments in %d chunks", nseg, nchunks);
    ZSG_REQUIRE(((uintptr_t)g & 15) == 0 && ((uintptr_t)partials & 7) == 0, "grad_norm: misaligned buffer");
    if (nseg == 0) return 0;          // nothing listed: no launch, out is not written
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("grad_norm", st, 0, (double)nchunks * ZSG_ADAM_CHUNK * 4);      // (bytes: an upper bound)
    if (inf_norm)
        ZSG_LAUNCH(grad_norm_kernel<true>, dim3(nchunks), dim3(256), 0, st, g, segs, (int)nseg, max_norm, partials, ticket, out);
    else
        ZSG_LAUNCH(grad_norm_kernel<false>, dim3(nchunks), dim3(256), 0, st, g, segs, (int)nseg, max_norm, partials, ticket, out);
    ZSG_CHECK_LAUNCH("grad_norm");
    return 0;
}

extern "C" int zsg_grad_scale(float* g, const zsg_adam_seg* segs, int32_t nseg, int32_t nchunks, const float* coef, void* stream) {
    ZSG_REQUIRE(g && segs && coef, "grad_scale: null pointer");
    ZSG_REQUIRE(nseg >= 0 && nchunks >= nseg, "grad_scale: %d segments in %d chunks", nseg, nchunks);
    ZSG_REQUIRE(((uintptr_t)g & 15) == 0, "grad_scale: the gradient buffer must be 16-byte aligned");
    if (nseg == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("grad_scale", st, 0, (double)nchunks * ZSG_ADAM_CHUNK * 8);     // (bytes: an upper bound, when it engages)
    ZSG_LAUNCH(grad_scale_kernel, dim3(nchunks), dim3(256), 0, st, g, segs, (int)nseg, coef);
    ZSG_CHECK_LAUNCH("grad_scale");
    return 0;
}
