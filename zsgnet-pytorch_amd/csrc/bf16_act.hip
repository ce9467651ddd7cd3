// bf16_act.hip — the element-wise kernels of an eval plan whose activations are STORED as bf16 (eval_dtype = "bf16_act"), NHWC, gfx950.
//
// The contract (include/zsg.h): a value is rounded exactly once, where it is stored (round-to-nearest-even, bf16.h: the conversion the
// weight packer and the convolution's operand loader use); all arithmetic is fp32 on the widened inputs, in the order of the fp32 kernel
// of the same name in misc.hip, so a result equals that kernel's on the widened inputs, rounded.  Layouts, element offsets and leading
// dimensions are the fp32 kernels'; an element is a uint16.
// All of them are a load and a store per element: a lane moves 8 channels (16 bytes of bf16) where the channel count is a multiple of 8
// and 4 channels (8 bytes) otherwise.  No kernel here has been timed on its own: they are a few microseconds of an eval forward
// (profiles/bf16act_eval_time.txt has the per-kernel times of one forward).
#include "bf16.h"

ZSG_DEFINE_PRIO_FLAG()

static inline int grid_for(int64_t n_items, int block = 256, int cap = ZSG_NUM_CU * 16) {
    int64_t b = (n_items + block - 1) / block;
    if (b < 1) b = 1;
    return (int)(b > cap ? cap : b);
}

// V channels (4 or 8) of a bf16 row, widened / rounded
template <int V>
struct Grp {
    f32x4 v[V / 4];
};
template <int V>
__device__ __forceinline__ Grp<V> load16(const uint16_t* p) {
    Grp<V> g;
    if constexpr (V == 8) {
        const u32x4 h = *(const u32x4*)p;
        g.v[0] = bf16_widen4(u32x2{h[0], h[1]});
        g.v[1] = bf16_widen4(u32x2{h[2], h[3]});
    } else {
        g.v[0] = bf16_widen4(*(const u32x2*)p);
    }
    return g;
}
template <int V>
__device__ __forceinline__ Grp<V> load32(const float* p) {
    Grp<V> g;
#pragma unroll
    for (int k = 0; k < V / 4; ++k) g.v[k] = *(const f32x4*)(p + 4 * k);
    return g;
}
template <int V>
__device__ __forceinline__ void store16(uint16_t* p, const Grp<V>& g) {
    if constexpr (V == 8) {
        const u32x2 a = bf16_pack4(g.v[0]), b = bf16_pack4(g.v[1]);
        *(u32x4*)p = u32x4{a[0], a[1], b[0], b[1]};
    } else {
        *(u32x2*)p = bf16_pack4(g.v[0]);
    }
}

// ---- max pool (no index output: an eval plan has no backward) ----------------------------------------------------------------
template <int V, bool X16>
__global__ void maxpool_fwd_bf16_kernel(const void* __restrict__ x, int B, int H, int W, int CV, int k, int s, int p, int Ho, int Wo,
                                        uint16_t* __restrict__ out) {
    ZSG_SET_MAIN_PRIO();
    const int64_t total = (int64_t)B * Ho * Wo * CV;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int cv = (int)(i % CV);
        int64_t t = i / CV;
        const int wo = (int)(t % Wo);
        t /= Wo;
        const int ho = (int)(t % Ho);
        const int b = (int)(t / Ho);
        Grp<V> best;
#pragma unroll
        for (int e = 0; e < V; ++e) best.v[e / 4][e % 4] = -INFINITY;
        for (int r = 0; r < k; ++r) {
            const int hi = ho * s - p + r;
            if ((unsigned)hi >= (unsigned)H) continue;
            for (int q = 0; q < k; ++q) {
                const int wi = wo * s - p + q;
                if ((unsigned)wi >= (unsigned)W) continue;
                const int64_t o = ((((int64_t)b * H + hi) * W + wi) * CV + cv) * V;
                Grp<V> v;
                if constexpr (X16) v = load16<V>((const uint16_t*)x + o);
                else v = load32<V>((const float*)x + o);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const float u = v.v[e / 4][e % 4];
                    if (u > best.v[e / 4][e % 4] || u != u) best.v[e / 4][e % 4] = u;      // NaN propagates (torch rule), as maxpool_fwd_kernel
                }
            }
        }
        store16<V>(out + i * V, best);
    }
}

extern "C" int zsg_maxpool_fwd_bf16(const void* x, int32_t x_bf16, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k, int32_t s, int32_t p,
                                    int32_t Ho, int32_t Wo, uint16_t* out, void* stream) {
    ZSG_REQUIRE(x && out && C > 0 && (C % 4) == 0 && k > 0 && k <= 15 && s > 0 && B > 0 && Ho > 0 && Wo > 0, "maxpool_fwd_bf16: bad argument");
    const bool v8 = (C % 8) == 0;
    ZSG_REQUIRE((((uintptr_t)x | (uintptr_t)out) & (v8 ? 15 : 7)) == 0 && (x_bf16 || ((uintptr_t)x & 15) == 0), "maxpool_fwd_bf16: alignment");
    const int V = v8 ? 8 : 4;
    const int64_t n = (int64_t)B * Ho * Wo * (C / V);
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("maxpool_fwd_bf16", st, 0, (double)B * H * W * C * (x_bf16 ? 2 : 4) + (double)B * Ho * Wo * C * 2);
    const dim3 g(grid_for(n)), blk(256);
    if (v8 && x_bf16) ZSG_LAUNCH((maxpool_fwd_bf16_kernel<8, true>), g, blk, 0, st, x, B, H, W, C / 8, k, s, p, Ho, Wo, out);
    else if (v8) ZSG_LAUNCH((maxpool_fwd_bf16_kernel<8, false>), g, blk, 0, st, x, B, H, W, C / 8, k, s, p, Ho, Wo, out);
    else if (x_bf16) ZSG_LAUNCH((maxpool_fwd_bf16_kernel<4, true>), g, blk, 0, st, x, B, H, W, C / 4, k, s, p, Ho, Wo, out);
    else ZSG_LAUNCH((maxpool_fwd_bf16_kernel<4, false>), g, blk, 0, st, x, B, H, W, C / 4, k, s, p, Ho, Wo, out);
    ZSG_CHECK_LAUNCH("maxpool_fwd_bf16");
    return 0;
}

// ---- nearest upsample + add (the index rule of upsample_add_fwd_kernel) --------------------------------------------------------
__device__ __forceinline__ int nearest_src(int dst, float scale, int in_size) {
    const int s = (int)floorf((float)dst * scale);
    return s < in_size - 1 ? s : in_size - 1;
}

template <int V>
__global__ void upsample_add_fwd_bf16_kernel(const uint16_t* __restrict__ a, const uint16_t* __restrict__ p, int B, int Hs, int Ws, int Hd, int Wd,
                                             int CV, float sh, float sw, uint16_t* __restrict__ out) {
    ZSG_SET_MAIN_PRIO();
    const int64_t total = (int64_t)B * Hd * Wd * CV;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int cv = (int)(i % CV);
        int64_t t = i / CV;
        const int x = (int)(t % Wd);
        t /= Wd;
        const int y = (int)(t % Hd);
        const int b = (int)(t / Hd);
        const int ys = nearest_src(y, sh, Hs), xs = nearest_src(x, sw, Ws);
        const Grp<V> u = load16<V>(p + ((((int64_t)b * Hs + ys) * Ws + xs) * CV + cv) * V);
        Grp<V> r = load16<V>(a + i * V);
#pragma unroll
        for (int k = 0; k < V / 4; ++k) r.v[k] = r.v[k] + u.v[k];
        store16<V>(out + i * V, r);
    }
}

extern "C" int zsg_upsample_add_fwd_bf16(const uint16_t* a, const uint16_t* p, int32_t B, int32_t Hs, int32_t Ws, int32_t Hd, int32_t Wd, int32_t C,
                                         uint16_t* out, void* stream) {
    ZSG_REQUIRE(a && p && out && C > 0 && (C % 4) == 0 && B > 0 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0, "upsample_add_fwd_bf16: bad argument");
    const bool v8 = (C % 8) == 0;
    ZSG_REQUIRE((((uintptr_t)a | (uintptr_t)p | (uintptr_t)out) & (v8 ? 15 : 7)) == 0, "upsample_add_fwd_bf16: alignment");
    const int V = v8 ? 8 : 4;
    const int64_t n = (int64_t)B * Hd * Wd * (C / V);
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("upsample_add_fwd_bf16", st, 0, (double)B * Hd * Wd * C * 2 * 2.25);
    const float sh = (float)Hs / (float)Hd, sw = (float)Ws / (float)Wd;
    if (v8) ZSG_LAUNCH((upsample_add_fwd_bf16_kernel<8>), dim3(grid_for(n)), dim3(256), 0, st, a, p, B, Hs, Ws, Hd, Wd, C / 8, sh, sw, out);
    else ZSG_LAUNCH((upsample_add_fwd_bf16_kernel<4>), dim3(grid_for(n)), dim3(256), 0, st, a, p, B, Hs, Ws, Hd, Wd, C / 4, sh, sw, out);
    ZSG_CHECK_LAUNCH("upsample_add_fwd_bf16");
    return 0;
}

// ---- relu (fmaxf(x, 0), as relu_fwd_kernel) -----------------------------------------------------------------------------------
template <int V>
__global__ void relu_fwd_bf16_kernel(const uint16_t* __restrict__ x, int64_t nv, uint16_t* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
        Grp<V> g = load16<V>(x + i * V);
#pragma unroll
        for (int e = 0; e < V; ++e) g.v[e / 4][e % 4] = fmaxf(g.v[e / 4][e % 4], 0.f);
        store16<V>(out + i * V, g);
    }
}
extern "C" int zsg_relu_fwd_bf16(const uint16_t* x, int64_t n, uint16_t* out, void* stream) {
    ZSG_REQUIRE(x && out && n >= 0 && (n % 4) == 0, "relu_fwd_bf16: bad argument");
    const bool v8 = (n % 8) == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
    ZSG_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 7) == 0, "relu_fwd_bf16: alignment");
    if (v8) ZSG_LAUNCH((relu_fwd_bf16_kernel<8>), dim3(grid_for(n / 8)), dim3(256), 0, (hipStream_t)stream, x, n / 8, out);
    else ZSG_LAUNCH((relu_fwd_bf16_kernel<4>), dim3(grid_for(n / 4)), dim3(256), 0, (hipStream_t)stream, x, n / 4, out);
    ZSG_CHECK_LAUNCH("relu_fwd_bf16");
    return 0;
}

// ---- adaptive average pool to 1x1 (the pixel-ascending fp32 sum of avgpool_fwd_kernel) -----------------------------------------
__global__ void avgpool_fwd_bf16_kernel(const uint16_t* __restrict__ x, int B, int HW, int C, uint16_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * C) return;
    const int b = i / C, c = i % C;
    float s = 0.f;
    for (int k = 0; k < HW; ++k) s += bf16_widen1(x[((int64_t)b * HW + k) * C + c]);
    out[i] = bf16_round1(s / (float)HW);
}
extern "C" int zsg_avgpool_fwd_bf16(const uint16_t* x, int32_t B, int32_t HW, int32_t C, uint16_t* out, void* stream) {
    ZSG_REQUIRE(x && out && B > 0 && HW > 0 && C > 0 && (int64_t)B * C < (1ll << 31), "avgpool_fwd_bf16: bad argument");
    ZSG_LAUNCH(avgpool_fwd_bf16_kernel, dim3(cdiv((int64_t)B * C, 256)), dim3(256), 0, (hipStream_t)stream, x, B, HW, C, out);
    ZSG_CHECK_LAUNCH("avgpool_fwd_bf16");
    return 0;
}

// ---- casts -----------------------------------------------------------------------------------------------------------------------
// 4 elements per lane where the pointers allow, the rest (and any tail) one by one
__global__ void cast_f32_bf16_kernel(const float* __restrict__ x, int64_t n, int vec, uint16_t* __restrict__ out) {
    const int64_t n4 = vec ? n / 4 : 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = i0; i < n4; i += stride) *(u32x2*)(out + i * 4) = bf16_pack4(*(const f32x4*)(x + i * 4));
    for (int64_t i = n4 * 4 + i0; i < n; i += stride) out[i] = bf16_round1(x[i]);
}
__global__ void cast_bf16_f32_kernel(const uint16_t* __restrict__ x, int64_t n, int vec, float* __restrict__ out) {
    const int64_t n4 = vec ? n / 4 : 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = i0; i < n4; i += stride) *(f32x4*)(out + i * 4) = bf16_widen4(*(const u32x2*)(x + i * 4));
    for (int64_t i = n4 * 4 + i0; i < n; i += stride) out[i] = bf16_widen1(x[i]);
}
extern "C" int zsg_cast_f32_bf16(const float* x, int64_t n, uint16_t* out, void* stream) {
    ZSG_REQUIRE(x && out && n >= 0, "cast_f32_bf16: bad argument");
    if (n == 0) return 0;
    const int vec = (((uintptr_t)x & 15) | ((uintptr_t)out & 7)) == 0;
    ZSG_LAUNCH(cast_f32_bf16_kernel, dim3(grid_for((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, n, vec, out);
    ZSG_CHECK_LAUNCH("cast_f32_bf16");
    return 0;
}
extern "C" int zsg_cast_bf16_f32(const uint16_t* x, int64_t n, float* out, void* stream) {
    ZSG_REQUIRE(x && out && n >= 0, "cast_bf16_f32: bad argument");
    if (n == 0) return 0;
    const int vec = (((uintptr_t)out & 15) | ((uintptr_t)x & 7)) == 0;
    ZSG_LAUNCH(cast_bf16_f32_kernel, dim3(grid_for((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, n, vec, out);
    ZSG_CHECK_LAUNCH("cast_bf16_f32");
    return 0;
}

// ---- head conv0's shared-image epilogue with a bf16 h1 ---------------------------------------------------------------------------
// zsg_head_shared_conv0 (misc.hip: head_shared_conv0_kernel) with the one difference that h1 is stored as bf16.  Y, G, V and bias are
// fp32; the summation order is that kernel's:  c = (taps in row-major order, summed from 0) + bias;  h1 = relu((Y + G) + c);  without G:
// relu(Y + c);  without V: c = bias — then ONE rounding.  Same block order, same NaN rows for an index outside [0, Bi).
struct SharedLevels {
    int nlev;
    int h[ZSG_MAX_SEG], w[ZSG_MAX_SEG];
    int p0[ZSG_MAX_SEG + 1];      // first pixel of a level in the concatenation of all levels
};

__global__ __launch_bounds__(256) void head_shared_conv0_bf16_kernel(const float* __restrict__ Y, const void* __restrict__ img_idx, int idx_i64,
                                                                     const float* __restrict__ bias, const float* __restrict__ G,
                                                                     const float* __restrict__ V, int Bi, int Q, int N, SharedLevels L,
                                                                     uint16_t* __restrict__ out, int parts, int nblocks, int n8) {
    extern __shared__ __attribute__((aligned(16))) float S[];      // [16][N]
    const int lb = (int)(blockIdx.x % 8) * n8 + (int)(blockIdx.x / 8);
    if (lb >= nblocks) return;                                     // (block-uniform, in front of the barrier)
    const int part = lb / Q, q = lb - part * Q;
    const long long im = idx_i64 ? ((const long long*)img_idx)[q] : (long long)((const int*)img_idx)[q];
    const bool live = im >= 0 && im < Bi;
    for (int n = threadIdx.x; n < N; n += 256) {
        float v[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) v[t] = V ? V[(int64_t)q * N * 9 + (int64_t)n * 9 + t] : 0.f;
        const float bn = bias[n];
#pragma unroll
        for (int cls = 0; cls < 16; ++cls) {       // bit 0: top row, 1: bottom row, 2: left column, 3: right column
            float a = 0.f;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                if ((r == 0 && (cls & 1)) || (r == 2 && (cls & 2))) continue;
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    if ((t == 0 && (cls & 4)) || (t == 2 && (cls & 8))) continue;
                    a += v[r * 3 + t];
                }
            }
            S[cls * N + n] = a + bn;
        }
    }
    __syncthreads();
    const int n4 = N / 4, P = L.p0[L.nlev];
    const int64_t total = (int64_t)P * n4;
    const float qnan = __builtin_nanf("");
    for (int64_t i = (int64_t)part * 256 + threadIdx.x; i < total; i += (int64_t)parts * 256) {
        const int c = (int)(i % n4) * 4;
        const int p = (int)(i / n4);
        int lv = 0;
#pragma unroll
        for (int j = 1; j < ZSG_MAX_SEG; ++j)
            if (j < L.nlev && p >= L.p0[j]) lv = j;
        const int px = p - L.p0[lv], w = L.w[lv], h = L.h[lv];
        const int y = px / w, x = px - y * w;
        const int cls = (y == 0 ? 1 : 0) | (y == h - 1 ? 2 : 0) | (x == 0 ? 4 : 0) | (x == w - 1 ? 8 : 0);
        f32x4 acc;
        if (live) {
            acc = *(const f32x4*)(Y + ((int64_t)Bi * L.p0[lv] + im * h * w + px) * N + c);
            if (G) acc += *(const f32x4*)(G + ((int64_t)L.p0[lv] + px) * N + c);
            acc += *(const f32x4*)(S + cls * N + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaxf(acc[e], 0.f);
        } else {
            acc = f32x4{qnan, qnan, qnan, qnan};
        }
        *(u32x2*)(out + ((int64_t)Q * L.p0[lv] + (int64_t)q * h * w + px) * N + c) = bf16_pack4(acc);
    }
}
extern "C" int zsg_head_shared_conv0_bf16(const float* Y, const void* img_idx, int32_t idx_i64, const float* bias, const float* G, const float* V,
                                          int32_t Bi, int32_t Q, int32_t nlev, const int32_t* hw, int32_t N, uint16_t* out, void* stream) {
    ZSG_REQUIRE(Y && img_idx && bias && out && hw && Bi > 0 && Q > 0 && nlev > 0 && nlev <= ZSG_MAX_SEG && N > 0 && (N % 4) == 0 && N <= 1024,
                "head_shared_conv0_bf16: bad argument");
    ZSG_REQUIRE((((uintptr_t)Y | (uintptr_t)G) & 15) == 0 && ((uintptr_t)out & 7) == 0, "head_shared_conv0_bf16: alignment");
    SharedLevels L;
    memset(&L, 0, sizeof(L));
    L.nlev = nlev;
    for (int i = 0; i < nlev; ++i) {
        ZSG_REQUIRE(hw[2 * i] > 0 && hw[2 * i + 1] > 0, "head_shared_conv0_bf16: level %d is empty", i);
        L.h[i] = hw[2 * i];
        L.w[i] = hw[2 * i + 1];
        L.p0[i + 1] = L.p0[i] + L.h[i] * L.w[i];
    }
    const int64_t per = (int64_t)L.p0[nlev] * (N / 4);
    int parts = (int)((per + 256 * 8 - 1) / (256 * 8));        // ~8 groups per thread
    const int cap = (4 * ZSG_NUM_CU + Q - 1) / Q;
    if (parts > cap) parts = cap;
    if (parts < 1) parts = 1;
    const int nblocks = parts * Q, n8 = (nblocks + 7) / 8;
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("head_shared_conv0_bf16", st, 0, ((double)Q * 2 + (double)Bi * 4) * L.p0[nlev] * N);
    ZSG_LAUNCH(head_shared_conv0_bf16_kernel, dim3(8 * n8), dim3(256), (size_t)16 * N * sizeof(float), st, Y, img_idx, idx_i64, bias, G, V, Bi, Q, N, L,
               out, parts, nblocks, n8);
    ZSG_CHECK_LAUNCH("head_shared_conv0_bf16");
    return 0;
}
