// film.hip — FiLM language modulation of head conv0 (cfg lang_fuse = "film"), gfx950.  Contracts: include/zsg.h.
//
// The feature GEMM of conv0 leaves its raw accumulator Y [Bi][P][N] (no bias, no additive map, no ReLU: the form the shared-image plans
// already have).  The language vector then acts on it twice: additively through V (the language columns of W0, as before) and
// multiplicatively through gamma[q][n] = sum_c Wg[n][c] * we[q][c]:
//   h1[q][p][n] = relu( (1 + gamma[q][n]) * Y[img_idx[q]][p][n] + bias[n] + G[p][n] + sum_{tap valid at p} V[q][n*9 + tap] )
// Three launches, all streaming passes over level-major packed pyramids (misc.hip: head_shared_conv0_kernel's layouts, 16-byte
// accesses, N % 4 == 0), all HBM-bound with no reuse a cache could serve beyond the Q / Bi re-reads of Y:
//   zsg_head_film_conv0      forward               (Q + Bi) * P * N * 4 bytes  (bf16 h1: Q * 2 + Bi * 4)
//   zsg_head_film_conv0_bwd  dY = sum_q (1+g) dy   (Q + Bi) * P * N * 4 bytes
//   zsg_head_film_dgamma     dgamma = sum_p dy * Y  ~ 2 * Q * P * N * 4 bytes (Y from L2 for the queries of one image) + the fp64 partials
// FIXED ARITHMETIC ORDER (this file is compiled with -ffp-contract=off: a product is rounded before the sum that follows it):
//   s = 1.0f + gamma;  t = s * Y;  c = (taps in row-major order, summed from 0) + bias;  h1 = relu((t + G) + c);  without G: relu(t + c).
// With gamma = 0, s = 1 and t = Y bit for bit, so the forward has zsg_head_shared_conv0's bits and the backward zsg_head_shared_conv0_bwd's.
// No float atomics, no inline assembly: every result is bit-identical run to run.
#include "bf16.h"

struct FilmLevels {
    int nlev;
    int h[ZSG_MAX_SEG], w[ZSG_MAX_SEG];
    int p0[ZSG_MAX_SEG + 1];           // first pixel of level i within an image's pixel list (prefix sums of h * w)
};

static int film_levels(FilmLevels& L, int nlev, const int32_t* hw, const char* who) {
    memset(&L, 0, sizeof(L));
    L.nlev = nlev;
    for (int i = 0; i < nlev; ++i) {
        ZSG_REQUIRE(hw[2 * i] > 0 && hw[2 * i + 1] > 0, "%s: level %d is empty", who, i);
        L.h[i] = hw[2 * i];
        L.w[i] = hw[2 * i + 1];
        L.p0[i + 1] = L.p0[i] + L.h[i] * L.w[i];
    }
    return 0;
}

// img_idx[q], or q itself without an index (the identity of a plain plan)
__device__ __forceinline__ long long film_index(const void* img_idx, int idx_i64, int q) {
    if (!img_idx) return q;
    return idx_i64 ? ((const long long*)img_idx)[q] : (long long)((const int*)img_idx)[q];
}

__device__ __forceinline__ int film_level(const FilmLevels& L, int p) {
    int lv = 0;
#pragma unroll
    for (int j = 1; j < ZSG_MAX_SEG; ++j)
        if (j < L.nlev && p >= L.p0[j]) lv = j;
    return lv;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------
// head_shared_conv0_kernel (misc.hip) with the scale: a block owns one query and a strided set of 16-byte elements; it builds the 16
// border-class values c[cls][n] = taps + bias of its query and the N scales s[n] = 1 + gamma[q][n] once in LDS (17 N floats), then
// streams.  Same block order (the query index runs fastest, dealt so that the queries of one pixel range land on one XCD: Y is read from
// HBM once per image and from L2 for the image's other queries).  A query whose index lies outside [0, Bi) gets NaN rows.
template <bool B16>
__global__ __launch_bounds__(256) void head_film_conv0_kernel(const float* __restrict__ Y, const void* __restrict__ img_idx, int idx_i64,
                                                              const float* __restrict__ bias, const float* __restrict__ G, const float* __restrict__ V,
                                                              const float* __restrict__ gamma, int Bi, int Q, int N, FilmLevels L, void* __restrict__ out,
                                                              int parts, int nblocks, int n8) {
    extern __shared__ __attribute__((aligned(16))) float S[];      // [16][N] border classes | [N] scales
    const int lb = (int)(blockIdx.x % 8) * n8 + (int)(blockIdx.x / 8);
    if (lb >= nblocks) return;                                     // (block-uniform, in front of the barrier)
    const int part = lb / Q, q = lb - part * Q;
    const long long im = film_index(img_idx, idx_i64, q);
    const bool live = im >= 0 && im < Bi;
    float* Sc = S + 16 * N;
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
        Sc[n] = 1.0f + gamma[(int64_t)q * N + n];
    }
    __syncthreads();
    const int n4 = N / 4, P = L.p0[L.nlev];
    const int64_t total = (int64_t)P * n4;
    const float qnan = __builtin_nanf("");
    for (int64_t i = (int64_t)part * 256 + threadIdx.x; i < total; i += (int64_t)parts * 256) {
        const int c = (int)(i % n4) * 4;
        const int p = (int)(i / n4);
        const int lv = film_level(L, p);
        const int px = p - L.p0[lv], w = L.w[lv], h = L.h[lv];
        const int y = px / w, x = px - y * w;
        const int cls = (y == 0 ? 1 : 0) | (y == h - 1 ? 2 : 0) | (x == 0 ? 4 : 0) | (x == w - 1 ? 8 : 0);
        f32x4 acc;
        if (live) {
            acc = *(const f32x4*)(Y + ((int64_t)Bi * L.p0[lv] + im * h * w + px) * N + c);
            acc = *(const f32x4*)(Sc + c) * acc;                   // t = s * Y, rounded here
            if (G) acc += *(const f32x4*)(G + ((int64_t)L.p0[lv] + px) * N + c);
            acc += *(const f32x4*)(S + cls * N + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaxf(acc[e], 0.f);
        } else {
            acc = f32x4{qnan, qnan, qnan, qnan};
        }
        const int64_t o = ((int64_t)Q * L.p0[lv] + (int64_t)q * h * w + px) * N + c;
        if constexpr (B16)
            *(u32x2*)((uint16_t*)out + o) = bf16_pack4(acc);
        else
            *(f32x4*)((float*)out + o) = acc;
    }
}

extern "C" int zsg_head_film_conv0(const float* Y, const void* img_idx, int32_t idx_i64, const float* bias, const float* G, const float* V, const float* gamma,
                                   int32_t Bi, int32_t Q, int32_t nlev, const int32_t* hw, int32_t N, void* out, int32_t out_bf16, void* stream) {
    ZSG_REQUIRE(Y && bias && gamma && out && hw && Bi > 0 && Q > 0 && nlev > 0 && nlev <= ZSG_MAX_SEG && N > 0 && (N % 4) == 0 && N <= 1024,
                "head_film_conv0: bad argument");
    ZSG_REQUIRE(img_idx || Bi == Q, "head_film_conv0: without img_idx (the identity) Bi must equal Q (%d vs %d)", Bi, Q);
    ZSG_REQUIRE((((uintptr_t)Y | (uintptr_t)G) & 15) == 0 && ((uintptr_t)out & (out_bf16 ? 7 : 15)) == 0, "head_film_conv0: alignment");
    FilmLevels L;
    if (film_levels(L, nlev, hw, "head_film_conv0")) return -1;
    const int64_t per = (int64_t)L.p0[nlev] * (N / 4);
    int parts = (int)((per + 256 * 8 - 1) / (256 * 8));        // ~8 16-byte elements per thread
    const int cap = (4 * ZSG_NUM_CU + Q - 1) / Q;
    if (parts > cap) parts = cap;
    if (parts < 1) parts = 1;
    const int nblocks = parts * Q, n8 = (nblocks + 7) / 8;
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("head_film_conv0", st, 0, ((double)Q * (out_bf16 ? 2 : 4) + (double)Bi * 4) * L.p0[nlev] * N);
    const size_t lds = (size_t)17 * N * sizeof(float);
    if (out_bf16)
        ZSG_LAUNCH(head_film_conv0_kernel<true>, dim3(8 * n8), dim3(256), lds, st, Y, img_idx, idx_i64, bias, G, V, gamma, Bi, Q, N, L, out, parts, nblocks,
                   n8);
    else
        ZSG_LAUNCH(head_film_conv0_kernel<false>, dim3(8 * n8), dim3(256), lds, st, Y, img_idx, idx_i64, bias, G, V, gamma, Bi, Q, N, L, out, parts, nblocks,
                   n8);
    ZSG_CHECK_LAUNCH("head_film_conv0");
    return 0;
}

// ---- backward: the gradient of the per-image accumulator --------------------------------------------------------------------------
// head_shared_conv0_bwd_kernel (misc.hip) with each query's row scaled: a block owns ONE image slot and a strided set of 16-byte
// elements of it, fetches the Q indices once into LDS (a value outside [0, Bi) becomes -1 and matches no slot), then walks q = 0 .. Q-1
// (a block-uniform loop and branch) and adds s[q] * dy[q] in that order with plain fp32 operations: the product is rounded, then added.
// Every element of dY is written (zeros for a slot no query points to).  s = 1 + gamma is formed per use (one add per 16 bytes read).
__global__ __launch_bounds__(256) void head_film_conv0_bwd_kernel(const float* __restrict__ dy, const void* __restrict__ img_idx, int idx_i64,
                                                                  const float* __restrict__ gamma, int Bi, int Q, int N, FilmLevels L, float* __restrict__ dY,
                                                                  int parts) {
    extern __shared__ __attribute__((aligned(16))) int sidx[];     // [Q]
    const int part = (int)blockIdx.x / Bi, im = (int)blockIdx.x - part * Bi;
    for (int q = threadIdx.x; q < Q; q += 256) {
        const long long v = film_index(img_idx, idx_i64, q);
        sidx[q] = (v >= 0 && v < Bi) ? (int)v : -1;
    }
    __syncthreads();
    const int n4 = N / 4, P = L.p0[L.nlev];
    const int64_t total = (int64_t)P * n4, step = (int64_t)parts * 256;
    for (int64_t i0 = (int64_t)part * 256 + threadIdx.x; i0 < total; i0 += 4 * step) {
        int64_t src[4], qs[4], dst[4];
        int ch[4];
        f32x4 acc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = i0 + k * step;
            acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            src[k] = -1;
            qs[k] = dst[k] = 0;
            ch[k] = 0;
            if (i < total) {
                const int c = (int)(i % n4) * 4;
                const int p = (int)(i / n4);
                const int lv = film_level(L, p);
                const int64_t hw = (int64_t)L.h[lv] * L.w[lv], px = p - L.p0[lv];
                src[k] = ((int64_t)Q * L.p0[lv] + px) * N + c;               // query 0's element; query q lies q * hw * N behind it
                qs[k] = hw * N;
                dst[k] = ((int64_t)Bi * L.p0[lv] + (int64_t)im * hw + px) * N + c;
                ch[k] = c;
            }
        }
        for (int q = 0; q < Q; ++q) {
            if (sidx[q] != im) continue;                                   // (block-uniform)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (src[k] >= 0) {
                    const f32x4 s = *(const f32x4*)(gamma + (int64_t)q * N + ch[k]) + 1.0f;
                    acc[k] += s * *(const f32x4*)(dy + src[k] + (int64_t)q * qs[k]);
                }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (src[k] >= 0) *(f32x4*)(dY + dst[k]) = acc[k];
    }
}

extern "C" int zsg_head_film_conv0_bwd(const float* dy, const void* img_idx, int32_t idx_i64, const float* gamma, int32_t Bi, int32_t Q, int32_t nlev,
                                       const int32_t* hw, int32_t N, float* dY, void* stream) {
    ZSG_REQUIRE(dy && gamma && dY && hw && Bi > 0 && Q > 0 && Q <= 8192 && nlev > 0 && nlev <= ZSG_MAX_SEG && N > 0 && (N % 4) == 0 && N <= 1024,
                "head_film_conv0_bwd: bad argument");
    ZSG_REQUIRE(img_idx || Bi == Q, "head_film_conv0_bwd: without img_idx (the identity) Bi must equal Q (%d vs %d)", Bi, Q);
    ZSG_REQUIRE((((uintptr_t)dy | (uintptr_t)dY | (uintptr_t)gamma) & 15) == 0, "head_film_conv0_bwd: alignment");
    FilmLevels L;
    if (film_levels(L, nlev, hw, "head_film_conv0_bwd")) return -1;
    const int64_t per = (int64_t)L.p0[nlev] * (N / 4);
    int parts = (int)((per + 256 * 4 - 1) / (256 * 4));        // 4 16-byte elements per thread per query of the slot
    const int cap = (8 * ZSG_NUM_CU + Bi - 1) / Bi;
    if (parts > cap) parts = cap;
    if (parts < 1) parts = 1;
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("head_film_conv0_bwd", st, 0, ((double)Q + Bi) * L.p0[nlev] * N * 4);
    ZSG_LAUNCH(head_film_conv0_bwd_kernel, dim3(parts * Bi), dim3(256), (size_t)Q * sizeof(int), st, dy, img_idx, idx_i64, gamma, Bi, Q, N, L, dY, parts);
    ZSG_CHECK_LAUNCH("head_film_conv0_bwd");
    return 0;
}

// ---- backward: the gradient of the scale --------------------------------------------------------------------------------------------
//   dgamma[q][n] = sum_p dy[q][p][n] * Y[img_idx[q]][p][n]      (all levels)
// A column sum of a product, in two stages.  Stage 1: block (q, part) walks the pixels  part * R + r + k * parts * R  (R = 256 / (N/4)
// pixel rows per block iteration, lane = one 16-byte channel group of one row), each lane keeps 4 fp64 sums (the fp32 x fp32 product is
// exact in fp64: one fma = one rounding per term), the R row sums of a channel are added through LDS in row order and the block writes
// partial[q][part][n] (fp64).  Stage 2: one lane per (q, n) adds the parts in index order, rounds ONCE to fp32 and writes dgamma[q][n]
// and, when asked, the transposed copy dgamma_t[n][q] (the operand layout of the small weight-gradient GEMM that forms d(we)).
// The order of every sum is fixed by (P, N, Q) alone: no atomics, the same bits on every run.  A query whose index lies outside
// [0, Bi) reads nothing and gets zeros.
static inline int film_dgamma_rows(int N) { return 256 / (N / 4); }       // pixel rows per block iteration (N <= 1024: >= 1)
static inline int film_dgamma_parts(int P, int Q, int N) {
    const int R = film_dgamma_rows(N);
    int parts = (P + R * 8 - 1) / (R * 8);                     // ~8 16-byte element pairs per lane
    const int cap = (4 * ZSG_NUM_CU + Q - 1) / Q;              // Q = 16: up to 64 parts, 1024 blocks = 4 per CU
    if (parts > cap) parts = cap;
    return parts < 1 ? 1 : parts;
}

__global__ __launch_bounds__(256) void head_film_dgamma_part_kernel(const float* __restrict__ dy, const float* __restrict__ Y, const void* __restrict__ img_idx,
                                                                    int idx_i64, int Bi, int Q, int N, FilmLevels L, double* __restrict__ partial, int parts, int R) {
    extern __shared__ __attribute__((aligned(16))) double D[];     // [R][N]
    const int part = (int)blockIdx.x / Q, q = (int)blockIdx.x - part * Q;
    const long long im = film_index(img_idx, idx_i64, q);
    const bool live = im >= 0 && im < Bi;
    const int n4 = N / 4, P = L.p0[L.nlev];
    const int r = (int)threadIdx.x / n4, c = ((int)threadIdx.x - r * n4) * 4;
    double a0 = 0., a1 = 0., a2 = 0., a3 = 0.;
    if (live && r < R) {
        for (int p = part * R + r; p < P; p += parts * R) {
            const int lv = film_level(L, p);
            const int64_t hw = (int64_t)L.h[lv] * L.w[lv], px = p - L.p0[lv];
            const f32x4 g = *(const f32x4*)(dy + ((int64_t)Q * L.p0[lv] + (int64_t)q * hw + px) * N + c);
            const f32x4 y = *(const f32x4*)(Y + ((int64_t)Bi * L.p0[lv] + im * hw + px) * N + c);
            a0 = fma((double)g[0], (double)y[0], a0);
            a1 = fma((double)g[1], (double)y[1], a1);
            a2 = fma((double)g[2], (double)y[2], a2);
            a3 = fma((double)g[3], (double)y[3], a3);
        }
    }
    if (r < R) {
        double* d = D + (int64_t)r * N + c;
        d[0] = a0, d[1] = a1, d[2] = a2, d[3] = a3;
    }
    __syncthreads();
    for (int n = threadIdx.x; n < N; n += 256) {
        double s = 0.;
        for (int k = 0; k < R; ++k) s += D[k * N + n];
        partial[((int64_t)q * parts + part) * N + n] = s;
    }
}

__global__ __launch_bounds__(256) void head_film_dgamma_final_kernel(const double* __restrict__ partial, int Q, int N, int parts, float* __restrict__ dgamma,
                                                                     float* __restrict__ dgamma_t) {
    const int64_t total = (int64_t)Q * N;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int q = (int)(i / N), n = (int)(i - (int64_t)q * N);
        double s = 0.;
        for (int k = 0; k < parts; ++k) s += partial[((int64_t)q * parts + k) * N + n];
        const float v = (float)s;
        dgamma[i] = v;
        if (dgamma_t) dgamma_t[(int64_t)n * Q + q] = v;
    }
}

extern "C" int64_t zsg_head_film_dgamma_ws_bytes(int32_t Q, int32_t nlev, const int32_t* hw, int32_t N) {
    if (!hw || Q <= 0 || nlev <= 0 || nlev > ZSG_MAX_SEG || N <= 0 || (N % 4) || N > 1024) return -1;
    int64_t P = 0;
    for (int i = 0; i < nlev; ++i) {
        if (hw[2 * i] <= 0 || hw[2 * i + 1] <= 0) return -1;
        P += (int64_t)hw[2 * i] * hw[2 * i + 1];
    }
    if (P > 0x7fffffff) return -1;
    return (int64_t)Q * film_dgamma_parts((int)P, Q, N) * N * (int64_t)sizeof(double);
}

extern "C" int zsg_head_film_dgamma(const float* dy, const float* Y, const void* img_idx, int32_t idx_i64, int32_t Bi, int32_t Q, int32_t nlev, const int32_t* hw,
                                    int32_t N, float* dgamma, float* dgamma_t, void* ws, int64_t ws_bytes, void* stream) {
    ZSG_REQUIRE(dy && Y && dgamma && ws && hw && Bi > 0 && Q > 0 && nlev > 0 && nlev <= ZSG_MAX_SEG && N > 0 && (N % 4) == 0 && N <= 1024,
                "head_film_dgamma: bad argument");
    ZSG_REQUIRE(img_idx || Bi == Q, "head_film_dgamma: without img_idx (the identity) Bi must equal Q (%d vs %d)", Bi, Q);
    ZSG_REQUIRE((((uintptr_t)dy | (uintptr_t)Y) & 15) == 0 && ((uintptr_t)ws & 7) == 0, "head_film_dgamma: alignment");
    FilmLevels L;
    if (film_levels(L, nlev, hw, "head_film_dgamma")) return -1;
    const int P = L.p0[nlev], R = film_dgamma_rows(N), parts = film_dgamma_parts(P, Q, N);
    const int64_t need = (int64_t)Q * parts * N * (int64_t)sizeof(double);
    ZSG_REQUIRE(ws_bytes >= need, "head_film_dgamma: workspace of %lld bytes, %lld needed (zsg_head_film_dgamma_ws_bytes)", (long long)ws_bytes,
                (long long)need);
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("head_film_dgamma", st, 2.0 * Q * P * N, 2.0 * Q * P * N * 4 + 2.0 * need);
    ZSG_LAUNCH(head_film_dgamma_part_kernel, dim3(parts * Q), dim3(256), (size_t)R * N * sizeof(double), st, dy, Y, img_idx, idx_i64, Bi, Q, N, L, (double*)ws,
               parts, R);
    ZSG_CHECK_LAUNCH("head_film_dgamma");
    int fb = (int)(((int64_t)Q * N + 255) / 256);
    if (fb > 4 * ZSG_NUM_CU) fb = 4 * ZSG_NUM_CU;
    ZSG_LAUNCH(head_film_dgamma_final_kernel, dim3(fb), dim3(256), 0, st, (const double*)ws, Q, N, parts, dgamma, dgamma_t);
    ZSG_CHECK_LAUNCH("head_film_dgamma(final)");
    return 0;
}
