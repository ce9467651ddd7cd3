// words.hip — word-level attention modulation of head conv0 (cfg lang_fuse = "words"), gfx950.  Contracts: include/zsg.h.
//
// film.hip's scale gamma[q][n] becomes a function of the pixel: conv0's raw feature accumulator Y [Bi][P][N] is also the pixel's
// attention query over the projected BiLSTM outputs Kw / Vw [Q][T][N] of its phrase (c = `scale`, 1 / sqrt(N) in the network):
//   s[q][p][t]  = c * sum_n Y[img_idx[q]][p][n] * Kw[q][t][n]                    t < len_q
//   alpha[q][p] = softmax over t < len_q of s (max subtracted), 0 at t >= len_q;  len_q = 0: alpha = 0
//   gamma[q][p][n] = sum_t alpha[q][p][t] * Vw[q][t][n]
//   h1[q][p][n] = relu( (1 + gamma[q][p][n]) * Y[img_idx[q]][p][n] + bias[n] + G[p][n] + sum_{tap valid at p} V[q][n*9 + tap] )
// Layouts are film.hip's (level-major packed pyramids, 16-byte accesses, N % 4 == 0).  ONE WAVE OWNS ONE PIXEL ROW: lane l holds the
// 16-byte channel groups l, l + 64, .. (N = 256: one group, 4 channels) of Y, read once for both uses; a score is one wave reduction
// (a 6-step xor butterfly: every lane ends with the same bits), lane t keeps the score of token t (T <= 64 = the wave), the softmax is
// two more wave reductions over the lanes, and alpha_t reaches the gamma sum by a lane broadcast.  A block (4 waves) owns one query and
// a strided set of pixels; len_q, the bound of every token loop, is block-uniform.
// TOKEN CHUNK: a query of len_q <= words_chunk(N) tokens (16 at N <= 256) has its Kw / Vw rows staged once per block in LDS
// (16 N + 2 * chunk * N floats with the 16 border classes: 48 KiB at N = 256, never above 64 KiB); a longer query reads the rows from
// global memory (L2), with the same arithmetic in the same order.
// COST at the workload's sizes (Q = 16, P ~ 1940, N = 256, len <~ 13): a streaming pass like film's — HBM bytes (Q + Bi) * P * N * 4
// (+ Q * P * T * 4 for alpha in training) — plus about 4 * len * N flops per pixel row (2 len N for the scores, 2 len N for gamma):
// 16 * 1940 * 4 * 13 * 256 = 0.41 GFLOP against 64 MB (Bi = Q = 16, one image per query; 40 MB at Bi = 4), far below the fp32 vector
// rate: fp32 vector math is enough, no MFMA.  (What sets the pace is the latency of the per-token wave reductions: DESIGN section 7.)
// The backward (three launches) has the same shape; its byte counts stand at zsg_head_words_conv0_bwd below.
// FIXED ARITHMETIC ORDER (compiled with -ffp-contract=off: every product is rounded before the sum that follows it): tokens ascending
// everywhere; a lane's part of a dot product runs over its groups, then the 4 channels of a group, ascending from 0; gamma is summed
// from 0; then film's  s = 1.0f + gamma; t = s * Y; c = (taps row-major from 0) + bias; h1 = relu((t + G) + c).  With Vw = 0 the
// forward has zsg_head_shared_conv0's bits; with len = 1 everywhere alpha = 1 and it has zsg_head_film_conv0's for gamma = Vw[:, 0].
// No float atomics, no inline assembly: every result is bit-identical run to run.
#include <math.h>

#include "bf16.h"

#define WORDS_MAXG 4            // 16-byte channel groups per lane: N <= 1024
#define WORDS_TT 4              // tokens per block of the dKw / dVw partial sums

struct WordLevels {
    int nlev;
    int h[ZSG_MAX_SEG], w[ZSG_MAX_SEG];
    int p0[ZSG_MAX_SEG + 1];           // first pixel of level i within an image's pixel list (prefix sums of h * w)
};

static int words_levels(WordLevels& L, int nlev, const int32_t* hw, const char* who) {
    memset(&L, 0, sizeof(L));
    L.nlev = nlev;
    int64_t P = 0;
    for (int i = 0; i < nlev; ++i) {
        ZSG_REQUIRE(hw[2 * i] > 0 && hw[2 * i + 1] > 0, "%s: level %d is empty", who, i);
        L.h[i] = hw[2 * i];
        L.w[i] = hw[2 * i + 1];
        P += (int64_t)L.h[i] * L.w[i];
        ZSG_REQUIRE(P <= 0x3fffffff, "%s: too many pixels", who);
        L.p0[i + 1] = (int)P;
    }
    return 0;
}

// tokens whose Kw / Vw rows fit in LDS beside the 16 border classes (64 KiB in all at most); 0 = never staged
static inline int words_chunk(int N) {
    const int c = (16384 - 16 * N) / (2 * N);
    return c > 16 ? 16 : (c < 0 ? 0 : c);
}

__device__ __forceinline__ long long words_index(const void* img_idx, int idx_i64, int q) {
    if (!img_idx) return q;
    return idx_i64 ? ((const long long*)img_idx)[q] : (long long)((const int*)img_idx)[q];
}

__device__ __forceinline__ int words_level(const WordLevels& L, int p) {
    int lv = 0;
#pragma unroll
    for (int j = 1; j < ZSG_MAX_SEG; ++j)
        if (j < L.nlev && p >= L.p0[j]) lv = j;
    return lv;
}

// clamp(lens[q], 0, T) as an integer (a NaN counts as 0)
__device__ __forceinline__ int words_len(const float* lens, int q, int T) { return (int)fminf(fmaxf(lens[q], 0.f), (float)T); }

__device__ __forceinline__ float words_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// a lane's part of the dot product of its pixel row (x: this lane's groups) with one token row (no reduction yet)
__device__ __forceinline__ float words_dot_part(const f32x4* x, const float* __restrict__ row, int lane, int n4) {
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < WORDS_MAXG; ++k) {
        const int g = lane + 64 * k;
        if (g < n4) {
            const f32x4 v = *(const f32x4*)(row + 4 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e) a += x[k][e] * v[e];
        }
    }
    return a;
}

// The dot products of the pixel row with the token rows t < len (row t at rows + t * N), scaled, token t's into lane t.  Four tokens
// per step: their four butterflies are independent chains the hardware overlaps; each token's sum is the
// 6-step xor butterfly (offsets 32 .. 1) over the lanes' parts: the same bits in every lane.
__device__ __forceinline__ float words_scores(const f32x4* x, const float* __restrict__ rows, int len, int N, float scale, int lane, int n4) {
    float sc = 0.f;
    for (int t0 = 0; t0 < len; t0 += 4) {
        float a[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = (t0 + j < len) ? words_dot_part(x, rows + (int64_t)(t0 + j) * N, lane, n4) : 0.f;      // (block-uniform guard)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] += __shfl_xor(a[j], o, 64);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (lane == t0 + j) sc = scale * a[j];
    }
    return sc;
}

// acc[k] += a * row (this lane's groups)
__device__ __forceinline__ void words_axpy(f32x4* acc, float a, const float* __restrict__ row, int lane, int n4) {
#pragma unroll
    for (int k = 0; k < WORDS_MAXG; ++k) {
        const int g = lane + 64 * k;
        if (g < n4) acc[k] += a * *(const f32x4*)(row + 4 * g);
    }
}

// rows t < len of src [T][N] (query q's) -> dst [len][N] in LDS
__device__ __forceinline__ void words_stage(float* dst, const float* __restrict__ src, int len, int N) {
    const int n = len * (N / 4);
    for (int i = threadIdx.x; i < n; i += 256) *(f32x4*)(dst + 4 * i) = *(const f32x4*)(src + 4 * (int64_t)i);
}

// alpha of this wave's pixel, token t in lane t: sc = the score of token `lane` (anything at lane >= len)
__device__ __forceinline__ float words_softmax(float sc, int lane, int len) {
    const bool on = lane < len;
    const float m = words_wave_max(on ? sc : -INFINITY);
    const float e = on ? expf(sc - m) : 0.f;
    const float sum = wave_sum(e);
    return on ? e / sum : 0.f;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------
// Block order as head_film_conv0_kernel (the query index runs fastest, dealt so that the queries of one pixel range land on one XCD).
template <bool B16>
__global__ __launch_bounds__(256) void head_words_conv0_kernel(const float* __restrict__ Y, const void* __restrict__ img_idx, int idx_i64,
                                                               const float* __restrict__ bias, const float* __restrict__ G, const float* __restrict__ V,
                                                               const float* __restrict__ Kw, const float* __restrict__ Vw, const float* __restrict__ lens,
                                                               float scale, int Bi, int Q, int T, int N, WordLevels L, void* __restrict__ out,
                                                               float* __restrict__ alpha, int parts, int nblocks, int n8, int TC) {
    extern __shared__ __attribute__((aligned(16))) float S[];      // [16][N] border classes | [TC][N] Kw rows | [TC][N] Vw rows
    const int lb = (int)(blockIdx.x % 8) * n8 + (int)(blockIdx.x / 8);
    if (lb >= nblocks) return;                                     // (block-uniform, in front of the barrier)
    const int part = lb / Q, q = lb - part * Q;
    const long long im = words_index(img_idx, idx_i64, q);
    const bool live = im >= 0 && im < Bi;
    const int len = live ? words_len(lens, q, T) : 0;
    const bool staged = len <= TC;                                 // (block-uniform)
    float* SK = S + 16 * N;
    float* SV = SK + (int64_t)TC * N;
    const float* Kq = Kw + (int64_t)q * T * N;
    const float* Vq = Vw + (int64_t)q * T * N;
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
    if (staged) {
        words_stage(SK, Kq, len, N);
        words_stage(SV, Vq, len, N);
    }
    __syncthreads();
    const int n4 = N / 4, P = L.p0[L.nlev];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const float qnan = __builtin_nanf("");
    for (int p = part * 4 + wave; p < P; p += parts * 4) {
        const int lv = words_level(L, p);
        const int px = p - L.p0[lv], w = L.w[lv], h = L.h[lv];
        const int y_ = px / w, x_ = px - y_ * w;
        const int cls = (y_ == 0 ? 1 : 0) | (y_ == h - 1 ? 2 : 0) | (x_ == 0 ? 4 : 0) | (x_ == w - 1 ? 8 : 0);
        const int64_t orow = (int64_t)Q * L.p0[lv] + (int64_t)q * h * w + px;
        f32x4 y[WORDS_MAXG], gm[WORDS_MAXG];
        float al = 0.f;
        if (live) {
            const float* yr = Y + ((int64_t)Bi * L.p0[lv] + im * h * w + px) * N;
#pragma unroll
            for (int k = 0; k < WORDS_MAXG; ++k) {
                const int g = lane + 64 * k;
                y[k] = g < n4 ? *(const f32x4*)(yr + 4 * g) : f32x4{0.f, 0.f, 0.f, 0.f};
                gm[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            const float sc = staged ? words_scores(y, SK, len, N, scale, lane, n4) : words_scores(y, Kq, len, N, scale, lane, n4);
            al = words_softmax(sc, lane, len);
            if (staged) {
                for (int t = 0; t < len; ++t) words_axpy(gm, __shfl(al, t, 64), SV + t * N, lane, n4);
            } else {
                for (int t = 0; t < len; ++t) words_axpy(gm, __shfl(al, t, 64), Vq + (int64_t)t * N, lane, n4);
            }
        }
#pragma unroll
        for (int k = 0; k < WORDS_MAXG; ++k) {
            const int g = lane + 64 * k;
            if (g >= n4) continue;
            const int c = 4 * g;
            f32x4 acc;
            if (live) {
                const f32x4 s = gm[k] + 1.0f;
                acc = s * y[k];                                    // t = s * Y, rounded here
                if (G) acc += *(const f32x4*)(G + ((int64_t)L.p0[lv] + px) * N + c);
                acc += *(const f32x4*)(S + cls * N + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = fmaxf(acc[e], 0.f);
            } else {
                acc = f32x4{qnan, qnan, qnan, qnan};
            }
            const int64_t o = orow * N + c;
            if constexpr (B16)
                *(u32x2*)((uint16_t*)out + o) = bf16_pack4(acc);
            else
                *(f32x4*)((float*)out + o) = acc;
        }
        if (alpha && lane < T) alpha[orow * T + lane] = al;
    }
}

static inline int words_fwd_parts(int P, int Q) {
    int parts = (P + 4 * 8 - 1) / (4 * 8);                     // ~8 pixel rows per wave
    const int cap = (2 * ZSG_NUM_CU + Q - 1) / Q;              // Q = 16: up to 32 parts, 512 blocks = 2 per CU
    if (parts > cap) parts = cap;
    return parts < 1 ? 1 : parts;
}

extern "C" int zsg_head_words_conv0(const float* Y, const void* img_idx, int32_t idx_i64, const float* bias, const float* G, const float* V, const float* Kw,
                                    const float* Vw, const float* lens, float scale, int32_t Bi, int32_t Q, int32_t T, int32_t nlev, const int32_t* hw, int32_t N,
                                    void* out, int32_t out_bf16, float* alpha, void* stream) {
    ZSG_REQUIRE(Y && bias && Kw && Vw && lens && out && hw && Bi > 0 && Q > 0 && nlev > 0 && nlev <= ZSG_MAX_SEG && N > 0 && (N % 4) == 0 && N <= 1024,
                "head_words_conv0: bad argument");
    ZSG_REQUIRE(T >= 1 && T <= 64, "head_words_conv0: T = %d outside [1, 64]", T);
    ZSG_REQUIRE(img_idx || Bi == Q, "head_words_conv0: without img_idx (the identity) Bi must equal Q (%d vs %d)", Bi, Q);
    ZSG_REQUIRE((((uintptr_t)Y | (uintptr_t)G | (uintptr_t)Kw | (uintptr_t)Vw) & 15) == 0 && ((uintptr_t)out & (out_bf16 ? 7 : 15)) == 0 &&
                    ((uintptr_t)alpha & 3) == 0,
                "head_words_conv0: alignment");
    WordLevels L;
    if (words_levels(L, nlev, hw, "head_words_conv0")) return -1;
    const int P = L.p0[nlev], parts = words_fwd_parts(P, Q), TC = words_chunk(N);
    const int nblocks = parts * Q, n8 = (nblocks + 7) / 8;
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("head_words_conv0", st, 4.0 * Q * P * (double)T * N,
             ((double)Q * (out_bf16 ? 2 : 4) + (double)Bi * 4) * P * N + (alpha ? 4.0 * Q * P * T : 0.0) + 8.0 * Q * T * N);
    const size_t lds = ((size_t)16 * N + (size_t)2 * TC * N) * sizeof(float);
    if (out_bf16)
        ZSG_LAUNCH(head_words_conv0_kernel<true>, dim3(8 * n8), dim3(256), lds, st, Y, img_idx, idx_i64, bias, G, V, Kw, Vw, lens, scale, Bi, Q, T, N, L, out,
                   alpha, parts, nblocks, n8, TC);
    else
        ZSG_LAUNCH(head_words_conv0_kernel<false>, dim3(8 * n8), dim3(256), lds, st, Y, img_idx, idx_i64, bias, G, V, Kw, Vw, lens, scale, Bi, Q, T, N, L, out,
                   alpha, parts, nblocks, n8, TC);
    ZSG_CHECK_LAUNCH("head_words_conv0");
    return 0;
}

// ---- backward, launch 1: per pixel row ----------------------------------------------------------------------------------------------
//   dgamma = dy * Y;  dalpha_t = dgamma . Vw_t;  ds_t = alpha_t (dalpha_t - sum_k alpha_k dalpha_k);
//   dYq = (1 + gamma) * dy + c * sum_t ds_t Kw_t         (gamma recomputed from alpha and Vw in the forward's order)
// The forward's wave-per-pixel shape and staging.  ds [Q][P][T] (0 at t >= len) goes to the workspace for launch 2.
__global__ __launch_bounds__(256) void head_words_bwd_pix_kernel(const float* __restrict__ dy, const float* __restrict__ Y, const void* __restrict__ img_idx,
                                                                 int idx_i64, const float* __restrict__ Kw, const float* __restrict__ Vw,
                                                                 const float* __restrict__ alpha, const float* __restrict__ lens, float scale, int Bi, int Q,
                                                                 int T, int N, WordLevels L, float* __restrict__ dYq, float* __restrict__ ds, int parts,
                                                                 int nblocks, int n8, int TC) {
    extern __shared__ __attribute__((aligned(16))) float S[];      // [TC][N] Kw rows | [TC][N] Vw rows
    const int lb = (int)(blockIdx.x % 8) * n8 + (int)(blockIdx.x / 8);
    if (lb >= nblocks) return;
    const int part = lb / Q, q = lb - part * Q;
    const long long im = words_index(img_idx, idx_i64, q);
    const bool live = im >= 0 && im < Bi;
    const int len = live ? words_len(lens, q, T) : 0;
    const bool staged = len <= TC;
    float* SK = S;
    float* SV = SK + (int64_t)TC * N;
    const float* Kq = Kw + (int64_t)q * T * N;
    const float* Vq = Vw + (int64_t)q * T * N;
    if (staged) {
        words_stage(SK, Kq, len, N);
        words_stage(SV, Vq, len, N);
    }
    __syncthreads();
    const int n4 = N / 4, P = L.p0[L.nlev];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    for (int p = part * 4 + wave; p < P; p += parts * 4) {
        const int lv = words_level(L, p);
        const int64_t hw = (int64_t)L.h[lv] * L.w[lv], px = p - L.p0[lv];
        const int64_t orow = (int64_t)Q * L.p0[lv] + (int64_t)q * hw + px;
        f32x4 g[WORDS_MAXG], dg[WORDS_MAXG], gm[WORDS_MAXG], acc[WORDS_MAXG];
        float dsv = 0.f;
#pragma unroll
        for (int k = 0; k < WORDS_MAXG; ++k) g[k] = dg[k] = gm[k] = acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (live) {
            const float* yr = Y + ((int64_t)Bi * L.p0[lv] + im * hw + px) * N;
#pragma unroll
            for (int k = 0; k < WORDS_MAXG; ++k) {
                const int c4 = lane + 64 * k;
                if (c4 < n4) {
                    g[k] = *(const f32x4*)(dy + orow * N + 4 * c4);
                    dg[k] = g[k] * *(const f32x4*)(yr + 4 * c4);
                }
            }
            const float al = lane < len ? alpha[orow * T + lane] : 0.f;
            const float da = staged ? words_scores(dg, SV, len, N, 1.0f, lane, n4) : words_scores(dg, Vq, len, N, 1.0f, lane, n4);
            const float dot = wave_sum(al * da);
            dsv = lane < len ? al * (da - dot) : 0.f;
            if (dYq) {
                if (staged) {
                    for (int t = 0; t < len; ++t) {
                        words_axpy(gm, __shfl(al, t, 64), SV + t * N, lane, n4);
                        words_axpy(acc, __shfl(dsv, t, 64), SK + t * N, lane, n4);
                    }
                } else {
                    for (int t = 0; t < len; ++t) {
                        words_axpy(gm, __shfl(al, t, 64), Vq + (int64_t)t * N, lane, n4);
                        words_axpy(acc, __shfl(dsv, t, 64), Kq + (int64_t)t * N, lane, n4);
                    }
                }
            }
        }
        if (dYq) {
#pragma unroll
            for (int k = 0; k < WORDS_MAXG; ++k) {
                const int c4 = lane + 64 * k;
                if (c4 >= n4) continue;
                const f32x4 s = gm[k] + 1.0f;
                const f32x4 a = s * g[k];
                const f32x4 b = scale * acc[k];
                *(f32x4*)(dYq + orow * N + 4 * c4) = a + b;        // (a dead query: g = acc = 0, zeros)
            }
        }
        if (ds && lane < T) ds[((int64_t)q * P + p) * T + lane] = dsv;
    }
}

// ---- backward, launches 2 and 3: the gradients of Kw and Vw -----------------------------------------------------------------------
//   dKw[q][t][n] = c * sum_p ds[q][p][t] * Y[img q][p][n]        dVw[q][t][n] = sum_p alpha[q][p][t] * dy[q][p][n] * Y[img q][p][n]
// Column sums of products, in two stages as zsg_head_film_dgamma.  Stage 1: block (q, part, token tile of WORDS_TT) walks the pixels
// part * R + r + k * parts * R (R = 256 / (N/4) rows per iteration, a lane = one 16-byte channel group of one row) with fp64
// accumulators (an fp32 x fp32 product is exact in fp64: one fma = one rounding per term), adds the R row sums of a channel through
// LDS in row order and writes partial[q][part][K|V][t][n] (fp64).  Stage 2: one lane per (q, t, n) adds the parts in index order,
// rounds ONCE to fp32 (dKw: after the fp64 product with c) and writes exact zeros at t >= len and for a dead query.
static inline int words_dkv_rows(int N) { return 256 / (N / 4); }
static inline int words_dkv_tiles(int T) { return (T + WORDS_TT - 1) / WORDS_TT; }
static inline int words_dkv_parts(int P, int Q, int T, int N) {
    const int R = words_dkv_rows(N);
    int parts = (P + R * 8 - 1) / (R * 8);
    int cap = (4 * ZSG_NUM_CU) / (Q * words_dkv_tiles(T));
    if (cap < 1) cap = 1;
    if (parts > cap) parts = cap;
    return parts < 1 ? 1 : parts;
}
static inline int64_t words_ds_bytes(int64_t P, int Q, int T) { return (((int64_t)Q * P * T * 4) + 15) & ~(int64_t)15; }

__global__ __launch_bounds__(256) void head_words_dkv_part_kernel(const float* __restrict__ dy, const float* __restrict__ Y, const void* __restrict__ img_idx,
                                                                  int idx_i64, const float* __restrict__ alpha, const float* __restrict__ ds,
                                                                  const float* __restrict__ lens, int Bi, int Q, int T, int N, WordLevels L,
                                                                  double* __restrict__ partial, int parts, int R, int ntiles, int doK, int doV) {
    extern __shared__ __attribute__((aligned(16))) double D[];     // [R][N]
    const int lb = xcd_remap((int)blockIdx.x, (int)gridDim.x);     // (the tiles of one (q, part) read the same rows: one XCD's L2)
    const int tile = lb % ntiles, qp = lb / ntiles;
    const int part = qp / Q, q = qp - part * Q;
    const long long im = words_index(img_idx, idx_i64, q);
    const bool live = im >= 0 && im < Bi;
    const int len = live ? words_len(lens, q, T) : 0;
    const int t0 = tile * WORDS_TT;
    if (t0 >= len) return;                                         // (block-uniform; the finalize launch reads no part of these rows)
    const int n4 = N / 4, P = L.p0[L.nlev];
    const int r = (int)threadIdx.x / n4, c = ((int)threadIdx.x - r * n4) * 4;
    double aK[WORDS_TT][4], aV[WORDS_TT][4];
#pragma unroll
    for (int j = 0; j < WORDS_TT; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) aK[j][e] = aV[j][e] = 0.;
    if (r < R) {
        for (int p = part * R + r; p < P; p += parts * R) {
            const int lv = words_level(L, p);
            const int64_t hw = (int64_t)L.h[lv] * L.w[lv], px = p - L.p0[lv];
            const int64_t orow = (int64_t)Q * L.p0[lv] + (int64_t)q * hw + px;
            const f32x4 y = *(const f32x4*)(Y + ((int64_t)Bi * L.p0[lv] + im * hw + px) * N + c);
            f32x4 g = f32x4{0.f, 0.f, 0.f, 0.f};
            if (doV) g = *(const f32x4*)(dy + orow * N + c);
            double dg[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) dg[e] = (double)g[e] * (double)y[e];
#pragma unroll
            for (int j = 0; j < WORDS_TT; ++j) {
                if (t0 + j >= len) continue;                       // (block-uniform)
                if (doK) {
                    const double s = (double)ds[((int64_t)q * P + p) * T + t0 + j];
#pragma unroll
                    for (int e = 0; e < 4; ++e) aK[j][e] = fma(s, (double)y[e], aK[j][e]);
                }
                if (doV) {
                    const double a = (double)alpha[orow * T + t0 + j];
#pragma unroll
                    for (int e = 0; e < 4; ++e) aV[j][e] = fma(a, dg[e], aV[j][e]);
                }
            }
        }
    }
#pragma unroll
    for (int which = 0; which < 2; ++which) {
        if (!(which ? doV : doK)) continue;
#pragma unroll
        for (int j = 0; j < WORDS_TT; ++j) {
            if (t0 + j >= len) continue;
            if (r < R) {
                double* d = D + (int64_t)r * N + c;
#pragma unroll
                for (int e = 0; e < 4; ++e) d[e] = which ? aV[j][e] : aK[j][e];
            }
            __syncthreads();
            for (int n = threadIdx.x; n < N; n += 256) {
                double s = 0.;
                for (int k = 0; k < R; ++k) s += D[k * N + n];
                partial[((((int64_t)q * parts + part) * 2 + which) * T + t0 + j) * N + n] = s;
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void head_words_dkv_final_kernel(const double* __restrict__ partial, const void* __restrict__ img_idx, int idx_i64,
                                                                   const float* __restrict__ lens, float scale, int Bi, int Q, int T, int N, int parts,
                                                                   float* __restrict__ dKw, float* __restrict__ dVw) {
    const int64_t total = (int64_t)Q * T * N;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int n = (int)(i % N);
        const int t = (int)((i / N) % T), q = (int)(i / ((int64_t)N * T));
        const long long im = words_index(img_idx, idx_i64, q);
        const bool on = im >= 0 && im < Bi && t < words_len(lens, q, T);
        double sk = 0., sv = 0.;
        if (on) {
            for (int k = 0; k < parts; ++k) {
                const int64_t b = (((int64_t)q * parts + k) * 2) * T;
                if (dKw) sk += partial[((b + t) * N) + n];
                if (dVw) sv += partial[((b + T + t) * N) + n];
            }
        }
        if (dKw) dKw[i] = on ? (float)((double)scale * sk) : 0.f;
        if (dVw) dVw[i] = on ? (float)sv : 0.f;
    }
}

extern "C" int64_t zsg_head_words_bwd_ws_bytes(int32_t Q, int32_t T, int32_t nlev, const int32_t* hw, int32_t N) {
    if (!hw || Q <= 0 || T < 1 || T > 64 || nlev <= 0 || nlev > ZSG_MAX_SEG || N <= 0 || (N % 4) || N > 1024) return -1;
    int64_t P = 0;
    for (int i = 0; i < nlev; ++i) {
        if (hw[2 * i] <= 0 || hw[2 * i + 1] <= 0) return -1;
        P += (int64_t)hw[2 * i] * hw[2 * i + 1];
        if (P > 0x3fffffff) return -1;
    }
    return words_ds_bytes(P, Q, T) + (int64_t)Q * words_dkv_parts((int)P, Q, T, N) * 2 * T * N * (int64_t)sizeof(double);
}

extern "C" int zsg_head_words_conv0_bwd(const float* dy, const float* Y, const void* img_idx, int32_t idx_i64, const float* Kw, const float* Vw,
                                        const float* alpha, const float* lens, float scale, int32_t Bi, int32_t Q, int32_t T, int32_t nlev, const int32_t* hw,
                                        int32_t N, float* dYq, float* dKw, float* dVw, void* ws, int64_t ws_bytes, void* stream) {
    ZSG_REQUIRE(dy && Y && Kw && Vw && alpha && lens && ws && hw && Bi > 0 && Q > 0 && nlev > 0 && nlev <= ZSG_MAX_SEG && N > 0 && (N % 4) == 0 &&
                    N <= 1024,
                "head_words_conv0_bwd: bad argument");
    ZSG_REQUIRE(T >= 1 && T <= 64, "head_words_conv0_bwd: T = %d outside [1, 64]", T);
    ZSG_REQUIRE(dYq || dKw || dVw, "head_words_conv0_bwd: no output");
    ZSG_REQUIRE(img_idx || Bi == Q, "head_words_conv0_bwd: without img_idx (the identity) Bi must equal Q (%d vs %d)", Bi, Q);
    ZSG_REQUIRE((((uintptr_t)dy | (uintptr_t)Y | (uintptr_t)Kw | (uintptr_t)Vw | (uintptr_t)dYq | (uintptr_t)ws) & 15) == 0 &&
                    (((uintptr_t)alpha | (uintptr_t)dKw | (uintptr_t)dVw) & 3) == 0,
                "head_words_conv0_bwd: alignment");
    WordLevels L;
    if (words_levels(L, nlev, hw, "head_words_conv0_bwd")) return -1;
    const int P = L.p0[nlev], R = words_dkv_rows(N), ntiles = words_dkv_tiles(T), bparts = words_dkv_parts(P, Q, T, N);
    const int64_t dsb = words_ds_bytes(P, Q, T), pb = (int64_t)Q * bparts * 2 * T * N * (int64_t)sizeof(double);
    ZSG_REQUIRE(ws_bytes >= dsb + pb, "head_words_conv0_bwd: workspace of %lld bytes, %lld needed (zsg_head_words_bwd_ws_bytes)", (long long)ws_bytes,
                (long long)(dsb + pb));
    float* ds = (float*)ws;
    double* partial = (double*)((char*)ws + dsb);
    hipStream_t st = (hipStream_t)stream;
    const double rows = (double)Q * P;
    const bool pix = dYq || dKw;           // the pixel launch has an output: dYq, or ds for dKw (dVw alone needs alpha and dy * Y only)
    ZSG_PROF("head_words_conv0_bwd", st, (pix ? rows * T * N * 6.0 : 0.0) + rows * T * N * ((dKw ? 2.0 : 0.0) + (dVw ? 2.0 : 0.0)),
             (pix ? rows * N * 4 * (2.0 + (dYq ? 1.0 : 0.0)) + rows * T * 4 * (1.0 + (dKw ? 1.0 : 0.0)) : 0.0) +
                 ((dKw || dVw) ? rows * N * 4 * 2 * ntiles + 2.0 * pb : 0.0));
    const int TC = words_chunk(N), parts = words_fwd_parts(P, Q), nblocks = parts * Q, n8 = (nblocks + 7) / 8;
    if (pix) {
        ZSG_LAUNCH(head_words_bwd_pix_kernel, dim3(8 * n8), dim3(256), (size_t)2 * TC * N * sizeof(float), st, dy, Y, img_idx, idx_i64, Kw, Vw, alpha, lens,
                   scale, Bi, Q, T, N, L, dYq, dKw ? ds : (float*)nullptr, parts, nblocks, n8, TC);
        ZSG_CHECK_LAUNCH("head_words_conv0_bwd(pixels)");
    }
    if (dKw || dVw) {
        ZSG_LAUNCH(head_words_dkv_part_kernel, dim3(Q * bparts * ntiles), dim3(256), (size_t)R * N * sizeof(double), st, dy, Y, img_idx, idx_i64, alpha,
                   (const float*)ds, lens, Bi, Q, T, N, L, partial, bparts, R, ntiles, dKw ? 1 : 0, dVw ? 1 : 0);
        ZSG_CHECK_LAUNCH("head_words_conv0_bwd(parts)");
        int fb = (int)(((int64_t)Q * T * N + 255) / 256);
        if (fb > 4 * ZSG_NUM_CU) fb = 4 * ZSG_NUM_CU;
        ZSG_LAUNCH(head_words_dkv_final_kernel, dim3(fb), dim3(256), 0, st, (const double*)partial, img_idx, idx_i64, lens, scale, Bi, Q, T, N, bparts, dKw,
                   dVw);
        ZSG_CHECK_LAUNCH("head_words_conv0_bwd(final)");
    }
    return 0;
}
