// gcblock.hip — global-context block of the head towers (cfg head_ctx = "gc"; GCNet, Cao et al. 2019), gfx950.  Contracts: include/zsg.h.
//
// Per head stack, query q and pyramid level l, over the rows x_p (p < P = h_l * w_l, N = 256 channels) of the post-ReLU h1, M = N / 4 = 64:
//   s_p = k . x_p                 alpha = softmax_p(s) (max subtracted)          c = sum_p alpha_p x_p
//   u = W1 c + b1                 uh = (u - mean u) / sqrt(var u + 1e-5)         (biased variance over M)
//   r = relu(gamma * uh + beta)   t = W2 r + b2                                  y_p = x_p + t
// Layout: film.hip's packed head layout [level][Q][P_l][N] — the rows of one (q, l) are contiguous, first row Q * p0_l + q * P_l.
// SHAPE.  The rows of a (q, l) are cut into CHUNKS of GC_CH = 64 rows; one block (4 waves) owns one chunk, ONE WAVE OWNS ONE ROW at a
// time (lane i holds the 16-byte channel group i: N = 256 is exactly one group per lane), a dot product is one 6-step xor butterfly.
//   forward:  gc_pool_part (per chunk: s_p, the chunk's max m, sum e, sum e x with e = exp(s - m))
//             gc_mlp_fwd   (per (q, l): combines the chunks in index order, the bottleneck MLP, t)
//             gc_add       (y = x + t)
//   backward: gc_gsum_part (per chunk: fp64 column sums of g)
//             gc_mlp_bwd   (per (q, l): dt, dr, dv, du, dc — the per-(q, l) vectors the parameter gradients are outer products of)
//             gc_a_part    (per chunk: a_p = dc . x_p and the chunk's sum alpha_p a_p)
//             gc_dx_part   (per chunk: abar, ds_p, dx_p and the chunk's fp64 sum ds_p x_p)
//             gc_final     (the seven parameter gradients: fp64 sums over (q, l) — over the chunks for dk — in index order, rounded ONCE)
// Separate launches on one stream: no tickets, flags or polling between blocks, no float atomics, no inline assembly.  Every sum's order
// is fixed by (Q, hw) alone: rows of a wave ascending, waves 0..3, chunks ascending, (l, q) ascending — the same bits on every run.
// COST at the workload's sizes (Q = 16, P = 1939, N = 256): h1 is 31.8 MB; the forward reads it twice and writes it once, the backward
// reads g three times, x twice and writes dx; all arithmetic is a few flops per byte of fp32 vector math, so no MFMA.  The two MLP
// launches have Q * nlev = 80 blocks reading W1 / W2 (64 KiB each) from L2: latency, not bandwidth.
#include <math.h>

#include "common.h"

#define GC_N 256                // channels: one 16-byte group per lane
#define GC_M 64                 // bottleneck width N / 4
#define GC_CH 64                // rows per chunk
#define GC_PLD 260              // floats per forward chunk partial: m, sum e, 2 pad, sum e x [256]

struct GcLevels {
    int nlev;
    int P[ZSG_MAX_SEG];                // rows per query of level i
    int p0[ZSG_MAX_SEG + 1];           // prefix sums of P
    int c0[ZSG_MAX_SEG + 1];           // prefix sums of the chunk counts cdiv(P, GC_CH)
};

// 0, or -1 with the error set; nblk = Q * (chunks per query)
static int gc_levels(GcLevels& L, int Q, int nlev, const int32_t* hw, const char* who) {
    memset(&L, 0, sizeof(L));
    L.nlev = nlev;
    int64_t P = 0, C = 0;
    for (int i = 0; i < nlev; ++i) {
        ZSG_REQUIRE(hw[2 * i] > 0 && hw[2 * i + 1] > 0, "%s: hw: level %d is empty", who, i);
        const int64_t p = (int64_t)hw[2 * i] * hw[2 * i + 1];
        P += p;
        ZSG_REQUIRE(p <= 0x3fffffff && P <= 0x3fffffff, "%s: hw: too many pixels", who);
        C += (p + GC_CH - 1) / GC_CH;
        L.P[i] = (int)p;
        L.p0[i + 1] = (int)P;
        L.c0[i + 1] = (int)C;
    }
    ZSG_REQUIRE((int64_t)Q * C <= 0x3fffffff && (int64_t)Q * nlev <= 0x3fffffff, "%s: Q: too many blocks", who);
    return 0;
}

// chunk block b -> level, query, chunk within the (q, l), first row of the chunk, rows in it; returns the (q, l) index l * Q + q
__device__ __forceinline__ int gc_locate(const GcLevels& L, int Q, int b, int& b0, int& nch, int64_t& row0, int& n) {
    int lv = 0;
#pragma unroll
    for (int j = 1; j < ZSG_MAX_SEG; ++j)
        if (j < L.nlev && b >= Q * L.c0[j]) lv = j;
    nch = L.c0[lv + 1] - L.c0[lv];
    const int r = b - Q * L.c0[lv], q = r / nch, ch = r - q * nch;
    b0 = Q * L.c0[lv] + q * nch;
    row0 = (int64_t)Q * L.p0[lv] + (int64_t)q * L.P[lv] + (int64_t)ch * GC_CH;
    n = L.P[lv] - ch * GC_CH;
    if (n > GC_CH) n = GC_CH;
    return lv * Q + q;
}

__device__ __forceinline__ float gc_dot4(const f32x4 a, const f32x4 b) { return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]; }

// ---- forward ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gc_pool_part_kernel(const float* __restrict__ x, const float* __restrict__ key, GcLevels L, int Q,
                                                           float* __restrict__ s_out, float* __restrict__ part) {
    __shared__ float S[GC_CH], E[GC_CH];
    __shared__ f32x4 V[4][64];
    const int b = (int)blockIdx.x, wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    int b0, nch, n;
    int64_t row0;
    gc_locate(L, Q, b, b0, nch, row0, n);
    const f32x4 k4 = *(const f32x4*)(key + 4 * lane);
    const float* xb = x + row0 * GC_N + 4 * lane;
    f32x4 v[GC_CH / 4];
#pragma unroll
    for (int j = 0; j < GC_CH / 4; ++j) {
        const int i = wave + 4 * j;                                 // (wave-uniform guard)
        if (i < n) {
            v[j] = *(const f32x4*)(xb + (int64_t)i * GC_N);
            const float a = wave_sum(gc_dot4(v[j], k4));
            if (lane == 0) {
                S[i] = a;
                if (s_out) s_out[row0 + i] = a;
            }
        } else {
            v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    __syncthreads();
    float m = S[0];
    for (int i = 1; i < n; ++i) m = fmaxf(m, S[i]);
    if ((int)threadIdx.x < n) E[threadIdx.x] = expf(S[threadIdx.x] - m);
    __syncthreads();
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < GC_CH / 4; ++j) {
        const int i = wave + 4 * j;
        if (i < n) acc += E[i] * v[j];
    }
    V[wave][lane] = acc;
    __syncthreads();
    float* pb = part + (int64_t)b * GC_PLD;
    if (wave == 0) *(f32x4*)(pb + 4 + 4 * lane) = ((V[0][lane] + V[1][lane]) + V[2][lane]) + V[3][lane];
    if (threadIdx.x == 64) {
        float se = 0.f;
        for (int i = 0; i < n; ++i) se += E[i];
        pb[0] = m;
        pb[1] = se;
    }
}

// one block per (q, l); stat (or NULL): ZSG_GC_STAT_LD floats per (q, l)
__global__ __launch_bounds__(256) void gc_mlp_fwd_kernel(const float* __restrict__ part, const float* __restrict__ W1, const float* __restrict__ b1,
                                                         const float* __restrict__ lnw, const float* __restrict__ lnb, const float* __restrict__ W2,
                                                         const float* __restrict__ b2, GcLevels L, int Q, float* __restrict__ tbuf,
                                                         float* __restrict__ stat) {
    __shared__ __attribute__((aligned(16))) float C[GC_N];
    __shared__ __attribute__((aligned(16))) float R[GC_M];
    __shared__ float U[GC_M];
    const int ql = (int)blockIdx.x, lv = ql / Q, q = ql - lv * Q;
    const int nch = L.c0[lv + 1] - L.c0[lv], b0 = Q * L.c0[lv] + q * nch;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float* pb = part + (int64_t)b0 * GC_PLD;
    float M = pb[0];
    for (int c = 1; c < nch; ++c) M = fmaxf(M, pb[(int64_t)c * GC_PLD]);
    float den = 0.f, acc = 0.f;
    for (int c = 0; c < nch; ++c) {
        const float w = expf(pb[(int64_t)c * GC_PLD] - M);
        den += w * pb[(int64_t)c * GC_PLD + 1];
        acc += w * pb[(int64_t)c * GC_PLD + 4 + tid];
    }
    const float cv = acc / den;
    C[tid] = cv;
    __syncthreads();
    const f32x4 c4 = *(const f32x4*)(C + 4 * lane);
    for (int j = wave; j < GC_M; j += 4) {
        const float a = wave_sum(gc_dot4(*(const f32x4*)(W1 + (int64_t)j * GC_N + 4 * lane), c4));
        if (lane == 0) U[j] = a + b1[j];
    }
    __syncthreads();
    float mu = 0.f;
    for (int j = 0; j < GC_M; ++j) mu += U[j];
    mu *= 1.0f / GC_M;
    float var = 0.f;
    for (int j = 0; j < GC_M; ++j) var += (U[j] - mu) * (U[j] - mu);
    var *= 1.0f / GC_M;
    const float rstd = 1.0f / sqrtf(var + 1e-5f);
    float* st = stat ? stat + (int64_t)ql * ZSG_GC_STAT_LD : nullptr;
    if (tid < GC_M) {
        const float uh = (U[tid] - mu) * rstd;
        const float r = fmaxf(lnw[tid] * uh + lnb[tid], 0.f);
        R[tid] = r;
        if (st) {
            st[ZSG_GC_STAT_UHAT + tid] = uh;
            st[ZSG_GC_STAT_R + tid] = r;
        }
    }
    if (st) {
        st[ZSG_GC_STAT_C + tid] = cv;
        if (tid == 0) {
            st[ZSG_GC_STAT_MAX] = M;
            st[ZSG_GC_STAT_DEN] = den;
            st[ZSG_GC_STAT_VAR] = var;
            st[ZSG_GC_STAT_RSTD] = rstd;
        }
    }
    __syncthreads();
    float t = 0.f;
    const float* wr = W2 + (int64_t)tid * GC_M;
#pragma unroll
    for (int j = 0; j < GC_M; j += 4) t += gc_dot4(*(const f32x4*)(wr + j), *(const f32x4*)(R + j));
    tbuf[(int64_t)ql * GC_N + tid] = t + b2[tid];
}

// y = x + t of the row's (q, l): one wave per row
__global__ __launch_bounds__(256) void gc_add_kernel(const float* __restrict__ x, const float* __restrict__ tbuf, GcLevels L, int Q, int64_t rows,
                                                     float* __restrict__ y) {
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
        int lv = 0;
#pragma unroll
        for (int j = 1; j < ZSG_MAX_SEG; ++j)
            if (j < L.nlev && row >= (int64_t)Q * L.p0[j]) lv = j;
        const int q = (int)((row - (int64_t)Q * L.p0[lv]) / L.P[lv]);
        const f32x4 t = *(const f32x4*)(tbuf + ((int64_t)lv * Q + q) * GC_N + 4 * lane);
        *(f32x4*)(y + row * GC_N + 4 * lane) = *(const f32x4*)(x + row * GC_N + 4 * lane) + t;
    }
}

static inline int64_t gc_al16(int64_t b) { return (b + 15) & ~(int64_t)15; }

static int gc_check(const char* who, int32_t Q, int32_t nlev, const int32_t* hw, int32_t N) {
    ZSG_REQUIRE(hw, "%s: hw is NULL", who);
    ZSG_REQUIRE(N == GC_N, "%s: N = %d (the block is built for N = %d)", who, N, GC_N);
    ZSG_REQUIRE(nlev >= 1 && nlev <= ZSG_MAX_SEG, "%s: nlev = %d outside [1, %d]", who, nlev, ZSG_MAX_SEG);
    ZSG_REQUIRE(Q >= 1, "%s: Q = %d", who, Q);
    return 0;
}
#define GC_PTR(who, p) ZSG_REQUIRE((p) != nullptr, "%s: %s is NULL", who, #p)
#define GC_AL16(who, p) ZSG_REQUIRE(((uintptr_t)(p) & 15) == 0, "%s: %s is not 16-byte aligned", who, #p)

extern "C" int64_t zsg_head_gc_fwd_ws_bytes(int32_t Q, int32_t nlev, const int32_t* hw, int32_t N) {
    GcLevels L;
    if (gc_check("head_gc_fwd_ws_bytes", Q, nlev, hw, N) || gc_levels(L, Q, nlev, hw, "head_gc_fwd_ws_bytes")) return -1;
    return gc_al16((int64_t)Q * L.c0[nlev] * GC_PLD * 4) + (int64_t)Q * nlev * GC_N * 4;
}

extern "C" int zsg_head_gc_fwd(const float* x, const float* key, const float* W1, const float* b1, const float* lnw, const float* lnb, const float* W2,
                               const float* b2, int32_t Q, int32_t nlev, const int32_t* hw, int32_t N, float* y, float* s, float* stat, void* ws,
                               int64_t ws_bytes, void* stream) {
    const char* who = "head_gc_fwd";
    GC_PTR(who, x);
    GC_PTR(who, key);
    GC_PTR(who, W1);
    GC_PTR(who, b1);
    GC_PTR(who, lnw);
    GC_PTR(who, lnb);
    GC_PTR(who, W2);
    GC_PTR(who, b2);
    GC_PTR(who, y);
    GC_PTR(who, ws);
    if (gc_check(who, Q, nlev, hw, N)) return -1;
    ZSG_REQUIRE((s == nullptr) == (stat == nullptr), "%s: s and stat are saved together (training) or not at all (eval)", who);
    GC_AL16(who, x);
    GC_AL16(who, key);
    GC_AL16(who, W1);
    GC_AL16(who, W2);
    GC_AL16(who, y);
    GC_AL16(who, ws);
    ZSG_REQUIRE((((uintptr_t)b1 | (uintptr_t)lnw | (uintptr_t)lnb | (uintptr_t)b2 | (uintptr_t)s | (uintptr_t)stat) & 3) == 0, "%s: alignment", who);
    GcLevels L;
    if (gc_levels(L, Q, nlev, hw, who)) return -1;
    const int nblk = Q * L.c0[nlev], nql = Q * nlev;
    const int64_t pbytes = gc_al16((int64_t)nblk * GC_PLD * 4), need = pbytes + (int64_t)nql * GC_N * 4;
    ZSG_REQUIRE(ws_bytes >= need, "%s: ws_bytes = %lld, %lld needed (zsg_head_gc_fwd_ws_bytes)", who, (long long)ws_bytes, (long long)need);
    float* part = (float*)ws;
    float* tbuf = (float*)((char*)ws + pbytes);
    const int64_t rows = (int64_t)Q * L.p0[nlev];
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("head_gc_fwd", st, 6.0 * rows * GC_N + 4.0 * nql * GC_N * GC_M, 12.0 * rows * GC_N + 8.0 * nql * GC_N * GC_M);
    ZSG_LAUNCH(gc_pool_part_kernel, dim3(nblk), dim3(256), 0, st, x, key, L, Q, s, part);
    ZSG_CHECK_LAUNCH("head_gc_fwd(pool)");
    ZSG_LAUNCH(gc_mlp_fwd_kernel, dim3(nql), dim3(256), 0, st, (const float*)part, W1, b1, lnw, lnb, W2, b2, L, Q, tbuf, stat);
    ZSG_CHECK_LAUNCH("head_gc_fwd(mlp)");
    int ab = (int)((rows + 3) / 4 > 8 * ZSG_NUM_CU ? 8 * ZSG_NUM_CU : (rows + 3) / 4);
    ZSG_LAUNCH(gc_add_kernel, dim3(ab), dim3(256), 0, st, x, (const float*)tbuf, L, Q, rows, y);
    ZSG_CHECK_LAUNCH("head_gc_fwd(add)");
    return 0;
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
// the 4 waves' fp64 channel sums of one chunk, added in wave order, to out[256]
__device__ __forceinline__ void gc_reduce_d(double (*D)[GC_N], const double* a, int wave, int lane, double* __restrict__ out) {
#pragma unroll
    for (int e = 0; e < 4; ++e) D[wave][4 * lane + e] = a[e];
    __syncthreads();
    const int t = (int)threadIdx.x;
    out[t] = ((D[0][t] + D[1][t]) + D[2][t]) + D[3][t];
}

__global__ __launch_bounds__(256) void gc_gsum_part_kernel(const float* __restrict__ g, GcLevels L, int Q, double* __restrict__ dtp) {
    __shared__ double D[4][GC_N];
    const int b = (int)blockIdx.x, wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    int b0, nch, n;
    int64_t row0;
    gc_locate(L, Q, b, b0, nch, row0, n);
    const float* gb = g + row0 * GC_N + 4 * lane;
    double a[4] = {0., 0., 0., 0.};
    for (int i = wave; i < n; i += 4) {
        const f32x4 v = *(const f32x4*)(gb + (int64_t)i * GC_N);
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] += (double)v[e];
    }
    gc_reduce_d(D, a, wave, lane, dtp + (int64_t)b * GC_N);
}

__global__ __launch_bounds__(256) void gc_mlp_bwd_kernel(const double* __restrict__ dtp, const float* __restrict__ stat, const float* __restrict__ W1,
                                                         const float* __restrict__ lnw, const float* __restrict__ W2, GcLevels L, int Q,
                                                         double* __restrict__ dtd, float* __restrict__ dc, float* __restrict__ dv,
                                                         float* __restrict__ du) {
    __shared__ float DT[GC_N], PR[4][GC_M], DH[GC_M], UH[GC_M], DU[GC_M];
    const int ql = (int)blockIdx.x, lv = ql / Q, q = ql - lv * Q;
    const int nch = L.c0[lv + 1] - L.c0[lv], b0 = Q * L.c0[lv] + q * nch;
    const int tid = (int)threadIdx.x, part = tid >> 6, j = tid & 63;
    const float* st = stat + (int64_t)ql * ZSG_GC_STAT_LD;
    double s = 0.;
    for (int c = 0; c < nch; ++c) s += dtp[(int64_t)(b0 + c) * GC_N + tid];
    dtd[(int64_t)ql * GC_N + tid] = s;
    DT[tid] = (float)s;
    __syncthreads();
    float a = 0.f;
    for (int n = part * 64; n < part * 64 + 64; ++n) a += W2[(int64_t)n * GC_M + j] * DT[n];        // dr = W2^T dt
    PR[part][j] = a;
    __syncthreads();
    if (tid < GC_M) {
        const float dr = ((PR[0][tid] + PR[1][tid]) + PR[2][tid]) + PR[3][tid];
        const float v = st[ZSG_GC_STAT_R + tid] > 0.f ? dr : 0.f;
        dv[(int64_t)ql * GC_M + tid] = v;
        DH[tid] = v * lnw[tid];
        UH[tid] = st[ZSG_GC_STAT_UHAT + tid];
    }
    __syncthreads();
    float m1 = 0.f, m2 = 0.f;
    for (int i = 0; i < GC_M; ++i) {
        m1 += DH[i];
        m2 += DH[i] * UH[i];
    }
    m1 *= 1.0f / GC_M;
    m2 *= 1.0f / GC_M;
    if (tid < GC_M) {
        const float d = ((DH[tid] - m1) - UH[tid] * m2) * st[ZSG_GC_STAT_RSTD];
        DU[tid] = d;
        du[(int64_t)ql * GC_M + tid] = d;
    }
    __syncthreads();
    float c = 0.f;
    for (int i = 0; i < GC_M; ++i) c += W1[(int64_t)i * GC_N + tid] * DU[i];                         // dc = W1^T du
    dc[(int64_t)ql * GC_N + tid] = c;
}

__global__ __launch_bounds__(256) void gc_a_part_kernel(const float* __restrict__ x, const float* __restrict__ s, const float* __restrict__ stat,
                                                        const float* __restrict__ dc, GcLevels L, int Q, float* __restrict__ abuf,
                                                        float* __restrict__ apart) {
    __shared__ float AL[GC_CH];
    const int b = (int)blockIdx.x, wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    int b0, nch, n;
    int64_t row0;
    const int ql = gc_locate(L, Q, b, b0, nch, row0, n);
    const float* st = stat + (int64_t)ql * ZSG_GC_STAT_LD;
    const float M = st[ZSG_GC_STAT_MAX], den = st[ZSG_GC_STAT_DEN];
    const f32x4 d4 = *(const f32x4*)(dc + (int64_t)ql * GC_N + 4 * lane);
    const float* xb = x + row0 * GC_N + 4 * lane;
    for (int i = wave; i < n; i += 4) {
        const float a = wave_sum(gc_dot4(*(const f32x4*)(xb + (int64_t)i * GC_N), d4));
        if (lane == 0) {
            abuf[row0 + i] = a;
            AL[i] = (expf(s[row0 + i] - M) / den) * a;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int i = 0; i < n; ++i) t += AL[i];
        apart[b] = t;
    }
}

__global__ __launch_bounds__(256) void gc_dx_part_kernel(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ s,
                                                         const float* __restrict__ stat, const float* __restrict__ key, const float* __restrict__ dc,
                                                         const float* __restrict__ abuf, const float* __restrict__ apart, GcLevels L, int Q,
                                                         float* __restrict__ dx, double* __restrict__ dkp) {
    __shared__ double D[4][GC_N];
    const int b = (int)blockIdx.x, wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    int b0, nch, n;
    int64_t row0;
    const int ql = gc_locate(L, Q, b, b0, nch, row0, n);
    const float* st = stat + (int64_t)ql * ZSG_GC_STAT_LD;
    const float M = st[ZSG_GC_STAT_MAX], den = st[ZSG_GC_STAT_DEN];
    float abar = 0.f;
    for (int c = 0; c < nch; ++c) abar += apart[b0 + c];
    const f32x4 d4 = *(const f32x4*)(dc + (int64_t)ql * GC_N + 4 * lane);
    const f32x4 k4 = *(const f32x4*)(key + 4 * lane);
    double a[4] = {0., 0., 0., 0.};
    for (int i = wave; i < n; i += 4) {
        const int64_t row = row0 + i;
        const float al = expf(s[row] - M) / den;
        const float ds = al * (abuf[row] - abar);
        if (dx) {
            const f32x4 gv = *(const f32x4*)(g + row * GC_N + 4 * lane);
            *(f32x4*)(dx + row * GC_N + 4 * lane) = (gv + al * d4) + ds * k4;
        }
        if (dkp) {
            const f32x4 xv = *(const f32x4*)(x + row * GC_N + 4 * lane);
#pragma unroll
            for (int e = 0; e < 4; ++e) a[e] = fma((double)ds, (double)xv[e], a[e]);
        }
    }
    if (dkp) gc_reduce_d(D, a, wave, lane, dkp + (int64_t)b * GC_N);          // (block-uniform)
}

// The seven parameter gradients, one thread per element: fp64 sums over the (q, l) vectors in index order (dk: over the chunk partials),
// every term one fma of an exact fp32 x fp32 product, rounded once.  acc: out += (the flat gradient buffer's convention), else out =.
__global__ __launch_bounds__(256) void gc_final_kernel(const double* __restrict__ dtd, const double* __restrict__ dkp, const float* __restrict__ stat,
                                                       const float* __restrict__ dv, const float* __restrict__ du, int nql, int nblk,
                                                       float* __restrict__ dkey, float* __restrict__ dW1, float* __restrict__ db1,
                                                       float* __restrict__ dlnw, float* __restrict__ dlnb, float* __restrict__ dW2,
                                                       float* __restrict__ db2, int acc) {
    const int NW = GC_N * GC_M;
    const int total = GC_N + NW + 3 * GC_M + NW + GC_N;
    int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= total) return;
    float* out = nullptr;
    double s = 0.;
    if (i < GC_N) {                                     // dk[n]
        if (dkey) {
            out = dkey + i;
            for (int b = 0; b < nblk; ++b) s += dkp[(int64_t)b * GC_N + i];
        }
    } else if ((i -= GC_N) < NW) {                      // dW1[j][n] = sum du[j] c[n]
        if (dW1) {
            out = dW1 + i;
            const int j = i / GC_N, n = i - j * GC_N;
            for (int k = 0; k < nql; ++k) s = fma((double)du[(int64_t)k * GC_M + j], (double)stat[(int64_t)k * ZSG_GC_STAT_LD + ZSG_GC_STAT_C + n], s);
        }
    } else if ((i -= NW) < GC_M) {                      // db1[j] = sum du[j]
        if (db1) {
            out = db1 + i;
            for (int k = 0; k < nql; ++k) s += (double)du[(int64_t)k * GC_M + i];
        }
    } else if ((i -= GC_M) < GC_M) {                    // dgamma[j] = sum dv[j] uh[j]
        if (dlnw) {
            out = dlnw + i;
            for (int k = 0; k < nql; ++k) s = fma((double)dv[(int64_t)k * GC_M + i], (double)stat[(int64_t)k * ZSG_GC_STAT_LD + ZSG_GC_STAT_UHAT + i], s);
        }
    } else if ((i -= GC_M) < GC_M) {                    // dbeta[j] = sum dv[j]
        if (dlnb) {
            out = dlnb + i;
            for (int k = 0; k < nql; ++k) s += (double)dv[(int64_t)k * GC_M + i];
        }
    } else if ((i -= GC_M) < NW) {                      // dW2[n][j] = sum dt[n] r[j]      (dt: the fp32 value the chain used)
        if (dW2) {
            out = dW2 + i;
            const int n = i / GC_M, j = i - n * GC_M;
            for (int k = 0; k < nql; ++k)
                s = fma((double)(float)dtd[(int64_t)k * GC_N + n], (double)stat[(int64_t)k * ZSG_GC_STAT_LD + ZSG_GC_STAT_R + j], s);
        }
    } else {                                            // db2[n] = sum over every pixel of g, fp64 throughout
        i -= NW;
        if (db2) {
            out = db2 + i;
            for (int k = 0; k < nql; ++k) s += dtd[(int64_t)k * GC_N + i];
        }
    }
    if (out) *out = acc ? *out + (float)s : (float)s;
}

struct GcBwdWs {
    int64_t dtp, dtd, dkp, dc, dv, du, a, apart, total;
};
static GcBwdWs gc_bwd_ws(const GcLevels& L, int Q) {
    const int64_t nblk = (int64_t)Q * L.c0[L.nlev], nql = (int64_t)Q * L.nlev, rows = (int64_t)Q * L.p0[L.nlev];
    GcBwdWs w;
    int64_t o = 0;
    w.dtp = o, o += nblk * GC_N * 8;
    w.dtd = o, o += nql * GC_N * 8;
    w.dkp = o, o += nblk * GC_N * 8;
    w.dc = o, o += nql * GC_N * 4;
    w.dv = o, o += nql * GC_M * 4;
    w.du = o, o += nql * GC_M * 4;
    w.a = o, o += gc_al16(rows * 4);
    w.apart = o, o += gc_al16(nblk * 4);
    w.total = o;
    return w;
}

extern "C" int64_t zsg_head_gc_bwd_ws_bytes(int32_t Q, int32_t nlev, const int32_t* hw, int32_t N) {
    GcLevels L;
    if (gc_check("head_gc_bwd_ws_bytes", Q, nlev, hw, N) || gc_levels(L, Q, nlev, hw, "head_gc_bwd_ws_bytes")) return -1;
    return gc_bwd_ws(L, Q).total;
}

extern "C" int zsg_head_gc_bwd(const float* g, const float* x, const float* s, const float* stat, const float* key, const float* W1, const float* lnw,
                               const float* W2, int32_t Q, int32_t nlev, const int32_t* hw, int32_t N, float* dx, float* dkey, float* dW1, float* db1,
                               float* dlnw, float* dlnb, float* dW2, float* db2, int32_t accumulate, void* ws, int64_t ws_bytes, void* stream) {
    const char* who = "head_gc_bwd";
    GC_PTR(who, g);
    GC_PTR(who, x);
    GC_PTR(who, s);
    GC_PTR(who, stat);
    GC_PTR(who, key);
    GC_PTR(who, W1);
    GC_PTR(who, lnw);
    GC_PTR(who, W2);
    GC_PTR(who, ws);
    if (gc_check(who, Q, nlev, hw, N)) return -1;
    const bool params = dkey || dW1 || db1 || dlnw || dlnb || dW2 || db2;
    ZSG_REQUIRE(dx || params, "%s: no output (dx and the seven gradients are all NULL)", who);
    GC_AL16(who, g);
    GC_AL16(who, x);
    GC_AL16(who, key);
    GC_AL16(who, W1);
    GC_AL16(who, W2);
    GC_AL16(who, dx);
    GC_AL16(who, ws);
    ZSG_REQUIRE((((uintptr_t)s | (uintptr_t)stat | (uintptr_t)lnw | (uintptr_t)dkey | (uintptr_t)dW1 | (uintptr_t)db1 | (uintptr_t)dlnw | (uintptr_t)dlnb |
                  (uintptr_t)dW2 | (uintptr_t)db2) & 3) == 0,
                "%s: alignment", who);
    GcLevels L;
    if (gc_levels(L, Q, nlev, hw, who)) return -1;
    const GcBwdWs w = gc_bwd_ws(L, Q);
    ZSG_REQUIRE(ws_bytes >= w.total, "%s: ws_bytes = %lld, %lld needed (zsg_head_gc_bwd_ws_bytes)", who, (long long)ws_bytes, (long long)w.total);
    char* base = (char*)ws;
    double* dtp = (double*)(base + w.dtp);
    double* dtd = (double*)(base + w.dtd);
    double* dkp = (double*)(base + w.dkp);
    float* dc = (float*)(base + w.dc);
    float* dv = (float*)(base + w.dv);
    float* du = (float*)(base + w.du);
    float* abuf = (float*)(base + w.a);
    float* apart = (float*)(base + w.apart);
    const int nblk = Q * L.c0[nlev], nql = Q * nlev;
    const double rows = (double)Q * L.p0[nlev];
    const bool pix = dx || dkey;           // a_p / abar / ds_p feed dx and dk only
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("head_gc_bwd", st, rows * GC_N * (1.0 + (pix ? 8.0 : 0.0)) + 6.0 * nql * GC_N * GC_M,
             rows * GC_N * 4 * (1.0 + (pix ? 1.0 : 0.0) + (dx ? 2.0 : 0.0) + (dkey ? 1.0 : 0.0)) + 8.0 * nql * GC_N * GC_M);
    ZSG_LAUNCH(gc_gsum_part_kernel, dim3(nblk), dim3(256), 0, st, g, L, Q, dtp);
    ZSG_CHECK_LAUNCH("head_gc_bwd(gsum)");
    ZSG_LAUNCH(gc_mlp_bwd_kernel, dim3(nql), dim3(256), 0, st, (const double*)dtp, stat, W1, lnw, W2, L, Q, dtd, dc, dv, du);
    ZSG_CHECK_LAUNCH("head_gc_bwd(mlp)");
    if (pix) {
        ZSG_LAUNCH(gc_a_part_kernel, dim3(nblk), dim3(256), 0, st, x, s, stat, (const float*)dc, L, Q, abuf, apart);
        ZSG_CHECK_LAUNCH("head_gc_bwd(a)");
        ZSG_LAUNCH(gc_dx_part_kernel, dim3(nblk), dim3(256), 0, st, g, x, s, stat, key, (const float*)dc, (const float*)abuf, (const float*)apart, L, Q, dx,
                   dkey ? dkp : (double*)nullptr);
        ZSG_CHECK_LAUNCH("head_gc_bwd(dx)");
    }
    if (params) {
        const int total = GC_N + 2 * GC_N * GC_M + 3 * GC_M + GC_N;
        ZSG_LAUNCH(gc_final_kernel, dim3((total + 255) / 256), dim3(256), 0, st, (const double*)dtd, (const double*)dkp, stat, (const float*)dv,
                   (const float*)du, nql, nblk, dkey, dW1, db1, dlnw, dlnb, dW2, db2, accumulate ? 1 : 0);
        ZSG_CHECK_LAUNCH("head_gc_bwd(final)");
    }
    return 0;
}
