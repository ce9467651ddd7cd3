// lstm_seq.hip — the query encoder's full-sequence recurrence and the pooling of its outputs (cfg lang_pool = final / mean / attn).
// zsg_lstm_seq_fwd / zsg_lstm_seq_bwd are lstm.hip's two kernels (one workgroup per query, 4H threads, one gate row per thread, the
// recurrent weights in registers up to H = 128) with a walk direction and the hidden state of EVERY step as an output: reverse = 1
// consumes x[len-1], x[len-2], .., x[0], and everything a step saves is stored at its TOKEN's position, so the weight gradients stay
// plain GEMMs over the token-aligned [B*T] rows (zsg_conv_wgrad / zsg_colsum).  zsg_lang_pool_fwd / _bwd reduce the padded output
// o_t = [f_t | r_t] over the valid steps of each query (mean, or softmax(w . o_t) attention), one workgroup per query.
// No float atomics anywhere in this file: every sum runs in a fixed order, the same inputs give the same bits.
// The arithmetic of the cell step is lstm.hip's, expression for expression: reverse = 0 reproduces zsg_lstm_fwd / zsg_lstm_bwd bit for bit.
#include "common.h"

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// rank of sample b in a stable descending sort of the lengths (lstm.hip's sorted_rank; reference mdl.py:309)
__device__ __forceinline__ int sorted_rank(const float* __restrict__ qlens, int B, int b) {
    const float me = qlens[b];
    int r = 0;
    for (int j = 0; j < B; ++j) {
        const float o = qlens[j];
        r += (o > me) || (o == me && j < b);
    }
    return r;
}

__device__ __forceinline__ int clamped_len(const float* __restrict__ lens, int b, int T) {
    int len = lens ? (int)lens[b] : 1;
    return len < 0 ? 0 : (len > T ? T : len);
}

template <int H, bool REG>
__global__ __launch_bounds__(4 * H) void lstm_seq_fwd_kernel(const float* __restrict__ gin, const float* __restrict__ w_hh,
                                                             const float* __restrict__ b_hh, const float* __restrict__ h0,
                                                             const float* __restrict__ c0, const float* __restrict__ qlens,
                                                             const float* __restrict__ lens, int B, int T, int reverse,
                                                             float* __restrict__ gates, float* __restrict__ cst, float* __restrict__ hprev,
                                                             float* __restrict__ hseq, int hs_ld, int hs_off, float* __restrict__ we,
                                                             int we_ld, int we_off) {
    __shared__ __attribute__((aligned(16))) float hs[H];
    __shared__ float gs[4 * H];
    const int b = blockIdx.x;
    const int j = threadIdx.x;          // gate row
    const int rank = sorted_rank(qlens, B, b);
    const int len = clamped_len(lens, b, T);
    float w[REG ? H : 1];
    if (REG) {
#pragma unroll
        for (int k = 0; k < H; k += 4) {
            const f32x4 v = *(const f32x4*)(w_hh + (size_t)j * H + k);
            w[k] = v[0];
            w[k + 1] = v[1];
            w[k + 2] = v[2];
            w[k + 3] = v[3];
        }
    }
    const float bias = b_hh[j];
    float c = 0.f;
    if (j < H) {
        hs[j] = h0[rank * H + j];
        c = c0[rank * H + j];
    }
    // the padded output is exactly 0 behind the query's length
    if (hseq && j < H)
        for (int t = len; t < T; ++t) hseq[((size_t)b * T + t) * hs_ld + hs_off + j] = 0.f;
    __syncthreads();
    for (int s = 0; s < len; ++s) {
        const int t = reverse ? len - 1 - s : s;          // the token this step consumes
        float pre = gin[((size_t)b * T + t) * 4 * H + j] + bias;
        if (REG) {
#pragma unroll
            for (int k = 0; k < H; k += 4) {
                const f32x4 hv = *(const f32x4*)(hs + k);
                pre += w[k] * hv[0] + w[k + 1] * hv[1] + w[k + 2] * hv[2] + w[k + 3] * hv[3];
            }
        } else {
            // (partially unrolled for the reason lstm.hip gives: fully unrolled, hipcc hoists all H / 4 row loads and spills)
#pragma unroll 8
            for (int k = 0; k < H; k += 4) {
                const f32x4 hv = *(const f32x4*)(hs + k);
                const f32x4 wv = *(const f32x4*)(w_hh + (size_t)j * H + k);
                pre += wv[0] * hv[0] + wv[1] * hv[1] + wv[2] * hv[2] + wv[3] * hv[3];
            }
        }
        const float act = (j >= 2 * H && j < 3 * H) ? tanhf(pre) : sigmoidf_(pre);
        gs[j] = act;
        gates[((size_t)b * T + t) * 4 * H + j] = act;
        if (j < H) hprev[((size_t)b * T + t) * H + j] = hs[j];
        __syncthreads();
        if (j < H) {
            c = gs[H + j] * c + gs[j] * gs[2 * H + j];
            const float h = gs[3 * H + j] * tanhf(c);
            cst[((size_t)b * T + t) * H + j] = c;
            hs[j] = h;
            if (hseq) hseq[((size_t)b * T + t) * hs_ld + hs_off + j] = h;
        }
        __syncthreads();
    }
    if (we && j < H) we[(size_t)b * we_ld + we_off + j] = hs[j];
}

template <int H>
__global__ __launch_bounds__(4 * H) void lstm_seq_bwd_kernel(const float* __restrict__ dwe, int we_ld, int we_off,
                                                             const float* __restrict__ dhseq, int hs_ld, int hs_off,
                                                             const float* __restrict__ w_hh, const float* __restrict__ gates,
                                                             const float* __restrict__ cst, const float* __restrict__ c0,
                                                             const float* __restrict__ qlens, const float* __restrict__ lens, int B, int T,
                                                             int reverse, float* __restrict__ dgates) {
    __shared__ float dpre[4 * H];
    __shared__ float part[4][H];
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int u = tid % H, q = tid / H;
    const int rank = sorted_rank(qlens, B, b);
    const int len = clamped_len(lens, b, T);
    float dh = 0.f, dc = 0.f;
    if (q == 0 && dwe) dh = dwe[(size_t)b * we_ld + we_off + u];
    for (int t = T - 1; t >= len; --t) dgates[((size_t)b * T + t) * 4 * H + tid] = 0.f;
    for (int s = len - 1; s >= 0; --s) {
        const int t = reverse ? len - 1 - s : s;
        if (q == 0) {
            if (dhseq) dh += dhseq[((size_t)b * T + t) * hs_ld + hs_off + u];
            const float* g = gates + ((size_t)b * T + t) * 4 * H;
            const float gi = g[u], gf = g[H + u], gg = g[2 * H + u], go = g[3 * H + u];
            const float c = cst[((size_t)b * T + t) * H + u];
            const int tp = reverse ? t + 1 : t - 1;          // the token of the walk's previous step
            const float cp = s > 0 ? cst[((size_t)b * T + tp) * H + u] : c0[rank * H + u];
            const float tc = tanhf(c);
            const float d_o = dh * tc;
            dc += dh * go * (1.f - tc * tc);
            const float d_i = dc * gg, d_g = dc * gi, d_f = dc * cp;
            dpre[u] = d_i * gi * (1.f - gi);
            dpre[H + u] = d_f * gf * (1.f - gf);
            dpre[2 * H + u] = d_g * (1.f - gg * gg);
            dpre[3 * H + u] = d_o * go * (1.f - go);
            dc = dc * gf;
        }
        __syncthreads();
        dgates[((size_t)b * T + t) * 4 * H + tid] = dpre[tid];
        float sum = 0.f;
        for (int k = 0; k < H; ++k) sum += w_hh[(size_t)(q * H + k) * H + u] * dpre[q * H + k];
        part[q][u] = sum;
        __syncthreads();
        if (q == 0) dh = part[0][u] + part[1][u] + part[2][u] + part[3][u];
        __syncthreads();
    }
}

// ---- pooling over the valid steps -------------------------------------------------------------------------------------------------
#define POOL_THREADS 256

// dot[t] = a . hseq[b][t][:] for t < len, one wave per step (lanes stride over D, butterfly sum: a fixed order), into LDS
__device__ __forceinline__ void pool_step_dots(const float* __restrict__ a, const float* __restrict__ o, int len, int D, float* __restrict__ dot) {
    const int wave = threadIdx.x / ZSG_WAVE, lane = threadIdx.x % ZSG_WAVE;
    for (int t = wave; t < len; t += POOL_THREADS / ZSG_WAVE) {
        float s = 0.f;
        for (int d = lane; d < D; d += ZSG_WAVE) s += a[d] * o[(size_t)t * D + d];
        s = wave_sum(s);
        if (lane == 0) dot[t] = s;
    }
}

// dynamic LDS: T floats
__global__ __launch_bounds__(POOL_THREADS) void lang_pool_fwd_kernel(const float* __restrict__ hseq, const float* __restrict__ lens,
                                                                     const float* __restrict__ w, int attn, int T, int D,
                                                                     float* __restrict__ we, float* __restrict__ alpha) {
    extern __shared__ __attribute__((aligned(16))) float sc[];          // scores, then weights
    const int b = blockIdx.x;
    const int len = clamped_len(lens, b, T);
    const float* o = hseq + (size_t)b * T * D;
    if (attn) {
        pool_step_dots(w, o, len, D, sc);
        __syncthreads();
        if (threadIdx.x == 0 && len > 0) {
            float m = sc[0];
            for (int t = 1; t < len; ++t) m = fmaxf(m, sc[t]);
            float den = 0.f;
            for (int t = 0; t < len; ++t) {
                sc[t] = expf(sc[t] - m);
                den += sc[t];
            }
            for (int t = 0; t < len; ++t) sc[t] = sc[t] / den;
        }
        __syncthreads();
        if (alpha)
            for (int t = threadIdx.x; t < T; t += POOL_THREADS) alpha[(size_t)b * T + t] = t < len ? sc[t] : 0.f;
    }
    for (int d = threadIdx.x; d < D; d += POOL_THREADS) {
        float s = 0.f;
        if (attn) {
            for (int t = 0; t < len; ++t) s += sc[t] * o[(size_t)t * D + d];
        } else {
            for (int t = 0; t < len; ++t) s += o[(size_t)t * D + d];
            if (len > 0) s = s / (float)len;
        }
        we[(size_t)b * D + d] = s;
    }
}

// dynamic LDS: T floats
__global__ __launch_bounds__(POOL_THREADS) void lang_pool_bwd_kernel(const float* __restrict__ dwe, const float* __restrict__ hseq,
                                                                     const float* __restrict__ lens, const float* __restrict__ w,
                                                                     const float* __restrict__ alpha, int attn, int T, int D,
                                                                     float* __restrict__ dhseq, float* __restrict__ ds) {
    extern __shared__ __attribute__((aligned(16))) float sc[];          // d(alpha), then d(scores)
    const int b = blockIdx.x;
    const int len = clamped_len(lens, b, T);
    const float* o = hseq + (size_t)b * T * D;
    const float* g = dwe + (size_t)b * D;
    float* dx = dhseq + (size_t)b * T * D;
    if (attn) {
        const float* al = alpha + (size_t)b * T;
        pool_step_dots(g, o, len, D, sc);
        __syncthreads();
        if (threadIdx.x == 0) {
            float dot = 0.f;
            for (int t = 0; t < len; ++t) dot += al[t] * sc[t];
            for (int t = 0; t < len; ++t) sc[t] = al[t] * (sc[t] - dot);
        }
        __syncthreads();
        if (ds)
            for (int t = threadIdx.x; t < T; t += POOL_THREADS) ds[(size_t)b * T + t] = t < len ? sc[t] : 0.f;
        for (int d = threadIdx.x; d < D; d += POOL_THREADS) {
            const float gd = g[d], wd = w[d];
            for (int t = 0; t < T; ++t) dx[(size_t)t * D + d] = t < len ? al[t] * gd + sc[t] * wd : 0.f;
        }
    } else {
        for (int d = threadIdx.x; d < D; d += POOL_THREADS) {
            const float gd = len > 0 ? g[d] / (float)len : 0.f;
            for (int t = 0; t < T; ++t) dx[(size_t)t * D + d] = t < len ? gd : 0.f;
        }
    }
}

// dw[d] (+)= sum_r ds[r] * hseq[r][d] over the R = B*T rows (ds and hseq are 0 on the padded rows).  A block owns 16 columns: its 16
// row groups each add the rows r = g, g + 16, .. in ascending order, then one thread per column adds the 16 partial sums in group order —
// a fixed order whatever the launch's timing (a single serial chain over the rows measured 91 us at B*T = 320: latency, not bytes).
#define POOL_WG_COLS 16
#define POOL_WG_GROUPS (POOL_THREADS / POOL_WG_COLS)
__global__ __launch_bounds__(POOL_THREADS) void lang_pool_wgrad_kernel(const float* __restrict__ ds, const float* __restrict__ hseq, int R,
                                                                       int D, float* __restrict__ dw, int accumulate) {
    __shared__ float part[POOL_WG_GROUPS][POOL_WG_COLS];
    const int c = threadIdx.x % POOL_WG_COLS, g = threadIdx.x / POOL_WG_COLS;
    const int d = blockIdx.x * POOL_WG_COLS + c;
    float s = 0.f;
    if (d < D) {
#pragma unroll 4
        for (int r = g; r < R; r += POOL_WG_GROUPS) s += ds[r] * hseq[(size_t)r * D + d];
    }
    part[g][c] = s;
    __syncthreads();
    if (g == 0 && d < D) {
        float t = part[0][c];
#pragma unroll
        for (int k = 1; k < POOL_WG_GROUPS; ++k) t += part[k][c];
        dw[d] = accumulate ? dw[d] + t : t;
    }
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------------------
extern "C" int zsg_lstm_seq_fwd(const float* gin, const float* w_hh, const float* b_hh, const float* h0, const float* c0,
                                const float* qlens_rank, const float* lens, int32_t B, int32_t T, int32_t H, int32_t reverse, float* gates,
                                float* cst, float* hprev, float* hseq, int32_t hs_ld, int32_t hs_off, float* we, int32_t we_ld,
                                int32_t we_off, void* stream) {
    ZSG_REQUIRE(gin && w_hh && b_hh && h0 && c0 && qlens_rank && gates && cst && hprev && B > 0 && T > 0, "lstm_seq_fwd: null argument");
    ZSG_REQUIRE(hseq || we, "lstm_seq_fwd: null argument (one of hseq / we is required)");
    ZSG_REQUIRE(!hseq || (hs_off >= 0 && hs_ld >= hs_off + H), "lstm_seq_fwd: window [%d, %d + %d) outside rows of %d", hs_off, hs_off, H, hs_ld);
    ZSG_REQUIRE(!we || (we_off >= 0 && we_ld >= we_off + H), "lstm_seq_fwd: window [%d, %d + %d) outside rows of %d", we_off, we_off, H, we_ld);
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("lstm_seq_fwd", st, 2.0 * B * T * 4 * H * H, 0);
#define ZSG_LSTM_SEQ_FWD(HH, REG)                                                                                                      \
    ZSG_LAUNCH((lstm_seq_fwd_kernel<HH, REG>), dim3(B), dim3(4 * HH), 0, st, gin, w_hh, b_hh, h0, c0, qlens_rank, lens, B, T, \
               reverse != 0, gates, cst, hprev, hseq, hs_ld, hs_off, we, we_ld, we_off)
    if (H == 128) ZSG_LSTM_SEQ_FWD(128, true);
    else if (H == 64) ZSG_LSTM_SEQ_FWD(64, true);
    else if (H == 256) ZSG_LSTM_SEQ_FWD(256, false);
    else if (H == 32) ZSG_LSTM_SEQ_FWD(32, true);
    else ZSG_FAIL(-1, "lstm_seq_fwd: lstm_dim %d not supported (32/64/128/256)", H);
#undef ZSG_LSTM_SEQ_FWD
    ZSG_CHECK_LAUNCH("lstm_seq_fwd");
    return 0;
}

extern "C" int zsg_lstm_seq_bwd(const float* dwe, int32_t we_ld, int32_t we_off, const float* dhseq, int32_t hs_ld, int32_t hs_off,
                                const float* w_hh, const float* gates, const float* cst, const float* c0, const float* qlens_rank,
                                const float* lens, int32_t B, int32_t T, int32_t H, int32_t reverse, float* dgates, void* stream) {
    ZSG_REQUIRE(w_hh && gates && cst && c0 && qlens_rank && dgates && B > 0 && T > 0, "lstm_seq_bwd: null argument");
    ZSG_REQUIRE(dwe || dhseq, "lstm_seq_bwd: null argument (one of dwe / dhseq is required)");
    ZSG_REQUIRE(!dhseq || (hs_off >= 0 && hs_ld >= hs_off + H), "lstm_seq_bwd: window [%d, %d + %d) outside rows of %d", hs_off, hs_off, H, hs_ld);
    ZSG_REQUIRE(!dwe || (we_off >= 0 && we_ld >= we_off + H), "lstm_seq_bwd: window [%d, %d + %d) outside rows of %d", we_off, we_off, H, we_ld);
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("lstm_seq_bwd", st, 2.0 * B * T * 4 * H * H, 0);
#define ZSG_LSTM_SEQ_BWD(HH)                                                                                                          \
    ZSG_LAUNCH((lstm_seq_bwd_kernel<HH>), dim3(B), dim3(4 * HH), 0, st, dwe, we_ld, we_off, dhseq, hs_ld, hs_off, w_hh, gates, cst, c0, \
               qlens_rank, lens, B, T, reverse != 0, dgates)
    if (H == 128) ZSG_LSTM_SEQ_BWD(128);
    else if (H == 64) ZSG_LSTM_SEQ_BWD(64);
    else if (H == 256) ZSG_LSTM_SEQ_BWD(256);
    else if (H == 32) ZSG_LSTM_SEQ_BWD(32);
    else ZSG_FAIL(-1, "lstm_seq_bwd: lstm_dim %d not supported (32/64/128/256)", H);
#undef ZSG_LSTM_SEQ_BWD
    ZSG_CHECK_LAUNCH("lstm_seq_bwd");
    return 0;
}

#define POOL_MAX_T 4096          // the per-query scores live in LDS

extern "C" int zsg_lang_pool_fwd(const float* hseq, const float* lens, const float* w, int32_t mode, int32_t B, int32_t T, int32_t D, float* we,
                                 float* alpha, void* stream) {
    ZSG_REQUIRE(hseq && lens && we && B > 0 && T > 0 && D > 0, "lang_pool_fwd: null argument");
    ZSG_REQUIRE(mode == ZSG_LANG_POOL_MEAN || mode == ZSG_LANG_POOL_ATTN, "lang_pool_fwd: mode %d (0 mean, 1 attn)", mode);
    ZSG_REQUIRE(mode == ZSG_LANG_POOL_MEAN || w, "lang_pool_fwd: null argument (attn needs w)");
    ZSG_REQUIRE(T <= POOL_MAX_T, "lang_pool_fwd: T = %d > %d", T, POOL_MAX_T);
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("lang_pool_fwd", st, 2.0 * B * T * D, 4.0 * B * T * D);
    ZSG_LAUNCH(lang_pool_fwd_kernel, dim3(B), dim3(POOL_THREADS), (size_t)T * sizeof(float), st, hseq, lens, w, mode == ZSG_LANG_POOL_ATTN, T, D, we,
               alpha);
    ZSG_CHECK_LAUNCH("lang_pool_fwd");
    return 0;
}

extern "C" int zsg_lang_pool_bwd(const float* dwe, const float* hseq, const float* lens, const float* w, const float* alpha, int32_t mode,
                                 int32_t B, int32_t T, int32_t D, float* dhseq, float* ds, void* stream) {
    ZSG_REQUIRE(dwe && lens && dhseq && B > 0 && T > 0 && D > 0, "lang_pool_bwd: null argument");
    ZSG_REQUIRE(mode == ZSG_LANG_POOL_MEAN || mode == ZSG_LANG_POOL_ATTN, "lang_pool_bwd: mode %d (0 mean, 1 attn)", mode);
    ZSG_REQUIRE(mode == ZSG_LANG_POOL_MEAN || (hseq && w && alpha), "lang_pool_bwd: null argument (attn needs hseq, w and alpha)");
    ZSG_REQUIRE(T <= POOL_MAX_T, "lang_pool_bwd: T = %d > %d", T, POOL_MAX_T);
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("lang_pool_bwd", st, 4.0 * B * T * D, 8.0 * B * T * D);
    ZSG_LAUNCH(lang_pool_bwd_kernel, dim3(B), dim3(POOL_THREADS), (size_t)T * sizeof(float), st, dwe, hseq, lens, w, alpha,
               mode == ZSG_LANG_POOL_ATTN, T, D, dhseq, ds);
    ZSG_CHECK_LAUNCH("lang_pool_bwd");
    return 0;
}

extern "C" int zsg_lang_pool_wgrad(const float* ds, const float* hseq, int32_t B, int32_t T, int32_t D, float* dw, int32_t accumulate,
                                   void* stream) {
    ZSG_REQUIRE(ds && hseq && dw && B > 0 && T > 0 && D > 0, "lang_pool_wgrad: null argument");
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("lang_pool_wgrad", st, 2.0 * B * T * D, 4.0 * B * T * D);
    ZSG_LAUNCH(lang_pool_wgrad_kernel, dim3(cdiv(D, POOL_WG_COLS)), dim3(POOL_THREADS), 0, st, ds, hseq, B * T, D, dw, accumulate);
    ZSG_CHECK_LAUNCH("lang_pool_wgrad");
    return 0;
}
