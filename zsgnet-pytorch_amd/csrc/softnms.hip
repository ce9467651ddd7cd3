// softnms.hip — Soft-NMS selection of the evaluator's K boxes per query (Evaluator with cfg eval_nms = "soft_linear" / "soft_gauss"):
// zsg_eval_topk_soft.  (Bodla et al., "Soft-NMS — Improving Object Detection With One Line of Code", ICCV 2017.)
//
// zsg_eval_topk's greedy NMS deletes every candidate whose IoU with a kept box exceeds nms_thr.  Here a kept box lowers the scores of
// its neighbours as a function of their overlap and selection goes on over the decayed scores: the overlapping second object stays
// reachable, the emitted rows carry the decayed scores, and a score floor (min_score) ends the rows.  The contract is in include/zsg.h,
// the host definition in tests/softnms_ref.py.
//
// The candidates are zsg_eval_topk's, found again from out5 by the same two stages (loss.hip keeps its lists to itself, as for
// vote.hip): (SN_CHUNKS x B) blocks sort their anchor range in LDS and leave its best pre_n composites in the workspace, one block per
// query merges the lists by rank counting and decodes the candidates into LDS.  The ranking composite, the score expression, the box
// decode and the IoU are loss.hip's, restated here operation by operation (this file is built with -ffp-contract=off, as loss.hip is),
// so ranks, boxes and IoUs carry the same bits.  Each thread of the finishing block then owns candidates tid and tid + 256 with their
// fp64 weights in registers; a round is a wave-wide arg-max by lane exchange, four wave records in LDS (double-buffered by round
// parity: one barrier per round), a block-uniform winner and stop test, the row written by thread 0, and the decay of every thread's
// two candidates.  No atomics, a fixed reduction order, the same bits on every run.
#include <math.h>

#include "common.h"

typedef unsigned long long u64;
#define SN_CHUNKS 16            // anchor ranges per query (EV_CHUNKS of loss.hip)
#define SN_SORT 2048            // LDS sort buffer of a range block (composites)
#define SN_MAX_PRE 512
#define SN_MAX_K 64
#define SN_LDS_PRE 256          // the finishing block keeps the lists in LDS up to this pre_n (32 KB), beyond it it reads them from L2

// ---- loss.hip's pieces, in its operation order ---------------------------------------------------------------------------------
__device__ __forceinline__ float sn_iou(const f32x4 b, const f32x4 a) {       // iou_exact
    const float tly = fmaxf(b[0], a[0]), tlx = fmaxf(b[1], a[1]);
    const float bry = fminf(b[2], a[2]), brx = fminf(b[3], a[3]);
    const float sy = fmaxf(bry - tly, 0.f), sx = fmaxf(brx - tlx, 0.f);
    const float inter = sy * sx;
    const float barea = (b[2] - b[0]) * (b[3] - b[1]);
    const float aarea = (a[2] - a[0]) * (a[3] - a[1]);
    const float uni = (barea + aarea) - inter;
    return inter / (uni + 1e-8f);
}
__device__ __forceinline__ f32x4 sn_decode(const f32x4 an, const float* __restrict__ r) {    // decode_box
    const float acy = (an[0] + an[2]) / 2.f, acx = (an[1] + an[3]) / 2.f;
    const float ah = an[2] - an[0], aw = an[3] - an[1];
    const float cy = ah * r[0] + acy, cx = aw * r[1] + acx;
    const float h = expf(r[2]) * ah, w = expf(r[3]) * aw;
    f32x4 o = {cy - h / 2.f, cx - w / 2.f, cy + h / 2.f, cx + w / 2.f};
    return o;
}
__device__ __forceinline__ u64 sn_pack(float p, int a) {                       // tk_pack: (score descending, index ascending), NaN last
    const unsigned key = (p != p) ? 0u : __float_as_uint(p) + 1u;
    return ((u64)key << 32) | (unsigned)~a;
}
__device__ __forceinline__ float sn_score(u64 c) {                             // tk_score
    const unsigned key = (unsigned)(c >> 32);
    return key ? __uint_as_float(key - 1u) : __uint_as_float(0x7fc00000u);
}
__device__ __forceinline__ int sn_index(u64 c) { return (int)~(unsigned)c; }

__global__ __launch_bounds__(256) void softnms_chunk_kernel(const float* __restrict__ out5, int A, int pre_n, u64* __restrict__ lists) {
    __shared__ u64 sm[SN_SORT];
    const int b = blockIdx.y, c = blockIdx.x;
    const int per = (A + SN_CHUNKS - 1) / SN_CHUNKS;
    const int a0 = min(A, c * per), a1 = min(A, a0 + per);
    const float* o = out5 + (size_t)b * A * 5;
    u64* dst = lists + ((size_t)b * SN_CHUNKS + c) * pre_n;
    if (a0 >= a1) {                                                // an empty range (A < SN_CHUNKS ranges): padding only
        for (int i = threadIdx.x; i < pre_n; i += 256) dst[i] = 0;
        return;
    }
    int N = 64;                                                   // sort width: the carried list + one tile of the range
    while (N < pre_n + (a1 - a0) && N < SN_SORT) N <<= 1;       // (N > pre_n: the range is not empty and pre_n <= 512 < SN_SORT)
    const int tile = N - pre_n;
    for (int i = threadIdx.x; i < pre_n; i += 256) sm[i] = 0;
    int base = a0;
    do {
        for (int i = threadIdx.x; i < tile; i += 256) {
            const int a = base + i;
            u64 v = 0;
            if (a < a1) v = sn_pack(1.0f / (1.0f + expf(-o[(size_t)a * 5 + 4])), a);
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

__device__ __forceinline__ int sn_count_greater(const u64* l, int n, u64 x) {     // l sorted descending
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (l[mid] > x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the better of two (weight, position) records: the larger weight, ties to the smaller position; position -1 is "none"
__device__ __forceinline__ void sn_better(double& w, int& p, double ow, int op) {
    if (op >= 0 && (p < 0 || ow > w || (ow == w && op < p))) { w = ow; p = op; }
}

__global__ __launch_bounds__(256) void softnms_finish_kernel(const float* __restrict__ out5, const float* __restrict__ annot,
                                                             const float* __restrict__ anchors, const float* __restrict__ img_size,
                                                             int A, int pre_n, int K, float nms_thr, float acc_thr, int method,
                                                             float sigma, float min_score, const u64* __restrict__ lists,
                                                             float* __restrict__ topk_boxes, float* __restrict__ topk_scores,
                                                             int* __restrict__ topk_idx, int* __restrict__ topk_n,
                                                             int* __restrict__ hit_rank) {
    __shared__ u64 sm_lists[SN_CHUNKS * SN_LDS_PRE];
    __shared__ u64 sm_cand[SN_MAX_PRE];
    __shared__ f32x4 sm_box[SN_MAX_PRE];          // decoded, y1x1y2x2 in [-1, 1]: what the IoU compares
    __shared__ double sm_rw[2][4];                // the four waves' best weight of a round, by round parity
    __shared__ int sm_rp[2][4];                   // ... and its candidate position (-1: the wave has no eligible candidate)
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    const float* o = out5 + (size_t)b * A * 5;
    const u64* L = lists + (size_t)b * SN_CHUNKS * pre_n;
    const int nl = SN_CHUNKS * pre_n;
    for (int r = tid; r < SN_MAX_PRE; r += 256) sm_cand[r] = 0;
    if (pre_n <= SN_LDS_PRE) {
        for (int e = tid; e < nl; e += 256) sm_lists[e] = L[e];
        L = sm_lists;
    }
    __syncthreads();
    for (int e = tid; e < nl; e += 256) {                          // merge: a composite's rank is the number of larger ones
        const u64 x = L[e];
        if (x == 0) continue;
        int r = 0;
        for (int c = 0; c < SN_CHUNKS; ++c) r += sn_count_greater(L + c * pre_n, pre_n, x);
        if (r < pre_n) sm_cand[r] = x;
    }
    __syncthreads();
    const int nc = min(pre_n, A);
    bool elig[2];                                                  // not yet picked, a score that is a number
    double wgt[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {                                  // candidate r = tid + 256 s
        const int r = tid + 256 * s;
        const u64 cd = sm_cand[r];
        const int a = r < nc ? sn_index(cd) : -1;
        const unsigned key = (unsigned)(cd >> 32);
        const bool there = (unsigned)a < (unsigned)A;              // (every rank below nc is filled; the test keeps a stray index off memory)
        elig[s] = there && key != 0u;
        wgt[s] = elig[s] ? (double)__uint_as_float(key - 1u) : 0.0;
        if (there) sm_box[r] = sn_decode(*(const f32x4*)(anchors + 4 * (size_t)a), o + (size_t)a * 5);
    }
    f32x4 gt = {0.f, 0.f, 0.f, 0.f};
    if (annot) gt = *(const f32x4*)(annot + 4 * b);
    const float hh = img_size[2 * b], ww = img_size[2 * b + 1];
    const double floor_w = (double)min_score, dsigma = (double)sigma;
    __syncthreads();                                               // sm_box before the first row's reads
    int kept = 0, hit = K;
    for (; kept < K; ++kept) {
        int win = -1;
        double bw = 0.0;
        if (kept == 0) {                                           // row 0: candidate 0 whatever its score, as under hard NMS
            if ((unsigned)sn_index(sm_cand[0]) < (unsigned)A) win = 0;
        } else {
            double w = 0.0;
            int p = -1;
            if (elig[0]) { w = wgt[0]; p = tid; }
            if (elig[1]) sn_better(w, p, wgt[1], tid + 256);
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const double ow = __shfl_xor(w, d, 64);
                const int op = __shfl_xor(p, d, 64);
                sn_better(w, p, ow, op);
            }
            if ((tid & 63) == 0) { sm_rw[kept & 1][wave] = w; sm_rp[kept & 1][wave] = p; }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) sn_better(bw, win, sm_rw[kept & 1][q], sm_rp[kept & 1][q]);
            if (win >= 0 && bw < floor_w) win = -1;
        }
        if (win < 0) break;                                        // block-uniform
        const f32x4 kb = sm_box[win];
        if (tid == 0) {
            const u64 cd = sm_cand[win];
            float* pb = topk_boxes + ((size_t)b * K + kept) * 4;
            // (box+1)/2 * (h,w) then y1x1y2x2 -> x1y1x2y2, the expressions of eval_finish_kernel
            pb[0] = ww * ((kb[1] + 1.f) / 2.f);
            pb[1] = hh * ((kb[0] + 1.f) / 2.f);
            pb[2] = ww * ((kb[3] + 1.f) / 2.f);
            pb[3] = hh * ((kb[2] + 1.f) / 2.f);
            topk_scores[(size_t)b * K + kept] = kept == 0 ? sn_score(cd) : (float)bw;
            topk_idx[(size_t)b * K + kept] = sn_index(cd);
            if (annot && hit == K && sn_iou(kb, gt) >= acc_thr) hit = kept;
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int r = tid + 256 * s;
            if (r == win) elig[s] = false;
            if (!elig[s]) continue;
            const float u = sn_iou(kb, sm_box[r]);
            if (method == 1) {
                if (u > nms_thr) wgt[s] *= 1.0 - (double)u;
            } else {
                if (u == u) wgt[s] *= exp(-((double)u * (double)u) / dsigma);
            }
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

__global__ __launch_bounds__(64) void softnms_acc_kernel(const int* __restrict__ hit_rank, int B, int K, float* __restrict__ acc_at) {
    const int j = threadIdx.x;
    if (j >= K) return;
    double ok = 0;                                                 // (counts of 0 / 1: exact in any order)
    for (int b = 0; b < B; ++b) ok += hit_rank[b] <= j ? 1.0 : 0.0;
    acc_at[j] = (float)ok / (float)B;
}

extern "C" size_t zsg_eval_topk_soft_workspace_bytes(int32_t B, int32_t A, int32_t pre_n, int32_t K) {
    (void)A; (void)K;
    if (B <= 0 || pre_n <= 0) return 0;
    return (size_t)B * SN_CHUNKS * (size_t)pre_n * sizeof(u64);
}

extern "C" int zsg_eval_topk_soft(const float* out5, const float* annot, const float* anchors, const float* img_size, int32_t B,
                                  int32_t A, int32_t pre_n, int32_t K, float nms_thr, float acc_thr, int32_t method, float sigma,
                                  float min_score, float* topk_boxes, float* topk_scores, int32_t* topk_idx, int32_t* topk_n,
                                  int32_t* hit_rank, float* acc_at, void* ws, size_t ws_bytes, void* stream) {
    ZSG_REQUIRE(out5 && anchors && img_size && topk_boxes && topk_scores && topk_idx && topk_n && ws,
                "eval_topk_soft: null pointer argument");
    ZSG_REQUIRE(B > 0 && B <= 65535 && A > 0, "eval_topk_soft: bad shape B=%d A=%d", B, A);
    ZSG_REQUIRE(pre_n >= 1 && pre_n <= SN_MAX_PRE, "eval_topk_soft: pre_n=%d outside 1..%d", pre_n, SN_MAX_PRE);
    ZSG_REQUIRE(K >= 1 && K <= SN_MAX_K, "eval_topk_soft: K=%d outside 1..%d", K, SN_MAX_K);
    ZSG_REQUIRE(K <= pre_n, "eval_topk_soft: K=%d exceeds pre_n=%d", K, pre_n);
    ZSG_REQUIRE(method == 1 || method == 2, "eval_topk_soft: method=%d, expected 1 (linear) or 2 (gauss)", method);
    ZSG_REQUIRE(nms_thr >= 0.f && nms_thr <= 1.f, "eval_topk_soft: nms_thr=%g, expected a value in [0, 1]", (double)nms_thr);
    ZSG_REQUIRE(sigma > 0.f && sigma <= 3.402823466e38f, "eval_topk_soft: sigma=%g, expected a finite value > 0", (double)sigma);
    ZSG_REQUIRE(min_score >= 0.f && min_score < 1.f, "eval_topk_soft: min_score=%g, expected a value in [0, 1)", (double)min_score);
    ZSG_REQUIRE(!hit_rank || annot, "eval_topk_soft: hit_rank needs annot");
    ZSG_REQUIRE(!acc_at || hit_rank, "eval_topk_soft: acc_at needs hit_rank");
    ZSG_REQUIRE(ws_bytes >= zsg_eval_topk_soft_workspace_bytes(B, A, pre_n, K), "eval_topk_soft: ws_bytes=%zu, expected at least %zu",
                ws_bytes, zsg_eval_topk_soft_workspace_bytes(B, A, pre_n, K));
    ZSG_REQUIRE((((uintptr_t)ws) & 7) == 0, "eval_topk_soft: ws is not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("eval_topk_soft", st, 0, (double)B * A * 4);
    u64* lists = (u64*)ws;                           // [B][SN_CHUNKS][pre_n]
    ZSG_LAUNCH(softnms_chunk_kernel, dim3(SN_CHUNKS, B), dim3(256), 0, st, out5, A, pre_n, lists);
    ZSG_LAUNCH(softnms_finish_kernel, dim3(B), dim3(256), 0, st, out5, annot, anchors, img_size, A, pre_n, K, nms_thr, acc_thr,
               (int)method, sigma, min_score, (const u64*)lists, topk_boxes, topk_scores, topk_idx, topk_n, hit_rank);
    if (acc_at) ZSG_LAUNCH(softnms_acc_kernel, dim3(1), dim3(64), 0, st, (const int*)hit_rank, B, K, acc_at);
    ZSG_CHECK_LAUNCH("eval_topk_soft");
    return 0;
}
