// vote.hip — score-weighted box voting over the NMS candidates of the evaluator (Evaluator with cfg eval_box_vote > 0): zsg_eval_vote.
//
// The rows zsg_eval_topk kept stay what they are — their order, scores, anchor indices and count — and each row's box becomes the
// score-weighted mean of the candidates that overlap it (IoU >= vote_thr): the near-duplicates of neighbouring anchors, of the other
// scales of a multi-scale forward and of the mirrored pass, which the NMS only removes.  The contract is in include/zsg.h, the host
// definition in tests/vote_ref.py.
//
// The candidates are zsg_eval_topk's, found again from out5 by the same two stages (loss.hip keeps its lists to itself): (VT_CHUNKS x B)
// blocks sort their anchor range in LDS and leave its best pre_n composites in the workspace, one block per query merges the lists by
// rank counting and decodes the pre_n boxes into LDS.  The ranking composite, the score expression, the box decode and the IoU are
// loss.hip's, restated here operation by operation (this file is built with -ffp-contract=off, as loss.hip is), so ranks, boxes and
// IoUs carry the same bits.  Then one THREAD per kept row walks the candidates in rank order and sums in fp64: a fixed order, no
// atomics, the same bits on every run.  (K <= 64 rows of <= 512 candidates, every lane reading the same LDS word: a few microseconds.)
#include <math.h>

#include "common.h"

typedef unsigned long long u64;
#define VT_CHUNKS 16            // anchor ranges per query (EV_CHUNKS of loss.hip)
#define VT_SORT 2048            // LDS sort buffer of a range block (composites)
#define VT_MAX_PRE 512
#define VT_MAX_K 64
#define VT_LDS_PRE 128          // the finishing block keeps the lists in LDS up to this pre_n (16 KB), beyond it it reads them from L2

// ---- loss.hip's pieces, in its operation order ---------------------------------------------------------------------------------
__device__ __forceinline__ float vt_iou(const f32x4 b, const f32x4 a) {       // iou_exact
    const float tly = fmaxf(b[0], a[0]), tlx = fmaxf(b[1], a[1]);
    const float bry = fminf(b[2], a[2]), brx = fminf(b[3], a[3]);
    const float sy = fmaxf(bry - tly, 0.f), sx = fmaxf(brx - tlx, 0.f);
    const float inter = sy * sx;
    const float barea = (b[2] - b[0]) * (b[3] - b[1]);
    const float aarea = (a[2] - a[0]) * (a[3] - a[1]);
    const float uni = (barea + aarea) - inter;
    return inter / (uni + 1e-8f);
}
__device__ __forceinline__ f32x4 vt_decode(const f32x4 an, const float* __restrict__ r) {    // decode_box
    const float acy = (an[0] + an[2]) / 2.f, acx = (an[1] + an[3]) / 2.f;
    const float ah = an[2] - an[0], aw = an[3] - an[1];
    const float cy = ah * r[0] + acy, cx = aw * r[1] + acx;
    const float h = expf(r[2]) * ah, w = expf(r[3]) * aw;
    f32x4 o = {cy - h / 2.f, cx - w / 2.f, cy + h / 2.f, cx + w / 2.f};
    return o;
}
__device__ __forceinline__ f32x4 vt_pixels(const f32x4 kb, float hh, float ww) {    // (box+1)/2 * (h,w), y1x1y2x2 -> x1y1x2y2
    f32x4 o = {ww * ((kb[1] + 1.f) / 2.f), hh * ((kb[0] + 1.f) / 2.f), ww * ((kb[3] + 1.f) / 2.f), hh * ((kb[2] + 1.f) / 2.f)};
    return o;
}
__device__ __forceinline__ u64 vt_pack(float p, int a) {                       // tk_pack: (score descending, index ascending), NaN last
    const unsigned key = (p != p) ? 0u : __float_as_uint(p) + 1u;
    return ((u64)key << 32) | (unsigned)~a;
}
__device__ __forceinline__ int vt_index(u64 c) { return (int)~(unsigned)c; }

__global__ __launch_bounds__(256) void vote_chunk_kernel(const float* __restrict__ out5, int A, int pre_n, u64* __restrict__ lists) {
    __shared__ u64 sm[VT_SORT];
    const int b = blockIdx.y, c = blockIdx.x;
    const int per = (A + VT_CHUNKS - 1) / VT_CHUNKS;
    const int a0 = min(A, c * per), a1 = min(A, a0 + per);
    const float* o = out5 + (size_t)b * A * 5;
    u64* dst = lists + ((size_t)b * VT_CHUNKS + c) * pre_n;
    if (a0 >= a1) {                                                // an empty range (A < VT_CHUNKS ranges): padding only
        for (int i = threadIdx.x; i < pre_n; i += 256) dst[i] = 0;
        return;
    }
    int N = 64;                                                   // sort width: the carried list + one tile of the range
    while (N < pre_n + (a1 - a0) && N < VT_SORT) N <<= 1;       // (N > pre_n: the range is not empty and pre_n <= 512 < VT_SORT)
    const int tile = N - pre_n;
    for (int i = threadIdx.x; i < pre_n; i += 256) sm[i] = 0;
    int base = a0;
    do {
        for (int i = threadIdx.x; i < tile; i += 256) {
            const int a = base + i;
            u64 v = 0;
            if (a < a1) v = vt_pack(1.0f / (1.0f + expf(-o[(size_t)a * 5 + 4])), a);
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

__device__ __forceinline__ int vt_count_greater(const u64* l, int n, u64 x) {     // l sorted descending
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (l[mid] > x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool vt_finite4(const f32x4 v) {
    return fabsf(v[0]) <= 3.402823466e38f && fabsf(v[1]) <= 3.402823466e38f && fabsf(v[2]) <= 3.402823466e38f && fabsf(v[3]) <= 3.402823466e38f;
}

__global__ __launch_bounds__(256) void vote_finish_kernel(const float* __restrict__ out5, const float* __restrict__ annot,
                                                          const float* __restrict__ anchors, const float* __restrict__ img_size, int A,
                                                          int pre_n, int K, float vote_thr, float acc_thr, const u64* __restrict__ lists,
                                                          const float* __restrict__ topk_boxes, const int* __restrict__ topk_idx,
                                                          const int* __restrict__ topk_n, float* __restrict__ vote_boxes,
                                                          int* __restrict__ vote_n, int* __restrict__ hit_rank) {
    __shared__ u64 sm_lists[VT_CHUNKS * VT_LDS_PRE];
    __shared__ u64 sm_cand[VT_MAX_PRE];
    __shared__ f32x4 sm_box[VT_MAX_PRE];          // decoded, y1x1y2x2 in [-1, 1]: what the NMS compared
    __shared__ f32x4 sm_px[VT_MAX_PRE];           // the same boxes in pixels x1y1x2y2: what the vote averages
    __shared__ float sm_w[VT_MAX_PRE];            // the score; a negative value marks a candidate that is never a member
    __shared__ int sm_hit[VT_MAX_K];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* o = out5 + (size_t)b * A * 5;
    const u64* L = lists + (size_t)b * VT_CHUNKS * pre_n;
    const int nl = VT_CHUNKS * pre_n;
    for (int r = tid; r < VT_MAX_PRE; r += 256) sm_cand[r] = 0;
    if (pre_n <= VT_LDS_PRE) {
        for (int e = tid; e < nl; e += 256) sm_lists[e] = L[e];
        L = sm_lists;
    }
    __syncthreads();
    for (int e = tid; e < nl; e += 256) {                          // merge: a composite's rank is the number of larger ones
        const u64 x = L[e];
        if (x == 0) continue;
        int r = 0;
        for (int c = 0; c < VT_CHUNKS; ++c) r += vt_count_greater(L + c * pre_n, pre_n, x);
        if (r < pre_n) sm_cand[r] = x;
    }
    __syncthreads();
    const int nc = min(pre_n, A);
    const float hh = img_size[2 * b], ww = img_size[2 * b + 1];
    for (int r = tid; r < VT_MAX_PRE; r += 256) {
        const u64 cd = sm_cand[r];
        const int a = r < nc ? vt_index(cd) : -1;
        float wgt = -1.f;
        f32x4 bx = {0.f, 0.f, 0.f, 0.f}, px = {0.f, 0.f, 0.f, 0.f};
        if ((unsigned)a < (unsigned)A) {                           // (every rank below nc is filled; the test keeps a stray index off memory)
            bx = vt_decode(*(const f32x4*)(anchors + 4 * (size_t)a), o + (size_t)a * 5);
            px = vt_pixels(bx, hh, ww);
            const unsigned key = (unsigned)(cd >> 32);
            if (key && vt_finite4(bx) && vt_finite4(px)) wgt = __uint_as_float(key - 1u);      // tk_score; key 0 is a NaN score
        }
        sm_box[r] = bx;
        sm_px[r] = px;
        sm_w[r] = wgt;
    }
    __syncthreads();
    const int kept = min(max(topk_n[b], 0), K);
    const int row = (tid >> 6) + 4 * (tid & 63);                   // rows spread over the four waves
    if (row < VT_MAX_K && row < K) {
        float* vb = vote_boxes + ((size_t)b * K + row) * 4;
        int members = 0, hit = 0;
        f32x4 res = {0.f, 0.f, 0.f, 0.f};
        if (row < kept) {
            const float* tb = topk_boxes + ((size_t)b * K + row) * 4;
            res = f32x4{tb[0], tb[1], tb[2], tb[3]};
            const int want = topk_idx[(size_t)b * K + row];
            int own = -1;
            for (int c = 0; c < nc; ++c)
                if (vt_index(sm_cand[c]) == want) { own = c; break; }
            f32x4 vn = {0.f, 0.f, 0.f, 0.f};                       // the voted box in the NMS's coordinates, for the hit test
            bool have_vn = false;
            if (own >= 0) {
                vn = sm_box[own];
                have_vn = true;
            }
            if (own >= 0 && sm_w[own] >= 0.f) {
                const f32x4 kb = sm_box[own];
                double sw = 0, sp[4] = {0, 0, 0, 0}, sn[4] = {0, 0, 0, 0};
                for (int c = 0; c < nc; ++c) {                     // candidate order: the summation order of the contract
                    const float s = sm_w[c];
                    if (s < 0.f) continue;
                    if (c != own && !(vt_iou(kb, sm_box[c]) >= vote_thr)) continue;
                    ++members;
                    const f32x4 p = sm_px[c], q = sm_box[c];
                    sw += (double)s;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        sp[j] += (double)s * (double)p[j];
                        sn[j] += (double)s * (double)q[j];
                    }
                }
                if (sw > 0) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        res[j] = (float)(sp[j] / sw);
                        vn[j] = (float)(sn[j] / sw);
                    }
                }
            }
            if (annot && have_vn) hit = vt_iou(vn, *(const f32x4*)(annot + 4 * b)) >= acc_thr ? 1 : 0;
        }
        vb[0] = res[0], vb[1] = res[1], vb[2] = res[2], vb[3] = res[3];
        vote_n[(size_t)b * K + row] = members;
        sm_hit[row] = hit;
    }
    __syncthreads();
    if (tid == 0 && hit_rank) {
        int h = K;
        for (int r = kept - 1; r >= 0; --r)
            if (sm_hit[r]) h = r;
        hit_rank[b] = h;
    }
}

__global__ __launch_bounds__(64) void vote_acc_kernel(const int* __restrict__ hit_rank, int B, int K, float* __restrict__ acc_at) {
    const int j = threadIdx.x;
    if (j >= K) return;
    double ok = 0;                                                 // (counts of 0 / 1: exact in any order)
    for (int b = 0; b < B; ++b) ok += hit_rank[b] <= j ? 1.0 : 0.0;
    acc_at[j] = (float)ok / (float)B;
}

extern "C" size_t zsg_eval_vote_workspace_bytes(int32_t B, int32_t A, int32_t pre_n, int32_t K) {
    (void)A; (void)K;
    if (B <= 0 || pre_n <= 0) return 0;
    return (size_t)B * VT_CHUNKS * (size_t)pre_n * sizeof(u64);
}

extern "C" int zsg_eval_vote(const float* out5, const float* annot, const float* anchors, const float* img_size, int32_t B, int32_t A,
                             int32_t pre_n, int32_t K, float vote_thr, float acc_thr, const float* topk_boxes, const float* topk_scores,
                             const int32_t* topk_idx, const int32_t* topk_n, float* vote_boxes, int32_t* vote_n, int32_t* hit_rank,
                             float* acc_at, void* ws, size_t ws_bytes, void* stream) {
    ZSG_REQUIRE(out5 && anchors && img_size && topk_boxes && topk_scores && topk_idx && topk_n && vote_boxes && vote_n && ws,
                "eval_vote: null pointer argument");
    ZSG_REQUIRE(B > 0 && B <= 65535 && A > 0, "eval_vote: bad shape B=%d A=%d", B, A);
    ZSG_REQUIRE(pre_n >= 1 && pre_n <= VT_MAX_PRE, "eval_vote: pre_n=%d outside 1..%d", pre_n, VT_MAX_PRE);
    ZSG_REQUIRE(K >= 1 && K <= VT_MAX_K, "eval_vote: K=%d outside 1..%d", K, VT_MAX_K);
    ZSG_REQUIRE(K <= pre_n, "eval_vote: K=%d exceeds pre_n=%d", K, pre_n);
    ZSG_REQUIRE(vote_thr > 0.f && vote_thr <= 1.f, "eval_vote: vote_thr=%g, expected a value in (0, 1]", (double)vote_thr);
    ZSG_REQUIRE(!hit_rank || annot, "eval_vote: hit_rank needs annot");
    ZSG_REQUIRE(!acc_at || hit_rank, "eval_vote: acc_at needs hit_rank");
    ZSG_REQUIRE(ws_bytes >= zsg_eval_vote_workspace_bytes(B, A, pre_n, K), "eval_vote: ws_bytes=%zu, expected at least %zu", ws_bytes,
                zsg_eval_vote_workspace_bytes(B, A, pre_n, K));
    ZSG_REQUIRE((((uintptr_t)ws) & 7) == 0, "eval_vote: ws is not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("eval_vote", st, 0, (double)B * A * 4);
    u64* lists = (u64*)ws;                           // [B][VT_CHUNKS][pre_n]
    ZSG_LAUNCH(vote_chunk_kernel, dim3(VT_CHUNKS, B), dim3(256), 0, st, out5, A, pre_n, lists);
    ZSG_LAUNCH(vote_finish_kernel, dim3(B), dim3(256), 0, st, out5, annot, anchors, img_size, A, pre_n, K, vote_thr, acc_thr,
               (const u64*)lists, topk_boxes, topk_idx, topk_n, vote_boxes, vote_n, hit_rank);
    if (acc_at) ZSG_LAUNCH(vote_acc_kernel, dim3(1), dim3(64), 0, st, (const int*)hit_rank, B, K, acc_at);
    ZSG_CHECK_LAUNCH("eval_vote");
    return 0;
}
