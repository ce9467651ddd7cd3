// igemm.hip — implicit-GEMM convolution (forward and data-gradient) on fp32 MFMA, NHWC x OHWI, gfx950.
//
// GEMM view:  Out[row][n] = sum_{taps} sum_{c<C} Src[gather(row, tap)][c] * Wt[n][tap][c]
//   rows  = (segment, b, y, x)      -> M   (pixels; A operand, channels contiguous)
//   n     = output channel          -> N   (B operand = weight rows, channels contiguous)
//   K     = taps x C, walked tap-major in BK=32 chunks.
// Both operands are K-contiguous, so a tile row is staged with 16-byte loads and each lane reads its MFMA
// fragments with ds_read_b128: lane (i = lane&31, h = lane>>5) reads k = kq*8 + 4h .. +3 of row i and feeds
// value j to the j-th of four v_mfma_f32_32x32x2_f32 (k permuted identically for A and B, the sum is over all k).
// LDS rows are padded to 36 floats (9 x 16 B: odd) so the b128 reads of 16 distinct rows are conflict-free.
// Pipeline: global->registers for tile t+1 is issued before the MFMAs of tile t; registers->LDS after them into
// the other buffer; one barrier per K-tile.
#include <stdlib.h>

#include "common.h"
#include "bn_tail.h"

ZSG_DEFINE_PRIO_FLAG()

#define IG_BK 32
#define IG_LDK 36

struct IgSegDev {
    int rows_y, rows_x, rows;   // rows = B*rows_y*rows_x
    int tile0;                  // first M tile of the segment
    int src_H, src_W, sy, sx;
    int out_W, osy, osx, opy, opx;
    int src_off, src_bstride, out_off, out_bstride;   // elements, < 2^31
    zsg_taps ty, tx;
};

// The producer BatchNorm applied by the operand loader (round 5, template flag PRE): `src` is the RAW output x of the previous block's last
// convolution; the loader stages relu((x - mean) * invstd * gamma + beta + residual) — exactly what zsg_bn_apply writes — and the
// blocks of the first column tile also write that activation (y) and its packed ReLU bits out, so that the separate apply launch
// (read x + residual, write y: 280 MB at layer1's size, then y read again by this convolution) disappears.  1x1 / stride-1 dense
// convolutions only: a source element belongs to exactly one row of the GEMM.
struct IgPre {
    const float* mean;
    const float* invstd;
    const float* gamma;
    const float* beta;
    const float* residual;      // same [rows][C] layout as src
    float* y;                   // the materialised activation (same layout) — the residual of the next block, the weight gradient's input
    unsigned char* mask;        // 4 ReLU bits per 16-byte group, as zsg_bn_apply writes them (or nullptr)
};

struct IgParams {
    const float* src;
    const float* wt;
    float* out;
    const float* bias;
    const float* add_src;
    const float* mask_src;
    float* stats;     // optional BatchNorm partials [m_tiles][2][N]: per-tile column sums / sums of squares of the output
    int C, N, src_ld, out_ld, wS, wC, wc0, wt_ld, relu, nseg;
    int m_tiles, n_tiles;
    int splits;       // split-K factor (1: plain stores; >1: fp32 atomic accumulation into a zeroed / pre-filled output)
    int remap;        // XCD-aware tile order (only when every segment carries the same amount of K work)
    int vec;          // 16-byte epilogue allowed (alignment of every operand checked on the host)
    int bk64;         // tile_hint bit 27: 64-deep K tiles
    double alg_bytes; // host only: algorithmic HBM bytes of the launch (profile)
    int add_is_out;   // add_src aliases out (accumulate): with split-K the existing values are simply added to
    BnbDev bnb;       // bnb.x != nullptr: `stats` receives BatchNorm-BACKWARD partials of the stored values (see common.h)
    BnTail tail;      // tail.tickets != nullptr: the last-arriving tile of a column block finalises the statistics (bn_tail.h)
    IgPre pre;        // PRE kernels only
    // stream-K (SK kernels only; tile_hint bits 28-29): sk_grid workgroups share the launch's (tile, K step) units evenly, sk_per
    // consecutive units each; a tile cut between workgroups is completed by the one that holds its FIRST K step
    int sk_grid, sk_per;
    float* sk_ws;         // partial accumulator tiles, one BM x BN slot per workgroup (zsg_set_stream_workspace)
    unsigned* sk_flags;   // one word per workgroup: "its partial tile is published"; zero at entry, zero at exit
    IgSegDev seg[ZSG_MAX_SEG];
};

// BM x BN block tile computed by NW = WM x WN waves (4: 2 x 2; 8: 2 x 4, or 4 x 2 for the 128x64 tile; each wave: TM x TN MFMA tiles
// of 32x32), times KS "K groups": wave group
// kg multiplies the kg-th 1/KS of every 32-deep K tile and the groups' accumulators are summed through LDS before the
// epilogue (intra-block split-K: fixed order, no atomics).  It puts KS times as many waves on a SIMD for the same tile —
// what the small-grid layers (a few hundred 64x64 tiles for 256 CUs) need to hide LDS / barrier latency.
//
// BK: K-tile depth.  32 = one barrier per 32 reduction elements; 64 halves the number of K steps — each step carries ~0.3-0.4 us
// that no MFMA overlaps (address arithmetic, load issue, fragment-read latency, the barrier: tools/igemm_model.py, profiles/
// r03_igemm_model_*.txt), which at one or two resident blocks per CU is 25-45 % of a step — at twice the LDS per block.
//
// (SK: four waves per SIMD = 128 registers — inside the pass loop hipcc otherwise parks every hoisted constant in a register of its own,
// 114 -> 244 registers, and a CU holds ONE stream-K workgroup where the launch counts on two.)
// __launch_bounds__' second argument (two waves per SIMD = at most 256 registers per lane): without it hipcc parks the accumulators
// of the 4-wave tiles in AGPRs and copies one tile in and out of them every K step (32 v_accvgpr moves per 16 MFMAs — VALU-class
// instructions that are paid in full next to fp32 MFMAs).  The 64-deep 128x128 4-wave tile needs more than 256 registers.
//
// SK (stream-K, round 6; tile_hint bits 28-29 = workgroups per CU): the grids of layer3 / layer4's 1x1 convolutions are one to two rounds of tiles on 256 CUs (364 tiles of 64x64 =
// two rounds at 71 %; 184 tiles of 128x64 = 72 idle CUs).  With SK the launch has a FIXED number of workgroups (256 x blocks-per-CU) and
// the work is cut into (tile, K step) units dealt evenly: workgroup l owns units [l * per, (l + 1) * per) in tile-major order, i.e. the
// tail of one tile (its last K steps) followed by the head of the next.  The workgroup that holds a tile's first K step FINISHES the tile:
// it adds the partial accumulator tiles of the workgroups behind it in workgroup order (fixed order: deterministic) and runs the complete
// epilogue (fused BatchNorm partials, in-kernel finalize and all) — nothing downstream changes.  A workgroup works through its range in
// ascending order, so its producer segment (a tile's tail) always comes first and never waits: the finisher's poll cannot deadlock
// whatever the dispatch order (producers only need to be dispatched, and a waiting finisher holds one workgroup slot).  Hand-off
// (MI355X_MICROARCH.md, inter-workgroup visibility): partial tile by 16-byte write-through (sc1) stores -> every storing wave drains
// (s_waitcnt vmcnt(0)) -> barrier -> one relaxed agent-scope flag store; the finisher polls the flag with relaxed agent-scope loads
// (+ s_sleep), re-zeroes it, and reads the tile with sc1 loads.  No fences (an agent-scope release writes back the XCD's whole L2).
template <int BM, int BN, int NW, bool MERGE_X, int KS = 1, int BK = IG_BK, bool PRE = false, bool SK = false>
__global__ __launch_bounds__(64 * NW * KS, (BK == 64 && BM * BN >= 128 * 128 && NW * KS <= 4) ? 1 : (SK && !(BM * BN >= 128 * 128 && NW * KS <= 4)) ? 4 : 2)
void igemm_kernel(const IgParams p) {
    ZSG_SET_MAIN_PRIO();
    static_assert(!PRE || !MERGE_X, "the BatchNorm-applying loader is for 1x1 convolutions");
    static_assert(!SK || (!PRE && !MERGE_X), "stream-K: plain single-segment convolutions");
    static_assert(NW == 4 || NW == 8, "4 or 8 waves per K group");
    constexpr int WM = (NW == 8 && BN == 64) ? 4 : 2, WN = NW / WM;     // the wave grid over the tile
    constexpr int NB = 2;                    // LDS tile buffers
    static_assert(BK == 32 || (BK == 64 && !MERGE_X), "K tile depth");
    constexpr int LDR = BK + 4;              // floats per LDS tile row (an odd number of 16-byte units: conflict-free b128 fragment reads)
    constexpr int NT = 64 * WM * WN * KS;     // threads
    constexpr int KG = BK / 4;           // threads (16-byte groups) per tile row
    constexpr int RP = NT / KG;          // tile rows staged per pass
    constexpr int RA = BM / RP;          // A rows staged per thread
    constexpr int RB = BN / RP;          // B rows staged per thread
    constexpr int TM = BM / WM / 32;     // 32x32 MFMA tiles per wave along M
    constexpr int TN = BN / WN / 32;
    static_assert(RA >= 1 && RB >= 1 && TM >= 1 && TN >= 1, "tile too small for the wave grid");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                                  // [NB][BM][LDR]
    float* Bs = smem + NB * BM * LDR;                  // [NB][BN][LDR]
    int* rowout = (int*)(smem + NB * (BM + BN) * LDR); // [BM]


    const int n_tiles_mn = p.m_tiles * p.n_tiles;
    // SK: this workgroup's range of (tile, K step) units, [sk_u, sk_u1) in tile-major order; workgroups that land on one XCD own
    // neighbouring ranges (the partial tiles they exchange and the operand rows they share stay in that XCD's neighbourhood)
    int sk_l = 0, sk_u = 0, sk_u1 = 0, sk_nit = 1;
    if constexpr (SK) {
        sk_l = xcd_remap(blockIdx.x, p.sk_grid);
        sk_nit = p.seg[0].ty.n * p.seg[0].tx.n * ((p.C + BK - 1) / BK);
        sk_u = sk_l * p.sk_per;
        sk_u1 = min(n_tiles_mn * sk_nit, sk_u + p.sk_per);
        if (sk_u >= sk_u1) return;
    }
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int kg = wave / (WM * WN);     // K group of this wave
    const int wmn = wave % (WM * WN);
    const int wm = wmn / WN, wn = wmn % WN;
    const int g = tid % KG;              // 16-byte k-group staged by this thread
    const int r0 = tid / KG;             // first staged row
    const int li = lane & 31, lh = lane >> 5;
    // the tile of the current pass (what the epilogue behind the pass loop completes)
    int mt = 0, nt = 0, n0 = 0, split = 0;
    int sk_t = 0, sk_k0 = 0, sk_k1 = 0;  // SK: the tile of this pass and its K steps [sk_k0, sk_k1)
    f32x16 acc[TM][TN];
  // One pass, unless SK: then a workgroup's unit range is at most a tile's TAIL (K steps [k0, n): a producer pass — K loop, publish, next
  // pass) followed by a tile's HEAD or a whole tile (the finishing pass, which leaves the loop for the epilogue).  The epilogue stays
  // OUTSIDE the loop: inside it hipcc keeps the epilogue's per-thread state live across the next pass's K loop (96 -> 244 registers).
  for (;;) {
    if constexpr (SK) {
        sk_t = sk_u / sk_nit;
        sk_k0 = sk_u - sk_t * sk_nit;
        sk_k1 = min(sk_nit, sk_k0 + (sk_u1 - sk_u));
    } else
        split = blockIdx.x / n_tiles_mn;
    const int bid0 = SK ? sk_t : blockIdx.x - split * n_tiles_mn;
    const int bid = (!SK && p.remap) ? xcd_remap(bid0, n_tiles_mn) : bid0;
    mt = bid / p.n_tiles;
    nt = bid % p.n_tiles;
    int si = 0;
#pragma unroll
    for (int s = 1; s < ZSG_MAX_SEG; ++s)
        if (s < p.nseg && mt >= p.seg[s].tile0) si = s;
    const IgSegDev sg = p.seg[si];       // by value: keeps the geometry in SGPRs for the whole K loop
    const int srcH = sg.src_H, srcW = sg.src_W, src_ld = p.src_ld, Cdim = p.C;
    const int m0 = (mt - sg.tile0) * BM;
    n0 = nt * BN;

    // ---- per-row gather state (fixed for the whole K loop) --------------------------------------------------
    int a_by[RA], a_bx[RA], a_off[RA];   // a_off: element offset of the row's tap (0, 0) pixel — a tap adds a WAVE-UNIFORM offset
    constexpr int RPRE = PRE ? RA : 1;
    unsigned pre_off[RPRE];              // PRE: byte offset of the row's channel 0 in src / residual / y (out of range for dead rows)
#pragma unroll
    for (int j = 0; j < RA; ++j) {
        const int m = m0 + r0 + RP * j;
        const bool ok = m < sg.rows;
        const int mm = ok ? m : 0;
        const int per = sg.rows_y * sg.rows_x;
        const int b = mm / per;
        const int rem = mm - b * per;
        const int y = rem / sg.rows_x;
        const int x = rem - y * sg.rows_x;
        a_by[j] = ok ? (y * sg.sy + sg.ty.d0) : -(1 << 28);      // invalid rows fail the bounds test for every tap
        a_bx[j] = x * sg.sx + sg.tx.d0;
        a_off[j] = ok ? sg.src_off + b * sg.src_bstride + (a_by[j] * sg.src_W + a_bx[j]) * p.src_ld : 0;
        if constexpr (PRE) pre_off[j] = ok ? 4u * (unsigned)a_off[j] : ZSG_OOB;
        if (g == 0)
            rowout[r0 + RP * j] =
                ok ? sg.out_off + b * sg.out_bstride + ((y * sg.osy + sg.opy) * sg.out_W + (x * sg.osx + sg.opx)) * p.out_ld
                   : -1;
    }
    int b_off[RB];
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        const int n = n0 + r0 + RP * j;
        b_off[j] = (n < p.N) ? n * p.wt_ld + p.wc0 : -1;
    }

    const int n_cc = MERGE_X ? 1 : (p.C + BK - 1) / BK;
    const int n_jx = MERGE_X ? 1 : sg.tx.n;
    const int n_it_all = sg.ty.n * n_jx * n_cc;
    int it0 = 0, n_it = n_it_all;
    if (p.splits > 1) {                  // this block's slice of the K iterations
        const int per = (n_it_all + p.splits - 1) / p.splits;
        it0 = min(split * per, n_it_all);
        n_it = min(per, n_it_all - it0);
    }
    if constexpr (SK) {
        it0 = sk_k0;
        n_it = sk_k1 - sk_k0;
    }

    // Register stages: the global loads run NS K tiles ahead of the MFMAs.  NS = 2.  Deeper prefetch (4 stages where a stage is
    // <= 16 registers, 3 up to 24) was measured in round 3 on the hypothesis that one or two resident blocks per CU are
    // latency-starved: single launches did not move (M=1600 N=512 K=2048 64x64: 59.0 -> 59.0 us, 8-wave 52.0 -> 52.4; tools/
    // igemm_model.py) and the step lost 1.6 % to the registers (14.32 -> 14.55 ms): not what the K loop waits for.
    constexpr int NS = 2;
    f32x4 ra[NS][RA], rb[NS][RB];
    f32x4 rres[NS][RPRE], pvec[NS][3];   // PRE: the residual rows of a stage; (mean, invstd * gamma, beta) of its four channels
    int pch[NS];                         // PRE: the stage's first channel (bytes), or -1 past the last K tile
    const rsrc_t rsrc_res = make_rsrc(PRE ? (const void*)p.pre.residual : (const void*)p.src);
    const rsrc_t rsrc_y = make_rsrc(PRE ? (const void*)p.pre.y : (const void*)p.src);
    const rsrc_t rsrc_pm = make_rsrc(PRE && p.pre.mask ? (const void*)p.pre.mask : (const void*)p.src);
    const rsrc_t rsrc_a = make_rsrc(p.src);
    const rsrc_t rsrc_b = make_rsrc(p.wt);
    // K-iteration counters of the NEXT tile to load (wave-uniform)
    int cc = it0 % n_cc;
    int jx = (it0 / n_cc) % n_jx;
    int jy = it0 / (n_cc * n_jx);

    unsigned a_vo[RA], b_vo[RB];       // per-lane byte offsets of the current tap's tile rows (see load_tile)
    int so_a = 0, so_b = 0, skip = 0;  // the tile's channel offset in both operands (bytes, SGPRs); tiles until the offsets are recomputed
    const bool c_tail = (Cdim % BK) != 0;
    // live == false (past the last K tile): every lane gets an out-of-range offset, i.e. the loads still issue — and
    // return zeros without touching memory — so the K loop has no branch around them and the compiler can count the
    // outstanding loads exactly (a branch made it wait for ALL of them, vmcnt(0), before parking the previous tile).
    auto load_tile = [&](f32x4 (&ra)[RA], f32x4 (&rb)[RB], bool live, int stg = 0) {
        const int wr = sg.ty.w0 + jy * sg.ty.wstep;
        const int dyy = jy * sg.ty.dstep;
        int ws_, dxx, koff;
        bool kok;
        if (MERGE_X) {                    // C == 4: the tx.n taps of this row are one contiguous run
            ws_ = sg.tx.w0;
            dxx = g;
            koff = 4 * g;
            kok = live & (g < sg.tx.n);
        } else {
            ws_ = sg.tx.w0 + jx * sg.tx.wstep;
            dxx = jx * sg.tx.dstep;
            koff = cc * BK + 4 * g;
            kok = live & (koff < Cdim);
        }
        if constexpr (!MERGE_X) {
            // Nothing co-issues with a SIMD's fp32 MFMA stream on gfx950 and a VALU instruction costs ~6 cycles on top of it
            // (tools/ubench/mfma_coissue.hip): the per-lane byte offsets of a tile (tap validity, channel group; out of range = zeros)
            // are STATE that changes only when the filter tap changes (or in the channel tail); inside a tap the channel offset
            // advances in an SGPR (the buffer instructions' soffset) and a K tile costs no address arithmetic at all.
            if (skip == 0 || !live) {                      // wave-uniform: first tile of a tap, the channel tail, past the end
                const bool tail = c_tail && cc == n_cc - 1;
                const bool klane = live & (!tail || koff < Cdim);
                const int tap = (dyy * srcW + dxx) * src_ld + 4 * g;
#pragma unroll
                for (int j = 0; j < RA; ++j) {
                    const int yy = a_by[j] + dyy, xx = a_bx[j] + dxx;
                    const bool ok = klane & ((unsigned)yy < (unsigned)srcH) & ((unsigned)xx < (unsigned)srcW);
                    a_vo[j] = ok ? 4u * (unsigned)(a_off[j] + tap) : ZSG_OOB;
                }
#pragma unroll
                for (int j = 0; j < RB; ++j) b_vo[j] = (klane & (b_off[j] >= 0)) ? 4u * (unsigned)(b_off[j] + 4 * g) : ZSG_OOB;
                so_a = 4 * cc * BK;
                so_b = 4 * ((wr * p.wS + ws_) * p.wC + cc * BK);
                // tiles until the next recomputation: up to the tap's last chunk, which is recomputed when it is a channel tail
                skip = tail ? 0 : n_cc - 1 - cc - (c_tail ? 1 : 0);
                if (skip < 0) skip = 0;
            } else {
                --skip;
            }
            typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
            for (int j = 0; j < RA; ++j) ra[j] = __builtin_bit_cast(f32x4, (u32x4)__builtin_amdgcn_raw_buffer_load_b128(rsrc_a, (int)a_vo[j], so_a, 0));
#pragma unroll
            for (int j = 0; j < RB; ++j) rb[j] = __builtin_bit_cast(f32x4, (u32x4)__builtin_amdgcn_raw_buffer_load_b128(rsrc_b, (int)b_vo[j], so_b, 0));
            if constexpr (PRE) {          // (1x1: the K tile's channels are so_a / 4 + 4 g .. + 3)
                pch[stg] = live ? so_a + 16 * g : -1;
#pragma unroll
                for (int j = 0; j < RA; ++j)
                    rres[stg][j] = __builtin_bit_cast(f32x4, (u32x4)__builtin_amdgcn_raw_buffer_load_b128(rsrc_res, (int)(live ? pre_off[j] + 16u * (unsigned)g : ZSG_OOB), so_a, 0));
                const int c = (so_a >> 2) + 4 * g;
                const int cs = live ? c : 0;
                pvec[stg][0] = *(const f32x4*)(p.pre.mean + cs);
                pvec[stg][1] = *(const f32x4*)(p.pre.invstd + cs) * *(const f32x4*)(p.pre.gamma + cs);
                pvec[stg][2] = *(const f32x4*)(p.pre.beta + cs);
            }
            so_a += 4 * BK;
            so_b += 4 * BK;
        } else {                          // (the 7x7x4 stem: one K tile per filter row, nothing to carry between tiles)
            const int wtap = (wr * p.wS + ws_) * p.wC + 4 * g;
            const int toff = dyy * srcW * src_ld + 4 * g;
#pragma unroll
            for (int j = 0; j < RA; ++j) {
                const int yy = a_by[j] + dyy, xx = a_bx[j] + dxx;
                // branch-free validity (bitwise &): out-of-image taps / dead rows get an out-of-range buffer offset (zeros)
                const bool ok = kok & ((unsigned)yy < (unsigned)srcH) & ((unsigned)xx < (unsigned)srcW);
                ra[j] = buf_load4(rsrc_a, ok ? 4u * (unsigned)(a_off[j] + toff) : ZSG_OOB);
            }
#pragma unroll
            for (int j = 0; j < RB; ++j) rb[j] = buf_load4(rsrc_b, (kok & (b_off[j] >= 0)) ? 4u * (unsigned)(b_off[j] + wtap) : ZSG_OOB);
        }
        // advance counters
        if (++cc == n_cc) {
            cc = 0;
            if (++jx == n_jx) {
                jx = 0;
                ++jy;
            }
        }
    };
    auto store_tile = [&](int buf, const f32x4 (&ra)[RA], const f32x4 (&rb)[RB], int stg = 0) {
        float* a = As + buf * BM * LDR;
        float* b = Bs + buf * BN * LDR;
        if constexpr (PRE) {
            // the producer BatchNorm + residual + ReLU, in zsg_bn_apply's own arithmetic; dead rows / dead tiles stage exact zeros (the
            // fused statistics of THIS convolution rely on it).  Column tile 0 materialises the activation and its ReLU bits.
            const bool tlive = pch[stg] >= 0;
            const bool wr = tlive & (nt == 0);
            typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
            for (int j = 0; j < RA; ++j) {
                f32x4 v = (ra[j] - pvec[stg][0]) * pvec[stg][1] + pvec[stg][2];
                v += rres[stg][j];
                const unsigned bits = (unsigned)(v[0] > 0.f) | ((unsigned)(v[1] > 0.f) << 1) | ((unsigned)(v[2] > 0.f) << 2) | ((unsigned)(v[3] > 0.f) << 3);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                const bool ok = tlive & (pre_off[j] != ZSG_OOB);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = ok ? v[e] : 0.f;
                const unsigned off = (wr & ok) ? pre_off[j] + (unsigned)pch[stg] : ZSG_OOB;
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rsrc_y, (int)off, 0, 0);
                if (p.pre.mask) {
                    // the KG = 8 threads of a tile row hold 8 consecutive mask bytes: gathered into one 8-byte store by the row's first thread
                    static_assert(KG == 8, "mask packing assumes 8 16-byte groups per K tile row");
                    unsigned lo = bits << (8 * (g & 3)), hi;
                    lo |= __shfl_xor(lo, 1, 64);
                    lo |= __shfl_xor(lo, 2, 64);
                    hi = __shfl_xor(lo, 4, 64);
                    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
                    const u32x2 pk = {lo, hi};
                    __builtin_amdgcn_raw_buffer_store_b64(pk, rsrc_pm, (int)((off == ZSG_OOB || g != 0) ? ZSG_OOB : off >> 4), 0, 0);
                }
                *(f32x4*)(a + (r0 + RP * j) * LDR + 4 * g) = v;
            }
        } else
#pragma unroll
        for (int j = 0; j < RA; ++j) *(f32x4*)(a + (r0 + RP * j) * LDR + 4 * g) = ra[j];
#pragma unroll
        for (int j = 0; j < RB; ++j) *(f32x4*)(b + (r0 + RP * j) * LDR + 4 * g) = rb[j];
    };

#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    if (n_it > 0) {                      // a parity class of a strided dgrad may have no contributing tap at all
        load_tile(ra[0], rb[0], true, 0);
        store_tile(0, ra[0], rb[0], 0);
#pragma unroll
        for (int st = 0; st < NS - 1; ++st) load_tile(ra[st], rb[st], n_it > st + 1, st);      // tiles 1 .. NS-1 stay in flight
    }
    __syncthreads();

    const int a_row = wm * (BM / WM) + li;
    const int b_row = wn * (BN / WN) + li;

    // one K tile: prefetch tile it+NS into `nxt` (the stage tile `it` has left), MFMA on LDS[it&1], then park tile it+1 (in `cur`,
    // requested NS-1 steps ago) in the other LDS buffer.
    auto k_step = [&](int it, f32x4 (&cur_a)[RA], f32x4 (&cur_b)[RB], f32x4 (&nxt_a)[RA], f32x4 (&nxt_b)[RB], int cur_s, int nxt_s) {
        load_tile(nxt_a, nxt_b, it + NS < n_it, nxt_s);
        const float* a = As + (it & 1) * BM * LDR + a_row * LDR + 4 * lh;
        const float* b = Bs + (it & 1) * BN * LDR + b_row * LDR + 4 * lh;
#pragma unroll
        for (int kk = 0; kk < BK / 8 / KS; ++kk) {
            const int kq = kg * (BK / 8 / KS) + kk;
            f32x4 fa[TM], fb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[i] = *(const f32x4*)(a + i * 32 * LDR + kq * 8);
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j] = *(const f32x4*)(b + j * 32 * LDR + kq * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][e], fb[j][e], acc[i][j], 0, 0, 0);
        }
        store_tile((it + 1) & 1, cur_a, cur_b, cur_s);      // (after the last tile: zeros into the idle buffer)
        __syncthreads();
    };
    for (int it = 0; it < n_it; it += NS) {
#pragma unroll
        for (int st = 0; st < NS; ++st)
            if (it + st < n_it) k_step(it + st, ra[st], rb[st], ra[(st + NS - 1) % NS], rb[(st + NS - 1) % NS], st, (st + NS - 1) % NS);
    }

    // ---- K groups: sum the accumulators into group 0 (fixed order) -----------------------------------------------------------
    if (KS > 1) {
        float* xch = smem;                            // [WM*WN][TM*TN*16][64] — the K-loop tiles are no longer needed
#pragma unroll
        for (int gk = 1; gk < KS; ++gk) {
            if (kg == gk) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int e = 0; e < 16; ++e) xch[(wmn * TM * TN * 16 + (i * TN + j) * 16 + e) * 64 + lane] = acc[i][j][e];
            }
            __syncthreads();
            if (kg == 0) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int e = 0; e < 16; ++e) acc[i][j][e] += xch[(wmn * TM * TN * 16 + (i * TN + j) * 16 + e) * 64 + lane];
            }
            __syncthreads();
        }
    }

    // ---- stream-K hand-off, producer side: a tile's tail is published, then the next pass -----------------------------------------
    if constexpr (!SK) break;
    else {
        if (sk_k0 == 0) break;                        // the head of a tile (or a whole tile): the finishing pass
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        constexpr int NT0 = 64 * WM * WN;             // threads of K group 0 (they hold the accumulators)
        const int t0 = tid % NT0;                     // 16-byte unit q of thread t at ((q * NT0 + t) * 16) bytes of a slot
        if (kg == 0) {
            const rsrc_t rs = make_rsrc(p.sk_ws + (size_t)sk_l * (BM * BN));
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const f32x4 v = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, 16 * ((((i * TN + j) * 4 + q) * NT0) + t0), 0, 16);      // sc1: write-through
                    }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every storing wave drains its own stores ...
        __syncthreads();                                      // ... before the one flag store (also: the staging area is free again)
        if (tid == 0) __hip_atomic_store(p.sk_flags + sk_l, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sk_u += sk_k1 - sk_k0;
        if (sk_u >= sk_u1) return;                    // this workgroup's range ended inside the tile
    }
  }
    // ---- stream-K hand-off, finisher side: the workgroups sk_l + 1 .. last hold the remaining K steps of this cut tile ------------------
    if constexpr (SK) {
        if (sk_k1 < sk_nit) {
            typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
            constexpr int NT0 = 64 * WM * WN;
            constexpr int NQ = TM * TN * 4;
            const int t0 = tid % NT0;
            const int last = ((sk_t + 1) * sk_nit - 1) / p.sk_per;
            if (tid == 0) {
                for (int j = sk_l + 1; j <= last; ++j) {
                    // bounded poll (~1 s): a producer that never arrives (a lost workgroup, a clobbered flag word) must not hang the step —
                    // the finisher gives up, the tile is wrong, and the last flag word says so (ZSG_SK_ERR_WORD; nonzero = poisoned launch)
                    int spins = 0;
                    while (__hip_atomic_load(p.sk_flags + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u && ++spins < (1 << 20)) __builtin_amdgcn_s_sleep(4);
                    if (spins >= (1 << 20)) __hip_atomic_store(p.sk_flags + ZSG_SK_ERR_WORD, 0xdeadu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(p.sk_flags + j, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // zero again for the next launch
                }
            }
            __syncthreads();
            if (kg == 0) {
                for (int j = sk_l + 1; j <= last; ++j) {          // fixed order: deterministic
                    const rsrc_t rs = make_rsrc(p.sk_ws + (size_t)j * (BM * BN));
                    constexpr int QB = NQ < 8 ? NQ : 8;           // 16-byte loads in flight per thread
#pragma unroll
                    for (int q0 = 0; q0 < NQ; q0 += QB) {
                        f32x4 v[QB];
#pragma unroll
                        for (int q = 0; q < QB; ++q) v[q] = __builtin_bit_cast(f32x4, (u32x4)__builtin_amdgcn_raw_buffer_load_b128(rs, 16 * ((q0 + q) * NT0 + t0), 0, 16));
#pragma unroll
                        for (int q = 0; q < QB; ++q)
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[(q0 + q) / (4 * TN)][((q0 + q) / 4) % TN][4 * ((q0 + q) & 3) + e] += v[q][e];
                    }
                }
            }
        }
    }
  {
    // ---- fused BatchNorm statistics: per-column (sum, sum^2) over this tile's rows (dead rows hold exact zeros) -----
    const bool tail_on = p.tail.tickets != nullptr;       // (host: only with the vectorised epilogue, unsplit)
    if (p.stats && !p.bnb.x) {
        float* red = smem;                            // [2][WM][BN] — the K-loop tiles are no longer needed
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float v = acc[i][j][e];
                    s1 += v;
                    s2 += v * v;
                }
            s1 += __shfl_xor(s1, 32, 64);
            s2 += __shfl_xor(s2, 32, 64);
            if (lh == 0 && kg == 0) {
                const int cl = wn * (BN / WN) + j * 32 + li;
                red[wm * BN + cl] = s1;
                red[(WM + wm) * BN + cl] = s2;
            }
        }
        __syncthreads();
        if (tid < BN && n0 + tid < p.N) {
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int w = 0; w < WM; ++w) {
                s1 += red[w * BN + tid];
                s2 += red[(WM + w) * BN + tid];
            }
            float* o = p.stats + (size_t)mt * 2 * p.N;
            if (tail_on) {                            // write-through: another CU's workgroup reduces the rows inside this launch
                bn_tail_store(o + n0 + tid, s1);
                bn_tail_store(o + p.N + n0 + tid, s2);
            } else {
                o[n0 + tid] = s1;
                o[p.N + n0 + tid] = s2;
            }
        }
    }

    // ---- epilogue: bias, residual add, relu, relu-mask ---------------------------------------------------------
    // Fast path (output rows are 16-byte addressable and no split-K): the accumulators are transposed through LDS so
    // that every lane stores 16 contiguous bytes and a row of the tile leaves as one 256-512 B run; the add_src /
    // mask_src operands are read the same way.  (The direct path issues 4-byte accesses in 128-byte runs: measured 3x
    // off the HBM bound on the K=64 1x1 layers.)
    const bool vec_ok = p.vec && (p.splits == 1);
    if (vec_ok) {
        constexpr int LDC = BN + 4;
        float* ct = smem;                             // [BM][LDC] — reuses the K-loop staging area
        static_assert(BM * LDC <= 2 * (BM + BN) * LDR, "the transposed output tile must fit the K-loop staging area (a 256x128 tile does not)");
        constexpr int CG = BN / 4;                    // 16-byte column groups per row
        constexpr int RPP = NT / CG;                  // rows per pass
        constexpr int NR = BM / RPP;                  // rows per thread
        static_assert(BM % RPP == 0, "epilogue row passes");
        const int cg = tid % CG, rr = tid / CG;
        const int n = n0 + 4 * cg;
        const bool bnb = p.bnb.x != nullptr;
        // BatchNorm-backward fusion: this thread's x values and ReLU bits are requested BEFORE the accumulators go through LDS
        // (cold HBM reads: their latency hides behind the transposition instead of ending the block)
        f32x4 xpre[NR], apre[NR];
        unsigned mpre[NR];
        if (bnb) {
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int ro = rowout[rr + RPP * i];
                const bool ok = (ro >= 0) & (n < p.N);
                const size_t o = ok ? (size_t)ro + n : 0;
                xpre[i] = *(const f32x4*)(p.bnb.x + o);
                mpre[i] = p.bnb.mask ? p.bnb.mask[o >> 2] : 0xfu;
                if (p.add_src) apre[i] = *(const f32x4*)(p.add_src + o);      // (accumulate: what earlier consumers left in dout)
            }
        }
        if (p.stats && !p.bnb.x) __syncthreads();     // the statistics block above also used smem
        if (kg == 0) {
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int row = wm * (BM / WM) + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                        ct[row * LDC + wn * (BN / WN) + j * 32 + li] = acc[i][j][e];
                    }
        }
        __syncthreads();
        f32x4 q1 = {0.f, 0.f, 0.f, 0.f}, q2 = {0.f, 0.f, 0.f, 0.f};
        if (n < p.N) {
            f32x4 bv = {0.f, 0.f, 0.f, 0.f}, mu = {0.f, 0.f, 0.f, 0.f}, is = {0.f, 0.f, 0.f, 0.f};
            if (p.bias) bv = *(const f32x4*)(p.bias + n);
            if (bnb) {
                mu = *(const f32x4*)(p.bnb.mean + n);
                is = *(const f32x4*)(p.bnb.invstd + n);
            }
            if (bnb) {                                // (bias / ReLU / float mask are excluded by the host for this mode)
                // pass 1: the values this thread will store (kept in apre[]) and their share of the two sums; the stores themselves
                // follow the partial row and the ticket (pass 2), so the ticket's round trip hides under them
#pragma unroll
                for (int i = 0; i < NR; ++i) {
                    const int row = rr + RPP * i;
                    const int ro = rowout[row];
                    mpre[i] = ro < 0 ? 0u : (mpre[i] | 0x100u);      // bit 8: this row is stored
                    if (ro < 0) continue;
                    f32x4 v = *(const f32x4*)(ct + row * LDC + 4 * cg);
                    if (p.add_src) v += apre[i];
                    f32x4 g = v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) g[e] = ((mpre[i] >> e) & 1u) ? g[e] : 0.f;
                    apre[i] = p.bnb.store_masked ? g : v;
                    q1 += g;
                    q2 += g * ((xpre[i] - mu) * is);
                }
            } else
#pragma unroll 4
            for (int row = rr; row < BM; row += RPP) {
                const int ro = rowout[row];
                if (ro < 0) continue;
                const size_t o = (size_t)ro + n;
                f32x4 v = *(const f32x4*)(ct + row * LDC + 4 * cg) + bv;
                if (p.add_src) v += *(const f32x4*)(p.add_src + o);
                if (p.relu) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                }
                if (p.mask_src) {
                    const f32x4 m = *(const f32x4*)(p.mask_src + o);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = m[e] > 0.f ? v[e] : 0.f;
                }
                *(f32x4*)(p.out + o) = v;
            }
        }
        if (bnb) {                                    // fixed-order (deterministic) reduction over the RPP row lanes
            __syncthreads();                          // every row of ct has been read
            float* red = smem;                        // [2][RPP][BN]
            *(f32x4*)(red + rr * BN + 4 * cg) = q1;
            *(f32x4*)(red + (RPP + rr) * BN + 4 * cg) = q2;
            __syncthreads();
            if (tid < BN && n0 + tid < p.N) {
                float a1 = 0.f, a2 = 0.f;
#pragma unroll 8
                for (int r = 0; r < RPP; ++r) {
                    a1 += red[r * BN + tid];
                    a2 += red[(RPP + r) * BN + tid];
                }
                float* o = p.stats + (size_t)mt * 2 * p.N;
                if (tail_on) {
                    bn_tail_store(o + n0 + tid, a1);
                    bn_tail_store(o + p.N + n0 + tid, a2);
                } else {
                    o[n0 + tid] = a1;
                    o[p.N + n0 + tid] = a2;
                }
            }
            // pass 2: the output stores
            if (n < p.N) {
#pragma unroll
                for (int i = 0; i < NR; ++i)
                    if (mpre[i] & 0x100u) *(f32x4*)(p.out + (size_t)rowout[rr + RPP * i] + n) = apre[i];
            }
        }
        if (tail_on) {
            // in-kernel BatchNorm finalize (bn_tail.h): the storing waves of every tile but the column block's last row tile drain and
            // fire their arrival; the last row tile's workgroup waits for them, reduces the rows and publishes the statistics
            if (mt != p.m_tiles - 1) {
                if (tid < BN) bn_tail_arrive(p.tail.tickets + nt);
            } else {
                __syncthreads();                      // smem (ct / red) is free
                bn_tail_reduce<NT, BN>(p.tail, p.tail.tickets + nt, p.stats, p.m_tiles, p.N, n0, (double*)smem);
            }
        }
    } else if (kg == 0) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * (BN / WN) + j * 32 + li;
        const bool nok = n < p.N;
        const float bv = (p.bias && nok) ? p.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = wm * (BM / WM) + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                const int ro = rowout[row];
                if (ro >= 0 && nok) {
                    const size_t o = (size_t)ro + n;
                    if (p.splits > 1) {          // split-K: every term of the epilogue is linear (no ReLU here)
                        float v = acc[i][j][e];
                        if (split == 0) {
                            v += bv;
                            if (p.add_src && !p.add_is_out) v += p.add_src[o];
                        }
                        if (p.mask_src) v = (p.mask_src[o] > 0.f) ? v : 0.f;
                        unsafeAtomicAdd(p.out + o, v);
                    } else {
                        float v = acc[i][j][e] + bv;
                        if (p.add_src) v += p.add_src[o];
                        if (p.relu) v = fmaxf(v, 0.f);
                        if (p.mask_src) v = (p.mask_src[o] > 0.f) ? v : 0.f;
                        p.out[o] = v;
                    }
                }
            }
        }
    }
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------

static int fill_params(const zsg_conv_desc* d, IgParams& p, int BM, int BN, double* flops) {
    ZSG_REQUIRE(d->nseg >= 1 && d->nseg <= ZSG_MAX_SEG, "conv: nseg=%d", d->nseg);
    ZSG_REQUIRE(d->C > 0 && (d->C % 4) == 0 && (d->src_ld % 4) == 0 && (d->wC % 4) == 0 && (d->wc0 % 4) == 0 &&
                    (d->wt_ld % 4) == 0,
                "conv: C=%d src_ld=%d wC=%d wc0=%d wt_ld=%d must be multiples of 4", d->C, d->src_ld, d->wC, d->wc0, d->wt_ld);
    ZSG_REQUIRE(d->N > 0 && d->B > 0, "conv: N=%d B=%d", d->N, d->B);
    p.C = d->C; p.N = d->N; p.src_ld = d->src_ld; p.out_ld = d->out_ld; p.wS = d->wS; p.wC = d->wC; p.wc0 = d->wc0;
    p.wt_ld = d->wt_ld; p.relu = d->relu; p.nseg = d->nseg;
    int tiles = 0;
    double fl = 0;
    for (int s = 0; s < d->nseg; ++s) {
        const zsg_seg& a = d->seg[s];
        IgSegDev& o = p.seg[s];
        const int64_t rows = (int64_t)d->B * a.rows_y * a.rows_x;
        ZSG_REQUIRE(rows > 0 && rows < (1ll << 30), "conv: seg %d rows=%lld", s, (long long)rows);
        const int64_t src_hi = a.src_off + (int64_t)d->B * a.src_bstride;
        const int64_t out_hi = a.out_off + (int64_t)d->B * a.out_bstride;
        ZSG_REQUIRE(src_hi < (1ll << 29) && out_hi < (1ll << 29), "conv: tensor exceeds 2^29 elements (2 GB window)");
        ZSG_REQUIRE((a.src_off % 4) == 0 && (a.src_bstride % 4) == 0, "conv: seg %d source not 16-byte aligned", s);
        if (d->merge_x)
            ZSG_REQUIRE(d->C == 4 && d->src_ld == 4 && a.tx.n <= 8 && a.tx.dstep == 1 && a.tx.wstep == 1 && d->wC == 4,
                        "conv: merge_x needs C=4, unit x taps, <= 8 taps");
        o.rows_y = a.rows_y; o.rows_x = a.rows_x; o.rows = (int)rows; o.tile0 = tiles;
        o.src_H = a.src_H; o.src_W = a.src_W; o.sy = a.sy; o.sx = a.sx;
        o.out_W = a.out_W; o.osy = a.osy; o.osx = a.osx; o.opy = a.opy; o.opx = a.opx;
        o.src_off = (int)a.src_off; o.src_bstride = (int)a.src_bstride;
        o.out_off = (int)a.out_off; o.out_bstride = (int)a.out_bstride;
        o.ty = a.ty; o.tx = a.tx;
        tiles += cdiv(rows, BM);
        fl += 2.0 * rows * d->N * (double)a.ty.n * a.tx.n * d->C;
    }
    p.m_tiles = tiles;
    p.n_tiles = cdiv(d->N, BN);
    p.remap = 1;
    for (int s = 1; s < d->nseg; ++s)
        if (d->seg[s].ty.n * d->seg[s].tx.n != d->seg[0].ty.n * d->seg[0].tx.n) p.remap = 0;   // unequal K work: keep round-robin
    if (flops) *flops = fl;
    return 0;
}

// kname: the kernel's name as rocprofv3 prints it, so the event-timed profile (zsg_prof_*) and the rocprof trace line up
template <int BM, int BN, int NW, bool MX, int KS, int BK, bool PRE = false, bool SK = false>
static int launch_cfg1(const IgParams& p, hipStream_t st, double flops, const char* kname) {
    const size_t lds = (size_t)2 * (BM + BN) * (BK + 4) * sizeof(float) + BM * sizeof(int);
    static bool attr_done[ZSG_MAX_DEV] = {};      // per device; idempotent (a benign race sets it twice)
    int dev = 0;
    (void)hipGetDevice(&dev);
    ZSG_REQUIRE(dev >= 0 && dev < ZSG_MAX_DEV, "igemm: device %d", dev);
    if (!attr_done[dev]) {
        hipError_t e = hipFuncSetAttribute((const void*)igemm_kernel<BM, BN, NW, MX, KS, BK, PRE, SK>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) ZSG_FAIL(-3, "igemm: hipFuncSetAttribute: %s", hipGetErrorString(e));
        attr_done[dev] = true;
    }
    ZSG_PROF(kname, st, flops, p.alg_bytes);
    ZSG_LAUNCH((igemm_kernel<BM, BN, NW, MX, KS, BK, PRE, SK>), dim3(SK ? p.sk_grid : p.m_tiles * p.n_tiles * p.splits), dim3(64 * NW * KS), lds, st, p);
    ZSG_CHECK_LAUNCH("igemm");
    return 0;
}
// stream-K launch of one tile configuration (profile name = kname + "+sk", + "+k64" for the 64-deep K tile): the workgroup count and
// the units per workgroup follow from the tile; the partial-tile slots and flags come from the stream's workspace
template <int BM, int BN, int NW, int KS, int BK>
static int launch_sk(IgParams& p, hipStream_t st, double flops, const char* kname, int bpc) {
    size_t ws_bytes = 0;
    char* ws = (char*)zsg_stream_workspace(st, &ws_bytes);
    ZSG_REQUIRE(ws, "conv_igemm: a stream-K tile hint needs zsg_set_stream_workspace() for this stream");
    const int tiles = p.m_tiles * p.n_tiles;
    const int grid = ZSG_NUM_CU * bpc;
    const int nit = p.seg[0].ty.n * p.seg[0].tx.n * ((p.C + BK - 1) / BK);
    ZSG_REQUIRE(tiles <= grid && grid < ZSG_SK_ERR_WORD, "conv_igemm: stream-K is for grids below one round (%d tiles, %d workgroups)", tiles, grid);
    if ((size_t)ZSG_SK_FLAG_BYTES + (size_t)grid * BM * BN * sizeof(float) > ws_bytes)
        ZSG_FAIL(-2, "conv_igemm: stream-K needs %zu bytes of stream workspace (%zu registered)", (size_t)ZSG_SK_FLAG_BYTES + (size_t)grid * BM * BN * sizeof(float), ws_bytes);
    p.sk_grid = grid;
    p.sk_per = cdiv((int64_t)tiles * nit, grid);
    p.sk_flags = (unsigned*)ws;
    p.sk_ws = (float*)(ws + ZSG_SK_FLAG_BYTES);
    static char nm[96];
    snprintf(nm, sizeof(nm), "%s+sk%s", kname, BK == 64 ? "+k64" : "");
    return launch_cfg1<BM, BN, NW, false, KS, BK, false, true>(p, st, flops, nm);
}
// p.bk64 selects the 64-deep K tile (profile name = kname + "+k64")
template <int BM, int BN, int NW, bool MX, int KS = 1>
static int launch_cfg(const IgParams& p, hipStream_t st, double flops, const char* kname) {
    if constexpr (!MX) {
        if (p.pre.y) {                   // the BatchNorm-applying loader (32-deep K tiles; profile name = kname + "+pre")
            // (not for the 4-wave 128x128 tile: its 64 accumulator registers + the loader's residual / coefficient stages spill)
            if constexpr (BM * BN >= 128 * 128 && NW * KS <= 4) ZSG_FAIL(-1, "conv_igemm_bnpre: no 4-wave 128x128 variant (use the 8-wave tile)");
            else {
                static char nm[96];
                snprintf(nm, sizeof(nm), "%s+pre", kname);
                return launch_cfg1<BM, BN, NW, MX, KS, IG_BK, true>(p, st, flops, nm);
            }
        }
    }
    if constexpr (!MX) {
        if (p.bk64) {
            static char nm[96];
            snprintf(nm, sizeof(nm), "%s+k64", kname);
            return launch_cfg1<BM, BN, NW, MX, KS, 64>(p, st, flops, nm);
        }
    }
    return launch_cfg1<BM, BN, NW, MX, KS, IG_BK>(p, st, flops, kname);
}

// tile_hint = BM | (BN << 8) | (splits << 16); 0 = heuristic.  The Python lowering autotunes the hint per layer on
// the device (measure, don't guess); the heuristic below is the fallback: blocks go out in rounds of one per CU and the
// 64x64 tile (4 resident blocks per CU) hides latency best.
static void pick_tile(const zsg_conv_desc* d, int* BM, int* BN, int* splits, int* w8) {
    *splits = 1;
    *w8 = 0;
    if (d->tile_hint) {
        *BM = d->tile_hint & 0xff;
        *BN = (d->tile_hint >> 8) & 0xff;
        *splits = (d->tile_hint >> 16) & 0xff;
        *w8 = (d->tile_hint >> 24) & 1;          // 8-wave workgroup variant (64x64: two K groups)
        if (*splits < 1) *splits = 1;
        return;
    }
    static const int cand[3][2] = {{64, 64}, {128, 64}, {128, 128}};
    static const double eff[3] = {1.0, 0.85, 0.82};
    double best = 1e300;
    for (int c = 0; c < 3; ++c) {
        const int bm = cand[c][0], bn = cand[c][1];
        if (bn == 128 && d->N <= 64) continue;
        int64_t tiles = 0;
        for (int s = 0; s < d->nseg; ++s) tiles += cdiv((int64_t)d->B * d->seg[s].rows_y * d->seg[s].rows_x, bm);
        const int64_t blocks = tiles * cdiv(d->N, bn);
        const double cost = (double)cdiv(blocks, ZSG_NUM_CU) * bm * bn / eff[c];
        if (cost < best) {
            best = cost;
            *BM = bm;
            *BN = bn;
        }
    }
}

static int conv_igemm_impl(const zsg_conv_desc* d, const float* src, const float* wt, float* out, const float* bias,
                           const float* add_src, const float* mask_src, float* bn_partials, const BnbDev* bnb, void* stream,
                           const BnTail* tail = nullptr, const IgPre* pre = nullptr) {
    ZSG_REQUIRE(d && src && wt && out, "conv_igemm: null argument");
    int BM = 64, BN = 64, splits = 1, w8 = 0;
    pick_tile(d, &BM, &BN, &splits, &w8);
    if (d->merge_x && BN == 128) BN = 64;
    if (d->merge_x) w8 = 0;
    const int sk_bpc = d->tile_hint ? (d->tile_hint >> 28) & 3 : 0;      // stream-K: workgroups per CU (tile_hint bits 28-29), 0 = off
    const bool sk = sk_bpc > 0;
    if (sk)
        ZSG_REQUIRE(BM != 32 && !d->merge_x && !pre && d->nseg == 1 && splits <= 1,
                    "conv_igemm: stream-K needs an implicit-GEMM tile, one segment, no split-K");
    if (pre) {
        const zsg_seg& s0 = d->seg[0];
        ZSG_REQUIRE(pre->mean && pre->invstd && pre->gamma && pre->beta && pre->residual && pre->y, "conv_igemm_bnpre: null argument");
        ZSG_REQUIRE(d->nseg == 1 && !d->merge_x && s0.ty.n == 1 && s0.tx.n == 1 && s0.ty.d0 == 0 && s0.tx.d0 == 0 && s0.sy == 1 && s0.sx == 1 &&
                        s0.src_H == s0.rows_y && s0.src_W == s0.rows_x && d->src_ld == d->C && s0.src_off == 0 &&
                        s0.src_bstride == (int64_t)s0.src_H * s0.src_W * d->src_ld && d->wc0 == 0 && d->wC == d->C && (d->C % IG_BK) == 0,
                    "conv_igemm_bnpre: a 1x1 / stride-1 convolution over a dense [rows][C] source with C %% 32 == 0");
        ZSG_REQUIRE(BM != 32 && splits <= 1 && !((d->tile_hint >> 27) & 1) && !bnb && !bias && !add_src && !mask_src && !d->relu,
                    "conv_igemm_bnpre: implicit-GEMM tiles with 32-deep K tiles, no split-K, plain epilogue");
        const uintptr_t al = (uintptr_t)pre->mean | (uintptr_t)pre->invstd | (uintptr_t)pre->gamma | (uintptr_t)pre->beta | (uintptr_t)pre->residual | (uintptr_t)pre->y;
        ZSG_REQUIRE((al & 15) == 0, "conv_igemm_bnpre: operands not 16-byte aligned");
    }
    if (BM == 32 && d->merge_x) {                 // the filter-resident streaming kernel of the network's first convolution (mx.hip)
        ZSG_REQUIRE(splits <= 1 && !tail && !bnb, "conv_igemm: the streaming first-layer kernel has no split-K / in-kernel finalize / bnb variant");
        return zsg_conv_mx_launch(d, src, wt, out, bias, add_src, mask_src, bn_partials, (hipStream_t)stream);
    }
    if (BM == 32) {                               // the filter-resident streaming kernel of the 1x1 layers (pw.hip); BN = unit width
        ZSG_REQUIRE(splits <= 1, "conv_igemm: the streaming 1x1 kernel has no split-K variant");
        ZSG_REQUIRE(!tail, "conv_igemm: the streaming 1x1 kernel has no in-kernel BatchNorm finalize (zsg_conv_bn_tail_tickets says so)");
        return zsg_conv_pw_launch(d, BN, src, wt, out, bias, add_src, mask_src, bn_partials, bnb, (hipStream_t)stream);
    }
    IgParams p;
    memset(&p, 0, sizeof(p));
    double flops = 0;
    int rc = fill_params(d, p, BM, BN, &flops);
    if (rc) return rc;
    p.src = src; p.wt = wt; p.out = out; p.bias = bias; p.add_src = add_src; p.mask_src = mask_src;
    p.splits = splits;
    p.add_is_out = (add_src == out) ? 1 : 0;
    p.stats = bn_partials;
    p.alg_bytes = zsg_conv_alg_bytes(d, add_src != nullptr);
    p.bk64 = ((d->tile_hint >> 27) & 1) && !d->merge_x;
    if (pre) {
        p.pre = *pre;
        p.alg_bytes += 4.0 * 2.0 * (double)d->B * d->seg[0].src_H * d->seg[0].src_W * d->C;      // + the residual read and the activation written
    }

    {
        bool v = (d->out_ld % 4) == 0 && (d->N % 4) == 0;
        for (int s = 0; s < d->nseg; ++s) v = v && (d->seg[s].out_off % 4) == 0 && (d->seg[s].out_bstride % 4) == 0;
        const uintptr_t al = (uintptr_t)out | (uintptr_t)bias | (uintptr_t)add_src | (uintptr_t)mask_src;
        p.vec = (v && (al & 15) == 0) ? 1 : 0;
    }
    if (bnb) {
        ZSG_REQUIRE(bn_partials && bnb->x && bnb->mean && bnb->invstd, "conv_igemm_bnb: null argument");
        ZSG_REQUIRE(splits == 1 && p.vec && !bias && !d->relu && !mask_src && !d->merge_x,
                    "conv_igemm_bnb: needs an unsplit, bias-free convolution with 16-byte addressable output rows");
        ZSG_REQUIRE((((uintptr_t)bnb->x | (uintptr_t)bnb->mean | (uintptr_t)bnb->invstd) & 15) == 0, "conv_igemm_bnb: operands not 16-byte aligned");
        p.bnb = *bnb;
        p.bnb.store_masked = d->epi_flags & 1;
    } else if (bn_partials) {
        ZSG_REQUIRE(splits == 1 && !bias && !add_src && !d->relu, "conv_igemm: BN-statistics fusion needs a plain (bias-free, unsplit) convolution");
    }
    if (tail) {
        // (zsg_conv_bn_tail_tickets sizes the ticket words from the hint's column blocks and says -1 without one: the heuristic's tile
        // may have more column blocks than any ticket buffer the caller could have sized)
        ZSG_REQUIRE(d->tile_hint, "conv_igemm: in-kernel BatchNorm finalize needs a tile hint (zsg_conv_bn_tail_tickets says so)");
        ZSG_REQUIRE(tail->tickets && bn_partials && splits == 1 && p.vec && !d->merge_x && p.m_tiles <= BN_TAIL_MAX_ROWS,
                    "conv_igemm: in-kernel BatchNorm finalize needs fused partials, the vectorised epilogue and at most %d row tiles (%d)",
                    BN_TAIL_MAX_ROWS, p.m_tiles);
        ZSG_REQUIRE((((uintptr_t)bn_partials) & 15) == 0 && (d->N % 4) == 0, "conv_igemm: partial rows not 16-byte aligned");
        p.tail = *tail;
        int64_t rows = 0;
        for (int s = 0; s < d->nseg; ++s) rows += (int64_t)d->B * d->seg[s].rows_y * d->seg[s].rows_x;
        p.tail.rows = rows;
    }
    hipStream_t st = (hipStream_t)stream;
    // the tile must exist BEFORE anything is written (the split-K preparation below zeroes the output): a refused launch leaves every
    // output byte as it was.  Every tile that exists has its 8-wave form; merge_x maps any tile field onto its two kernels.
    if (!d->merge_x)
        ZSG_REQUIRE((BM == 64 && BN == 64) || (BM == 128 && (BN == 64 || BN == 128)), "conv_igemm: unsupported tile %dx%d", BM, BN);
    if (splits > 1) {
        ZSG_REQUIRE(!d->relu && d->nseg == 1 && d->out_ld == d->N && d->seg[0].osy == 1 && d->seg[0].osx == 1 &&
                        d->seg[0].out_W == d->seg[0].rows_x && d->seg[0].out_bstride == (int64_t)d->seg[0].rows_y * d->seg[0].rows_x * d->N,
                    "conv_igemm: split-K needs a single dense segment without ReLU");
        if (!p.add_is_out) {
            hipError_t e = hipMemsetAsync(out + d->seg[0].out_off, 0, (size_t)d->B * d->seg[0].out_bstride * sizeof(float), st);
            if (e != hipSuccess) ZSG_FAIL(-3, "conv_igemm: memset: %s", hipGetErrorString(e));
        }
    }
    if (sk) {
        ZSG_REQUIRE(p.vec, "conv_igemm: stream-K needs 16-byte addressable output rows");
        const bool k64 = p.bk64;
        if (BM == 64 && BN == 64 && !w8 && !k64) return launch_sk<64, 64, 4, 1, 32>(p, st, flops, "igemm_kernel<64, 64, 4, false>", sk_bpc);
        if (BM == 64 && BN == 64 && w8 && !k64) return launch_sk<64, 64, 4, 2, 32>(p, st, flops, "igemm_kernel<64, 64, 4, false, 2>", sk_bpc);
        if (BM == 64 && BN == 64 && w8 && k64) return launch_sk<64, 64, 4, 2, 64>(p, st, flops, "igemm_kernel<64, 64, 4, false, 2>", sk_bpc);
        if (BM == 128 && BN == 64 && w8 && !k64) return launch_sk<128, 64, 8, 1, 32>(p, st, flops, "igemm_kernel<128, 64, 8, false>", sk_bpc);
        if (BM == 128 && BN == 128 && w8 && !k64) return launch_sk<128, 128, 8, 1, 32>(p, st, flops, "igemm_kernel<128, 128, 8, false>", sk_bpc);
        if (BM == 128 && BN == 128 && !w8 && !k64) return launch_sk<128, 128, 4, 1, 32>(p, st, flops, "igemm_kernel<128, 128, 4, false>", sk_bpc);
        ZSG_FAIL(-1, "conv_igemm: no stream-K variant for tile %dx%d (w8 %d, k64 %d)", BM, BN, w8, (int)k64);
    }
    if (d->merge_x) {
        if (BM == 128) return launch_cfg<128, 64, 4, true>(p, st, flops, "igemm_kernel<128, 64, 4, true>");
        return launch_cfg<64, 64, 4, true>(p, st, flops, "igemm_kernel<64, 64, 4, true>");
    }
    if (w8 && BM == 64 && BN == 64) {
        return launch_cfg<64, 64, 4, false, 2>(p, st, flops, "igemm_kernel<64, 64, 4, false, 2>");
    }
    if (w8) {
        if (BM == 128 && BN == 128) return launch_cfg<128, 128, 8, false>(p, st, flops, "igemm_kernel<128, 128, 8, false>");
        if (BM == 128 && BN == 64) return launch_cfg<128, 64, 8, false>(p, st, flops, "igemm_kernel<128, 64, 8, false>");
        ZSG_FAIL(-1, "conv_igemm: no 8-wave variant for tile %dx%d", BM, BN);
    }
    if (BM == 128 && BN == 128) return launch_cfg<128, 128, 4, false>(p, st, flops, "igemm_kernel<128, 128, 4, false>");
    if (BM == 128 && BN == 64) return launch_cfg<128, 64, 4, false>(p, st, flops, "igemm_kernel<128, 64, 4, false>");
    if (BM == 64 && BN == 64) return launch_cfg<64, 64, 4, false>(p, st, flops, "igemm_kernel<64, 64, 4, false>");
    ZSG_FAIL(-1, "conv_igemm: unsupported tile %dx%d", BM, BN);
}

extern "C" int zsg_conv_igemm(const zsg_conv_desc* d, const float* src, const float* wt, float* out, const float* bias,
                              const float* add_src, const float* mask_src, float* bn_partials, void* stream) {
    return conv_igemm_impl(d, src, wt, out, bias, add_src, mask_src, bn_partials, nullptr, stream);
}

// The data gradient that COMPLETES dout of a BatchNorm (out = acc [+ add_src]) also emits that BatchNorm's backward partials
// [m_tiles][2][N] = per tile (sum g, sum g * xhat), g = out * relu-bit: zsg_bn_backward_from_partials then needs no pass of
// its own over dout and x for the two sums (reference: autograd's native_batch_norm_backward after the conv's backward).
extern "C" int zsg_conv_igemm_bnb(const zsg_conv_desc* d, const float* src, const float* wt, float* out, const float* add_src,
                                  const float* bn_x, const float* bn_mean, const float* bn_invstd, const uint8_t* bn_relu_mask,
                                  float* partials, void* stream) {
    BnbDev b = {bn_x, bn_mean, bn_invstd, bn_relu_mask};
    return conv_igemm_impl(d, src, wt, out, nullptr, add_src, nullptr, partials, &b, stream);
}

// The 1x1 convolution that CONSUMES a train-mode BatchNorm + residual + ReLU (the next bottleneck's conv1 behind bn3, fpn_resnet.py:
// 86-100) applies it in its operand loader and materialises the activation itself (IgPre): `x` is the previous block's raw conv3
// output.  Optional fused statistics of THIS convolution's output: bn_partials, and (tickets != NULL) their in-kernel finalize
// exactly as zsg_conv_igemm_bnstat.
extern "C" int zsg_conv_igemm_bnpre(const zsg_conv_desc* d, const float* x, const float* wt, float* out, float* bn_partials, uint32_t* tickets,
                                    float* mean, float* invstd, float* running_mean, float* running_var, float momentum, float eps,
                                    const float* pre_mean, const float* pre_invstd, const float* pre_gamma, const float* pre_beta,
                                    const float* pre_residual, float* pre_y, uint8_t* pre_relu_mask, void* stream) {
    IgPre pre = {pre_mean, pre_invstd, pre_gamma, pre_beta, pre_residual, pre_y, pre_relu_mask};
    if (tickets) {
        ZSG_REQUIRE(mean && invstd && bn_partials, "conv_igemm_bnpre: null argument");
        BnTail t;
        memset(&t, 0, sizeof(t));
        t.tickets = tickets; t.mean = mean; t.invstd = invstd; t.rmean = running_mean; t.rvar = running_var;
        t.momentum = momentum; t.eps = eps; t.mode = 0;
        return conv_igemm_impl(d, x, wt, out, nullptr, nullptr, nullptr, bn_partials, nullptr, stream, &t, &pre);
    }
    return conv_igemm_impl(d, x, wt, out, nullptr, nullptr, nullptr, bn_partials, nullptr, stream, nullptr, &pre);
}

// ---- in-kernel BatchNorm finalize (bn_tail.h) ---------------------------------------------------------------------------------
// Column blocks (= ticket words) of the launch this descriptor + tile hint selects, or -1 when that launch cannot finalise the
// statistics itself: no tile hint, the streaming 1x1 kernel, split-K, merge_x, or more than BN_TAIL_MAX_ROWS partial rows per column
// block.  is_wino: the hint is zsg_conv_wino's.
extern "C" int32_t zsg_conv_bn_tail_tickets(const zsg_conv_desc* d, int32_t is_wino) {
    if (!d || !d->tile_hint || ((d->tile_hint >> 16) & 0xff) > 1 || d->merge_x) return -1;
    const int bm = d->tile_hint & 0xff, bn = (d->tile_hint >> 8) & 0xff;
    if (bm <= 0 || bn <= 0) return -1;
    // the vectorised epilogue conv_*_impl requires for the in-kernel finalize: 16-byte addressable output rows (the same
    // predicates here, so that a mismatch is a -1 at lowering time, not a failed launch in the first forward)
    if ((d->out_ld % 4) != 0 || (d->N % 4) != 0) return -1;
    for (int s = 0; s < d->nseg; ++s)
        if ((d->seg[s].out_off % 4) != 0 || (d->seg[s].out_bstride % 4) != 0) return -1;
    int64_t t = 0;
    if (is_wino) {
        if (!((bm == 32 || bm == 64) && (bn == 32 || bn == 64))) return -1;
        for (int s = 0; s < d->nseg; ++s) t += cdiv((int64_t)d->B * ((d->seg[s].src_H + 1) / 2) * ((d->seg[s].src_W + 1) / 2), bm);
    } else {
        if (bm == 32 || !((bm == 64 && bn == 64) || (bm == 128 && (bn == 64 || bn == 128)))) return -1;
        for (int s = 0; s < d->nseg; ++s) t += cdiv((int64_t)d->B * d->seg[s].rows_y * d->seg[s].rows_x, bm);
    }
    if (t > BN_TAIL_MAX_ROWS) return -1;
    return cdiv(d->N, bn);
}

// zsg_conv_igemm with bn_partials whose LAST tile per column block also finalises the BatchNorm statistics: mean / invstd (and the
// running statistics, momentum as torch) are ready when the launch ends — no zsg_bn_stats_from_partials launch, no re-reduction in the
// apply pass.  tickets: zsg_conv_bn_tail_tickets(d, 0) zeroed 32-bit words, left zero.  Reference: nn.BatchNorm2d in training mode
// behind the convolutions of fpn_resnet.py:80-100 (F.batch_norm's statistics pass).
extern "C" int zsg_conv_igemm_bnstat(const zsg_conv_desc* d, const float* src, const float* wt, float* out, float* partials, uint32_t* tickets,
                                     float* mean, float* invstd, float* running_mean, float* running_var, float momentum, float eps, void* stream) {
    ZSG_REQUIRE(tickets && mean && invstd && partials, "conv_igemm_bnstat: null argument");
    BnTail t;
    memset(&t, 0, sizeof(t));
    t.tickets = tickets; t.mean = mean; t.invstd = invstd; t.rmean = running_mean; t.rvar = running_var; t.momentum = momentum; t.eps = eps; t.mode = 0;
    return conv_igemm_impl(d, src, wt, out, nullptr, nullptr, nullptr, partials, nullptr, stream, &t);
}

// zsg_conv_igemm_bnb whose last tile per column block also finalises the BatchNorm BACKWARD sums: coef[0][c] = sum g / n,
// coef[1][c] = sum g xhat / n, d(gamma) / d(beta) written or accumulated — zsg_bn_bwd_apply is all that is left of the BatchNorm's
// backward.  Reference: autograd's native_batch_norm_backward behind the convolution's backward (utils.py:412).
extern "C" int zsg_conv_igemm_bnb_tail(const zsg_conv_desc* d, const float* src, const float* wt, float* out, const float* add_src,
                                       const float* bn_x, const float* bn_mean, const float* bn_invstd, const uint8_t* bn_relu_mask,
                                       float* partials, uint32_t* tickets, float* coef, float* dgamma, float* dbeta, int32_t accumulate,
                                       void* stream) {
    ZSG_REQUIRE(tickets && coef && partials, "conv_igemm_bnb_tail: null argument");
    BnbDev b = {bn_x, bn_mean, bn_invstd, bn_relu_mask};
    BnTail t;
    memset(&t, 0, sizeof(t));
    t.tickets = tickets; t.coef = coef; t.dgamma = dgamma; t.dbeta = dbeta; t.accumulate = accumulate ? 1 : 0; t.mode = 1;
    return conv_igemm_impl(d, src, wt, out, nullptr, add_src, nullptr, partials, &b, stream, &t);
}

