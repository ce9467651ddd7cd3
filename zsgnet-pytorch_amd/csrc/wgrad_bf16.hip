// wgrad_bf16.hip — convolution weight gradient on bf16 MFMA (v_mfma_f32_32x32x16_bf16, fp32 accumulation), gfx950.
// wgrad_dtype = "bf16": zsg_conv_wgrad's descriptor, GEMM view, split-K slabs and deterministic reduction (wgrad.hip, wgrad_common.h):
//   dW[n][col] += sum_rows bf16(dY[row][n]) * bf16(Src[gather(row, tap(col))][c(col)])
//   n = output channel -> M,   col = (tap, c) tap-major -> N,   rows = (segment, b, y, x) pixels of dY -> K, 32 pixels per K tile.
// src, dy and dw stay fp32 in memory; the operand loader rounds every element to bf16 (round-to-nearest-even, bf16.h) on its way to LDS.
//
// LDS image.  Both operands are contiguous along the GEMM's M / N index in memory (a pixel row holds all channels) and strided along
// K (the pixels), but a bf16 MFMA lane needs 8 consecutive K values of ONE m.  The tile is transposed while it is written to LDS: a
// thread loads RPT = BM/32 consecutive pixel rows of one 16-byte channel group (4 channels), converts, and stores for each of the 4
// channels its RPT pixels packed (8 or 4 bytes) into a [m][k] image of 32 bf16 per row, padded to WB_LDK = 40 (80 bytes).  The MFMA
// operand is then one 16-byte row read, as in igemm_bf16.hip.  Banks:
//   - reads (ds_read_b128, 64 banks): lane li reads row m0 + li at byte 16*lh + 32*kk; 80 bytes = 5 slots of 16 bytes, 5 is coprime
//     with the 16 slots of a bank row, so 16 consecutive rows cover 16 distinct slots: conflict-free;
//   - writes (32 banks): the threads of a wave run along K first (tid % KQ), so the wave writes 64 contiguous bytes (16 banks) of each
//     of 8 (4) rows whose starts alternate between banks 0 and 16 (4 rows x 80 bytes = 320 bytes = 16 banks mod 32): every bank gets
//     the minimum number of distinct addresses of a 512-byte (256-byte) store.
// The alternative of staging [k][m] rows and reading them with ds_read_b64_tr_b16 was not built: with it a ragged tile needs padding
// instead of masked lanes and the conversion cost is the same.  The price of the K-first lane order is on the global side: one load
// instruction of a wave touches 16 (8) pixel rows with 64 (128) contiguous bytes each instead of whole rows; WB_ROW_LOADS builds the
// row-contiguous order (conflicting LDS stores) for an A/B — which is faster is not measured yet (profiles/wgrad_bf16_step_time.txt).
//
// Zero fill: a tap outside the image, a pixel row beyond a segment's last and a channel group beyond N / ncols are buffer loads with
// an out-of-range offset (zeros, no memory touched); the channels of dy's last 16-byte group beyond N (N = 45 in a 48-wide row) are
// replaced by +0 with a select before the conversion, so no value from there can enter an MFMA.
#include "bf16.h"
#include "wgrad_common.h"

#define WB_BK 32      // pixel rows per K tile (two MFMA K steps of 16)
#define WB_LDK 40     // bf16 elements per LDS row: 32 + 8 padding (80 bytes)

typedef __bf16 wb_bf16x8 __attribute__((ext_vector_type(8)));

// Block tile BM x BN (each 64 or 128) by 2 x 2 waves, each TM x TN MFMA tiles of 32x32; 256 threads.
template <int BM, int BN>
__global__ __launch_bounds__(256, 2) void wgrad_bf16_kernel(const WgParams p) {
    constexpr int TM = BM / 64, TN = BN / 64;
    constexpr int RA = BM / 32, KQA = WB_BK / RA;      // A staging: pixel rows per thread, threads along K
    constexpr int RB = BN / 32, KQB = WB_BK / RB;
    __shared__ __attribute__((aligned(16))) uint16_t As[2][BM][WB_LDK];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[2][BN][WB_LDK];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, lh = lane >> 5;

    const int nmn = p.m_tiles * p.n_tiles;
    const int split = blockIdx.x / nmn;
    const int mn = xcd_remap(blockIdx.x % nmn, nmn);
    const int mt = mn / p.n_tiles, nt = mn % p.n_tiles;
    const int m0 = mt * BM, n0 = nt * BN;
    const int kt_begin = split * p.kt_chunk;
    const int kt_end = min(p.kt_total, kt_begin + p.kt_chunk);

    // ---- fixed per-thread column state -----------------------------------------------------------------------
#ifdef WB_ROW_LOADS      // A/B build (make EXTRA=-DWB_ROW_LOADS): lanes run along the channels first — row-contiguous global loads, conflicting LDS writes
    const int ka = (tid / (BM / 4)) * RA, ga = tid % (BM / 4);
    const int kb = (tid / (BN / 4)) * RB, gb = tid % (BN / 4);
#else
    const int ka = (tid % KQA) * RA, ga = tid / KQA;      // first pixel row inside the K tile, 16-byte channel group
    const int kb = (tid % KQB) * RB, gb = tid / KQB;
#endif
    const int na = m0 + 4 * ga;                    // first dY channel of this thread's group
    const bool a_colok = na < p.N;
    const int q = n0 + 4 * gb;                     // first logical weight column of this thread's group (ncols % 4 == 0: all or none)
    const bool b_colok = q < p.ncols;
    int b_dy, b_dx, b_c;
    {
        const int qq = b_colok ? q : 0;
        const int tapi = qq / p.C;
        b_c = qq - tapi * p.C;
        const int jy = tapi / p.txn, jx = tapi - jy * p.txn;
        b_dy = p.ty.d0 + jy * p.ty.dstep;
        b_dx = p.tx.d0 + jx * p.tx.dstep;
    }
    const rsrc_t rs_a = make_rsrc(p.dy);
    const rsrc_t rs_b = make_rsrc(p.src);

    int si = 0;
#pragma unroll
    for (int s = 1; s < ZSG_MAX_SEG; ++s)
        if (s < p.nseg && kt_begin >= p.seg[s].kt0) si = s;
    WgSegDev sg = p.seg[si];
    int kt_next = kt_begin;

    // register stages: the global loads run 2 K tiles ahead (wgrad.hip's pipeline)
    constexpr int NS = 2;
    f32x4 ra[NS][RA], rb[NS][RB];
    // live == false (past this block's last K tile): every lane gets an out-of-range offset — zeros, no memory touched, no branch
    auto load_tile = [&](f32x4 (&ra)[RA], f32x4 (&rb)[RB], bool live) {
        if (si + 1 < p.nseg && kt_next >= p.seg[si + 1].kt0) {     // wave-uniform segment switch
            ++si;
            sg = p.seg[si];
        }
        const int rbase = (kt_next - sg.kt0) * WB_BK;
        const int per = sg.rows_y * sg.rows_x;
#pragma unroll
        for (int j = 0; j < RA; ++j) {
            const int r = rbase + ka + j;
            const bool rok = live & (r < sg.rows);
            const int rr = rok ? r : 0;
            int b = fdiv(rr, per, sg.inv_per);
            int rem = rr - mul24(b, per);
            int y = fdiv(rem, sg.rows_x, sg.inv_rx);
            int x = rem - mul24(y, sg.rows_x);
            const unsigned off = 4u * (unsigned)(sg.out_off + mul24(b, sg.out_bstride) +
                                                  mul24(mul24(mul24(y, sg.osy) + sg.opy, sg.out_W) + (mul24(x, sg.osx) + sg.opx), p.out_ld) + na);
            ra[j] = buf_load4(rs_a, (rok & a_colok) ? off : ZSG_OOB);
        }
#pragma unroll
        for (int j = 0; j < RB; ++j) {
            const int r = rbase + kb + j;
            const bool rok = live & (r < sg.rows);
            const int rr = rok ? r : 0;
            int b = fdiv(rr, per, sg.inv_per);
            int rem = rr - mul24(b, per);
            int y = fdiv(rem, sg.rows_x, sg.inv_rx);
            int x = rem - mul24(y, sg.rows_x);
            const int yy = mul24(y, sg.sy) + b_dy, xx = mul24(x, sg.sx) + b_dx;
            const bool ok = rok & b_colok & ((unsigned)yy < (unsigned)sg.src_H) & ((unsigned)xx < (unsigned)sg.src_W);
            const unsigned off = 4u * (unsigned)(sg.src_off + mul24(b, sg.src_bstride) + mul24(mul24(yy, sg.src_W) + xx, p.src_ld) + b_c);
            rb[j] = buf_load4(rs_b, ok ? off : ZSG_OOB);
        }
        ++kt_next;
    };
    // convert + transpose: channel e of the thread's group gets its R pixel rows packed at [m][k .. k+R-1]
    auto store_tile = [&](int buf, const f32x4 (&ra)[RA], const f32x4 (&rb)[RB]) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool ok = na + e < p.N;          // dy's row padding beyond N never reaches the operand
            if constexpr (RA == 4) {
                const u32x2 v = {bf16_pack2(ok ? ra[0][e] : 0.f, ok ? ra[1][e] : 0.f), bf16_pack2(ok ? ra[2][e] : 0.f, ok ? ra[3][e] : 0.f)};
                *(u32x2*)&As[buf][4 * ga + e][ka] = v;
            } else {
                *(unsigned*)&As[buf][4 * ga + e][ka] = bf16_pack2(ok ? ra[0][e] : 0.f, ok ? ra[1][e] : 0.f);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if constexpr (RB == 4) {
                const u32x2 v = {bf16_pack2(rb[0][e], rb[1][e]), bf16_pack2(rb[2][e], rb[3][e])};
                *(u32x2*)&Bs[buf][4 * gb + e][kb] = v;
            } else {
                *(unsigned*)&Bs[buf][4 * gb + e][kb] = bf16_pack2(rb[0][e], rb[1][e]);
            }
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int n_kt = kt_end - kt_begin;
    if (n_kt > 0) {
        load_tile(ra[0], rb[0], true);
        store_tile(0, ra[0], rb[0]);
        load_tile(ra[0], rb[0], n_kt > 1);
    }
    __syncthreads();

    // MFMA sub-tile i of a wave covers rows m = wm*32*TM + 32*i + li (columns likewise); lane half lh holds K 8*lh .. 8*lh+7 of a step
    const int am = wm * (32 * TM) + li;
    const int bn = wn * (32 * TN) + li;
    auto k_step = [&](int it, f32x4 (&cur_a)[RA], f32x4 (&cur_b)[RB], f32x4 (&nxt_a)[RA], f32x4 (&nxt_b)[RB]) {
        const int buf = it & 1;
        load_tile(nxt_a, nxt_b, it + NS < n_kt);
        __builtin_amdgcn_sched_barrier(0);           // keep the global loads ahead of the MFMA phase
#pragma unroll
        for (int kk = 0; kk < WB_BK / 16; ++kk) {
            wb_bf16x8 fa[TM], fb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[i] = *(const wb_bf16x8*)&As[buf][am + 32 * i][16 * kk + 8 * lh];
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j] = *(const wb_bf16x8*)&Bs[buf][bn + 32 * j][16 * kk + 8 * lh];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        store_tile(buf ^ 1, cur_a, cur_b);           // (after the last tile: zeros into the idle buffer)
        __syncthreads();
    };
    for (int it = 0; it < n_kt; it += NS) {
#pragma unroll
        for (int st = 0; st < NS; ++st)
            if (it + st < n_kt) k_step(it + st, ra[st], rb[st], ra[(st + NS - 1) % NS], rb[(st + NS - 1) % NS]);
    }
    if (kt_begin >= kt_end) return;

    // ---- epilogue: D[i][j] -> (n = output channel, q = logical weight column); 32 lanes store 32 consecutive columns ------------
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int qc = n0 + wn * (32 * TN) + 32 * j + li;
        const bool cok = qc < p.ncols;
        size_t coff;
        if (p.ws) {
            coff = (size_t)split * p.N * p.ncols + qc;
        } else {
            const int qq = cok ? qc : 0;
            const int tapi = qq / p.C;
            const int c = qq - tapi * p.C;
            const int jy = tapi / p.txn, jx = tapi - jy * p.txn;
            const int wr = p.ty.w0 + jy * p.ty.wstep, ws_ = p.tx.w0 + jx * p.tx.wstep;
            coff = (size_t)((wr * p.wS + ws_) * p.wC + p.wc0 + c);
        }
        const int ld = p.ws ? p.ncols : p.wt_ld;
        float* dst = p.ws ? p.ws : p.dw;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int n = m0 + wm * (32 * TM) + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (cok && n < p.N) {
                    float* o = dst + (size_t)n * ld + coff;
                    *o = (!p.ws && p.accumulate) ? *o + acc[i][j][e] : acc[i][j][e];
                }
            }
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------

// The one list of what the entry accepts: zsg_conv_wgrad_bf16_supported and zsg_conv_wgrad_bf16 both go through it.  Returns the reason
// as a static string (nullptr: supported), the tile and the requested split count (0: heuristic).
static const char* wgrad_bf16_check(const zsg_conv_desc* d, int* BM, int* BN, int* want_splits) {
    if (!d) return "null descriptor";
    if (d->nseg < 1 || d->nseg > ZSG_MAX_SEG) return "nseg out of range";
    if (d->merge_x) return "merge_x (the stem's weight gradient stays fp32)";
    if (d->C <= 0 || (d->C % 4) != 0 || (d->src_ld % 4) != 0 || (d->wC % 4) != 0 || (d->wc0 % 4) != 0)
        return "C, src_ld, wC and wc0 must be multiples of 4";
    if (d->N <= 0 || d->B <= 0) return "N and B must be positive";
    if (d->out_ld <= 0 || (d->out_ld % 4) != 0) return "out_ld must be a multiple of 4 (16-byte dy rows)";
    const int h = d->tile_hint;
    *want_splits = 0;
    if (h) {
        if ((h >> 24) & 0xf) return "tile_hint variant bits 24-27";
        if ((h >> 28) & 0xf) return "tile_hint bits 28-31";
        const int bm = h & 0xff, bn = (h >> 8) & 0xff;
        if (bn == 255) return "tile_hint BN field 255 (the 256-column tile is fp32 only)";
        if ((bm != 64 && bm != 128) || (bn != 64 && bn != 128)) return "tile_hint tile (BM, BN out of 64, 128)";
        *BM = bm;
        *BN = bn;
        *want_splits = (h >> 16) & 0xff;
    } else {
        *BM = d->N > 64 ? 128 : 64;
        *BN = (int64_t)d->seg[0].ty.n * d->seg[0].tx.n * d->C > 64 ? 128 : 64;
    }
    if (d->src_ld >= (1 << 23) || d->out_ld >= (1 << 23)) return "a row pitch exceeds 2^23";
    if ((int64_t)d->N * d->seg[0].ty.n * d->seg[0].tx.n * d->C >= (1ll << 30)) return "weight gradient exceeds 2^30 elements";
    for (int s = 0; s < d->nseg; ++s) {
        const zsg_seg& a = d->seg[s];
        if (memcmp(&a.ty, &d->seg[0].ty, sizeof(zsg_taps)) != 0 || memcmp(&a.tx, &d->seg[0].tx, sizeof(zsg_taps)) != 0)
            return "segments must share one tap structure (pass the forward descriptor)";
        if (a.ty.n <= 0 || a.tx.n <= 0) return "segment taps";
        const int64_t rows = (int64_t)d->B * a.rows_y * a.rows_x;
        if (rows <= 0 || rows >= (1ll << 24)) return "segment rows (must be positive and < 2^24)";
        if (a.src_off < 0 || a.out_off < 0) return "segment offsets";
        if (a.src_off + (int64_t)d->B * a.src_bstride >= (1ll << 29) || a.out_off + (int64_t)d->B * a.out_bstride >= (1ll << 29))
            return "tensor exceeds 2^29 elements (2 GB window)";
        if ((a.src_off % 4) != 0 || (a.src_bstride % 4) != 0) return "segment source not 16-byte aligned";
        if ((a.out_off % 4) != 0 || (a.out_bstride % 4) != 0) return "segment dy not 16-byte aligned";
        if ((int64_t)a.src_H * a.src_W >= (1 << 23) || (int64_t)(a.rows_y * a.osy + a.opy + 1) * a.out_W >= (1 << 23))
            return "a per-image pixel count exceeds 2^23";
        if (a.src_bstride >= (1 << 23) || a.out_bstride >= (1 << 23)) return "image stride >= 2^23 (the fp32 entry's wide fallback)";
    }
    return nullptr;
}

extern "C" int32_t zsg_conv_wgrad_bf16_supported(const zsg_conv_desc* d) {
    int bm = 0, bn = 0, sp = 0;
    return wgrad_bf16_check(d, &bm, &bn, &sp) == nullptr ? 1 : 0;
}

extern "C" int zsg_conv_wgrad_bf16(const zsg_conv_desc* d, const float* src, const float* dy, float* dw, int32_t accumulate, void* ws,
                                   size_t ws_bytes, void* stream) {
    ZSG_REQUIRE(d && src && dy && dw, "conv_wgrad_bf16: null argument");
    int BM = 0, BN = 0, want_splits = 0;
    const char* why = wgrad_bf16_check(d, &BM, &BN, &want_splits);
    ZSG_REQUIRE(why == nullptr, "conv_wgrad_bf16: not supported: %s", why);
    WgParams p;
    memset(&p, 0, sizeof(p));
    p.src = src; p.dy = dy; p.dw = dw; p.accumulate = accumulate ? 1 : 0;
    p.C = d->C; p.N = d->N; p.src_ld = d->src_ld; p.out_ld = d->out_ld; p.wS = d->wS; p.wC = d->wC; p.wc0 = d->wc0;
    p.wt_ld = d->wt_ld; p.nseg = d->nseg;
    p.ty = d->seg[0].ty; p.tx = d->seg[0].tx;
    p.txn = p.tx.n;
    p.ncols = p.ty.n * p.tx.n * d->C;
    p.bk = WB_BK;
    int kt = 0;
    double rows_all = 0;
    for (int s = 0; s < d->nseg; ++s) {
        const zsg_seg& a = d->seg[s];
        const int64_t rows = (int64_t)d->B * a.rows_y * a.rows_x;
        WgSegDev& o = p.seg[s];
        o.rows_y = a.rows_y; o.rows_x = a.rows_x; o.rows = (int)rows; o.kt0 = kt;
        o.src_H = a.src_H; o.src_W = a.src_W; o.sy = a.sy; o.sx = a.sx;
        o.out_W = a.out_W; o.osy = a.osy; o.osx = a.osx; o.opy = a.opy; o.opx = a.opx;
        o.src_off = (int)a.src_off; o.src_bstride = (int)a.src_bstride;
        o.out_off = (int)a.out_off; o.out_bstride = (int)a.out_bstride;
        o.inv_per = 1.0f / (float)(a.rows_y * a.rows_x);
        o.inv_rx = 1.0f / (float)a.rows_x;
        kt += cdiv(rows, WB_BK);                  // K tiles never straddle a segment
        rows_all += (double)rows;
    }
    p.kt_total = kt;
    p.m_tiles = cdiv(d->N, BM);
    p.n_tiles = cdiv(p.ncols, BN);
    const int nmn = p.m_tiles * p.n_tiles;
    // heuristic (wgrad.hip's): two blocks per CU, at least two K tiles per slice, at most 64 slices
    int splits = want_splits > 0 ? want_splits : (2 * ZSG_NUM_CU + nmn - 1) / nmn;
    if (splits > 64 && want_splits <= 0) splits = 64;
    if (splits > kt / 2) splits = kt / 2;
    if (splits < 1) splits = 1;
    p.kt_chunk = cdiv(kt, splits);
    p.splits = cdiv(kt, p.kt_chunk);              // every slice holds at least one K tile: every slab is written in full
    if (p.splits > 1) {
        const size_t need = (size_t)p.splits * d->N * p.ncols * sizeof(float);
        if (!ws || ws_bytes < need) ZSG_FAIL(-2, "conv_wgrad_bf16: workspace too small (%zu < %zu bytes)", ws_bytes, need);
        p.ws = (float*)ws;
    }
    hipStream_t st = (hipStream_t)stream;
    const double wg_flops = 2.0 * rows_all * d->N * p.ncols;
    const double wg_bytes = zsg_conv_alg_bytes(d, accumulate != 0);
    const dim3 grid(nmn * p.splits);
#define WB_LAUNCH(BM_, BN_)                                                                     \
    do {                                                                                        \
        ZSG_PROF("wgrad_bf16_kernel<" #BM_ ", " #BN_ ">", st, wg_flops, wg_bytes);                \
        ZSG_LAUNCH((wgrad_bf16_kernel<BM_, BN_>), grid, dim3(256), 0, st, p);                    \
    } while (0)
    if (BM == 128 && BN == 128) WB_LAUNCH(128, 128);
    else if (BM == 128) WB_LAUNCH(128, 64);
    else if (BN == 128) WB_LAUNCH(64, 128);
    else WB_LAUNCH(64, 64);
#undef WB_LAUNCH
    if (p.splits > 1) {
        WgReduceJob j;
        wg_reduce_job_fill(j, d, p.ws, dw, p.accumulate, p.splits);
        wg_reduce_launch(j, st);
    }
    ZSG_CHECK_LAUNCH("conv_wgrad_bf16");
    return 0;
}
