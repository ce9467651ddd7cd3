// igemm_bf16.hip — the eval-only implicit-GEMM convolution on bf16 MFMA (eval_dtype = "bf16" / "bf16_act"), NHWC x packed bf16 weights, gfx950.
//
// Three entries, one kernel template.  zsg_conv_igemm_bf16: activations fp32 in memory (the text below).  zsg_conv_igemm_bf16_m (the
// training plans of train_dtype = "bf16_head": forward convolutions and data gradients of the pyramid and the heads): the same, plus
// igemm.hip's last epilogue term, the ReLU mask of a data gradient (mask_src, the template parameter MK: a compile-time variant of the
// IO = 0 kernel, so the kernels without it keep their code; mask_src == NULL launches the first entry's kernel).  zsg_conv_igemm_bf16_io: each of src /
// out / add_src is fp32 or bf16 in memory (io_flags, the template parameter IO; IO = 0 is the first entry's kernel, instruction for
// instruction the same source path).  With a bf16 src the loader converts nothing: the 8-channel group of a tile row is ONE 16-byte buffer
// load where src_ld and the segment offsets are multiples of 8, else two 8-byte loads (C = 36, src_ld = 36: rows are only 8-byte aligned),
// each half bounds-checked as the fp32 halves are, so the C % 8 == 4 tail zero-fills.  The group goes global -> registers -> LDS like the
// fp32 one (the same one-stage prefetch, half the registers); a direct global -> LDS load was NOT built or timed.  With a bf16 out the
// epilogue rounds once (bf16.h: the packer's conversion) and stores 8-byte groups of 4 channels, or 2 bytes per lane on the scalar path.
// What was timed on the bf16 storage path is in profiles/bf16act_eval_time.txt (whole eval forwards and their per-kernel times; no
// micro-benchmark of the loader alone).
//
// Same GEMM view, descriptor and epilogue as igemm.hip (rows = (segment, b, y, x), n = output channel, K = taps x C walked tap-major):
//      Out[row][n] = relu( sum_{taps} sum_{c<C} bf16(Src[gather(row, tap)][c]) * Wp[n][tap][c]  + bias[n] + add_src[row][n] )
// Activations stay fp32 in memory: the operand loader reads 8 consecutive channels of a tile row (two 16-byte buffer loads), rounds
// them to bf16 (round-to-nearest-even: the compiler's float -> __bf16 conversion, v_cvt_pk_bf16_f32 on gfx950 — the SAME conversion
// the weight packer below uses) and parks them in LDS as one 16-byte write.  Weights come from the packed image
// uint16 [N][T][C8] (zsg_pack_w_bf16_batched; C8 = roundup(C, 8), the channels C..C8-1 are zero), so a tile row of the B operand is one
// 16-byte load and needs no conversion.  Products are accumulated in fp32 by v_mfma_f32_32x32x16_bf16.
//
// MFMA shape: 32x32x16.  Lane (r = lane & 31, h = lane >> 5) holds k = 8h .. 8h+7 of row r — one ds_read_b128 per fragment — and the
// accumulator layout is that of v_mfma_f32_32x32x2_f32, so the epilogue (transposition through LDS, 16-byte stores) is igemm.hip's.
// v_mfma_f32_16x16x32_bf16 was built as a template variant of this kernel (same tiles, same LDS image, 16x16 blocks) and timed against
// it on random data over eight eval shapes of ResNet-50 FPN at B = 16 and all three tiles: 32x32x16 was faster or equal in 19 of 24
// cases, 3.1 % over the sum of each shape's best tile (profiles/bf16_mfma_shape.txt), and the variant was dropped.  The kernel is bound
// by its operand traffic through L2 (fp32 activations: a 64x64 tile moves 24 KB per 0.5 MFLOP), not by the matrix pipe.
// K tile: 64 channels of one tap (bf16: 128 B per row).  LDS rows are padded to 144 B (9 x 16 B: odd), so the b128 fragment reads of 32
// distinct rows are conflict-free, as IG_LDK does for fp32.  A channel tail (C % 64 != 0) is zero-filled by the loaders: the A operand
// by out-of-range buffer offsets per 4-channel group (C % 8 == 4: the upper half of the last group), the B operand by the image's own
// padding up to C8 and out-of-range offsets beyond.
// Pipeline: global -> registers for tile t+1 is issued before the MFMAs of tile t; conversion + registers -> LDS after them into the
// other buffer; one barrier per K tile.  (Two / three register stages of prefetch, as igemm.hip has them, were measured on the same
// shapes: slower on 20 of 24, +4 % over the sum — more registers, and the round trip is not what a K step waits for.)  K order is fixed (tap-major, channels ascending), no split-K, no stream-K, no atomics: the
// same input gives the same bits on every run.
#include <stdlib.h>

#include "bf16.h"

ZSG_DEFINE_PRIO_FLAG()

#define BF_BK 64                // channels per K tile
#define BF_LDR 72               // bf16 elements per LDS tile row (144 B)

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---- weight packer ------------------------------------------------------------------------------------------------------------
struct BfPackJob {
    int64_t src, dst;           // absolute device addresses: fp32 OHWI source, uint16 [N][T][C8] destination
    int32_t N, T, wC, wc0, C, C8, blk0, pad;
};

// one thread per 8-channel group of the destination (16-byte store); a job owns the blocks [blk0, blk0 + ceil(N*T*C8/8 / 256))
__global__ __launch_bounds__(256) void pack_w_bf16_kernel(const BfPackJob* __restrict__ jobs, int njobs) {
    int lo = 0, hi = njobs - 1;
    const int b = blockIdx.x;
    while (lo < hi) {                    // the last job whose blk0 <= b
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].blk0 <= b) lo = mid; else hi = mid - 1;
    }
    const BfPackJob j = jobs[lo];
    const int g8 = j.C8 >> 3;
    const int64_t groups = (int64_t)j.N * j.T * g8;
    const int64_t gi = (int64_t)(b - j.blk0) * 256 + threadIdx.x;
    if (gi >= groups) return;
    const int64_t row = gi / g8;         // n * T + t
    const int c = (int)(gi - row * g8) * 8;
    const float* s = (const float*)j.src + row * j.wC + j.wc0 + c;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (c + e < j.C) ? s[e] : 0.f;
    const u32x4 o = {bf16_pack2(v[0], v[1]), bf16_pack2(v[2], v[3]), bf16_pack2(v[4], v[5]), bf16_pack2(v[6], v[7])};
    *(u32x4*)((uint16_t*)j.dst + row * j.C8 + c) = o;
}

extern "C" int zsg_pack_w_bf16_batched(const void* jobs_dev, int32_t njobs, int32_t total_blocks, void* stream) {
    ZSG_REQUIRE(jobs_dev && njobs > 0 && total_blocks > 0, "pack_w_bf16_batched: jobs=%p njobs=%d total_blocks=%d", jobs_dev, njobs, total_blocks);
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("pack_w_bf16_kernel", st, 0.0, 0.0);
    ZSG_LAUNCH(pack_w_bf16_kernel, dim3(total_blocks), dim3(256), 0, st, (const BfPackJob*)jobs_dev, (int)njobs);
    ZSG_CHECK_LAUNCH("pack_w_bf16_batched");
    return 0;
}

// ---- convolution ----------------------------------------------------------------------------------------------------------------
struct BfSegDev {
    int rows_y, rows_x, rows;   // rows = B*rows_y*rows_x
    int tile0;                  // first M tile of the segment
    int src_H, src_W, sy, sx;
    int out_W, osy, osx, opy, opx;
    int src_off, src_bstride, out_off, out_bstride;   // elements, < 2^31
    zsg_taps ty, tx;
};

struct BfParams {
    const void* src;            // fp32, or bf16 with BF_SRC16
    const uint16_t* wt;         // packed [N][T][C8]
    void* out;                  // fp32, or bf16 with BF_OUT16
    const float* bias;
    const void* add_src;        // fp32, or bf16 with BF_ADD16 (may alias out when both are bf16)
    int C, C8, N, src_ld, out_ld, wS, T, relu, nseg;
    int m_tiles, n_tiles;
    int remap;                  // XCD-aware tile order (only when every segment carries the same amount of K work)
    int vec;                    // 4-channel epilogue groups allowed (alignment of every operand checked on the host)
    double alg_bytes;           // host only
    BfSegDev seg[ZSG_MAX_SEG];
    const float* mask_src;      // MK kernels only: fp32, indexed like out (behind the segments: the other kernels' argument offsets stay)
    float* stats;               // BS kernels only: BatchNorm partials [m_tiles][2][N] of the stored values (behind everything, as mask_src)
    BnbDev bnb;                 // BB kernels only: the BatchNorm whose backward sums go to stats instead (behind everything, as stats)
};

// BM x BN block tile, 4 waves (2 x 2), each wave TM x TN MFMA tiles of 32x32.  Two blocks per CU (at most 256 registers per lane).
// IO: the storage formats of src / out / add_src (BF_SRC16 | BF_OUT16 | BF_ADD16); IO = 0 is the fp32-in-memory kernel of eval_dtype = "bf16".
// BF_SRC8 (with BF_SRC16): the two-halves loader.  A compile-time choice: a run-time branch around the loads made the compiler wait for
// them where the paths join, i.e. in front of the MFMAs they are meant to fly under.
// MK (with IO = 0): the epilogue's last term, out = v * (mask_src[same index] > 0) behind the ReLU — a data gradient into a ReLU's input.
// BS (with IO = 0, no mask, the vectorised epilogue only): behind the output store the tile also writes its BatchNorm partial row,
// stats[mt][0][n] = sum over the tile's valid rows of v, stats[mt][1][n] = sum of v * v, v the fp32 value stored — igemm.hip's bn_partials
// layout.  Order: a thread owns 4 columns and the rows rr, rr + RPP, ... ascending (s += v; q = fma(v, v, q)); the RPP row groups are
// combined through LDS in index order by one thread per column group.  No atomics, nothing between workgroups.
// BB (with IO = 0, no mask, no BS, the vectorised epilogue only): igemm.hip's bnb epilogue — a data gradient that
// completes the dout of a BatchNorm.  v = acc [+ add_src]; g = relu-bit ? v : 0 (bnb.mask, 4 bits per 16-byte group, NULL = all ones);
// stored: v, or g with bnb.store_masked; stats[mt][0][n] = sum g, stats[mt][1][n] = sum g * ((bnb.x - mean) * invstd) over the tile's
// valid rows, in the BS variant's order (s += g; q += g * xhat).  The thread's bnb.x values, bits and add_src values are requested
// before the accumulators go through LDS, as in igemm.hip.
#define BF_SRC8 8
template <int BM, int BN, int IO, bool MK = false, bool BS = false, bool BB = false>
__global__ __launch_bounds__(256, 2) void igemm_bf16_kernel(const BfParams p) {
    static_assert(!MK || IO == 0, "the mask variant is built for fp32 storage only");
    static_assert(!BS || (IO == 0 && !MK), "the BatchNorm-statistics variant is built for fp32 storage without a mask only");
    static_assert(!BB || (IO == 0 && !MK && !BS), "the BatchNorm-backward variant is built for fp32 storage without a mask or forward statistics only");
    ZSG_SET_MAIN_PRIO();
    constexpr int WM = 2, WN = 2, NT = 256;
    constexpr int KG = BF_BK / 8;        // threads (8-channel groups) per tile row
    constexpr int RP = NT / KG;          // tile rows staged per pass (32)
    constexpr int RA = BM / RP;
    constexpr int RB = BN / RP;
    constexpr int TM = BM / WM / 32;
    constexpr int TN = BN / WN / 32;
    constexpr int LDR = BF_LDR;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __bf16* As = (__bf16*)smem_raw;                          // [2][BM][LDR]
    __bf16* Bs = As + 2 * BM * LDR;                          // [2][BN][LDR]
    int* rowout = (int*)(Bs + 2 * BN * LDR);                 // [BM]
    float* smem = (float*)smem_raw;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int g = tid % KG;              // 8-channel group staged by this thread
    const int r0 = tid / KG;             // first staged row
    const int li = lane & 31, lh = lane >> 5;

    const int n_tiles_mn = p.m_tiles * p.n_tiles;
    const int bid = p.remap ? xcd_remap(blockIdx.x, n_tiles_mn) : (int)blockIdx.x;
    const int mt = bid / p.n_tiles;
    const int nt = bid % p.n_tiles;
    int si = 0;
#pragma unroll
    for (int s = 1; s < ZSG_MAX_SEG; ++s)
        if (s < p.nseg && mt >= p.seg[s].tile0) si = s;
    const BfSegDev sg = p.seg[si];
    const int srcH = sg.src_H, srcW = sg.src_W, src_ld = p.src_ld, Cdim = p.C;
    const int m0 = (mt - sg.tile0) * BM;
    const int n0 = nt * BN;

    // ---- per-row gather state (fixed for the whole K loop) ----
    int a_by[RA], a_bx[RA], a_off[RA];
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
        if (g == 0)
            rowout[r0 + RP * j] =
                ok ? sg.out_off + b * sg.out_bstride + ((y * sg.osy + sg.opy) * sg.out_W + (x * sg.osx + sg.opx)) * p.out_ld
                   : -1;
    }
    int b_off[RB];                       // element offset of the weight row in the packed image, or -1 past N
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        const int n = n0 + r0 + RP * j;
        b_off[j] = (n < p.N) ? n * p.T * p.C8 : -1;
    }

    const int n_cc = (Cdim + BF_BK - 1) / BF_BK;
    const int n_jx = sg.tx.n;
    const int n_it = sg.ty.n * n_jx * n_cc;

    const rsrc_t rsrc_a = make_rsrc(p.src);
    const rsrc_t rsrc_b = make_rsrc(p.wt);
    int cc = 0, jx = 0, jy = 0;          // K-iteration counters of the NEXT tile to load (wave-uniform)
    constexpr bool S16 = (IO & BF_SRC16) != 0;
    f32x4 ra[S16 ? 1 : RA][2];           // fp32 source: two 4-channel halves, converted on the way to LDS
    u32x4 rh[S16 ? RA : 1];              // bf16 source: the group as it lies in memory
    u32x4 rb[RB];
    bool hi_dead = false;                // the staged group's upper half lies past C (set by load_tile, applied by store_tile)
    // live == false (past the last K tile): every lane gets an out-of-range offset — the loads still issue and return zeros
    auto load_tile = [&](bool live) {
        const int wr = sg.ty.w0 + jy * sg.ty.wstep;
        const int ws_ = sg.tx.w0 + jx * sg.tx.wstep;
        const int dyy = jy * sg.ty.dstep;
        const int dxx = jx * sg.tx.dstep;
        const int koff = cc * BF_BK + 8 * g;
        const bool k0 = live & (koff < Cdim), k1 = live & (koff + 4 < Cdim);      // the two 4-channel halves of this thread's group
        hi_dead = !k1;
        const int tap = (dyy * srcW + dxx) * src_ld + koff;
#pragma unroll
        for (int j = 0; j < RA; ++j) {
            const int yy = a_by[j] + dyy, xx = a_bx[j] + dxx;
            const bool ok = ((unsigned)yy < (unsigned)srcH) & ((unsigned)xx < (unsigned)srcW);
            if constexpr (S16) {
                const unsigned o = 2u * (unsigned)(a_off[j] + tap);
                if constexpr (!(IO & BF_SRC8)) {      // one 16-byte load; a C % 8 == 4 tail's upper half (it lies inside the row's padding) is
                                                      // dropped in store_tile: touching the loaded value here would wait for the load in front of the MFMAs
                    rh[j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_a, (int)((ok & k0) ? o : ZSG_OOB), 0, 0);
                } else {                 // rows that are only 8-byte aligned (src_ld % 8 == 4): two halves, each bounds-checked by itself
                    const u32x2 lo = __builtin_amdgcn_raw_buffer_load_b64(rsrc_a, (int)((ok & k0) ? o : ZSG_OOB), 0, 0);
                    const u32x2 hi = __builtin_amdgcn_raw_buffer_load_b64(rsrc_a, (int)((ok & k1) ? o + 8u : ZSG_OOB), 0, 0);
                    rh[j] = u32x4{lo[0], lo[1], hi[0], hi[1]};
                }
            } else {
                const unsigned o = 4u * (unsigned)(a_off[j] + tap);
                ra[j][0] = buf_load4(rsrc_a, (ok & k0) ? o : ZSG_OOB);
                ra[j][1] = buf_load4(rsrc_a, (ok & k1) ? o + 16u : ZSG_OOB);
            }
        }
        const int wtap = (wr * p.wS + ws_) * p.C8 + koff;
        const bool kb = live & (koff < p.C8);
#pragma unroll
        for (int j = 0; j < RB; ++j)
            rb[j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_b, (int)((kb & (b_off[j] >= 0)) ? 2u * (unsigned)(b_off[j] + wtap) : ZSG_OOB), 0, 0);
        if (++cc == n_cc) {
            cc = 0;
            if (++jx == n_jx) {
                jx = 0;
                ++jy;
            }
        }
    };
    auto store_tile = [&](int buf) {
        __bf16* a = As + buf * BM * LDR;
        __bf16* b = Bs + buf * BN * LDR;
#pragma unroll
        for (int j = 0; j < RA; ++j) {
            if constexpr (S16) {
                u32x4 v = rh[j];
                if (hi_dead) v[2] = v[3] = 0u;
                *(u32x4*)(a + (r0 + RP * j) * LDR + 8 * g) = v;
            } else {
                const u32x4 v = {bf16_pack2(ra[j][0][0], ra[j][0][1]), bf16_pack2(ra[j][0][2], ra[j][0][3]),
                                 bf16_pack2(ra[j][1][0], ra[j][1][1]), bf16_pack2(ra[j][1][2], ra[j][1][3])};
                *(u32x4*)(a + (r0 + RP * j) * LDR + 8 * g) = v;
            }
        }
#pragma unroll
        for (int j = 0; j < RB; ++j) *(u32x4*)(b + (r0 + RP * j) * LDR + 8 * g) = rb[j];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    if (n_it > 0) {
        load_tile(true);
        store_tile(0);
    }
    __syncthreads();

    const int a_row = wm * (BM / WM) + li;
    const int b_row = wn * (BN / WN) + li;
    for (int it = 0; it < n_it; ++it) {
        load_tile(it + 1 < n_it);        // tile it+1 -> registers
        const __bf16* a = As + (it & 1) * BM * LDR + a_row * LDR + 8 * lh;
        const __bf16* b = Bs + (it & 1) * BN * LDR + b_row * LDR + 8 * lh;
#pragma unroll
        for (int kk = 0; kk < BF_BK / 16; ++kk) {
            bf16x8 fa[TM], fb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[i] = *(const bf16x8*)(a + i * 32 * LDR + kk * 16);
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j] = *(const bf16x8*)(b + j * 32 * LDR + kk * 16);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        store_tile((it + 1) & 1);        // (after the last tile: zeros into the idle buffer)
        __syncthreads();
    }

    // ---- epilogue: bias, residual add, relu (igemm.hip's two paths) ----
    if (p.vec) {
        constexpr int LDC = BN + 4;
        float* ct = smem;                             // [BM][LDC] — reuses the K-loop staging area (rowout lies behind it)
        static_assert(BM * LDC * 4 <= 2 * (BM + BN) * LDR * 2, "the transposed output tile must fit the K-loop staging area");
        constexpr int CG = BN / 4;
        constexpr int RPP = NT / CG;
        static_assert(BM % RPP == 0, "epilogue row passes");
        const int cg = tid % CG, rr = tid / CG;
        const int n = n0 + 4 * cg;
        constexpr int NR = BB ? BM / RPP : 1;         // BB: rows per thread
        [[maybe_unused]] f32x4 xpre[NR], apre[NR];
        [[maybe_unused]] unsigned mpre[NR];
        if constexpr (BB) {
            // cold HBM reads: their latency hides behind the transposition (rows that are not stored read element 0)
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int ro = rowout[rr + RPP * i];
                const bool ok = (ro >= 0) & (n < p.N);
                const size_t o = ok ? (size_t)ro + n : 0;
                xpre[i] = *(const f32x4*)(p.bnb.x + o);
                mpre[i] = p.bnb.mask ? p.bnb.mask[o >> 2] : 0xfu;
                if (p.add_src) apre[i] = *(const f32x4*)((const float*)p.add_src + o);
            }
        }
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int row = wm * (BM / WM) + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                    ct[row * LDC + wn * (BN / WN) + j * 32 + li] = acc[i][j][e];
                }
        __syncthreads();
        [[maybe_unused]] f32x4 bs_s = {0.f, 0.f, 0.f, 0.f}, bs_q = {0.f, 0.f, 0.f, 0.f};
        if (n < p.N) {
            f32x4 bv = {0.f, 0.f, 0.f, 0.f};
            if (p.bias) bv = *(const f32x4*)(p.bias + n);
            if constexpr (BB) {                       // (bias / ReLU / float mask are excluded by the host for this variant)
                const f32x4 mu = *(const f32x4*)(p.bnb.mean + n), is = *(const f32x4*)(p.bnb.invstd + n);
#pragma unroll
                for (int i = 0; i < NR; ++i) {
                    const int row = rr + RPP * i;
                    const int ro = rowout[row];
                    if (ro < 0) continue;
                    f32x4 v = *(const f32x4*)(ct + row * LDC + 4 * cg);
                    if (p.add_src) v += apre[i];
                    f32x4 gv = v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) gv[e] = ((mpre[i] >> e) & 1u) ? gv[e] : 0.f;
                    *(f32x4*)((float*)p.out + (size_t)ro + n) = p.bnb.store_masked ? gv : v;
                    bs_s += gv;
                    bs_q += gv * ((xpre[i] - mu) * is);
                }
            } else
#pragma unroll 4
            for (int row = rr; row < BM; row += RPP) {
                const int ro = rowout[row];
                if (ro < 0) continue;
                const size_t o = (size_t)ro + n;
                f32x4 v = *(const f32x4*)(ct + row * LDC + 4 * cg) + bv;
                if (p.add_src) {
                    if constexpr (IO & BF_ADD16) v += bf16_widen4(*(const u32x2*)((const uint16_t*)p.add_src + o));
                    else v += *(const f32x4*)((const float*)p.add_src + o);
                }
                if (p.relu) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                }
                if constexpr (MK) {
                    const f32x4 m = *(const f32x4*)(p.mask_src + o);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (m[e] > 0.f) ? v[e] : 0.f;
                }
                if constexpr (IO & BF_OUT16) *(u32x2*)((uint16_t*)p.out + o) = bf16_pack4(v);      // rounded once, here
                else *(f32x4*)((float*)p.out + o) = v;
                if constexpr (BS) {
                    bs_s += v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) bs_q[e] = fmaf(v[e], v[e], bs_q[e]);
                }
            }
        }
        if constexpr (BS || BB) {
            // the RPP row groups of a column group meet in LDS (the transposed tile is dead behind the barrier; rowout lies behind it)
            f32x4* red = (f32x4*)smem;                // [RPP][2][CG]
            static_assert(RPP * 2 * CG * 16 <= 2 * (BM + BN) * LDR * 2, "the row-group sums must fit the K-loop staging area");
            __syncthreads();
            red[(rr * 2 + 0) * CG + cg] = bs_s;
            red[(rr * 2 + 1) * CG + cg] = bs_q;
            __syncthreads();
            if (tid < 2 * CG) {
                const int which = tid / CG, c = tid % CG;
                const int nn = n0 + 4 * c;
                f32x4 t = red[which * CG + c];
#pragma unroll
                for (int r = 1; r < RPP; ++r) t += red[(r * 2 + which) * CG + c];
                if (nn < p.N) *(f32x4*)(p.stats + ((size_t)mt * 2 + which) * p.N + nn) = t;
            }
        }
    } else {
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
                        float v = acc[i][j][e] + bv;
                        if (p.add_src) {
                            if constexpr (IO & BF_ADD16) v += bf16_widen1(((const uint16_t*)p.add_src)[o]);
                            else v += ((const float*)p.add_src)[o];
                        }
                        if (p.relu) v = fmaxf(v, 0.f);
                        if constexpr (MK) v = (p.mask_src[o] > 0.f) ? v : 0.f;
                        if constexpr (IO & BF_OUT16) ((uint16_t*)p.out)[o] = bf16_round1(v);
                        else ((float*)p.out)[o] = v;
                    }
                }
            }
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------

// The one list of what the entry accepts: zsg_conv_igemm_bf16_supported and zsg_conv_igemm_bf16 both go through it.  Returns the
// reason as a static string (nullptr: supported) and the tile.
static const char* bf16_check(const zsg_conv_desc* d, int* BM, int* BN) {
    if (!d) return "null descriptor";
    if (d->nseg < 1 || d->nseg > ZSG_MAX_SEG) return "nseg out of range";
    if (d->merge_x) return "merge_x (the stem's streaming kernel stays fp32)";
    if (d->C <= 0 || (d->C % 4) != 0 || (d->src_ld % 4) != 0) return "C and src_ld must be positive multiples of 4";
    if (d->N <= 0 || d->B <= 0 || d->wR <= 0 || d->wS <= 0) return "N, B, wR, wS must be positive";
    if (d->epi_flags) return "epi_flags (BatchNorm-backward epilogues are fp32 only)";
    const int h = d->tile_hint;
    if (h) {
        if (((h >> 16) & 0xff) > 1) return "tile_hint split_k > 1 (no split-K)";
        if ((h >> 28) & 3) return "tile_hint stream-K bits (no stream-K)";
        if ((h >> 24) & 0xf) return "tile_hint variant bits 24-27 (4-wave, 64-channel K tiles only)";
        const int bm = h & 0xff, bn = (h >> 8) & 0xff;
        if (!((bm == 64 && bn == 64) || (bm == 128 && bn == 64) || (bm == 128 && bn == 128))) return "tile_hint tile (64x64, 128x64, 128x128)";
        *BM = bm;
        *BN = bn;
    } else {
        // the library heuristic (igemm.hip's): blocks go out in rounds of one per CU; the cheapest total of rounds x tile area, the
        // smaller tiles favoured (more resident blocks per CU hide latency)
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
    const int64_t C8 = (d->C + 7) / 8 * 8;
    if ((int64_t)d->N * d->wR * d->wS * C8 >= (1ll << 30)) return "packed weight image exceeds 2^30 elements";
    for (int s = 0; s < d->nseg; ++s) {
        const zsg_seg& a = d->seg[s];
        const int64_t rows = (int64_t)d->B * a.rows_y * a.rows_x;
        if (rows <= 0 || rows >= (1ll << 30)) return "segment rows out of range";
        if (a.src_off + (int64_t)d->B * a.src_bstride >= (1ll << 29) || a.out_off + (int64_t)d->B * a.out_bstride >= (1ll << 29))
            return "tensor exceeds 2^29 elements (2 GB window)";
        if ((a.src_off % 4) != 0 || (a.src_bstride % 4) != 0) return "segment source not 16-byte aligned";
        if (a.src_off < 0 || a.out_off < 0 || a.ty.n <= 0 || a.tx.n <= 0) return "segment offsets / taps";
        if (a.ty.w0 < 0 || a.tx.w0 < 0 || a.ty.w0 + (a.ty.n - 1) * a.ty.wstep >= d->wR || a.tx.w0 + (a.tx.n - 1) * a.tx.wstep >= d->wS ||
            a.ty.w0 + (a.ty.n - 1) * a.ty.wstep < 0 || a.tx.w0 + (a.tx.n - 1) * a.tx.wstep < 0)
            return "weight taps outside the wR x wS grid";
    }
    return nullptr;
}

extern "C" int32_t zsg_conv_igemm_bf16_supported(const zsg_conv_desc* d) {
    int bm = 0, bn = 0;
    return bf16_check(d, &bm, &bn) == nullptr ? 1 : 0;
}

// What the storage formats add to bf16_check.  A bf16 source needs what the 8-byte half loads need (C, src_ld and the segment offsets
// multiples of 4: bf16_check's own conditions, which the fp32 loader needs for its 16-byte halves); a bf16 output or add_src of any
// leading dimension is served by the scalar epilogue.  So only the flag word itself can be refused here.
static const char* bf16_io_check(const zsg_conv_desc* d, int32_t io, int* BM, int* BN) {
    if (io < 0 || io > (BF_SRC16 | BF_OUT16 | BF_ADD16)) return "io_flags (SRC_BF16 = 1 | OUT_BF16 = 2 | ADD_BF16 = 4)";
    return bf16_check(d, BM, BN);
}

extern "C" int32_t zsg_conv_igemm_bf16_io_supported(const zsg_conv_desc* d, int32_t io_flags) {
    int bm = 0, bn = 0;
    return bf16_io_check(d, io_flags, &bm, &bn) == nullptr ? 1 : 0;
}

extern "C" int32_t zsg_conv_igemm_bf16_m_supported(const zsg_conv_desc* d) {
    int bm = 0, bn = 0;
    return bf16_check(d, &bm, &bn) == nullptr ? 1 : 0;
}

// What the fused BatchNorm statistics add to bf16_check (the descriptor's share; the pointers are the entry's business): a plain
// convolution whose every operand layout takes the 16-byte epilogue.
static const char* bf16_bn_check(const zsg_conv_desc* d) {
    int bm = 0, bn = 0;
    const char* why = bf16_check(d, &bm, &bn);
    if (why) return why;
    if (d->relu) return "relu (the statistics are those of a plain convolution in front of a BatchNorm)";
    if ((d->N % 4) != 0) return "N must be a multiple of 4 (16-byte partial rows)";
    if ((d->out_ld % 4) != 0) return "out_ld must be a multiple of 4 (the 16-byte epilogue)";
    for (int s = 0; s < d->nseg; ++s)
        if ((d->seg[s].out_off % 4) != 0 || (d->seg[s].out_bstride % 4) != 0) return "segment output not 16-byte aligned (the 16-byte epilogue)";
    return nullptr;
}

extern "C" int32_t zsg_conv_igemm_bf16_bn_supported(const zsg_conv_desc* d) { return bf16_bn_check(d) == nullptr ? 1 : 0; }

// What the BatchNorm-backward epilogue changes in bf16_bn_check: bit 0 of epi_flags is its own (store the masked gradient).  All three
// tiles are served (128x128: 16 rows per thread, 237 registers, no scratch at two blocks per CU).  plain: the descriptor without the bit.
static const char* bf16_bnb_check(const zsg_conv_desc* d, zsg_conv_desc* plain) {
    if (!d) return "null descriptor";
    if (d->epi_flags & ~1) return "epi_flags bits other than bit 0 (store the masked gradient)";
    *plain = *d;
    plain->epi_flags = 0;
    const char* why = bf16_bn_check(plain);
    if (why) return why;
    return nullptr;
}

extern "C" int32_t zsg_conv_igemm_bf16_bnb_supported(const zsg_conv_desc* d) {
    zsg_conv_desc plain;
    return bf16_bnb_check(d, &plain) == nullptr ? 1 : 0;
}

extern "C" int32_t zsg_conv_igemm_bf16_partial_rows(const zsg_conv_desc* d) {
    if (bf16_bn_check(d) != nullptr) return -1;
    int bm = 64, bn = 64;
    (void)bf16_check(d, &bm, &bn);
    int64_t tiles = 0;
    for (int s = 0; s < d->nseg; ++s) tiles += cdiv((int64_t)d->B * d->seg[s].rows_y * d->seg[s].rows_x, bm);
    return (int32_t)tiles;
}

template <int BM, int BN, int IO, bool MK = false, bool BS = false, bool BB = false>
static int launch_bf16(const BfParams& p, hipStream_t st, double flops, const char* kname) {
    const size_t lds = (size_t)2 * (BM + BN) * BF_LDR * sizeof(uint16_t) + BM * sizeof(int);
    static bool attr_done[ZSG_MAX_DEV] = {};      // per device; idempotent (a benign race sets it twice)
    int dev = 0;
    (void)hipGetDevice(&dev);
    ZSG_REQUIRE(dev >= 0 && dev < ZSG_MAX_DEV, "igemm_bf16: device %d", dev);
    if (!attr_done[dev]) {
        hipError_t e = hipFuncSetAttribute((const void*)igemm_bf16_kernel<BM, BN, IO, MK, BS, BB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) ZSG_FAIL(-3, "igemm_bf16: hipFuncSetAttribute: %s", hipGetErrorString(e));
        attr_done[dev] = true;
    }
    ZSG_PROF(kname, st, flops, p.alg_bytes);
    ZSG_LAUNCH((igemm_bf16_kernel<BM, BN, IO, MK, BS, BB>), dim3(p.m_tiles * p.n_tiles), dim3(256), lds, st, p);
    ZSG_CHECK_LAUNCH("igemm_bf16");
    return 0;
}

template <int IO, bool MK = false, bool BS = false>
static int launch_bf16_tile(int BM, int BN, const BfParams& p, hipStream_t st, double fl, const char* n64, const char* n128x64, const char* n128) {
    if (BM == 128 && BN == 128) return launch_bf16<128, 128, IO, MK, BS>(p, st, fl, n128);
    if (BM == 128 && BN == 64) return launch_bf16<128, 64, IO, MK, BS>(p, st, fl, n128x64);
    return launch_bf16<64, 64, IO, MK, BS>(p, st, fl, n64);
}

static int conv_bf16_run(const char* who, const zsg_conv_desc* d, const void* src, const uint16_t* wt_packed, void* out, const float* bias,
                         const void* add_src, int32_t io, void* stream, const float* mask_src = nullptr, float* bn_partials = nullptr,
                         bool want_stats = false, const BnbDev* bnb = nullptr) {
    ZSG_REQUIRE(d && src && wt_packed && out, "%s: null argument", who);
    if (want_stats) {
        const char* why_bn = bf16_bn_check(d);
        ZSG_REQUIRE(why_bn == nullptr, "%s: unsupported: %s", who, why_bn);
        ZSG_REQUIRE(bn_partials && ((uintptr_t)bn_partials & 15) == 0, "%s: bn_partials null or not 16-byte aligned", who);
        ZSG_REQUIRE(((uintptr_t)out & 15) == 0, "%s: out not 16-byte aligned (the BatchNorm statistics ride on the 16-byte epilogue)", who);
    }
    ZSG_REQUIRE(!mask_src || io == 0, "%s: mask_src with io_flags %d (fp32 storage only)", who, io);
    ZSG_REQUIRE(((uintptr_t)mask_src & 3) == 0, "%s: mask_src not element-aligned", who);
    int BM = 64, BN = 64;
    const char* why = bf16_io_check(d, io, &BM, &BN);
    ZSG_REQUIRE(why == nullptr, "%s: unsupported: %s", who, why);
    ZSG_REQUIRE(!(io & BF_ADD16) || add_src, "%s: ADD_BF16 without add_src", who);
    const bool s16 = (io & BF_SRC16) != 0, o16 = (io & BF_OUT16) != 0, a16 = (io & BF_ADD16) != 0;
    ZSG_REQUIRE((((uintptr_t)src & (s16 ? 7 : 15)) | ((uintptr_t)wt_packed & 15)) == 0, "%s: src / wt_packed not aligned (16 bytes; a bf16 src: 8)", who);
    ZSG_REQUIRE(((uintptr_t)out & (o16 ? 1 : 3)) == 0 && ((uintptr_t)add_src & (a16 ? 1 : 3)) == 0, "%s: out / add_src not element-aligned", who);
    ZSG_REQUIRE(add_src != out || a16 == o16, "%s: add_src aliases out in another format", who);
    BfParams p;
    memset(&p, 0, sizeof(p));
    p.src = src; p.wt = wt_packed; p.out = out; p.bias = bias; p.add_src = add_src; p.mask_src = mask_src;
    p.C = d->C; p.C8 = (d->C + 7) / 8 * 8; p.N = d->N; p.src_ld = d->src_ld; p.out_ld = d->out_ld; p.wS = d->wS; p.T = d->wR * d->wS;
    p.relu = d->relu; p.nseg = d->nseg;
    int tiles = 0;
    double fl = 0;
    for (int s = 0; s < d->nseg; ++s) {
        const zsg_seg& a = d->seg[s];
        BfSegDev& o = p.seg[s];
        const int64_t rows = (int64_t)d->B * a.rows_y * a.rows_x;
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
        if (d->seg[s].ty.n * d->seg[s].tx.n != d->seg[0].ty.n * d->seg[0].tx.n) p.remap = 0;
    {
        // 4-channel groups in the epilogue: 16 bytes of fp32, 8 bytes of bf16
        bool v = (d->out_ld % 4) == 0 && (d->N % 4) == 0;
        for (int s = 0; s < d->nseg; ++s) v = v && (d->seg[s].out_off % 4) == 0 && (d->seg[s].out_bstride % 4) == 0;
        const uintptr_t al = ((uintptr_t)out & (o16 ? 7 : 15)) | ((uintptr_t)bias & 15) | ((uintptr_t)add_src & (a16 ? 7 : 15)) | ((uintptr_t)mask_src & 15);
        p.vec = (v && al == 0) ? 1 : 0;
    }
    int kio = io;                // the kernel's template word: the flags + the loader width of a bf16 source
    if (s16) {
        bool w = (d->src_ld % 8) == 0 && ((uintptr_t)src & 15) == 0;
        for (int s = 0; s < d->nseg; ++s) w = w && (d->seg[s].src_off % 8) == 0 && (d->seg[s].src_bstride % 8) == 0;
        if (!w) kio |= BF_SRC8;
    }
    // algorithmic bytes: the activations at their storage width, the filter at 2 bytes per element
    {
        double in_e = 0, out_e = 0;
        for (int s = 0; s < d->nseg; ++s) {
            in_e += (double)d->B * d->seg[s].src_H * d->seg[s].src_W * d->C;
            out_e += (double)d->B * d->seg[s].rows_y * d->seg[s].rows_x * d->N;
        }
        p.alg_bytes = zsg_conv_alg_bytes(d, add_src != nullptr) - 2.0 * (double)d->N * d->seg[0].ty.n * d->seg[0].tx.n * d->C
                      - (s16 ? 2.0 * in_e : 0.0) - (o16 ? 2.0 * out_e : 0.0) - ((a16 && add_src) ? 2.0 * out_e : 0.0);
    }
    hipStream_t st = (hipStream_t)stream;
    if (want_stats) {            // (the partial rows: 8 more bytes per tile row and output channel)
        ZSG_REQUIRE(p.vec, "%s: out / add_src / descriptor do not qualify for the 16-byte epilogue", who);
        p.stats = bn_partials;
        p.alg_bytes += 8.0 * (double)p.m_tiles * d->N;
        if (bnb) {               // (bn_x: 4 more bytes per output element)
            p.bnb = *bnb;
            double out_e = 0;
            for (int s = 0; s < d->nseg; ++s) out_e += (double)d->B * d->seg[s].rows_y * d->seg[s].rows_x * d->N;
            p.alg_bytes += 4.0 * out_e;
            if (BM == 128 && BN == 128) return launch_bf16<128, 128, 0, false, false, true>(p, st, fl, "igemm_bf16_kernel<128, 128, 0, bnb>");
            if (BM == 128) return launch_bf16<128, 64, 0, false, false, true>(p, st, fl, "igemm_bf16_kernel<128, 64, 0, bnb>");
            return launch_bf16<64, 64, 0, false, false, true>(p, st, fl, "igemm_bf16_kernel<64, 64, 0, bnb>");
        }
        return launch_bf16_tile<0, false, true>(BM, BN, p, st, fl, "igemm_bf16_kernel<64, 64, 0, bn>", "igemm_bf16_kernel<128, 64, 0, bn>",
                                                "igemm_bf16_kernel<128, 128, 0, bn>");
    }
    if (mask_src) {              // (the mask reads 4 more bytes per output element)
        double out_e = 0;
        for (int s = 0; s < d->nseg; ++s) out_e += (double)d->B * d->seg[s].rows_y * d->seg[s].rows_x * d->N;
        p.alg_bytes += 4.0 * out_e;
        return launch_bf16_tile<0, true>(BM, BN, p, st, fl, "igemm_bf16_kernel<64, 64, 0, m>", "igemm_bf16_kernel<128, 64, 0, m>",
                                         "igemm_bf16_kernel<128, 128, 0, m>");
    }
    // (the fp32-in-memory kernel keeps the profile names it had; the others carry their flag word, "h" = the two-halves loader)
#define BF_CASE(k, suf)                                                                                                                      \
    case k:                                                                                                                                  \
        return launch_bf16_tile<k>(BM, BN, p, st, fl, "igemm_bf16_kernel<64, 64" suf ">", "igemm_bf16_kernel<128, 64" suf ">",                \
                                   "igemm_bf16_kernel<128, 128" suf ">");
    switch (kio) {
        BF_CASE(0, "")
        BF_CASE(1, ", 1")
        BF_CASE(2, ", 2")
        BF_CASE(3, ", 3")
        BF_CASE(4, ", 4")
        BF_CASE(5, ", 5")
        BF_CASE(6, ", 6")
        BF_CASE(7, ", 7")
        BF_CASE(9, ", 1h")
        BF_CASE(11, ", 3h")
        BF_CASE(13, ", 5h")
        BF_CASE(15, ", 7h")
    }
#undef BF_CASE
    ZSG_FAIL(-1, "%s: io_flags %d", who, io);
}

extern "C" int zsg_conv_igemm_bf16(const zsg_conv_desc* d, const float* src, const uint16_t* wt_packed, float* out, const float* bias,
                                   const float* add_src, void* stream) {
    return conv_bf16_run("conv_igemm_bf16", d, src, wt_packed, out, bias, add_src, 0, stream);
}

extern "C" int zsg_conv_igemm_bf16_m(const zsg_conv_desc* d, const float* src, const uint16_t* wt_packed, float* out, const float* bias,
                                     const float* add_src, const float* mask_src, void* stream) {
    return conv_bf16_run("conv_igemm_bf16_m", d, src, wt_packed, out, bias, add_src, 0, stream, mask_src);
}

extern "C" int zsg_conv_igemm_bf16_io(const zsg_conv_desc* d, const void* src, const uint16_t* wt_packed, void* out, const float* bias,
                                      const void* add_src, int32_t io_flags, void* stream) {
    return conv_bf16_run("conv_igemm_bf16_io", d, src, wt_packed, out, bias, add_src, io_flags, stream);
}

extern "C" int zsg_conv_igemm_bf16_bn(const zsg_conv_desc* d, const float* src, const uint16_t* wt_packed, float* out, float* bn_partials,
                                      void* stream) {
    return conv_bf16_run("conv_igemm_bf16_bn", d, src, wt_packed, out, nullptr, nullptr, 0, stream, nullptr, bn_partials, true);
}

extern "C" int zsg_conv_igemm_bf16_bnb(const zsg_conv_desc* d, const float* src, const uint16_t* wt_packed, float* out, const float* add_src,
                                       const float* bn_x, const float* bn_mean, const float* bn_invstd, const uint8_t* bn_relu_mask,
                                       float* partials, void* stream) {
    static const char* who = "conv_igemm_bf16_bnb";
    zsg_conv_desc plain;
    const char* why = bf16_bnb_check(d, &plain);
    ZSG_REQUIRE(why == nullptr, "%s: unsupported: %s", who, why);
    ZSG_REQUIRE(bn_x && bn_mean && bn_invstd, "%s: bn_x / bn_mean / bn_invstd null", who);
    ZSG_REQUIRE((((uintptr_t)bn_x | (uintptr_t)bn_mean | (uintptr_t)bn_invstd) & 15) == 0, "%s: bn_x / bn_mean / bn_invstd not 16-byte aligned", who);
    ZSG_REQUIRE(partials && ((uintptr_t)partials & 15) == 0, "%s: partials null or not 16-byte aligned", who);
    const BnbDev b = {bn_x, bn_mean, bn_invstd, bn_relu_mask, d->epi_flags & 1};
    return conv_bf16_run(who, &plain, src, wt_packed, out, nullptr, add_src, 0, stream, nullptr, partials, true, &b);
}
