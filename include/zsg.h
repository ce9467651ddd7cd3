/*
 * zsg.h — C ABI of libzsg.so: the MI355X (gfx950) HIP kernels behind the ZSGNet training step.
 *
 * Drop-in boundary.  The reference (TheShadow29/zsgnet-pytorch) is pure Python on PyTorch and has
 * NO native interface of its own: every device kernel it runs is an implicit nn / F / torch call.  Each entry
 * point below therefore cites the reference call site whose implicit PyTorch/cuDNN kernel(s) it replaces.  The host
 * side (the Python modules of zsgnet-pytorch_amd) mirrors the reference's nn.Module / loss / evaluator signatures and binds these
 * symbols with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain pointers and sizes only; no torch types.  All tensors are fp32 unless stated, device memory owned by the
 *     caller (PyTorch): the library never allocates, frees or retains device memory.
 *   - activations are NHWC ("pixel-major"): element (b,y,x,c) at  off + b*bstride + (y*W + x)*ld + c.
 *     weights are OHWI: element (co,r,s,ci) at ((co*R + r)*S + s)*C + ci   (== torch channels_last of an OIHW tensor).
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), re-entrant, and never synchronises.
 *   - return 0 on success, <0 on error: -1 bad argument/shape, -2 workspace too small, -3 HIP error, -4 RCCL error.
 *     zsg_last_error() returns a thread-local message.  Nothing throws across the ABI.
 */
#ifndef ZSG_H
#define ZSG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZSG_VERSION 100
#define ZSG_MAX_SEG 8

int zsg_version(void);
/* sha256 stamp (16 hex digits) of the kernel sources this library was BUILT from (csrc/stamp.py): the host ties the shipped tuning
 * table and the committed rocprof summaries to the library that is actually loaded (ZSG_LIB_PATH may point at another build), not to the
 * source files lying next to it.  No reference counterpart (the reference has no tuned native kernels). */
const char* zsg_source_stamp(void);
const char* zsg_last_error(void);
/* on != 0: the column-sum kernels (bias gradients, the head's border sums) use one block per output element group
 * instead of combining block partials with fp32 atomics, so every kernel of the library sums in a fixed order
 * (convolution split-K with atomics is only ever requested through tile_hint: the host tuner does not offer it in this
 * mode).  Process-global; the Python binding sets it from ZSG_DETERMINISTIC=1. */
int zsg_set_deterministic(int32_t on);

/* ---------------------------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution family (fp32 MFMA v_mfma_f32_32x32x2_f32).
 * Replaces nn.Conv2d forward and its autograd backward at: encoder mdl.py:149-156 (-> fpn_resnet.py:80-100),
 * FPN fpn_resnet.py:157-172, head mdl.py:379-380, SSD ssd_vgg.py:72-95; LSTM input projection (mdl.py:227).
 *
 * One launch covers up to ZSG_MAX_SEG "segments" that share weights / channel counts but have their own geometry
 * (pyramid levels of the shared head; stride-parity classes of a strided dgrad).  A segment enumerates output rows
 * (b, y, x) over rows_y x rows_x per image; row (b,y,x) and tap (jy,jx) gather the source pixel
 *      (y*sy + ty.d0 + jy*ty.dstep,  x*sx + tx.d0 + jx*tx.dstep)      (zero outside [0,src_H) x [0,src_W))
 * and multiply it with weight tap (ty.w0 + jy*ty.wstep, tx.w0 + jx*tx.wstep).  The row is stored at output pixel
 *      (y*osy + opy, x*osx + opx) of an out_W-wide image.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n;      /* taps along this axis                      */
    int32_t w0;     /* first weight tap index                    */
    int32_t wstep;  /* weight tap index step                     */
    int32_t d0;     /* source offset of the first tap (pixels)   */
    int32_t dstep;  /* source offset step per tap                */
} zsg_taps;

typedef struct {
    int32_t rows_y, rows_x;          /* row grid per image                                   */
    int32_t src_H, src_W;            /* bounds of the gathered tensor                        */
    int32_t sy, sx;                  /* row -> source multiply                               */
    int32_t out_W;                   /* output image width (pixels)                          */
    int32_t osy, osx, opy, opx;      /* row -> output pixel                                  */
    int32_t reserved;
    int64_t src_off, src_bstride;    /* elements                                             */
    int64_t out_off, out_bstride;    /* elements                                             */
    zsg_taps ty, tx;
} zsg_seg;

typedef struct {
    int32_t B;            /* images                                                                         */
    int32_t C;            /* reduction channels per tap (multiple of 4)                                     */
    int32_t N;            /* output channels                                                                */
    int32_t src_ld;       /* source pixel stride (elements, multiple of 4)                                  */
    int32_t out_ld;       /* output pixel stride (elements)                                                 */
    int32_t wR, wS;       /* weight tap grid; weight row n starts at n*wt_ld, tap (r,s) at (r*wS+s)*wC       */
    int32_t wC;           /* channels per weight tap (>= C; C < wC selects a channel sub-range with wc0)     */
    int32_t wc0;          /* first weight channel used                                                      */
    int32_t wt_ld;        /* elements between consecutive weight rows                                       */
    int32_t relu;         /* epilogue: max(.,0)                                                             */
    int32_t merge_x;      /* 1: C==4 and all x-taps of a row are one contiguous run (stem / RGB input)       */
    int32_t nseg;
    int32_t tile_hint;    /* 0 heuristic, else BM | (BN << 8) | (split_k << 16) | variant bits; chosen by the host autotuner.
                           * bit 24: 8-wave workgroup (igemm, wgrad) / four position groups (wino); bit 25: 32-pixel K tiles
                           * (wgrad); bit 27 (igemm): 64-deep K tiles; bits 28-29 (igemm): stream-K with 1..3 workgroups per CU —
                           * 256 x that many workgroups share the (tile, K step) units evenly, cut tiles are completed in a fixed
                           * order (deterministic; needs zsg_set_stream_workspace, fewer tiles than workgroups, one segment,
                           * split_k <= 1)                                                                                    */
    int32_t epi_flags;    /* bit 0, BatchNorm-backward epilogues only (zsg_conv_*_bnb, *_bnb_tail): STORE the ReLU-masked gradient
                           * g = (acc [+ add_src]) * relu-bit instead of the unmasked sum — the stored dout is then at once the
                           * residual branch's gradient (autograd's ReLU backward of `out = relu(bn3(x) + residual)`,
                           * fpn_resnet.py:96-100), and the BatchNorm's apply pass needs neither the mask nor a second output     */
    zsg_seg seg[ZSG_MAX_SEG];
} zsg_conv_desc;

/* out = epilogue( sum_taps src * wt ) ;  epilogue: + bias[n] ; + add_src[same index as out] ; relu ;
 * * (mask_src[same index] > 0).   bias / add_src / mask_src may be NULL.  add_src may alias out (accumulate).
 * split_k > 1 (single dense segment, no ReLU): K slices are combined with fp32 atomics (output zeroed by the call). */
int zsg_conv_igemm(const zsg_conv_desc* d, const float* src, const float* wt, float* out, const float* bias,
                   const float* add_src, const float* mask_src, float* bn_partials, void* stream);
/* bn_partials (optional, may be NULL): [m_tiles][2][N] per-tile column (sum, sum of squares) of the output, written
 * by the epilogue so the following train-mode BatchNorm needs no extra pass over the activation
 * (m_tiles = sum over segments of ceil(rows / BM), BM = tile_hint & 0xff); finalize with zsg_bn_stats_from_partials. */

/* Read / write contract of the fp32 entries (zsg_conv_igemm, zsg_conv_wino, zsg_conv_wgrad, zsg_conv_wgrad_wino[_batched]), held at
 * zero tolerance by tests/test_gpu_conv_exact.py on integer data between NaN guards:
 *   - a tap outside the image, a row beyond a segment's last, a channel beyond C (K tails of the 32- / 64-deep tiles, Winograd's
 *     half chunk at C % 8 == 4) and a column beyond N contribute exactly +0;
 *   - memory outside the operand extents is never read in a way that reaches a result, and nothing outside the addressed output
 *     elements is written: pad lanes N..out_ld-1, gaps between images and levels, dw outside the [wc0, wc0+C) window and the wt_ld
 *     slack keep their bits;
 *   - elements INSIDE an operand's extent that the descriptor does not address (row padding C..src_ld-1, gaps, weight channels
 *     outside the window) may be read only against an exact zero, so any finite value may stand there.  The data gradient's
 *     descriptor reduces over C = dy.ld channels: there dy's pad lanes and the weight image's pad columns ARE operands and must be
 *     zero (zsg_transpose_w writes those zeros).
 * Refusals (-1, zsg_last_error says why, no output byte is touched) beyond the ones stated at the entries:
 *   - zsg_conv_igemm tiles are 64x64, 128x64 and 128x128 (8-wave and 64-deep-K forms of each; a C that is no multiple of 64 takes the
 *     64-deep tiles with a zero-filled tail); any other BM / BN field is refused.  A merge_x descriptor has the 64x64 and 128x64
 *     kernels only: BM = 128 selects the latter, every other BM the former, the BN field and the 8-wave / 64-deep-K bits are ignored.
 *   - stream-K exists for 64x64 (4-wave; 8-wave with 32- and 64-deep K), 128x64 (8-wave) and 128x128 (4- and 8-wave), and needs
 *     16-byte addressable output rows (out_ld, N, the output offsets and strides multiples of 4, aligned pointers).
 *   - BM = 32 (the streaming kernels): one dense 1x1 / stride-1 segment with C % 64 == 0 and N a multiple of the unit width whose
 *     filter panel fits the LDS — or one merge_x segment with a 7x7 / 3x3 window and N = 64 —, 16-byte aligned operands, no split-K,
 *     no stream-K; the merge_x form has no add_src / mask_src.
 *   - bn_partials need a plain convolution: no bias, add_src or ReLU, split_k <= 1 (zsg_conv_wino: also 16-byte addressable rows).
 *   - zsg_conv_wino: stream-K is the 32-tile x 64-channel four-group tile only, one segment, at most 256 tiles.
 * zsg_conv_wgrad refuses no tile hint: a field it has no kernel for runs the nearest tile (dy rows that are not 16-byte addressable
 * and image strides of 2^23 elements or more always take the 64x64 tile).
 * Split-K and the epilogue (zsg_conv_igemm and zsg_conv_wino alike): the output is zeroed unless add_src aliases it, every K slice
 * adds its term with an fp32 atomic, slice 0 also adds bias and a separate add_src, and mask_src multiplies EACH SLICE'S TERM, not what
 * `out` already holds.  bias, a separate add_src and mask_src therefore give the documented epilogue; add_src aliasing out together
 * with mask_src gives prev + (mask > 0) * sum, which is the documented (prev + sum) * (mask > 0) only where prev is zero wherever
 * mask <= 0 — what the training plans hold in dx, every earlier writer having applied the same mask. */

/* Weight gradient.  dw[n][(r*wS+s)*wC + wc0 + c] (+)= sum_rows dy[row][n] * src[gather(row, r, s)][c]
 * The descriptor is the FORWARD descriptor of the convolution (src = forward input, "out" geometry = dy); all
 * segments (pyramid levels of the shared head) are reduced in the one launch.  The pixel dimension is split over
 * tile_hint's split_k blocks whose partial tiles go to the workspace and are summed in a fixed order (deterministic).
 * Limits (error -1 otherwise): every tensor within a 2^29-element window, fewer than 2^24 pixel rows per segment, row pitches and
 * per-image pixel counts below 2^23; an IMAGE STRIDE of 2^23 elements or more (stem / layer1 maps of inputs beyond ~724x724) is
 * served by a 32-bit-multiply variant of the 64x64 tile (correct, not tuned).  1x1 / stride-1 / unpadded convolutions over
 * batch-dense tensors (src_bstride = H*W*src_ld, out_bstride = rows*out_ld) take the address-arithmetic-free DENSE loader. */
size_t zsg_conv_wgrad_workspace_bytes(const zsg_conv_desc* d);
int zsg_conv_wgrad(const zsg_conv_desc* d, const float* src, const float* dy, float* dw, int32_t accumulate, void* ws,
                   size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Reduced-precision TRAINING weight gradient (wgrad_dtype = "bf16"; csrc/wgrad_bf16.hip): zsg_conv_wgrad's descriptor (the forward
 * descriptor), dw layout with the wC / wc0 / wt_ld window, accumulate flag and workspace rule (zsg_conv_wgrad_workspace_bytes serves
 * both entries) on v_mfma_f32_32x32x16_bf16.  Same GEMM: M = output channel, N = (tap, c) tap-major, K = pixel rows of dy.  The
 * reference has no counterpart (autograd's fp32 weight gradient, or torch.autocast where the user asks for it).
 * Numerical contract:
 *   - src, dy and dw are fp32 in memory.  Every src and dy element is rounded to bf16 on its way into the matrix operand,
 *     round-to-nearest-even, exactly as torch.Tensor.to(torch.bfloat16) (the conversion of zsg_conv_igemm_bf16: +-0 and +-inf preserved,
 *     NaN stays NaN, a finite value above the largest bf16 becomes inf).
 *   - a tap outside the image, a pixel row beyond a segment's last and a column beyond N / ncols contribute exactly +0: memory there is
 *     never read (out-of-range buffer loads), and the channels N..out_ld-1 of a padded dy row (N = 45 in 48-wide rows) are replaced by
 *     +0 before the conversion — their values never enter an MFMA, so 0 * NaN cannot happen.
 *   - every product of two bf16 values is exact in fp32; products are accumulated in fp32 by the MFMA.  K tiles are 32 pixel rows and
 *     never straddle a segment; a K slice accumulates its tiles in ascending pixel-row order (the order inside one MFMA is the
 *     hardware's).
 *   - with more than one K slice, the slices go to the workspace as fp32 slabs [splits][N][ncols] and are summed in a fixed order by the
 *     slab reduction of zsg_conv_wgrad, which applies the window and accumulate; with one slice the kernel writes dw itself and honours
 *     both.  accumulate == 0 never reads dw.  No atomics: the same input and the same tile_hint give the same bits on every run.
 *   - tile_hint: 0 = the heuristic (128-wide tiles where N / ncols exceed 64; two blocks per CU, at most 64 slices, at least two K
 *     tiles per slice), else BM | BN << 8 | splits << 16 with BM, BN out of {64, 128} and splits in 1..255 (clipped to half the K
 *     tiles).  Workspace too small for the slices: -2.
 * Not supported (-1, nothing launched, zsg_last_error names the argument; zsg_conv_wgrad_bf16_supported returns 0): merge_x (the
 * stem: C = 4), out_ld % 4 != 0 or dy offsets that are not multiples of 4, an image stride >= 2^23 elements (the fp32 entry's wide
 * fallback), tile_hint variant bits 24-27 and the BN field 255.  All other limits are zsg_conv_wgrad's.
 * zsg_conv_wgrad_bf16_supported: 1 when zsg_conv_wgrad_bf16 accepts the descriptor (and its tile_hint), else 0 — the host asks at
 * lowering time and keeps the fp32 launch instead of failing inside a backward. */
int zsg_conv_wgrad_bf16(const zsg_conv_desc* d, const float* src, const float* dy, float* dw, int32_t accumulate, void* ws,
                        size_t ws_bytes, void* stream);
int32_t zsg_conv_wgrad_bf16_supported(const zsg_conv_desc* d);

/* ---------------------------------------------------------------------------------------------------------------
 * Winograd F(2x2,3x3) convolution on fp32 MFMA: the 3x3 / stride 1 / pad 1 convolutions (forward and data gradient)
 * of the same call sites as zsg_conv_igemm — fpn_resnet.py:73-74,92-94 (Bottleneck.conv2), :141-152 (P*_2),
 * mdl.py:211-219 (the shared head) — at 4 instead of 9 multiply-adds per (pixel, cin, cout), still fp32 throughout
 * (what cuDNN's fp32 path runs for the reference; tolerances in tests/test_gpu_ops.py).  Same descriptor, epilogue
 * terms and bn_partials contract as zsg_conv_igemm; `U` is the transformed filter image made by zsg_wino_weights.
 * tile_hint = tiles_per_block | (BN << 8) | (split_k << 16), both tile sizes in {32, 64}; bn_partials rows =
 * sum over segments of ceil(B * ceil(H/2) * ceil(W/2) / tiles_per_block).
 * ------------------------------------------------------------------------------------------------------------- */
int zsg_conv_wino(const zsg_conv_desc* d, const float* src, const float* U, float* out, const float* bias,
                  const float* add_src, const float* mask_src, float* bn_partials, void* stream);

/* Data gradient that COMPLETES dout of a train-mode BatchNorm (out = dgrad [+ add_src]; autograd's conv backward followed by
 * native_batch_norm_backward of fpn_resnet.py:86-97's conv-bn-relu chains): the epilogue also reduces that BatchNorm's
 * backward sums per output tile — partials[m_tile][0][n] = sum g, partials[m_tile][1][n] = sum g * (x - mean) * invstd with
 * g = out * relu-bit (bn_relu_mask as written by zsg_bn_apply, or NULL) — so that zsg_bn_backward_from_partials needs no
 * pass of its own over dout and x.  bn_x / bn_relu_mask are indexed with the convolution's OUTPUT element offsets (dense
 * [rows][N], the layout of dout).  Rows of partials: as bn_partials of zsg_conv_igemm / zsg_conv_wino for the same
 * tile_hint.  Requires split_k <= 1, every output element covered by the launch, N % 4 == 0. */
int zsg_conv_igemm_bnb(const zsg_conv_desc* d, const float* src, const float* wt, float* out, const float* add_src,
                       const float* bn_x, const float* bn_mean, const float* bn_invstd, const uint8_t* bn_relu_mask,
                       float* partials, void* stream);
/* tile_hint BM = 32 (BN field = unit width 32 / 64 / 128) selects the filter-resident streaming kernel for the 1x1 / stride-1
 * convolutions whose filter fits a CU's LDS (fpn_resnet.py:66-72: the bottleneck conv1 / conv3 / projection shortcut of the
 * first stage, forward and data gradient): one persistent workgroup per CU, every wave walks units of 32 pixels x BN channels
 * on its own.  It writes ONE partial row per workgroup; every other tile writes one per BM rows per segment.
 * zsg_conv_igemm_partial_rows: rows of bn_partials / partials a zsg_conv_igemm / zsg_conv_igemm_bnb launch with this
 * descriptor (and its tile_hint) writes; -1 when the hint is 0 (heuristic) or the streaming kernel does not cover the geometry. */
int32_t zsg_conv_igemm_partial_rows(const zsg_conv_desc* d);

/* ---- BatchNorm statistics finalised INSIDE the producing convolution (round 5; csrc/bn_tail.h) -----------------------------------
 * The tiles of one column block (BN output channels) take a ticket after writing their partial row; the tile that draws the last
 * ticket reduces the column block's rows in a fixed order in fp64 (deterministic) and publishes the result, so no finalize launch
 * (zsg_bn_stats_from_partials / the finalize half of zsg_bn_backward_from_partials) and no re-reduction in the apply pass remain on
 * the conv -> BatchNorm -> conv chain (fpn_resnet.py:80-100 forward; its autograd backward).
 * zsg_conv_bn_tail_tickets: the number of 32-bit ticket words the launch selected by d->tile_hint needs (its column blocks), or -1
 * when that launch cannot finalise in-kernel (no hint, the streaming 1x1 kernel, split_k > 1, merge_x, or more than 128 partial rows
 * per column block) — the caller then keeps the separate finalize.  is_wino != 0: the hint is zsg_conv_wino's.
 * tickets must be ZERO at entry and are zero again when the launch ends (the caller allocates them zeroed once; one set per call
 * site, never shared between launches that may be in flight together).  The entries below that finalise in-kernel refuse (-1, nothing
 * written) every launch for which this function says -1 — a descriptor without a tile hint included: the heuristic's tile may have more
 * column blocks than any ticket buffer the caller could have sized.  tests/test_gpu_conv_bn_exact.py holds these entries, zsg_conv_*_bnb
 * and zsg_conv_igemm_bnpre to exact integer references between guards. */
int32_t zsg_conv_bn_tail_tickets(const zsg_conv_desc* d, int32_t is_wino);
/* The 1x1 / stride-1 convolution that consumes a train-mode BatchNorm + residual + ReLU — the next bottleneck's conv1 behind bn3
 * (fpn_resnet.py:86-100: `out = relu(bn3(conv3(..)) + residual)` ... `conv1(out)`) — applies that BatchNorm in its operand loader
 * (round 5): `x` is the RAW conv3 output [rows][C]; the loader stages relu((x - pre_mean) * pre_invstd * pre_gamma + pre_beta +
 * pre_residual), zsg_bn_apply's own arithmetic, and the first column tile's workgroups also write that activation to pre_y and its
 * packed ReLU bits to pre_relu_mask (NULL: no bits) — the separate zsg_bn_apply launch and the second read of the activation
 * disappear.  64x64 / 128x64 tiles with 32-deep K tiles only (tile_hint), C % 32 == 0, dense source.  bn_partials (optional): this
 * convolution's own fused statistics; tickets != NULL: finalised in-kernel exactly as zsg_conv_igemm_bnstat does. */
int zsg_conv_igemm_bnpre(const zsg_conv_desc* d, const float* x, const float* wt, float* out, float* bn_partials, uint32_t* tickets,
                         float* mean, float* invstd, float* running_mean, float* running_var, float momentum, float eps,
                         const float* pre_mean, const float* pre_invstd, const float* pre_gamma, const float* pre_beta,
                         const float* pre_residual, float* pre_y, uint8_t* pre_relu_mask, void* stream);
/* zsg_conv_igemm / zsg_conv_wino with bn_partials (plain, bias-free convolution feeding a train-mode BatchNorm, fpn_resnet.py:86-97)
 * + in-kernel finalize: mean / invstd (and running statistics, momentum as torch.nn.BatchNorm2d; NULL to skip) are valid when the
 * launch ends; zsg_bn_apply follows directly. */
int zsg_conv_igemm_bnstat(const zsg_conv_desc* d, const float* src, const float* wt, float* out, float* partials, uint32_t* tickets,
                          float* mean, float* invstd, float* running_mean, float* running_var, float momentum, float eps, void* stream);
int zsg_conv_wino_bnstat(const zsg_conv_desc* d, const float* src, const float* U, float* out, float* partials, uint32_t* tickets,
                         float* mean, float* invstd, float* running_mean, float* running_var, float momentum, float eps, void* stream);
/* zsg_conv_igemm_bnb / zsg_conv_wino_bnb + in-kernel finalize of the BatchNorm BACKWARD sums: coef[0][c] = sum g / n,
 * coef[1][c] = sum g * xhat / n (coef: 2*N floats), d(gamma) = sum g * xhat and d(beta) = sum g written (accumulate == 0) or added;
 * zsg_bn_bwd_apply is all that remains of the BatchNorm's backward. */
int zsg_conv_igemm_bnb_tail(const zsg_conv_desc* d, const float* src, const float* wt, float* out, const float* add_src,
                            const float* bn_x, const float* bn_mean, const float* bn_invstd, const uint8_t* bn_relu_mask,
                            float* partials, uint32_t* tickets, float* coef, float* dgamma, float* dbeta, int32_t accumulate, void* stream);
int zsg_conv_wino_bnb_tail(const zsg_conv_desc* d, const float* src, const float* U, float* out, const float* add_src,
                           const float* bn_x, const float* bn_mean, const float* bn_invstd, const uint8_t* bn_relu_mask,
                           float* partials, uint32_t* tickets, float* coef, float* dgamma, float* dbeta, int32_t accumulate, void* stream);
int zsg_conv_wino_bnb(const zsg_conv_desc* d, const float* src, const float* U, float* out, const float* add_src,
                      const float* bn_x, const float* bn_mean, const float* bn_invstd, const uint8_t* bn_relu_mask,
                      float* partials, void* stream);
/* ---------------------------------------------------------------------------------------------------------------
 * Reduced-precision INFERENCE convolution (eval_dtype = "bf16"; csrc/igemm_bf16.hip): zsg_conv_igemm's descriptor, gather and epilogue
 * on v_mfma_f32_32x32x16_bf16.  Same call sites as zsg_conv_igemm, forward only, behind a BatchNorm fold (zsg_bn_fold) — the
 * reference has no counterpart (it evaluates in fp32, or under torch.autocast where the user asks for it).
 * Numerical contract:
 *   - activations (src, add_src, out) and bias are fp32 in memory; every src element is rounded to bf16 by the operand loader,
 *     round-to-nearest-even, exactly as torch.Tensor.to(torch.bfloat16): +-0 and +-inf are preserved, NaN stays NaN, a finite value
 *     above the largest bf16 becomes inf.  The weights are rounded once, by the same rule, by zsg_pack_w_bf16_batched.
 *   - fp32 subnormals go through the hardware conversion (v_cvt_pk_bf16_f32) like every other value: they round to a bf16 subnormal or
 *     to zero under the kernel's denormal mode; no test pins this down.
 *   - every product of two bf16 values is exact in fp32; products are accumulated in fp32 by the MFMA in a fixed K order (tap-major,
 *     channels ascending, 64 per K tile; the order inside one MFMA is the hardware's).  No split-K, no stream-K, no atomics: the same
 *     input gives the same bits on every run and for every tile hint the order of K tiles is the same.
 *   - epilogue in fp32, in zsg_conv_igemm's order: acc + bias[n] + add_src[.], then ReLU.  add_src may alias out.
 * Supported: C % 4 == 0 (a half group at C % 8 == 4 is zero-filled), any N (N = 45 with out_ld = 45 takes the 4-byte epilogue), any row
 * count, up to ZSG_MAX_SEG segments, strides, dilation, tap tables.  d->wC / wc0 / wt_ld are NOT read: the weight operand is the packed
 * image uint16 [N][wR*wS][C8], C8 = roundup(d->C, 8).  tile_hint: 0 = the library heuristic (igemm's: fewest rounds of 256 blocks x
 * tile area, smaller tiles favoured), else BM | BN << 8 out of 64x64, 128x64, 128x128.
 * Not supported (-1, nothing launched, zsg_last_error names the argument): merge_x, epi_flags, tile_hint split_k > 1, stream-K bits
 * (28-29) or variant bits 24-27.  There is no mask_src and no bn_partials operand.
 * zsg_conv_igemm_bf16_supported: 1 when zsg_conv_igemm_bf16 accepts the descriptor (and its tile_hint), else 0 — the host asks at
 * lowering time and keeps the fp32 launch instead of failing inside a forward. */
int zsg_conv_igemm_bf16(const zsg_conv_desc* d, const float* src, const uint16_t* wt_packed, float* out, const float* bias,
                        const float* add_src, void* stream);
int32_t zsg_conv_igemm_bf16_supported(const zsg_conv_desc* d);
/* Every bf16 weight image of an eval plan in ONE launch.  jobs: device array of { int64 src, dst (absolute device addresses); int32 N,
 * T, wC, wc0, C, C8, blk0, pad }: fp32 OHWI source element (n, t, c) at n*T*wC + t*wC + wc0 + c (wc0 + C <= wC: a channel window, what
 * head conv0's feature GEMM needs), destination uint16 [N][T][C8] with C8 = roundup(C, 8), 16-byte aligned, channels C..C8-1 zero;
 * blk0 = running sum of ceil(N*T*C8/8 / 256); total_blocks = the final sum.  Rounding: the contract above. */
int zsg_pack_w_bf16_batched(const void* jobs_dev, int32_t njobs, int32_t total_blocks, void* stream);
/* ---------------------------------------------------------------------------------------------------------------
 * Reduced-precision TRAINING convolution of the pyramid and the heads (train_dtype = "bf16_head"; csrc/igemm_bf16.hip): the forward
 * convolutions and the data gradients of layers without BatchNorm.  zsg_conv_igemm_bf16_m is zsg_conv_igemm_bf16 (fp32 in memory) plus
 * zsg_conv_igemm's last epilogue term, the ReLU mask of a data gradient.
 * Numerical contract: zsg_conv_igemm_bf16's, word for word (src rounded to bf16 by the loader, round-to-nearest-even; weights rounded
 * once by zsg_pack_w_bf16_batched; exact products, fp32 accumulation in the fixed tap-major K order; no split-K, no stream-K, no
 * atomics: the same input gives the same bits on every run), and the epilogue in zsg_conv_igemm's order:
 *       v = acc + bias[n] + add_src[o];  if relu: v = max(v, 0);  out[o] = mask_src[o] > 0 ? v : 0
 *   - mask_src is fp32, indexed with the OUTPUT offsets (the forward activation whose gradient out is, rebased by the caller where
 *     the two live at different offsets); an element passes where mask_src > 0: -0.0, +0.0, negative values and NaN give +0.0,
 *     whatever v is (a select, not a product: an inf or NaN in a masked position does not spread).
 *   - mask_src == NULL launches zsg_conv_igemm_bf16's kernel: the same bits.  The mask is a compile-time variant of the kernel, so the
 *     kernels of the entries without it are the instructions they were.
 *   - add_src may alias out; mask_src must not alias out.  mask_src 16-byte aligned takes the 16-byte epilogue with out / bias / add_src,
 *     else the 4-byte one.
 * For a data gradient the weight operand is the packed image of the TRANSPOSED filter [n][wR*wS][cred] (zsg_transpose_w_batched, then
 * zsg_pack_w_bf16_batched with N = n, T = wR*wS, wC = C = cred): dy is rounded by the loader, the transposed weights by the packer.
 * Supported / not supported: zsg_conv_igemm_bf16's lists (one check, bf16_check); there is no bn_partials operand and no epi_flags:
 * a data gradient that carries a BatchNorm's backward sums stays fp32 or takes zsg_conv_igemm_bf16_bnb (below).
 * zsg_conv_igemm_bf16_m_supported: 1 when zsg_conv_igemm_bf16_m accepts the descriptor (and its tile_hint), else 0. */
int zsg_conv_igemm_bf16_m(const zsg_conv_desc* d, const float* src, const uint16_t* wt_packed, float* out, const float* bias,
                          const float* add_src, const float* mask_src, void* stream);
int32_t zsg_conv_igemm_bf16_m_supported(const zsg_conv_desc* d);
/* ---------------------------------------------------------------------------------------------------------------
 * Reduced-precision TRAINING forward of the ResNet encoder (enc_dtype = "bf16_fwd"; csrc/igemm_bf16.hip): the plain, bias-free
 * convolution in front of a train-mode BatchNorm (fpn_resnet.py:86-97) on bf16 MFMA, with zsg_conv_igemm's fused BatchNorm statistics.
 * zsg_conv_igemm_bf16_bn is zsg_conv_igemm_bf16 without bias, add_src and ReLU, plus the partial rows:
 *       bn_partials[mt][0][n] = sum over the valid rows of M tile mt of v,   bn_partials[mt][1][n] = sum of v * v
 *   v the fp32 value stored to out, mt the kernel's M-tile index counted across segments, the layout [m_tiles][2][N] with
 *   m_tiles = sum over segments of ceil(B * rows_y * rows_x / BM) — zsg_conv_igemm's bn_partials, so zsg_bn_stats_from_partials,
 *   zsg_bn_apply_from_partials and zsg_bn_sync_fwd_sums read it unchanged.
 * Numerical contract of out: zsg_conv_igemm_bf16's, word for word (src rounded to bf16 by the loader, round-to-nearest-even; weights
 * rounded once by zsg_pack_w_bf16_batched; exact products, fp32 accumulation in the fixed tap-major K order; no split-K, no stream-K):
 * out is bit-equal to what zsg_conv_igemm_bf16 writes for the same descriptor, operands and hint (bias = add_src = NULL).
 * Order of the sums (fp32, fixed, the same on every run): the output tile lies transposed in LDS; a thread owns 4 adjacent columns and
 * the tile rows r, r + R, r + 2R, ... (R = 1024 / BN: 16 row groups at BN = 64, 8 at BN = 128), which it adds in ascending order
 * (s += v; q = fma(v, v, q), invalid rows skipped); the R row-group sums of a column then meet in LDS and one thread adds them in
 * ascending group order.  No atomics and nothing between workgroups: every (mt, n < N) element is written exactly once, by a 16-byte
 * vector store; columns n >= N of a column tile that reaches past N are not written, nor is any row >= m_tiles.  No in-kernel
 * finalize (no tickets), no bnpre loader, no BatchNorm-backward sums: those stay fp32 (zsg_conv_igemm_bnstat / _bnpre / _bnb).
 * Not supported (-1, nothing launched, zsg_last_error names the argument): everything zsg_conv_igemm_bf16 refuses (merge_x,
 * epi_flags, split-K / stream-K / variant hint bits); d->relu; N % 4 != 0; a descriptor or out pointer that does not take the 16-byte
 * epilogue (out_ld, segment out_off / out_bstride multiples of 4, out 16-byte aligned); bn_partials NULL or not 16-byte aligned.
 * zsg_conv_igemm_bf16_bn_supported: 1 when the DESCRIPTOR (and its tile_hint) is accepted, else 0 (the pointers are the entry's
 * business).  zsg_conv_igemm_bf16_partial_rows: the rows of bn_partials the launch selected by d->tile_hint writes (hint 0: the tile
 * the bf16 heuristic picks), or -1 where zsg_conv_igemm_bf16_bn_supported is 0. */
int zsg_conv_igemm_bf16_bn(const zsg_conv_desc* d, const float* src, const uint16_t* wt_packed, float* out, float* bn_partials,
                           void* stream);
int32_t zsg_conv_igemm_bf16_bn_supported(const zsg_conv_desc* d);
int32_t zsg_conv_igemm_bf16_partial_rows(const zsg_conv_desc* d);
/* ---------------------------------------------------------------------------------------------------------------
 * Reduced-precision TRAINING data gradient of the ResNet encoder (enc_bwd_dtype = "bf16"; csrc/igemm_bf16.hip): the data gradient that
 * completes the dout of a train-mode (or frozen, or synchronized) BatchNorm, on bf16 MFMA, with zsg_conv_igemm_bnb's epilogue — the one
 * bf16 entry that carries a BatchNorm's backward sums (every other bf16 entry still refuses epi_flags).
 * Matrix part: zsg_conv_igemm_bf16's contract, word for word (src = dy rounded to bf16 by the loader, round-to-nearest-even; wt_packed
 * the packed image of the TRANSPOSED filter as for zsg_conv_igemm_bf16_m; exact products, fp32 accumulation in the fixed tap-major K
 * order; no split-K, no stream-K, no atomics: the same input gives the same bits on every run).
 * Epilogue (o = the element's output offset; bn_x and bn_relu_mask are indexed with the OUTPUT offsets, as in zsg_conv_igemm_bnb):
 *       v = acc [+ add_src[o]];   g[e] = bit e of bn_relu_mask[o >> 2] ? v[e] : 0   (4 bits per 16-byte group, as zsg_bn_apply writes
 *       them; bn_relu_mask == NULL: all ones);   out[o] = (d->epi_flags & 1) ? g : v
 *       partials[mt][0][n] = sum g,   partials[mt][1][n] = sum g * ((bn_x[o] - bn_mean[n]) * bn_invstd[n])   over the valid rows of M tile mt
 *   layout [m_tiles][2][N], m_tiles counted exactly as zsg_conv_igemm_bf16_partial_rows counts it for the same descriptor WITHOUT the
 *   epi_flags bit (that function keeps refusing epi_flags): zsg_bn_backward_from_partials, zsg_bn_frozen_backward and
 *   zsg_bn_sync_bwd_sums read it unchanged.  add_src may alias out (a thread reads its elements before it writes them).
 * Order of the sums (fp32, fixed, the same on every run; zsg_conv_igemm_bf16_bn's): the output tile lies transposed in LDS; a thread
 * owns 4 adjacent columns and the tile rows r, r + R, r + 2R, ... (R = 1024 / BN), which it adds in ascending order (s += g;
 * q += g * xhat with xhat = (x - mean) * invstd, invalid rows skipped); the R row-group sums of a column then meet in LDS and one thread
 * adds them in ascending group order.  Every (mt, n < N) element is written exactly once, by a 16-byte store; columns n >= N of a column
 * tile that reaches past N are not written, nor is any row >= m_tiles.  The thread's bn_x values, mask bits and add_src values are
 * requested before the accumulators go through LDS.  No in-kernel finalize (no tickets): zsg_bn_backward_from_partials finalizes.
 * Tiles served: 64x64, 128x64 and 128x128 (the last: 16 rows per thread, 237 vector registers, no scratch at two blocks per CU).
 * Not supported (-1, nothing launched, zsg_last_error names the argument): everything zsg_conv_igemm_bf16 refuses except epi_flags bit 0
 * (merge_x, split-K / stream-K / variant hint bits, ...); bits of epi_flags other than bit 0; d->relu; N % 4 != 0; a descriptor, out or
 * add_src pointer that does not take the 16-byte epilogue; bn_x, bn_mean, bn_invstd or partials NULL or not 16-byte aligned.
 * zsg_conv_igemm_bf16_bnb_supported: 1 when the DESCRIPTOR (and its tile_hint) is accepted, else 0. */
int zsg_conv_igemm_bf16_bnb(const zsg_conv_desc* d, const float* src, const uint16_t* wt_packed, float* out, const float* add_src,
                            const float* bn_x, const float* bn_mean, const float* bn_invstd, const uint8_t* bn_relu_mask, float* partials,
                            void* stream);
int32_t zsg_conv_igemm_bf16_bnb_supported(const zsg_conv_desc* d);

/* ---------------------------------------------------------------------------------------------------------------
 * bf16 ACTIVATION STORAGE for inference (eval_dtype = "bf16_act"; csrc/igemm_bf16.hip, csrc/bf16_act.hip).  Everything "bf16" has;
 * in addition the activations between the stem's max-pool and the heads' last convolution are stored as bf16 (uint16 elements, the
 * same NHWC / packed-pyramid layouts, the same ELEMENT offsets and leading dimensions as the fp32 plan).  Contract:
 *   - Rounding: a value is rounded exactly once, when it is stored; round-to-nearest-even, the rule above (Tensor.to(torch.bfloat16)).
 *   - Arithmetic: everything is computed in fp32 from the widened inputs (widening is exact) — bias, residual add, ReLU, max,
 *     upsample-add, the l2 norm, the shared conv0 sum — in the order of the fp32 kernels.  The convolution's operand loader rounds an
 *     fp32 activation to bf16 anyway, so a convolution fed a bf16 activation sees the operand bits the "bf16" plan's sees for the same
 *     fp32 value; results differ only where an fp32 activation was consumed in fp32 (residual add_src, upsample_add, l2norm, ReLU,
 *     the average pool).
 *   - fp32 in memory: the image and the stem convolution's output, the LSTM and the language vector, the language-map operands V, G
 *     and lmap (lmap enters conv0 as an fp32 add_src), the shared-image plan's per-slot accumulator Y, and the network's outputs (the
 *     heads' final convolutions read bf16 and write fp32).  Training plans never see any of this.
 *
 * zsg_conv_igemm_bf16_io: zsg_conv_igemm_bf16 with the storage format of each activation operand chosen by io_flags:
 *     ZSG_IO_SRC_BF16 = 1 (src is uint16), ZSG_IO_OUT_BF16 = 2 (out is uint16), ZSG_IO_ADD_BF16 = 4 (add_src is uint16).
 *   io_flags = 0 is zsg_conv_igemm_bf16 (same kernel, same bits).  With SRC_BF16 the loader converts nothing: an 8-channel group is one
 *   16-byte load when src_ld and every segment's src_off / src_bstride are multiples of 8 and src is 16-byte aligned, else two 8-byte
 *   halves (C = 36 with src_ld = 36; src 8-byte aligned); the C % 8 == 4 tail is zero-filled either way.  With OUT_BF16 the epilogue
 *   rounds and stores 8-byte groups of 4 channels (2-byte stores where N / out_ld / the offsets are not multiples of 4: N = 45).
 *   add_src may alias out when both have the same format.  Same K order, same refusals as zsg_conv_igemm_bf16; in addition: io_flags
 *   outside 0..7, ADD_BF16 without add_src, a src that is not 8-byte aligned (SRC_BF16), add_src aliasing out in another format.
 * zsg_conv_igemm_bf16_io_supported: what the DESCRIPTOR and the flag word decide of that (the pointers are the entry's business). */
#define ZSG_IO_SRC_BF16 1
#define ZSG_IO_OUT_BF16 2
#define ZSG_IO_ADD_BF16 4
int zsg_conv_igemm_bf16_io(const zsg_conv_desc* d, const void* src, const uint16_t* wt_packed, void* out, const float* bias,
                           const void* add_src, int32_t io_flags, void* stream);
int32_t zsg_conv_igemm_bf16_io_supported(const zsg_conv_desc* d, int32_t io_flags);
/* Element-wise kernels of such a plan (forward only; the fp32 kernel of the same name on the widened inputs, rounded once).
 * zsg_maxpool_fwd_bf16: x fp32 (x_bf16 = 0: the stem's output) or bf16, out bf16, no index output; NaN propagates.  C % 4 == 0. */
int zsg_maxpool_fwd_bf16(const void* x, int32_t x_bf16, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k, int32_t s, int32_t p,
                         int32_t Ho, int32_t Wo, uint16_t* out, void* stream);
/* out = a + nearest-upsampled p (zsg_upsample_add_fwd's index rule), all bf16.  C % 4 == 0. */
int zsg_upsample_add_fwd_bf16(const uint16_t* a, const uint16_t* p, int32_t B, int32_t Hs, int32_t Ws, int32_t Hd, int32_t Wd, int32_t C,
                              uint16_t* out, void* stream);
/* out = fmaxf(x, 0) (a NaN becomes 0, as zsg_relu_fwd).  n % 4 == 0. */
int zsg_relu_fwd_bf16(const uint16_t* x, int64_t n, uint16_t* out, void* stream);
/* mean over HW pixels: the pixel-ascending fp32 sum of zsg_avgpool_fwd, divided, rounded. */
int zsg_avgpool_fwd_bf16(const uint16_t* x, int32_t B, int32_t HW, int32_t C, uint16_t* out, void* stream);
/* zsg_head_shared_conv0 with h1 stored as bf16: Y, bias, G, V fp32, the same summation order ((Y + G) + (taps + bias)), ReLU, one
 * rounding; an img_idx outside [0, Bi) gives NaN rows. */
int zsg_head_shared_conv0_bf16(const float* Y, const void* img_idx, int32_t idx_i64, const float* bias, const float* G, const float* V,
                               int32_t Bi, int32_t Q, int32_t nlev, const int32_t* hw, int32_t N, uint16_t* out, void* stream);
/* The cast pair (any n, any element alignment): what a bf16_act plan puts around an operation that has no bf16 form (l2norm). */
int zsg_cast_f32_bf16(const float* x, int64_t n, uint16_t* out, void* stream);
int zsg_cast_bf16_f32(const uint16_t* x, int64_t n, float* out, void* stream);

/* elements of the transformed image of a C -> N 3x3 filter: [ceil(C/8)][16][roundup(N,64)][8] */
int64_t zsg_wino_u_elems(int32_t C, int32_t N);
/* U = G g G^T for every job in ONE launch.  jobs: device array of { int64 src, dst (absolute device addresses);
 * int32 N, C, src_row_ld, src_tap_ld, flip, Npad, chunks, blk0 }: source element (n, tap, c) at n*src_row_ld +
 * tap*src_tap_ld + c (an OHWI weight or a channel window of it; or a zsg_transpose_w image with flip = 1: the filter
 * rotated by 180 degrees, for the data gradient); blk0 = running sum of ceil(chunks*Npad*8 / 256). */
int zsg_wino_weights(const void* jobs, int32_t njobs, int32_t total_blocks, void* stream);

/* Winograd F(3x3,2x2) weight gradient of a 3x3 / stride 1 / pad 1 convolution: same contract as zsg_conv_wgrad (forward
 * descriptor, accumulate flag, split-K workspace [splits][N][9*C] with the deterministic slab reduction), 16 instead of
 * 36 multiply-adds per 2x2 output tile.  tile_hint: split_k << 16 (0: heuristic), bit 24: block order "whole K slices per XCD". */
size_t zsg_conv_wgrad_wino_workspace_bytes(const zsg_conv_desc* d);
int zsg_conv_wgrad_wino(const zsg_conv_desc* d, const float* src, const float* dy, float* dw, int32_t accumulate, void* ws,
                        size_t ws_bytes, void* stream);
/* Round 6: njobs (<= 8) convolutions of ONE geometry in one launch — job j: (src[j], dy[j]) -> dw[j]; the pointer arrays are HOST arrays
 * (read at the call).  The identical bottlenecks of a ResNet stage (/root/reference/code/fpn_resnet.py:86-100: layerN.1 .. layerN.k conv2;
 * autograd's weight gradient of each) are leaves of the backward graph: released together they are njobs x the (n, c) blocks at a
 * fraction of the split-K slabs.  Workspace: njobs x zsg_conv_wgrad_wino_workspace_bytes(d) is always enough; tile_hint as above
 * (the split-K factor is per job). */
int zsg_conv_wgrad_wino_batched(const zsg_conv_desc* d, int32_t njobs, const float* const* src, const float* const* dy, float* const* dw,
                                int32_t accumulate, void* ws, size_t ws_bytes, void* stream);

/* dst[c][t][n] = src[n][t][c]  (OHWI -> IHWO, the dgrad weight image); T = R*S; dst rows are dst_ld >= N wide
 * (columns N..dst_ld-1 are zeroed: the 45-channel head output is handled as a 48-channel GEMM operand). */
int zsg_transpose_w(const float* src, float* dst, int32_t N, int32_t T, int32_t C, int32_t dst_ld, void* stream);
/* All dgrad weight images of a step in ONE launch.  jobs: device array of
 * {int64 src_off, dst_off; int32 N, T, C, dst_ld, tile0, tiles_c, tiles_n, pad} (offsets in elements from the bases;
 * tiles_c = ceil(C/64), tiles_n = ceil(dst_ld/64), tile0 = running sum of T*tiles_c*tiles_n; round 5: 64 x 64 tiles moved with
 * 16-byte accesses — C, dst_ld and both offsets multiples of 4, bases 16-byte aligned). */
int zsg_transpose_w_batched(const float* src_base, float* dst_base, const void* jobs, int32_t njobs, int32_t total_tiles,
                            void* stream);
/* dst[r][0:dst_ld] = [ src[r*src_ld + 0:C] | 0 ... ] */
int zsg_pad_rows(const float* src, int64_t rows, int32_t C, int32_t src_ld, float* dst, int32_t dst_ld, void* stream);

/* out[g][c] (+)= sum_{r<rows} x[g*gstride + r*ld + c0 + c],  c < C   (bias gradients; per-image language-vector grads).
 * 16-byte loads when C, ld, c0, gstride are multiples of 4 and x is 16-byte aligned, else a scalar kernel; under
 * zsg_set_deterministic one block per column group adds in a fixed order (the scalar form accumulates in fp64 there). */
int zsg_colsum(const float* x, int32_t groups, int64_t gstride, int32_t rows, int32_t ld, int32_t c0, int32_t C,
               float* out, int32_t accumulate, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * BatchNorm2d (train-mode batch statistics, momentum/eps as nn.BatchNorm2d) fused with ReLU / residual add.
 * Replaces nn.BatchNorm2d + ReLU(inplace) + `out += residual` of fpn_resnet.py:80-100 (53 layers, utils.py:395).
 * x: [rows][C] contiguous NHWC (ld == C), C % 4 == 0.
 * ------------------------------------------------------------------------------------------------------------- */
size_t zsg_bn_workspace_bytes(int64_t rows, int32_t C);
/* mean/invstd out; running_mean/var updated in place (unbiased var), NULL to skip. */
int zsg_bn_stats(const float* x, int64_t rows, int32_t C, float* mean, float* invstd, float* running_mean,
                 float* running_var, float momentum, float eps, void* ws, size_t ws_bytes, void* stream);
int zsg_bn_stats_from_partials(const float* partials, int32_t chunks, int64_t rows, int32_t C, float* mean, float* invstd,
                               float* running_mean, float* running_var, float momentum, float eps, void* stream);
/* Stem: nn.BatchNorm2d -> nn.ReLU -> nn.MaxPool2d(3, 2, 1) (mdl.py:149-152 on fpn_resnet.py's conv1 / bn1) in ONE pass over the
 * stem activation x [B][H][W][C] (the network's largest tensor): out [B][Ho][Wo][C] = maxpool(relu(bn(x))), idx = window position
 * of the first maximum (uint8, as zsg_maxpool_fwd).  The backward takes d(out): per-channel sums over the pooled gradient (the only
 * non-zero entries of the BatchNorm's grad_output), then dx per input pixel; dgamma / dbeta as zsg_bn_backward.
 * ws >= zsg_bn_workspace_bytes(B * Ho * Wo, C).
 * The ReLU is fmaxf(bn(x), 0) (a NaN becomes 0, as zsg_relu_fwd) and runs BEFORE the pool: a NaN tap counts as 0 and does not
 * propagate into the window's maximum; among equal values (zeros after the ReLU above all) the first in-bounds tap in (row, column)
 * order wins.  In the backward a NaN position passes no gradient (relu(bn(x)) > 0 is false there). */
int zsg_bn_relu_maxpool_fwd(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, const float* mean, const float* invstd,
                            const float* gamma, const float* beta, int32_t k, int32_t s, int32_t p, int32_t Ho, int32_t Wo, float* out,
                            uint8_t* idx, void* stream);
int zsg_bn_relu_maxpool_bwd(const float* dout, const uint8_t* idx, const float* x, int32_t B, int32_t H, int32_t W, int32_t C,
                            const float* mean, const float* invstd, const float* gamma, const float* beta, int32_t k, int32_t s, int32_t p,
                            int32_t Ho, int32_t Wo, float* dx, float* dgamma, float* dbeta, int32_t accumulate, void* ws, size_t ws_bytes,
                            void* stream);
/* BatchNorm apply straight from the convolution epilogue's partial rows when there are at most zsg_bn_inline_max_chunks()
 * of them (small maps: layer3 / layer4 / pyramid sizes): every block reduces the rows for its own channels (fp64, fixed
 * order), block 0 publishes mean / invstd / the running statistics — no separate finalize launch between the convolution
 * and the normalisation.  (The backward's partial rows are never that few at useful occupancy: a 64-chunk partial pass
 * measured 3x slower than the finalize launch it would save.) */
int32_t zsg_bn_inline_max_chunks(void);
int zsg_bn_apply_from_partials(const float* x, int64_t rows, int32_t C, const float* partials, int32_t chunks, const float* gamma,
                               const float* beta, const float* residual, int32_t relu, float* out, uint8_t* relu_mask,
                               float* mean, float* invstd, float* running_mean, float* running_var, float momentum, float eps,
                               void* stream);
/* eval mode, folded: every (conv, BatchNorm) pair of the job list gets W*s and (beta - mean*s), s = gamma/sqrt(var+eps)
 * per output channel, written to `arena` in ONE launch; the plan then runs conv(+bias, +residual, ReLU) without any
 * BatchNorm launch.  jobs: device array of { int64 w_off, dst_off, gamma_off, beta_off, bias_off; int32 row0, N, row_len,
 * bn_index } (element offsets into flat / arena; rows are OHWI output channels, row_len % 4 == 0). */
int zsg_bn_fold(const float* flat, const float* running_mean, const float* running_var, float eps, const void* jobs,
                int32_t njobs, int32_t total_rows, float* arena, void* stream);
/* eval mode: mean = running_mean, invstd = rsqrt(running_var + eps) */
int zsg_bn_eval_stats(const float* running_mean, const float* running_var, int32_t C, float eps, float* mean,
                      float* invstd, void* stream);
/* out = [relu]( (x-mean)*invstd*gamma + beta [+ residual] ).  relu_mask (optional, rows*C/4 bytes): bit e of byte i =
 * (element 4i+e > 0) — what zsg_bn_backward needs of the output, at 1/16 of its HBM traffic.  Bits 4-7 are 0; the mask is written
 * only when relu != 0 (with relu == 0 a given buffer stays untouched).  relu: out = fmaxf(v, 0) (a NaN becomes 0, as zsg_relu_fwd) and
 * its mask bit is 0; without relu a NaN stays.  zsg_bn_apply_from_partials follows the same rules. */
int zsg_bn_apply(const float* x, int64_t rows, int32_t C, const float* mean, const float* invstd, const float* gamma,
                 const float* beta, const float* residual, int32_t relu, float* out, uint8_t* relu_mask, void* stream);
/* g = dout * (out > 0), the mask taken from relu_mask if given, else from relu_out if given, else g = dout;  dgamma = sum g*xhat ; dbeta = sum g ;
 * dx = gamma*invstd*(g - dbeta/n - xhat*dgamma/n) ; optional g_out = g (gradient of the residual branch).
 * dgamma/dbeta are ACCUMULATED (+=) when accumulate != 0, else overwritten. */
int zsg_bn_backward(const float* dout, const float* relu_out, const uint8_t* relu_mask, const float* x, int64_t rows, int32_t C,
                    const float* mean, const float* invstd, const float* gamma, float* dx, float* g_out,
                    float* dgamma, float* dbeta, int32_t accumulate, void* ws, size_t ws_bytes, void* stream);
/* The apply pass alone: dx = gamma*invstd*(g - coef[0] - xhat*coef[1]), g = dout * relu-bit, optional g_out = g; coef (2*C floats)
 * as finalised by zsg_conv_igemm_bnb_tail / zsg_conv_wino_bnb_tail (native_batch_norm_backward's input-gradient formula). */
int zsg_bn_bwd_apply(const float* dout, const uint8_t* relu_mask, const float* x, int64_t rows, int32_t C, const float* mean,
                     const float* invstd, const float* gamma, const float* coef, float* dx, float* g_out, void* stream);
/* Frozen (eval-mode) BatchNorm inside a training network: the backward of F.batch_norm(training=False) with mean = running_mean and
 * invstd = rsqrt(running_var + eps) (zsg_bn_eval_stats).  g = dout * relu-bit (relu_mask, or NULL: g = dout);  dx = gamma*invstd*g
 * (no mean-subtraction terms; NULL: the input needs no gradient);  optional g_out = g (gradient of the residual branch);
 * dgamma = sum g*xhat, dbeta = sum g (each NULL to skip: frozen affine), ACCUMULATED (+=) when accumulate != 0, else overwritten.
 * partials (optional): the [chunks][2][C] (sum g, sum g*xhat) rows a *_bnb data gradient wrote for the same mean / invstd; then x is
 * not read and ws >= 2*C floats.  Without partials the one pass over dout / x also reduces the sums: ws >= zsg_bn_workspace_bytes(rows, C).
 * The sums are reduced in a fixed order (fp64 finalize): deterministic.  With dgamma and dbeta both NULL the launch is a pure
 * per-channel scale that never reads x or mean (ws unused). */
int zsg_bn_frozen_backward(const float* dout, const uint8_t* relu_mask, const float* x, int64_t rows, int32_t C, const float* mean,
                           const float* invstd, const float* gamma, float* dx, float* g_out, float* dgamma, float* dbeta,
                           int32_t accumulate, const float* partials, int32_t chunks, void* ws, size_t ws_bytes, void* stream);
/* Frozen counterpart of zsg_bn_relu_maxpool_bwd (forward: zsg_bn_relu_maxpool_fwd fed the eval statistics): one pass per INPUT
 * pixel gathers d(out) at the window positions idx selected, masks it by relu(bn(x)) > 0 and writes dx = gamma*invstd*g (NULL: no
 * input gradient); dgamma / dbeta as zsg_bn_frozen_backward (NULL to skip; then ws is unused), else ws >= zsg_bn_workspace_bytes(B*H*W, C). */
int zsg_bn_frozen_relu_maxpool_bwd(const float* dout, const uint8_t* idx, const float* x, int32_t B, int32_t H, int32_t W, int32_t C,
                                   const float* mean, const float* invstd, const float* gamma, const float* beta, int32_t k, int32_t s,
                                   int32_t p, int32_t Ho, int32_t Wo, float* dx, float* dgamma, float* dbeta, int32_t accumulate,
                                   void* ws, size_t ws_bytes, void* stream);
/* The same from the partial rows [chunks][2][C] of zsg_conv_igemm_bnb / zsg_conv_wino_bnb (finalize + apply: one pass over
 * dout and x instead of two).  ws: >= 2*C floats. */
int zsg_bn_backward_from_partials(const float* dout, const uint8_t* relu_mask, const float* x, int64_t rows, int32_t C,
                                  const float* mean, const float* invstd, const float* gamma, float* dx, float* g_out,
                                  float* dgamma, float* dbeta, int32_t accumulate, const float* partials, int32_t chunks,
                                  void* ws, size_t ws_bytes, void* stream);
/* Synchronized BatchNorm (torch.nn.SyncBatchNorm) across data-parallel ranks, split at the collective: a sums launch writes the
 * rank-local per-channel sums in fp64, the caller all-reduces them over the ranks (SUM), and the finalize / apply launch restarts from
 * the global sums.  Fixed-order reductions, no float atomics: bit-reproducible.  With one rank and the same partial rows the results
 * equal those of zsg_bn_stats, zsg_bn_stats_from_partials and zsg_bn_backward(_from_partials) bit for bit (not those of the in-kernel
 * finalizes of the *_bnstat / *_bnb_tail convolutions or of zsg_bn_apply_from_partials, which sum in another order).
 * Forward sums (2*C + 1 doubles): [sum x | sum x^2 | n], from the producing convolution's partial rows [chunks][2][C] (x and ws unused)
 * or from one pass over x (partials NULL: ws >= zsg_bn_workspace_bytes(rows, C)).  The finalize writes mean / invstd / running
 * statistics (unbiased variance, factor N / (N - 1), N = the all-reduced n) with zsg_bn_stats_from_partials's arithmetic. */
int zsg_bn_sync_fwd_sums(const float* x, int64_t rows, int32_t C, const float* partials, int32_t chunks, double* sums, void* ws,
                         size_t ws_bytes, void* stream);
int zsg_bn_sync_fwd_finalize(const double* sums, int32_t C, float* mean, float* invstd, float* running_mean, float* running_var,
                             float momentum, float eps, void* stream);
/* Backward sums (2*C doubles): [sum g | sum g*xhat], g = dout * relu-bit, xhat from the global mean / invstd; from a *_bnb data
 * gradient's partial rows (dout / x unread, ws unused) or one pass over dout and x (ws >= zsg_bn_workspace_bytes(rows, C)).  dgamma /
 * dbeta (NULL to skip) receive the RANK-LOCAL sums, accumulated when accumulate != 0 (the gradient reducer averages them as any other).
 * The apply writes dx = gamma*invstd*(g - sum g / N - xhat * sum g*xhat / N) from the all-reduced sums and the forward's all-reduced
 * N (fwd_sums[2*C]); optional g_out = g. */
int zsg_bn_sync_bwd_sums(const float* dout, const uint8_t* relu_mask, const float* x, int64_t rows, int32_t C, const float* mean,
                         const float* invstd, const float* partials, int32_t chunks, double* sums, float* dgamma, float* dbeta,
                         int32_t accumulate, void* ws, size_t ws_bytes, void* stream);
int zsg_bn_sync_bwd_apply(const float* dout, const uint8_t* relu_mask, const float* x, int64_t rows, int32_t C, const float* mean,
                          const float* invstd, const float* gamma, const double* sums, const double* fwd_sums, float* dx, float* g_out,
                          void* stream);
/* zsg_bn_relu_maxpool_bwd split at the collective: the sums over the pooled gradient (ws >= zsg_bn_workspace_bytes(B*Ho*Wo, C)), then
 * the per-input-pixel apply with the all-reduced sums and N. */
int zsg_bn_sync_relu_maxpool_bwd_sums(const float* dout, const uint8_t* idx, const float* x, int32_t B, int32_t H, int32_t W, int32_t C,
                                      const float* mean, const float* invstd, const float* gamma, const float* beta, int32_t k, int32_t s,
                                      int32_t p, int32_t Ho, int32_t Wo, double* sums, float* dgamma, float* dbeta, int32_t accumulate,
                                      void* ws, size_t ws_bytes, void* stream);
int zsg_bn_sync_relu_maxpool_bwd_apply(const float* dout, const uint8_t* idx, const float* x, int32_t B, int32_t H, int32_t W, int32_t C,
                                       const float* mean, const float* invstd, const float* gamma, const float* beta, int32_t k, int32_t s,
                                       int32_t p, int32_t Ho, int32_t Wo, const double* sums, const double* fwd_sums, float* dx, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Pooling / resampling / elementwise (NHWC, C % 4 == 0).
 * ------------------------------------------------------------------------------------------------------------- */
/* nn.MaxPool2d(k, s, p, ceil_mode) — mdl.py:152 (3,2,1), ssd_vgg.py:122,124,132.  idx: uint8 window position r * k + q (k <= 15,
 * both directions): the first maximum of the window, the last NaN if it holds one, its first in-bounds tap if every value is -inf
 * (torch's rules: the backward gives the window's gradient to that element). */
int zsg_maxpool_fwd(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k, int32_t s, int32_t p,
                    int32_t Ho, int32_t Wo, float* out, uint8_t* idx, void* stream);
int zsg_maxpool_bwd(const float* dout, const uint8_t* idx, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k,
                    int32_t s, int32_t p, int32_t Ho, int32_t Wo, float* dx, void* stream);
/* out = a + nearest_upsample(p -> Hd x Wd)   (F.interpolate(size=) + add, fpn_resnet.py:161-162,166-167) */
int zsg_upsample_add_fwd(const float* a, const float* p, int32_t B, int32_t Hs, int32_t Ws, int32_t Hd, int32_t Wd,
                         int32_t C, float* out, void* stream);
/* dp (+)= nearest-upsample adjoint of dout */
int zsg_upsample_add_bwd(const float* dout, int32_t B, int32_t Hs, int32_t Ws, int32_t Hd, int32_t Wd, int32_t C,
                         float* dp, int32_t accumulate, void* stream);
/* out = max(x,0) (fpn_resnet.py:172 F.relu(p6)) ; dx = dout * (x > 0) [+ dx] */
int zsg_relu_fwd(const float* x, int64_t n, float* out, void* stream);
int zsg_relu_bwd(const float* dout, const float* x, int64_t n, float* dx, int32_t accumulate, void* stream);
/* adaptive_avg_pool2d(.,1) — fpn_resnet.py:177 ; x [B][HW][C] -> out [B][C] ; and its adjoint */
int zsg_avgpool_fwd(const float* x, int32_t B, int32_t HW, int32_t C, float* out, void* stream);
int zsg_avgpool_bwd(const float* dout, int32_t B, int32_t HW, int32_t C, float* dx, int32_t accumulate, void* stream);
/* channel L2 normalisation x / ||x||_2 (no eps) — ssd_vgg.py:80, mdl.py:118-130 ; rows x C */
int zsg_l2norm_fwd(const float* x, int64_t rows, int32_t C, float* out, float* norm, void* stream);
int zsg_l2norm_bwd(const float* dout, const float* out, const float* norm, int64_t rows, int32_t C, float* dx,
                   void* stream);
/* image NCHW [B][3][H][W] -> NHWC4 [B][H][W][4] (4th channel zero) */
int zsg_nchw_to_nhwc4(const float* img, int32_t B, int32_t C, int32_t H, int32_t W, float* out, void* stream);
/* uint8 [pixels][3] (HWC, as PIL decodes) -> float [pixels][4] = (r,g,b)/255, 0 — `pil2tensor(img).float().div_(255)`
 * (dat_loader.py:26-33, 134) fused with the stem layout; IEEE division: equal to the host conversion bit for bit. */
int zsg_u8hwc_to_nhwc4(const uint8_t* img, int64_t pixels, float* out, void* stream);
/* Flip test-time augmentation (ZSGNet.eval_tta("flip"); csrc/tta.hip).
 * Staging: img uint8 [B][H][W][3] (_u8) or fp32 [B][3][H][W] (_f32) -> out [2B][H][W][4], 16-byte aligned.  For pixel (b, y, x) the four
 * floats zsg_u8hwc_to_nhwc4 / zsg_nchw_to_nhwc4 write for it go to row b at (y, x) and to row B + b at (y, W - 1 - x): rows 0..B-1 are
 * the batch as given, rows B..2B-1 its mirror along W, bit for bit what the plain entries give on the flipped image.  Every input
 * element is read once.  Returns -1 (nothing launched) for a null pointer, a non-positive size or a misaligned out. */
int zsg_tta_flip_stage_u8(const uint8_t* img, int32_t B, int32_t H, int32_t W, float* out, void* stream);
int zsg_tta_flip_stage_f32(const float* img, int32_t B, int32_t H, int32_t W, float* out, void* stream);
/* Merge: out5_2b [2B][A][5] (ty, tx, th, tw, att per anchor; rows B..2B-1 from the mirrored images) -> out [B][A][5].  levels = HOST
 * array int32 [L][4] of (first anchor, h, w, n) per pyramid level, anchor (y, x, k) of a level at first + (y * w + x) * n + k; its
 * partner under the mirror is p = first + (y * w + (w - 1 - x)) * n + k.  With u = out5_2b[b][a], v = out5_2b[B + b][p]:
 *   out[b][a] = 0.5f * (u0 + v0, u1 - v1, u2 + v2, u3 + v3, u4 + v4)
 * one fp32 add / subtract and one multiply each (reproducible in numpy; NaN and infinities propagate as IEEE has it).  Fixed order,
 * no atomics.  Returns -1 and launches nothing when a pointer is null, B or A is not positive, L is outside 1..ZSG_TTA_MAX_LEVELS, the
 * levels do not tile [0, A) exactly in order, or out overlaps the input. */
#define ZSG_TTA_MAX_LEVELS 8      /* as the loss kernels' level tables (zsg_match_atss) */
int zsg_tta_flip_merge(const float* out5_2b, int32_t B, int32_t A, const int32_t* levels, int32_t L, float* out, void* stream);
/* `img.resize((Wo, Ho))` of the reference loader (dat_loader.py:121: PIL.Image.resize, default filter = bicubic) for one uint8
 * [H][W][C] image, byte-identical to Pillow: its two fixed-point passes (horizontal into tmp [H][Wo][C], then vertical) with the
 * per-axis tap tables the HOST computes from the two axis lengths (bounds[o] = {first tap, tap count}, coef[o][ksize] 22-bit
 * fixed-point weights; zsgnet_pytorch_amd.dat_loader.resize_tables).  A NULL table pair = that axis keeps its length. */
int zsg_resize_u8(const uint8_t* src, int32_t H, int32_t W, int32_t C, const int32_t* x_bounds, const int32_t* x_coef, int32_t x_ksize,
                  const int32_t* y_bounds, const int32_t* y_coef, int32_t y_ksize, int32_t Ho, int32_t Wo, uint8_t* tmp, uint8_t* out,
                  void* stream);
/* The same for a whole batch in TWO launches (round 5): jobs = device array of
 * {int64 src, tmp, out; int64 x_bounds, x_coef, y_bounds, y_coef; int32 h, w, x_ksize, y_ksize, blk0_x, blk0_y, pad, pad} — absolute
 * device addresses of the raw image [h][w][C], its scratch [h][Wo][C] and its result [Ho][Wo][C], the tap tables of its horizontal and
 * vertical pass (an axis that keeps its length carries the identity table: one tap, coefficient 2^22), the first 1024-output block of
 * the job in each launch (blocks_x / blocks_y = their totals).  Byte-identical to zsg_resize_u8 (dat_loader.py:98-146, :121). */
int zsg_resize_u8_batched(const void* jobs_dev, int32_t njobs, int32_t C, int32_t Ho, int32_t Wo, int32_t blocks_x, int32_t blocks_y,
                          void* stream);
/* Training augmentation of a whole batch (3 channels): `img.crop(box).resize((Wo, Ho))` — the reference's resampling call,
 * dat_loader.py:121, applied to a window of the raw image — followed by brightness, contrast and saturation jitter, byte-identical to
 * zsgnet_pytorch_amd.dat_loader.augment_host.  jobs = device array of
 * {int64 src, tmp, out; int64 x_bounds, x_coef, y_bounds, y_coef; int32 h, w, pitch, x_ksize, y_ksize, blk0_x, blk0_y, pad;
 *  float brightness, contrast, saturation; int32 pad} (104 bytes): src = the address of the WINDOW's first pixel inside the raw image,
 * pitch = that image's row pitch in pixels, h / w = the window's sides (the tap tables are built for them), tmp = scratch [h][Wo][3]
 * (4-byte aligned for dword stores), blk0_x / blk0_y = the first 256-pixel block of the job in launch 1 (h * Wo pixels) / in launches
 * 2 and 3 (Ho * Wo pixels), blocks_x / blocks_y their totals.  gray_sums: njobs uint32 accumulators (zeroed by launch 1; the mean
 * gray value contrast blends with is their exact integer sum / (Ho * Wo)); Ho * Wo <= 2^24.  Launch 3 (contrast, saturation; in place)
 * runs only when do_cs != 0: pass 0 when every job has contrast == saturation == 1. */
int zsg_augment_u8_batched(const void* jobs_dev, int32_t njobs, int32_t Ho, int32_t Wo, int32_t blocks_x, int32_t blocks_y,
                           void* gray_sums, int32_t do_cs, void* stream);
/* The same three launches for windows that may leave the image (zoom-out: the outside is a fill colour) and for the horizontal flip,
 * byte-identical to dat_loader.augment_host(..., flip, fill).  jobs = device array of
 * {int64 img, tmp, out; int64 x_bounds, x_coef, y_bounds, y_coef; int32 ih, iw; int32 wx0, wy0, wh, ww; int32 x_ksize, y_ksize;
 *  int32 blk0_x, blk0_y; int32 flags; uint32 fill; float brightness, contrast, saturation; int32 pad} (120 bytes): img = the address of
 * the IMAGE's pixel (0, 0), ih / iw = its height and width (the row pitch is the width), wx0 / wy0 = the window's origin in image
 * pixels (any sign), wh / ww = its sides (the tap tables are built for them), tmp = scratch [wh][Wo][3] (4-byte aligned), blk0_x /
 * blk0_y = the first 256-pixel block of the job in launch 1 (wh * Wo pixels) / in launches 2 and 3, flags bit 0 = mirror left-right
 * (applied last; launch 2 reads scratch column Wo - 1 - x for output column x), fill = r | g << 8 | b << 16.  Launch 1 takes a tap's
 * source pixel from the image only when it lies inside [0, ih) x [0, iw) and `fill` otherwise, through the same integer sum: no window
 * makes it read outside the image.  jobs_host (may be NULL): the same table in host memory; every record is then validated before
 * anything is launched (addresses, image and window sides in 1..32768, wh * Wo <= 2^28, the origin within +-2^24, the first blocks equal
 * to the running block sums and blocks_x / blocks_y to their totals).  gray_sums, do_cs, Ho * Wo <= 2^24: as zsg_augment_u8_batched.
 * Returns -1 (nothing launched) for a bad argument or record. */
int zsg_augment_geom_u8_batched(const void* jobs_dev, const void* jobs_host, int32_t njobs, int32_t Ho, int32_t Wo, int32_t blocks_x,
                                int32_t blocks_y, void* gray_sums, int32_t do_cs, void* stream);
/* Affine warp (rotation + shear about the image centre) and separable Gaussian blur of a finished uint8 batch, byte-identical to steps 6
 * and 7 of dat_loader.augment_host(..., warp, blur) — integers only.  jobs = device array (8-byte aligned) of
 * {int64 src, out; int32 m[6]; uint32 fill; int32 flags; int32 radius; int32 taps[17]; int32 pad[2]} (128 bytes): src / out = the
 * addresses of the job's image [Ho][Wo][3] and of its result; flags bit 0 = warp: output pixel (x, y) samples the source at the 16.16
 * position SU = m0 x + m1 y + m2, SV = m3 x + m4 y + m5 (64-bit sums: every int32 coefficient is valid) — ix = SU >> 16,
 * fx = (SU >> 8) & 255, likewise iy, fy; the four taps (iy, ix) .. (iy + 1, ix + 1), each `fill` (r | g << 8 | b << 16) when outside
 * [0, Ho) x [0, Wo); v = ((p00 (256 - fx) + p01 fx)(256 - fy) + (p10 (256 - fx) + p11 fx) fy + 32768) >> 16 per channel.  flags bit 1 =
 * blur: along x, then along y, (sum_k taps[k + radius] p[clamp(i + k, 0, n - 1)] + 32768) >> 16 over k = -radius .. radius, radius in
 * 0..8, taps >= 0 with sum 65536.  stages: bit 0 = some job warps, bit 1 = some job blurs; one launch for the warp, two for the blur,
 * none for a stage no job has, and a job without a stage passes through it unchanged.  tmp: scratch of njobs slices of Ho * Wo * 3
 * bytes rounded up to a multiple of 4 (4-byte aligned; needed with stages bit 1 only).  The sources are never written.  jobs_host (may
 * be NULL): the same table in host memory; every record is then validated before anything is launched (addresses, flags within
 * `stages`, radius, taps and their sum, fill < 2^24, sources / results / scratch in three disjoint address ranges).  Returns -1
 * (nothing launched) for a bad argument or record; Ho, Wo in 1..32768. */
int zsg_augment_warp_u8_batched(const void* jobs_dev, const void* jobs_host, int32_t njobs, int32_t Ho, int32_t Wo, void* tmp, int32_t stages,
                                void* stream);
/* Head input BackBone.concat_we (mdl.py:69-104) + head conv0 (mdl.py:216, 514 -> 256, 3x3 pad 1) without ever materialising
 * the concatenated tensor, and without its spatially-constant input channels: the language vector
 * is constant over the image and the grid channels do not depend on the batch index, so only the 256 feature channels
 * go through the implicit GEMM (half the MACs of the reference's dense conv); their contribution is an additive map
 *   out[b][p][n] = G[p][n] + sum_{tap valid at p} V[b][n*9 + tap],   V = W[:, :, lang] * we[b]  (tiny GEMM),
 * and the backward needs the validity-masked sums  S1[b][n*9+tap] += sum_{p: tap valid at p} dy[b][p][n]  (S2 = the
 * [n*9+tap][b] transpose) plus the batch sum of dy for the grid weights.  The masked sums come by inclusion-exclusion
 * from nine plain per-image sums Q (all pixels, first/last row, first/last column, four corners) that
 * zsg_head_border_sums accumulates level by level (caller zeroes Q) and zsg_head_border_finalize turns into S1, S2 and,
 * optionally, the bias gradient sum_b Q[0][b][:].  dy / out: one pyramid level [B][h*w][N]. */
int zsg_head_lang_map(const float* V, const float* G, int32_t B, int32_t h, int32_t w, int32_t N, float* out, void* stream);
/* Per-forward input staging in one launch (round 5): what `batch[k].to(device)` of the trainer (utils.py:403-405), the zero padding of
 * the query bucket, lstm_init_hidden's host draws (mdl.py:279-294: hc_src = h0 | c0, hc_n floats, may be PINNED HOST memory) and the
 * BatchNorm layers' num_batches_tracked += 1 (n_nbt int64 counters; 0 in eval mode) do at the head of ZSGNet.forward.
 * qvec [B][T][E] device fp32 -> qbuf [B][Tplan][E] (zeros behind T); qlens [B] (int64, or fp32 when qlens_f32) -> qlens_dst float [B]. */
int zsg_stage_inputs(const float* qvec, int32_t B, int32_t T, int32_t E, int32_t Tplan, float* qbuf, const void* qlens, int32_t qlens_f32, float* qlens_dst,
                     const float* hc_src, int32_t hc_n, float* hc_dst, int64_t* nbt, int32_t n_nbt, void* stream);
/* the same map for ALL pyramid levels in one launch (round 5): `out` [B][h_i*w_i][N] per level, levels packed level-major (level i
 * starts at B * N * sum_{j<i} h_j w_j); G (or NULL) packed the same way with B = 1; hw = {h_0, w_0, h_1, w_1, ...} (host memory,
 * nlev <= ZSG_MAX_SEG pairs).  A block sums V's taps once per border class instead of once per output element. */
int zsg_head_lang_map_packed(const float* V, const float* G, int32_t B, int32_t nlev, const int32_t* hw, int32_t N, float* out, void* stream);
/* conv0's epilogue of the eval-only shared-image plan (Q queries over Bi <= Q images, one launch per head stack):
 *   h1[q][p][n] = relu( Y[img_idx[q]][p][n] + bias[n] + G[p][n] + sum_{tap valid at p} V[q][n*9 + tap] )
 * Y [Bi][h_i*w_i][N]: the raw accumulator of conv0's feature GEMM (no bias, no ReLU); G (or NULL) and `out` as in
 * zsg_head_lang_map_packed with batch counts 1 and Q; V [Q][N*9] or NULL; img_idx: Q device integers (int64 when idx_i64, else int32),
 * read by the kernel — a value outside [0, Bi) yields NaN rows for that query and no access outside Y.  Image slots no query points to
 * are never read.  Summation order: ((Y + G) + (taps row-major + bias)); N % 4 == 0, N <= 1024. */
int zsg_head_shared_conv0(const float* Y, const void* img_idx, int32_t idx_i64, const float* bias, const float* G, const float* V, int32_t Bi, int32_t Q,
                          int32_t nlev, const int32_t* hw, int32_t N, float* out, void* stream);
/* Backward of that sharing point (the shared-image training plan; the reference has no counterpart: it is the adjoint of the
 * `Y[img_idx[q]]` read above, i.e. of concat_we's per-pair feature copy, mdl.py:69-104, folded over the queries of one image):
 *   dY[i][p][n] = sum over q ascending with img_idx[q] == i of dy[q][p][n]
 * dy [Q][h_i*w_i][N] per level (the gradient of h1, already ReLU-masked), dY [Bi][h_i*w_i][N] per level, both packed level-major.
 * dY is WRITTEN (no zero fill needed): an image slot no query points to gets zeros.  A query whose index lies outside [0, Bi)
 * contributes to no slot; nothing is read or written outside the buffers.  Fixed order, plain fp32 adds, no atomics: bit-identical
 * run to run.  img_idx is read by the kernel.  N % 4 == 0, N <= 1024, Q <= 8192. */
int zsg_head_shared_conv0_bwd(const float* dy, const void* img_idx, int32_t idx_i64, int32_t Bi, int32_t Q, int32_t nlev, const int32_t* hw, int32_t N,
                              float* dY, void* stream);
/* FiLM language modulation of head conv0 (cfg lang_fuse = "film"; csrc/film.hip).  zsg_head_shared_conv0 with a per-query, per-channel
 * scale on the feature accumulator:
 *   h1[q][p][n] = relu( (1 + gamma[q][n]) * Y[img_idx[q]][p][n] + bias[n] + G[p][n] + sum_{tap valid at p} V[q][n*9 + tap] )
 * Layouts, block order and the out-of-range rule (NaN rows, no access outside Y) are zsg_head_shared_conv0's; gamma [Q][N] fp32.
 * img_idx == NULL is the identity (query q reads image q) and requires Bi == Q.  FIXED ORDER, each operation rounded on its own:
 * s = 1.0f + gamma; t = s * Y; c = (taps row-major, summed from 0) + bias; h1 = relu((t + G) + c) (without G: relu(t + c)) — with
 * gamma = 0 the output carries the bits of zsg_head_shared_conv0.  out_bf16 = 1: `out` is bf16 [same offsets], the fp32 result rounded
 * once to nearest-even (zsg_head_shared_conv0_bf16's store).  N % 4 == 0, N <= 1024.
 * HBM bytes: (Q + Bi) * P * N * 4 (bf16 out: Q * 2 + Bi * 4), P = sum of h_i * w_i. */
int zsg_head_film_conv0(const float* Y, const void* img_idx, int32_t idx_i64, const float* bias, const float* G, const float* V, const float* gamma,
                        int32_t Bi, int32_t Q, int32_t nlev, const int32_t* hw, int32_t N, void* out, int32_t out_bf16, void* stream);
/* Its backward into the per-image accumulator (zsg_head_shared_conv0_bwd with each query's row scaled):
 *   dY[i][p][n] = sum over q ascending with img_idx[q] == i of (1 + gamma[q][n]) * dy[q][p][n]
 * plain fp32 (s = 1.0f + gamma; the product rounded, then added to the running sum, which starts at 0), no atomics, every element of
 * dY WRITTEN (zeros for a slot no query points to; an out-of-range index contributes to no slot).  With gamma = 0 it has the bits of
 * zsg_head_shared_conv0_bwd.  img_idx == NULL: identity, Bi == Q.  N % 4 == 0, N <= 1024, Q <= 8192.  HBM bytes: (Q + Bi) * P * N * 4. */
int zsg_head_film_conv0_bwd(const float* dy, const void* img_idx, int32_t idx_i64, const float* gamma, int32_t Bi, int32_t Q, int32_t nlev,
                            const int32_t* hw, int32_t N, float* dY, void* stream);
/* The gradient of the scale:  dgamma[q][n] = sum_p dy[q][p][n] * Y[img_idx[q]][p][n]  over all levels.  Accumulated in fp64 in an order
 * fixed by (P, N, Q) alone (per-query parts write fp64 partials [q][part][N] into ws, a finalize launch adds the parts in index order) and
 * rounded to fp32 ONCE: |error| <= 2^-23 * sum_p |dy * Y|; no float atomics, the same bits on every run.  A query whose index lies
 * outside [0, Bi) reads nothing and gets zeros.  dgamma_t (or NULL): the transposed copy [N][Q], written by the same finalize launch.
 * ws: zsg_head_film_dgamma_ws_bytes(Q, nlev, hw, N) bytes (-1 for a bad argument), 8-byte aligned.  N % 4 == 0, N <= 1024.
 * HBM bytes: about 2 * Q * P * N * 4 (dy once; Y once per query, from L2 for the later queries of an image) + the partials twice. */
int64_t zsg_head_film_dgamma_ws_bytes(int32_t Q, int32_t nlev, const int32_t* hw, int32_t N);
int zsg_head_film_dgamma(const float* dy, const float* Y, const void* img_idx, int32_t idx_i64, int32_t Bi, int32_t Q, int32_t nlev, const int32_t* hw,
                         int32_t N, float* dgamma, float* dgamma_t, void* ws, int64_t ws_bytes, void* stream);
/* Word-level attention modulation of head conv0 (cfg lang_fuse = "words"; csrc/words.hip).  zsg_head_film_conv0 with a scale that
 * depends on the pixel: the raw accumulator row Y[img_idx[q]][p] is the attention query over the projected tokens of phrase q,
 *   s_t = scale * sum_n Y[img_idx[q]][p][n] * Kw[q][t][n]   (t < len),   alpha = softmax over t < len of s (max subtracted),
 *   gamma[n] = sum_t alpha_t * Vw[q][t][n],   h1[q][p][n] = relu( (1 + gamma[n]) * Y[..][n] + bias[n] + G[p][n] + taps of V[q] )
 * Kw, Vw [Q][T][N] fp32; lens [Q] float as the collater makes it, len = clamp(lens[q], 0, T) (a NaN counts as 0); only rows t < len of
 * Kw / Vw are ever read.  len = 0: alpha = 0, gamma = 0.  alpha (or NULL): [Q][P][T] packed like `out` (row (Q * p0_i + q * h_i w_i + px)
 * of T floats), every element written, exact zeros at t >= len and for an out-of-range query.  Layouts, img_idx (int32 / int64 / NULL =
 * identity, Bi == Q), the out-of-range rule (NaN rows, no access outside Y) and out_bf16 are zsg_head_film_conv0's.
 * FIXED ORDER, each operation rounded on its own: tokens ascending everywhere; a dot product is summed per lane over the channels
 * 4 (l + 64 k) + e (k, then e, ascending from 0) and across the 64 lanes by a 6-step xor butterfly (offsets 32 .. 1); the softmax sums
 * exp(s_t - max) by the same butterfly and divides; gamma is summed from 0; then film's  s = 1.0f + gamma; t = s * Y;
 * c = (taps row-major, summed from 0) + bias; h1 = relu((t + G) + c).  With Vw = 0 the output carries the bits of zsg_head_shared_conv0;
 * with every len = 1 (alpha = 1 exactly) those of zsg_head_film_conv0 for gamma = Vw[:, 0].  N % 4 == 0, N <= 1024, 1 <= T <= 64.
 * HBM bytes: (Q + Bi) * P * N * 4 (bf16 out: Q * 2 + Bi * 4) + Q * P * T * 4 for alpha + 2 * Q * T * N * 4; about 4 * len * N flops per
 * pixel row (fp32 vector math). */
int zsg_head_words_conv0(const float* Y, const void* img_idx, int32_t idx_i64, const float* bias, const float* G, const float* V, const float* Kw,
                         const float* Vw, const float* lens, float scale, int32_t Bi, int32_t Q, int32_t T, int32_t nlev, const int32_t* hw, int32_t N,
                         void* out, int32_t out_bf16, float* alpha, void* stream);
/* Its backward.  dy [Q][P][N] is the ReLU-masked gradient of h1, alpha the forward's:
 *   dgamma = dy * Y;   dalpha_t = dgamma . Vw_t;   ds_t = alpha_t (dalpha_t - sum_k alpha_k dalpha_k)
 *   dYq[q][p]  = (1 + gamma) * dy + scale * sum_t ds_t Kw_t       (gamma recomputed from alpha and Vw in the forward's order;
 *                                                                  s = 1.0f + gamma; a = s * dy; b = scale * sum; dYq = a + b)
 *   dKw[q][t] = scale * sum_p ds_t(p) * Y[img_idx[q]][p]          dVw[q][t] = sum_p alpha_t(p) * dgamma(p)
 * dYq [Q][P][N] packed like dy: one row per query, every element written (a shared-image plan folds it into the per-image accumulator
 * with zsg_head_shared_conv0_bwd; with Vw = 0 it carries dy's values).  dKw / dVw [Q][T][N]: the sums over p run in fp64 (every term one
 * fma of exact fp32 products) in an order fixed by (P, N, Q, T) alone — per-block partials in ws, then a finalize launch adds the parts in
 * index order — and are rounded to fp32 ONCE (dKw after the fp64 product with scale): given the fp32 ds / alpha of the first launch,
 * |error| <= 2^-23 * scale * sum_p |ds_t * Y|  resp.  2^-23 * sum_p |alpha_t * dy * Y|.  Rows t >= len are exact zeros; a query whose
 * index lies outside [0, Bi) reads nothing and gets zeros everywhere.  No float atomics: the same bits on every run.  Each of dYq, dKw,
 * dVw may be NULL (a frozen consumer), not all three; with dVw alone the per-pixel launch (dYq, ds) is not issued.  ws: zsg_head_words_bwd_ws_bytes(Q, T, nlev, hw, N) bytes (-1 for a bad argument),
 * 16-byte aligned.  N % 4 == 0, N <= 1024, 1 <= T <= 64.
 * HBM bytes: 3 * Q * P * N * 4 (dy, Y, dYq) + 2 * Q * P * T * 4 for the pixel launch; dy and Y once more per tile of 4 tokens below
 * max len (from L2 where they fit) and the fp64 partials twice for dKw / dVw. */
int64_t zsg_head_words_bwd_ws_bytes(int32_t Q, int32_t T, int32_t nlev, const int32_t* hw, int32_t N);
int zsg_head_words_conv0_bwd(const float* dy, const float* Y, const void* img_idx, int32_t idx_i64, const float* Kw, const float* Vw, const float* alpha,
                             const float* lens, float scale, int32_t Bi, int32_t Q, int32_t T, int32_t nlev, const int32_t* hw, int32_t N, float* dYq,
                             float* dKw, float* dVw, void* ws, int64_t ws_bytes, void* stream);
/* Global-context block of the head towers (cfg head_ctx = "gc"; csrc/gcblock.hip; GCNet, Cao et al. 2019).  Per query q and pyramid level
 * l, over the rows x_p (p < P = h_l * w_l) of the post-ReLU h1, N = 256, M = N / 4 = 64:
 *   s_p = key . x_p;   alpha = softmax_p(s) (max subtracted);   c = sum_p alpha_p x_p
 *   u = W1 c + b1;     uh = (u - mean u) / sqrt(var u + 1e-5) (biased variance over M);   r = relu(lnw * uh + lnb)
 *   t = W2 r + b2;     y_p = x_p + t
 * x, y [level][Q][P_l][N] fp32, the packed head layout of zsg_head_film_conv0's output (hw: nlev (h, w) pairs); key [N], W1 [M][N],
 * b1 / lnw / lnb [M], W2 [N][M], b2 [N].  All arithmetic is fp32.  With W2 = 0 and b2 = 0, t = 0 and y carries x's values.
 * Training saves s [level][Q][P_l] (the logits, packed like the rows of x) and stat [level][Q][ZSG_GC_STAT_LD]: the (q, l)'s softmax
 * max and denominator, var u, 1 / sqrt(var u + 1e-5), c, uh and r at the ZSG_GC_STAT_* offsets; eval passes s = stat = NULL and saves nothing.
 * Three launches (chunk partials of 64 rows; combine + MLP per (q, l); the add); no float atomics, no hand-offs between blocks; every
 * sum's order is fixed by (Q, hw): the same bits on every run.  ws: zsg_head_gc_fwd_ws_bytes(Q, nlev, hw, N) bytes, 16-byte aligned.
 * Refused with -1 and the argument's name, nothing launched: a NULL pointer, N != 256, nlev outside [1, ZSG_MAX_SEG], Q < 1, an empty
 * level, a short workspace, x / y / key / W1 / W2 / ws off 16-byte alignment.
 * HBM bytes: 3 * Q * P * N * 4 (x twice — the second read of a 64-row chunk comes from registers, the add's from memory — and y). */
#define ZSG_GC_STAT_MAX 0
#define ZSG_GC_STAT_DEN 1
#define ZSG_GC_STAT_VAR 2
#define ZSG_GC_STAT_RSTD 3
#define ZSG_GC_STAT_C 4        /* [256] */
#define ZSG_GC_STAT_UHAT 260   /* [64] */
#define ZSG_GC_STAT_R 324      /* [64] */
#define ZSG_GC_STAT_LD 388
int64_t zsg_head_gc_fwd_ws_bytes(int32_t Q, int32_t nlev, const int32_t* hw, int32_t N);
int zsg_head_gc_fwd(const float* x, const float* key, const float* W1, const float* b1, const float* lnw, const float* lnb, const float* W2,
                    const float* b2, int32_t Q, int32_t nlev, const int32_t* hw, int32_t N, float* y, float* s, float* stat, void* ws,
                    int64_t ws_bytes, void* stream);
/* Its backward, g = dL/dy [level][Q][P_l][N], s / stat the forward's:
 *   dt = sum_p g_p;  db2 = dt;  dW2 = dt r^T;  dr = W2^T dt;  dv = dr * [r > 0];  dlnw = dv * uh;  dlnb = dv;  duh = dv * lnw
 *   du = (duh - mean duh - uh * mean(duh * uh)) / sqrt(var u + 1e-5);  db1 = du;  dW1 = du c^T;  dc = W1^T du
 *   a_p = dc . x_p;  abar = sum_p alpha_p a_p;  ds_p = alpha_p (a_p - abar);  dx_p = g_p + alpha_p dc + ds_p key;  dkey = sum_p ds_p x_p
 * dx is the gradient of the post-ReLU x (the caller applies the ReLU mask).  With W2 = 0: dc = 0, every a_p and ds_p is 0 and dx
 * carries g's values.  The seven parameter gradients are summed over every (q, l): the column sums of g run in fp64, the chain
 * dt -> dc -> ds in fp32 per (q, l), and the final sums over (q, l) (dkey: over the 64-row chunk partials of sum ds_p x_p) are fp64 fmas
 * of exact fp32 products in index order, rounded to fp32 ONCE; accumulate != 0 adds that value to the output (the flat gradient
 * buffer's convention), 0 stores it.  Any of dx and the seven gradients may be NULL (a frozen parameter, nothing in front of x), not
 * all eight; without dx and dkey the two per-row launches are not issued.  Up to five launches, no float atomics, no hand-offs between
 * blocks, the same bits on every run.  ws: zsg_head_gc_bwd_ws_bytes(Q, nlev, hw, N) bytes, 16-byte aligned.  Refusals as the forward's.
 * HBM bytes: Q * P * N * 4 * (g for the column sums + x for a_p + g and dx + x for dkey). */
int64_t zsg_head_gc_bwd_ws_bytes(int32_t Q, int32_t nlev, const int32_t* hw, int32_t N);
int zsg_head_gc_bwd(const float* g, const float* x, const float* s, const float* stat, const float* key, const float* W1, const float* lnw,
                    const float* W2, int32_t Q, int32_t nlev, const int32_t* hw, int32_t N, float* dx, float* dkey, float* dW1, float* db1,
                    float* dlnw, float* dlnb, float* dW2, float* db2, int32_t accumulate, void* ws, int64_t ws_bytes, void* stream);
int zsg_head_border_sums(const float* dy, int32_t B, int32_t h, int32_t w, int32_t N, float* Q /* [9][B][N], += */, void* stream);
int zsg_head_border_finalize(const float* Q, int32_t B, int32_t N, float* S1, float* S2, float* bias_grad /* [N], += ; or NULL */,
                             void* stream);
int zsg_batch_sum(const float* x, int32_t B, int64_t stride, float* out, void* stream);

/* Separate attention / box heads (use_same_atb = False, mdl.py:220-225, 383-389): their [rows][groups*k] outputs are
 * interleaved into the [B, A, 5] tensor the loss / evaluator read (dir 0), and the incoming gradient is split the same
 * way (dir 1):  strided[(r*groups + a)*group_stride + offset + e] <-> compact[(r*groups + a)*k + e]. */
int zsg_interleave(float* compact, int64_t rows, int32_t groups, int32_t k, float* strided, int32_t group_stride, int32_t offset,
                   int32_t dir, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * BiLSTM query encoder — nn.LSTM(300,128,bidirectional) on a PackedSequence + last-token gather, mdl.py:296-336.
 * gin: input projections x_t W_ih^T + b_ih  [B][T][4H] (made with zsg_conv_igemm);  one launch per direction.
 * The sorted-position rule (h0/c0 [B][H] of this direction are indexed by the rank of the sample in a stable
 * descending sort of the lengths, mdl.py:309) is evaluated on device.
 * forward direction: lens = qlens (float, as the collater makes them, dat_loader.py:193);
 * reverse direction: one cell step on x[len-1]: pass T=1, lens=NULL (all ones).
 * Saves for backward: gates [B][T][4H] (post-activation i,f,g,o), cst [B][T][H] (c_t), hprev [B][T][H] (h_{t-1}).
 * out: h at the last valid step, written to we[b*we_ld + we_off : +H].
 * ------------------------------------------------------------------------------------------------------------- */
int zsg_lstm_gather_last(const float* qvec, const float* qlens, int32_t B, int32_t T, int32_t E, float* out,
                         void* stream);
int zsg_lstm_fwd(const float* gin, const float* w_hh, const float* b_hh, const float* h0, const float* c0,
                 const float* qlens_rank, const float* lens, int32_t B, int32_t T, int32_t H, float* gates,
                 float* cst, float* hprev, float* we, int32_t we_ld, int32_t we_off, void* stream);
/* dgates [B][T][4H] (zero beyond the sample's length) from dwe; weight grads then come from zsg_conv_wgrad/colsum */
int zsg_lstm_bwd(const float* dwe, int32_t we_ld, int32_t we_off, const float* w_hh, const float* gates,
                 const float* cst, const float* c0, const float* qlens_rank, const float* lens, int32_t B, int32_t T,
                 int32_t H, float* dgates, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Full-sequence query pooling (cfg lang_pool = final / mean / attn; csrc/lstm_seq.hip).
 * With f_t the forward state after x_0..x_t and r_t the reverse state after x_{len-1}, .., x_t (len = clamp(lens[b], 0, T),
 * each direction from row rank[b] of its h0 / c0 as above), o_t = [f_t | r_t] for t < len is nn.LSTM's padded output:
 *   final  we = [f_{len-1} | r_0]  (nn.LSTM's h_n);   mean  we = (1/len) sum_{t<len} o_t;
 *   attn   s_t = w . o_t,  alpha = softmax over t < len of s (max subtracted),  we = sum_t alpha_t o_t.
 *
 * zsg_lstm_seq_fwd: zsg_lstm_fwd with a walk direction and the state of every step as an output.  reverse = 1 walks
 * t = len-1 .. 0.  hseq [B][T][hs_ld] (optional): h of the step that consumed token t, written to [hs_off, hs_off + H) of row
 * (b, t) and exactly 0 there at t >= len — every element of the window is written, nothing outside it.  we (optional): the
 * state after the walk's last step (the starting state at len = 0), window as zsg_lstm_fwd.  One of hseq / we is required.
 * gates / cst / hprev are saved at TOKEN positions; hprev[t] is the state the step at t started from.  lens = NULL: all ones.
 * H in {32, 64, 128, 256}, others return -1.  reverse = 0 with we alone computes zsg_lstm_fwd's bits.
 *
 * zsg_lstm_seq_bwd: BPTT in the walk's reverse order.  dwe (optional; gradient of the end state, window as zsg_lstm_bwd) starts dh,
 * dhseq [B][T][hs_ld] (optional; window [hs_off, hs_off + H)) is added to dh at every step; one of the two is required.
 * dgates [B][T][4H] at token positions, exactly 0 at t >= len; c_prev is cst at the walk's previous step, or c0.
 * Weight gradients: zsg_conv_wgrad / zsg_colsum over the token-aligned rows, as for zsg_lstm_bwd.
 *
 * zsg_lang_pool_fwd: hseq [B][T][D] (dense; 0 at t >= len) -> we [B][D]; one workgroup per query.  mode ZSG_LANG_POOL_ATTN reads
 * w [D] and writes alpha [B][T] (optional; 0 at t >= len); ZSG_LANG_POOL_MEAN takes w = alpha = NULL.  len = 0: we = 0.
 * zsg_lang_pool_bwd: dalpha_t = dwe . o_t, ds_t = alpha_t (dalpha_t - sum_k alpha_k dalpha_k), dhseq_t = alpha_t dwe + ds_t w
 * (mean: dhseq_t = dwe / len); dhseq [B][T][D] is written everywhere, 0 at t >= len; ds [B][T] (optional) likewise.
 * zsg_lang_pool_wgrad: dw[d] (+)= sum_b sum_t ds[b][t] hseq[b][t][d]; per column 16 interleaved partial sums over the rows (b, t), each
 * in ascending order, added in a fixed order.
 * No float atomics in any of them: the same inputs give the same bits.
 * ------------------------------------------------------------------------------------------------------------- */
#define ZSG_LANG_POOL_MEAN 0
#define ZSG_LANG_POOL_ATTN 1
int zsg_lstm_seq_fwd(const float* gin, const float* w_hh, const float* b_hh, const float* h0, const float* c0,
                     const float* qlens_rank, const float* lens, int32_t B, int32_t T, int32_t H, int32_t reverse,
                     float* gates, float* cst, float* hprev, float* hseq, int32_t hs_ld, int32_t hs_off, float* we,
                     int32_t we_ld, int32_t we_off, void* stream);
int zsg_lstm_seq_bwd(const float* dwe, int32_t we_ld, int32_t we_off, const float* dhseq, int32_t hs_ld, int32_t hs_off,
                     const float* w_hh, const float* gates, const float* cst, const float* c0, const float* qlens_rank,
                     const float* lens, int32_t B, int32_t T, int32_t H, int32_t reverse, float* dgates, void* stream);
int zsg_lang_pool_fwd(const float* hseq, const float* lens, const float* w, int32_t mode, int32_t B, int32_t T, int32_t D,
                      float* we, float* alpha, void* stream);
int zsg_lang_pool_bwd(const float* dwe, const float* hseq, const float* lens, const float* w, const float* alpha,
                      int32_t mode, int32_t B, int32_t T, int32_t D, float* dhseq, float* ds, void* stream);
int zsg_lang_pool_wgrad(const float* ds, const float* hseq, int32_t B, int32_t T, int32_t D, float* dw, int32_t accumulate,
                        void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Anchor matching + focal / smooth-L1 loss, forward and backward in one call — ZSGLoss.forward, loss.py:43-143
 * (IoU_values anchors.py:90-116, simple_match_anchors :153-165, bbox_to_reg_params :168-179).
 * out5: network output [B][A][5] = (dy,dx,dh,dw,att);  annot [B][4] y1x1y2x2;  anchors [A][4] fp32 tlbr.
 * losses[3] = (loss, cls_ls, box_ls);  grad5 [B][A][5] = d loss / d out5 (already includes lamb_reg, 1/B, 1/#pos).
 * match_idx [B] int32 = arg-max-IoU anchor (lowest index wins; bit-exact IoU: no FMA contraction, IEEE divide).
 * flags: bit0 use_focal, bit1 use_multi, bit2 use_softmax.  NaN branch (loss.py:128-133) is taken on device.
 * Limit: B <= 512 samples per call (one LDS record per sample in the merge kernel); larger batches are rejected with -1
 * (the reference's per-GPU batches are 16-32, BASELINE configs; split a larger batch over calls and sum the losses).
 * ------------------------------------------------------------------------------------------------------------- */
size_t zsg_loss_workspace_bytes(int32_t B, int32_t A);   /* one size for zsg_loss_fwd_bwd, _iou, _q and _m */
int zsg_loss_fwd_bwd(const float* out5, const float* annot, const float* anchors, int32_t B, int32_t A, float alpha,
                     float gamma, float lamb_reg, float match_thr, int32_t flags, float grad_scale, float* losses,
                     float* grad5, int32_t* match_idx, int32_t* npos, void* ws, size_t ws_bytes, void* stream);
/* zsg_loss_fwd_bwd with a box IoU term (no counterpart in the reference, whose criterion stops at loss.py:91's smooth-L1; it extends
 * that criterion, and the pieces are the reference's: the positives of simple_match_anchors anchors.py:153-165, the decode of
 * reg_params_to_bbox anchors.py:182-197).  For every positive anchor, p = the decoded box, g = annot, eps = 1e-7:
 *   inter = max(min(p.y2,g.y2) - max(p.y1,g.y1), 0) * (same in x);  union = area(p) + area(g) - inter;  iou = inter / (union + eps);
 *   ey = max(p.y2,g.y2) - min(p.y1,g.y1), ex likewise;
 *   iou_kind 1 (giou): L = 1 - iou + (ey ex - union) / (ey ex + eps)
 *   iou_kind 2 (diou): L = 1 - iou + |centre(p) - centre(g)|^2 / (ey^2 + ex^2 + eps)
 * iou_ls = mean over samples of (sum of L over the sample's positives / #pos);  loss = lamb_reg box_ls + lamb_iou iou_ls + cls_ls.
 * losses[4] = (loss, cls_ls, box_ls, iou_ls); grad5 also carries d(lamb_iou iou_ls) / d out5[..,0:4] (through the decode, exp
 * included; positives only; the classification gradient is that of zsg_loss_fwd_bwd bit for bit).  NaN branch: box_ls, cls_ls or
 * iou_ls NaN -> the constants of loss.py:128-133, iou_ls = 0, grad5 = 0.  Same launches, limits and workspace as zsg_loss_fwd_bwd. */
int zsg_loss_fwd_bwd_iou(const float* out5, const float* annot, const float* anchors, int32_t B, int32_t A, float alpha,
                         float gamma, float lamb_reg, float match_thr, int32_t flags, float grad_scale, int32_t iou_kind,
                         float lamb_iou, float* losses, float* grad5, int32_t* match_idx, int32_t* npos, void* ws,
                         size_t ws_bytes, void* stream);
/* zsg_loss_fwd_bwd_iou with an IoU-aware classification target (no counterpart in the reference, whose att logit is trained against the
 * hard 0 / 1 positives mask alone, loss.py:73-87 and :111-125).  x = the att logit, s = sigmoid(x), m = the positives mask exactly as
 * above, q = m ? iou : 0 with iou the very iou defined above for the decoded box of the anchor (evaluated for every positive also when
 * iou_kind = 0), held constant: no gradient flows through q into the box channels.  BCE(x, q) = max(x,0) - x q + log1p(exp(-|x|)).
 *   cls_kind 0 (none): the classification term of zsg_loss_fwd_bwd
 *   cls_kind 1 (qfl):  l = |q - s|^gamma BCE(x, q) for every anchor                    (Quality Focal Loss, Li et al. 2020)
 *   cls_kind 2 (vfl):  l = q BCE(x, q) at positives, alpha s^gamma BCE(x, 0) at negatives   (Varifocal Loss, Zhang et al. 2021)
 * cls_ls = sum of l over all samples and anchors / sum of m (loss.py:125's normaliser); its gradient is the true derivative of l with
 * respect to x, through the modulating factor (unlike the focal weights of loss.py:118, which are detached).  cls_kind 1 / 2 need
 * flags bit0 set, bit2 clear and gamma >= 1 (else -1).  iou_kind: 0 (no IoU term, iou_ls = 0), 1, 2.
 * losses[5] = (loss, cls_ls, box_ls, iou_ls, pos_iou), pos_iou = mean over samples of (sum of q over the sample's positives / #pos).
 * With cls_kind = 0, losses[0:4], grad5, match_idx and npos are those of zsg_loss_fwd_bwd (iou_kind 0) / zsg_loss_fwd_bwd_iou bit for
 * bit (outside the NaN branch).  NaN branch: box_ls, cls_ls or iou_ls NaN -> the constants of loss.py:128-133, iou_ls = pos_iou = 0
 * and grad5 = +0 everywhere, for every cls_kind and iou_kind (zsg_loss_fwd_bwd writes 0 * derivative there: a -0 or a NaN may remain).
 * Same launches, limits and workspace as zsg_loss_fwd_bwd. */
int zsg_loss_fwd_bwd_q(const float* out5, const float* annot, const float* anchors, int32_t B, int32_t A, float alpha, float gamma,
                       float lamb_reg, float match_thr, int32_t flags, float grad_scale, int32_t iou_kind, float lamb_iou,
                       int32_t cls_kind, float* losses, float* grad5, int32_t* match_idx, int32_t* npos, void* ws, size_t ws_bytes,
                       void* stream);
/* zsg_loss_fwd_bwd_q on a positives mask made beforehand (ZSGLoss.forward with cfg matcher = "atss"; no counterpart in the reference,
 * whose positives are simple_match_anchors' fixed rule, anchors.py:153-165 as called at loss.py:73-87).  pos_mask [B][A] uint8: anchor a
 * of sample b is positive where pos_mask[b][a] != 0 or a is the sample's arg-max IoU anchor (lowest index, as above: every sample keeps a
 * positive, match_idx and the NaN branch keep their meaning).  flags bit1 (use_multi) and match_thr are not consulted.  Everything else
 * is zsg_loss_fwd_bwd_q's: the sums and their order, grad_scale, losses[5], match_idx, npos, the limits, the workspace
 * (zsg_loss_workspace_bytes) and the launches.  Given the mask of the fixed rule it returns zsg_loss_fwd_bwd_q's bits. */
int zsg_loss_fwd_bwd_m(const float* out5, const float* annot, const float* anchors, int32_t B, int32_t A, float alpha, float gamma,
                       float lamb_reg, float match_thr, int32_t flags, float grad_scale, int32_t iou_kind, float lamb_iou,
                       int32_t cls_kind, const uint8_t* pos_mask, float* losses, float* grad5, int32_t* match_idx, int32_t* npos,
                       void* ws, size_t ws_bytes, void* stream);
/* ATSS anchor assignment (Adaptive Training Sample Selection, Zhang et al. 2020) — ZSGLoss.forward with cfg matcher = "atss", in the
 * place of simple_match_anchors anchors.py:153-165; the mask goes to zsg_loss_fwd_bwd_m.  One annotation g = annot[b] per sample.
 * level_off [L + 1] int32 in HOST memory (read before anything is launched): pyramid level l owns the anchors
 * [level_off[l], level_off[l + 1]) of create_anchors' flattened order, level_off[0] = 0, level_off[L] = A, strictly ascending.
 * All fp32, in this order, no contraction:
 *   acy = (a.y1 + a.y2) / 2, acx = (a.x1 + a.x2) / 2;  gcy, gcx likewise;  d(a) = (acy - gcy)(acy - gcy) + (acx - gcx)(acx - gcx)
 *   C = per level the min(topk, n_l) anchors with the smallest key (d, index), lexicographic; ordered by level, then by rank
 *   v(a) = IoU(g, a) exactly as zsg_loss_fwd_bwd's;  t = mean(v over C) + std(v over C): fp64 from the fp32 values, summed in the order
 *   of C, mean = sum v / |C|, std = sqrt(sum (v - mean)^2 / (|C| - 1)), 0 for |C| = 1
 *   positive: (a in C and (double)v(a) >= t and g.y1 < acy < g.y2 and g.x1 < acx < g.x2)  or  a == the arg-max IoU anchor of the sample
 * pos_mask [B][A] uint8: every byte is written, 0 or 1.  thr [B] double = t (may be null).  cand [B][8 * 16] int32 = C in its order,
 * -1 behind it (may be null).  Two launches, no atomics, no host synchronisation, the same bits on every run.
 * Limits (else -1, nothing launched): 1 <= L <= 8, 1 <= topk <= 16, B <= 512, level_off as above. */
size_t zsg_match_atss_workspace_bytes(int32_t B, int32_t L);
int zsg_match_atss(const float* annot, const float* anchors, const int32_t* level_off, int32_t L, int32_t B, int32_t A, int32_t topk,
                   uint8_t* pos_mask, double* thr, int32_t* cand, void* ws, size_t ws_bytes, void* stream);
/* Task-aligned anchor assignment (TOOD's Task-Aligned Assigner, Feng et al. 2021) — ZSGLoss.forward with cfg matcher = "tal"; the mask
 * goes to zsg_loss_fwd_bwd_m.  Unlike the fixed rule and ATSS it reads what the network predicts.  Per sample b: one annotation
 * g = annot[b] (y1x1y2x2), the anchors a in create_anchors' flattened order, the network output out5[b][a] = (dy, dx, dh, dw, att).
 *   s(a) = the fp32 sigmoid of att, 1 / (1 + expf(-att)): the score zsg_loss_fwd_bwd_q's quality term trains
 *   p(a) = the decoded box (reg_params_to_bbox, anchors.py:182-197; the fp64 expressions of zsg_loss_fwd_bwd_iou)
 *   u(a) = inter / (union + 1e-7) of p(a) with g, rounded to fp32: exactly the q of zsg_loss_fwd_bwd_q, here for EVERY anchor
 *   inside(a) = g.y1 < acy < g.y2 and g.x1 < acx < g.x2, acy = (a.y1 + a.y2) / 2, acx likewise in fp32 (zsg_match_atss's centres)
 *   t(a) = pow((double)s, alpha) * pow((double)u, beta) in fp64; NaN where any of the five values of the row is NaN or u(a) is NaN
 *          (a decode that overflows to inf - inf; min / max inside u are C's fmin / fmax, as in zsg_loss_fwd_bwd_q)
 *   a is a candidate iff inside(a) and t(a) > 0 (false for NaN: an anchor with a NaN in its row or in u is never a candidate)
 *   selected: the min(topk, #candidates) candidates that come first when ordered by t descending, then by index ascending
 * pos_mask [B][A] uint8: 1 at the selected anchors, else 0; every byte is written.  zsg_loss_fwd_bwd_m adds the sample's arg-max IoU
 * anchor as for every mask, so every sample keeps a positive.  The mask is a constant of the backward: no gradient flows through the
 * selection.  metric [B][A] double (may be null): t(a) where inside(a) (a NaN t stays NaN), -1.0 elsewhere; the selection can be redone
 * from this array alone (candidates are its entries > 0).  ws: zsg_match_tal_workspace_bytes(B, A) bytes; it holds the fp64 keys when
 * metric is null.  With metric given the keys are the metric, ws is neither read nor written and may be the same buffer as metric.
 * Two launches, no atomics, no host synchronisation, the same bits on every run.
 * Limits (else -1, nothing launched or written, zsg_last_error names the argument): 1 <= topk <= 32, B <= 512, alpha >= 0 and
 * beta >= 0 and both finite, ws_bytes large enough, every pointer but metric non-null. */
size_t zsg_match_tal_workspace_bytes(int32_t B, int32_t A);
int zsg_match_tal(const float* out5, const float* annot, const float* anchors, int32_t B, int32_t A, int32_t topk, float alpha,
                  float beta, uint8_t* pos_mask, double* metric /* may be NULL */, void* ws, size_t ws_bytes, void* stream);

/* Evaluator.forward, evaluator.py:48-117 (reg_params_to_bbox anchors.py:182-197): arg-max score anchor -> decode ->
 * IoU >= thr.  metrics[2] = (Acc, MaxPos); pred_boxes [B][4] pixels x1y1x2y2; pred_scores [B]; pred_idx [B] int32. */
size_t zsg_eval_workspace_bytes(int32_t B);
int zsg_eval(const float* out5, const float* annot, const float* anchors, const float* img_size, int32_t B, int32_t A,
             float acc_thr, float* metrics, float* pred_boxes, float* pred_scores, int32_t* pred_idx, int32_t* best_idx,
             float* ws /* zsg_eval_workspace_bytes(B): per-sample, per-anchor-range arg-max records */, void* stream);
/* Top-k grounding per query (no counterpart in the reference, whose evaluator keeps one box: evaluator.py:74-75 ranks by the sigmoid
 * score, anchors.py:182-197 decodes, anchors.py:106-116 is the IoU; the pieces are the reference's, the NMS is this build's).
 * Candidates are ordered by (score descending, anchor index ascending), a NaN score below every number; the first min(pre_n, A) are
 * decoded; greedy NMS in that order keeps a candidate unless IoU(kept, candidate) > nms_thr for a box already kept, up to K boxes.
 * topk_boxes [B][K][4] pixels x1y1x2y2, topk_scores [B][K], topk_idx [B][K] int32 anchor index, topk_n [B] int32 boxes kept; rows past
 * topk_n are boxes 0, score 0, index -1.  Row 0 is bit-identical to zsg_eval's pred_boxes / pred_scores / pred_idx.
 * With annot: hit_rank [B] int32 = first rank r with IoU(box_r, annot) >= acc_thr (evaluator.py:115-117), K when none;
 * acc_at [K] = mean over the batch of (hit_rank <= j).  annot, hit_rank and acc_at may be NULL (acc_at needs hit_rank, hit_rank
 * needs annot).  Limits: 1 <= K <= 64, K <= pre_n <= 512.  ws: zsg_eval_topk_workspace_bytes(B, A, pre_n, K) bytes, 8-byte aligned. */
size_t zsg_eval_topk_workspace_bytes(int32_t B, int32_t A, int32_t pre_n, int32_t K);
int zsg_eval_topk(const float* out5, const float* annot, const float* anchors, const float* img_size, int32_t B, int32_t A,
                  int32_t pre_n, int32_t K, float nms_thr, float acc_thr, float* topk_boxes, float* topk_scores,
                  int32_t* topk_idx, int32_t* topk_n, int32_t* hit_rank, float* acc_at, void* ws, void* stream);
/* Score-weighted box voting over the NMS candidates (csrc/vote.hip; Evaluator with cfg eval_box_vote > 0; no counterpart in the
 * reference; the host definition is tests/vote_ref.py).  Called after zsg_eval_topk on the SAME out5 / anchors / img_size / pre_n / K,
 * with the topk_boxes / topk_scores / topk_idx / topk_n it produced; none of the four is written (topk_scores is not read either: the
 * scores are the ranking's).  Scores, indices, count and row order of the kept rows stay: no re-sort, no second NMS.
 * Candidates: exactly zsg_eval_topk's — the first min(pre_n, A) anchors ordered by (score descending, anchor index ascending), a NaN
 * score below every number — decoded as there (y1x1y2x2 in [-1, 1], then pixels x1y1x2y2).  A candidate is VALID when its score is not
 * NaN and its eight decoded coordinates (both forms) are finite.
 * Members of the kept row r < topk_n[b], whose own candidate is the one of anchor topk_idx[b][r]: if that candidate is valid, itself and
 * every other valid candidate c with IoU(box_r, box_c) >= vote_thr (the NMS's IoU: kept box first, the [-1, 1] coordinates, fp32 in
 * loss.hip's operation order); if it is not valid (or topk_idx[b][r] is no candidate), nobody.
 * voted[r][j] = (float)(sum_{c in M_r, in candidate order} (double)s_c (double)box_c[j] / sum (double)s_c), box_c in pixels, s_c the
 * fp32 sigmoid score the ranking uses; with no member or a weight sum of 0 the row keeps topk_boxes[b][r].
 * vote_boxes [B][K][4] pixels x1y1x2y2, rows past topk_n zero; vote_n [B][K] int32 member counts, 0 past topk_n.
 * With annot: hit_rank [B] int32 = first row r whose voted box has IoU >= acc_thr with annot (zsg_eval_topk's rule, in its [-1, 1]
 * coordinates: the voted box there is the same weighted mean of the candidates' y1x1y2x2 coordinates, the row's own decoded box where
 * the row kept its box), K when none; acc_at [K] = mean over the batch of (hit_rank <= j).  annot, hit_rank and acc_at may be NULL
 * (acc_at needs hit_rank, hit_rank needs annot).
 * Three launches, one thread per kept row summing in candidate order: no atomics, no host synchronisation, the same bits on every run.
 * Limits (else -1, nothing launched or written, zsg_last_error names the argument): zsg_eval_topk's 1 <= K <= 64, K <= pre_n <= 512,
 * B <= 65535; 0 < vote_thr <= 1; ws 8-byte aligned with ws_bytes >= zsg_eval_vote_workspace_bytes(B, A, pre_n, K). */
size_t zsg_eval_vote_workspace_bytes(int32_t B, int32_t A, int32_t pre_n, int32_t K);
int zsg_eval_vote(const float* out5, const float* annot, const float* anchors, const float* img_size, int32_t B, int32_t A,
                  int32_t pre_n, int32_t K, float vote_thr, float acc_thr, const float* topk_boxes, const float* topk_scores,
                  const int32_t* topk_idx, const int32_t* topk_n, float* vote_boxes, int32_t* vote_n, int32_t* hit_rank, float* acc_at,
                  void* ws, size_t ws_bytes, void* stream);
/* Soft-NMS selection of the K boxes per query (csrc/softnms.hip; Evaluator with cfg eval_nms = "soft_linear" / "soft_gauss"; Bodla et
 * al., ICCV 2017; no counterpart in the reference; the host definition is tests/softnms_ref.py).  zsg_eval_topk with another selection
 * rule: a picked box lowers the weights of its neighbours instead of deleting them, and selection goes on over the decayed weights.
 * Candidates: exactly zsg_eval_topk's — the first nc = min(pre_n, A) anchors ordered by (fp32 sigmoid score descending, anchor index
 * ascending), a NaN score below every number — decoded as there (y1x1y2x2 in [-1, 1], then pixels x1y1x2y2).  Candidate position c is
 * its rank.
 * Weights: fp64, w_c = (double)s_c at the start.  A candidate with a NaN score is never eligible after row 0.
 * Row 0: unconditionally candidate 0, as under hard NMS: row 0 is bit-identical to zsg_eval_topk's row 0 and so to zsg_eval's
 * pred_boxes / pred_scores / pred_idx (a query whose scores are all NaN: box and index of anchor 0 as there, the score NaN as in
 * zsg_eval_topk).
 * Rows r = 1 .. K-1: among the candidates not yet picked whose score is not NaN, the one with the largest w_c, ties to the smaller
 * position; the rows end when there is none, or when that weight is < (double)min_score.
 * Decay after picking m: for every unpicked candidate c, u = IoU(box_m, box_c) (the NMS's IoU: kept box first, the [-1, 1] coordinates,
 * fp32 in loss.hip's operation order); method 1 (linear): if u > nms_thr (fp32 compare), w_c *= 1.0 - (double)u;  method 2 (gauss):
 * if u == u, w_c *= exp(-((double)u * (double)u) / (double)sigma) with the fp64 exp (nms_thr is not read).  A NaN u never decays.
 * Outputs: zsg_eval_topk's arrays — topk_boxes [B][K][4] pixels x1y1x2y2, topk_scores [B][K] = (float)w at pick time (row 0: the
 * score itself), topk_idx [B][K] int32, topk_n [B] int32; rows past topk_n are boxes 0, score 0, index -1.  With annot: hit_rank [B] =
 * first row r with IoU(box_r, annot) >= acc_thr, K when none; acc_at [K] = mean over the batch of (hit_rank <= j).  annot, hit_rank and
 * acc_at may be NULL (acc_at needs hit_rank, hit_rank needs annot).
 * Three launches (range sort, one 256-thread finishing block per query, the Acc@ mean): no atomics, no host synchronisation, the same
 * bits on every run.
 * Limits (else -1, nothing launched or written, zsg_last_error names the argument): 1 <= K <= 64, K <= pre_n <= 512, B <= 65535;
 * method 1 or 2; 0 <= nms_thr <= 1; sigma > 0 and finite; 0 <= min_score < 1; ws 8-byte aligned with
 * ws_bytes >= zsg_eval_topk_soft_workspace_bytes(B, A, pre_n, K). */
size_t zsg_eval_topk_soft_workspace_bytes(int32_t B, int32_t A, int32_t pre_n, int32_t K);
int zsg_eval_topk_soft(const float* out5, const float* annot, const float* anchors, const float* img_size, int32_t B, int32_t A,
                       int32_t pre_n, int32_t K, float nms_thr, float acc_thr, int32_t method, float sigma, float min_score,
                       float* topk_boxes, float* topk_scores, int32_t* topk_idx, int32_t* topk_n, int32_t* hit_rank, float* acc_at,
                       void* ws, size_t ws_bytes, void* stream);
/* IoU table [B][A] (tests / diagnostics) */
int zsg_iou(const float* boxes, const float* anchors, int32_t B, int32_t A, float* iou, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Fused Adam over a flat parameter buffer — torch.optim.Adam(betas=(0.9,0.99)) at main_dist.py:50 / utils.py:413.
 * step_count: device int32[2], zero-initialised by the caller: [0] = steps taken, incremented by the kernel (graph-capturable);
 * [1] = the kernel's completion ticket (0 between launches).  grad_scale folds 1/world_size.
 * ------------------------------------------------------------------------------------------------------------- */
int zsg_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, float grad_scale, int32_t* step_count, void* stream);
/* The same step as several launches over disjoint ranges (pointers offset by the caller, 16-byte aligned): every launch computes with
 * t = counter + 1; exactly the last one passes publish = 1 — and it must be ordered behind the others (same stream, or an event
 * edge): it advances the counter they read.  Lets the update of the parameters whose gradients are complete overlap the tail of
 * the backward (the stem's weight gradient). */
int zsg_adam_step_range(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                        float weight_decay, float grad_scale, int32_t* step_count, int32_t publish, void* stream);

/* Adam over listed segments of the flat buffer (fine-tuning: frozen parameters are not listed; parameter groups).  segs: a DEVICE
 * table of nseg segments in increasing chunk0 order, one per stepped parameter; the kernel reads and writes p, m, v inside the
 * listed ranges only.  Every segment is cut into work chunks of at most ZSG_ADAM_CHUNK elements (a chunk never straddles two
 * segments); chunk0 = the sum of ceil(len / ZSG_ADAM_CHUNK) over the segments before it, nchunks = that sum over all of them.
 * groups: a HOST table of ngroups <= ZSG_ADAM_MAX_GROUPS hyperparameter sets, passed to the kernel by value (an lr change costs
 * no copy).  counters: device int32, one per segment (distinct indices) = the steps its parameter has taken (torch's
 * state['step']); a segment computes with t = counters[counter] + 1 and the block that finishes last advances every listed
 * counter.  ticket: a device int32, 0 between launches, owned by the caller's optimizer.  A one-segment, one-group launch is
 * bit-identical to zsg_adam_step over the same range. */
#define ZSG_ADAM_MAX_GROUPS 8
#define ZSG_ADAM_CHUNK 16384
typedef struct zsg_adam_seg {
    int64_t off;          /* first element (a multiple of 4: 16-byte aligned) */
    int64_t len;          /* elements (any count; the parameter store pads to multiples of 4) */
    int32_t group;        /* index into groups[] */
    int32_t counter;      /* index into counters[] */
    int32_t chunk0;       /* index of the segment's first work chunk */
    int32_t reserved;
} zsg_adam_seg;
typedef struct zsg_adam_group {
    float lr, beta1, beta2, eps, weight_decay;
} zsg_adam_group;
int zsg_adam_step_segments(float* p, const float* g, float* m, float* v, const zsg_adam_seg* segs, int32_t nseg, int32_t nchunks,
                           const zsg_adam_group* groups, int32_t ngroups, float grad_scale, int32_t* counters, int32_t* ticket,
                           void* stream);

/* Gradient-norm clipping over listed segments of the flat gradient buffer: torch.nn.utils.clip_grad_norm_ (torch/nn/utils/clip_grad.py)
 * in two launches with no host round trip.  segs / nseg / nchunks: a DEVICE segment table as zsg_adam_step_segments takes it (group and
 * counter are not read); nothing outside the listed ranges is read or written.  nseg == 0: no launch, nothing written.
 * zsg_grad_norm replaces _get_total_norm (torch._foreach_norm + linalg.vector_norm) and the coefficient of _clip_grads_with_norm_: the
 * total 2-norm (inf_norm = 0: sums of squares in fp64) or inf-norm (inf_norm = 1: max |g|, NaN propagates) of the listed ranges, and
 * clip_coef = clamp(max_norm / (total_norm + 1e-6), max=1.0) computed as torch does (fp32, reciprocal times max_norm, NaN kept);
 * out[0] = total_norm, out[1] = clip_coef (fp32, device).  partials: device fp64 scratch of nchunks; ticket: a device int32, 0 between
 * launches.  The last block reduces the partials in a fixed order: the same bits from run to run, whatever ZSG_DETERMINISTIC says. */
int zsg_grad_norm(const float* g, const zsg_adam_seg* segs, int32_t nseg, int32_t nchunks, int32_t inf_norm, float max_norm,
                  double* partials, int32_t* ticket, float* out, void* stream);
/* g *= *coef over the listed ranges (torch._foreach_mul_ of _clip_grads_with_norm_): coef is read on the device (zsg_grad_norm's out + 1);
 * a coefficient of exactly 1.0f leaves the buffer untouched (g * 1.0f == g). */
int zsg_grad_scale(float* g, const zsg_adam_seg* segs, int32_t nseg, int32_t nchunks, const float* coef, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Weight EMA: an exponential moving average of flat fp32 buffers — torch.optim.swa_utils.AveragedModel with
 * multi_avg_fn=get_ema_multi_avg_fn(decay), use_buffers=True (torch._foreach_lerp_(ema, p, 1 - decay)).  The rule, for every element
 * and the same in every kernel below:
 *     ema <- fmaf(w, p - ema, ema),   w = 1 - decay in fp32          (one subtraction, one fused multiply-add)
 * w == 1.0f stores p exactly (a copy, as torch.lerp returns `end` at weight 1); w == 0.0f leaves a finite ema unchanged; NaN and inf in p
 * propagate.  w is passed by value: the caller keeps the update count on the host, nothing is read back.
 * ------------------------------------------------------------------------------------------------------------- */
/* One launch over one or two ranges (the flat parameter buffer and the BatchNorm statistics buffer); ema_b = b = NULL and nb = 0 for
 * one.  Any lengths > 0 (16-byte accesses plus a tail), every pointer 16-byte aligned, ema_x and x disjoint.  w outside [0, 1] (NaN
 * included), a NULL required pointer or a misaligned buffer returns -1 before anything is launched.  12 B per element of HBM traffic. */
int zsg_ema_update(float* ema_a, const float* a, int64_t na, float* ema_b, const float* b, int64_t nb, float w, void* stream);
/* zsg_adam_step with the average updated in the same launch (the same kernel body): the rule is applied to the freshly updated p before
 * it is stored.  p, m, v and step_count come out bit-identical to zsg_adam_step, ema bit-identical to zsg_ema_update on the post-step p.
 * 36 B per parameter, against 28 + 12 for the step followed by a separate update.  All buffers 16-byte aligned; ema_w as w above. */
int zsg_adam_step_ema(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                      float weight_decay, float grad_scale, int32_t* step_count, float* ema, float ema_w, void* stream);
/* Exchanges the contents of two disjoint buffers of n > 0 floats in one pass (16 B per element); overlapping ranges return -1. */
int zsg_swap_f32(float* a, float* b, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Fused optimizer steps with a choice of rule (csrc/optim.hip), in the three launch shapes of the Adam block above.  Each rule follows
 * torch's single-tensor implementation and replaces one optimizer.step() of
 *     ZSG_OPT_ADAM   torch.optim.Adam(lr, betas, eps, weight_decay, amsgrad)      coupled decay g += wd * p
 *     ZSG_OPT_ADAMW  torch.optim.AdamW(lr, betas, eps, weight_decay, amsgrad)     decoupled decay p *= 1 - lr * wd, then Adam on the raw g
 *     ZSG_OPT_SGD    torch.optim.SGD(lr, momentum, dampening, weight_decay, nesterov)
 *                    g += wd * p;  buf = g on the parameter's FIRST step, else momentum * buf + (1 - dampening) * g;
 *                    p -= lr * (nesterov ? g + momentum * buf : buf);  momentum == 0: p -= lr * g, no buffer
 * over one flat buffer instead of one update per parameter tensor.  flags: ZSG_OPT_AMSGRAD (Adam / AdamW only) keeps
 * vmax = max(vmax, v) and divides by sqrt(vmax) / sqrt(bc2) + eps.  One call uses one rule; groups differ in hyperparameters only.
 *
 * Buffers (fp32, n elements each, 16-byte aligned, zero-initialised by the caller before the first step, disjoint):
 *     Adam / AdamW   s0 = m (exp_avg), s1 = v (exp_avg_sq), s2 = vmax (max_exp_avg_sq) with ZSG_OPT_AMSGRAD, else not read (NULL is legal)
 *     SGD            s0 = the momentum buffer when some group has momentum != 0, else not read (NULL is legal); s1, s2 not read
 * A parameter's first step is decided on the device from the counter the kernel reads (t == 1; the per-segment counter on the segmented
 * path): a parameter that joins later starts its momentum buffer from its first gradient, whatever the buffer holds.
 * HBM traffic per parameter: Adam / AdamW 28 B, with amsgrad 36 B, SGD with momentum 20 B, plain SGD 12 B; + 8 B with the average riding.
 * Rule ZSG_OPT_ADAM without flags gives the bits of zsg_adam_step / _ema / _segments; AdamW with weight_decay == 0 gives Adam's bits.
 * A NULL required pointer, a misaligned buffer, ngroups outside 1..ZSG_ADAM_MAX_GROUPS, ema_w outside [0, 1], nesterov without
 * momentum or with dampening, an unknown algo or flag: -1 before anything is launched (zsg_last_error names the argument).
 * ------------------------------------------------------------------------------------------------------------- */
#define ZSG_OPT_ADAM 0
#define ZSG_OPT_ADAMW 1
#define ZSG_OPT_SGD 2
#define ZSG_OPT_AMSGRAD 1          /* flags */
typedef struct zsg_optim_group {
    float lr, beta1, beta2, eps, weight_decay;          /* (the fields of zsg_adam_group; beta1, beta2, eps unused by SGD) */
    float momentum, dampening;                          /* SGD */
    int32_t nesterov;                                   /* SGD: 0 / 1 */
} zsg_optim_group;
/* One launch over p[0:n] (16-byte accesses plus a tail of n % 4).  hp: ONE hyperparameter set on the host, passed to the kernel by value.
 * step_count: device int32[2] as zsg_adam_step's ([0] = steps taken, [1] = the completion ticket): no host round trip, capturable. */
int zsg_optim_step(int32_t algo, int32_t flags, float* p, const float* g, float* s0, float* s1, float* s2, int64_t n,
                   const zsg_optim_group* hp, float grad_scale, int32_t* step_count, void* stream);
/* The same launch with the weight average riding: ema <- the rule of "Weight EMA" on the p this step stores.  p, the state and step_count
 * come out bit-identical to zsg_optim_step, ema bit-identical to zsg_ema_update on the post-step p. */
int zsg_optim_step_ema(int32_t algo, int32_t flags, float* p, const float* g, float* s0, float* s1, float* s2, int64_t n,
                       const zsg_optim_group* hp, float grad_scale, int32_t* step_count, float* ema, float ema_w, void* stream);
/* The step over listed segments: segs / nseg / nchunks, counters and ticket exactly as zsg_adam_step_segments takes them (the same DEVICE
 * table, which zsg_grad_norm / zsg_grad_scale read too); groups: a HOST table of ngroups sets, passed by value.  Nothing outside the
 * listed ranges is read or written, in p or in any state buffer.  One segment in one group gives the bits of zsg_optim_step. */
int zsg_optim_step_segments(int32_t algo, int32_t flags, float* p, const float* g, float* s0, float* s1, float* s2,
                            const zsg_adam_seg* segs, int32_t nseg, int32_t nchunks, const zsg_optim_group* groups, int32_t ngroups,
                            float grad_scale, int32_t* counters, int32_t* ticket, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Fused LAMB (You et al., "Large Batch Optimization for Deep Learning"; csrc/lamb.hip): Adam's moments, and every parameter tensor's
 * update rescaled by its trust ratio.  For every listed segment (one parameter tensor w with gradient g * grad_scale, moments m, v, its
 * group's lr, beta1, beta2, eps, weight_decay = wd and flag adapt, t = counters[counter] + 1):
 *     m <- beta1 * m + (1 - beta1) * g          v <- beta2 * v + (1 - beta2) * g * g
 *     u  = (m / bc1) / (sqrt(v / bc2) + eps) + wd * w          fp32, element-wise, every operation rounded on its own;
 *                                                              bc = 1 - beta^t formed in fp64 and rounded once to fp32
 *     Nw = sqrt(sum w^2)   Nu = sqrt(sum u^2)                  sums in fp64 over the segment, each result rounded to fp32
 *     r  = Nw / Nu  if adapt and Nw > 0 and Nu > 0,  else 1    (adapt and a NaN in either norm: r = NaN — it propagates, in that segment only)
 *     w <- w - (lr * r) * u
 * No clamp on Nw, no global gradient pre-normalisation (zsg_grad_norm / zsg_grad_scale in front cover that).  Elements with w = g = 0 and
 * zero moments (the parameter store's padding) have u = 0: they change neither norm and stay 0.
 *
 * Two launches over a DEVICE segment table exactly as zsg_adam_step_segments takes it (segs / nseg / nchunks; one 256-thread block per
 * work chunk; 16-byte accesses plus a tail); nothing outside the listed ranges is read or written in p, m or v.  groups: a HOST table of
 * ngroups <= ZSG_ADAM_MAX_GROUPS sets, passed by value; the same table to both launches.  counters / ticket as zsg_adam_step_segments:
 * both launches compute with t = counters[counter] + 1, zsg_lamb_apply's last block advances every listed counter; ticket is 0 between
 * launches and serves both.  HBM traffic 24 + 16 B per parameter (u is formed twice, from the same stored m, v with the same code: the
 * same bits, never stored).
 * zsg_lamb_moments: partials = device fp64 scratch of 2 * nchunks; ratio / norm_w / norm_u = device fp32 of nseg each, indexed by the
 * segment's position in the table (r, Nw, Nu).  The block that arrives last reduces the chunks' sums per segment in an order fixed by the
 * chunk index (zsg_grad_norm's hand-off): no float atomics, the same bits from run to run, whatever ZSG_DETERMINISTIC says.
 * zsg_lamb_apply: ratio as zsg_lamb_moments wrote it, on the same stream behind it.
 * A NULL required pointer (every pointer but stream is required), a misaligned buffer (p, g, m, v: 16 bytes; partials: 8), ngroups outside
 * 1..ZSG_ADAM_MAX_GROUPS, nseg < 0 or nchunks < nseg: -1 before anything is launched (zsg_last_error names the argument).  nseg == 0: 0,
 * no launch, nothing written, no counter moves.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct zsg_lamb_group {
    float lr, beta1, beta2, eps, weight_decay;
    int32_t adapt;          /* 0: r = 1 for the group's segments (biases, normalisation scales), their norms are still reported */
} zsg_lamb_group;
int zsg_lamb_moments(const float* p, const float* g, float* m, float* v, const zsg_adam_seg* segs, int32_t nseg, int32_t nchunks,
                     const zsg_lamb_group* groups, int32_t ngroups, float grad_scale, const int32_t* counters, double* partials,
                     int32_t* ticket, float* ratio, float* norm_w, float* norm_u, void* stream);
int zsg_lamb_apply(float* p, const float* m, const float* v, const zsg_adam_seg* segs, int32_t nseg, int32_t nchunks,
                   const zsg_lamb_group* groups, int32_t ngroups, const float* ratio, int32_t* counters, int32_t* ticket, void* stream);

int zsg_memset_f32(float* p, int64_t n, float value, void* stream);

/* Wave priority of the kernels of the step's dependent chain (convolutions forward / data gradient, BatchNorm passes, the small
 * main-stream kernels): 3 (default) = they issue ahead of the weight-gradient kernels wherever a CU holds waves of both streams
 * (s_setprio 3 as their first instruction), 0 = off.  A run-time switch since round 6 (a build-time constant before) so that a multi-GPU
 * run can compare both beside RCCL's priority-0 kernels.  Applies to the CURRENT device, synchronises it; call between steps.  No
 * reference counterpart (PyTorch / cuDNN kernels carry no priorities; the reference's overlap is NCCL's own, main_dist.py:36-40). */
int zsg_set_main_priority(int32_t prio);
int zsg_get_main_priority(void);

/* Scratch for the launches of one stream (round 6).  The reference has no counterpart: cuDNN / cuBLAS take their split-K workspace from
 * PyTorch's caching allocator behind nn.Conv2d (mdl.py:149-156, fpn_resnet.py:86-100).  Here the caller owns it: `ws` (256-byte aligned,
 * more than 16 KB; device memory of the current device) serves every later libzsg launch on `stream` that needs scratch — today the
 * stream-K implicit GEMM (tile_hint bits 28-29: one partial accumulator tile per workgroup + hand-off flags).  Launches of one stream are
 * ordered, so they share the buffer; two streams that run such launches concurrently register one buffer each.  The call clears the
 * first 16 KB (the flags) on `stream`; launches leave them zero.  ws = NULL unregisters.  A launch that needs scratch on a stream
 * without a registered buffer fails with -1, with a buffer that is too small with -2. */
int zsg_set_stream_workspace(void* stream, void* ws, size_t bytes);

/* ---------------------------------------------------------------------------------------------------------------
 * Cross-stream ordering without marker packets (SURVEY 8b "Threading / streams": asynchronous launches on the passed stream, a
 * dedicated side stream + hipEvents; the reference gets its concurrency from PyTorch's autograd / DDP reducer streams,
 * main_dist.py:37-40, utils.py:407-414).  The weight gradients of the backward (and some leaves of the forward) run on a side
 * stream; releasing them used to cost the main stream one hipEventRecord (a marker packet: ~4.3 us of main-stream time each, ~35
 * per step).  Instead the caller arms an event for its thread, makes ONE libzsg call — every kernel that call launches carries the
 * event as its dispatch packet's completion signal, the last launch wins — disarms it (NULL) and lets the other stream wait:
 *     zsg_set_completion_event(ev); zsg_conv_igemm(..., main); zsg_set_completion_event(NULL); zsg_stream_wait_event(side, ev);
 * Events are plain hipEvent_t (timing disabled) owned by the caller between create and destroy; zsg_event_record is the marker
 * fallback for a release point that no libzsg launch precedes, or when the armed call launched nothing (zsg_set_completion_event
 * returned 0 on disarming).  Thread-local arming: re-entrant across threads. */
void* zsg_event_create(void);
int zsg_event_destroy(void* ev);
int zsg_set_completion_event(void* ev);     /* returns how many launches carried the event armed before this call (0: none did) */
int zsg_event_record(void* ev, void* stream);
int zsg_stream_wait_event(void* stream, void* ev);

/* ---------------------------------------------------------------------------------------------------------------
 * Gradient exchange over RCCL (xGMI) — the NCCL collectives torch DistributedDataParallel issues for the reference
 * (main_dist.py:36-40, utils.py:395-414): C1 bucketed gradient all-reduce during backward, C2 BatchNorm-buffer
 * broadcast per training forward, C3 parameter broadcast at wrap time.  One process per GPU, one communicator per
 * process; the collectives run on the communicator's own non-blocking HIP stream, fenced against the caller's compute
 * stream with events (no host synchronisation).  librccl is bound with dlopen on first use (the copy PyTorch loaded).
 *   rank 0: zsg_comm_unique_id(id) -> share the 128 bytes with every rank (TCPStore / torch.distributed) ->
 *   every rank, on its own device: zsg_comm_init(&c, id, nranks, rank).
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct zsg_comm zsg_comm;
int zsg_comm_unique_id(void* id128 /* out: 128 bytes */);
int zsg_comm_init(zsg_comm** out, const void* id128, int32_t nranks, int32_t rank);
/* in-place SUM all-reduce of buf[0:count], ordered after everything already enqueued on compute_stream; returns at once */
int zsg_comm_allreduce_bucket(zsg_comm* c, float* buf, int64_t count, void* compute_stream);
/* buf[0:count] of `root` to all ranks; compute_stream waits for it on the device */
int zsg_comm_broadcast(zsg_comm* c, float* buf, int64_t count, int32_t root, void* compute_stream);
/* compute_stream waits (device-side) for every bucket enqueued so far — call before the optimizer step */
int zsg_comm_wait(zsg_comm* c, void* compute_stream);
int zsg_comm_destroy(zsg_comm* c);

/* ---------------------------------------------------------------------------------------------------------------
 * Per-launch timing (HIP events on the launch stream) used by bench.py's roofline leg.  Not used in timed steps.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
    char name[48];
    int64_t launches;
    double ms;        /* summed kernel time between the bracketing events */
    double flops;     /* algorithmic 2*MAC for conv kernels, else 0       */
    double bytes;     /* algorithmic bytes moved (HBM-bound kernels)      */
} zsg_prof_entry;
int zsg_prof_enable(int32_t on);
int zsg_prof_collect(zsg_prof_entry* out, int32_t max_entries); /* syncs the recorded events; returns #entries */

#ifdef __cplusplus
}
#endif
#endif /* ZSG_H */
