// aug.hip — training augmentation on the GPU: box-safe crop + resize + colour jitter of a whole batch (uint8 HWC, 3 channels).
// Built with -ffp-contract=off (Makefile): every fp32 product and sum below is rounded separately, as dat_loader.augment_host
// (the byte-exact host definition) does it, so the bytes are equal.
//
// Step 1 is Pillow's `img.crop(box).resize((Wo, Ho))` (the reference's only resampling call is dat_loader.py:121): the two-pass
// fixed-point bicubic of resize_batched_kernel (misc.hip), with tap tables built for the WINDOW's side lengths and the window
// addressed inside the full image through a row pitch — no copy of the crop.  Steps 2-4: brightness, contrast, saturation
// (blend(x, m, f) = trunc(clamp(f * x + (1 - f) * m, 0, 255)); gray = trunc((0.2989 r + 0.587 g) + 0.114 b)).
//
// Thread mapping: one thread per output PIXEL, 256 pixels per block.  A block's 768 bytes are contiguous in its job's image, so
// they go through LDS and leave (launch 3: also arrive) as 192 coalesced dword accesses instead of 768 single bytes; a job whose
// base address is not dword aligned, and the last few bytes of an image, take byte accesses.
#include "common.h"

struct ZsgAugJob {
    int64_t src, tmp, out;                 // absolute device addresses: the window's first pixel, scratch [h][Wo][3], result [Ho][Wo][3]
    int64_t xb, xc, yb, yc;                // tap tables (int32) for the window's sides: bounds [n_out][2], coefficients [n_out][ksize]
    int32_t h, w, pitch, xk, yk;           // window height / width, row pitch of the source IMAGE in pixels, tap-table widths
    int32_t blk0_x, blk0_y, pad0;          // first block of the job in launch 1 / launches 2 and 3 (256 pixels per block)
    float fb, fc, fs;                      // brightness, contrast, saturation factors (1 = identity)
    int32_t pad1;
};
static_assert(sizeof(ZsgAugJob) == 104, "ZsgAugJob is packed by dat_loader.GpuResizer");

#define AUG_PIX 256

template <int AXIS>
__device__ __forceinline__ int aug_find_job(const ZsgAugJob* __restrict__ jobs, int njobs) {
    int lo = 0, hi = njobs - 1;                      // last job whose first block <= blockIdx.x
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((AXIS == 0 ? jobs[mid].blk0_x : jobs[mid].blk0_y) <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the block's bytes [0, nbytes) at `base`: LDS -> global, dwords where the address allows it
__device__ __forceinline__ void aug_store_block(uint8_t* __restrict__ base, const uint32_t* stage, int nbytes) {
    const int t = (int)threadIdx.x;
    if ((((uintptr_t)base) & 3) == 0) {
        if (t < AUG_PIX * 3 / 4 && 4 * t + 4 <= nbytes) ((uint32_t*)base)[t] = stage[t];
        const int tail = nbytes & ~3;
        if (t < (nbytes & 3)) base[tail + t] = ((const uint8_t*)stage)[tail + t];
    } else {
        for (int i = t; i < nbytes; i += AUG_PIX) base[i] = ((const uint8_t*)stage)[i];
    }
}
__device__ __forceinline__ void aug_load_block(const uint8_t* __restrict__ base, uint32_t* stage, int nbytes) {
    const int t = (int)threadIdx.x;
    if ((((uintptr_t)base) & 3) == 0) {
        if (t < AUG_PIX * 3 / 4 && 4 * t + 4 <= nbytes) stage[t] = ((const uint32_t*)base)[t];
        const int tail = nbytes & ~3;
        if (t < (nbytes & 3)) ((uint8_t*)stage)[tail + t] = base[tail + t];
    } else {
        for (int i = t; i < nbytes; i += AUG_PIX) ((uint8_t*)stage)[i] = base[i];
    }
}

__device__ __forceinline__ int aug_clip8(int acc) {
    acc >>= 22;                                      // (arithmetic shift, as Pillow's clip8 lookup index)
    return acc < 0 ? 0 : (acc > 255 ? 255 : acc);
}
__device__ __forceinline__ float aug_blend(float x, float m, float f) {
    const float a = f * x;
    const float b = (1.0f - f) * m;
    float v = a + b;
    v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
    return (float)(int)v;                            // truncation to uint8, kept as a float for the next step
}
__device__ __forceinline__ int aug_gray(float r, float g, float b) {
    const float rg = 0.2989f * r + 0.587f * g;       // (-ffp-contract=off: two products, one sum)
    return (int)(rg + 0.114f * b);
}

// launch 1: horizontal pass of every job over its window -> tmp [h][Wo][3]; zeroes the job's gray accumulator
__global__ __launch_bounds__(AUG_PIX) void aug_hpass_kernel(const ZsgAugJob* __restrict__ jobs, int njobs, int Wo, uint32_t* __restrict__ gray_sums) {
    __shared__ uint32_t stage[AUG_PIX * 3 / 4];
    const int j = aug_find_job<0>(jobs, njobs);
    const ZsgAugJob jb = jobs[j];
    const int lb = (int)blockIdx.x - jb.blk0_x;
    if (lb == 0 && threadIdx.x == 0) gray_sums[j] = 0u;
    const int total = jb.h * Wo;
    const int i = lb * AUG_PIX + (int)threadIdx.x;
    if (i < total) {
        const int x = i % Wo, y = i / Wo;
        const int32_t* bounds = (const int32_t*)jb.xb;
        const int first = bounds[2 * x], n = bounds[2 * x + 1];
        const int32_t* k = (const int32_t*)jb.xc + (int64_t)x * jb.xk;
        const uint8_t* p = (const uint8_t*)jb.src + ((int64_t)y * jb.pitch + first) * 3;
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
        for (int t = 0; t < n; ++t) {
            const int kt = k[t];
            a0 += (int)p[3 * t] * kt;
            a1 += (int)p[3 * t + 1] * kt;
            a2 += (int)p[3 * t + 2] * kt;
        }
        uint8_t* s = (uint8_t*)stage + 3 * (int)threadIdx.x;
        s[0] = (uint8_t)aug_clip8(a0);
        s[1] = (uint8_t)aug_clip8(a1);
        s[2] = (uint8_t)aug_clip8(a2);
    }
    __syncthreads();
    const int nb = min(AUG_PIX, total - lb * AUG_PIX) * 3;
    aug_store_block((uint8_t*)jb.tmp + (int64_t)lb * AUG_PIX * 3, stage, nb);
}

// launch 2: vertical pass, brightness, store, gray value of the pixel added to the job's integer accumulator (one atomic per block)
__global__ __launch_bounds__(AUG_PIX) void aug_vpass_kernel(const ZsgAugJob* __restrict__ jobs, int njobs, int Ho, int Wo, uint32_t* __restrict__ gray_sums) {
    __shared__ uint32_t stage[AUG_PIX * 3 / 4];
    __shared__ int wave_part[AUG_PIX / ZSG_WAVE];
    const int j = aug_find_job<1>(jobs, njobs);
    const ZsgAugJob jb = jobs[j];
    const int lb = (int)blockIdx.x - jb.blk0_y;
    const int total = Ho * Wo;
    const int i = lb * AUG_PIX + (int)threadIdx.x;
    int gray = 0;
    if (i < total) {
        const int x = i % Wo, y = i / Wo;
        const int32_t* bounds = (const int32_t*)jb.yb;
        const int first = bounds[2 * y], n = bounds[2 * y + 1];
        const int32_t* k = (const int32_t*)jb.yc + (int64_t)y * jb.yk;
        const uint8_t* p = (const uint8_t*)jb.tmp + ((int64_t)first * Wo + x) * 3;
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
        for (int t = 0; t < n; ++t) {
            const int kt = k[t];
            const uint8_t* q = p + (int64_t)t * Wo * 3;
            a0 += (int)q[0] * kt;
            a1 += (int)q[1] * kt;
            a2 += (int)q[2] * kt;
        }
        const float r = aug_blend((float)aug_clip8(a0), 0.0f, jb.fb);
        const float g = aug_blend((float)aug_clip8(a1), 0.0f, jb.fb);
        const float b = aug_blend((float)aug_clip8(a2), 0.0f, jb.fb);
        uint8_t* s = (uint8_t*)stage + 3 * (int)threadIdx.x;
        s[0] = (uint8_t)(int)r;
        s[1] = (uint8_t)(int)g;
        s[2] = (uint8_t)(int)b;
        gray = aug_gray(r, g, b);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) gray += __shfl_xor(gray, o, ZSG_WAVE);
    if ((threadIdx.x & (ZSG_WAVE - 1)) == 0) wave_part[threadIdx.x / ZSG_WAVE] = gray;
    __syncthreads();
    const int nb = min(AUG_PIX, total - lb * AUG_PIX) * 3;
    aug_store_block((uint8_t*)jb.out + (int64_t)lb * AUG_PIX * 3, stage, nb);
    if (threadIdx.x == 0) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < AUG_PIX / ZSG_WAVE; ++w) s += wave_part[w];
        atomicAdd(&gray_sums[j], (uint32_t)s);       // integers: the sum does not depend on the order of the blocks
    }
}

// launch 3: contrast against the image's mean gray value, then saturation against the pixel's own gray value, in place
__global__ __launch_bounds__(AUG_PIX) void aug_cs_kernel(const ZsgAugJob* __restrict__ jobs, int njobs, int Ho, int Wo, const uint32_t* __restrict__ gray_sums) {
    __shared__ uint32_t stage[AUG_PIX * 3 / 4];
    const int j = aug_find_job<1>(jobs, njobs);
    const ZsgAugJob jb = jobs[j];
    if (jb.fc == 1.0f && jb.fs == 1.0f) return;      // (block-uniform: both steps are the identity)
    const int lb = (int)blockIdx.x - jb.blk0_y;
    const int total = Ho * Wo;
    const int nb = min(AUG_PIX, total - lb * AUG_PIX) * 3;
    uint8_t* base = (uint8_t*)jb.out + (int64_t)lb * AUG_PIX * 3;
    aug_load_block(base, stage, nb);
    __syncthreads();
    const float mean = (float)((double)gray_sums[j] / (double)total);      // exact integer sum, one rounding to fp32
    if (lb * AUG_PIX + (int)threadIdx.x < total) {
        uint8_t* s = (uint8_t*)stage + 3 * (int)threadIdx.x;
        const float r = aug_blend((float)s[0], mean, jb.fc);
        const float g = aug_blend((float)s[1], mean, jb.fc);
        const float b = aug_blend((float)s[2], mean, jb.fc);
        const float gr = (float)aug_gray(r, g, b);
        s[0] = (uint8_t)(int)aug_blend(r, gr, jb.fs);
        s[1] = (uint8_t)(int)aug_blend(g, gr, jb.fs);
        s[2] = (uint8_t)(int)aug_blend(b, gr, jb.fs);
    }
    __syncthreads();
    aug_store_block(base, stage, nb);
}

extern "C" int zsg_augment_u8_batched(const void* jobs_dev, int32_t njobs, int32_t Ho, int32_t Wo, int32_t blocks_x, int32_t blocks_y,
                                      void* gray_sums, int32_t do_cs, void* stream) {
    ZSG_REQUIRE(jobs_dev && gray_sums && njobs > 0 && Ho > 0 && Wo > 0 && blocks_x > 0 && blocks_y > 0, "augment_u8_batched: bad argument");
    ZSG_REQUIRE((int64_t)Ho * Wo <= (1 << 24), "augment_u8_batched: %d x %d outputs overflow the 32-bit gray accumulator", Ho, Wo);
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("augment_u8", st, 0, 0);
    const ZsgAugJob* jobs = (const ZsgAugJob*)jobs_dev;
    ZSG_LAUNCH(aug_hpass_kernel, dim3(blocks_x), dim3(AUG_PIX), 0, st, jobs, njobs, Wo, (uint32_t*)gray_sums);
    ZSG_LAUNCH(aug_vpass_kernel, dim3(blocks_y), dim3(AUG_PIX), 0, st, jobs, njobs, Ho, Wo, (uint32_t*)gray_sums);
    if (do_cs) ZSG_LAUNCH(aug_cs_kernel, dim3(blocks_y), dim3(AUG_PIX), 0, st, jobs, njobs, Ho, Wo, (const uint32_t*)gray_sums);
    ZSG_CHECK_LAUNCH("augment_u8_batched");
    return 0;
}

// ---- windows that leave the image (zoom-out) and the horizontal flip: zsg_augment_geom_u8_batched ---------------------------------------
// The same three launches, thread mapping and staging; the kernels above stay as they are.  The job names its IMAGE (pixel (0, 0),
// height, width) and the window by a signed origin and its sides: launch 1 checks every tap's source pixel against the image and takes
// the fill colour outside it (a window row above or below the image is fill through the same sum), so no window can make it read
// outside [0, ih) x [0, iw).  The flip mirrors on the READ side of launch 2 — the thread of output column x filters scratch column
// Wo - 1 - x — so a block's output bytes stay the contiguous run the dword stores need.
struct ZsgAugGeomJob {
    int64_t img, tmp, out;                 // absolute device addresses: the image's pixel (0, 0), scratch [wh][Wo][3], result [Ho][Wo][3]
    int64_t xb, xc, yb, yc;                // tap tables (int32) for the window's sides
    int32_t ih, iw;                        // image height / width (the row pitch is the width)
    int32_t wx0, wy0, wh, ww;              // window origin in image pixels (any sign) and its sides
    int32_t xk, yk;                        // tap-table widths
    int32_t blk0_x, blk0_y;                // first block of the job in launch 1 / launches 2 and 3 (256 pixels per block)
    int32_t flags;                         // bit 0: mirror left-right
    uint32_t fill;                         // r | g << 8 | b << 16: the colour outside the image
    float fb, fc, fs;                      // brightness, contrast, saturation factors (1 = identity)
    int32_t pad;
};
static_assert(sizeof(ZsgAugGeomJob) == 120, "ZsgAugGeomJob is packed by dat_loader.GpuResizer");

#define AUG_MAX_SIDE (1 << 15)             // window and image sides: h * Wo and every pixel index stay far inside 32 / 64 bits

template <int AXIS>
__device__ __forceinline__ int aug_geom_find_job(const ZsgAugGeomJob* __restrict__ jobs, int njobs) {
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((AXIS == 0 ? jobs[mid].blk0_x : jobs[mid].blk0_y) <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(AUG_PIX) void aug_geom_hpass_kernel(const ZsgAugGeomJob* __restrict__ jobs, int njobs, int Wo, uint32_t* __restrict__ gray_sums) {
    __shared__ uint32_t stage[AUG_PIX * 3 / 4];
    const int j = aug_geom_find_job<0>(jobs, njobs);
    const ZsgAugGeomJob jb = jobs[j];
    const int lb = (int)blockIdx.x - jb.blk0_x;
    if (lb == 0 && threadIdx.x == 0) gray_sums[j] = 0u;
    const int total = jb.wh * Wo;
    const int i = lb * AUG_PIX + (int)threadIdx.x;
    if (i < total) {
        const int x = i % Wo, y = i / Wo;
        const int32_t* bounds = (const int32_t*)jb.xb;
        const int first = bounds[2 * x], n = bounds[2 * x + 1];
        const int32_t* k = (const int32_t*)jb.xc + (int64_t)x * jb.xk;
        const int iy = jb.wy0 + y;
        const bool row_in = iy >= 0 && iy < jb.ih;
        const uint8_t* row = (const uint8_t*)jb.img + (int64_t)(row_in ? iy : 0) * jb.iw * 3;
        const int c0 = jb.wx0 + first;                                       // image column of the first tap
        const int f0 = (int)(jb.fill & 255u), f1 = (int)((jb.fill >> 8) & 255u), f2 = (int)((jb.fill >> 16) & 255u);
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
        for (int t = 0; t < n; ++t) {
            const int kt = k[t];
            const int c = c0 + t;
            int p0 = f0, p1 = f1, p2 = f2;
            if (row_in && c >= 0 && c < jb.iw) {                             // the only reads of the image: inside it
                const uint8_t* p = row + (int64_t)c * 3;
                p0 = p[0];
                p1 = p[1];
                p2 = p[2];
            }
            a0 += p0 * kt;
            a1 += p1 * kt;
            a2 += p2 * kt;
        }
        uint8_t* s = (uint8_t*)stage + 3 * (int)threadIdx.x;
        s[0] = (uint8_t)aug_clip8(a0);
        s[1] = (uint8_t)aug_clip8(a1);
        s[2] = (uint8_t)aug_clip8(a2);
    }
    __syncthreads();
    const int nb = min(AUG_PIX, total - lb * AUG_PIX) * 3;
    aug_store_block((uint8_t*)jb.tmp + (int64_t)lb * AUG_PIX * 3, stage, nb);
}

__global__ __launch_bounds__(AUG_PIX) void aug_geom_vpass_kernel(const ZsgAugGeomJob* __restrict__ jobs, int njobs, int Ho, int Wo, uint32_t* __restrict__ gray_sums) {
    __shared__ uint32_t stage[AUG_PIX * 3 / 4];
    __shared__ int wave_part[AUG_PIX / ZSG_WAVE];
    const int j = aug_geom_find_job<1>(jobs, njobs);
    const ZsgAugGeomJob jb = jobs[j];
    const int lb = (int)blockIdx.x - jb.blk0_y;
    const int total = Ho * Wo;
    const int i = lb * AUG_PIX + (int)threadIdx.x;
    int gray = 0;
    if (i < total) {
        const int x = i % Wo, y = i / Wo;
        const int xs = (jb.flags & 1) ? Wo - 1 - x : x;                      // the flip: output column x is scratch column Wo - 1 - x
        const int32_t* bounds = (const int32_t*)jb.yb;
        const int first = bounds[2 * y], n = bounds[2 * y + 1];
        const int32_t* k = (const int32_t*)jb.yc + (int64_t)y * jb.yk;
        const uint8_t* p = (const uint8_t*)jb.tmp + ((int64_t)first * Wo + xs) * 3;
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
        for (int t = 0; t < n; ++t) {
            const int kt = k[t];
            const uint8_t* q = p + (int64_t)t * Wo * 3;
            a0 += (int)q[0] * kt;
            a1 += (int)q[1] * kt;
            a2 += (int)q[2] * kt;
        }
        const float r = aug_blend((float)aug_clip8(a0), 0.0f, jb.fb);
        const float g = aug_blend((float)aug_clip8(a1), 0.0f, jb.fb);
        const float b = aug_blend((float)aug_clip8(a2), 0.0f, jb.fb);
        uint8_t* s = (uint8_t*)stage + 3 * (int)threadIdx.x;
        s[0] = (uint8_t)(int)r;
        s[1] = (uint8_t)(int)g;
        s[2] = (uint8_t)(int)b;
        gray = aug_gray(r, g, b);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) gray += __shfl_xor(gray, o, ZSG_WAVE);
    if ((threadIdx.x & (ZSG_WAVE - 1)) == 0) wave_part[threadIdx.x / ZSG_WAVE] = gray;
    __syncthreads();
    const int nb = min(AUG_PIX, total - lb * AUG_PIX) * 3;
    aug_store_block((uint8_t*)jb.out + (int64_t)lb * AUG_PIX * 3, stage, nb);
    if (threadIdx.x == 0) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < AUG_PIX / ZSG_WAVE; ++w) s += wave_part[w];
        atomicAdd(&gray_sums[j], (uint32_t)s);
    }
}

// launch 3 of aug_cs_kernel for the other job record: the same arithmetic, in place
__global__ __launch_bounds__(AUG_PIX) void aug_geom_cs_kernel(const ZsgAugGeomJob* __restrict__ jobs, int njobs, int Ho, int Wo, const uint32_t* __restrict__ gray_sums) {
    __shared__ uint32_t stage[AUG_PIX * 3 / 4];
    const int j = aug_geom_find_job<1>(jobs, njobs);
    const ZsgAugGeomJob jb = jobs[j];
    if (jb.fc == 1.0f && jb.fs == 1.0f) return;
    const int lb = (int)blockIdx.x - jb.blk0_y;
    const int total = Ho * Wo;
    const int nb = min(AUG_PIX, total - lb * AUG_PIX) * 3;
    uint8_t* base = (uint8_t*)jb.out + (int64_t)lb * AUG_PIX * 3;
    aug_load_block(base, stage, nb);
    __syncthreads();
    const float mean = (float)((double)gray_sums[j] / (double)total);
    if (lb * AUG_PIX + (int)threadIdx.x < total) {
        uint8_t* s = (uint8_t*)stage + 3 * (int)threadIdx.x;
        const float r = aug_blend((float)s[0], mean, jb.fc);
        const float g = aug_blend((float)s[1], mean, jb.fc);
        const float b = aug_blend((float)s[2], mean, jb.fc);
        const float gr = (float)aug_gray(r, g, b);
        s[0] = (uint8_t)(int)aug_blend(r, gr, jb.fs);
        s[1] = (uint8_t)(int)aug_blend(g, gr, jb.fs);
        s[2] = (uint8_t)(int)aug_blend(b, gr, jb.fs);
    }
    __syncthreads();
    aug_store_block(base, stage, nb);
}

// jobs_host (optional): the table as the caller packed it — every record is checked before anything is launched: addresses present,
// sides positive and within AUG_MAX_SIDE, the origin within +-2^24, tap-table widths positive, and the first blocks exactly the running
// sums of ceil(wh * Wo / 256) and ceil(Ho * Wo / 256) with blocks_x / blocks_y their totals (a block past its job's pixels would index
// the tap tables out of range).
extern "C" int zsg_augment_geom_u8_batched(const void* jobs_dev, const void* jobs_host, int32_t njobs, int32_t Ho, int32_t Wo, int32_t blocks_x,
                                           int32_t blocks_y, void* gray_sums, int32_t do_cs, void* stream) {
    ZSG_REQUIRE(jobs_dev && gray_sums && njobs > 0 && Ho > 0 && Wo > 0 && blocks_x > 0 && blocks_y > 0, "augment_geom_u8_batched: bad argument");
    ZSG_REQUIRE((int64_t)Ho * Wo <= (1 << 24), "augment_geom_u8_batched: %d x %d outputs overflow the 32-bit gray accumulator", Ho, Wo);
    if (jobs_host) {
        const ZsgAugGeomJob* h = (const ZsgAugGeomJob*)jobs_host;
        int64_t bx = 0, by = 0;
        for (int32_t i = 0; i < njobs; ++i) {
            const ZsgAugGeomJob& q = h[i];
            ZSG_REQUIRE(q.img && q.tmp && q.out && q.xb && q.xc && q.yb && q.yc, "augment_geom_u8_batched: job %d: null address", i);
            ZSG_REQUIRE(q.ih > 0 && q.iw > 0 && q.ih <= AUG_MAX_SIDE && q.iw <= AUG_MAX_SIDE, "augment_geom_u8_batched: job %d: image %d x %d", i, q.ih, q.iw);
            ZSG_REQUIRE(q.wh > 0 && q.ww > 0 && q.wh <= AUG_MAX_SIDE && q.ww <= AUG_MAX_SIDE, "augment_geom_u8_batched: job %d: window %d x %d (sides 1..%d)",
                        i, q.wh, q.ww, AUG_MAX_SIDE);
            ZSG_REQUIRE((int64_t)q.wh * Wo <= (1 << 28), "augment_geom_u8_batched: job %d: %d window rows x %d columns of scratch", i, q.wh, Wo);
            ZSG_REQUIRE(q.wx0 > -(1 << 24) && q.wx0 < (1 << 24) && q.wy0 > -(1 << 24) && q.wy0 < (1 << 24), "augment_geom_u8_batched: job %d: window origin", i);
            ZSG_REQUIRE(q.xk > 0 && q.yk > 0 && (q.tmp & 3) == 0, "augment_geom_u8_batched: job %d: tap-table width / scratch alignment", i);
            ZSG_REQUIRE(q.blk0_x == bx && q.blk0_y == by, "augment_geom_u8_batched: job %d: first blocks %d, %d are not the running sums", i, q.blk0_x, q.blk0_y);
            bx += ((int64_t)q.wh * Wo + AUG_PIX - 1) / AUG_PIX;
            by += ((int64_t)Ho * Wo + AUG_PIX - 1) / AUG_PIX;
        }
        ZSG_REQUIRE(bx == blocks_x && by == blocks_y, "augment_geom_u8_batched: blocks_x / blocks_y are not the jobs' totals");
    }
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("augment_geom_u8", st, 0, 0);
    const ZsgAugGeomJob* jobs = (const ZsgAugGeomJob*)jobs_dev;
    ZSG_LAUNCH(aug_geom_hpass_kernel, dim3(blocks_x), dim3(AUG_PIX), 0, st, jobs, njobs, Wo, (uint32_t*)gray_sums);
    ZSG_LAUNCH(aug_geom_vpass_kernel, dim3(blocks_y), dim3(AUG_PIX), 0, st, jobs, njobs, Ho, Wo, (uint32_t*)gray_sums);
    if (do_cs) ZSG_LAUNCH(aug_geom_cs_kernel, dim3(blocks_y), dim3(AUG_PIX), 0, st, jobs, njobs, Ho, Wo, (const uint32_t*)gray_sums);
    ZSG_CHECK_LAUNCH("augment_geom_u8_batched");
    return 0;
}

// ---- affine warp and Gaussian blur of the finished batch: zsg_augment_warp_u8_batched ---------------------------------------------------
// Steps 6 and 7 of dat_loader.augment_host, on the [Ho][Wo][3] result of either entry above.  No floating point: the host rounds the
// inverse map to six 16.16 integers and the blur to at most 17 16-bit taps that sum to 65536; host and GPU evaluate the same integer
// expressions.  Up to three launches — warp, blur along x, blur along y — of one thread per output pixel, 256 pixels per block; every
// job has Ho * Wo pixels, so the running block sums are j * ceil(Ho * Wo / 256) and a block finds its job by one division.  A job
// without a stage is copied through that stage; a launch no job needs is not made.  Buffers: warp src -> out; blur-x (src or out) ->
// scratch; blur-y scratch -> out.  The source is only ever read.
struct ZsgAugWarpJob {
    int64_t src, out;                      // absolute device addresses: the image [Ho][Wo][3] to warp / blur, the result [Ho][Wo][3]
    int32_t m[6];                          // a, b, c0, d, e, c1: source position of output pixel (x, y) in 16.16, SU = a x + b y + c0, SV = d x + e y + c1
    uint32_t fill;                         // r | g << 8 | b << 16: the colour of a tap outside the image
    int32_t flags;                         // bit 0: warp, bit 1: blur
    int32_t radius;                        // blur radius r, 0..8: taps[0 .. 2r] weigh pixels i - r .. i + r (clamped to the image)
    int32_t taps[17];
    int32_t pad[2];
};
static_assert(sizeof(ZsgAugWarpJob) == 128, "ZsgAugWarpJob is packed by dat_loader.GpuResizer");

#define AUG_WARP_MAX_R 8

// the buffer a launch reads or writes: 0 = the job's source, 1 = the job's result, 2 = the job's slice of the scratch batch
__device__ __forceinline__ uint8_t* aug_warp_buf(const ZsgAugWarpJob* jp, int sel, int j, uint8_t* tmp, int64_t tmp_stride) {
    return sel == 0 ? (uint8_t*)jp->src : (sel == 1 ? (uint8_t*)jp->out : tmp + (int64_t)j * tmp_stride);
}

// STAGE 0: warp, 1: blur along x, 2: blur along y
template <int STAGE>
__global__ __launch_bounds__(AUG_PIX) void aug_warp_stage_kernel(const ZsgAugWarpJob* __restrict__ jobs, int Ho, int Wo, int bpj, int in_sel, int out_sel,
                                                                 uint8_t* tmp, int64_t tmp_stride) {
    __shared__ uint32_t stage[AUG_PIX * 3 / 4];
    const int j = (int)blockIdx.x / bpj, lb = (int)blockIdx.x - j * bpj;
    const ZsgAugWarpJob* jp = jobs + j;
    const uint8_t* in = aug_warp_buf(jp, in_sel, j, tmp, tmp_stride);
    uint8_t* out = aug_warp_buf(jp, out_sel, j, tmp, tmp_stride);
    const int total = Ho * Wo;
    const int nb = min(AUG_PIX, total - lb * AUG_PIX) * 3;
    const int64_t boff = (int64_t)lb * AUG_PIX * 3;
    if (!(jp->flags & (STAGE == 0 ? 1 : 2))) {       // (block-uniform) the job has no such stage: its bytes pass through
        aug_load_block(in + boff, stage, nb);
        __syncthreads();
        aug_store_block(out + boff, stage, nb);
        return;
    }
    const int i = lb * AUG_PIX + (int)threadIdx.x;
    if (i < total) {
        const int x = i % Wo, y = i / Wo;
        int v0, v1, v2;
        if (STAGE == 0) {
            const int64_t SU = (int64_t)jp->m[0] * x + (int64_t)jp->m[1] * y + jp->m[2];      // 64 bits: exact for any int32 coefficients
            const int64_t SV = (int64_t)jp->m[3] * x + (int64_t)jp->m[4] * y + jp->m[5];
            const int fx = (int)((SU >> 8) & 255), fy = (int)((SV >> 8) & 255);
            // [-2, side]: far outside stays outside for both taps of the axis, and the indices fit 32 bits
            const int ix = (int)max(min(SU >> 16, (int64_t)Wo), (int64_t)-2), iy = (int)max(min(SV >> 16, (int64_t)Ho), (int64_t)-2);
            const uint32_t fill = jp->fill;
            int p[4][3];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int xx = ix + (t & 1), yy = iy + (t >> 1);
                p[t][0] = (int)(fill & 255u);
                p[t][1] = (int)((fill >> 8) & 255u);
                p[t][2] = (int)((fill >> 16) & 255u);
                if (xx >= 0 && xx < Wo && yy >= 0 && yy < Ho) {                             // the only reads of the image: inside it
                    const uint8_t* q = in + ((int64_t)yy * Wo + xx) * 3;
                    p[t][0] = q[0];
                    p[t][1] = q[1];
                    p[t][2] = q[2];
                }
            }
            const int gx = 256 - fx, gy = 256 - fy;
            v0 = ((p[0][0] * gx + p[1][0] * fx) * gy + (p[2][0] * gx + p[3][0] * fx) * fy + 32768) >> 16;
            v1 = ((p[0][1] * gx + p[1][1] * fx) * gy + (p[2][1] * gx + p[3][1] * fx) * fy + 32768) >> 16;
            v2 = ((p[0][2] * gx + p[1][2] * fx) * gy + (p[2][2] * gx + p[3][2] * fx) * fy + 32768) >> 16;
        } else {
            const int r = min(max(jp->radius, 0), AUG_WARP_MAX_R);
            const int n = STAGE == 1 ? Wo : Ho, c = STAGE == 1 ? x : y;
            int a0 = 32768, a1 = 32768, a2 = 32768;
            for (int k = -r; k <= r; ++k) {
                const int t = jp->taps[k + r];
                const int cc = min(max(c + k, 0), n - 1);
                const uint8_t* q = in + (STAGE == 1 ? (int64_t)y * Wo + cc : (int64_t)cc * Wo + x) * 3;
                a0 += t * (int)q[0];
                a1 += t * (int)q[1];
                a2 += t * (int)q[2];
            }
            v0 = a0 >> 16;
            v1 = a1 >> 16;
            v2 = a2 >> 16;
        }
        uint8_t* s = (uint8_t*)stage + 3 * (int)threadIdx.x;
        s[0] = (uint8_t)v0;
        s[1] = (uint8_t)v1;
        s[2] = (uint8_t)v2;
    }
    __syncthreads();
    aug_store_block(out + boff, stage, nb);
}

// stages: bit 0 = some job warps, bit 1 = some job blurs (the launches made).  tmp: scratch of njobs slices of Ho * Wo * 3 bytes rounded
// up to a multiple of 4, needed only with bit 1.  jobs_host (optional): the table as the caller packed it — every record is checked
// before anything is launched: addresses present, flags within `stages`, a blur's radius in 0..8 with taps >= 0 that sum to 65536, fill
// below 2^24, and the sources, the results and the scratch lying in three disjoint address ranges (no stage may write what another
// block of its launch reads).  The map's sums are taken in 64 bits, so every int32 coefficient is valid.
extern "C" int zsg_augment_warp_u8_batched(const void* jobs_dev, const void* jobs_host, int32_t njobs, int32_t Ho, int32_t Wo, void* tmp,
                                           int32_t stages, void* stream) {
    ZSG_REQUIRE(jobs_dev && (((uintptr_t)jobs_dev) & 7) == 0, "augment_warp_u8_batched: the job table is null or not 8-byte aligned");
    ZSG_REQUIRE(njobs > 0 && Ho > 0 && Wo > 0 && Ho <= AUG_MAX_SIDE && Wo <= AUG_MAX_SIDE, "augment_warp_u8_batched: %d jobs of %d x %d (sides 1..%d)",
                njobs, Ho, Wo, AUG_MAX_SIDE);
    ZSG_REQUIRE(stages >= 1 && stages <= 3, "augment_warp_u8_batched: stages = %d (bit 0 warp, bit 1 blur; at least one)", stages);
    ZSG_REQUIRE(!(stages & 2) || (tmp && (((uintptr_t)tmp) & 3) == 0), "augment_warp_u8_batched: a blur needs 4-byte aligned scratch");
    const int64_t per = (int64_t)Ho * Wo * 3, tmp_stride = (per + 3) / 4 * 4;
    const int64_t bpj = ((int64_t)Ho * Wo + AUG_PIX - 1) / AUG_PIX;
    ZSG_REQUIRE(bpj * njobs <= 0x7fffffffLL, "augment_warp_u8_batched: %d jobs of %d x %d need too many blocks", njobs, Ho, Wo);
    if (jobs_host) {
        ZSG_REQUIRE((((uintptr_t)jobs_host) & 7) == 0, "augment_warp_u8_batched: the host table is not 8-byte aligned");
        const ZsgAugWarpJob* h = (const ZsgAugWarpJob*)jobs_host;
        int64_t s_lo = INT64_MAX, s_hi = INT64_MIN, o_lo = INT64_MAX, o_hi = INT64_MIN;
        for (int32_t i = 0; i < njobs; ++i) {
            const ZsgAugWarpJob& q = h[i];
            ZSG_REQUIRE(q.src && q.out, "augment_warp_u8_batched: job %d: null address", i);
            ZSG_REQUIRE(q.flags >= 0 && (q.flags & ~stages) == 0, "augment_warp_u8_batched: job %d: flags %d outside stages %d", i, q.flags, stages);
            ZSG_REQUIRE(q.fill < (1u << 24), "augment_warp_u8_batched: job %d: fill", i);
            if (q.flags & 2) {
                ZSG_REQUIRE(q.radius >= 0 && q.radius <= AUG_WARP_MAX_R, "augment_warp_u8_batched: job %d: radius %d (0..%d)", i, q.radius, AUG_WARP_MAX_R);
                int64_t sum = 0;
                for (int k = 0; k <= 2 * q.radius; ++k) {
                    ZSG_REQUIRE(q.taps[k] >= 0, "augment_warp_u8_batched: job %d: tap %d is negative", i, k);
                    sum += q.taps[k];
                }
                ZSG_REQUIRE(sum == 65536, "augment_warp_u8_batched: job %d: the taps sum to %lld, not 65536", i, (long long)sum);
            }
            s_lo = q.src < s_lo ? q.src : s_lo;
            s_hi = q.src + per > s_hi ? q.src + per : s_hi;
            o_lo = q.out < o_lo ? q.out : o_lo;
            o_hi = q.out + per > o_hi ? q.out + per : o_hi;
        }
        ZSG_REQUIRE(s_hi <= o_lo || o_hi <= s_lo, "augment_warp_u8_batched: the results overlap the sources");
        if (stages & 2) {
            const int64_t t_lo = (int64_t)(uintptr_t)tmp, t_hi = t_lo + tmp_stride * njobs;
            ZSG_REQUIRE((t_hi <= o_lo || o_hi <= t_lo) && (t_hi <= s_lo || s_hi <= t_lo), "augment_warp_u8_batched: the scratch overlaps the sources or the results");
        }
    }
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("augment_warp_u8", st, 0, 0);
    const ZsgAugWarpJob* jobs = (const ZsgAugWarpJob*)jobs_dev;
    const dim3 grid((unsigned)(bpj * njobs));
    if (stages & 1) ZSG_LAUNCH(aug_warp_stage_kernel<0>, grid, dim3(AUG_PIX), 0, st, jobs, Ho, Wo, (int)bpj, 0, 1, (uint8_t*)tmp, tmp_stride);
    if (stages & 2) {
        ZSG_LAUNCH(aug_warp_stage_kernel<1>, grid, dim3(AUG_PIX), 0, st, jobs, Ho, Wo, (int)bpj, (stages & 1) ? 1 : 0, 2, (uint8_t*)tmp, tmp_stride);
        ZSG_LAUNCH(aug_warp_stage_kernel<2>, grid, dim3(AUG_PIX), 0, st, jobs, Ho, Wo, (int)bpj, 2, 1, (uint8_t*)tmp, tmp_stride);
    }
    ZSG_CHECK_LAUNCH("augment_warp_u8_batched");
    return 0;
}
