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
