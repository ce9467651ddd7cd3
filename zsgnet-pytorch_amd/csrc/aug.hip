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
