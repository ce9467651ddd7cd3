// ema.hip — exponential moving average of the weights over flat fp32 buffers (torch.optim.swa_utils.AveragedModel with
// get_ema_multi_avg_fn, use_buffers=True), and the one-pass exchange of two buffers that puts the average into the network for evaluation.
// HBM-bound: the update reads p and ema and writes ema (12 B per element), the exchange reads and writes both (16 B per element).
// The update that rides in the Adam launch is adam.hip's adam_kernel<true>; the rule itself is ema.h's, the same in every kernel.
#include "common.h"
#include "ema.h"

// One grid-stride loop over the 16-byte groups of range a followed by those of range b (n4b == 0: one range); the < 4 element tails of
// both ranges go to the first threads of block 0.
__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ ea, const float* __restrict__ a, int64_t n4a, int64_t na,
                                                         float* __restrict__ eb, const float* __restrict__ b, int64_t n4b, int64_t nb,
                                                         float w) {
    const int64_t n4 = n4a + n4b;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const bool first = i < n4a;
        const int64_t k = 4 * (first ? i : i - n4a);
        float* e = (first ? ea : eb) + k;
        const f32x4 pp = *(const f32x4*)((first ? a : b) + k);
        f32x4 ee = *(const f32x4*)e;
#pragma unroll
        for (int c = 0; c < 4; ++c) ee[c] = zsg_ema_rule(ee[c], pp[c], w);
        *(f32x4*)e = ee;
    }
    if (blockIdx.x == 0) {
        const int ta = (int)(na - 4 * n4a), tb = (int)(nb - 4 * n4b);
        const int t = threadIdx.x;
        if (t < ta) {
            const int64_t i = 4 * n4a + t;
            ea[i] = zsg_ema_rule(ea[i], a[i], w);
        } else if (t - ta < tb) {
            const int64_t i = 4 * n4b + (t - ta);
            eb[i] = zsg_ema_rule(eb[i], b[i], w);
        }
    }
}

// a <-> b in one pass: both 16-byte groups are loaded before either is stored
__global__ __launch_bounds__(256) void swap_kernel(float* __restrict__ a, float* __restrict__ b, int64_t n4, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const f32x4 x = *(const f32x4*)(a + 4 * i);
        const f32x4 y = *(const f32x4*)(b + 4 * i);
        *(f32x4*)(a + 4 * i) = y;
        *(f32x4*)(b + 4 * i) = x;
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(n - 4 * n4)) {
        const int64_t i = 4 * n4 + threadIdx.x;
        const float x = a[i], y = b[i];
        a[i] = y;
        b[i] = x;
    }
}

// the grid of a streaming pass over n4 16-byte groups: capped as adam_launch caps its own
static int stream_blocks(int64_t n4) {
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > ZSG_NUM_CU * 8) blocks = ZSG_NUM_CU * 8;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

extern "C" int zsg_ema_update(float* ema_a, const float* a, int64_t na, float* ema_b, const float* b, int64_t nb, float w, void* stream) {
    ZSG_REQUIRE(ema_a && a && na > 0, "ema_update: bad first range");
    ZSG_REQUIRE((ema_b && b && nb > 0) || (!ema_b && !b && nb == 0), "ema_update: the second range is given in full (ema_b, b, nb > 0) or not at all");
    ZSG_REQUIRE(w >= 0.f && w <= 1.f, "ema_update: weight %g outside [0, 1]", (double)w);
    ZSG_REQUIRE((((uintptr_t)ema_a | (uintptr_t)a | (uintptr_t)ema_b | (uintptr_t)b) & 15) == 0, "ema_update: buffers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("ema_update", st, 0, (double)(na + nb) * 12);
    const int64_t n4a = na / 4, n4b = nb / 4;
    ZSG_LAUNCH(ema_update_kernel, dim3(stream_blocks(n4a + n4b)), dim3(256), 0, st, ema_a, a, n4a, na, ema_b, b, n4b, nb, w);
    ZSG_CHECK_LAUNCH("ema_update");
    return 0;
}

extern "C" int zsg_swap_f32(float* a, float* b, int64_t n, void* stream) {
    ZSG_REQUIRE(a && b && n > 0, "swap_f32: bad argument");
    ZSG_REQUIRE((((uintptr_t)a | (uintptr_t)b) & 15) == 0, "swap_f32: buffers must be 16-byte aligned");
    ZSG_REQUIRE((uintptr_t)a + 4 * (uintptr_t)n <= (uintptr_t)b || (uintptr_t)b + 4 * (uintptr_t)n <= (uintptr_t)a, "swap_f32: the buffers overlap");
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("swap_f32", st, 0, (double)n * 16);
    ZSG_LAUNCH(swap_kernel, dim3(stream_blocks(n / 4)), dim3(256), 0, st, a, b, n / 4, n);
    ZSG_CHECK_LAUNCH("swap_f32");
    return 0;
}
