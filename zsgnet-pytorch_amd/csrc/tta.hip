// tta.hip — flip test-time augmentation of the eval path (ZSGNet.eval_tta("flip")): the two launches around the 2B-row eval forward.
//
//   zsg_tta_flip_stage_*   the caller's B images -> the NHWC4 input of 2B rows: row b is the image as given, row B + b its mirror along W.
//                          Per pixel exactly the four floats zsg_u8hwc_to_nhwc4 / zsg_nchw_to_nhwc4 (misc.hip) write; every input
//                          element is read once and stored twice.
//   zsg_tta_flip_merge     the [2B, A, 5] head output -> [B, A, 5]: anchor a of row b with its mirror partner p of row B + b, one fp32
//                          add (tx: subtract) and one multiply by 0.5 per output, so numpy reproduces the bits (tests/tta_ref.py).
//
// Thread mapping: one thread per input pixel / per (b, a) pair, grid-stride, 256 threads per block.  Plain C++, vector stores, no atomics.
#include "common.h"

static inline int grid_for(int64_t n_items, int block = 256, int cap = ZSG_NUM_CU * 16) {
    const int64_t g = (n_items + block - 1) / block;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// ---- staging ----------------------------------------------------------------------------------------------------------
// U8 = true: img uint8 [B][H][W][3], (r, g, b) / 255 (IEEE division, as u8hwc_to_nhwc4_kernel); U8 = false: img fp32 [B][3][H][W].
template <bool U8>
__global__ void tta_flip_stage_kernel(const void* __restrict__ img, int B, int H, int W, float* __restrict__ out) {
    const int64_t HW = (int64_t)H * W, total = (int64_t)B * HW;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / HW, px = i - b * HW;
        const int64_t y = px / W, x = px - y * W;
        f32x4 v;
        if (U8) {
            const uint8_t* p = (const uint8_t*)img + i * 3;
            v = f32x4{(float)p[0] / 255.0f, (float)p[1] / 255.0f, (float)p[2] / 255.0f, 0.f};
        } else {
            const float* p = (const float*)img + b * 3 * HW + px;
            v = f32x4{p[0], p[HW], p[2 * HW], 0.f};
        }
        *(f32x4*)(out + i * 4) = v;                                                 // row b, (y, x)
        *(f32x4*)(out + (((int64_t)B + b) * HW + y * W + (W - 1 - x)) * 4) = v;      // row B + b, (y, W - 1 - x)
    }
}

static int tta_stage(bool u8, const void* img, int32_t B, int32_t H, int32_t W, float* out, void* stream, const char* name) {
    ZSG_REQUIRE(img && out && B > 0 && H > 0 && W > 0, "%s: bad argument (B=%d H=%d W=%d)", name, B, H, W);
    ZSG_REQUIRE((((uintptr_t)out) & 15) == 0, "%s: out is not 16-byte aligned", name);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)B * H * W;
    ZSG_PROF(name, st, 0, (double)n * (u8 ? 35 : 44));
    if (u8) ZSG_LAUNCH(tta_flip_stage_kernel<true>, dim3(grid_for(n)), dim3(256), 0, st, img, B, H, W, out);
    else ZSG_LAUNCH(tta_flip_stage_kernel<false>, dim3(grid_for(n)), dim3(256), 0, st, img, B, H, W, out);
    ZSG_CHECK_LAUNCH(name);
    return 0;
}
extern "C" int zsg_tta_flip_stage_u8(const uint8_t* img, int32_t B, int32_t H, int32_t W, float* out, void* stream) {
    return tta_stage(true, img, B, H, W, out, stream, "tta_flip_stage_u8");
}
extern "C" int zsg_tta_flip_stage_f32(const float* img, int32_t B, int32_t H, int32_t W, float* out, void* stream) {
    return tta_stage(false, img, B, H, W, out, stream, "tta_flip_stage_f32");
}

// ---- merge ------------------------------------------------------------------------------------------------------------
struct TtaLevels {      // the level table, by value: `levels` is a host array, checked before anything is launched
    int32_t L;
    int32_t off[ZSG_TTA_MAX_LEVELS], w[ZSG_TTA_MAX_LEVELS], n[ZSG_TTA_MAX_LEVELS];      // (a level's height is not needed: y stays)
};

__global__ void tta_flip_merge_kernel(const float* __restrict__ in, int B, int A, TtaLevels lv, float* __restrict__ out) {
    const int64_t total = (int64_t)B * A;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / A;
        const int a = (int)(i - b * A);
        int l = 0;
        while (l + 1 < lv.L && a >= lv.off[l + 1]) ++l;
        const int r = a - lv.off[l], n = lv.n[l], w = lv.w[l];
        const int cell = r / n, k = r - cell * n;
        const int y = cell / w, x = cell - y * w;
        const int p = lv.off[l] + (y * w + (w - 1 - x)) * n + k;
        const float* u = in + i * 5;
        const float* v = in + (((int64_t)B + b) * A + p) * 5;
        float* o = out + i * 5;
        o[0] = 0.5f * (u[0] + v[0]);
        o[1] = 0.5f * (u[1] - v[1]);
        o[2] = 0.5f * (u[2] + v[2]);
        o[3] = 0.5f * (u[3] + v[3]);
        o[4] = 0.5f * (u[4] + v[4]);
    }
}

extern "C" int zsg_tta_flip_merge(const float* out5_2b, int32_t B, int32_t A, const int32_t* levels, int32_t L, float* out, void* stream) {
    ZSG_REQUIRE(out5_2b && levels && out && B > 0 && A > 0, "tta_flip_merge: bad argument");
    ZSG_REQUIRE(L >= 1 && L <= ZSG_TTA_MAX_LEVELS, "tta_flip_merge: L=%d levels, expected 1..%d", L, ZSG_TTA_MAX_LEVELS);
    TtaLevels lv;
    memset(&lv, 0, sizeof(lv));
    lv.L = L;
    int64_t next = 0;
    for (int l = 0; l < L; ++l) {
        const int32_t* e = levels + 4 * l;
        ZSG_REQUIRE(e[1] >= 1 && e[2] >= 1 && e[3] >= 1, "tta_flip_merge: level %d is %d x %d x %d", l, e[1], e[2], e[3]);
        ZSG_REQUIRE(e[0] == next, "tta_flip_merge: level %d starts at anchor %d, expected %lld", l, e[0], (long long)next);
        const int64_t cells = (int64_t)e[1] * e[2];
        ZSG_REQUIRE(cells <= A, "tta_flip_merge: level %d has more cells than A=%d anchors", l, A);
        next += cells * e[3];
        ZSG_REQUIRE(next <= A, "tta_flip_merge: the levels hold more than A=%d anchors", A);
        lv.off[l] = e[0], lv.w[l] = e[2], lv.n[l] = e[3];
    }
    ZSG_REQUIRE(next == A, "tta_flip_merge: the levels hold %lld anchors, expected A=%d", (long long)next, A);
    const int64_t n = (int64_t)B * A;
    const uintptr_t i0 = (uintptr_t)out5_2b, i1 = i0 + (uintptr_t)n * 40, o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)n * 20;
    ZSG_REQUIRE(o1 <= i0 || i1 <= o0, "tta_flip_merge: out overlaps the input");
    hipStream_t st = (hipStream_t)stream;
    ZSG_PROF("tta_flip_merge", st, 0, (double)n * 60);
    ZSG_LAUNCH(tta_flip_merge_kernel, dim3(grid_for(n)), dim3(256), 0, st, out5_2b, B, A, lv, out);
    ZSG_CHECK_LAUNCH("tta_flip_merge");
    return 0;
}
