// bf16.h — the ONE fp32 <-> bf16 conversion of libzsg (igemm_bf16.hip, bf16_act.hip), gfx950.
#pragma once
#include "common.h"

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// io_flags of zsg_conv_igemm_bf16_io (include/zsg.h)
#define BF_SRC16 1
#define BF_OUT16 2
#define BF_ADD16 4

// fp32 -> bf16, round-to-nearest-even; +-0, +-inf preserved, NaN stays NaN, a finite value above the largest bf16 becomes inf.  One
// function for the packer, the activation loader and every bf16 store: everything is rounded by the same rule (v_cvt_pk_bf16_f32).
__device__ __forceinline__ unsigned bf16_pack2(float lo, float hi) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const f32x2 v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ uint16_t bf16_round1(float v) { return (uint16_t)(bf16_pack2(v, 0.f) & 0xffffu); }
__device__ __forceinline__ u32x2 bf16_pack4(f32x4 v) { return u32x2{bf16_pack2(v[0], v[1]), bf16_pack2(v[2], v[3])}; }

// bf16 -> fp32: exact (the 16 bits become the high half)
__device__ __forceinline__ float bf16_widen1(uint16_t h) { return __builtin_bit_cast(float, (unsigned)h << 16); }
__device__ __forceinline__ f32x4 bf16_widen4(u32x2 h) {
    return f32x4{__builtin_bit_cast(float, h[0] << 16), __builtin_bit_cast(float, h[0] & 0xffff0000u), __builtin_bit_cast(float, h[1] << 16),
                 __builtin_bit_cast(float, h[1] & 0xffff0000u)};
}
