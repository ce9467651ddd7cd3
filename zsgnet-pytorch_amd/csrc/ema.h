// ema.h — the update rule of the weight average (include/zsg.h, "Weight EMA"), shared by ema.hip and the fused Adam step in adam.hip:
//     ema <- fmaf(w, p - ema, ema),   w = 1 - decay in fp32
// one subtraction and one fused multiply-add.  w == 1 stores p itself (fl(p - ema) + ema need not round back to p, so the copy is a
// select, as torch.lerp returns `end` at weight 1); w == 0 leaves a finite average unchanged (0 * d + ema); a NaN / inf in p propagates.
#pragma once

__device__ __forceinline__ float zsg_ema_rule(float ema, float p, float w) {
    return w == 1.0f ? p : fmaf(w, p - ema, ema);
}
