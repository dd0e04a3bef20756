// Per-row fp8 e4m3fn quantisation rule shared by o3v_fp8.hip (o3v_quantize_rows_fp8, o3v_rmsnorm_quantize_fp8) and
// o3v_repack.hip (o3v_repack_rows): scale = 2^e, e = the smallest integer with amax / 2^e <= 448 (amax = 0: scale 1);
// q = fp8(y / scale) (exact division, RNE).  Restates weights.quantize_rows_fp8 bit for bit.
#pragma once
#include "o3v_common.h"

__device__ __forceinline__ float pow2_scale_for(float amax) {
    if (!(amax > 0.f)) return 1.0f;
    int e;
    const float m = frexpf(amax, &e);  // amax = m * 2^e, m in [0.5, 1); 448 = 0.875 * 2^9: amax / 2^E <= 448 <=> m * 2^(e-E) <= 0.875 * 2^9
    return ldexpf(1.0f, m <= 0.875f ? e - 9 : e - 8);
}

__device__ __forceinline__ uint2 pack8_fp8(const float (&y)[8], float inv) {
    uint32_t lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[0] * inv, y[1] * inv, lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[2] * inv, y[3] * inv, lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[4] * inv, y[5] * inv, hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[6] * inv, y[7] * inv, hi, true);
    return make_uint2(lo, hi);
}
