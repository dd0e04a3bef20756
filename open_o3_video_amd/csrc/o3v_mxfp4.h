// OCP MX v1.0 MXFP4 of the decode MLP weights, shared by o3v_gemm.hip (the kernels that stream it), o3v_mxfp4.hip
// (o3v_quantize_rows_mxfp4) and o3v_repack.hip (o3v_repack_rows).  Restates weights.quantize_rows_mxfp4 bit for bit.
//
//   block    32 consecutive k of one packed matrix row: one e8m0 scale byte + 32 e2m1 codes, two per byte, element 2i in the low
//            nibble of byte i (16 bytes: one lane's load)
//   scale    2^e, e = floor(log2(amax)) - 2 clamped to [-125, 125] (amax = 0: e = 0), stored as e + 127.  amax / 2^e is in [4, 8):
//            the top binade of e2m1; the clamp keeps every dequantised value a normal, finite bf16
//   codes    v / 2^e (exact) rounded to nearest even on {0, 0.5, 1, 1.5, 2, 3, 4, 6}, saturating at 6; bit 3 = sign
//
// Everything is decided on bit patterns and exact products, so no rounding mode or denormal setting can make the device and
// torch disagree: amax is the largest |bf16| pattern of the block, its exponent field gives e, and v * 2^-e is exact (or, far
// below the first threshold, an underflow that rounds to code 0 either way).
#pragma once
#include "o3v_common.h"

// scale code of a block from the largest 15-bit magnitude pattern of its bf16 values
__device__ __forceinline__ uint32_t mx4_scale_code(uint32_t amax15) {
    if (amax15 == 0u) return 127u;
    int e = (int)(amax15 >> 7) - 127 - 2;  // biased exponent field; subnormals (field 0) land below the clamp
    e = e < -125 ? -125 : (e > 125 ? 125 : e);
    return (uint32_t)(e + 127);
}
// 2^-e as a float (scale code 2..252: a normal number)
__device__ __forceinline__ float mx4_inv_scale(uint32_t code) { return __uint_as_float((254u - code) << 23); }
// 2^e as a float: what v_cvt_scalef32_pk_bf16_fp4 takes as its scale
__device__ __forceinline__ float mx4_scale(uint32_t code) { return __uint_as_float(code << 23); }

// e2m1 code of one bf16 value (`bits`: its 16-bit pattern) under the block's 2^-e: thresholds are the midpoints of the grid, a tie
// goes to the code with an even mantissa bit (0, 1, 2, 4: codes 0, 2, 4, 6)
__device__ __forceinline__ uint32_t mx4_code(uint32_t bits, float inv) {
    const float a = __uint_as_float((bits & 0x7fffu) << 16) * inv;
    const uint32_t c = (uint32_t)(a > 0.25f) + (uint32_t)(a >= 0.75f) + (uint32_t)(a > 1.25f) + (uint32_t)(a >= 1.75f) +
                       (uint32_t)(a > 2.5f) + (uint32_t)(a >= 3.5f) + (uint32_t)(a > 5.0f);
    return c | ((bits >> 12) & 8u);
}
// four codes of two packed bf16 pairs p0 (elements 0, 1), p1 (elements 2, 3) -> two code bytes
__device__ __forceinline__ uint32_t mx4_codes4(uint32_t p0, uint32_t p1, float inv) {
    return mx4_code(p0 & 0xffffu, inv) | (mx4_code(p0 >> 16, inv) << 4) | (mx4_code(p1 & 0xffffu, inv) << 8) |
           (mx4_code(p1 >> 16, inv) << 12);
}
// largest magnitude pattern of a packed pair
__device__ __forceinline__ uint32_t mx4_amax2(uint32_t p) {
    const uint32_t a = p & 0x7fffu, b = (p >> 16) & 0x7fffu;
    return a > b ? a : b;
}
