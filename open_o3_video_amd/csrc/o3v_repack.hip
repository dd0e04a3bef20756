// In-place weight update (DeviceWeights.load_weights): one launch rewrites a set of 16-row destination blocks of one packed
// weight slot from one HF-named source tensor, producing in a single read of the source every image the slot keeps --
//
//   bf16 row-major      [rows][cols] at the slot's row offset: q|k|v fusion, the 16-row gate/up interleave (pack_gate_up), zero
//                       column padding (pad_cols, fc1 / patch_w), Qwen3-VL head_rows on rows (row_map) or columns (col_map)
//   bf16 fragment-major [rows/16][cols/32][64 lanes][8]   (weights.pack_mfma_fragments)
//   fp8 e4m3fn codes    [rows][cols] + one power-of-two f32 scale per row (weights.quantize_rows_fp8, o3v_fp8_rows.h)
//   fp8 fragment-major  [rows/16][cols/64][64 lanes][16]  (weights.pack_mfma_fragments_fp8)
//   MXFP4 codes         [rows][cols/2] + one e8m0 scale byte per 32 columns [rows][cols/32] (weights.quantize_rows_mxfp4, o3v_mxfp4.h)
//   MXFP4 fragment-major [rows/16][cols/128][64 lanes][16] + its scale image [rows/16][ceil(cols/512)][64 lanes][4]
//                       (weights.pack_mfma_fragments_mxfp4)
//
// The source is bf16 (copied bit for bit) or fp32 (rounded to nearest even with torch's rule: any NaN -> 0x7FC0), so the bytes
// equal what a fresh DeviceWeights load of the same tensor builds.  One workgroup (4 waves) per 16-row block; wave w takes the
// 64-column groups w, w+4, ...; lane l of a wave takes row l & 15, columns 64t + 16 (l >> 4) .. +16.  Then the fp8 fragment store
// of a wave is one contiguous KiB, its bf16 fragment stores cover two contiguous KiB, and its row-major stores 16 rows x 128 B.
// With fp8 images the block is read twice: a row-amax pass, then the pass that writes (the second read comes from L2 / MALL).
// An MX block is the 32 columns of two neighbouring lanes (l, l ^ 16): they exchange their maxima and each writes its 8 code bytes.
// Rows outside the launched blocks are not touched in any image.
#include <hip/hip_runtime.h>

#include "../../include/o3v.h"
#include "o3v_common.h"
#include "o3v_fp8_rows.h"
#include "o3v_mxfp4.h"

namespace {

// 16 destination columns c0..c0+15 of source row s (s < 0: a zero row) as 8 packed bf16 pairs.  vec: the widest load the
// source rows allow (16 or 8 bytes; 0: element loads) -- a row pitch like the ViT down_proj's 3420 bf16 is only 8-byte aligned
template <bool F32>
__device__ __forceinline__ void load16(const o3v_repack_desc& d, int vec, int s, int c0, uint32_t (&p)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = 0u;
    if (s < 0) return;
    if (vec && !d.col_map && c0 + 16 <= d.src_cols) {
        if constexpr (F32) {
            const float* r = static_cast<const float*>(d.src) + (size_t)s * d.src_ld + c0;
            if (vec == 16) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 v = reinterpret_cast<const float4*>(r)[q];
                    p[2 * q] = torch_bf16(v.x) | (torch_bf16(v.y) << 16);
                    p[2 * q + 1] = torch_bf16(v.z) | (torch_bf16(v.w) << 16);
                }
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const float2 v = reinterpret_cast<const float2*>(r)[q];
                    p[q] = torch_bf16(v.x) | (torch_bf16(v.y) << 16);
                }
            }
        } else {
            const bf16_t* r = static_cast<const bf16_t*>(d.src) + (size_t)s * d.src_ld + c0;
            if (vec == 16) {
                const uint4 a = reinterpret_cast<const uint4*>(r)[0], b = reinterpret_cast<const uint4*>(r)[1];
                p[0] = a.x, p[1] = a.y, p[2] = a.z, p[3] = a.w, p[4] = b.x, p[5] = b.y, p[6] = b.z, p[7] = b.w;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint2 v = reinterpret_cast<const uint2*>(r)[q];
                    p[2 * q] = v.x, p[2 * q + 1] = v.y;
                }
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int c = c0 + j;
        const int sc = d.col_map ? d.col_map[c] : (c < d.src_cols ? c : -1);
        uint32_t b = 0u;
        if (sc >= 0) {
            if constexpr (F32)
                b = torch_bf16(static_cast<const float*>(d.src)[(size_t)s * d.src_ld + sc]);
            else
                b = static_cast<const bf16_t*>(d.src)[(size_t)s * d.src_ld + sc];
        }
        p[j >> 1] |= b << (16 * (j & 1));
    }
}

__device__ __forceinline__ void st16(void* dst, uint32_t a, uint32_t b, uint32_t c, uint32_t e) {
    u32x4 v = {a, b, c, e};
    __builtin_nontemporal_store(v, static_cast<u32x4*>(dst));   // written once, never read by this launch
}

__device__ __forceinline__ void st8(void* dst, uint32_t a, uint32_t b) {
    u32x2 v = {a, b};
    __builtin_nontemporal_store(v, static_cast<u32x2*>(dst));
}

template <bool F32, bool FP8, bool FP4>
__global__ __launch_bounds__(256) void repack_rows_kernel(const o3v_repack_desc d, const int vec) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, sub = lane >> 4;
    const int i = blockIdx.x;
    const int blk = d.blk0 + i * d.blk_stride;
    const int row = blk * 16 + r;
    const bool row_ok = row < d.rows;
    int s = d.row_map ? d.row_map[i * 16 + r] : i * 16 + r;
    if (s >= d.src_rows) s = -1;
    const int groups = d.cols >> 4;            // 16-column units per row
    const int tgroups = (groups + 3) >> 2;     // 64-column groups

    float inv = 1.0f;
    if constexpr (FP8) {
        __shared__ float s_amax[4][16];
        float amax = 0.f;
        if (row_ok) {
            for (int t = wave; t < tgroups; t += 4) {
                const int g = 4 * t + sub;
                if (g >= groups) continue;
                uint32_t p[8];
                load16<F32>(d, vec, s, 16 * g, p);
#pragma unroll
                for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fmaxf(fabsf(bf_lo(p[j])), fabsf(bf_hi(p[j]))));
            }
        }
        amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
        amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
        if (lane < 16) s_amax[wave][lane] = amax;
        __syncthreads();
        amax = fmaxf(fmaxf(s_amax[0][r], s_amax[1][r]), fmaxf(s_amax[2][r], s_amax[3][r]));
        const float sc = pow2_scale_for(amax);
        inv = 1.0f / sc;
        if (wave == 0 && lane < 16 && row_ok) d.dst8_scale[row] = sc;
    }
    if (!row_ok) return;

    bf16_t* dst = static_cast<bf16_t*>(d.dst);
    bf16_t* frag = static_cast<bf16_t*>(d.dst_frag);
    uint8_t* q8 = static_cast<uint8_t*>(d.dst8);
    uint8_t* q8f = static_cast<uint8_t*>(d.dst8_frag);
    const size_t blk_base = (size_t)blk * 16 * d.cols;   // a block's fragment images start where its row-major rows do
    for (int t = wave; t < tgroups; t += 4) {
        const int g = 4 * t + sub;
        if (g >= groups) continue;
        const int c0 = 16 * g;
        uint32_t p[8];
        load16<F32>(d, vec, s, c0, p);
        bf16_t* o = dst + (size_t)row * d.cols + c0;
        st16(o, p[0], p[1], p[2], p[3]);
        st16(o + 8, p[4], p[5], p[6], p[7]);
        if (frag) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {   // 8-column chunk c8 = 2g + h: k-step c8 / 4, fragment lane r + 16 (c8 % 4)
                const int c8 = 2 * g + h;
                st16(frag + blk_base + ((size_t)(c8 >> 2) * 64 + r + 16 * (c8 & 3)) * 8, p[4 * h], p[4 * h + 1], p[4 * h + 2],
                     p[4 * h + 3]);
            }
        }
        if constexpr (FP8) {
            float ya[8], yb[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ya[2 * j] = bf_lo(p[j]), ya[2 * j + 1] = bf_hi(p[j]);
                yb[2 * j] = bf_lo(p[4 + j]), yb[2 * j + 1] = bf_hi(p[4 + j]);
            }
            const uint2 a = pack8_fp8(ya, inv), b = pack8_fp8(yb, inv);
            st16(q8 + (size_t)row * d.cols + c0, a.x, a.y, b.x, b.y);
            if (q8f) st16(q8f + blk_base + ((size_t)t * 64 + lane) * 16, a.x, a.y, b.x, b.y);   // 64-wide step t, lane r + 16 sub
        }
        if constexpr (FP4) {
            // MX block b32 = 2 t + (sub >> 1) of the row: this lane's 16 columns are its half (sub & 1)
            uint32_t amax = 0u;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t a = mx4_amax2(p[j]);
                amax = a > amax ? a : amax;
            }
            const uint32_t other = (uint32_t)__shfl_xor((int)amax, 16, 64);
            amax = other > amax ? other : amax;
            const uint32_t code = mx4_scale_code(amax);
            const float inv4 = mx4_inv_scale(code);
            const uint32_t lo = mx4_codes4(p[0], p[1], inv4) | (mx4_codes4(p[2], p[3], inv4) << 16);
            const uint32_t hi = mx4_codes4(p[4], p[5], inv4) | (mx4_codes4(p[6], p[7], inv4) << 16);
            const int b32 = 2 * t + (sub >> 1), half = sub & 1, nb32 = d.cols >> 5;
            st8(static_cast<uint8_t*>(d.dst4) + ((size_t)row * nb32 + b32) * 16 + half * 8, lo, hi);
            if (!half) static_cast<uint8_t*>(d.dst4_scale)[(size_t)row * nb32 + b32] = (uint8_t)code;
            if (d.dst4_frag) {   // 128-wide step b32 / 4, fragment lane r + 16 (b32 % 4)
                const int st = b32 >> 2, fl = r + 16 * (b32 & 3), nt = d.cols >> 7, nt4 = (nt + 3) >> 2;
                st8(static_cast<uint8_t*>(d.dst4_frag) + (((size_t)blk * nt + st) * 64 + fl) * 16 + half * 8, lo, hi);
                if (!half) static_cast<uint8_t*>(d.dst4_frag_scale)[(((size_t)blk * nt4 + (st >> 2)) * 64 + fl) * 4 + (st & 3)] = (uint8_t)code;
            }
        }
    }
}

}  // namespace

extern "C" int o3v_repack_rows(const o3v_repack_desc* d, hipStream_t stream) {
    if (!d || !d->src || !d->dst || (d->src_dtype != O3V_SRC_BF16 && d->src_dtype != O3V_SRC_F32)) return O3V_ERR_ARG;
    if (d->rows <= 0 || d->cols <= 0 || d->src_rows < 0 || d->src_cols < 0 || d->src_ld < d->src_cols || d->nblk < 0 ||
        d->blk0 < 0 || d->blk_stride < 1)
        return O3V_ERR_ARG;
    if (d->nblk == 0) return O3V_OK;
    if ((int64_t)(d->blk0 + (int64_t)(d->nblk - 1) * d->blk_stride) * 16 >= d->rows) return O3V_ERR_ARG;
    if (d->dst8 && !d->dst8_scale) return O3V_ERR_ARG;
    if (d->dst8_frag && !d->dst8) return O3V_ERR_ARG;
    auto mis16 = [](const void* p) { return ((uintptr_t)p & 15) != 0; };
    if (mis16(d->dst) || mis16(d->dst_frag) || mis16(d->dst8) || mis16(d->dst8_frag)) return O3V_ERR_ARG;
    if (d->cols & 15) return O3V_ERR_SHAPE;
    if (d->dst4 && !d->dst4_scale) return O3V_ERR_ARG;
    if (d->dst4_frag && (!d->dst4 || !d->dst4_frag_scale)) return O3V_ERR_ARG;
    if (mis16(d->dst4) || mis16(d->dst4_frag) || ((uintptr_t)d->dst4_frag_scale & 3)) return O3V_ERR_ARG;
    if (d->dst4 && (d->cols & 31)) return O3V_ERR_SHAPE;
    if (d->dst4_frag && ((d->rows & 15) || (d->cols & 127))) return O3V_ERR_SHAPE;
    if (d->dst_frag && ((d->rows & 15) || (d->cols & 31))) return O3V_ERR_SHAPE;
    if (d->dst8_frag && ((d->rows & 15) || (d->cols & 63))) return O3V_ERR_SHAPE;
    const int esize = d->src_dtype == O3V_SRC_F32 ? 4 : 2;
    const uintptr_t pitch = (uintptr_t)d->src | (uintptr_t)(d->src_ld * esize);   // alignment every source row start shares
    const int vec = (pitch & 15) == 0 ? 16 : (pitch & 7) == 0 ? 8 : 0;
    const dim3 grid(d->nblk), block(256);
#define O3V_RP(F, Q, Q4) O3V_KLAUNCH((repack_rows_kernel<F, Q, Q4>), grid, block, 0, stream, *d, vec)
#define O3V_RPQ(F)                                \
    do {                                          \
        if (d->dst8 && d->dst4) O3V_RP(F, true, true);   \
        else if (d->dst8) O3V_RP(F, true, false);  \
        else if (d->dst4) O3V_RP(F, false, true);  \
        else O3V_RP(F, false, false);              \
    } while (0)
    if (d->src_dtype == O3V_SRC_F32)
        O3V_RPQ(true);
    else
        O3V_RPQ(false);
#undef O3V_RPQ
#undef O3V_RP
    O3V_CHECK_LAUNCH();
    return O3V_OK;
}
