// LoRA merge (DeviceWeights.load_adapter): out[n][k] = bf16( fp32(base[row(n)][k]) + scale * sum_j B[n][j] * A[j][k] ), one launch per
// adapted matrix.  The base is read where the packed bf16 row image keeps it (row(n) = 16 (blk0 + (n / 16) blk_stride) + n % 16: q / k / v
// inside qkv_w, the 16-row gate / up interleave of gu_w, padded columns through base_ld); the merged matrix goes to a plain bf16
// staging tensor that o3v_repack_rows then packs into the adapter's images.
//
// Memory-bound: 2 bytes read and 2 written per element, A and B are tiny.  A workgroup (4 waves) owns a stripe of 64 or 128 columns
// and a run of 8..32 16-row blocks.  It stages its stripe of A once, transposed and zero-padded to rpad = pad32(r), in LDS
// ([column][rpad + 8] bf16: the + 8 keeps the 16-byte fragment reads of neighbouring columns on different banks).  A wave then takes
// row blocks wave, wave + 4, ...: it loads the block's B fragments once (8 bf16 per lane and 32-wide r step, straight from global
// memory), and per 64-column group each lane loads its 16 base columns (two 16-byte loads, lane l: row l & 15, columns 16 (l >> 4) ..),
// runs 4 MFMA 16x16x32 per r step and stores two 16-byte chunks.
//
// The product is computed transposed (D[column][row] = sum_j A^T[column][j] B^T[j][row]) so that the accumulator registers of a
// lane are consecutive COLUMNS of one row: with the C/D map (col = lane & 15, row = 4 (lane >> 4) + reg) and MFMA row i of tile q
// standing for stripe column 16 (i >> 2) + 4 q + (i & 3), lane l's registers of tiles 0..3 are columns 16 (l >> 4) + 0..15 of row
// l & 15 -- exactly the 32 bytes it loaded.  fp32 accumulation; scale and the base addition in fp32 (a multiply, then an add, as
// torch evaluates W + s * (B @ A)); one rounding to bf16 at the end with torch's rule.
#include <hip/hip_runtime.h>

#include "../../include/o3v.h"
#include "o3v_common.h"

namespace {

constexpr int LORA_MAX_STEPS = O3V_LORA_MAX_RANK / 32;   // 32-wide r steps

// 8 consecutive elements p[0..7] of a bf16 / fp32 row as an MFMA fragment; elements at or past `n` are zero.  vec: 16-byte loads
// are allowed (aligned row start, index a multiple of 8)
template <bool F32>
__device__ __forceinline__ bf16x8 load8(const void* row, int j0, int n, bool vec) {
    bf16x8 f = {0, 0, 0, 0, 0, 0, 0, 0};
    if (j0 >= n) return f;
    if (vec && j0 + 8 <= n) {
        if constexpr (F32) {
            const float4 a = reinterpret_cast<const float4*>(static_cast<const float*>(row) + j0)[0];
            const float4 b = reinterpret_cast<const float4*>(static_cast<const float*>(row) + j0)[1];
            f[0] = (short)torch_bf16(a.x), f[1] = (short)torch_bf16(a.y), f[2] = (short)torch_bf16(a.z), f[3] = (short)torch_bf16(a.w);
            f[4] = (short)torch_bf16(b.x), f[5] = (short)torch_bf16(b.y), f[6] = (short)torch_bf16(b.z), f[7] = (short)torch_bf16(b.w);
        } else {
            f = *reinterpret_cast<const bf16x8*>(static_cast<const bf16_t*>(row) + j0);
        }
        return f;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if (j0 + e < n) {
            if constexpr (F32)
                f[e] = (short)torch_bf16(static_cast<const float*>(row)[j0 + e]);
            else
                f[e] = (short)static_cast<const bf16_t*>(row)[j0 + e];
        }
    }
    return f;
}

// kc: 64-column groups per stripe (1 or 2); bpw: 16-row blocks per workgroup; dynamic LDS: 64 kc (rpad + 8) bf16
template <bool F32>
__global__ __launch_bounds__(256) void lora_merge_kernel(const o3v_lora_desc d, const int rpad, const int kc, const int bpw, const int vecb) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lora_smem[];
    bf16_t* sA = reinterpret_cast<bf16_t*>(lora_smem);
    const int P = rpad + 8;                       // LDS pitch of a stripe column, bf16 elements (16-byte multiple)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int kcols = 64 * kc;
    const int col0 = blockIdx.x * kcols;          // first column of the stripe
    const int nsteps = rpad >> 5;

    // ---- stage A^T: sA[c][j] = A[j][col0 + c], zeros for j >= r and columns >= K.  A thread takes 8 columns of the row pair
    // (j, j + 1) (16-byte loads; K % 8 == 0, so a chunk is inside or outside as a whole) and stores 8 dwords {A[j][c], A[j + 1][c]};
    // neighbouring lanes take neighbouring row pairs of the same columns, so one store instruction fills consecutive dwords
    const int chunks = kcols >> 3, pairs = rpad >> 1;
    for (int idx = threadIdx.x; idx < pairs * chunks; idx += 256) {
        const int ci = idx / pairs, c8 = ci * 8, j = (idx - ci * pairs) * 2;
        bf16x8 v0 = {0, 0, 0, 0, 0, 0, 0, 0}, v1 = v0;
        if (col0 + c8 < d.K) {
            const size_t esz = F32 ? 4 : 2;
            const char* a0 = static_cast<const char*>(d.A) + (size_t)j * d.a_ld * esz;
            if (j < d.r) v0 = load8<F32>(a0, col0 + c8, d.K, true);
            if (j + 1 < d.r) v1 = load8<F32>(a0 + (size_t)d.a_ld * esz, col0 + c8, d.K, true);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e)
            *reinterpret_cast<uint32_t*>(sA + (c8 + e) * P + j) = (uint32_t)(uint16_t)v0[e] | ((uint32_t)(uint16_t)v1[e] << 16);
    }
    __syncthreads();

    const int nblocks = d.N >> 4;
    const int nb_end = min(nblocks, (int)(blockIdx.y + 1) * bpw);
    const bf16_t* base = static_cast<const bf16_t*>(d.base);
    bf16_t* out = static_cast<bf16_t*>(d.out);
    for (int nb = blockIdx.y * bpw + wave; nb < nb_end; nb += 4) {    // wave-uniform: every MFMA runs with all lanes on
        const int n = nb * 16 + r16;
        const size_t brow = (size_t)16 * (d.blk0 + (size_t)nb * d.blk_stride) + r16;
        // every global load of the block is issued before the first use: the base words of both column groups, then B
        u32x4 w[2][2];
#pragma unroll
        for (int cg = 0; cg < 2; ++cg) {
            const int c = col0 + cg * 64 + g * 16;
            w[cg][0] = w[cg][1] = (u32x4){0u, 0u, 0u, 0u};
            if (cg < kc && c < d.K) w[cg][0] = *reinterpret_cast<const u32x4*>(base + brow * d.base_ld + c);
            if (cg < kc && c + 8 < d.K) w[cg][1] = *reinterpret_cast<const u32x4*>(base + brow * d.base_ld + c + 8);
        }
        bf16x8 bfr[LORA_MAX_STEPS];
        {
            const void* brp = F32 ? static_cast<const void*>(static_cast<const float*>(d.B) + (size_t)n * d.b_ld)
                                  : static_cast<const void*>(static_cast<const bf16_t*>(d.B) + (size_t)n * d.b_ld);
#pragma unroll
            for (int s = 0; s < LORA_MAX_STEPS; ++s)
                if (s < nsteps) bfr[s] = load8<F32>(brp, s * 32 + 8 * g, d.r, vecb != 0);
        }
#pragma unroll
        for (int cg = 0; cg < 2; ++cg) {
            if (cg >= kc) break;                   // wave-uniform
            const int c = col0 + cg * 64 + g * 16;   // this lane's 16 columns
            const bool ok0 = c < d.K, ok1 = c + 8 < d.K;
            const u32x4 w0 = w[cg][0], w1 = w[cg][1];
            f32x4 acc[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < LORA_MAX_STEPS; ++s) {
                if (s < nsteps) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        // MFMA row i = r16 of tile q is stripe column cg * 64 + 16 (i >> 2) + 4 q + (i & 3); k = 32 s + 8 g + 0..7
                        const int ac = cg * 64 + 16 * (r16 >> 2) + 4 * q + (r16 & 3);
                        const bf16x8 af = *reinterpret_cast<const bf16x8*>(sA + ac * P + s * 32 + 8 * g);
                        acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr[s], acc[q], 0, 0, 0);
                    }
                }
            }
            u32x4 o0, o1;
#pragma unroll
            for (int h = 0; h < 2; ++h) {          // 32-bit word h of tile q: its registers 2h, 2h + 1
                o0[h] = torch_bf16(__fadd_rn(bf_lo(w0[h]), __fmul_rn(d.scale, acc[0][2 * h]))) |
                        (torch_bf16(__fadd_rn(bf_hi(w0[h]), __fmul_rn(d.scale, acc[0][2 * h + 1]))) << 16);
                o0[2 + h] = torch_bf16(__fadd_rn(bf_lo(w0[2 + h]), __fmul_rn(d.scale, acc[1][2 * h]))) |
                            (torch_bf16(__fadd_rn(bf_hi(w0[2 + h]), __fmul_rn(d.scale, acc[1][2 * h + 1]))) << 16);
                o1[h] = torch_bf16(__fadd_rn(bf_lo(w1[h]), __fmul_rn(d.scale, acc[2][2 * h]))) |
                        (torch_bf16(__fadd_rn(bf_hi(w1[h]), __fmul_rn(d.scale, acc[2][2 * h + 1]))) << 16);
                o1[2 + h] = torch_bf16(__fadd_rn(bf_lo(w1[2 + h]), __fmul_rn(d.scale, acc[3][2 * h]))) |
                            (torch_bf16(__fadd_rn(bf_hi(w1[2 + h]), __fmul_rn(d.scale, acc[3][2 * h + 1]))) << 16);
            }
            if (ok0) *reinterpret_cast<u32x4*>(out + (size_t)n * d.out_ld + c) = o0;
            if (ok1) *reinterpret_cast<u32x4*>(out + (size_t)n * d.out_ld + c + 8) = o1;
        }
    }
}

}  // namespace

extern "C" int o3v_lora_merge(const o3v_lora_desc* d, hipStream_t stream) {
    if (!d || !d->base || !d->A || !d->B || !d->out || (d->ab_dtype != O3V_SRC_BF16 && d->ab_dtype != O3V_SRC_F32)) return O3V_ERR_ARG;
    if (d->N <= 0 || d->K <= 0 || d->r < 1 || d->blk0 < 0 || d->blk_stride < 1 || d->base_rows <= 0) return O3V_ERR_ARG;
    if (d->base_ld < d->K || d->out_ld < d->K || d->a_ld < d->K || d->b_ld < d->r) return O3V_ERR_ARG;
    if (!(d->scale == d->scale) || d->scale - d->scale != 0.f) return O3V_ERR_ARG;   // NaN / infinity
    if (d->r > O3V_LORA_MAX_RANK || (d->N & 15) || (d->K & 7)) return O3V_ERR_SHAPE;
    // the last 16-row block read must lie inside the base image
    if (((int64_t)d->blk0 + (int64_t)(d->N / 16 - 1) * d->blk_stride) * 16 + 16 > (int64_t)d->base_rows) return O3V_ERR_ARG;
    const int esize = d->ab_dtype == O3V_SRC_F32 ? 4 : 2;
    auto mis16 = [](uintptr_t p) { return (p & 15) != 0; };
    if (mis16((uintptr_t)d->base) || mis16((uintptr_t)d->out) || mis16((uintptr_t)d->A) || mis16((uintptr_t)d->B)) return O3V_ERR_ARG;
    if (mis16((uintptr_t)(d->base_ld * 2)) || mis16((uintptr_t)(d->out_ld * 2)) || mis16((uintptr_t)(d->a_ld * esize))) return O3V_ERR_SHAPE;
    const int vecb = !mis16((uintptr_t)(d->b_ld * esize));       // B rows of an odd rank are read element by element
    const int rpad = (d->r + 31) & ~31;
    const int kc = (d->K > 64 && 128 * (rpad + 8) * 2 <= 48 * 1024) ? 2 : 1;
    const size_t lds = (size_t)64 * kc * (rpad + 8) * 2;
    const int nblocks = d->N / 16, gx = (d->K + 64 * kc - 1) / (64 * kc);
    int bpw = (int)(((int64_t)nblocks * gx) / 1024);             // aim at a few workgroups per CU, A staged once per 8..32 blocks
    bpw = bpw < 8 ? 8 : (bpw > 32 ? 32 : bpw);
    const dim3 grid(gx, (nblocks + bpw - 1) / bpw), block(256);
    if (d->ab_dtype == O3V_SRC_F32)
        O3V_KLAUNCH((lora_merge_kernel<true>), grid, block, lds, stream, *d, rpad, kc, bpw, vecb);
    else
        O3V_KLAUNCH((lora_merge_kernel<false>), grid, block, lds, stream, *d, rpad, kc, bpw, vecb);
    O3V_CHECK_LAUNCH();
    return O3V_OK;
}
