// Decode MLP linears on MXFP4 weights (OCP MX v1.0: e2m1 codes, one e8m0 scale per 32 k -- o3v_mxfp4.h), opt-in
// (DeviceWeights(mxfp4_decode=True)): the weight stream that bounds a decode step at a quarter of the bf16 bytes plus 1/32 for the
// scales.  The design is the fp8 rows': gfx950 widens packed fp4 to bf16 in one instruction with the block scale applied
// (v_cvt_scalef32_pk_bf16_fp4) and the result is EXACT -- an e2m1 value has one mantissa bit, the scale is a power of two and the
// quantiser's clamp keeps the product a normal bf16 -- so the widened weights meet bf16 activations in the arithmetic of the bf16
// path (v_dot2c_f32_bf16 / v_mfma_f32_16x16x32_bf16, fp32 accumulation, the same rounding points and epilogues).  Run on weights
// that are MXFP4-representable, the bf16 kernels and these differ by summation order only.
//
//   o3v_linear_decode_mxfp4        M <= 3 rows: the weight-streaming GEMV body (o3v_gemv_body.h, WB = 0) on row-major codes + scales
//   o3v_linear_decode_mxfp4_rows   4 <= M <= 32 rows of normalised x: the skinny matrix-core GEMM on the fragment-major image
//   o3v_quantize_rows_mxfp4        bf16 rows -> codes + scales (weights.quantize_rows_mxfp4 bit for bit)
#include "../../include/o3v.h"
#include "o3v_common.h"
#include "o3v_gemv_body.h"
#include "o3v_mxfp4.h"

namespace {

template <int M, int R, int KS, int EPI, bool NORM, int NW, int UU>
__global__ __launch_bounds__(NW * 64) void gemv_mxfp4_kernel(const bf16_t* __restrict__ X, const uint8_t* __restrict__ W4,
                                                             const uint8_t* __restrict__ S4, const bf16_t* __restrict__ bias,
                                                             const bf16_t* __restrict__ res, bf16_t* __restrict__ out,
                                                             const bf16_t* __restrict__ norm_w, float eps, int N, int K, int ldx, int ldo,
                                                             int ldr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [NORM: M*K bf16] [KS>1: NW*R*M f32] [NORM: 4*M f32]
    gemv_body<M, R, KS, EPI, NORM, false, UU, NW, 0>(X, reinterpret_cast<const bf16_t*>(W4), bias, res, out, norm_w, eps, N, K, ldx, K, ldo,
                                                    ldr, RopeArgs{}, blockIdx.x, smem, nullptr, S4);
}

struct G4Args {
    const bf16_t *X, *bias, *res, *norm_w;
    const uint8_t *W4, *S4;
    bf16_t* out;
    float eps;
    int N, K, ldx, ldo, ldr, epi;
    hipStream_t s;
};

template <int M, int R, int KS, bool NORM, int NW, int UU = 0>
int launch_g4(const G4Args& a) {
    const int per_wave = a.epi == EPI_SWIGLU ? R / 2 : R;
    const int outs = a.epi == EPI_SWIGLU ? a.N / 2 : a.N;
    const int per_block = per_wave * (NW / KS);
    const dim3 grid((outs + per_block - 1) / per_block), block(NW * 64);
    const size_t shmem = (NORM ? (size_t)M * a.K * 2 : 0) + (size_t)NW * R * M * 4 + (NORM ? 4 * M * 4 : 0);
    if (shmem > 160 * 1024) return O3V_ERR_SHAPE;
#define O3V_G4(E)                                                                                                                     \
    O3V_KLAUNCH((gemv_mxfp4_kernel<M, R, KS, E, NORM, NW, UU>), grid, block, shmem, a.s, a.X, a.W4, a.S4, a.bias, a.res, a.out, a.norm_w, a.eps, \
                a.N, a.K, a.ldx, a.ldo, a.ldr)
    switch (a.epi) {
        case EPI_NONE: O3V_G4(EPI_NONE); break;
        case EPI_RESIDUAL: O3V_G4(EPI_RESIDUAL); break;
        case EPI_SWIGLU: O3V_G4(EPI_SWIGLU); break;
        default: return O3V_ERR_ARG;
    }
#undef O3V_G4
    return O3V_OK;
}

// Decomposition, chosen by A/B at the 7B shapes (profiles/mxfp4_cost.txt has the times of the chosen forms).  A lane's step is one MX
// block (16 bytes of codes, 64 bytes of x), so at the row lengths of the MLP a wave has few steps (hidden 3584: 112 blocks, two steps
// of 64 lanes) and little to keep in flight along k: the bytes in flight come from the rows of a wave and the waves of a CU instead.
//   gate/up   one row of x: four (gate, up) pairs per wave, one step per trip (20.8 us; two pairs x two steps 22.0, eight pairs 35);
//             two rows: two pairs per wave, as the fp8 rows
//   long k    (down_proj: >= 256 blocks per row) one row of x and a grid of 7 waves per CU: one workgroup of 7 waves per CU, whole
//             rows per wave (11.6 us); else two K slices per row pair (14 waves per CU where that is whole: 12.9 us)
// What bounds them is not the stream: 72 MB in 20.8 us is 3.5 TB/s where the fp8 rows reach 5.1.  Every workgroup normalises x again
// and lives for two or three memory latencies, and at half the bytes per workgroup those fixed costs weigh twice as much.
#ifdef O3V_TUNE
int g_t4[4] = {0, 0, 0, 0}, g_t4r[3] = {0, 0, 0};  // tuning build only: force one decomposition (R, KS, NW, U) / (KS, waves, U)
#endif

template <int M, bool NORM>
int launch_g4_m(const G4Args& a) {
    const int outs = a.epi == EPI_SWIGLU ? a.N / 2 : a.N;
#ifdef O3V_TUNE
    if (g_t4[0]) {
        if constexpr (M == 1) {
#define O3V_T4(RR, KK, NN, UV) \
    if (g_t4[0] == RR && g_t4[1] == KK && g_t4[2] == NN && g_t4[3] == UV) return launch_g4<M, RR, KK, NORM, NN, UV>(a)
            if constexpr (NORM) {  // gate/up
                O3V_T4(4, 1, 4, 2); O3V_T4(8, 1, 4, 2); O3V_T4(8, 1, 4, 1); O3V_T4(4, 1, 8, 2); O3V_T4(8, 1, 8, 2); O3V_T4(4, 1, 2, 2);
                O3V_T4(2, 1, 4, 2); O3V_T4(16, 1, 4, 1); O3V_T4(8, 1, 2, 2);
            } else {  // down_proj
                O3V_T4(2, 2, 14, 2); O3V_T4(2, 2, 14, 1); O3V_T4(2, 2, 14, 4); O3V_T4(4, 4, 16, 2); O3V_T4(2, 1, 7, 2); O3V_T4(2, 1, 7, 4);
                O3V_T4(4, 2, 4, 2); O3V_T4(2, 2, 4, 2); O3V_T4(4, 2, 8, 2); O3V_T4(2, 4, 8, 2); O3V_T4(4, 4, 8, 2);
            }
#undef O3V_T4
        }
        return O3V_ERR_ARG;
    }
#endif
    if (a.epi == EPI_SWIGLU) {
        if (M == 1 && outs >= 8192) return launch_g4<M, 8, 1, NORM, 4, 1>(a);
        if (M <= 2 && outs >= 8192) return launch_g4<M, 4, 1, NORM, 4>(a);
        return launch_g4<M, 2, 1, NORM, 4>(a);
    }
    if ((a.K >> 5) >= 256) {
        if constexpr (M == 1) {
            const int pairs = (a.N + 1) / 2;  // waves per K slice
            if (pairs % 256 == 0 && pairs / 256 == 7) return launch_g4<M, 2, 1, NORM, 7, 2>(a);
            if ((2 * pairs) % 256 == 0 && (2 * pairs) / 256 == 14) return launch_g4<M, 2, 2, NORM, 14>(a);
        }
        return launch_g4<M, 2, 2, NORM, 4>(a);
    }
    return launch_g4<M, 2, 1, NORM, 4>(a);
}

// ------------------------------------------------------------------------------------------------
// 4..32 rows of already normalised x: gemv_mfma_fp8_kernel's skinny GEMM on the fragment-major MXFP4 image
//   W4p  [N/16][K/128][64 lanes][16 B]: lane (row = lane & 15, g = lane >> 4) of (row block, 128-wide step t) holds the MX block
//        W[row][128 t + 32 g .. + 32) -- one contiguous KiB per wave-instruction (weights.pack_mfma_fragments_mxfp4)
//   S4p  [N/16][ceil(K/512)][64 lanes][4 B]: the same lane's scale bytes of steps 4 q .. 4 q + 3, so a lane fetches a dword per
//        four steps (bytes of steps past K/128 are padding)
// Dword j of a lane's block widens to one bf16x8 A fragment (k = 128 t + 32 g + 8 j .. + 8); its B fragment is x[m][the same k] --
// the k order differs from the bf16 kernel's, the set does not.  Four MFMAs per block and column block.
// ------------------------------------------------------------------------------------------------
template <int EPI, int KS, int CB, int NWV = 4, int UT = 0>
__global__ __launch_bounds__(NWV * 64) void gemv_mfma_mxfp4_kernel(const bf16_t* __restrict__ X, const uint8_t* __restrict__ W4p,
                                                              const uint8_t* __restrict__ S4p, const bf16_t* __restrict__ bias,
                                                              const bf16_t* __restrict__ res, bf16_t* __restrict__ out, int M, int N, int K,
                                                              int ldx, int ldo, int ldr) {
    constexpr int RB = EPI == EPI_SWIGLU ? 2 : 1;
    constexpr int RG = NWV / KS;
    // steps per trip (UT, the launcher's choice): a step pairs 16 bytes of weights with 64 bytes of x per lane and column block, so
    // the x fragments (16 VGPRs per step, column block and buffer) bound the trip, and with them the waves a SIMD holds: four steps
    // per trip measured 40 us on gate/up at 8 rows where one step takes 20-22 (the register file, not the stream, was the limit)
    constexpr int U = UT > 0 ? UT : 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [KS > 1: NWV x RB x CB x 64 x 4 f32]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int rg = wave / KS, ks = wave % KS;
    const int grp = blockIdx.x * RG + rg;
    int rb0[RB];
    if (EPI == EPI_SWIGLU) {
        rb0[0] = grp * 32;
        rb0[RB - 1] = grp * 32 + 16;
    } else {
        rb0[0] = grp * 16;
    }
    const int nt = K >> 7;         // 128-wide steps
    const int nt4 = (nt + 3) >> 2;  // scale dwords per lane and row block
    const u32x4* wrow[RB];
    const uint32_t* srow[RB];
#pragma unroll
    for (int b = 0; b < RB; ++b) {
        const int blk = (rb0[b] < N ? rb0[b] : 0) >> 4;
        wrow[b] = reinterpret_cast<const u32x4*>(W4p) + (size_t)blk * nt * 64 + lane;
        srow[b] = reinterpret_cast<const uint32_t*>(S4p) + (size_t)blk * nt4 * 64 + lane;
    }
    const int per = (nt + KS - 1) / KS;
    const int t_begin = ks * per;
    int t_end = t_begin + per;
    t_end = t_end < nt ? t_end : nt;

    float e_bias[RB][4], e_res[CB][4];
#pragma unroll
    for (int b = 0; b < RB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int n = rb0[b] + fg * 4 + r;
            n = n < N ? n : N - 1;
            e_bias[b][r] = bias ? bf2f(bias[n]) : 0.f;
        }
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
        const int m = fr + 16 * cb < M ? fr + 16 * cb : 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int n = rb0[0] + fg * 4 + r;
            n = n < N ? n : N - 1;
            e_res[cb][r] = (EPI == EPI_RESIDUAL) ? bf2f(res[(size_t)m * ldr + n]) : 0.f;
        }
    }
    f32x4 acc[RB][CB];
#pragma unroll
    for (int b = 0; b < RB; ++b)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) acc[b][cb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    u32x4 wf0[U][RB], wf1[U][RB];
    uint32_t sf0[U][RB], sf1[U][RB];
    bf16x8 xf0[U][CB][4], xf1[U][CB][4];
    auto load_w = [&](u32x4 (&wf)[U][RB], uint32_t (&sf)[U][RB], bf16x8 (&xf)[U][CB][4], int t0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = t0 + u;
            if (t < t_end) {  // wave-uniform
#pragma unroll
                for (int b = 0; b < RB; ++b) {
                    wf[u][b] = __builtin_nontemporal_load(wrow[b] + (size_t)t * 64);
                    sf[u][b] = (srow[b][(size_t)(t >> 2) * 64] >> (8 * (t & 3))) & 0xffu;
                }
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) {
                    const bool has = fr + 16 * cb < M;
                    const bf16_t* xp = X + (size_t)(fr + 16 * cb) * ldx + t * 128 + fg * 32;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        xf[u][cb][j] = has ? *reinterpret_cast<const bf16x8*>(xp + 8 * j) : (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
                }
            } else {
#pragma unroll
                for (int b = 0; b < RB; ++b) {
                    wf[u][b] = (u32x4){0u, 0u, 0u, 0u};  // code 0 widens to 0.0 under any scale
                    sf[u][b] = 127u;
                }
#pragma unroll
                for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                    for (int j = 0; j < 4; ++j) xf[u][cb][j] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
            }
        }
    };
    auto widen = [](uint32_t w, float sc) -> bf16x8 {  // 8 e2m1 codes of one dword -> 8 bf16, k order preserved, block scale applied
        const bf16x2_t a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 0), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 1);
        const bf16x2_t c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 2), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 3);
        const u32x4 p = {__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b), __builtin_bit_cast(uint32_t, c),
                         __builtin_bit_cast(uint32_t, d)};
        return __builtin_bit_cast(bf16x8, p);
    };
    auto compute = [&](u32x4 (&wf)[U][RB], uint32_t (&sf)[U][RB], bf16x8 (&xf)[U][CB][4]) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int b = 0; b < RB; ++b) {
                const float sc = mx4_scale(sf[u][b]);
                const uint32_t w0 = wf[u][b][0], w1 = wf[u][b][1], w2 = wf[u][b][2], w3 = wf[u][b][3];
                const bf16x8 a0 = widen(w0, sc), a1 = widen(w1, sc), a2 = widen(w2, sc), a3 = widen(w3, sc);
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) {
                    acc[b][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, xf[u][cb][0], acc[b][cb], 0, 0, 0);
                    acc[b][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, xf[u][cb][1], acc[b][cb], 0, 0, 0);
                    acc[b][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, xf[u][cb][2], acc[b][cb], 0, 0, 0);
                    acc[b][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a3, xf[u][cb][3], acc[b][cb], 0, 0, 0);
                }
            }
    };
    load_w(wf0, sf0, xf0, t_begin);
    for (int t0 = t_begin; t0 < t_end; t0 += 2 * U) {
        load_w(wf1, sf1, xf1, t0 + U);
        compute(wf0, sf0, xf0);
        load_w(wf0, sf0, xf0, t0 + 2 * U);
        compute(wf1, sf1, xf1);
    }
    if (KS > 1) {
        f32x4* part = reinterpret_cast<f32x4*>(smem);
#pragma unroll
        for (int b = 0; b < RB; ++b)
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) part[((wave * RB + b) * CB + cb) * 64 + lane] = acc[b][cb];
        __syncthreads();
        if (ks != 0) return;
#pragma unroll
        for (int b = 0; b < RB; ++b)
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                f32x4 t = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k2 = 0; k2 < KS; ++k2) t += part[(((rg * KS + k2) * RB + b) * CB + cb) * 64 + lane];
                acc[b][cb] = t;
            }
    }
    // ---- epilogue: this lane holds C[n = rb0 + 4*fg + r][m = fr + 16 cb] (no row scale: the block scales went in at the widening)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
        const int m = fr + 16 * cb;
        if (m >= M) continue;
        if (EPI == EPI_SWIGLU) {
            const int no0 = grp * 16 + fg * 4;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int no = no0 + r;
                if (no >= (N >> 1)) continue;
                const float g = rbf(acc[0][cb][r] + e_bias[0][r]);
                const float u = rbf(acc[RB - 1][cb][r] + e_bias[RB - 1][r]);
                out[(size_t)m * ldo + no] = f2bf(rbf(silu_f(g)) * u);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = rb0[0] + fg * 4 + r;
                if (n >= N) continue;
                float v = acc[0][cb][r] + e_bias[0][r];
                if (EPI == EPI_RESIDUAL) v = rbf(v) + e_res[cb][r];
                out[(size_t)m * ldo + n] = f2bf(v);
            }
        }
    }
}

// one thread per MX block: 64 bytes of bf16 in, 16 bytes of codes and one scale byte out
__global__ __launch_bounds__(256) void quantize_rows_mxfp4_kernel(const bf16_t* __restrict__ x, uint8_t* __restrict__ q,
                                                                  uint8_t* __restrict__ s, int rows, int nblk, int ld_in) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)rows * nblk) return;
    const int row = (int)(idx / nblk), b = (int)(idx % nblk);
    const uint4* src = reinterpret_cast<const uint4*>(x + (size_t)row * ld_in + (size_t)b * 32);
    uint32_t p[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint4 v = src[i];
        p[4 * i] = v.x, p[4 * i + 1] = v.y, p[4 * i + 2] = v.z, p[4 * i + 3] = v.w;
    }
    uint32_t amax = 0u;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t a = mx4_amax2(p[j]);
        amax = a > amax ? a : amax;
    }
    const uint32_t code = mx4_scale_code(amax);
    const float inv = mx4_inv_scale(code);
    uint4 o;
    o.x = mx4_codes4(p[0], p[1], inv) | (mx4_codes4(p[2], p[3], inv) << 16);
    o.y = mx4_codes4(p[4], p[5], inv) | (mx4_codes4(p[6], p[7], inv) << 16);
    o.z = mx4_codes4(p[8], p[9], inv) | (mx4_codes4(p[10], p[11], inv) << 16);
    o.w = mx4_codes4(p[12], p[13], inv) | (mx4_codes4(p[14], p[15], inv) << 16);
    reinterpret_cast<uint4*>(q)[idx] = o;
    s[idx] = (uint8_t)code;
}

}  // namespace

#ifdef O3V_TUNE
extern "C" void o3v_mxfp4_tune(int R, int KS, int NW, int U) { g_t4[0] = R, g_t4[1] = KS, g_t4[2] = NW, g_t4[3] = U; }
extern "C" void o3v_mxfp4_rows_tune(int KS, int waves, int U) { g_t4r[0] = KS, g_t4r[1] = waves, g_t4r[2] = U; }
#endif

extern "C" int o3v_quantize_rows_mxfp4(const void* x, void* codes, void* scales, int rows, int cols, int ld_in, hipStream_t stream) {
    if (!x || !codes || !scales || rows < 0 || cols <= 0 || ld_in < cols || ((uintptr_t)x & 15) || ((uintptr_t)codes & 15)) return O3V_ERR_ARG;
    if ((cols & 31) || (ld_in & 7)) return O3V_ERR_SHAPE;
    if (rows == 0) return O3V_OK;
    const int nblk = cols >> 5;
    const size_t total = (size_t)rows * nblk;
    O3V_KLAUNCH(quantize_rows_mxfp4_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const bf16_t*)x, (uint8_t*)codes,
                (uint8_t*)scales, rows, nblk, ld_in);
    O3V_CHECK_LAUNCH();
    return O3V_OK;
}

extern "C" int o3v_linear_decode_mxfp4(const void* X, const void* norm_w, float eps, const void* W4, const void* S4, const void* bias,
                                       const void* res, void* out, int M, int N, int K, int ldx, int ldo, int ldr, int epilogue,
                                       hipStream_t stream) {
    if (!X || !W4 || !S4 || !out || M < 0 || M > 3 || N <= 0 || K <= 0) return O3V_ERR_ARG;
    if (epilogue != EPI_NONE && epilogue != EPI_RESIDUAL && epilogue != EPI_SWIGLU) return O3V_ERR_ARG;
    if (epilogue == EPI_RESIDUAL && !res) return O3V_ERR_ARG;
    if ((K & 31) || (ldx & 7) || ldx < K || ((uintptr_t)W4 & 15)) return O3V_ERR_SHAPE;  // whole MX blocks, 16-byte chunks of x
    if (epilogue == EPI_SWIGLU && (N % 32)) return O3V_ERR_SHAPE;
    if (M == 0) return O3V_OK;
    const G4Args a{(const bf16_t*)X, (const bf16_t*)bias, (const bf16_t*)res, (const bf16_t*)norm_w, (const uint8_t*)W4, (const uint8_t*)S4,
                   (bf16_t*)out, eps, N, K, ldx, ldo, ldr, epilogue, stream};
    int rc;
    switch (M) {
        case 1: rc = norm_w ? launch_g4_m<1, true>(a) : launch_g4_m<1, false>(a); break;
        case 2: rc = norm_w ? launch_g4_m<2, true>(a) : launch_g4_m<2, false>(a); break;
        default: rc = norm_w ? launch_g4_m<3, true>(a) : launch_g4_m<3, false>(a); break;
    }
    if (rc != O3V_OK) return rc;
    O3V_CHECK_LAUNCH();
    return O3V_OK;
}

extern "C" int o3v_linear_decode_mxfp4_rows(const void* X, const void* W4p, const void* S4p, const void* bias, const void* res, void* out,
                                            int M, int N, int K, int ldx, int ldo, int ldr, int epilogue, hipStream_t stream) {
    if (!X || !W4p || !S4p || !out || M < 4 || M > 32 || N <= 0 || K <= 0) return O3V_ERR_ARG;
    if (epilogue != EPI_NONE && epilogue != EPI_RESIDUAL && epilogue != EPI_SWIGLU) return O3V_ERR_ARG;
    if (epilogue == EPI_RESIDUAL && !res) return O3V_ERR_ARG;
    if ((K & 127) || (N & 15) || (ldx & 7) || ldx < K || (epilogue == EPI_SWIGLU && (N & 31)) || ((uintptr_t)W4p & 15) || ((uintptr_t)S4p & 3))
        return O3V_ERR_SHAPE;
    const int RB = epilogue == EPI_SWIGLU ? 2 : 1;
    const int groups = RB == 2 ? N / 32 : N / 16;
    const int cbn = M > 16 ? 2 : 1;
    // K slices x waves per workgroup x steps per trip, by A/B at the 7B shapes (us at 8 / 16 rows; the fp8 fragments: gate/up 25.5 /
    // 29.8, down_proj 20.1 / 25.1):
    //   few row groups, long K (down_proj: 224 groups x 148 steps): 8 slices in workgroups of 8 waves, two steps per trip -- 19.0 / 22.6
    //       (4 slices of 4 waves 28.6 / 29.8: 3.5 waves per CU keep too little in flight; 16 x 16 17.2 / 25.9)
    //   gate/up: one step per trip; 2 slices up to 8 rows (19.6 us, 4 slices 21.9), 4 above (28.5, 2 slices 29.8)
    //   else as the fp8 fragments: no split from 2048 row groups on, 4 slices below
    const bool long_k = groups < 1024 && (K >> 7) >= 64;
    const int ks = long_k ? 8 : groups >= 2048 ? 1 : (RB == 2 && M <= 8) ? 2 : 4;
#ifdef O3V_TUNE
    if (g_t4r[0]) {
#define O3V_T4R(E, KK, NN, UV)                                                                                                       \
    if (epilogue == E && g_t4r[0] == KK && g_t4r[1] == NN && g_t4r[2] == UV && cbn == 1) {                                            \
        constexpr int RG_ = NN / KK;                                                                                                 \
        O3V_KLAUNCH((gemv_mfma_mxfp4_kernel<E, KK, 1, NN, UV>), dim3((groups + RG_ - 1) / RG_), dim3(NN * 64),                       \
                    KK > 1 ? (size_t)NN * RB * 64 * 16 : 0, stream, (const bf16_t*)X, (const uint8_t*)W4p, (const uint8_t*)S4p,      \
                    (const bf16_t*)bias, (const bf16_t*)res, (bf16_t*)out, M, N, K, ldx, ldo, ldr);                                  \
        O3V_CHECK_LAUNCH();                                                                                                          \
        return O3V_OK;                                                                                                               \
    }
        O3V_T4R(EPI_SWIGLU, 4, 4, 4) O3V_T4R(EPI_SWIGLU, 4, 4, 2) O3V_T4R(EPI_SWIGLU, 4, 4, 1) O3V_T4R(EPI_SWIGLU, 2, 4, 2)
        O3V_T4R(EPI_SWIGLU, 1, 4, 2) O3V_T4R(EPI_SWIGLU, 2, 4, 1) O3V_T4R(EPI_SWIGLU, 1, 4, 1) O3V_T4R(EPI_SWIGLU, 1, 4, 4)
        O3V_T4R(EPI_RESIDUAL, 4, 4, 4) O3V_T4R(EPI_RESIDUAL, 4, 4, 2) O3V_T4R(EPI_RESIDUAL, 8, 8, 4) O3V_T4R(EPI_RESIDUAL, 8, 8, 2)
        O3V_T4R(EPI_RESIDUAL, 16, 16, 2) O3V_T4R(EPI_RESIDUAL, 16, 16, 1) O3V_T4R(EPI_RESIDUAL, 4, 4, 8) O3V_T4R(EPI_RESIDUAL, 8, 8, 8)
#undef O3V_T4R
        return O3V_ERR_ARG;
    }
#endif
#define O3V_F4K(E, KK, CC, NN, UV)                                                                                                  \
    do {                                                                                                                            \
        constexpr int RG_ = NN / KK;                                                                                                \
        const dim3 grid((groups + RG_ - 1) / RG_), block(NN * 64);                                                                  \
        const size_t sh = KK > 1 ? (size_t)NN * RB * CC * 64 * 16 : 0;                                                              \
        O3V_KLAUNCH((gemv_mfma_mxfp4_kernel<E, KK, CC, NN, UV>), grid, block, sh, stream, (const bf16_t*)X, (const uint8_t*)W4p,     \
                    (const uint8_t*)S4p, (const bf16_t*)bias, (const bf16_t*)res, (bf16_t*)out, M, N, K, ldx, ldo, ldr);            \
    } while (0)
    // (E: epilogue, U1: steps per trip at <= 16 rows; above, two column blocks and one step)
#define O3V_F4E(E, U1)                        \
    do {                                      \
        if (ks == 8) {                        \
            if (cbn == 2)                     \
                O3V_F4K(E, 8, 2, 8, 1);       \
            else                              \
                O3V_F4K(E, 8, 1, 8, 2);       \
        } else if (ks == 1) {                 \
            if (cbn == 2)                     \
                O3V_F4K(E, 1, 2, 4, 1);       \
            else                              \
                O3V_F4K(E, 1, 1, 4, U1);      \
        } else if (ks == 2) {                 \
            if (cbn == 2)                     \
                O3V_F4K(E, 2, 2, 4, 1);       \
            else                              \
                O3V_F4K(E, 2, 1, 4, U1);      \
        } else {                              \
            if (cbn == 2)                     \
                O3V_F4K(E, 4, 2, 4, 1);       \
            else                              \
                O3V_F4K(E, 4, 1, 4, U1);      \
        }                                     \
    } while (0)
    switch (epilogue) {
        case EPI_NONE: O3V_F4E(EPI_NONE, 2); break;
        case EPI_RESIDUAL: O3V_F4E(EPI_RESIDUAL, 2); break;
        default: O3V_F4E(EPI_SWIGLU, 1); break;
    }
#undef O3V_F4E
#undef O3V_F4K
    O3V_CHECK_LAUNCH();
    return O3V_OK;
}
