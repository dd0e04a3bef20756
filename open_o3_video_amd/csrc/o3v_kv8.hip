// Opt-in fp8 K/V cache of the independent-row decode (vLLM kv_cache_dtype="fp8").
//   K8, V8  u8  [layer][B][Hkv][Tmax][128]  OCP e4m3fn codes
//   Ks, Vs  f32 [layer][B][Hkv][Tmax]       one power-of-two scale per (token, kv head) row of 128
// Rule of a row: o3v_quantize_rows_fp8's (o3v_fp8_rows.h), bit for bit.  code * scale is exactly a bf16 value (e4m3 has 4
// significant bits, the scale is a power of two), so the attention kernel below widens a tile to the bf16 fragments the bf16
// kernel would have loaded from the dequantised cache and then runs the same instruction sequence: same bits out.
#include "o3v_common.h"
#include "o3v_fp8_rows.h"
#include "o3v_attn_decode_body.h"

namespace {

// 8 codes * scale -> 8 bf16, exact: v_cvt_scalef32_pk_bf16_fp8 widens two codes and applies the power-of-two scale in one
// instruction (4 per 8 values; converting to f32, multiplying and packing costs 12 and made the attention kernel VALU-bound)
__device__ __forceinline__ u32x4 kv8_widen8(const u32x2 w, const float sc) {
    return (u32x4){__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[0], sc, false)),
                   __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[0], sc, true)),
                   __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[1], sc, false)),
                   __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[1], sc, true))};
}

// One row of 128 bf16 held by 16 consecutive lanes (8 values each) -> this lane's 8 codes and the row's scale
__device__ __forceinline__ u32x2 kv8_quant_chunk(const u32x4& v, float& sc) {
    float y[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        y[2 * j] = bf_lo(v[j]);
        y[2 * j + 1] = bf_hi(v[j]);
    }
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(y[j]));
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    sc = pow2_scale_for(amax);
    const uint2 q = pack8_fp8(y, 1.0f / sc);
    return (u32x2){q.x, q.y};
}

// bf16 [heads][S][128] (what prefill wrote; heads = layers * B * Hkv) -> slots 0..S-1 of the fp8 caches of capacity Tmax.
// 16 lanes per row, one 16-byte load per lane; blockIdx.y: 0 = K, 1 = V.  Written once and read by later launches only.
__global__ __launch_bounds__(256) void kv8_quantize_kernel(const bf16_t* __restrict__ Ksrc, const bf16_t* __restrict__ Vsrc,
                                                           uint8_t* __restrict__ K8, uint8_t* __restrict__ V8, float* __restrict__ Ks,
                                                           float* __restrict__ Vs, long rows, int S, int Tmax) {
    const long r = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (r >= rows) return;
    const int c = threadIdx.x & 15;
    const bool isv = blockIdx.y != 0;
    const long head = r / S, dst = head * Tmax + (r - head * S);
    const u32x4 v = *reinterpret_cast<const u32x4*>((isv ? Vsrc : Ksrc) + (size_t)r * 128 + c * 8);
    float sc;
    const u32x2 q = kv8_quant_chunk(v, sc);
    __builtin_nontemporal_store(q, reinterpret_cast<u32x2*>((isv ? V8 : K8) + (size_t)dst * 128 + c * 8));
    if (c == 0) __builtin_nontemporal_store(sc, (isv ? Vs : Ks) + dst);
}

// in place on bf16 caches [heads][Tmax][128]: rows slot0 .. slot0+n-1 of every head become dequant(quant(row))
__global__ __launch_bounds__(256) void kv8_roundtrip_kernel(bf16_t* __restrict__ Kc, bf16_t* __restrict__ Vc, long rows, int n, int slot0,
                                                            int Tmax) {
    const long r = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (r >= rows) return;
    const int c = threadIdx.x & 15;
    const long head = r / n;
    u32x4* p = reinterpret_cast<u32x4*>((blockIdx.y ? Vc : Kc) + (size_t)(head * Tmax + slot0 + (r - head * n)) * 128 + c * 8);
    float sc;
    const u32x2 q = kv8_quant_chunk(*p, sc);
    *p = kv8_widen8(q, sc);
}

// ------------------------------------------------------------------------------------------------
// Decode attention over the fp8 cache: the tiling of attn_decode_mfma_body<false> (32-key tiles per wave, the GQA group as the
// 16 MFMA rows, context splits, the same merge), with a tile arriving as 8 B per lane per k-step (K) / per chunk (V) plus one
// scale per lane (lanes 0..31: the K scale of key key0 + lane, lanes 32..63: the V scale of key key0 + lane - 32, handed to the
// lanes that need it by ds_bpermute).  Widened at once to the bf16 fragments, then the bf16 kernel's instruction sequence.
//
// The newest key (ctx-1) arrives as a bf16 row in Knew / Vnew [B][Hkv][128].  The ONE wave whose key range holds ctx-1 quantises
// it, stores codes and scale to slot ctx-1 (plain vector stores) and uses the dequantised row in its own tile: the step sees
// what later steps will read.  Only that wave's last tile reaches rows >= ctx-1 (every other wave's tiles end at or before
// ctx-1), so the stale bytes of slot ctx-1 are never used: K rows there are masked, V rows are replaced.
// V rows of keys outside [k_lo, ctx) are zero in the LDS image whatever their bytes and scales are: their p is 0, and 0 x NaN
// must not reach the sum.  (The bf16 kernel multiplies 0 by a finite value there: the same +-0 terms.)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 3) void attn_decode_kv8_kernel(const bf16_t* __restrict__ Q, uint8_t* __restrict__ K8,
                                                              uint8_t* __restrict__ V8, float* __restrict__ Ks, float* __restrict__ Vs,
                                                              const bf16_t* __restrict__ Knew, const bf16_t* __restrict__ Vnew,
                                                              float* __restrict__ part_o, float* __restrict__ part_ml,
                                                              const int* __restrict__ k_lo_arr, int ctx, int Hq, int Hkv, int n_rep,
                                                              int Tmax, float scale_log2e) {
    extern __shared__ __attribute__((aligned(16))) char smem[];  // 4 x V slice, reused for the merge
    constexpr int D = 128, KT = 32, VSTRIDE = 288, V_BYTES = KT * VSTRIDE;
    const int split = blockIdx.x, nsplit = gridDim.x, hk = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int k_lo = k_lo_arr ? k_lo_arr[b] : 0;
    char* Vl = smem + wave * V_BYTES;

    int chunk = (ctx + nsplit - 1) / nsplit;
    chunk = (chunk + 4 * KT - 1) / (4 * KT) * (4 * KT);  // whole 32-key tiles per wave
    const int per_wave = chunk >> 2;
    const int kw0 = split * chunk + wave * per_wave;
    int kw1 = kw0 + per_wave;
    kw1 = kw1 < ctx ? kw1 : ctx;
    const int last = ctx - 1;

    const size_t head = (size_t)b * Hkv + hk;
    uint8_t* Kb = K8 + head * Tmax * D;
    uint8_t* Vb = V8 + head * Tmax * D;
    float* Ksb = Ks + head * Tmax;
    float* Vsb = Vs + head * Tmax;

    // ---- the newest key: lanes 0..15 hold K's chunks, lanes 16..31 V's (32..63 repeat them and store nothing)
    const bool owner = kw0 <= last && last < kw1;  // wave-uniform, true for exactly one wave of the (b, kv head)
    u32x2 nq = {0u, 0u};
    float nsc = 1.0f;
    if (owner) {
        const int c = lane & 15;
        const bool isv = (lane & 16) != 0;
        nq = kv8_quant_chunk(*reinterpret_cast<const u32x4*>((isv ? Vnew : Knew) + head * D + c * 8), nsc);
        if (lane < 32) {
            *reinterpret_cast<u32x2*>((isv ? Vb : Kb) + (size_t)last * D + c * 8) = nq;
            if (c == 0) (isv ? Vsb : Ksb)[last] = nsc;
        }
    }

    bf16x8 qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        if (fr < n_rep)
            qf[ks] = *reinterpret_cast<const bf16x8*>(Q + ((size_t)b * Hq + hk * n_rep + fr) * D + ks * 32 + fg * 8);
        else
            qf[ks] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    }

    float m_run = -1e30f, l_run = 0.f;
    f32x4 o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int tq = fr >> 2, tp = fr & 3;

    for (int key0 = kw0; key0 < kw1; key0 += KT) {
        // ---- the tile's codes and scales (rows past ctx-1 are clamped onto it, as in the bf16 kernel)
        u32x2 kq[2][4], vq[8];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            int kr = key0 + kb * 16 + fr;
            kr = kr < last ? kr : last;
            const uint8_t* Kr = Kb + (size_t)kr * D;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) kq[kb][ks] = *reinterpret_cast<const u32x2*>(Kr + ks * 32 + fg * 8);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = i * 64 + lane, row = c >> 4, ch = c & 15;
            int kr = key0 + row;
            kr = kr < last ? kr : last;
            vq[i] = *reinterpret_cast<const u32x2*>(Vb + (size_t)kr * D + ch * 8);
        }
        float sc;
        {
            int kr = key0 + (lane & 31);
            kr = kr < last ? kr : last;
            sc = (lane < 32 ? Ksb : Vsb)[kr];
        }
        if (owner && key0 + KT > last) {  // the newest key's row from registers, not from the slot written above
            const float ksn = __shfl(nsc, 0, 64), vsn = __shfl(nsc, 16, 64);
            if (key0 + (lane & 31) >= last) sc = lane < 32 ? ksn : vsn;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const bool hit = key0 + kb * 16 + fr >= last;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const uint32_t t0 = __shfl(nq[0], ks * 4 + fg, 64), t1 = __shfl(nq[1], ks * 4 + fg, 64);
                    if (hit) kq[kb][ks] = (u32x2){t0, t1};
                }
            }
            const uint32_t v0 = __shfl(nq[0], 16 + fr, 64), v1 = __shfl(nq[1], 16 + fr, 64);  // chunk ch == fr for every i
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (key0 + i * 4 + fg >= last) vq[i] = (u32x2){v0, v1};
        }
        // ---- widen: K to the A fragments, V to this wave's LDS slice
        bf16x8 kf[2][4];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const float ksc = __shfl(sc, kb * 16 + fr, 64);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) kf[kb][ks] = __builtin_bit_cast(bf16x8, kv8_widen8(kq[kb][ks], ksc));
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = i * 4 + fg, ch = fr, j = key0 + row;
            const float vsc = __shfl(sc, 32 + row, 64);
            u32x4 w = kv8_widen8(vq[i], vsc);
            if (j >= ctx || j < k_lo) w = (u32x4){0u, 0u, 0u, 0u};
            *reinterpret_cast<u32x4*>(Vl + row * VSTRIDE + ch * 16) = w;
        }
        // ---- from here on the bf16 kernel: S^T = K . Q^T
        f32x4 s[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            s[kb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) s[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kb][ks], qf[ks], s[kb], 0, 0, 0);
        }
        float mx = -1e30f;
        bool ok[2][4];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = key0 + kb * 16 + fg * 4 + r;
                ok[kb][r] = (j < kw1) && (j >= k_lo);
                const float sv = ok[kb][r] ? s[kb][r] * scale_log2e : -1e30f;
                s[kb][r] = sv;
                mx = fmaxf(mx, sv);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        m_run = m_new;
        float psum = 0.f;
        bf16x8 pb;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = ok[kb][r] ? __builtin_amdgcn_exp2f(s[kb][r] - m_new) : 0.f;
                const bf16_t pq = f2bf(p);
                psum += bf2f(pq);
                pb[kb * 4 + r] = (short)pq;
            }
        l_run = l_run * alpha + psum;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] *= alpha;
        // ---- O^T += V^T . P^T   (LDS ops of one wave execute in order: the tr-reads see the stores above)
        const char* r0 = Vl + (fg * 4 + tq) * VSTRIDE + tp * 8;
        const char* r1 = r0 + 16 * VSTRIDE;
#pragma unroll
        for (int db = 0; db < 8; ++db) {
            const bf16x4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(r0 + db * 32));
            const bf16x4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(r1 + db * 32));
            const bf16x8 av = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
            o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, pb, o[db], 0, 0, 0);
        }
    }
    // ---- merge the 4 waves: so[w][q][d], sm/sl[w][q] in LDS (the V slices are dead)
    float l_tot = l_run + __shfl_xor(l_run, 16, 64);
    l_tot += __shfl_xor(l_tot, 32, 64);
    __syncthreads();
    float* so = reinterpret_cast<float*>(smem);  // [4][16][128] = 32 KiB
    float* sm = so + 4 * 16 * D;                  // [4][16]
    float* sl = sm + 64;                          // [4][16]
#pragma unroll
    for (int db = 0; db < 8; ++db) *reinterpret_cast<f32x4*>(so + ((size_t)(wave * 16 + fr) * D + db * 16 + fg * 4)) = o[db];
    if (fg == 0) {
        sm[wave * 16 + fr] = m_run;
        sl[wave * 16 + fr] = l_tot;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_rep * D; i += 256) {
        const int q = i / D, d = i % D;
        const float mn = fmaxf(fmaxf(sm[q], sm[16 + q]), fmaxf(sm[32 + q], sm[48 + q]));
        float acc = 0.f, lt = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float sc = __builtin_amdgcn_exp2f(sm[w * 16 + q] - mn);
            acc += so[(size_t)(w * 16 + q) * D + d] * sc;
            lt += sl[w * 16 + q] * sc;
        }
        const size_t idx = ((size_t)b * Hq + hk * n_rep + q) * nsplit + split;
        part_o[idx * D + d] = acc;
        if (d == 0) {
            part_ml[idx * 2] = mn;
            part_ml[idx * 2 + 1] = lt;
        }
    }
}

}  // namespace

extern "C" int o3v_kv8_quantize(const void* Ksrc, const void* Vsrc, void* K8, void* V8, float* Ks, float* Vs, long heads, int S, int Tmax,
                                int D, hipStream_t stream) {
    if (!Ksrc || !Vsrc || !K8 || !V8 || !Ks || !Vs || heads < 0 || S < 0 || S > Tmax) return O3V_ERR_ARG;
    if (D != 128) return O3V_ERR_SHAPE;
    const long rows = heads * S, blocks = (rows + 15) / 16;
    if (blocks > 0x7fffffffL) return O3V_ERR_SHAPE;
    if (rows == 0) return O3V_OK;
    O3V_KLAUNCH(kv8_quantize_kernel, dim3((unsigned)blocks, 2), dim3(256), 0, stream, (const bf16_t*)Ksrc, (const bf16_t*)Vsrc,
                (uint8_t*)K8, (uint8_t*)V8, Ks, Vs, rows, S, Tmax);
    O3V_CHECK_LAUNCH();
    return O3V_OK;
}

extern "C" int o3v_kv8_roundtrip(void* Kc, void* Vc, long heads, int Tmax, int slot0, int n, int D, hipStream_t stream) {
    if (!Kc || !Vc || heads < 0 || slot0 < 0 || n < 0 || slot0 + n > Tmax) return O3V_ERR_ARG;
    if (D != 128) return O3V_ERR_SHAPE;
    const long rows = heads * n, blocks = (rows + 15) / 16;
    if (blocks > 0x7fffffffL) return O3V_ERR_SHAPE;
    if (rows == 0) return O3V_OK;
    O3V_KLAUNCH(kv8_roundtrip_kernel, dim3((unsigned)blocks, 2), dim3(256), 0, stream, (bf16_t*)Kc, (bf16_t*)Vc, rows, n, slot0, Tmax);
    O3V_CHECK_LAUNCH();
    return O3V_OK;
}

extern "C" int o3v_attn_decode_kv8(const void* Q, void* K8, void* V8, float* Ks, float* Vs, const void* Knew, const void* Vnew, void* out,
                                   float* part_o, float* part_ml, const int* k_lo, int B, int Hq, int Hkv, int D, int ctx, int Tmax,
                                   int nsplit, float scale, hipStream_t stream) {
    if (!Q || !K8 || !V8 || !Ks || !Vs || !Knew || !Vnew || !out || !part_o || !part_ml || B < 0 || Hq <= 0 || Hkv <= 0 || (Hq % Hkv) ||
        ctx <= 0 || ctx > Tmax || nsplit <= 0 || nsplit > 64)
        return O3V_ERR_ARG;
    const int n_rep = Hq / Hkv;
    if (D != 128 || n_rep > NREP_MAX) return O3V_ERR_SHAPE;
    if (B == 0) return O3V_OK;
    O3V_KLAUNCH(attn_decode_kv8_kernel, dim3(nsplit, Hkv, B), dim3(256), 4 * 32 * 288, stream, (const bf16_t*)Q, (uint8_t*)K8, (uint8_t*)V8, Ks,
                Vs, (const bf16_t*)Knew, (const bf16_t*)Vnew, part_o, part_ml, k_lo, ctx, Hq, Hkv, n_rep, Tmax, scale * 1.4426950408889634f);
    O3V_CHECK_LAUNCH();
    return o3v_attn_decode_combine128(part_o, part_ml, out, B * Hq, nsplit, stream);
}
