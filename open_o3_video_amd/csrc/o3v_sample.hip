// Rollout sampler: repetition penalty -> temperature -> top-k -> top-p -> multinomial, 32 blocks per sequence, no sort.
// Restates TF:generation/logits_process.py:404-414 (penalty), :301-303 (temperature), :590-594 (top-k: drop every score
// below the k-th largest; ties with it stay), :527-539 (top-p over what top-k kept: drop the ascending-sorted prefix whose
// cumulative probability is <= 1-top_p, keep >= 1)
// and TF:generation/utils.py:2921-2923 (softmax -> multinomial) as used by the GSPO rollout
// (R:src/r1-v/src/open_r1/trainer/grpo_trainer.py:306-313: do_sample, top_p 0.95, temperature 1).
//
// The row (152064 bf16 logits = 300 KB, L2-resident right after the lm_head) is streamed five times with 16-byte
// loads, eight groups in flight per thread; nothing is written back.  Probability mass is carried as 2^-40 fixed point
// (e = exp(s - max) <= 1), so every sum -- the normaliser, the radix-select histograms, the draw -- is an integer sum:
// exact and independent of the order the atomics land in, hence reproducible.
//   pass A  max of the processed scores
//   top-k   (top_k > 0 only) three count histograms over 12 / 12 / 8 bits of the score's order-preserving key, then one
//           block per row walks them from the top to the key of the k-th largest score; the passes below skip smaller keys
//   pass B  z = sum e and the level-0 histogram of mass over the top 12 bits of e (values below 2^-24 are lumped)
//   pass C/D levels 1 and 2 (12 and 7 more bits) of the radix select for the smallest tau with mass{e <= tau} > (1-top_p) z
//   pass E  kept mass {e >= tau} per thread, block scan, the thread holding the drawn target walks its own elements
// RNG: counter-based (splitmix64 of seed, completion id, step) so a completion is reproducible wherever it is generated
// (SURVEY.md section 8e).
#include "../../include/o3v.h"
#include "o3v_common.h"
#include <string.h>

namespace {

constexpr int NT = 256, NBLK = 32;                  // threads per block, blocks per row
constexpr float FX_SCALE = 1099511627776.0f;        // 2^40

typedef unsigned long long u64;

// per-row workspace (u64 units) inside the caller's scratch: O3V_SAMPLE_SCRATCH_FLOATS floats per row
constexpr int WS_H0 = 0, WS_H1 = 4096, WS_H2 = 8192, WS_BM = 8320, WS_Z = 8352, WS_PREFIX = 8353, WS_KTH = 8354;
constexpr int WS_C0 = 8356, WS_C1 = WS_C0 + 4096, WS_C2 = WS_C1 + 4096;   // top-k count histograms (descending key order)
constexpr int WS_PMAX = WS_C2 + 256;                                      // everything below is cleared by pass A
constexpr int WS_U64 = WS_PMAX + NBLK / 2;                                // pmax: NBLK floats
constexpr int WS_FLOATS = 40960;
static_assert(WS_U64 * 2 <= WS_FLOATS, "row workspace");

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int m) {
    const unsigned lo = __shfl_xor((unsigned)v, m, 64), hi = __shfl_xor((unsigned)(v >> 32), m, 64);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_up_u64(u64 v, int d) {
    const unsigned lo = __shfl_up((unsigned)v, d, 64), hi = __shfl_up((unsigned)(v >> 32), d, 64);
    return ((u64)hi << 32) | lo;
}

__device__ float block_max(float v, float* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = -INFINITY;
    for (int i = 0; i < NT / 64; ++i) t = fmaxf(t, red[i]);
    return t;
}
__device__ u64 block_sum_u64(u64 v, u64* red) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += shfl_xor_u64(v, m);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 t = 0;
    for (int i = 0; i < NT / 64; ++i) t += red[i];
    return t;
}
// exclusive prefix of `v` over the block in thread order; *total = block sum
__device__ u64 block_scan_excl_u64(u64 v, u64* red, u64* total) {
    u64 incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = shfl_up_u64(incl, o);
        if ((int)(threadIdx.x & 63) >= o) incl += t;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6] = incl;
    __syncthreads();
    u64 off = 0, tot = 0;
    for (int w = 0; w < NT / 64; ++w) {
        if (w < (int)(threadIdx.x >> 6)) off += red[w];
        tot += red[w];
    }
    *total = tot;
    return off + incl - v;
}

typedef o3v_samp_x SampX;

struct Row {
    const bf16_t* lr;
    const uint8_t* sr;
    int V;
    bool vec;
    float rep, temp;
    // extended controls (read by the EX instantiations only): static edits f32 [V], the row's output counts u16 [V], penalties
    const float* bias;
    const uint16_t* cr;
    float pres, freq;
    const int16_t* gr;   // the guide's table row of this row's state (negative entry: the token is masked) or NULL
};

template <bool EX = false>
__device__ __forceinline__ Row make_row(const bf16_t* logits, const uint8_t* seen, int b, int V, int ldl, float rep, float temp,
                                        const SampX& x = SampX{}) {
    Row r;
    r.bias = EX ? x.bias : nullptr;   // the entry points check their 16-byte alignment, so `vec` below covers them
    r.cr = (EX && x.counts) ? x.counts + (size_t)b * V : nullptr;
    r.pres = EX ? x.pres : 0.f;
    r.freq = EX ? x.freq : 0.f;
    r.gr = EX ? o3v_guide_row(x, b) : nullptr;
    r.lr = logits + (size_t)b * ldl;
    r.sr = seen + (size_t)b * V;
    r.V = V;
    r.vec = ((V & 7) == 0) && ((ldl & 7) == 0) && ((reinterpret_cast<uintptr_t>(logits) & 15) == 0) &&
            ((reinterpret_cast<uintptr_t>(seen) & 7) == 0);
    r.rep = rep;
    r.temp = temp;
    return r;
}

// presence / frequency penalty of a token this row has emitted c > 0 times (vLLM sampler.py apply_penalties, in fp32)
__device__ __forceinline__ float count_penalty(float x, unsigned c, float pres, float freq) { return x - (freq * (float)c + pres); }

// processed scores of elements 8g..8g+7 (TF:404-414 penalty, :301-303 temperature); -inf past the vocabulary.
// EX: the static edits are added first and the count penalties follow the repetition penalty (vLLM 0.7.2 V0 sampler order); a guide
// masks before all of them (vLLM runs guided decoding as a logits processor): eight i16 next-states beside the counts.
template <bool EX = false>
__device__ __forceinline__ void load_group(const Row& r, int g, float s[8]) {
    const int base = g * 8;
    if (r.vec && base + 8 <= r.V) {
        const u32x4 lv = *reinterpret_cast<const u32x4*>(r.lr + base);
        const uint2 sv = *reinterpret_cast<const uint2*>(r.sr + base);
        float bv[8];
        u32x4 cv = {0u, 0u, 0u, 0u};
        if (EX && r.bias) {
            const float4 b0 = *reinterpret_cast<const float4*>(r.bias + base), b1 = *reinterpret_cast<const float4*>(r.bias + base + 4);
            bv[0] = b0.x, bv[1] = b0.y, bv[2] = b0.z, bv[3] = b0.w, bv[4] = b1.x, bv[5] = b1.y, bv[6] = b1.z, bv[7] = b1.w;
        }
        if (EX && r.cr) cv = *reinterpret_cast<const u32x4*>(r.cr + base);
        u32x4 gv = {0u, 0u, 0u, 0u};
        if (EX && r.gr) gv = *reinterpret_cast<const u32x4*>(r.gr + base);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float x = bf2f((bf16_t)((lv[k >> 1] >> (16 * (k & 1))) & 0xffffu));
            const unsigned sb = ((k < 4 ? sv.x : sv.y) >> (8 * (k & 3))) & 0xffu;
            if (EX && ((gv[k >> 1] >> (16 * (k & 1))) & 0x8000u)) x = -INFINITY;   // next state < 0
            if (EX && r.bias) x += bv[k];
            if (r.rep != 1.0f && sb) x = (x < 0.f) ? x * r.rep : x / r.rep;
            if (EX) {
                const unsigned c = (cv[k >> 1] >> (16 * (k & 1))) & 0xffffu;
                if (c) x = count_penalty(x, c, r.pres, r.freq);
            }
            s[k] = x / r.temp;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = base + k;
            float x = -INFINITY;
            if (i < r.V) {
                x = bf2f(r.lr[i]);
                if (EX && r.gr && r.gr[i] < 0) x = -INFINITY;
                if (EX && r.bias) x += r.bias[i];
                if (r.rep != 1.0f && r.sr[i]) x = (x < 0.f) ? x * r.rep : x / r.rep;
                if (EX && r.cr) {
                    const unsigned c = r.cr[i];
                    if (c) x = count_penalty(x, c, r.pres, r.freq);
                }
                x = x / r.temp;
            }
            s[k] = x;
        }
    }
}

// Visits the elements of block `blk`'s slice of the row: thread t owns groups g0+t, g0+t+NT, ...
template <bool EX = false, typename F>
__device__ __forceinline__ void for_each_score(const Row& r, int blk, F&& f) {
    const int NG = (r.V + 7) / 8, per_blk = (NG + NBLK - 1) / NBLK;
    const int g0 = blk * per_blk, g1 = (g0 + per_blk < NG) ? g0 + per_blk : NG;
    for (int g = g0 + threadIdx.x; g < g1; g += NT) {
        float s[8];
        load_group<EX>(r, g, s);
#pragma unroll
        for (int k = 0; k < 8; ++k) f(g * 8 + k, s[k]);
    }
}

__device__ __forceinline__ u64 to_fx(float e) { return (u64)(e * FX_SCALE); }

// order-preserving 32-bit key of a score (larger score <=> larger key); kth key 0 keeps everything
__device__ __forceinline__ unsigned score_key(float s) {
    const unsigned b = __float_as_uint(s);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float row_max(const u64* ws) {
    const float* pm = reinterpret_cast<const float*>(ws + WS_PMAX);
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < NBLK; ++i) m = fmaxf(m, pm[i]);
    return m;
}

// Bin of `hist[0..nb)` in which the running mass (starting at *below) first exceeds `cut`; *below becomes the mass
// before that bin.  Every thread of the block returns the same value.
__device__ int pick_bin(const u64* __restrict__ hist, int nb, u64 cut, u64* below, u64* red, int* s_pick, u64* s_below) {
    const int per = (nb + NT - 1) / NT, tid = threadIdx.x;
    const int k0 = tid * per, k1 = (k0 + per < nb) ? k0 + per : nb;
    u64 mine = 0;
    for (int k = k0; k < k1; ++k) mine += hist[k];
    u64 tot;
    const u64 before = *below + block_scan_excl_u64(mine, red, &tot);
    if (tid == 0) *s_pick = -1;
    __syncthreads();
    if (mine > 0 && before <= cut && before + mine > cut) {
        u64 run = before;
        for (int k = k0; k < k1; ++k) {
            const u64 h = hist[k];
            if (h > 0 && run + h > cut) {
                *s_pick = k;
                *s_below = run;
                break;
            }
            run += h;
        }
    }
    __syncthreads();
    if (*s_pick < 0) {  // cut >= all the mass at this level (top_p ~ 0): take the highest non-empty bin
        if (tid == 0) {
            u64 run = *below, lastrun = *below;
            int lastb = 0;
            for (int k = 0; k < nb; ++k)
                if (hist[k] > 0) {
                    lastb = k;
                    lastrun = run;
                    run += hist[k];
                }
            *s_pick = lastb;
            *s_below = lastrun;
        }
        __syncthreads();
    }
    const int pick = *s_pick;
    *below = *s_below;
    __syncthreads();
    return pick;
}

// K1: slice maxima of the processed scores; clears the row's accumulators for the kernels that follow
// Every kernel below is a body templated on EX with two entry points: the plain one (EX false: the sampler as it always was)
// and `_x` (EX true: static edits, count penalties and min_p of o3v_sampling_opts feeding the same passes).
template <bool EX>
__device__ __forceinline__ void sample_max_body(const bf16_t* __restrict__ logits, const uint8_t* __restrict__ seen,
                                                u64* __restrict__ wsp, int V, int ldl, float rep, float temp, const SampX& x) {
    __shared__ float redf[NT / 64];
    const int blk = blockIdx.x, b = blockIdx.y;
    u64* ws = wsp + (size_t)b * (WS_FLOATS / 2);
    const Row r = make_row<EX>(logits, seen, b, V, ldl, rep, temp, x);
    for (int i = blk * NT + threadIdx.x; i < WS_PMAX; i += NBLK * NT) ws[i] = 0;
    float mx = -INFINITY;
    for_each_score<EX>(r, blk, [&](int, float s) { mx = fmaxf(mx, s); });
    mx = block_max(mx, redf);
    if (threadIdx.x == 0) reinterpret_cast<float*>(ws + WS_PMAX)[blk] = mx;
}
__global__ __launch_bounds__(NT) void sample_max_kernel(const bf16_t* __restrict__ logits, const uint8_t* __restrict__ seen,
                                                        u64* __restrict__ wsp, int V, int ldl, float rep, float temp) {
    sample_max_body<false>(logits, seen, wsp, V, ldl, rep, temp, SampX{});
}
__global__ __launch_bounds__(NT) void sample_max_kernel_x(const bf16_t* __restrict__ logits, const uint8_t* __restrict__ seen,
                                                          u64* __restrict__ wsp, int V, int ldl, float rep, float temp, SampX x) {
    sample_max_body<true>(logits, seen, wsp, V, ldl, rep, temp, x);
}

// top-k, levels 0..2: histogram of COUNTS over 12 / 12 / 8 bits of the inverted key (bin 0 = largest scores), restricted to
// the bins the earlier levels chose for the k-th largest element
template <int LVL, bool EX>
__device__ __forceinline__ void sample_count_body(const bf16_t* __restrict__ logits, const uint8_t* __restrict__ seen,
                                                  u64* __restrict__ wsp, int V, int ldl, float rep, float temp, int top_k,
                                                  const SampX& x) {
    constexpr int SH = LVL == 0 ? 20 : (LVL == 1 ? 8 : 0), NB = LVL == 2 ? 256 : 4096;
    __shared__ unsigned hist[NB];
    __shared__ u64 red[NT / 64];
    __shared__ int s_pick;
    __shared__ u64 s_below;
    const int blk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    u64* ws = wsp + (size_t)b * (WS_FLOATS / 2);
    const Row r = make_row<EX>(logits, seen, b, V, ldl, rep, temp, x);
    for (int i = tid; i < NB; i += NT) hist[i] = 0;
    unsigned prefix = 0, hi_mask = 0;
    if (LVL > 0) {
        const u64 cut = (u64)(top_k - 1);
        u64 below = 0;
        prefix = (unsigned)pick_bin(ws + WS_C0, 4096, cut, &below, red, &s_pick, &s_below) << 20;
        hi_mask = 0xffffffffu << 20;
        if (LVL > 1) {
            prefix |= (unsigned)pick_bin(ws + WS_C1, 4096, cut, &below, red, &s_pick, &s_below) << 8;
            hi_mask = 0xffffffffu << 8;
        }
    }
    __syncthreads();
    for_each_score<EX>(r, blk, [&](int i, float s) {
        if (i >= V) return;
        const unsigned inv = ~score_key(s);
        if ((inv & hi_mask) == prefix) atomicAdd(&hist[(inv >> SH) & (NB - 1)], 1u);
    });
    __syncthreads();
    u64* gh = ws + (LVL == 0 ? WS_C0 : (LVL == 1 ? WS_C1 : WS_C2));
    for (int i = tid; i < NB; i += NT)
        if (hist[i]) atomicAdd(gh + i, (u64)hist[i]);
}
template <int LVL>
__global__ __launch_bounds__(NT) void sample_count_kernel(const bf16_t* __restrict__ logits, const uint8_t* __restrict__ seen,
                                                          u64* __restrict__ wsp, int V, int ldl, float rep, float temp, int top_k) {
    sample_count_body<LVL, false>(logits, seen, wsp, V, ldl, rep, temp, top_k, SampX{});
}
template <int LVL>
__global__ __launch_bounds__(NT) void sample_count_kernel_x(const bf16_t* __restrict__ logits, const uint8_t* __restrict__ seen,
                                                            u64* __restrict__ wsp, int V, int ldl, float rep, float temp, int top_k,
                                                            SampX x) {
    sample_count_body<LVL, true>(logits, seen, wsp, V, ldl, rep, temp, top_k, x);
}

// top-k: one block per row resolves the key of the k-th largest score (fewer than k scores: the smallest one)
__global__ __launch_bounds__(NT) void sample_kth_kernel(u64* __restrict__ wsp, int top_k) {
    __shared__ u64 red[NT / 64];
    __shared__ int s_pick;
    __shared__ u64 s_below;
    u64* ws = wsp + (size_t)blockIdx.x * (WS_FLOATS / 2);
    const u64 cut = (u64)(top_k - 1);
    u64 below = 0;
    unsigned inv = (unsigned)pick_bin(ws + WS_C0, 4096, cut, &below, red, &s_pick, &s_below) << 20;
    inv |= (unsigned)pick_bin(ws + WS_C1, 4096, cut, &below, red, &s_pick, &s_below) << 8;
    inv |= (unsigned)pick_bin(ws + WS_C2, 256, cut, &below, red, &s_pick, &s_below);
    if (threadIdx.x == 0) ws[WS_KTH] = (u64)(~inv);
}

// K2..K4 (LVL 0,1,2): mass histogram over 12 / 12 / 7 bits of e = exp(s - max) for the elements that match the bits
// decided by the earlier levels.  Radix select of the smallest tau with mass{e <= tau} > (1 - top_p) z: the kept set
// is {e >= tau} (TF keeps the complement of the ascending prefix with cumulative probability <= 1 - top_p).
template <int LVL, bool EX>
__device__ __forceinline__ void sample_hist_body(const bf16_t* __restrict__ logits, const uint8_t* __restrict__ seen,
                                                 u64* __restrict__ wsp, int V, int ldl, float rep, float temp, float top_p,
                                                 const SampX& x) {
    constexpr int SH = LVL == 0 ? 19 : (LVL == 1 ? 7 : 0), NB = LVL == 2 ? 128 : 4096;
    __shared__ u64 hist[NB];
    __shared__ u64 red[NT / 64];
    __shared__ int s_pick;
    __shared__ u64 s_below;
    const int blk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    u64* ws = wsp + (size_t)b * (WS_FLOATS / 2);
    const Row r = make_row<EX>(logits, seen, b, V, ldl, rep, temp, x);
    const float mx = row_max(ws);
    for (int i = tid; i < NB; i += NT) hist[i] = 0;
    unsigned prefix = 0, hi_mask = 0;
    if (LVL > 0) {
        const u64 cut = (u64)((double)(1.0f - top_p) * (double)ws[WS_Z]);
        u64 below = 0;
        prefix = (unsigned)pick_bin(ws + WS_H0, 4096, cut, &below, red, &s_pick, &s_below) << 19;
        hi_mask = 0xffffffffu << 19;
        if (LVL > 1) {
            prefix |= (unsigned)pick_bin(ws + WS_H1, 4096, cut, &below, red, &s_pick, &s_below) << 7;
            hi_mask = 0xffffffffu << 7;
        }
    }
    __syncthreads();
    u64 zsum = 0;
    const unsigned kth = (unsigned)ws[WS_KTH];
    for_each_score<EX>(r, blk, [&](int, float s) {
        if (score_key(s) < kth) return;   // removed by top-k
        const float e = expf(s - mx);
        const u64 fx = to_fx(e);
        const unsigned bits = __float_as_uint(e);
        if (LVL == 0) zsum += fx;
        if (fx && (bits & hi_mask) == prefix) atomicAdd(&hist[(bits >> SH) & (NB - 1)], fx);
    });
    if (LVL == 0) {
        zsum = block_sum_u64(zsum, red);
        if (tid == 0) atomicAdd(ws + WS_Z, zsum);
    }
    __syncthreads();
    u64* gh = ws + (LVL == 0 ? WS_H0 : (LVL == 1 ? WS_H1 : WS_H2));
    for (int i = tid; i < NB; i += NT)
        if (hist[i]) atomicAdd(gh + i, hist[i]);
}
template <int LVL>
__global__ __launch_bounds__(NT) void sample_hist_kernel(const bf16_t* __restrict__ logits, const uint8_t* __restrict__ seen,
                                                         u64* __restrict__ wsp, int V, int ldl, float rep, float temp,
                                                         float top_p) {
    sample_hist_body<LVL, false>(logits, seen, wsp, V, ldl, rep, temp, top_p, SampX{});
}
template <int LVL>
__global__ __launch_bounds__(NT) void sample_hist_kernel_x(const bf16_t* __restrict__ logits, const uint8_t* __restrict__ seen,
                                                           u64* __restrict__ wsp, int V, int ldl, float rep, float temp,
                                                           float top_p, SampX x) {
    sample_hist_body<LVL, true>(logits, seen, wsp, V, ldl, rep, temp, top_p, x);
}

// K5: kept mass {bits(e) >= tau} of every slice; publishes tau (all blocks of a row compute the same value).
// EX: min_p (vLLM sampler.py _apply_min_p: drop probs < min_p * max prob, i.e. e < min_p) raises tau to at least bits(min_p); the
// draw and the log-prob kernels read the published tau, so they need no min_p of their own.
template <bool EX>
__device__ __forceinline__ void sample_mass_body(const bf16_t* __restrict__ logits, const uint8_t* __restrict__ seen,
                                                 u64* __restrict__ wsp, int V, int ldl, float rep, float temp, float top_p,
                                                 const SampX& x) {
    __shared__ u64 red[NT / 64];
    __shared__ int s_pick;
    __shared__ u64 s_below;
    const int blk = blockIdx.x, b = blockIdx.y;
    u64* ws = wsp + (size_t)b * (WS_FLOATS / 2);
    const Row r = make_row<EX>(logits, seen, b, V, ldl, rep, temp, x);
    const float mx = row_max(ws);
    unsigned prefix = 0;
    if (top_p < 1.0f) {
        const u64 cut = (u64)((double)(1.0f - top_p) * (double)ws[WS_Z]);
        u64 below = 0;
        prefix = (unsigned)pick_bin(ws + WS_H0, 4096, cut, &below, red, &s_pick, &s_below) << 19;
        prefix |= (unsigned)pick_bin(ws + WS_H1, 4096, cut, &below, red, &s_pick, &s_below) << 7;
        prefix |= (unsigned)pick_bin(ws + WS_H2, 128, cut, &below, red, &s_pick, &s_below);
    }
    if (EX && x.minp_bits > prefix) prefix = x.minp_bits;
    u64 mine = 0;
    const unsigned kth = (unsigned)ws[WS_KTH];
    for_each_score<EX>(r, blk, [&](int, float s) {
        const float e = expf(s - mx);
        if (score_key(s) >= kth && __float_as_uint(e) >= prefix) mine += to_fx(e);
    });
    mine = block_sum_u64(mine, red);
    if (threadIdx.x == 0) {
        ws[WS_BM + blk] = mine;
        ws[WS_PREFIX] = prefix;
    }
}
__global__ __launch_bounds__(NT) void sample_mass_kernel(const bf16_t* __restrict__ logits, const uint8_t* __restrict__ seen,
                                                         u64* __restrict__ wsp, int V, int ldl, float rep, float temp,
                                                         float top_p) {
    sample_mass_body<false>(logits, seen, wsp, V, ldl, rep, temp, top_p, SampX{});
}
__global__ __launch_bounds__(NT) void sample_mass_kernel_x(const bf16_t* __restrict__ logits, const uint8_t* __restrict__ seen,
                                                           u64* __restrict__ wsp, int V, int ldl, float rep, float temp,
                                                           float top_p, SampX x) {
    sample_mass_body<true>(logits, seen, wsp, V, ldl, rep, temp, top_p, x);
}

// K6: the draw.  Elements are ordered by slice, then by owning thread, then by that thread's visiting order; the block
// and then the thread whose mass range holds the target walk to the token.
// EX: the emitted token of an unfinished row is counted (u16, saturating); its count before the step goes to cnt_prev.
template <bool EX>
__device__ __forceinline__ void sample_draw_body(const bf16_t* __restrict__ logits, uint8_t* __restrict__ seen,
                                                 const u64* __restrict__ wsp, int* __restrict__ cur_tok,
                                                 int* __restrict__ finished, int* __restrict__ out_ids,
                                                 float* __restrict__ chosen_lp, const int* __restrict__ eos_ids,
                                                 int n_eos, int pad_id, int V, int ldl, float rep, float temp,
                                                 uint64_t seed, const int* __restrict__ row_id, int step,
                                                 int out_stride, uint8_t* __restrict__ seen_prev, const SampX& x) {
    __shared__ u64 red[NT / 64];
    const int blk = blockIdx.x, b = blockIdx.y;
    const u64* ws = wsp + (size_t)b * (WS_FLOATS / 2);
    u64 tot = 0, blk_before = 0;
    for (int i = 0; i < NBLK; ++i) {
        if (i < blk) blk_before += ws[WS_BM + i];
        tot += ws[WS_BM + i];
    }
    const uint64_t rid = row_id ? (uint64_t)row_id[b] : (uint64_t)b;
    const uint64_t rnd = splitmix64(splitmix64(seed ^ (rid * 0xD1B54A32D192ED03ull)) + (uint64_t)step);
    const double u = (double)(rnd >> 40) * (1.0 / 16777216.0);
    u64 target = (u64)(u * (double)tot);
    if (tot > 0 && target >= tot) target = tot - 1;
    const u64 blk_mass = ws[WS_BM + blk];
    if (!(blk_mass > 0 && blk_before <= target && target < blk_before + blk_mass)) return;  // block-uniform
    const Row r = make_row<EX>(logits, seen, b, V, ldl, rep, temp, x);
    const float mx = row_max(ws);
    const unsigned prefix = (unsigned)ws[WS_PREFIX], kth = (unsigned)ws[WS_KTH];
    u64 mine = 0;
    for_each_score<EX>(r, blk, [&](int, float s) {
        const float e = expf(s - mx);
        if (score_key(s) >= kth && __float_as_uint(e) >= prefix) mine += to_fx(e);
    });
    u64 btot;
    const u64 before = blk_before + block_scan_excl_u64(mine, red, &btot);
    if (mine > 0 && before <= target && target < before + mine) {
        u64 run = before;
        int pick = -1;
        float e_pick = 0.f;
        for_each_score<EX>(r, blk, [&](int i, float s) {
            if (pick >= 0) return;
            const float e = expf(s - mx);
            if (score_key(s) >= kth && __float_as_uint(e) >= prefix) {
                run += to_fx(e);
                if (run > target) {
                    pick = i;
                    e_pick = e;
                }
            }
        });
        const bool fin = finished[b] != 0;
        const int tok = fin ? pad_id : pick;
        if (!fin)
            for (int k = 0; k < n_eos; ++k)
                if (tok == eos_ids[k]) finished[b] = 1;
        if (seen_prev) seen_prev[b] = (tok >= 0 && tok < V) ? seen[(size_t)b * V + tok] : 0;  // log-probs see the map before this step
        if (tok >= 0 && tok < V) seen[(size_t)b * V + tok] = 1;
        if (EX && x.counts) o3v_count_token(x, b, V, tok, fin);
        if (EX) o3v_guide_advance(x, b, V, tok, fin);
        cur_tok[b] = tok;
        out_ids[(size_t)b * out_stride + step] = tok;
        if (chosen_lp) chosen_lp[(size_t)b * out_stride + step] = logf(e_pick / ((float)ws[WS_Z] * (1.0f / FX_SCALE)));
    }
}
__global__ __launch_bounds__(NT) void sample_draw_kernel(const bf16_t* __restrict__ logits, uint8_t* __restrict__ seen,
                                                         const u64* __restrict__ wsp, int* __restrict__ cur_tok,
                                                         int* __restrict__ finished, int* __restrict__ out_ids,
                                                         float* __restrict__ chosen_lp, const int* __restrict__ eos_ids,
                                                         int n_eos, int pad_id, int V, int ldl, float rep, float temp,
                                                         uint64_t seed, const int* __restrict__ row_id, int step,
                                                         int out_stride, uint8_t* __restrict__ seen_prev) {
    sample_draw_body<false>(logits, seen, wsp, cur_tok, finished, out_ids, chosen_lp, eos_ids, n_eos, pad_id, V, ldl, rep, temp, seed,
                            row_id, step, out_stride, seen_prev, SampX{});
}
__global__ __launch_bounds__(NT) void sample_draw_kernel_x(const bf16_t* __restrict__ logits, uint8_t* __restrict__ seen,
                                                           const u64* __restrict__ wsp, int* __restrict__ cur_tok,
                                                           int* __restrict__ finished, int* __restrict__ out_ids,
                                                           float* __restrict__ chosen_lp, const int* __restrict__ eos_ids,
                                                           int n_eos, int pad_id, int V, int ldl, float rep, float temp,
                                                           uint64_t seed, const int* __restrict__ row_id, int step,
                                                           int out_stride, uint8_t* __restrict__ seen_prev, SampX x) {
    sample_draw_body<true>(logits, seen, wsp, cur_tok, finished, out_ids, chosen_lp, eos_ids, n_eos, pad_id, V, ldl, rep, temp, seed,
                           row_id, step, out_stride, seen_prev, x);
}


// ------------------------------------------------------------------------------------------------
// Top-N log-probs (vLLM 0.7.2 SamplingParams.logprobs / prompt_logprobs, V0 sampler: log-probs of the PROCESSED distribution).
// Run after the sampler of a decode step, on the scores it drew from: penalty from the seen map as it was BEFORE the step set the
// chosen token (the sampler leaves that byte in seen_prev), then temperature; sampling rows keep only the tokens the draw kept
// (top-k key >= kth, e >= tau, read from the sampler's row workspace) and renormalise over the kept mass -- the same 2^-40 integer
// sum the draw walked, so log-probs and draw agree.  Greedy rows: penalty only, temperature 1, log-softmax over the whole row.
//   LP1  grid (nblk, rows): per slice the N largest keys (score key << 32 | ~id: larger = higher score, then lower id; all keys
//        distinct, so "ties to the lower id" is exact), the count of (kept) scores strictly above the chosen token's and, for greedy /
//        prompt rows, the slice's max and sum exp(s - max)
//   LP2  one wave per row: merges the nblk * N keys, the counts and the (max, sum) pairs
// Selection (N <= 20, the row L2-resident after the lm_head): every wave keeps a sorted top-N list in lanes 0..N-1.  A batch of 64
// candidates costs one compare + ballot against the list's N-th key; only the few that beat it are inserted (ballot popcount for
// the slot, one shfl_up to shift).  For a 4.7k-element slice that is ~N ln(slice / N) ~ 100 insertions per block, all in registers:
// no LDS histogram and no second radix select (which would cost three more passes over the row with their atomics).
// ------------------------------------------------------------------------------------------------
constexpr int LP_MAXN = 20;                              // O3V_MAX_LOGPROBS
constexpr int LP_REC = 24;                               // u64 per slice record: LP_MAXN keys, greater-count, {max, sum}
constexpr int LP_OFF = 18432;                            // u64 offset of a row's records inside its sampler scratch row
constexpr int LP_SEEN_PREV = LP_OFF + NBLK * LP_REC;     // row 0 only: u8 [B <= 32] chosen tokens' seen bytes before the step
constexpr int LP_CNT_PREV = LP_SEEN_PREV + 4;            // row 0 only: u16 [B <= 32] chosen tokens' output counts before the step
constexpr int LP_NB_ROWS = 8;                            // slices per row of the prompt-side entry (many rows in flight)
static_assert(WS_U64 <= LP_OFF && LP_CNT_PREV + 8 <= WS_FLOATS / 2, "log-prob records inside the sampler scratch row");
static_assert(LP_NB_ROWS * LP_REC * 2 == 384, "O3V_LOGPROB_ROW_SCRATCH_FLOATS");

__device__ __forceinline__ u64 shfl_u64(u64 v, int src) {
    const unsigned lo = __shfl((unsigned)v, src, 64), hi = __shfl((unsigned)(v >> 32), src, 64);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 lp_key(float s, int i) { return ((u64)score_key(s) << 32) | (u64)(~(unsigned)i); }
__device__ __forceinline__ int key_id(u64 k) { return (int)~(unsigned)k; }
__device__ __forceinline__ float key_score(u64 k) {
    const unsigned h = (unsigned)(k >> 32);
    return __uint_as_float((h & 0x80000000u) ? (h & 0x7fffffffu) : ~h);
}
__device__ __forceinline__ void lse_merge(float& m, float& z, float om, float oz) {
    const float M = fmaxf(m, om);
    if (M == -INFINITY) return;
    z = (m == -INFINITY ? 0.f : z * expf(m - M)) + (om == -INFINITY ? 0.f : oz * expf(om - M));
    m = M;
}

// descending top-n keys of a wave: lane i < n holds the i-th largest seen so far (0 = empty); every call is wave-uniform
struct WaveTopN {
    u64 mine = 0, thr = 0;  // thr: key of lane n-1 (0 until n keys are held)
    int n;
    __device__ explicit WaveTopN(int n_) : n(n_) {}
    __device__ void insert(u64 c) {
        const int lane = threadIdx.x & 63;
        const int pos = __popcll(__ballot(lane < n && mine > c));
        const u64 up = shfl_up_u64(mine, 1);
        if (lane == pos)
            mine = c;
        else if (lane > pos && lane < n)
            mine = up;
        thr = shfl_u64(mine, n - 1);
    }
    __device__ void offer(u64 c) {  // each lane offers one key (0: none)
        u64 hot = __ballot(c > thr);
        while (hot) {
            const int L = __ffsll((long long)hot) - 1;
            insert(shfl_u64(c, L));
            hot &= ~(1ull << L);
            hot &= __ballot(c > thr);
        }
    }
};

// score of the chosen / target token under the state it was drawn in (seen_prev NULL: raw logits, the prompt side)
// EX: with the static edits and the token's count as it was before the step counted it (cnt_prev)
template <bool EX = false>
__device__ __forceinline__ float lp_token_score(const bf16_t* lr, int tok, int V, const uint8_t* seen_prev, int b, float rep,
                                                float temp, const SampX& sx = SampX{}) {
    if (tok < 0 || tok >= V) return -INFINITY;
    float x = bf2f(lr[tok]);
    if (EX && sx.g_next && o3v_guide_row(sx, b)[tok] < 0) x = -INFINITY;   // (the state of before the step: the draw wrote the other half)
    if (EX && sx.bias) x += sx.bias[tok];
    if (seen_prev && rep != 1.0f && seen_prev[b]) x = (x < 0.f) ? x * rep : x / rep;
    if (EX && sx.counts && sx.cnt_prev) {
        const unsigned c = sx.cnt_prev[b];
        if (c) x = count_penalty(x, c, sx.pres, sx.freq);
    }
    return x / temp;
}

// the sampler's kept set: top-k key and top-p threshold of pass E (sampling rows)
struct KeptTest {
    float mx;
    unsigned kth, prefix;
    __device__ bool operator()(float s) const {
        if (score_key(s) < kth) return false;
        return prefix == 0 || __float_as_uint(expf(s - mx)) >= prefix;
    }
};

template <bool SAMPLED, bool EX>
__device__ __forceinline__ void lp_partial_body(const bf16_t* __restrict__ logits, const uint8_t* __restrict__ seen,
                                                const u64* __restrict__ wsp, u64* __restrict__ recp, int rec_stride, int nblk,
                                                const int* __restrict__ tok_arr, const uint8_t* __restrict__ seen_prev, int V,
                                                int ldl, float rep, float temp, int n, const SampX& sx) {
    __shared__ u64 s_keys[NT / 64][LP_MAXN];
    __shared__ float s_m[NT / 64], s_z[NT / 64];
    __shared__ unsigned s_c[NT / 64];
    const int blk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    Row r;
    r.lr = logits + (size_t)b * ldl;
    r.sr = seen ? seen + (size_t)b * V : nullptr;
    r.V = V;
    r.vec = ((V & 7) == 0) && ((ldl & 7) == 0) && ((reinterpret_cast<uintptr_t>(logits) & 15) == 0) &&
            ((reinterpret_cast<uintptr_t>(seen) & 7) == 0);
    r.rep = rep;
    r.temp = temp;
    r.bias = EX ? sx.bias : nullptr;
    r.cr = (EX && sx.counts) ? sx.counts + (size_t)b * V : nullptr;
    r.pres = EX ? sx.pres : 0.f;
    r.freq = EX ? sx.freq : 0.f;
    r.gr = EX ? o3v_guide_row(sx, b) : nullptr;
    KeptTest kept_test{0.f, 0u, 0u};
    if (SAMPLED) {
        const u64* ws = wsp + (size_t)b * (WS_FLOATS / 2);
        kept_test = KeptTest{row_max(ws), (unsigned)ws[WS_KTH], (unsigned)ws[WS_PREFIX]};
    }
    const int tok = tok_arr[b];
    const float s_tok = lp_token_score<EX>(r.lr, tok, V, seen_prev, b, rep, temp, sx);
    WaveTopN top(n);
    unsigned cnt = 0;
    float m = -INFINITY, z = 0.f;
    const int NG = (V + 7) / 8, per = (NG + nblk - 1) / nblk;
    const int g0 = blk * per, g1 = (g0 + per < NG) ? g0 + per : NG;
    for (int base = g0 + wave * 64; base < g1; base += NT) {  // trip count uniform per wave (ballots below)
        const int g = base + lane;
        float s[8];
        if (g < g1) {
            if (r.sr) {
                load_group<EX>(r, g, s);  // the sampler's own arithmetic
            } else if (r.vec) {
                const u32x4 lv = *reinterpret_cast<const u32x4*>(r.lr + g * 8);
#pragma unroll
                for (int k = 0; k < 8; ++k) s[k] = bf2f((bf16_t)((lv[k >> 1] >> (16 * (k & 1))) & 0xffffu));
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) s[k] = (g * 8 + k < V) ? bf2f(r.lr[g * 8 + k]) : -INFINITY;
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = g * 8 + k;
            const bool valid = g < g1 && i < V;
            const float sk = (i == tok) ? s_tok : s[k];  // the chosen token as it was drawn (its seen byte has changed since)
            bool kept = valid;
            if (SAMPLED) kept = kept && kept_test(sk);
            if (EX) kept = kept && sk > -INFINITY;  // a token the static edits removed is masked, whatever the thresholds say
            cnt += (kept && sk > s_tok) ? 1u : 0u;
            if (!SAMPLED && valid && sk > -INFINITY) {
                if (sk > m) {
                    z = z * expf(m - sk) + 1.f;
                    m = sk;
                } else {
                    z += expf(sk - m);
                }
            }
            if (n > 0) top.offer(kept ? lp_key(sk, i) : 0ull);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += (unsigned)__shfl_xor((int)cnt, o, 64);
        const float om = __shfl_xor(m, o, 64), oz = __shfl_xor(z, o, 64);
        lse_merge(m, z, om, oz);
    }
    if (lane < n) s_keys[wave][lane] = top.mine;
    if (lane == 0) {
        s_c[wave] = cnt;
        s_m[wave] = m;
        s_z[wave] = z;
    }
    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < NT / 64; ++w) top.offer(lane < n ? s_keys[w][lane] : 0ull);
    u64* rec = recp + (size_t)b * rec_stride + (size_t)blk * LP_REC;
    if (lane < n) rec[lane] = top.mine;
    if (lane == 0) {
        for (int w = 1; w < NT / 64; ++w) {
            cnt += s_c[w];
            lse_merge(m, z, s_m[w], s_z[w]);
        }
        rec[LP_MAXN] = cnt;
        float* mz = reinterpret_cast<float*>(rec + LP_MAXN + 1);
        mz[0] = m;
        mz[1] = z;
    }
}
template <bool SAMPLED>
__global__ __launch_bounds__(NT) void lp_partial_kernel(const bf16_t* __restrict__ logits, const uint8_t* __restrict__ seen,
                                                        const u64* __restrict__ wsp, u64* __restrict__ recp, int rec_stride, int nblk,
                                                        const int* __restrict__ tok_arr, const uint8_t* __restrict__ seen_prev, int V,
                                                        int ldl, float rep, float temp, int n) {
    lp_partial_body<SAMPLED, false>(logits, seen, wsp, recp, rec_stride, nblk, tok_arr, seen_prev, V, ldl, rep, temp, n, SampX{});
}
template <bool SAMPLED>
__global__ __launch_bounds__(NT) void lp_partial_kernel_x(const bf16_t* __restrict__ logits, const uint8_t* __restrict__ seen,
                                                          const u64* __restrict__ wsp, u64* __restrict__ recp, int rec_stride, int nblk,
                                                          const int* __restrict__ tok_arr, const uint8_t* __restrict__ seen_prev, int V,
                                                          int ldl, float rep, float temp, int n, SampX sx) {
    lp_partial_body<SAMPLED, true>(logits, seen, wsp, recp, rec_stride, nblk, tok_arr, seen_prev, V, ldl, rep, temp, n, sx);
}

template <bool SAMPLED, bool EX>
__device__ __forceinline__ void lp_final_body(const bf16_t* __restrict__ logits, const u64* __restrict__ wsp,
                                              const u64* __restrict__ recp, int rec_stride, int nblk,
                                              const int* __restrict__ tok_arr, const uint8_t* __restrict__ seen_prev, int V,
                                              int ldl, float rep, float temp, int n, float* __restrict__ chosen_lp,
                                              int* __restrict__ chosen_rank, int* __restrict__ top_ids,
                                              float* __restrict__ top_lp, int out_stride, int col, const SampX& sx) {
    __shared__ int s_ids[LP_MAXN];
    const int b = blockIdx.x, lane = threadIdx.x;
    const u64* rec0 = recp + (size_t)b * rec_stride;
    WaveTopN top(n);
    const int ncand = nblk * n;
    for (int c0 = 0; c0 < ncand; c0 += 64) {
        const int j = c0 + lane;
        top.offer(j < ncand ? rec0[(j / n) * LP_REC + j % n] : 0ull);
    }
    unsigned cnt = 0;
    float m = -INFINITY, z = 0.f;
    if (lane < nblk) {
        cnt = (unsigned)rec0[lane * LP_REC + LP_MAXN];
        const float* mz = reinterpret_cast<const float*>(rec0 + lane * LP_REC + LP_MAXN + 1);
        m = mz[0];
        z = mz[1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += (unsigned)__shfl_xor((int)cnt, o, 64);
        const float om = __shfl_xor(m, o, 64), oz = __shfl_xor(z, o, 64);
        lse_merge(m, z, om, oz);
    }
    // log-prob of a score s: s - (max + log Z) for greedy / prompt rows; (s - max) - log(kept mass) for sampling rows
    const float lse = m + logf(z);
    KeptTest kept_test{0.f, 0u, 0u};
    float lmass = 0.f;
    if (SAMPLED) {
        const u64* ws = wsp + (size_t)b * (WS_FLOATS / 2);
        u64 tot = 0;
        for (int i = 0; i < NBLK; ++i) tot += ws[WS_BM + i];
        kept_test = KeptTest{row_max(ws), (unsigned)ws[WS_KTH], (unsigned)ws[WS_PREFIX]};
        lmass = (float)(log((double)tot) - 40.0 * 0.69314718055994530942);  // log of the kept mass relative to exp(max)
    }
    auto logprob = [&](float s) { return SAMPLED ? (s - kept_test.mx) - lmass : s - lse; };
    const size_t pos = (size_t)b * out_stride + col;
    const int tok = tok_arr[b];
    const float s_tok = lp_token_score<EX>(logits + (size_t)b * ldl, tok, V, seen_prev, b, rep, temp, sx);
    const bool tok_kept = tok >= 0 && tok < V && (!SAMPLED || kept_test(s_tok));
    if (lane == 0) {
        chosen_lp[pos] = tok_kept ? logprob(s_tok) : -INFINITY;
        chosen_rank[pos] = 1 + (int)cnt;
    }
    if (n == 0) return;
    const int n_valid = __popcll(__ballot(lane < n && top.mine != 0));
    if (lane < n) s_ids[lane] = top.mine ? key_id(top.mine) : -1;
    if (lane < n_valid) {
        top_ids[pos * n + lane] = key_id(top.mine);
        top_lp[pos * n + lane] = logprob(key_score(top.mine));
    }
    __syncthreads();
    if (lane == 0 && n_valid < n) {  // fewer than n tokens survive the masks: the masked ones follow at -inf, lowest ids first
        int slot = n_valid;
        for (int id = 0; slot < n && id < V; ++id) {
            bool taken = false;
            for (int q = 0; q < n_valid; ++q) taken |= s_ids[q] == id;
            if (taken) continue;
            top_ids[pos * n + slot] = id;
            top_lp[pos * n + slot] = -INFINITY;
            ++slot;
        }
        for (; slot < n; ++slot) {  // vocabulary smaller than n
            top_ids[pos * n + slot] = -1;
            top_lp[pos * n + slot] = -INFINITY;
        }
    }
}
template <bool SAMPLED>
__global__ __launch_bounds__(64) void lp_final_kernel(const bf16_t* __restrict__ logits, const u64* __restrict__ wsp,
                                                      const u64* __restrict__ recp, int rec_stride, int nblk,
                                                      const int* __restrict__ tok_arr, const uint8_t* __restrict__ seen_prev, int V,
                                                      int ldl, float rep, float temp, int n, float* __restrict__ chosen_lp,
                                                      int* __restrict__ chosen_rank, int* __restrict__ top_ids,
                                                      float* __restrict__ top_lp, int out_stride, int col) {
    lp_final_body<SAMPLED, false>(logits, wsp, recp, rec_stride, nblk, tok_arr, seen_prev, V, ldl, rep, temp, n, chosen_lp, chosen_rank,
                                  top_ids, top_lp, out_stride, col, SampX{});
}
template <bool SAMPLED>
__global__ __launch_bounds__(64) void lp_final_kernel_x(const bf16_t* __restrict__ logits, const u64* __restrict__ wsp,
                                                        const u64* __restrict__ recp, int rec_stride, int nblk,
                                                        const int* __restrict__ tok_arr, const uint8_t* __restrict__ seen_prev, int V,
                                                        int ldl, float rep, float temp, int n, float* __restrict__ chosen_lp,
                                                        int* __restrict__ chosen_rank, int* __restrict__ top_ids,
                                                        float* __restrict__ top_lp, int out_stride, int col, SampX sx) {
    lp_final_body<SAMPLED, true>(logits, wsp, recp, rec_stride, nblk, tok_arr, seen_prev, V, ldl, rep, temp, n, chosen_lp, chosen_rank,
                                 top_ids, top_lp, out_stride, col, sx);
}

}  // namespace

int o3v_sample_top_k_top_p_ex(const void* logits, void* seen, int* cur_tok, int* finished, int* out_ids, float* chosen_logprob,
                               const int* eos_ids, int n_eos, int pad_id, int B, int V, int ldl, float rep_penalty, float temperature,
                               int top_k, float top_p, uint64_t seed, const int* row_id, int step, int out_stride, float* scratch,
                               uint8_t* seen_prev, const o3v_samp_x* sx, hipStream_t stream) {
    if (!logits || !seen || !cur_tok || !finished || !out_ids || !scratch || B < 0 || V <= 0 || step < 0 ||
        step >= out_stride || !(temperature > 0.f) || !(top_p > 0.f) || top_k < 0 || (reinterpret_cast<uintptr_t>(scratch) & 7))
        return O3V_ERR_ARG;
    if (B == 0) return O3V_OK;
    const bf16_t* lg = (const bf16_t*)logits;
    uint8_t* sn = (uint8_t*)seen;
    u64* ws = (u64*)scratch;
    const dim3 grid(NBLK, B), block(NT);
    if (sx) {  // the same passes on the extended row: no added launch
        const SampX x = *sx;
        O3V_KLAUNCH(sample_max_kernel_x, grid, block, 0, stream, lg, sn, ws, V, ldl, rep_penalty, temperature, x);
        if (top_k > 0 && top_k < V) {
            O3V_KLAUNCH((sample_count_kernel_x<0>), grid, block, 0, stream, lg, sn, ws, V, ldl, rep_penalty, temperature, top_k, x);
            O3V_KLAUNCH((sample_count_kernel_x<1>), grid, block, 0, stream, lg, sn, ws, V, ldl, rep_penalty, temperature, top_k, x);
            O3V_KLAUNCH((sample_count_kernel_x<2>), grid, block, 0, stream, lg, sn, ws, V, ldl, rep_penalty, temperature, top_k, x);
            O3V_KLAUNCH(sample_kth_kernel, dim3(B), block, 0, stream, ws, top_k);
        }
        O3V_KLAUNCH((sample_hist_kernel_x<0>), grid, block, 0, stream, lg, sn, ws, V, ldl, rep_penalty, temperature, top_p, x);
        if (top_p < 1.0f) {
            O3V_KLAUNCH((sample_hist_kernel_x<1>), grid, block, 0, stream, lg, sn, ws, V, ldl, rep_penalty, temperature, top_p, x);
            O3V_KLAUNCH((sample_hist_kernel_x<2>), grid, block, 0, stream, lg, sn, ws, V, ldl, rep_penalty, temperature, top_p, x);
        }
        O3V_KLAUNCH(sample_mass_kernel_x, grid, block, 0, stream, lg, sn, ws, V, ldl, rep_penalty, temperature, top_p, x);
        O3V_KLAUNCH(sample_draw_kernel_x, grid, block, 0, stream, lg, sn, ws, cur_tok, finished, out_ids, chosen_logprob, eos_ids,
                    n_eos, pad_id, V, ldl, rep_penalty, temperature, seed, row_id, step, out_stride, seen_prev, x);
        O3V_CHECK_LAUNCH();
        return O3V_OK;
    }
    O3V_KLAUNCH(sample_max_kernel, grid, block, 0, stream, lg, sn, ws, V, ldl, rep_penalty, temperature);
    if (top_k > 0 && top_k < V) {  // TF:591: top_k = min(top_k, vocabulary); k == V removes nothing
        O3V_KLAUNCH((sample_count_kernel<0>), grid, block, 0, stream, lg, sn, ws, V, ldl, rep_penalty, temperature, top_k);
        O3V_KLAUNCH((sample_count_kernel<1>), grid, block, 0, stream, lg, sn, ws, V, ldl, rep_penalty, temperature, top_k);
        O3V_KLAUNCH((sample_count_kernel<2>), grid, block, 0, stream, lg, sn, ws, V, ldl, rep_penalty, temperature, top_k);
        O3V_KLAUNCH(sample_kth_kernel, dim3(B), block, 0, stream, ws, top_k);
    }
    O3V_KLAUNCH((sample_hist_kernel<0>), grid, block, 0, stream, lg, sn, ws, V, ldl, rep_penalty, temperature, top_p);
    if (top_p < 1.0f) {
        O3V_KLAUNCH((sample_hist_kernel<1>), grid, block, 0, stream, lg, sn, ws, V, ldl, rep_penalty, temperature, top_p);
        O3V_KLAUNCH((sample_hist_kernel<2>), grid, block, 0, stream, lg, sn, ws, V, ldl, rep_penalty, temperature, top_p);
    }
    O3V_KLAUNCH(sample_mass_kernel, grid, block, 0, stream, lg, sn, ws, V, ldl, rep_penalty, temperature, top_p);
    O3V_KLAUNCH(sample_draw_kernel, grid, block, 0, stream, lg, sn, ws, cur_tok, finished, out_ids, chosen_logprob, eos_ids, n_eos,
                pad_id, V, ldl, rep_penalty, temperature, seed, row_id, step, out_stride, seen_prev);
    O3V_CHECK_LAUNCH();
    return O3V_OK;
}

extern "C" int o3v_sample_top_k_top_p(const void* logits, void* seen, int* cur_tok, int* finished, int* out_ids,
                                      float* chosen_logprob, const int* eos_ids, int n_eos, int pad_id, int B, int V, int ldl,
                                      float rep_penalty, float temperature, int top_k, float top_p, uint64_t seed,
                                      const int* row_id, int step, int out_stride, float* scratch, hipStream_t stream) {
    return o3v_sample_top_k_top_p_ex(logits, seen, cur_tok, finished, out_ids, chosen_logprob, eos_ids, n_eos, pad_id, B, V, ldl,
                                     rep_penalty, temperature, top_k, top_p, seed, row_id, step, out_stride, scratch, nullptr, nullptr,
                                     stream);
}

extern "C" int o3v_sample_top_p(const void* logits, void* seen, int* cur_tok, int* finished, int* out_ids,
                                float* chosen_logprob, const int* eos_ids, int n_eos, int pad_id, int B, int V, int ldl,
                                float rep_penalty, float temperature, float top_p, uint64_t seed, const int* row_id, int step,
                                int out_stride, float* scratch, hipStream_t stream) {
    return o3v_sample_top_k_top_p(logits, seen, cur_tok, finished, out_ids, chosen_logprob, eos_ids, n_eos, pad_id, B, V, ldl,
                                  rep_penalty, temperature, 0, top_p, seed, row_id, step, out_stride, scratch, stream);
}

// One decode step's sampler exactly as o3v_llm_decode runs it (greedy: penalty + argmax, the embedding row gathered when `embed` is
// given; sampling: the top-k / top-p passes), then the two log-prob launches.  scratch: f32 [B, O3V_SAMPLE_SCRATCH_FLOATS] in both
// modes (the log-prob records sit above what either sampler uses).  sx (optional): the extended controls of this step -- the `_x`
// kernels then, and lp may be NULL (no log-prob launches).
int o3v_sample_lp_step(const void* logits, void* seen, int* cur_tok, int* finished, int* out_ids, float* margins, const int* eos_ids,
                       int n_eos, int pad_id, int B, int V, int ldl, int do_sample, float rep_penalty, float temperature, int top_k,
                       float top_p, uint64_t seed, const int* row_id, int step, int out_stride, float* scratch, const void* embed,
                       void* x_out, int hidden, const o3v_logprob_opts* lp, const o3v_samp_x* sx, hipStream_t stream) {
    if ((!lp && !sx) || !scratch || (reinterpret_cast<uintptr_t>(scratch) & 7) || B > 32 || ldl < V) return O3V_ERR_ARG;
    if (lp && (lp->n < 0 || lp->n > LP_MAXN || !lp->chosen_lp || !lp->chosen_rank || (lp->n > 0 && (!lp->top_ids || !lp->top_lp))))
        return O3V_ERR_ARG;
    u64* ws = (u64*)scratch;
    uint8_t* seen_prev = reinterpret_cast<uint8_t*>(ws + LP_SEEN_PREV);
    SampX x{};
    if (sx) {
        x = *sx;
        x.cnt_prev = reinterpret_cast<uint16_t*>(ws + LP_CNT_PREV);
    }
    if (do_sample) {
        const int rc = o3v_sample_top_k_top_p_ex(logits, seen, cur_tok, finished, out_ids, margins, eos_ids, n_eos, pad_id, B, V, ldl,
                                                 rep_penalty, temperature, top_k, top_p, seed, row_id, step, out_stride, scratch,
                                                 seen_prev, sx ? &x : nullptr, stream);
        if (rc != O3V_OK) return rc;
    } else {
        const int rc = o3v_sample_greedy_ex(logits, seen, cur_tok, finished, out_ids, margins, eos_ids, n_eos, pad_id, B, V, ldl,
                                            rep_penalty, step, out_stride, scratch, embed, x_out, hidden, seen_prev, sx ? &x : nullptr,
                                            stream);
        if (rc != O3V_OK) return rc;
        temperature = 1.0f;  // the greedy sampler applies the penalty only
    }
    if (B == 0 || !lp) return O3V_OK;
    const bf16_t* lg = (const bf16_t*)logits;
    const uint8_t* sn = (const uint8_t*)seen;
    const int rs = WS_FLOATS / 2;
    u64* rec = ws + LP_OFF;
#define LP_ARGS_P lg, sn, ws, rec, rs, NBLK, cur_tok, seen_prev, V, ldl, rep_penalty, temperature, lp->n
#define LP_ARGS_F \
    lg, ws, rec, rs, NBLK, cur_tok, seen_prev, V, ldl, rep_penalty, temperature, lp->n, lp->chosen_lp, lp->chosen_rank, lp->top_ids, \
        lp->top_lp, out_stride, step
    if (sx && do_sample) {
        O3V_KLAUNCH(lp_partial_kernel_x<true>, dim3(NBLK, B), dim3(NT), 0, stream, LP_ARGS_P, x);
        O3V_KLAUNCH(lp_final_kernel_x<true>, dim3(B), dim3(64), 0, stream, LP_ARGS_F, x);
    } else if (sx) {
        O3V_KLAUNCH(lp_partial_kernel_x<false>, dim3(NBLK, B), dim3(NT), 0, stream, LP_ARGS_P, x);
        O3V_KLAUNCH(lp_final_kernel_x<false>, dim3(B), dim3(64), 0, stream, LP_ARGS_F, x);
    } else if (do_sample) {
        O3V_KLAUNCH(lp_partial_kernel<true>, dim3(NBLK, B), dim3(NT), 0, stream, LP_ARGS_P);
        O3V_KLAUNCH(lp_final_kernel<true>, dim3(B), dim3(64), 0, stream, LP_ARGS_F);
    } else {
        O3V_KLAUNCH(lp_partial_kernel<false>, dim3(NBLK, B), dim3(NT), 0, stream, LP_ARGS_P);
        O3V_KLAUNCH(lp_final_kernel<false>, dim3(B), dim3(64), 0, stream, LP_ARGS_F);
    }
#undef LP_ARGS_P
#undef LP_ARGS_F
    O3V_CHECK_LAUNCH();
    return O3V_OK;
}

extern "C" int o3v_sample_logprobs(const void* logits, void* seen, int* cur_tok, int* finished, int* out_ids, float* margins,
                                   const int* eos_ids, int n_eos, int pad_id, int B, int V, int ldl, int do_sample, float rep_penalty,
                                   float temperature, int top_k, float top_p, uint64_t seed, const int* row_id, int step,
                                   int out_stride, float* scratch, const o3v_logprob_opts* lp, hipStream_t stream) {
    if (!lp) return O3V_ERR_ARG;
    return o3v_sample_lp_step(logits, seen, cur_tok, finished, out_ids, margins, eos_ids, n_eos, pad_id, B, V, ldl, do_sample,
                              rep_penalty, temperature, top_k, top_p, seed, row_id, step, out_stride, scratch, nullptr, nullptr, 0, lp,
                              nullptr, stream);
}

// o3v_sampling_opts -> the controls of decode step `step`; O3V_ERR_ARG for what the header rules out (host only, before any launch)
int o3v_sampling_resolve(const o3v_sampling_opts* so, int step, o3v_samp_x* x) {
    if (!so || !x || step < 0) return O3V_ERR_ARG;
    if (!(so->min_p >= 0.f && so->min_p <= 1.f) || !(fabsf(so->presence) <= 2.f) || !(fabsf(so->frequency) <= 2.f) || so->min_tokens < 0)
        return O3V_ERR_ARG;   // (the negated forms refuse NaN)
    if ((so->presence != 0.f || so->frequency != 0.f) && !so->out_counts) return O3V_ERR_ARG;
    if (so->min_tokens > 0 && !so->bias_early) return O3V_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(so->bias) & 15) || (reinterpret_cast<uintptr_t>(so->bias_early) & 15) ||
        (reinterpret_cast<uintptr_t>(so->out_counts) & 15))
        return O3V_ERR_ARG;
    x->bias = step < so->min_tokens ? so->bias_early : so->bias;
    x->counts = so->out_counts;
    x->cnt_prev = nullptr;
    x->pres = so->presence;
    x->freq = so->frequency;
    unsigned bits;
    memcpy(&bits, &so->min_p, 4);
    x->minp_bits = bits;
    x->g_next = nullptr;
    x->g_q = nullptr;
    x->g_qn = nullptr;
    x->g_n = x->g_ldn = 0;
    return O3V_OK;
}

// o3v_guided_opts -> the guide of decode step `step` of B rows over V tokens (V <= 0: the vocabulary is not known yet, the caller
// checks ldn against it later); O3V_ERR_ARG for what the header rules out (host only, before any launch)
int o3v_guided_resolve(const o3v_guided_opts* go, int B, int V, int step, o3v_samp_x* x) {
    if (!go || !x || step < 0 || B < 0) return O3V_ERR_ARG;
    if (!go->next || !go->state || (reinterpret_cast<uintptr_t>(go->next) & 15) || (reinterpret_cast<uintptr_t>(go->state) & 3))
        return O3V_ERR_ARG;
    if (go->n_states <= 0 || go->n_states > 32767 || go->ldn <= 0 || (go->ldn & 7) || (V > 0 && go->ldn < V)) return O3V_ERR_ARG;
    x->g_next = go->next;
    x->g_n = go->n_states;
    x->g_ldn = go->ldn;
    x->g_q = go->state + (size_t)(step & 1) * B;
    x->g_qn = go->state + (size_t)((step + 1) & 1) * B;
    return O3V_OK;
}

extern "C" int o3v_sample_step_ex(const void* logits, void* seen, int* cur_tok, int* finished, int* out_ids, float* margins,
                                  const int* eos_ids, int n_eos, int pad_id, int B, int V, int ldl, int do_sample, float rep_penalty,
                                  float temperature, int top_k, float top_p, uint64_t seed, const int* row_id, int step,
                                  int out_stride, float* scratch, const o3v_logprob_opts* lp, const o3v_sampling_opts* so,
                                  hipStream_t stream) {
    o3v_samp_x x;
    const int rc = o3v_sampling_resolve(so, step, &x);
    if (rc != O3V_OK) return rc;
    return o3v_sample_lp_step(logits, seen, cur_tok, finished, out_ids, margins, eos_ids, n_eos, pad_id, B, V, ldl, do_sample,
                              rep_penalty, temperature, top_k, top_p, seed, row_id, step, out_stride, scratch, nullptr, nullptr, 0, lp,
                              &x, stream);
}

extern "C" int o3v_sample_step_guided(const void* logits, void* seen, int* cur_tok, int* finished, int* out_ids, float* margins,
                                      const int* eos_ids, int n_eos, int pad_id, int B, int V, int ldl, int do_sample, float rep_penalty,
                                      float temperature, int top_k, float top_p, uint64_t seed, const int* row_id, int step,
                                      int out_stride, float* scratch, const o3v_logprob_opts* lp, const o3v_sampling_opts* so,
                                      const o3v_guided_opts* go, hipStream_t stream) {
    if (!go)
        return o3v_sample_step_ex(logits, seen, cur_tok, finished, out_ids, margins, eos_ids, n_eos, pad_id, B, V, ldl, do_sample,
                                  rep_penalty, temperature, top_k, top_p, seed, row_id, step, out_stride, scratch, lp, so, stream);
    const o3v_sampling_opts plain = {};   // a guide alone: the extended kernels on a zeroed control set
    o3v_samp_x x;
    int rc = o3v_sampling_resolve(so ? so : &plain, step, &x);
    if (rc != O3V_OK) return rc;
    if (V <= 0) return O3V_ERR_ARG;
    rc = o3v_guided_resolve(go, B, V, step, &x);
    if (rc != O3V_OK) return rc;
    return o3v_sample_lp_step(logits, seen, cur_tok, finished, out_ids, margins, eos_ids, n_eos, pad_id, B, V, ldl, do_sample,
                              rep_penalty, temperature, top_k, top_p, seed, row_id, step, out_stride, scratch, nullptr, nullptr, 0, lp,
                              &x, stream);
}

extern "C" int o3v_logprobs_rows(const void* logits, const int* target, int R, int V, int ldl, int n, float* target_lp,
                                 int* target_rank, int* top_ids, float* top_lp, float* scratch, hipStream_t stream) {
    if (!logits || !target || !target_lp || !target_rank || R < 0 || R > 65535 || V <= 0 || ldl < V || n < 0 || n > LP_MAXN ||
        (n > 0 && (!top_ids || !top_lp)) || !scratch || (reinterpret_cast<uintptr_t>(scratch) & 7))
        return O3V_ERR_ARG;
    if (R == 0) return O3V_OK;
    const bf16_t* lg = (const bf16_t*)logits;
    u64* rec = (u64*)scratch;
    const int rs = LP_NB_ROWS * LP_REC;
    O3V_KLAUNCH(lp_partial_kernel<false>, dim3(LP_NB_ROWS, R), dim3(NT), 0, stream, lg, nullptr, nullptr, rec, rs, LP_NB_ROWS, target,
                nullptr, V, ldl, 1.0f, 1.0f, n);
    O3V_KLAUNCH(lp_final_kernel<false>, dim3(R), dim3(64), 0, stream, lg, nullptr, rec, rs, LP_NB_ROWS, target, nullptr, V, ldl, 1.0f,
                1.0f, n, target_lp, target_rank, top_ids, top_lp, 1, 0);
    O3V_CHECK_LAUNCH();
    return O3V_OK;
}
