// Host-side runtime of libo3v_hip.so: the layer loops of the Qwen2.5-VL ViT, LLM prefill and decode,
// enqueued kernel by kernel on one HIP stream from C++ (no Python between launches, no allocation, no
// sync -- the whole forward is graph-capturable).  Arithmetic restated from transformers 5.15.0
// models/qwen2_5_vl/modeling_qwen2_5_vl.py (TF:) -- see include/o3v.h for the per-entry citations.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "../../include/o3v.h"
#include "o3v_common.h"

#define TRY(expr)                 \
    do {                          \
        int rc__ = (expr);        \
        if (rc__ != O3V_OK) return rc__; \
    } while (0)

namespace {

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

struct Carver {
    char* base;
    size_t off, cap;
    void* take(size_t bytes) {
        size_t o = off;
        off = align256(off + bytes);
        return off <= cap ? base + o : nullptr;
    }
};

constexpr int SPLITK_MAX_ROWS = 128;   // one row tile: the GEMM grid is N/128 blocks, far fewer than the 256 CUs
constexpr int SPLITK_MAX_N = 8192;

// nn.Linear for any row count: MFMA GEMM above 8 rows, weight-streaming GEMV (in groups of 8 rows) otherwise.
// splitk_ws (optional, SPLITK floats): lets a 9..128-row GEMM with few output tiles split K over more blocks.
int linear(const void* A, const void* W, const void* bias, const void* res, void* out, int M, int N, int K, int lda,
           int ldo, int ldr, int epi, o3v_stream_t s, float* splitk_ws = nullptr, size_t splitk_bytes = 0, int tile = 0) {
    if (M > 8) {
        const int tiles = ((M + 127) / 128) * ((N + 127) / 128);
        if (splitk_ws && M <= SPLITK_MAX_ROWS && N <= SPLITK_MAX_N && tiles < 128 && epi != O3V_EPI_SWIGLU) {
            int splits = 256 / tiles;                       // ~one block per CU
            const int nk = K / 64;
            while (splits > 1 && nk / splits < 4) --splits;  // keep >= 4 k-steps per block
            if (splits > 1 && (size_t)splits * M * N * 4 <= splitk_bytes)
                return o3v_gemm_bf16_splitk(A, W, bias, res, out, M, N, K, lda, K, ldo, ldr, epi, splits, splitk_ws,
                                            splitk_bytes, s);
        }
        return o3v_gemm_bf16_tile(A, W, bias, res, out, M, N, K, lda, K, ldo, ldr, epi, tile, s);
    }
    return o3v_gemv_bf16(A, W, bias, res, out, M, N, K, lda, K, ldo, ldr, epi, s);
}

}  // namespace

extern "C" int o3v_abi_version(void) { return 6; }

// ------------------------------------------------------------------------------------------------ context handle
// Owning host-side copy of the descriptors ("no global mutable state except an explicit o3v_ctx").
#include <new>
#include <vector>
struct o3v_ctx {
    bool has_llm = false, has_vit = false, has_vit3 = false;
    o3v_llm_desc llm{};
    o3v_vit_desc vit{};
    o3v_vit3_desc vit3{};
    std::vector<o3v_llm_layer_w> layers;
    std::vector<o3v_vit_block_w> blocks;
    std::vector<o3v_vit3_block_w> blocks3;
};

extern "C" o3v_ctx* o3v_ctx_create(const o3v_llm_desc* llm, const o3v_vit_desc* vit, const o3v_vit3_desc* vit3) {
    if ((llm && (llm->layers < 0 || (llm->layers > 0 && !llm->layer))) || (vit && (vit->depth < 0 || (vit->depth > 0 && !vit->blocks))) ||
        (vit3 && (vit3->depth < 0 || (vit3->depth > 0 && !vit3->blocks))))
        return nullptr;
    o3v_ctx* c = new (std::nothrow) o3v_ctx();
    if (!c) return nullptr;
    if (llm) {
        c->has_llm = true;
        c->llm = *llm;
        c->layers.assign(llm->layer, llm->layer + llm->layers);
        c->llm.layer = c->layers.data();
    }
    if (vit) {
        c->has_vit = true;
        c->vit = *vit;
        c->blocks.assign(vit->blocks, vit->blocks + vit->depth);
        c->vit.blocks = c->blocks.data();
    }
    if (vit3) {
        c->has_vit3 = true;
        c->vit3 = *vit3;
        c->blocks3.assign(vit3->blocks, vit3->blocks + vit3->depth);
        c->vit3.blocks = c->blocks3.data();
    }
    return c;
}
extern "C" void o3v_ctx_destroy(o3v_ctx* ctx) { delete ctx; }
extern "C" const o3v_llm_desc* o3v_ctx_llm(const o3v_ctx* ctx) { return ctx && ctx->has_llm ? &ctx->llm : nullptr; }
extern "C" const o3v_vit_desc* o3v_ctx_vit(const o3v_ctx* ctx) { return ctx && ctx->has_vit ? &ctx->vit : nullptr; }
extern "C" const o3v_vit3_desc* o3v_ctx_vit3(const o3v_ctx* ctx) { return ctx && ctx->has_vit3 ? &ctx->vit3 : nullptr; }

// ------------------------------------------------------------------------------------------------ ViT
extern "C" size_t o3v_vit_workspace_bytes(const o3v_vit_desc* d, int P) {
    if (!d || P <= 0) return 0;
    const size_t hid = d->hidden, e = 2;
    const size_t Pm = (size_t)P / d->merge_unit;
    size_t n = 0;
    n += align256((size_t)P * hid * e);          // x
    n += align256((size_t)P * hid * e);          // h
    n += align256((size_t)P * 3 * hid * e);      // qkv
    n += align256((size_t)P * hid * e);          // att
    n += align256((size_t)P * d->inter_pad * e); // mlp
    n += align256(Pm * hid * d->merge_unit * e); // m1
    n += align256(Pm * d->out_hidden * e);       // m2
    return n;
}

extern "C" int o3v_vit_forward(const o3v_vit_desc* d, const void* pixels, int P, const int* win_idx, const int* rev_idx,
                               const float* cosT, const float* sinT, const int* tiles_win, int n_tiles_win,
                               const int* tiles_full, int n_tiles_full, void* workspace, size_t ws_bytes, void* out,
                               o3v_stream_t s) {
    if (!d || !pixels || !win_idx || !rev_idx || !cosT || !sinT || !tiles_win || !tiles_full || !workspace || !out)
        return O3V_ERR_ARG;
    if (P <= 0 || d->merge_unit <= 0 || (P % d->merge_unit) || d->heads <= 0 || (d->hidden % d->heads)) return O3V_ERR_ARG;
    if (ws_bytes < o3v_vit_workspace_bytes(d, P)) return O3V_ERR_WORKSPACE;
    const int hid = d->hidden, H = d->heads, D = hid / H, unit = d->merge_unit, Pm = P / unit, ip = d->inter_pad;
    Carver cv{(char*)workspace, 0, ws_bytes};
    char* x = (char*)cv.take((size_t)P * hid * 2);
    char* h = (char*)cv.take((size_t)P * hid * 2);
    char* qkv = (char*)cv.take((size_t)P * 3 * hid * 2);
    char* att = (char*)cv.take((size_t)P * hid * 2);
    char* mlp = (char*)cv.take((size_t)P * ip * 2);
    char* m1 = (char*)cv.take((size_t)Pm * hid * unit * 2);
    char* m2 = (char*)cv.take((size_t)Pm * d->out_hidden * 2);
    if (!m2) return O3V_ERR_WORKSPACE;
    const float scale = 1.0f / sqrtf((float)D);

    // patch embed (Conv3d k=s == GEMM over flattened patches), then window order at merge-unit granularity
    TRY(o3v_gemm_bf16_tile(pixels, d->patch_w, nullptr, nullptr, h, P, hid, d->patch_k_pad, d->patch_k_pad, d->patch_k_pad, hid,
                      0, O3V_EPI_NONE, d->gemm_tile, s));
    TRY(o3v_gather_rows(h, win_idx, x, Pm, unit * hid * 2, s));

    for (int i = 0; i < d->depth; ++i) {
        const o3v_vit_block_w& w = d->blocks[i];
        const bool full = (d->fullatt_mask >> i) & 1;
        TRY(o3v_rmsnorm(x, w.norm1, h, P, hid, hid, hid, 1e-6f, s));
        TRY(o3v_gemm_bf16_tile(h, w.qkv_w, w.qkv_b, nullptr, qkv, P, 3 * hid, hid, hid, hid, 3 * hid, 0, O3V_EPI_NONE, d->gemm_tile, s));
        TRY(o3v_vit_rope(qkv, cosT, sinT, P, H, D, s));
        TRY(o3v_attn_tiles(qkv, qkv + (size_t)hid * 2, qkv + (size_t)2 * hid * 2, att, full ? tiles_full : tiles_win,
                           full ? n_tiles_full : n_tiles_win, 64, H, 1, D, 3L * hid, 3L * hid, D, 0, 3L * hid, D, 0, hid, scale,
                           s));
        TRY(o3v_gemm_bf16_tile(att, w.proj_w, w.proj_b, x, x, P, hid, hid, hid, hid, hid, hid, O3V_EPI_RESIDUAL, d->gemm_tile, s));
        TRY(o3v_rmsnorm(x, w.norm2, h, P, hid, hid, hid, 1e-6f, s));
        TRY(o3v_gemm_bf16_tile(h, w.gu_w, w.gu_b, nullptr, mlp, P, 2 * ip, hid, hid, hid, ip, 0, O3V_EPI_SWIGLU, d->gemm_tile, s));
        TRY(o3v_gemm_bf16_tile(mlp, w.down_w, w.down_b, x, x, P, hid, ip, ip, ip, hid, hid, O3V_EPI_RESIDUAL, d->gemm_tile, s));
    }
    // merger: RMSNorm -> [P/4, 4*hid] -> Linear+GELU -> Linear -> original token order
    TRY(o3v_rmsnorm(x, d->ln_q, h, P, hid, hid, hid, 1e-6f, s));
    const int mh = hid * unit;
    TRY(linear(h, d->m0_w, d->m0_b, nullptr, m1, Pm, mh, mh, mh, mh, 0, O3V_EPI_GELU, s, nullptr, 0, d->gemm_tile));
    TRY(linear(m1, d->m2_w, d->m2_b, nullptr, m2, Pm, d->out_hidden, mh, mh, d->out_hidden, 0, O3V_EPI_NONE, s, nullptr, 0, d->gemm_tile));
    TRY(o3v_gather_rows(m2, rev_idx, out, Pm, d->out_hidden * 2, s));
    return O3V_OK;
}

// ------------------------------------------------------------------------------------------------ ViT, Qwen3-VL
// TF3 = transformers 5.15.0 models/qwen3_vl/modeling_qwen3_vl.py.  Differences from the Qwen2.5-VL tower: patch-embed bias and
// a learned position table (interpolated per grid on the host side, added in the patch GEMM's epilogue), LayerNorm with bias,
// plain fc1 -> GELU(tanh) -> fc2 MLP, full attention inside every temporal patch (no windows, no row permutation), and
// DeepStack: after the blocks in deep_index[] a second kind of merger (LayerNorm over the 4-patch group) taps the stream.
// Heads of 72 dims are stored 80 wide ([36 | 4 zeros | 36 | 4 zeros], weights packed on the host), which keeps the rotary
// halves aligned and reuses the 80-wide attention tiles; the softmax scale stays 72^-1/2.
namespace {
inline int pad64(int n) { return (n + 63) & ~63; }
}

extern "C" size_t o3v_vit3_workspace_bytes(const o3v_vit3_desc* d, int P) {
    if (!d || P <= 0 || d->merge_unit <= 0) return 0;
    const size_t hid = d->hidden, hp = pad64(d->hidden), W = (size_t)d->heads * d->head_dim_pad;
    const size_t Pm = (size_t)P / d->merge_unit, mh = hid * d->merge_unit;
    size_t n = 0;
    n += align256((size_t)P * hid * 2);          // x
    n += align256((size_t)P * hp * 2);           // h (K-padded LayerNorm output)
    n += align256((size_t)P * 3 * W * 2);        // qkv
    n += align256((size_t)P * W * 2);            // att
    n += align256((size_t)P * d->inter_pad * 2); // mlp
    n += align256(Pm * mh * 2);                  // m0
    n += align256(Pm * mh * 2);                  // m1
    return n;
}

namespace {
int vit3_merger(const o3v_vit3_merger_w& m, const char* x, char* m0, char* m1, void* out, int P, int hid, int unit, int out_hidden,
                int tile, o3v_stream_t s) {
    const int Pm = P / unit, mh = hid * unit;
    if (m.postshuffle)
        TRY(o3v_layernorm(x, m.norm_w, m.norm_b, m0, Pm, mh, mh, mh, 1e-6f, s));
    else
        TRY(o3v_layernorm(x, m.norm_w, m.norm_b, m0, P, hid, hid, hid, 1e-6f, s));
    TRY(o3v_gemm_bf16_tile(m0, m.fc1_w, m.fc1_b, nullptr, m1, Pm, mh, mh, mh, mh, mh, 0, O3V_EPI_GELU, tile, s));
    TRY(o3v_gemm_bf16_tile(m1, m.fc2_w, m.fc2_b, nullptr, out, Pm, out_hidden, mh, mh, mh, out_hidden, 0, O3V_EPI_NONE, tile, s));
    return O3V_OK;
}
}  // namespace

extern "C" int o3v_vit3_forward(const o3v_vit3_desc* d, const void* pixels, int P, const void* pos_embed, const float* cosT,
                                const float* sinT, const int* tiles, int n_tiles, void* workspace, size_t ws_bytes, void* out,
                                void* deep_out, o3v_stream_t s) {
    if (!d || !pixels || !pos_embed || !cosT || !sinT || !tiles || !workspace || !out) return O3V_ERR_ARG;
    if (P <= 0 || d->merge_unit <= 0 || (P % d->merge_unit) || d->heads <= 0 || d->n_deep < 0 || d->n_deep > O3V_MAX_DEEPSTACK ||
        (d->n_deep && !deep_out))
        return O3V_ERR_ARG;
    const int hid = d->hidden, hp = pad64(hid), H = d->heads, Dp = d->head_dim_pad, W = H * Dp, unit = d->merge_unit,
              Pm = P / unit, ip = d->inter_pad;
    if ((W % 64) || (ip % 64) || ((hid * unit) % 64) || (hid & 7)) return O3V_ERR_SHAPE;
    if (ws_bytes < o3v_vit3_workspace_bytes(d, P)) return O3V_ERR_WORKSPACE;
    Carver cv{(char*)workspace, 0, ws_bytes};
    char* x = (char*)cv.take((size_t)P * hid * 2);
    char* h = (char*)cv.take((size_t)P * hp * 2);
    char* qkv = (char*)cv.take((size_t)P * 3 * W * 2);
    char* att = (char*)cv.take((size_t)P * W * 2);
    char* mlp = (char*)cv.take((size_t)P * ip * 2);
    char* m0 = (char*)cv.take((size_t)Pm * hid * unit * 2);
    char* m1 = (char*)cv.take((size_t)Pm * hid * unit * 2);
    if (!m1) return O3V_ERR_WORKSPACE;
    const float scale = 1.0f / sqrtf((float)d->head_dim);
    if (hp != hid && hipMemsetAsync(h, 0, (size_t)P * hp * 2, (hipStream_t)s) != hipSuccess) return O3V_ERR_LAUNCH;

    // patch embed: Conv3d(k = s) == GEMM, + bias, + interpolated position rows (TF3:606-640, :700-710)
    TRY(o3v_gemm_bf16_tile(pixels, d->patch_w, d->patch_b, pos_embed, x, P, hid, d->patch_k_pad, d->patch_k_pad, d->patch_k_pad, hid,
                           hid, O3V_EPI_RESIDUAL, d->gemm_tile, s));
    int next_deep = 0;
    for (int i = 0; i < d->depth; ++i) {
        const o3v_vit3_block_w& w = d->blocks[i];
        TRY(o3v_layernorm(x, w.norm1_w, w.norm1_b, h, P, hid, hid, hp, 1e-6f, s));
        TRY(o3v_gemm_bf16_tile(h, w.qkv_w, w.qkv_b, nullptr, qkv, P, 3 * W, hp, hp, hp, 3 * W, 0, O3V_EPI_NONE, d->gemm_tile, s));
        TRY(o3v_vit_rope(qkv, cosT, sinT, P, H, Dp, s));
        TRY(o3v_attn_tiles(qkv, qkv + (size_t)W * 2, qkv + (size_t)2 * W * 2, att, tiles, n_tiles, 64, H, 1, Dp, 3L * W, 3L * W, Dp, 0,
                           3L * W, Dp, 0, W, scale, s));
        TRY(o3v_gemm_bf16_tile(att, w.proj_w, w.proj_b, x, x, P, hid, W, W, W, hid, hid, O3V_EPI_RESIDUAL, d->gemm_tile, s));
        TRY(o3v_layernorm(x, w.norm2_w, w.norm2_b, h, P, hid, hid, hp, 1e-6f, s));
        TRY(o3v_gemm_bf16_tile(h, w.fc1_w, w.fc1_b, nullptr, mlp, P, ip, hp, hp, hp, ip, 0, O3V_EPI_GELU_TANH, d->gemm_tile, s));
        TRY(o3v_gemm_bf16_tile(mlp, w.fc2_w, w.fc2_b, x, x, P, hid, ip, ip, ip, hid, hid, O3V_EPI_RESIDUAL, d->gemm_tile, s));
        if (next_deep < d->n_deep && d->deep_index[next_deep] == i) {
            TRY(vit3_merger(d->deep[next_deep], x, m0, m1, (char*)deep_out + (size_t)next_deep * Pm * d->out_hidden * 2, P, hid, unit,
                            d->out_hidden, d->gemm_tile, s));
            ++next_deep;
        }
    }
    if (next_deep != d->n_deep) return O3V_ERR_ARG;  // deep_index must be ascending and < depth
    return vit3_merger(d->merger, x, m0, m1, out, P, hid, unit, d->out_hidden, d->gemm_tile, s);
}

// ------------------------------------------------------------------------------------------------ LLM
namespace {
// fp32 partials of the widest split-K linear (q/k/v or hidden outputs; gate/up has enough tiles on its own)
size_t splitk_bytes(const o3v_llm_desc* d, int rows) {
    const size_t nq = (size_t)(d->heads + 2 * d->kv_heads) * d->head_dim, nh = d->hidden;
    const size_t n = nq > nh ? nq : nh;
    const size_t tiles = (n + 127) / 128;
    const size_t splits = tiles < 256 ? 256 / tiles + 1 : 1;
    return splits * rows * n * sizeof(float);
}
}  // namespace

extern "C" size_t o3v_llm_workspace_bytes(const o3v_llm_desc* d, int rows) {
    if (!d || rows <= 0) return 0;
    const size_t R = rows, H = d->hidden, QD = (size_t)d->heads * d->head_dim, KD = (size_t)d->kv_heads * d->head_dim;
    size_t n = 0;
    n += align256(R * H * 2);               // h
    n += align256(R * (QD + 2 * KD) * 2);   // qkv
    n += align256(R * QD * 2);              // q (roped)
    n += align256(R * QD * 2);              // att
    n += align256(R * d->inter * 2);        // mlp
    n += align256(R * H * 2);               // normed (head)
    if (rows > 8 && rows <= SPLITK_MAX_ROWS) n += align256(splitk_bytes(d, rows));  // split-K partials of the few-tile GEMMs
    if (d->layer && d->layer[0].gu_w8) {    // fp8 rows present: room for the W8A8 prefill (o3v_prefill_opts.w8a8)
        n += align256(R * (H > QD ? H : QD));   // a8: fp8 activations of the q/k/v, o and gate/up linears
        n += align256(R * d->inter);            // m8: fp8 SwiGLU output
        n += align256(R * sizeof(float));       // per-row scales
    }
    return n;
}

namespace {
struct LlmWs {
    char *h, *qkv, *q, *att, *mlp, *normed;
    float* splitk;
    size_t splitk_bytes;
    char *a8 = nullptr, *m8 = nullptr;  // W8A8 prefill only
    float* sa = nullptr;
};
bool carve_llm(const o3v_llm_desc* d, int rows, void* ws, size_t bytes, LlmWs& w) {
    const size_t R = rows, H = d->hidden, QD = (size_t)d->heads * d->head_dim, KD = (size_t)d->kv_heads * d->head_dim;
    Carver cv{(char*)ws, 0, bytes};
    w.h = (char*)cv.take(R * H * 2);
    w.qkv = (char*)cv.take(R * (QD + 2 * KD) * 2);
    w.q = (char*)cv.take(R * QD * 2);
    w.att = (char*)cv.take(R * QD * 2);
    w.mlp = (char*)cv.take(R * d->inter * 2);
    w.normed = (char*)cv.take(R * H * 2);
    w.splitk = nullptr;
    w.splitk_bytes = 0;
    if (rows > 8 && rows <= SPLITK_MAX_ROWS) {
        w.splitk_bytes = splitk_bytes(d, rows);
        w.splitk = (float*)cv.take(w.splitk_bytes);
        if (!w.splitk) return false;
    }
    if (d->layer && d->layer[0].gu_w8) {
        w.a8 = (char*)cv.take(R * (H > QD ? H : QD));
        w.m8 = (char*)cv.take(R * d->inter);
        w.sa = (float*)cv.take(R * sizeof(float));
        if (!w.sa) return false;
    }
    return w.normed != nullptr;
}
}  // namespace

extern "C" int o3v_llm_prefill(const o3v_llm_desc* d, void* x, const void* cosT, const void* sinT, const int* tiles,
                               int n_tiles, int rows_per_tile, void* kcache, void* vcache, int B, int S, int past,
                               int Tmax, void* workspace, size_t ws_bytes, o3v_stream_t s) {
    return o3v_llm_prefill_ex(d, x, cosT, sinT, tiles, n_tiles, rows_per_tile, kcache, vcache, B, S, past, Tmax, nullptr, workspace,
                              ws_bytes, s);
}

// opts (may be NULL), see o3v_prefill_opts in include/o3v.h:
//  * DeepStack (TF3:839-862): after decoder layer l < n_deep, x[ds_rows[i]] += ds_feat[l][ds_src[i]] for the n_ds visual rows.
//  * shared prompt entry: the first prefix_len of the `past` tokens live ONCE per prompt in kprefix / vprefix; kcache / vcache
//    then hold only the tokens behind them (the S new ones land in slots past - prefix_len ..).
extern "C" int o3v_llm_prefill_ex(const o3v_llm_desc* d, void* x, const void* cosT, const void* sinT, const int* tiles, int n_tiles,
                                  int rows_per_tile, void* kcache, void* vcache, int B, int S, int past, int Tmax,
                                  const o3v_prefill_opts* opts, void* workspace, size_t ws_bytes, o3v_stream_t s) {
    if (!d || !x || !cosT || !sinT || !tiles || !kcache || !vcache || !workspace) return O3V_ERR_ARG;
    const o3v_prefill_opts none = {};
    const o3v_prefill_opts& o = opts ? *opts : none;
    const int n_ds = o.n_ds, n_deep = o.n_deep;
    if (n_ds < 0 || n_deep < 0 || (n_ds > 0 && n_deep > 0 && (!o.ds_rows || !o.ds_src || !o.ds_feat))) return O3V_ERR_ARG;
    const bool pfx = o.kprefix != nullptr;
    if (pfx && (!o.vprefix || o.prefix_len <= 0 || o.prefix_len > past || o.prefix_len > o.prefix_cap || o.rows_per_prefix <= 0 ||
                (B % o.rows_per_prefix)))
        return O3V_ERR_ARG;
    const int own_past = pfx ? past - o.prefix_len : past;  // tokens already in this call's own caches
    if (B <= 0 || S <= 0 || past < 0 || own_past + S > Tmax || d->kv_heads <= 0 || (d->heads % d->kv_heads)) return O3V_ERR_ARG;
    const int rows = B * S, H = d->hidden, Hq = d->heads, Hkv = d->kv_heads, D = d->head_dim, I = d->inter;
    const int QD = Hq * D, NQKV = (Hq + 2 * Hkv) * D;
    LlmWs w;
    if (ws_bytes < o3v_llm_workspace_bytes(d, rows) || !carve_llm(d, rows, workspace, ws_bytes, w)) return O3V_ERR_WORKSPACE;
    const float scale = 1.0f / sqrtf((float)D);
    const size_t layer_stride = (size_t)B * Hkv * Tmax * D * 2;
    const size_t pre_stride = pfx ? (size_t)(B / o.rows_per_prefix) * Hkv * o.prefix_cap * D * 2 : 0;
    const long p_hs = (long)o.prefix_cap * D, p_bs = (long)Hkv * o.prefix_cap * D;
    // W8A8 (opt-in): the four linears of every layer as fp8 x fp8 on the matrix cores -- activations quantised per token on the fly
    // (the RMSNorm kernels emit fp8 + a row scale directly), weights = the fp8 rows of the decode; whole 128-byte k-tiles only
    const bool w8a8 = o.w8a8 && w.sa && d->layer[0].qkv_w8 && d->layer[0].o_w8 && d->layer[0].gu_w8 && d->layer[0].down_w8 &&
                      (H % 128) == 0 && (QD % 128) == 0 && (I % 128) == 0;  // any row count: a log-prob must not depend on its chunk's size
    if (o.w8a8 && !w8a8 && o.w8a8 > 1) return O3V_ERR_SHAPE;  // w8a8 = 2: required, not merely preferred
    for (int l = 0; l < d->layers; ++l) {
        const o3v_llm_layer_w& lw = d->layer[l];
        char* kc = (char*)kcache + l * layer_stride;
        char* vc = (char*)vcache + l * layer_stride;
        const char* kp = pfx ? (const char*)o.kprefix + l * pre_stride : nullptr;
        const char* vp = pfx ? (const char*)o.vprefix + l * pre_stride : nullptr;
        if (w8a8) {
            TRY(o3v_rmsnorm_quantize_fp8(x, lw.ln1, w.a8, w.sa, rows, H, H, H, d->rms_eps, s));
            TRY(o3v_gemm_fp8(w.a8, w.sa, lw.qkv_w8, lw.qkv_s, lw.qkv_b, nullptr, w.qkv, rows, NQKV, H, H, H, NQKV, 0, O3V_EPI_NONE, s));
        } else {
            TRY(o3v_rmsnorm(x, lw.ln1, w.h, rows, H, H, H, d->rms_eps, s));
            TRY(linear(w.h, lw.qkv_w, lw.qkv_b, nullptr, w.qkv, rows, NQKV, H, H, NQKV, 0, O3V_EPI_NONE, s, w.splitk, w.splitk_bytes, d->gemm_tile));
        }
        if (lw.q_norm)
            TRY(o3v_qkv_norm_rope_cache(w.qkv, lw.q_norm, lw.k_norm, d->rms_eps, cosT, sinT, w.q, kc, vc, own_past, rows, S, Hq, Hkv, D,
                                        Tmax, S, 0, s));
        else
            TRY(o3v_qkv_rope_cache(w.qkv, cosT, sinT, w.q, kc, vc, own_past, rows, S, Hq, Hkv, D, Tmax, S, 0, s));
        TRY(o3v_attn_tiles_prefix(w.q, kc, vc, kp, vp, p_hs, p_bs, o.prefix_len, pfx ? o.rows_per_prefix : 1, w.att, tiles, n_tiles,
                                  rows_per_tile, Hq, Hq / Hkv, D, QD, D, (long)Tmax * D, (long)Hkv * Tmax * D, D, (long)Tmax * D,
                                  (long)Hkv * Tmax * D, QD, scale, s));
        if (w8a8) {
            TRY(o3v_quantize_rows_fp8(w.att, w.a8, w.sa, rows, QD, QD, QD, s));
            TRY(o3v_gemm_fp8(w.a8, w.sa, lw.o_w8, lw.o_s, nullptr, x, x, rows, H, QD, QD, QD, H, H, O3V_EPI_RESIDUAL, s));
            TRY(o3v_rmsnorm_quantize_fp8(x, lw.ln2, w.a8, w.sa, rows, H, H, H, d->rms_eps, s));
            TRY(o3v_gemm_fp8(w.a8, w.sa, lw.gu_w8, lw.gu_s, nullptr, nullptr, w.mlp, rows, 2 * I, H, H, H, I, 0, O3V_EPI_SWIGLU, s));
            TRY(o3v_quantize_rows_fp8(w.mlp, w.m8, w.sa, rows, I, I, I, s));
            TRY(o3v_gemm_fp8(w.m8, w.sa, lw.down_w8, lw.down_s, nullptr, x, x, rows, H, I, I, I, H, H, O3V_EPI_RESIDUAL, s));
        } else {
            TRY(linear(w.att, lw.o_w, nullptr, x, x, rows, H, QD, QD, H, H, O3V_EPI_RESIDUAL, s, w.splitk, w.splitk_bytes, d->gemm_tile));
            TRY(o3v_rmsnorm(x, lw.ln2, w.h, rows, H, H, H, d->rms_eps, s));
            TRY(linear(w.h, lw.gu_w, nullptr, nullptr, w.mlp, rows, 2 * I, H, H, I, 0, O3V_EPI_SWIGLU, s, nullptr, 0, d->gemm_tile));
            TRY(linear(w.mlp, lw.down_w, nullptr, x, x, rows, H, I, I, H, H, O3V_EPI_RESIDUAL, s, w.splitk, w.splitk_bytes, d->gemm_tile));
        }
        if (l < n_deep && n_ds > 0)
            TRY(o3v_add_rows(x, o.ds_rows, o.ds_src, (const char*)o.ds_feat + (size_t)l * o.ds_stride * 2, n_ds, H, s));
    }
    return O3V_OK;
}

namespace {
// what the decode linears stream: bf16, fp8 rows (<= 3 rows), fp8 fragments (4..32 rows); the MLP alone: MXFP4 rows / fragments
enum Weights { W_BF16, W_FP8_ROWS, W_FP8_FRAGS, W_MXFP4_ROWS, W_MXFP4_FRAGS };
int llm_head(const o3v_llm_desc* d, const void* x, int ldx, int rows, void* normed, void* logits, Weights wf, o3v_stream_t s) {
    if (!d || !x || !normed || !logits || rows <= 0) return O3V_ERR_ARG;
    const int H = d->hidden;
    if (wf == W_FP8_FRAGS && rows >= 4 && rows <= 32 && d->lm_head8p) {  // batched decode on fp8 rows: norm apart, fp8 fragments widened in registers
        TRY(o3v_rmsnorm(x, d->final_norm, normed, rows, H, ldx, H, d->rms_eps, s));
        return o3v_linear_decode_fp8_rows(normed, d->lm_head8p, d->lm_head_s, nullptr, nullptr, logits, rows, d->vocab, H, H, d->vocab, 0,
                                          O3V_EPI_NONE, s);
    }
    if (rows >= 8 && rows <= 32 && d->lm_head_p) {  // batched decode: norm apart, LDS-free matrix-core linear
        TRY(o3v_rmsnorm(x, d->final_norm, normed, rows, H, ldx, H, d->rms_eps, s));
        return o3v_linear_decode(normed, nullptr, 0.f, d->lm_head, d->lm_head_p, nullptr, nullptr, logits, rows, d->vocab, H, H,
                                 d->vocab, 0, O3V_EPI_NONE, s);
    }
    if (wf == W_FP8_ROWS && rows <= 3 && d->lm_head8)  // fp8 head (decode with fp8 weights): half the 1.09 GB
        return o3v_linear_decode_fp8(x, d->final_norm, d->rms_eps, d->lm_head8, d->lm_head_s, nullptr, nullptr, logits, rows,
                                     d->vocab, H, ldx, d->vocab, 0, O3V_EPI_NONE, s);
    if (rows <= 8)  // decode / last-token head: RMSNorm fused into the weight-streaming GEMV
        return o3v_linear_decode(x, d->final_norm, d->rms_eps, d->lm_head, d->lm_head_p, nullptr, nullptr, logits, rows,
                                 d->vocab, H, ldx, d->vocab, 0, O3V_EPI_NONE, s);
    TRY(o3v_rmsnorm(x, d->final_norm, normed, rows, H, ldx, H, d->rms_eps, s));
    return linear(normed, d->lm_head, nullptr, nullptr, logits, rows, d->vocab, H, H, d->vocab, 0, O3V_EPI_NONE, s);  // > 8 rows: one MFMA GEMM
}
}  // namespace

// bf16 weights always: the head of the prefill, of forward_logits and of the log-prob pass (R:grpo_trainer.py:371-384) -- the fp8
// rows are DECODE rows (o3v_llm_decode streams them), a log-prob must not depend on how many rows its chunk happens to hold
extern "C" int o3v_llm_head(const o3v_llm_desc* d, const void* x, int ldx, int rows, void* normed, void* logits,
                            o3v_stream_t s) {
    return llm_head(d, x, ldx, rows, normed, logits, W_BF16, s);
}

// o3v_sample.hip: the sampler of one step followed by its log-probs
int o3v_sample_lp_step(const void* logits, void* seen, int* cur_tok, int* finished, int* out_ids, float* margins, const int* eos_ids,
                       int n_eos, int pad_id, int B, int V, int ldl, int do_sample, float rep_penalty, float temperature, int top_k,
                       float top_p, uint64_t seed, const int* row_id, int step, int out_stride, float* scratch, const void* embed,
                       void* x_out, int hidden, const o3v_logprob_opts* lp, const o3v_samp_x* sx, hipStream_t stream);
int o3v_sampling_resolve(const o3v_sampling_opts* so, int step, o3v_samp_x* x);
int o3v_guided_resolve(const o3v_guided_opts* go, int B, int V, int step, o3v_samp_x* x);

extern "C" int o3v_llm_decode(const o3v_llm_desc* d, const o3v_decode_state* st, int step0, int n_steps,
                              int skip_last_forward, o3v_stream_t s) {
    return o3v_llm_decode_ex(d, st, nullptr, nullptr, step0, n_steps, skip_last_forward, s);
}

extern "C" int o3v_llm_decode_lp(const o3v_llm_desc* d, const o3v_decode_state* st, const o3v_logprob_opts* lp, int step0,
                                 int n_steps, int skip_last_forward, o3v_stream_t s) {
    return o3v_llm_decode_ex(d, st, lp, nullptr, step0, n_steps, skip_last_forward, s);
}

namespace {
// Which kernels the steps of one decode call launch; layer 0's weights speak for the stack.  Set and explained in decide_regime().
struct Regime {
    Weights weights, qkv_weights, mlp_weights;        // of the linears; of q/k/v; of gate/up and down_proj
    bool norm_apart, qkv_fused_norm, qk_norm, group;  // fixed for the call
    bool kv8, kv8_emulate;                            // fp8 K/V cache; its arithmetic emulated on a bf16 cache (tests)
    bool ragged;                                      // a context per row (row_base): staging rows, o3v_attn_decode_ragged
    const int* own_lo;                                // group rows with left-padded suffixes in their own caches: the gap mask, else NULL
    bool block;                                       // tried, may fall back: see settle()
};
// The one-launch attention block is tried and may fall back: O3V_ERR_SHAPE from its FIRST launch in a call (layer 0 of the first step)
// switches it off for the rest of the call; any other non-OK code, and O3V_ERR_SHAPE later on, is returned.  Every such condition of
// o3v_decode_attn_block* is a constant of the call (shapes, device, residency).
int settle(bool& on, bool first, int rc) {
    if (rc != O3V_ERR_SHAPE || !first) return rc;
    on = false;
    return O3V_OK;
}
// the only reader of st->flags, st->sync, st->group and of the fp8 / fragment / q_norm pointers for the choice of kernels
Regime decide_regime(const o3v_llm_desc* d, const o3v_decode_state* st) {
    const int B = st->B, H = d->hidden;
    const o3v_llm_layer_w& l0 = d->layer[0];
    Regime r;
    // B >= 4 rows run on the matrix-core linears, which stage the normalised x of a fused RMSNorm in LDS (57 KB at B=8, 115 KB
    // at B=16: two blocks, then one, per CU).  With a separate 3 us norm launch the linears are LDS-free: gate/up 54 -> 44 us
    // at B=8, 75 -> 50 us at B=16 (profiles/r01_m8_linear.txt).  Whole step, 7B: B=4 3.56 -> 3.61 ms (worse: two more
    // launches per layer), B=8 4.04 -> 3.97, B=16 5.63 -> 5.25: taken from B=8 on.
    r.norm_apart = B >= 8;  // (above 16 rows the linears take no fused norm at all)
    // ... except q/k/v at 8 rows: its grid is ~1 workgroup per CU (288 at 7B), so the LDS the fused norm stages x in costs no
    // residency, and the prologue replaces a 5.9 us launch.  Same sums, same rounding as o3v_rmsnorm: bit-identical.  Measured
    // (7B, G rows of one prompt, ms/step fused | apart): G=8 3.721 | 3.768, G=16 4.365 | 4.312 -- taken at 8 rows only.
    r.qkv_fused_norm = r.norm_apart && B <= 8 && !(st->flags & O3V_DECODE_NO_QKV_FUSED_NORM) && (size_t)B * (H * 2 + 16) <= 144 * 1024;
    // fp8 weights (batch <= 3): every decode linear streams the fp8 copy
    const bool fp8 = B <= 3 && l0.qkv_w8 && l0.o_w8 && l0.gu_w8 && l0.down_w8 && st->group <= 1;
    // fp8 rows at 4..32 rows (BASELINE config #5: N = 16 chains on fp8 weights): norms run apart, the linears stream the
    // fragment-major fp8 images
    const bool fp8b = B >= 4 && l0.gu_w8p && l0.down_w8p && l0.o_w8p;
    r.weights = fp8 ? W_FP8_ROWS : fp8b ? W_FP8_FRAGS : W_BF16;
    r.qkv_weights = fp8b && !l0.qkv_w8p ? W_BF16 : r.weights;  // (without a fragment image of its own q/k/v stays on the bf16 weights)
    // MXFP4 images of the MLP (opt-in, beside the fp8 copies): gate/up and down_proj stream them wherever the call runs on fp8 rows /
    // fp8 fragments and BOTH matrices have the image of that form; nothing else of the regime changes (norms, q/k/v, o_proj, the
    // one-launch attention block and the head are those of the fp8 call).  A matrix without the image (K no multiple of 128 for the
    // fragments) leaves the whole MLP on r.weights.
    r.mlp_weights = r.weights;
    if (r.weights == W_FP8_ROWS && l0.gu_w4 && l0.down_w4 && l0.gu_s4 && l0.down_s4) r.mlp_weights = W_MXFP4_ROWS;
    if (r.weights == W_FP8_FRAGS && l0.gu_w4p && l0.down_w4p && l0.gu_s4p && l0.down_s4p) r.mlp_weights = W_MXFP4_FRAGS;
    r.qk_norm = l0.q_norm != nullptr;  // Qwen3-VL: per-head RMSNorm between the q/k/v linear and the rotation
    r.group = st->group > 1;           // the rows of a group share the prompt K/V: read it once per group
    // batch 1: q/k/v + attention + merge + o_proj as ONE launch (o3v_fused.hip); epoch = index of the launch in this generate call
    r.block = st->sync && B == 1 && st->group <= 1 && st->nsplit > 0;
    // fp8 K/V (independent rows only; o3v_llm_decode_ex refuses it for groups): q/k/v writes the new token's bf16 K/V rows into one
    // layer's worth of staging rows, the attention kernel quantises them into the cache -- stand-alone launches, no one-launch form.
    // The emulation (tests) round-trips the new token's row of an ordinary bf16 cache after q/k/v instead.
    r.kv8 = st->k8 != nullptr;
    r.kv8_emulate = !r.kv8 && (st->flags & O3V_DECODE_KV8_EMULATE);
    if (r.kv8 || r.kv8_emulate) r.block = false;
    // ragged rows (continuous batching; the three fields exist only behind O3V_DECODE_RAGGED): q/k/v writes the staging rows as under
    // kv8, the attention kernel appends them at each row's own slot -- stand-alone launches
    r.ragged = (st->flags & O3V_DECODE_RAGGED) && st->row_base != nullptr;
    if (r.ragged) r.block = false;
    // suffixes behind a shared prefix (o3v_llm_decode_ex has checked that this is a group on a prompt entry): the group kernels mask
    // each row's padding slots; NULL launches the kernels of before
    r.own_lo = r.group ? st->own_lo : nullptr;
    return r;
}

// One decode call: its regime and what its step functions share (workspace, dimensions, strides, the running step)
struct Decode {
    const o3v_llm_desc* d;
    const o3v_decode_state* st;
    o3v_stream_t s;
    Regime r;
    // host_stats (optional, host memory): [0] += decode forwards, [1] += kernel launches inside their layer loops, [2] += layers whose
    // attention half ran as the one-launch block, [3] += layers whose attention half ran on the stand-alone kernels
    long long* hs;
    int step0, step, B, H, Hq, Hkv, D, I, V, QD, NQKV, slot0;
    LlmWs w;
    float scale;
    size_t layer_stride, pre_stride;
    // where q/k/v appends the new token's K/V: slot slot0 + step of layer l's cache; fp8 K/V: the staging rows [B][Hkv][1][D]
    // ragged rows: the staging rows kstage / vstage likewise
    char* kc(int l) const { return r.ragged ? (char*)st->kstage : (char*)st->kcache + (r.kv8 ? 0 : l * layer_stride); }
    char* vc(int l) const { return r.ragged ? (char*)st->vstage : (char*)st->vcache + (r.kv8 ? 0 : l * layer_stride); }
    int kv_slot() const { return r.kv8 || r.ragged ? 0 : slot0 + step; }
    int kv_cap() const { return r.kv8 || r.ragged ? 1 : st->Tmax; }
    uint32_t epoch(int l) const { return (uint32_t)(step * d->layers + l + 1); }  // of the one-launch block
    bool first(int l) const { return l == 0 && step == step0; }                   // the launch at which settle() may switch it off
    int sample(const o3v_logprob_opts* lp, const o3v_sampling_opts* so, const o3v_guided_opts* go) {
        // so: the extended sampler kernels on this step's controls, then (lp given) its log-probs
        // lp alone: the same sampler, then the log-probs of what it drew (sampling: the embedding row is gathered below as usual)
        // go: the extended kernels with the guide's mask and state (on a zeroed control set when so is NULL)
        static const o3v_sampling_opts plain = {};
        if (go && !so) so = &plain;
        o3v_samp_x sx;
        if (so) TRY(o3v_sampling_resolve(so, step, &sx));
        if (go) TRY(o3v_guided_resolve(go, B, V, step, &sx));
        if (so || lp)
            return o3v_sample_lp_step(st->logits, st->seen, st->cur_tok, st->finished, st->out_ids, st->margins, st->eos_ids, st->n_eos,
                                      st->pad_id, B, V, V, st->do_sample, st->rep_penalty, st->temperature, st->top_k, st->top_p, st->seed,
                                      st->row_id, step, st->Tnew, st->sample_scratch, st->do_sample ? nullptr : d->embed, st->x, H, lp,
                                      so ? &sx : nullptr, s);
        if (st->do_sample)
            return o3v_sample_top_k_top_p(st->logits, st->seen, st->cur_tok, st->finished, st->out_ids, st->margins, st->eos_ids,
                                          st->n_eos, st->pad_id, B, V, V, st->rep_penalty, st->temperature, st->top_k, st->top_p,
                                          st->seed, st->row_id, step, st->Tnew, st->sample_scratch, s);
        // greedy: the chosen token's embedding row is gathered by the sampler's last stage
        return o3v_sample_greedy_embed(st->logits, st->seen, st->cur_tok, st->finished, st->out_ids, st->margins, st->eos_ids,
                                       st->n_eos, st->pad_id, B, V, V, st->rep_penalty, step, st->Tnew, st->sample_scratch,
                                       d->embed, st->x, H, s);
    }
    // one decode linear [B,K] -> [B,N] on the weight form wf (W / Wp, W8 + sc, W8p + sc); O3V_EPI_RESIDUAL adds to x.  ln given: the
    // RMSNorm of X is fused -- never on fp8 fragments, whose X arrives normalised
    int lin(Weights wf, const void* X, const void* ln, const void* W, const void* Wp, const void* W8, const void* W8p, const float* sc,
            const void* bias, void* out, int N, int K, int ldo, int epi) {
        const void* res = epi == O3V_EPI_RESIDUAL ? st->x : nullptr;
        const float eps = ln ? d->rms_eps : 0.f;
        if (wf == W_FP8_ROWS) return o3v_linear_decode_fp8(X, ln, eps, W8, sc, bias, res, out, B, N, K, K, ldo, res ? H : 0, epi, s);
        if (wf == W_FP8_FRAGS) return o3v_linear_decode_fp8_rows(X, W8p, sc, bias, res, out, B, N, K, K, ldo, res ? H : 0, epi, s);
        return o3v_linear_decode(X, ln, eps, W, Wp, bias, res, out, B, N, K, K, ldo, res ? H : 0, epi, s);
    }
    // one MLP linear on the MXFP4 images (rows: W4 / S4 row-major, ln may be fused; fragments: X arrives normalised)
    int lin4(Weights wf, const void* X, const void* ln, const void* W4, const void* S4, void* out, int N, int K, int ldo, int epi) {
        const void* res = epi == O3V_EPI_RESIDUAL ? st->x : nullptr;
        if (wf == W_MXFP4_ROWS)
            return o3v_linear_decode_mxfp4(X, ln, ln ? d->rms_eps : 0.f, W4, S4, nullptr, res, out, B, N, K, K, ldo, res ? H : 0, epi, s);
        return o3v_linear_decode_mxfp4_rows(X, W4, S4, nullptr, res, out, B, N, K, K, ldo, res ? H : 0, epi, s);
    }
    // q/k/v (+norm, rope, cache append) of layer l
    int qkv(int l, const o3v_llm_layer_w& lw) {
        const Weights wf = r.qkv_weights;
        // the norm in front as a launch of its own: always on fp8 fragments; on bf16 rows where norms run apart
        const bool apart = wf == W_FP8_FRAGS || (r.norm_apart && !r.qkv_fused_norm);
        if (apart) TRY(o3v_rmsnorm(st->x, lw.ln1, w.h, B, H, H, H, d->rms_eps, s));
        const void *xin = apart ? w.h : st->x, *ln = apart ? nullptr : lw.ln1;  // normalised x, or x and the norm to fuse
        if (r.qk_norm) {
            TRY(lin(wf, xin, ln, lw.qkv_w, lw.qkv_wp, lw.qkv_w8, lw.qkv_w8p, lw.qkv_s, lw.qkv_b, w.qkv, NQKV, H, NQKV, O3V_EPI_NONE));
            return o3v_qkv_norm_rope_cache(w.qkv, lw.q_norm, lw.k_norm, d->rms_eps, st->cosT, st->sinT, w.q, kc(l), vc(l), kv_slot(), B, 1,
                                           Hq, Hkv, D, kv_cap(), st->Tnew, step, s);
        }
        if (wf == W_FP8_FRAGS)
            return o3v_qkv_rope_fp8_rows(w.h, lw.qkv_w8p, lw.qkv_s, lw.qkv_b, B, H, H, st->cosT, st->sinT, w.q, kc(l), vc(l), kv_slot(), Hq,
                                         Hkv, D, kv_cap(), st->Tnew, step, s);
        if (wf == W_FP8_ROWS)
            return o3v_gemv_norm_qkv_rope_fp8(st->x, lw.ln1, d->rms_eps, lw.qkv_w8, lw.qkv_s, lw.qkv_b, B, H, H, st->cosT, st->sinT, w.q,
                                              kc(l), vc(l), kv_slot(), Hq, Hkv, D, kv_cap(), st->Tnew, step, s);
        return o3v_gemv_norm_qkv_rope(xin, ln, ln ? d->rms_eps : 0.f, lw.qkv_w, lw.qkv_wp, lw.qkv_b, B, H, H, st->cosT, st->sinT, w.q, kc(l),
                                      vc(l), kv_slot(), Hq, Hkv, D, kv_cap(), st->Tnew, step, s);
    }
    // attention + merge of layer l on the stand-alone kernels
    int attention(int l) {
        if (r.ragged)
            return o3v_attn_decode_ragged(w.q, (char*)st->kcache + l * layer_stride, (char*)st->vcache + l * layer_stride, st->kstage,
                                          st->vstage, w.att, st->part_o, st->part_ml, st->row_base, step, B, Hq, Hkv, D, st->Tmax,
                                          st->nsplit, scale, s);
        if (r.kv8) {
            const size_t rows = (size_t)l * B * Hkv * st->Tmax;  // (token, kv head) rows of the layers before l
            return o3v_attn_decode_kv8(w.q, (char*)st->k8 + rows * D, (char*)st->v8 + rows * D, st->k8s + rows, st->v8s + rows, st->kcache,
                                       st->vcache, w.att, st->part_o, st->part_ml, st->k_lo, B, Hq, Hkv, D, st->S + step + 1, st->Tmax,
                                       st->nsplit, scale, s);
        }
        if (r.kv8_emulate) TRY(o3v_kv8_roundtrip(kc(l), vc(l), (long)B * Hkv, st->Tmax, slot0 + step, 1, D, s));
        if (r.group)
            return o3v_attn_decode_group_prefix_lo(w.q, kc(l), vc(l), st->kprefix ? (const char*)st->kprefix + l * pre_stride : nullptr,
                                                   st->kprefix ? (const char*)st->vprefix + l * pre_stride : nullptr, st->prefix_cap,
                                                   st->rows_per_prompt, w.att, st->part_o, st->part_ml, st->k_lo, r.own_lo, B, st->group,
                                                   Hq, Hkv, D, st->S, st->S + st->own_past + step + 1, st->Tmax, st->nsplit, scale, s);
        return o3v_attn_decode(w.q, kc(l), vc(l), w.att, st->part_o, st->part_ml, st->k_lo, B, Hq, Hkv, D, st->S + step + 1, st->Tmax,
                               st->nsplit, scale, s);
    }
    // o_proj + residual
    int o_proj(const o3v_llm_layer_w& lw) {
        return lin(r.weights, w.att, nullptr, lw.o_w, lw.o_wp, lw.o_w8, lw.o_w8p, lw.o_s, nullptr, st->x, H, QD, H, O3V_EPI_RESIDUAL);
    }
    // MLP half of a layer: (norm,) gate/up + SwiGLU, down_proj + residual
    int mlp(const o3v_llm_layer_w& lw) {
        const bool apart = r.weights == W_FP8_FRAGS || r.norm_apart;
        if (apart) TRY(o3v_rmsnorm(st->x, lw.ln2, w.h, B, H, H, H, d->rms_eps, s));
        const void *xin = apart ? w.h : st->x, *ln = apart ? nullptr : lw.ln2;
        if (r.mlp_weights == W_MXFP4_ROWS)
            TRY(lin4(W_MXFP4_ROWS, xin, ln, lw.gu_w4, lw.gu_s4, w.mlp, 2 * I, H, I, O3V_EPI_SWIGLU));
        else if (r.mlp_weights == W_MXFP4_FRAGS)
            TRY(lin4(W_MXFP4_FRAGS, xin, ln, lw.gu_w4p, lw.gu_s4p, w.mlp, 2 * I, H, I, O3V_EPI_SWIGLU));
        else
            TRY(lin(r.weights, xin, ln, lw.gu_w, lw.gu_wp, lw.gu_w8, lw.gu_w8p, lw.gu_s, nullptr, w.mlp, 2 * I, H, I, O3V_EPI_SWIGLU));
        return down_proj(lw);
    }
    int down_proj(const o3v_llm_layer_w& lw) {
        if (r.mlp_weights == W_MXFP4_ROWS) return lin4(W_MXFP4_ROWS, w.mlp, nullptr, lw.down_w4, lw.down_s4, st->x, H, I, H, O3V_EPI_RESIDUAL);
        if (r.mlp_weights == W_MXFP4_FRAGS) return lin4(W_MXFP4_FRAGS, w.mlp, nullptr, lw.down_w4p, lw.down_s4p, st->x, H, I, H, O3V_EPI_RESIDUAL);
        return lin(r.weights, w.mlp, nullptr, lw.down_w, lw.down_wp, lw.down_w8, lw.down_w8p, lw.down_s, nullptr, st->x, H, I, H,
                   O3V_EPI_RESIDUAL);
    }
    // attention half of layer l: the one-launch block, or q/k/v, attention + merge and o_proj as stand-alone launches
    int attention_half(int l, const o3v_llm_layer_w& lw) {
        const bool fp8 = r.weights == W_FP8_ROWS;
        if (r.block) {
            const int rc =
                r.qk_norm ? o3v_decode_attn_block_qknorm(st->x, lw.ln1, d->rms_eps, fp8 ? lw.qkv_w8 : lw.qkv_w, fp8 ? lw.qkv_s : nullptr,
                                                         fp8 ? lw.o_w8 : lw.o_w, fp8 ? lw.o_s : nullptr, lw.q_norm, lw.k_norm, w.qkv,
                                                         st->cosT, st->sinT, w.q, w.att, kc(l), vc(l), st->part_o, st->part_ml, st->k_lo, H,
                                                         Hq, Hkv, D, st->S + step, st->Tmax, st->Tnew, step, st->nsplit, scale, st->sync,
                                                         epoch(l), s)
                : fp8 ? o3v_decode_attn_block_fp8(st->x, lw.ln1, d->rms_eps, lw.qkv_w8, lw.qkv_s, lw.qkv_b, lw.o_w8, lw.o_s, st->cosT,
                                                  st->sinT, w.q, w.att, kc(l), vc(l), st->part_o, st->part_ml, st->k_lo, H, Hq, Hkv, D,
                                                  st->S + step, st->Tmax, st->Tnew, step, st->nsplit, scale, st->sync, epoch(l), s)
                      : o3v_decode_attn_block(st->x, lw.ln1, d->rms_eps, lw.qkv_w, lw.qkv_b, lw.o_w, st->cosT, st->sinT, w.q, w.att,
                                              kc(l), vc(l), st->part_o, st->part_ml, st->k_lo, H, Hq, Hkv, D, st->S + step, st->Tmax,
                                              st->Tnew, step, st->nsplit, scale, st->sync, epoch(l), s);
            TRY(settle(r.block, first(l), rc));  // off: shapes or residency do not allow the one-launch form: the stand-alone kernels instead
        }
        if (!r.block) {
            TRY(qkv(l, lw));
            TRY(attention(l));
            TRY(o_proj(lw));
        }
        if (hs) ++hs[r.block ? 2 : 3];
        return O3V_OK;
    }
    int layer(int l) {
        const o3v_llm_layer_w& lw = d->layer[l];
        TRY(attention_half(l, lw));
        return mlp(lw);
    }
};
}  // namespace

extern "C" int o3v_llm_decode_ex(const o3v_llm_desc* d, const o3v_decode_state* st, const o3v_logprob_opts* lp,
                                 const o3v_sampling_opts* so, int step0, int n_steps, int skip_last_forward, o3v_stream_t s) {
    return o3v_llm_decode_guided(d, st, lp, so, nullptr, step0, n_steps, skip_last_forward, s);
}

extern "C" int o3v_llm_decode_guided(const o3v_llm_desc* d, const o3v_decode_state* st, const o3v_logprob_opts* lp,
                                     const o3v_sampling_opts* so, const o3v_guided_opts* go, int step0, int n_steps,
                                     int skip_last_forward, o3v_stream_t s) {
    o3v_samp_x probe;
    if (so) TRY(o3v_sampling_resolve(so, 0, &probe));  // host-only checks of the controls, before anything else
    if (go) TRY(o3v_guided_resolve(go, 0, d ? d->vocab : 0, 0, &probe));   // (d NULL is refused below)
    if (!d || !st || !st->x || !st->kcache || !st->vcache || !st->cosT || !st->sinT || !st->logits || !st->seen ||
        !st->cur_tok || !st->finished || !st->out_ids || !st->part_o || !st->part_ml || !st->workspace || !st->sample_scratch)
        return O3V_ERR_ARG;
    const int B = st->B;
    // shared prompt entries: the caches hold only the generated tokens (slot = step), the prompt K/V live once per prompt
    const bool pfx = st->kprefix != nullptr;
    const bool ragged = (st->flags & O3V_DECODE_RAGGED) && st->row_base != nullptr;  // rows guard their own capacity
    if (B <= 0 || B > 32 || step0 < 0 || n_steps < 0 || step0 + n_steps > st->Tnew ||
        (!ragged && (pfx ? st->own_past + st->Tnew : st->S + st->Tnew) > st->Tmax + 1))
        return O3V_ERR_ARG;
    if (ragged && (st->group > 1 || pfx || st->k8 || st->own_past || st->own_lo || (st->flags & O3V_DECODE_KV8_EMULATE) || !st->kstage ||
                   !st->vstage || st->Tmax <= 0))
        return O3V_ERR_ARG;
    // suffixes behind a shared prefix: a group on a prompt entry, bf16 K/V
    if ((st->own_past || st->own_lo) && (st->own_past < 0 || !pfx || st->group <= 1 || st->k8)) return O3V_ERR_ARG;
    if (pfx && (!st->vprefix || st->group <= 1 || st->rows_per_prompt <= 0 || (B % st->rows_per_prompt) || st->S > st->prefix_cap))
        return O3V_ERR_ARG;
    if (st->k8 && (!st->v8 || !st->k8s || !st->v8s || st->group > 1 || pfx || st->nsplit <= 0)) return O3V_ERR_ARG;
    if (st->k8 && d->head_dim != 128) return O3V_ERR_SHAPE;
    Decode c{d, st, s, decide_regime(d, st), (long long*)st->host_stats, step0};
    c.B = B, c.H = d->hidden, c.Hq = d->heads, c.Hkv = d->kv_heads, c.D = d->head_dim, c.I = d->inter, c.V = d->vocab;
    c.QD = c.Hq * c.D, c.NQKV = (c.Hq + 2 * c.Hkv) * c.D, c.slot0 = pfx ? st->own_past : st->S;  // slot0: cache slot of generated token 0
    if (st->ws_bytes < o3v_llm_workspace_bytes(d, B) || !carve_llm(d, B, st->workspace, st->ws_bytes, c.w))
        return O3V_ERR_WORKSPACE;
    c.scale = 1.0f / sqrtf((float)c.D);
    c.layer_stride = (size_t)B * c.Hkv * st->Tmax * c.D * 2;
    c.pre_stride = pfx ? (size_t)(B / st->rows_per_prompt) * c.Hkv * st->prefix_cap * c.D * 2 : 0;
    for (int i = 0; i < n_steps; ++i) {
        c.step = step0 + i;
        TRY(c.sample(lp, so, go));
        if (skip_last_forward && i == n_steps - 1) break;
        if (!ragged && c.slot0 + c.step >= st->Tmax) return O3V_ERR_ARG;
        // one decode forward: token `step` sits in cache slot S+step, context = S+step+1 keys
        if (st->do_sample) TRY(o3v_embed_tokens(d->embed, st->cur_tok, st->x, B, c.H, s));
        const long long launches0 = o3v_tl_launches;
        for (int l = 0; l < d->layers; ++l) TRY(c.layer(l));
        if (c.hs) {
            ++c.hs[0];
            c.hs[1] += o3v_tl_launches - launches0;
        }
        // the head follows the layers: fp8 rows only when the layer stack of this call streams fp8 rows
        TRY(llm_head(d, st->x, c.H, B, c.w.normed, st->logits, c.r.weights, s));
    }
    return O3V_OK;
}
