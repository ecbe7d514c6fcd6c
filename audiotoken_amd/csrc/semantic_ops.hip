// Operator-level entry points of the semantic kernels for the parity tests (at_op_* in include/audiotoken_hip.h): one launcher each, no model handle.
#include "../../include/audiotoken_hip.h"
#include "gemm_bf16x3.h"
#include "w2vbert_kernels.h"

using namespace at;

extern "C" {

int at_op_layernorm(const float* x, const float* gamma, const float* beta, const float* row_mask, float* y, int64_t rows, int D,
                    at_stream_t stream) {
    AT_REQUIRE(x && y, "null pointer");
    return launch_layernorm(x, gamma, beta, row_mask, y, rows, D, (hipStream_t)stream);
}

int at_op_relpos_attention(const float* qkv, const float* attn_mask, const float* dist_emb80, float* ctx, int B, int T,
                           at_stream_t stream) {
    AT_REQUIRE(qkv && attn_mask && dist_emb80 && ctx && B >= 1 && T >= 1, "bad arguments");
    AttnArgs a;
    a.qkv = qkv; a.amask = attn_mask; a.dist_emb = dist_emb80; a.ctx = ctx; a.B = B; a.T = T;
    return launch_relpos_attention(a, (hipStream_t)stream);
}

int at_op_attention_f32(const float* qkv, const float* attn_mask, const float* dist_emb80, float* ctx, int B, int T, int heads, at_stream_t stream) {
    AT_REQUIRE(qkv && attn_mask && ctx && B >= 1 && T >= 1 && heads >= 1 && heads <= 64, "bad arguments");
    AttnArgs a;
    a.qkv = qkv; a.amask = attn_mask; a.dist_emb = dist_emb80; a.ctx = ctx; a.B = B; a.T = T; a.heads = heads; a.arith = 0;
    return launch_relpos_attention(a, (hipStream_t)stream);
}

int at_op_relpos_attention_kvp(const float* qkv, const float* attn_mask, const float* dist_emb80, float dist_max_abs, float* ctx, int B, int T, int heads, int w8,
                               void* kv_workspace, size_t kv_workspace_bytes, int32_t* status_dev, at_stream_t stream) {
    AT_REQUIRE(qkv && attn_mask && ctx && kv_workspace && B >= 1 && T >= 1 && heads >= 1 && heads <= 64, "bad arguments");
    const long long rows = (long long)B * T, rows_pad = (rows + 255) / 256 * 256;
    const int hid = heads * 64;
    const size_t kv_bytes = (size_t)4 * rows_pad * hid * 2, dist_bytes = (size_t)2 * 96 * 64 * 2;
    AT_REQUIRE(kv_workspace_bytes >= kv_bytes + dist_bytes, "kv workspace too small: 4 * ceil256(B * T) * heads * 64 * 2 + 24576 bytes");
    if (int rc = launch_kv_rowmajor_split(qkv, static_cast<__bf16*>(kv_workspace), rows, rows_pad, hid, status_dev, (hipStream_t)stream)) return rc;
    AttnArgs a;
    a.qkv = qkv; a.amask = attn_mask; a.dist_emb = dist_emb80; a.ctx = ctx; a.B = B; a.T = T; a.heads = heads; a.arith = 2;
    a.status = status_dev; a.rows_pad = rows_pad; a.kv_pieces = static_cast<const __bf16*>(kv_workspace); a.w8 = w8;
    if (dist_emb80) {   // what finalize() does once per layer: the distance embeddings as fp16 pieces times a power of two
        __bf16* dist_s = reinterpret_cast<__bf16*>(static_cast<char*>(kv_workspace) + kv_bytes);
        a.dist = SplitW{dist_s, xb_weight_scale(dist_max_abs)};
        if (int rc = launch_dist_split(dist_emb80, dist_s, a.dist.s, (hipStream_t)stream)) return rc;
    }
    return launch_relpos_attention(a, (hipStream_t)stream);
}

int at_op_dwconv_ln_swish(const float* g, const float* w31x1024, const float* gamma, const float* beta, float* out, int B, int T,
                          at_stream_t stream) {
    AT_REQUIRE(g && w31x1024 && gamma && beta && out && B >= 1 && T >= 1, "bad arguments");
    return launch_dwconv_ln_swish(g, w31x1024, gamma, beta, out, B, T, (hipStream_t)stream);
}

int at_op_dwconv_stream(const float* g, const float* w31x1024, const float* gamma, const float* beta, float* out, int B, int T,
                        at_stream_t stream) {
    AT_REQUIRE(g && w31x1024 && gamma && beta && out && B >= 1 && T >= 1, "bad arguments");
    return launch_dwconv_stream(g, w31x1024, gamma, beta, out, B, T, (hipStream_t)stream);
}

int at_op_vq_argmax(const float* x, const float* dots, const float* e2, int16_t* out, int64_t rows, int D, int C, at_stream_t stream) {
    AT_REQUIRE(x && dots && e2 && out && D % 4 == 0 && C % 4 == 0, "bad arguments");
    return launch_vq_argmax(x, dots, e2, out, rows, D, C, (hipStream_t)stream);
}

int at_op_vq_argmax_refined(const float* x, const float* dots, const float* e2, const float* codebook, int16_t* out, int64_t rows, int D, int C, at_stream_t stream) {
    AT_REQUIRE(x && dots && e2 && codebook && out && D % 4 == 0 && C % 4 == 0, "bad arguments");
    return launch_vq_argmax(x, dots, e2, out, rows, D, C, (hipStream_t)stream, nullptr, 0, codebook);
}

}  // extern "C"
