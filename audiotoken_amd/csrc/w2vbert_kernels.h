// Launchers of the semantic_m-specific kernels (w2vbert_kernels.hip).
#pragma once
#include "at_common.h"
#include "gemm_bf16x3.h"   // piece_t, SplitW, SplitOut

namespace at {

int launch_frame_prep(const float* wav, const float* smask, const float* window, double* frames, float* fmask, int B, int N,
                      int F, hipStream_t stream, int* status = nullptr);   // status: OR-ed with XB_STATUS_NONFINITE when a frame holds a NaN / infinity
int launch_dft_f64(const double* frames, const double* dft, float* spec, long long M, int N, hipStream_t stream);
int launch_fbank_normalize(const float* logmel, const float* fmask, float* stats, float* feats, float* amask, int B, int F, int Tp,
                           hipStream_t stream);
int launch_layernorm(const float* x, const float* gamma, const float* beta, const float* row_mask, float* y, long long rows, int D,
                     hipStream_t stream);
// One rel-pos self-attention call over qkv rows [B * T][3 * heads * 64]; the launchers below only unpack it.
struct AttnArgs {
    const float* qkv = nullptr;
    const float* amask = nullptr;       // [B][T], 0 = padded key
    const float* dist_emb = nullptr;    // distance embeddings [80][64]; nullptr = no rel-pos bias (HuBERT)
    float* ctx = nullptr;               // fp32 context [B * T][heads * 64] (nullptr when ctx_pieces is given)
    int B = 0, T = 0, heads = 16;
    // launch_relpos_attention only: 0 = fp32-MFMA kernel, 1 = bf16x3, 2 = f16x2 (attention_bf16x3.hip), -1 = the default ($AUDIOTOKEN_SEMANTIC_ARITH, else f16x2)
    int arith = -1;
    int* status = nullptr;              // device word for the fp16 range check (nullable)
    // split arithmetic only: the context is written as operand pieces [NP][hid/16][rows_pad][16] instead of fp32 ctx
    piece_t* ctx_pieces = nullptr;
    long long rows_pad = 0;
    // f16x2 only: k and v are read as the row-major fp16 pieces [which][piece][rows_pad][hid] the q / k / v projection wrote (XB_EPI_QKV) instead of being
    // split from the fp32 qkv rows by every query-tile workgroup; qkv then only supplies q
    const piece_t* kv_pieces = nullptr;
    int w8 = -1;                        // 1 / 0 = the 8-wave kernel (attention_f16x2_w8.hip) / its round-3 twin; -1 = $AUDIOTOKEN_ATTN_W8, default 1
    SplitW dist;                        // the distance embeddings as fp16 pieces [2][96][64] * dist.s (launch_dist_split; 24 576 bytes): what the 8-wave kernel reads
};
int launch_relpos_attention(const AttnArgs& a, hipStream_t stream);
// the same attention with both products as operand splits on the 16-bit matrix cores (attention_bf16x3.hip); scheme = XB_SCHEME_* (a.arith is not read)
int launch_relpos_attention_x3(const AttnArgs& a, int scheme, hipStream_t stream);
// round 4: the f16x2 attention with pre-split k / v as ONE 8-wave workgroup per CU, 64-key tiles and LDS-DMA staging (attention_f16x2_w8.hip);
// launch_relpos_attention_x3 dispatches to it when kv_pieces != nullptr and w8 != 0. Rel-pos bias iff a.dist.p != nullptr (a.dist_emb is not read)
bool relpos_attention_w8_eligible(int T, int heads, long long rows_pad, long long B, bool relpos);
int launch_relpos_attention_w8(const AttnArgs& a, hipStream_t stream);
int launch_dist_split(const float* dist_emb, __bf16* out, float scale, hipStream_t stream);
// fp32 qkv rows [rows][3 hid] -> row-major k / v pieces [which][piece][rows_pad][hid] * XB_F16_ACT_SCALE (what XB_EPI_QKV writes)
int launch_kv_rowmajor_split(const float* qkv, __bf16* out, long long rows, long long rows_pad, int hid, int* status, hipStream_t stream);
// Conformer conv-module middle: depthwise conv + LayerNorm + swish. split.pieces != nullptr: the output is written as the operand pieces of `split`
// ([NP][64][rows_pad][16]) instead of fp32 `out`.
int launch_dwconv_ln_swish(const float* g, const float* w, const float* gamma, const float* beta, float* out, int B, int T, hipStream_t stream,
                           const SplitOut& split = {});
// the same op as a streaming kernel: one channel per thread walking along time, 16 waves per CU, every input row read once (dwconv_stream.hip);
// bit-identical to launch_dwconv_ln_swish
int launch_dwconv_stream(const float* g, const float* w, const float* gamma, const float* beta, float* out, int B, int T, hipStream_t stream,
                         const SplitOut& split = {});
// LayerNorm(D = 1024 or 768) written as the operand pieces of `split` ([NP][D/16][rows_pad][16]); y != nullptr: also as fp32 [rows][D]
int launch_layernorm_split(const float* x, const float* gamma, const float* beta, const float* row_mask, float* y, long long rows, int D, const SplitOut& split,
                           hipStream_t stream);
// y = LN(x; gamma, beta) as fp32 rows and the pieces of `split` = LN(y; gamma2, beta2), one pass (D = 1024)
int launch_layernorm2_split(const float* x, const float* gamma, const float* beta, float* y, const float* gamma2, const float* beta2, long long rows, int D,
                            const SplitOut& split, hipStream_t stream);
// status (nullable): OR-ed with XB_STATUS_NONFINITE when a row of x holds a NaN / infinity
// ld: row stride of `dots` (0 = C; > C when the score GEMM ran against a zero-padded code book)
// codebook (nullable): the fp32 code rows [C][D]; when given, the codes within a relative window of the best approximate distance are re-evaluated exactly
// (sum of squared differences in float64) — see vq_argmax_kernel
int launch_vq_argmax(const float* x, const float* dots, const float* e2, int16_t* out, long long rows, int D, int C,
                     hipStream_t stream, int* status = nullptr, int ld = 0, const float* codebook = nullptr);

}  // namespace at
