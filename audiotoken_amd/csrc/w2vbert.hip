// semantic_m tokenizer (log-mel front-end -> Wav2Vec2-BERT conformer -> LayerNorm -> VQ) — host side.
// C ABI in include/audiotoken_hip.h. Replaces reference Wav2VecBertEncoder (audiotoken/encoder.py:111-186):
// processor (audiotoken/processors.py), HF Wav2Vec2BertModel with the reference's rel-pos SDPA attention
// (audiotoken/modeling_wav2vec2_bert.py:20-80), non-affine LayerNorm and VectorQuantize lookup.
// Arithmetic per SURVEY.md Appendix A.2 / A.3.
//
// The conformer is fp32 on the f32 matrix cores: token ids must equal the reference's fp32 CPU result and the
// bf16 autocast the reference uses on GPU is not reproducible. The front-end's frame
// arithmetic and DFT run in f64 (see w2vbert_kernels.hip: frame_prep_kernel / dft_f64_kernel for why).
//
// Weight repacking at finalize():
//   DFT            generated here in double: [520][400], rows 0..256 cos, 260..516 -sin (rest zero)
//   mel            [257][80] (reference layout) -> [80][260]
//   q,k,v Linear   -> one [3072][1024] matrix (one GEMM, one pass over the LayerNorm output)
//   pointwise_conv1 [2048][1024][1] -> rows interleaved (a_c, b_c) so GLU is the GEMM epilogue
//   depthwise_conv [1024][1][31] -> [31][1024]
//   distance_embedding [73][64] -> [80][64] zero padded (MFMA row tiles)
// The encode entry point is checks, plan, the Call struct, then one call per stage: front_end, feature_projection, conformer_layer_split /
// conformer_layer_f32 per layer, quantise. Every split GEMM goes through split_gemm_args (semantic_handle.h), which owns the f16x2 scale rule.
#include <string>
#include <vector>
#include <cstring>
#include <cmath>

#include "../../include/audiotoken_hip.h"
#include "semantic_handle.h"
#include "w2vbert_kernels.h"

namespace at {
const char* last_error_cstr();
}
using namespace at;

namespace {
constexpr int kHid = 1024, kFfn = 4096, kFeat = 160, kMel = 80, kFrame = 400, kHop = 160;
constexpr int kSpecLd = 520, kImOff = 260, kCodes = 2048, kBuckets = 73;

enum { W_1A = 0, W_1B, W_2A, W_2B, W_QKV, W_O, W_PW1, W_PW2, W_NLINEAR };
// output x input width of the eight linear layers
constexpr int kWN[W_NLINEAR] = {kFfn, kHid, kFfn, kHid, 3 * kHid, kHid, 2 * kHid, kHid}, kWK[W_NLINEAR] = {kHid, kFfn, kHid, kFfn, kHid, kHid, kHid, kHid};

// Sites of the handle's range table (semantic_handle.h, RangeTable): where activations become fp16 pieces. The same site in every layer.
enum WSite { WS_LN_FFN1 = 0, WS_FFN1_HIDDEN, WS_LN_ATTN, WS_QKV_KV, WS_ATTENTION, WS_LN_CONV, WS_DWCONV, WS_LN_FFN2, WS_FFN2_HIDDEN, WS_OTHER, W_NSITES };
static const char* const kWSiteNames[W_NSITES] = {"ln_ffn1", "ffn1_hidden", "ln_attn", "qkv_kv", "attention", "ln_conv", "dwconv_out", "ln_ffn2", "ffn2_hidden", "other"};
static_assert((int)W_NSITES == 10, "LayerW::site_scale has one entry per WSite");
// rows of the range table: one per conformer layer, layer l is row l, up to 64 layers
constexpr int kRangeLayers = 64, kRangeLayer0 = 0;

struct LayerW {
    const float *ln_ffn1_g, *ln_ffn1_b, *w1a, *b1a, *w1b, *b1b;
    const float *ln_att_g, *ln_att_b, *wqkv, *bqkv, *dist, *wo, *bo;
    const float *ln_conv_g, *ln_conv_b, *pw1, *dw, *ln_dw_g, *ln_dw_b, *pw2;
    const float *ln_ffn2_g, *ln_ffn2_b, *w2a, *b2a, *w2b, *b2b;
    const float *ln_fin_g, *ln_fin_b;
    SplitW ws[2][W_NLINEAR];   // the eight linear layers as operand pieces (gemm_bf16x3.hip), per scheme [XB_SCHEME_*][W_*]; split lazily per scheme
    SplitW dist_s;             // the distance embeddings as fp16 pieces [2][96][64] (attention_f16x2_w8.hip's rel-pos table MFMAs; f16x2 scheme only)
    // f16x2: the power of two every activation is multiplied by before it is split, per split site (WSite). XB_F16_ACT_SCALE (16) everywhere, except that
    // the LayerNorm-fed sites get the PROVABLE scale of xb_ln_site_scale() (gemm_bf16x3.h) when the LayerNorm's gains are large enough for 16 to overflow (finalize)
    float site_scale[W_NSITES] = {XB_F16_ACT_SCALE, XB_F16_ACT_SCALE, XB_F16_ACT_SCALE, XB_F16_ACT_SCALE, XB_F16_ACT_SCALE,
                                  XB_F16_ACT_SCALE, XB_F16_ACT_SCALE, XB_F16_ACT_SCALE, XB_F16_ACT_SCALE, XB_F16_ACT_SCALE};
};

// what finalize builds on the device
struct W2vBertW {
    const float *window = nullptr, *melw = nullptr;
    double* dft64 = nullptr;  // [520][400] DFT matrix in double (see dft_f64_kernel)
    const float *fp_ln_g = nullptr, *fp_ln_b = nullptr, *fp_w = nullptr, *fp_b = nullptr;
    std::vector<LayerW> layers;
    const float *codebook = nullptr, *e2 = nullptr;
    SplitW cb_s[2];   // the code book as operand pieces, per scheme (the VQ score GEMM on the split kernel; option "vq_split")
};
}  // namespace

struct at_w2vbert : SemanticHandle, W2vBertW {
    bool vq_split = true;
    bool dwconv_stream = true;  // option "dwconv_stream": depthwise conv + LayerNorm + swish on the streaming kernel (dwconv_stream.hip)
    explicit at_w2vbert(int device_id) : SemanticHandle(PACKED_MODEL_W2VBERT, device_id, RangeTable{kRangeLayers, (int)W_NSITES, kRangeLayer0}) {
        bool_opts = {{"dwconv_stream", &dwconv_stream}, {"vq_split", &vq_split}};
    }
    int finalize_model() override;
    int split_model(int scheme) override;
    void forget_model() override { static_cast<W2vBertW&>(*this) = W2vBertW{}; }
    int num_layers() const override { return (int)layers.size(); }
    bool has_codes() const override { return codebook != nullptr; }
};

namespace {

int frames_of(int N) { return N >= kFrame ? 1 + (N - kFrame) / kHop : 0; }
int tokens_of(int N, int mult) {
    int t = frames_of(N) / 2;
    if (mult > 0 && t % mult) t += mult - t % mult;
    return t;
}

struct Plan {
    int F, Tp;
    size_t off_frames, off_fmask, off_spec, off_logmel, off_stats, off_feats, off_amask, off_x, off_t1, off_big, off_tok, off_t1s, off_bigs, off_kvs;
    size_t Mpad;
    size_t total_floats;
};

Plan make_plan(int B, int N, int mult) {
    Plan p;
    p.F = frames_of(N);
    p.Tp = tokens_of(N, mult);
    size_t cur = 0;
    auto takef = [&](size_t n) { size_t o = cur; cur += (n + 63) / 64 * 64; return o; };
    const size_t M = (size_t)B * p.Tp, BF = (size_t)B * p.F;
    p.off_frames = takef(BF * kFrame * 2);  // float64 frames
    p.off_fmask = takef(BF);
    p.off_spec = takef(BF * kSpecLd);
    p.off_logmel = takef(BF * kMel);
    p.off_stats = takef((size_t)B * 2 * kMel);
    p.off_feats = takef(M * kFeat);
    p.off_amask = takef(M);
    p.off_x = takef(M * kHid);
    p.off_t1 = takef(M * kHid);
    p.off_big = takef(M * kFfn);
    p.off_tok = takef(M);
    p.Mpad = (M + 255) / 256 * 256;                       // split-bf16 operands: 3 pieces x 2 bytes = 1.5 floats per element
    p.off_t1s = takef(p.Mpad * kHid * 3 / 2);
    p.off_bigs = takef(p.Mpad * kFfn * 3 / 2);
    p.off_kvs = takef(p.Mpad * kHid * 2 * 2 / 2);        // k and v as two fp16 pieces each (XB_EPI_QKV): 2 x 2 x 2 bytes per element
    p.total_floats = cur;
    return p;
}

// ---- finalize: the staged tensors of one part of the model -> device, in the order the packed blob records ---------------------------------------
// front-end tables: window, mel filters [257][80] -> [80][260], the DFT matrix generated in double
int take_frontend(at_w2vbert* h) {
    const bool imp = h->arena.importing;
    bool ok = true;
    h->window = take(h, "frontend.window", {kFrame}, ok);
    if (!ok) return -1;
    if (int rc = take_repacked(h, (size_t)kMel * kImOff, &h->melw, [&](std::vector<float>& m) {
            const HostTensor* mf = find(h, "frontend.mel_filters");
            AT_REQUIRE(mf && mf->shape == (std::vector<int64_t>{257, kMel}), "frontend.mel_filters [257,80] missing");
            for (int k = 0; k < 257; ++k)
                for (int j = 0; j < kMel; ++j) m[(size_t)j * kImOff + k] = mf->data[(size_t)k * kMel + j];
            return 0;
        }))
        return rc;
    h->dft64 = static_cast<double*>(h->arena.alloc((size_t)kSpecLd * kFrame * sizeof(double)));
    if (imp) {
        AT_REQUIRE(h->melw && h->dft64, "import_packed: front-end tables");
        return 0;
    }
    AT_REQUIRE(h->melw != nullptr && h->dft64 != nullptr, "device allocation failed (front-end tables)");
    std::vector<double> d((size_t)kSpecLd * kFrame, 0.0);
    const double two_pi = 6.283185307179586476925286766559;
    for (int k = 0; k < 257; ++k)
        for (int t = 0; t < kFrame; ++t) {
            const int ph = (int)(((long long)k * t) % 512);  // exact argument reduction
            const double ang = two_pi * ph / 512.0;
            d[(size_t)k * kFrame + t] = std::cos(ang);
            d[(size_t)(kImOff + k) * kFrame + t] = -std::sin(ang);
        }
    AT_CHECK_HIP(hipMemcpy(h->dft64, d.data(), d.size() * sizeof(double), hipMemcpyHostToDevice));
    return 0;
}

// the attention block's repacked tensors: q, k, v as one matrix, the distance embeddings [73][64] zero padded to [80][64]
int take_attention(at_w2vbert* h, const std::string& p, LayerW& L) {
    static const char* const kQkv[3] = {"linear_q", "linear_k", "linear_v"};
    if (int rc = take_qkv(h, p + ".self_attn.", kQkv, kHid, &L.wqkv, &L.bqkv)) return rc;
    if (int rc = take_repacked(h, (size_t)80 * 64, &L.dist, [&](std::vector<float>& e) {
            const HostTensor* de = find(h, p + ".self_attn.distance_embedding.weight");
            AT_REQUIRE(de && de->shape == (std::vector<int64_t>{kBuckets, 64}), "distance_embedding [73,64] missing");
            std::memcpy(e.data(), de->data.data(), (size_t)kBuckets * 64 * sizeof(float));
            return 0;
        }))
        return rc;
    AT_REQUIRE(L.wqkv && L.bqkv && L.dist, h->arena.importing ? "import_packed: attention tensors" : "device allocation failed");
    return 0;
}

// the conv module's repacked tensors: pointwise_conv1 rows interleaved (a_c, b_c), depthwise_conv [1024][1][31] -> [31][1024]
int take_conv_module(at_w2vbert* h, const std::string& p, LayerW& L) {
    if (int rc = take_repacked(h, (size_t)2 * kHid * kHid, &L.pw1, [&](std::vector<float>& w) {
            const HostTensor* pw = find(h, p + ".conv_module.pointwise_conv1.weight");
            AT_REQUIRE(pw && pw->shape == (std::vector<int64_t>{2 * kHid, kHid, 1}), "pointwise_conv1 [2048,1024,1] missing");
            for (int c = 0; c < kHid; ++c) {
                std::memcpy(&w[(size_t)(2 * c) * kHid], &pw->data[(size_t)c * kHid], kHid * sizeof(float));
                std::memcpy(&w[(size_t)(2 * c + 1) * kHid], &pw->data[(size_t)(kHid + c) * kHid], kHid * sizeof(float));
            }
            return 0;
        }))
        return rc;
    if (int rc = take_repacked(h, (size_t)31 * kHid, &L.dw, [&](std::vector<float>& d) {
            const HostTensor* dw = find(h, p + ".conv_module.depthwise_conv.weight");
            AT_REQUIRE(dw && dw->shape == (std::vector<int64_t>{kHid, 1, 31}), "depthwise_conv [1024,1,31] missing");
            for (int c = 0; c < kHid; ++c)
                for (int j = 0; j < 31; ++j) d[(size_t)j * kHid + c] = dw->data[(size_t)c * 31 + j];
            return 0;
        }))
        return rc;
    AT_REQUIRE(L.pw1 && L.dw, h->arena.importing ? "import_packed: conv-module tensors" : "device allocation failed");
    return 0;
}

// conformer layer i, in state-dict order of its blocks
int take_layer(at_w2vbert* h, int i, LayerW& L) {
    const std::string p = "encoder.layers." + std::to_string(i);
    bool ok = true;
    L.ln_ffn1_g = take(h, p + ".ffn1_layer_norm.weight", {kHid}, ok);
    L.ln_ffn1_b = take(h, p + ".ffn1_layer_norm.bias", {kHid}, ok);
    L.w1a = take(h, p + ".ffn1.intermediate_dense.weight", {kFfn, kHid}, ok);
    L.b1a = take(h, p + ".ffn1.intermediate_dense.bias", {kFfn}, ok);
    L.w1b = take(h, p + ".ffn1.output_dense.weight", {kHid, kFfn}, ok);
    L.b1b = take(h, p + ".ffn1.output_dense.bias", {kHid}, ok);
    L.ln_att_g = take(h, p + ".self_attn_layer_norm.weight", {kHid}, ok);
    L.ln_att_b = take(h, p + ".self_attn_layer_norm.bias", {kHid}, ok);
    if (!ok) return -1;
    if (int rc = take_attention(h, p, L)) return rc;
    L.wo = take(h, p + ".self_attn.linear_out.weight", {kHid, kHid}, ok);
    L.bo = take(h, p + ".self_attn.linear_out.bias", {kHid}, ok);
    L.ln_conv_g = take(h, p + ".conv_module.layer_norm.weight", {kHid}, ok);
    L.ln_conv_b = take(h, p + ".conv_module.layer_norm.bias", {kHid}, ok);
    if (!ok) return -1;
    if (int rc = take_conv_module(h, p, L)) return rc;
    L.ln_dw_g = take(h, p + ".conv_module.depthwise_layer_norm.weight", {kHid}, ok);
    L.ln_dw_b = take(h, p + ".conv_module.depthwise_layer_norm.bias", {kHid}, ok);
    L.pw2 = take(h, p + ".conv_module.pointwise_conv2.weight", {kHid, kHid, 1}, ok);
    L.ln_ffn2_g = take(h, p + ".ffn2_layer_norm.weight", {kHid}, ok);
    L.ln_ffn2_b = take(h, p + ".ffn2_layer_norm.bias", {kHid}, ok);
    L.w2a = take(h, p + ".ffn2.intermediate_dense.weight", {kFfn, kHid}, ok);
    L.b2a = take(h, p + ".ffn2.intermediate_dense.bias", {kFfn}, ok);
    L.w2b = take(h, p + ".ffn2.output_dense.weight", {kHid, kFfn}, ok);
    L.b2b = take(h, p + ".ffn2.output_dense.bias", {kHid}, ok);
    L.ln_fin_g = take(h, p + ".final_layer_norm.weight", {kHid}, ok);
    L.ln_fin_b = take(h, p + ".final_layer_norm.bias", {kHid}, ok);
    if (!ok) return -1;
    L.site_scale[WS_LN_FFN1] = ln_site_scale(h, L.ln_ffn1_g, L.ln_ffn1_b, kHid);
    L.site_scale[WS_LN_ATTN] = ln_site_scale(h, L.ln_att_g, L.ln_att_b, kHid);
    L.site_scale[WS_LN_CONV] = ln_site_scale(h, L.ln_conv_g, L.ln_conv_b, kHid);
    L.site_scale[WS_DWCONV] = ln_site_scale(h, L.ln_dw_g, L.ln_dw_b, kHid);
    L.site_scale[WS_LN_FFN2] = ln_site_scale(h, L.ln_ffn2_g, L.ln_ffn2_b, kHid);
    // free the staged host copies of this layer early
    for (auto it = h->staged.begin(); it != h->staged.end();)
        it = it->first.compare(0, p.size() + 1, p + ".") == 0 ? h->staged.erase(it) : std::next(it);
    return 0;
}

// VQ codebook (state-dict key _codebook.embed [1, 2048, 1024], reference audiotoken/utils.py:331-339) and its squared norms
int take_codebook(at_w2vbert* h) {
    if (h->arena.importing) {
        if (h->imp.flags & 1) {
            h->codebook = reserve(h, (size_t)kCodes * kHid);
            h->e2 = reserve(h, kCodes);
            AT_REQUIRE(h->codebook && h->e2, "import_packed: code book");
        }
        return 0;
    }
    const HostTensor* cb = find(h, "vq._codebook.embed");
    if (!cb) return 0;
    AT_REQUIRE((cb->shape == std::vector<int64_t>{1, kCodes, kHid}) || (cb->shape == std::vector<int64_t>{kCodes, kHid}),
               "vq._codebook.embed must be [1,2048,1024]");
    h->codebook = upload(h, cb->data);
    const HostTensor* e = find(h, "vq._codebook.e2");
    if (e) AT_REQUIRE(e->data.size() == (size_t)kCodes, "bad e2 shape");
    h->e2 = upload(h, e ? e->data : code_norms(cb->data, kCodes, kHid));
    AT_REQUIRE(h->codebook && h->e2, "device allocation failed (codebook)");
    return 0;
}

}  // namespace

// Split the eight linear layers of every conformer layer into the 16-bit pieces of `scheme`
int at_w2vbert::split_model(int scheme) {
    for (LayerW& L : layers) {
        const float* src[W_NLINEAR] = {L.w1a, L.w1b, L.w2a, L.w2b, L.wqkv, L.wo, L.pw1, L.pw2};
        for (int j = 0; j < W_NLINEAR; ++j)
            if (int rc = split_one(this, scheme, src[j], kWN[j], kWK[j], &L.ws[scheme][j])) return rc;
        if (scheme == XB_SCHEME_F16X2) {   // distance embeddings -> pieces for the attention kernel's rel-pos table
            piece_t* d = static_cast<piece_t*>(arena.alloc((size_t)2 * 96 * 64 * sizeof(piece_t)));
            if (!d) return -1;
            float s = 1.f;
            if (int rc = weight_scale(this, L.dist, &s)) return rc;
            if (!arena.importing)
                if (int rc = launch_dist_split(L.dist, d, s, nullptr)) return rc;
            L.dist_s = SplitW{d, s};
        }
    }
    if (codebook)   // the VQ score GEMM dots = LN(x) . E^T [M x 1024] x [1024 x 2048]
        if (int rc = split_one(this, scheme, codebook, kCodes, kHid, &cb_s[scheme])) return rc;
    return 0;
}

// The model part of finalize(): staged host tensors -> device (semantic_handle.h, finalize_model)
int at_w2vbert::finalize_model() {
    if (int rc = take_frontend(this)) return rc;
    bool ok = true;
    fp_ln_g = take(this, "feature_projection.layer_norm.weight", {kFeat}, ok);
    fp_ln_b = take(this, "feature_projection.layer_norm.bias", {kFeat}, ok);
    fp_w = take(this, "feature_projection.projection.weight", {kHid, kFeat}, ok);
    fp_b = take(this, "feature_projection.projection.bias", {kHid}, ok);
    if (!ok) return -1;
    int nl = arena.importing ? imp.n_layers : 0;
    while (!arena.importing && find(this, "encoder.layers." + std::to_string(nl) + ".ffn1_layer_norm.weight")) ++nl;
    for (int i = 0; i < nl; ++i) {
        LayerW L{};
        if (int rc = take_layer(this, i, L)) return rc;
        layers.push_back(L);
    }
    return take_codebook(this);
}

extern "C" {

at_w2vbert_t* at_w2vbert_create(int device_id) { return device_exists("at_w2vbert_create", device_id) ? new at_w2vbert(device_id) : nullptr; }
int at_w2vbert_set_tensor(at_w2vbert_t* h, const char* name, const float* host_data, const int64_t* shape, int ndim) {
    return stage_tensor(h, name, host_data, shape, ndim);
}
int at_w2vbert_finalize(at_w2vbert_t* h) { return sem_finalize(h); }
int64_t at_w2vbert_packed_bytes(at_w2vbert_t* h) { return sem_packed_bytes(h, "at_w2vbert_packed_bytes"); }
int64_t at_w2vbert_packed_meta(at_w2vbert_t* h, void* host_dst, int64_t cap) { return sem_packed_meta(h, "at_w2vbert_packed_meta", host_dst, cap); }
int at_w2vbert_export_packed(at_w2vbert_t* h, void* device_dst, int64_t bytes, void* stream) {
    return sem_export_packed(h, "at_w2vbert_export_packed", device_dst, bytes, stream);
}
int at_w2vbert_import_packed(at_w2vbert_t* h, const void* host_meta, int64_t meta_bytes, const void* device_src, int64_t bytes, void* stream) {
    return sem_import_packed(h, "at_w2vbert_import_packed", host_meta, meta_bytes, device_src, bytes, stream);
}
void at_w2vbert_destroy(at_w2vbert_t* h) { sem_destroy(h); }

int at_w2vbert_num_layers(const at_w2vbert_t* h) { return h ? (int)h->layers.size() : 0; }
int at_w2vbert_num_tokens(int N, int pad_to_multiple_of) { return tokens_of(N, pad_to_multiple_of); }

size_t at_w2vbert_workspace_bytes(const at_w2vbert_t* h, int B, int N, int pad_to_multiple_of) {
    if (B <= 0 || N < kFrame) return 0;
    return make_plan(B, N, pad_to_multiple_of).total_floats * sizeof(float);
}

int at_w2vbert_profile(at_w2vbert_t* h, int enable) { return profile_enable(h, enable); }
int at_w2vbert_profile_read(at_w2vbert_t* h, char* names, size_t names_cap, float* total_ms, int* launches, int max_groups) {
    return profile_read(h, names, names_cap, total_ms, launches, max_groups);
}

int at_w2vbert_set_option(at_w2vbert_t* h, const char* name, int value) { return sem_set_option(h, "at_w2vbert_set_option", name, value); }
int at_w2vbert_get_option(const at_w2vbert_t* h, const char* name) { return sem_get_option(h, name); }

}  // extern "C"

// ---- encode -------------------------------------------------------------------------------------------------------------------------------------
namespace {

// One encode call: the model, the shapes, the stream and the workspace the plan carved
struct Call {
    at_w2vbert* h;
    hipStream_t stream;
    int B, N, F, T, n_layers;
    long long M, BF, Mpad;   // token rows, frame rows, token rows padded for the split operands
    int* status;             // the caller's status word (nullable)
    double* frames;
    float *fmask, *spec, *logmel, *stats, *feats, *amask, *x, *t1, *big;
    piece_t *t1s, *bigs, *kvs;
    // layer li's arithmetic: the handle's, unless that layer is pinned to another split scheme (option "layer_arith:<i>": what the product's range fallback
    // sets for a layer whose activations do not fit fp16 — the other layers stay on f16x2). Each layer has its own row of the range table.
    SplitCtx ctx_of(int li) const { return SplitCtx{scheme_of(h->arith_of(li)), h->range.layer_row(li)}; }
};

int linear(const Call& c, const float* X, int K, const float* W, const float* bias, float* C, int N, int epi, float alpha, const float* R, const float* row_mask,
           int ldc) {
    GemmArgs a;
    a.X = X; a.x_bstride = 0; a.Tin = (int)c.M; a.Cin = K; a.ldx = K;
    a.W = W; a.bias = bias; a.C = C; a.ldc = ldc; a.R = R; a.ldr = ldc;
    a.M = (int)c.M; a.N = N; a.K = K; a.batch = 1; a.epi = epi; a.alpha = alpha; a.row_mask = row_mask;
    return launch_gemm(a, c.stream);
}

// which split site produced the A operand of linear layer w, and which site its epilogue's split output belongs to
int a_site_of(int w) {
    switch (w) {
        case W_1A: return WS_LN_FFN1;  case W_1B: return WS_FFN1_HIDDEN;  case W_2A: return WS_LN_FFN2;  case W_2B: return WS_FFN2_HIDDEN;
        case W_QKV: return WS_LN_ATTN; case W_O: return WS_ATTENTION;     case W_PW1: return WS_LN_CONV; default: return WS_DWCONV;
    }
}
int out_site_of(int w) { return w == W_1A ? WS_FFN1_HIDDEN : w == W_2A ? WS_FFN2_HIDDEN : WS_OTHER; }

// One split-operand GEMM of the conformer: C / S = epi(A . W^T) with A given as pieces (gemm_bf16x3.hip)
int gemm_split(const Call& c, const SplitCtx& sc, const LayerW& L, int w, const piece_t* A, const float* bias, int epi, float alpha, float* C, const float* R,
               piece_t* S) {
    const int out_site = out_site_of(w), ldc = epi == XB_EPI_GLU ? kWN[w] / 2 : kWN[w];
    Bf16x3Args a = split_gemm_args(sc.scheme, A, sc.act(L.site_scale[a_site_of(w)]), L.ws[sc.scheme][w], c.M, kWN[w], kWK[w], c.Mpad, epi, sc.site(out_site),
                                   sc.act(L.site_scale[out_site]));
    a.bias = bias; a.C = C; a.ldc = ldc; a.R = R; a.ldr = ldc; a.alpha = alpha; a.S = S; a.Spad = (int)c.Mpad;
    return launch_gemm_bf16x3(a, c.stream);
}

// t1s = split(LayerNorm(x)) for split site `site` of the layer (L, sc): the A operand of the next GEMM, no fp32 rows
int ln_split(const Call& c, const SplitCtx& sc, const LayerW& L, int site, const float* g, const float* b, const float* row_mask) {
    c.h->prof.begin("layernorm", 1, c.stream);
    if (int rc = launch_layernorm_split(c.x, g, b, row_mask, nullptr, c.M, kHid, sc.out(c.t1s, c.Mpad, L.site_scale[site], sc.site(site)), c.stream)) return rc;
    c.h->prof.end(c.stream);
    return 0;
}

// log-mel front end (reference processors.py): frames -> power spectrum -> mel -> normalised, stacked features and the token mask
int front_end(const Call& c, const float* wav, const float* mask) {
    const at_w2vbert* h = c.h;
    c.h->prof.begin("frontend", 5, c.stream);
    if (int rc = launch_frame_prep(wav, mask, h->window, c.frames, c.fmask, c.B, c.N, c.F, c.stream, c.status)) return rc;
    if (int rc = launch_dft_f64(c.frames, h->dft64, c.spec, c.BF, kSpecLd, c.stream)) return rc;
    {   // |X|^2 folded into the mel projection's prologue, log(max(., floor)) into its epilogue
        GemmArgs a;
        a.X = c.spec; a.Tin = (int)c.BF; a.Cin = kImOff; a.ldx = kSpecLd; a.W = h->melw; a.C = c.logmel; a.ldc = kMel;
        a.M = (int)c.BF; a.N = kMel; a.K = kImOff; a.batch = 1; a.pro = PRO_POWER; a.aux_off = kImOff; a.epi = EPI_LOGFLOOR;
        if (int rc = launch_gemm(a, c.stream)) return rc;
    }
    if (int rc = launch_fbank_normalize(c.logmel, c.fmask, c.stats, c.feats, c.amask, c.B, c.F, c.T, c.stream)) return rc;
    c.h->prof.end(c.stream);
    return 0;
}

// feature projection; padded rows zeroed (HF encoder entry)
int feature_projection(const Call& c) {
    const at_w2vbert* h = c.h;
    c.h->prof.begin("feature_projection", 2, c.stream);
    if (int rc = launch_layernorm(c.feats, h->fp_ln_g, h->fp_ln_b, nullptr, c.t1, c.M, kFeat, c.stream)) return rc;
    if (int rc = linear(c, c.t1, kFeat, h->fp_w, h->fp_b, c.x, kHid, EPI_NONE, 1.f, nullptr, c.amask, kHid)) return rc;
    c.h->prof.end(c.stream);
    return 0;
}

// The attention block of a split layer: LayerNorm -> q/k/v projection -> attention -> output projection + residual
int attention_split(const Call& c, const SplitCtx& sc, const LayerW& L) {
    Profiler& prof = c.h->prof;
    if (int rc = ln_split(c, sc, L, WS_LN_ATTN, L.ln_att_g, L.ln_att_b, nullptr)) return rc;
    prof.begin("attn_proj", 1, c.stream);
    // f16x2: the projection's epilogue writes k and v directly as fp16 pieces (q stays fp32 for the rel-pos table); the attention kernel
    // then stages K / V tiles without splitting them
    const bool kvp = sc.scheme == XB_SCHEME_F16X2;
    if (kvp) {
        if (int rc = qkv_split_gemm(sc, WS_QKV_KV, c.t1s, L.site_scale[WS_LN_ATTN], L.ws[sc.scheme][W_QKV], L.bqkv, kHid, c.M, c.Mpad, c.big, c.kvs, c.stream)) return rc;
    } else if (int rc = gemm_split(c, sc, L, W_QKV, c.t1s, L.bqkv, XB_EPI_LINEAR, 1.f, c.big, nullptr, nullptr)) {
        return rc;
    }
    prof.end(c.stream);
    prof.begin("attention", 1, c.stream);
    AttnArgs at;   // the context goes straight to the output projection as pieces
    at.qkv = c.big; at.amask = c.amask; at.dist_emb = L.dist; at.B = c.B; at.T = c.T; at.heads = 16;
    at.arith = kvp ? ARITH_F16X2 : ARITH_BF16X3;   // attention follows the layer's arithmetic
    at.status = sc.site(WS_ATTENTION); at.ctx_pieces = c.t1s; at.rows_pad = c.Mpad; at.kv_pieces = kvp ? c.kvs : nullptr; at.w8 = c.h->attn_w8; at.dist = L.dist_s;
    if (int rc = launch_relpos_attention(at, c.stream)) return rc;
    prof.end(c.stream);
    prof.begin("attn_proj", 1, c.stream);
    if (int rc = gemm_split(c, sc, L, W_O, c.t1s, L.bo, XB_EPI_LINEAR, 1.f, c.x, c.x, nullptr)) return rc;
    prof.end(c.stream);
    return 0;
}

// Conformer layer li on the split arithmetic: every GEMM operand is produced directly as K-blocked pieces — LayerNorm (launch_layernorm_split), the first
// FFN GEMM's swish epilogue, the attention kernel's context and the depthwise-conv kernel's output — so no fp32 activation is written only to be re-read
// by a split pass.
int conformer_layer_split(const Call& c, int li) {
    at_w2vbert* const h = c.h;
    Profiler& prof = h->prof;
    const LayerW& L = h->layers[li];
    const SplitCtx sc = c.ctx_of(li);
    if (li == 0)   // layers > 0: the previous layer's final LayerNorm wrote these pieces in the same pass (launch_layernorm2_split below)
        if (int rc = ln_split(c, sc, L, WS_LN_FFN1, L.ln_ffn1_g, L.ln_ffn1_b, nullptr)) return rc;
    prof.begin("ffn", 2, c.stream);
    if (int rc = gemm_split(c, sc, L, W_1A, c.t1s, L.b1a, XB_EPI_SWISH_SPLIT, 1.f, nullptr, nullptr, c.bigs)) return rc;
    if (int rc = gemm_split(c, sc, L, W_1B, c.bigs, L.b1b, XB_EPI_LINEAR, 0.5f, c.x, c.x, nullptr)) return rc;
    prof.end(c.stream);

    if (int rc = attention_split(c, sc, L)) return rc;

    if (int rc = ln_split(c, sc, L, WS_LN_CONV, L.ln_conv_g, L.ln_conv_b, c.amask)) return rc;
    prof.begin("conv_module", 3, c.stream);
    if (int rc = gemm_split(c, sc, L, W_PW1, c.t1s, nullptr, XB_EPI_GLU, 1.f, c.big, nullptr, nullptr)) return rc;
    if (int rc = (h->dwconv_stream ? launch_dwconv_stream : launch_dwconv_ln_swish)(c.big, L.dw, L.ln_dw_g, L.ln_dw_b, nullptr, c.B, c.T, c.stream,
                                                                                    sc.out(c.t1s, c.Mpad, L.site_scale[WS_DWCONV], sc.site(WS_DWCONV))))
        return rc;
    if (int rc = gemm_split(c, sc, L, W_PW2, c.t1s, nullptr, XB_EPI_LINEAR, 1.f, c.x, c.x, nullptr)) return rc;
    prof.end(c.stream);

    if (int rc = ln_split(c, sc, L, WS_LN_FFN2, L.ln_ffn2_g, L.ln_ffn2_b, nullptr)) return rc;
    prof.begin("ffn", 2, c.stream);
    if (int rc = gemm_split(c, sc, L, W_2A, c.t1s, L.b2a, XB_EPI_SWISH_SPLIT, 1.f, nullptr, nullptr, c.bigs)) return rc;
    if (int rc = gemm_split(c, sc, L, W_2B, c.bigs, L.b2b, XB_EPI_LINEAR, 0.5f, c.x, c.x, nullptr)) return rc;
    prof.end(c.stream);
    prof.begin("layernorm", 1, c.stream);
    if (li + 1 < c.n_layers) {
        // final_layer_norm of this layer and ffn1_layer_norm of the next in ONE pass over the residual stream: x = LN(x) as fp32 rows and
        // t1s = split(LN'(x)) (bit-identical to the two launches; saves one read of x per layer)
        const LayerW& Ln = h->layers[li + 1];
        const SplitCtx scn = c.ctx_of(li + 1);   // the pieces are the NEXT layer's operand: its scheme, its site scale, its range row
        if (int rc = launch_layernorm2_split(c.x, L.ln_fin_g, L.ln_fin_b, c.x, Ln.ln_ffn1_g, Ln.ln_ffn1_b, c.M, kHid,
                                             scn.out(c.t1s, c.Mpad, Ln.site_scale[WS_LN_FFN1], scn.site(WS_LN_FFN1)), c.stream))
            return rc;
    } else if (int rc = launch_layernorm(c.x, L.ln_fin_g, L.ln_fin_b, nullptr, c.x, c.M, kHid, c.stream)) {
        return rc;
    }
    prof.end(c.stream);
    return 0;
}

// Conformer layer li on the fp32 MFMA path
int conformer_layer_f32(const Call& c, int li) {
    at_w2vbert* const h = c.h;
    Profiler& prof = h->prof;
    const LayerW& L = h->layers[li];
    prof.begin("ffn", 3, c.stream);
    if (int rc = launch_layernorm(c.x, L.ln_ffn1_g, L.ln_ffn1_b, nullptr, c.t1, c.M, kHid, c.stream)) return rc;
    if (int rc = linear(c, c.t1, kHid, L.w1a, L.b1a, c.big, kFfn, EPI_SWISH, 1.f, nullptr, nullptr, kFfn)) return rc;
    if (int rc = linear(c, c.big, kFfn, L.w1b, L.b1b, c.x, kHid, EPI_NONE, 0.5f, c.x, nullptr, kHid)) return rc;
    prof.end(c.stream);
    prof.begin("attn_proj", 3, c.stream);
    if (int rc = launch_layernorm(c.x, L.ln_att_g, L.ln_att_b, nullptr, c.t1, c.M, kHid, c.stream)) return rc;
    if (int rc = linear(c, c.t1, kHid, L.wqkv, L.bqkv, c.big, 3 * kHid, EPI_NONE, 1.f, nullptr, nullptr, 3 * kHid)) return rc;
    prof.end(c.stream);
    prof.begin("attention", 1, c.stream);
    AttnArgs at;
    at.qkv = c.big; at.amask = c.amask; at.dist_emb = L.dist; at.ctx = c.t1; at.B = c.B; at.T = c.T; at.heads = 16; at.arith = ARITH_F32;
    if (int rc = launch_relpos_attention(at, c.stream)) return rc;
    prof.end(c.stream);
    prof.begin("attn_proj", 0, c.stream);
    if (int rc = linear(c, c.t1, kHid, L.wo, L.bo, c.x, kHid, EPI_NONE, 1.f, c.x, nullptr, kHid)) return rc;
    prof.end(c.stream);
    prof.begin("conv_module", 4, c.stream);
    if (int rc = launch_layernorm(c.x, L.ln_conv_g, L.ln_conv_b, c.amask, c.t1, c.M, kHid, c.stream)) return rc;
    if (int rc = linear(c, c.t1, kHid, L.pw1, nullptr, c.big, 2 * kHid, EPI_GLU, 1.f, nullptr, nullptr, kHid)) return rc;
    if (int rc = (h->dwconv_stream ? launch_dwconv_stream : launch_dwconv_ln_swish)(c.big, L.dw, L.ln_dw_g, L.ln_dw_b, c.t1, c.B, c.T, c.stream, SplitOut{})) return rc;
    if (int rc = linear(c, c.t1, kHid, L.pw2, nullptr, c.x, kHid, EPI_NONE, 1.f, c.x, nullptr, kHid)) return rc;
    prof.end(c.stream);
    prof.begin("ffn", 4, c.stream);
    if (int rc = launch_layernorm(c.x, L.ln_ffn2_g, L.ln_ffn2_b, nullptr, c.t1, c.M, kHid, c.stream)) return rc;
    if (int rc = linear(c, c.t1, kHid, L.w2a, L.b2a, c.big, kFfn, EPI_SWISH, 1.f, nullptr, nullptr, kFfn)) return rc;
    if (int rc = linear(c, c.big, kFfn, L.w2b, L.b2b, c.x, kHid, EPI_NONE, 0.5f, c.x, nullptr, kHid)) return rc;
    if (int rc = launch_layernorm(c.x, L.ln_fin_g, L.ln_fin_b, nullptr, c.x, c.M, kHid, c.stream)) return rc;
    prof.end(c.stream);
    return 0;
}

// non-affine LayerNorm (reference encoder.py:138-143,176) then nearest code (encoder.py:180-181)
int quantise(const Call& c, int16_t* tokens) {
    const at_w2vbert* h = c.h;
    const SplitCtx sc{scheme_of(h->arith), nullptr};   // the model's scheme; no range row (see score_split_gemm)
    c.h->prof.begin("vq", 3, c.stream);
    if (h->arith != ARITH_F32 && h->vq_split && h->cb_s[sc.scheme].p) {
        // the score GEMM on the split kernel: the LayerNorm writes its fp32 rows (|x|^2 of the distance) and the operand pieces in one pass
        if (int rc = launch_layernorm_split(c.x, nullptr, nullptr, nullptr, c.t1, c.M, kHid, sc.out(c.t1s, c.Mpad, XB_F16_ACT_SCALE, nullptr), c.stream)) return rc;
        if (int rc = score_split_gemm(sc, c.t1s, h->cb_s[sc.scheme], kCodes, kHid, c.M, c.Mpad, c.big, c.stream)) return rc;
    } else {
        if (int rc = launch_layernorm(c.x, nullptr, nullptr, nullptr, c.t1, c.M, kHid, c.stream)) return rc;
        if (int rc = linear(c, c.t1, kHid, h->codebook, nullptr, c.big, kCodes, EPI_NONE, 1.f, nullptr, nullptr, kCodes)) return rc;
    }
    if (int rc = launch_vq_argmax(c.t1, c.big, h->e2, tokens, c.M, kHid, kCodes, c.stream, c.status, 0, h->vq_refine ? h->codebook : nullptr)) return rc;
    c.h->prof.end(c.stream);
    return 0;
}

}  // namespace

extern "C" {

int at_w2vbert_encode(at_w2vbert_t* h, const float* wav, const float* mask, int B, int N, int pad_to_multiple_of, int n_layers,
                      int16_t* tokens, int* T_out, float* features_out, float* attn_mask_out, float* hidden_out, void* workspace,
                      size_t workspace_bytes, at_stream_t stream_) {
    return at_w2vbert_encode_checked(h, wav, mask, B, N, pad_to_multiple_of, n_layers, tokens, T_out, features_out, attn_mask_out, hidden_out,
                                     workspace, workspace_bytes, stream_, nullptr);
}

int at_w2vbert_encode_checked(at_w2vbert_t* h, const float* wav, const float* mask, int B, int N, int pad_to_multiple_of, int n_layers,
                              int16_t* tokens, int* T_out, float* features_out, float* attn_mask_out, float* hidden_out, void* workspace,
                              size_t workspace_bytes, at_stream_t stream_, int32_t* status_dev) {
    AT_REQUIRE(h && h->finalized, "model not finalized");
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    AT_REQUIRE(wav && workspace, "null pointer");
    AT_REQUIRE(B >= 1 && N >= kFrame + kHop, "need B >= 1 and at least two frames (N >= 560 samples)");
    AT_REQUIRE(n_layers >= 0 && n_layers <= (int)h->layers.size(), "n_layers exceeds the loaded layers");
    AT_REQUIRE(tokens == nullptr || h->codebook != nullptr, "tokens requested but no VQ codebook loaded");
    hipStream_t stream = (hipStream_t)stream_;
    const Plan p = make_plan(B, N, pad_to_multiple_of);
    AT_REQUIRE(workspace_bytes >= p.total_floats * sizeof(float), "workspace too small");
    AT_REQUIRE(p.Tp >= 1, "clip too short");
    if (T_out) *T_out = p.Tp;
    if (status_dev) AT_CHECK_HIP(hipMemsetAsync(status_dev, 0, sizeof(int32_t), stream));
    AT_REQUIRE(n_layers <= kRangeLayers, "more conformer layers than range-table rows");
    if (int rc = h->range.reset(stream)) return rc;

    float* ws = (float*)workspace;
    Call c{};
    c.h = h; c.stream = stream; c.B = B; c.N = N; c.F = p.F; c.T = p.Tp; c.n_layers = n_layers;
    c.M = (long long)B * p.Tp; c.BF = (long long)B * p.F; c.Mpad = (long long)p.Mpad;
    c.status = reinterpret_cast<int*>(status_dev);
    c.frames = reinterpret_cast<double*>(ws + p.off_frames);
    c.fmask = ws + p.off_fmask; c.spec = ws + p.off_spec; c.logmel = ws + p.off_logmel; c.stats = ws + p.off_stats;
    c.feats = features_out ? features_out : ws + p.off_feats;
    c.amask = attn_mask_out ? attn_mask_out : ws + p.off_amask;
    c.x = ws + p.off_x; c.t1 = ws + p.off_t1; c.big = ws + p.off_big;
    c.t1s = reinterpret_cast<piece_t*>(ws + p.off_t1s);
    c.bigs = reinterpret_cast<piece_t*>(ws + p.off_bigs);
    c.kvs = reinterpret_cast<piece_t*>(ws + p.off_kvs);

    if (int rc = front_end(c, wav, mask)) return rc;
    if (int rc = feature_projection(c)) return rc;
    for (int li = 0; li < n_layers; ++li)
        if (int rc = h->arith != ARITH_F32 ? conformer_layer_split(c, li) : conformer_layer_f32(c, li)) return rc;
    if (status_dev)   // every site's range verdict of this call -> the caller's status word
        if (int rc = launch_range_combine(h->range.dev, n_layers * (int)W_NSITES, c.status, stream)) return rc;
    if (hidden_out) AT_CHECK_HIP(hipMemcpyAsync(hidden_out, c.x, (size_t)c.M * kHid * sizeof(float), hipMemcpyDeviceToDevice, stream));
    if (tokens)
        if (int rc = quantise(c, tokens)) return rc;
    return 0;
}

int at_w2vbert_range_report(at_w2vbert_t* h, float* max_scaled, int cap) { return sem_range_report(h, "at_w2vbert_range_report", max_scaled, cap); }
// flags[l] = conformer layer l: `layers` entries
int at_w2vbert_layer_status(at_w2vbert_t* h, int32_t* flags, int cap) { return sem_layer_status(h, "at_w2vbert_layer_status", flags, cap); }
// The activation scale of every (layer, site): scales[l * n_sites + k], n_sites = at_w2vbert_range_sites. 16 everywhere unless a LayerNorm's gains force
// the provable scale of a LayerNorm-fed site below that (xb_ln_site_scale). Returns the number of floats written. Host-only.
int at_w2vbert_site_scales(const at_w2vbert_t* h, float* scales, int cap) {
    AT_REQUIRE(h && h->finalized && scales, "at_w2vbert_site_scales: bad arguments");
    const int n = (int)h->layers.size() * (int)W_NSITES;
    AT_REQUIRE(cap >= n, "at_w2vbert_site_scales: buffer too small");
    for (size_t l = 0; l < h->layers.size(); ++l)
        for (int k = 0; k < (int)W_NSITES; ++k) scales[l * W_NSITES + k] = h->layers[l].site_scale[k];
    return n;
}
int at_w2vbert_range_sites(char* names, size_t cap) { return range_sites(kWSiteNames, (int)W_NSITES, names, cap); }

}  // extern "C"
