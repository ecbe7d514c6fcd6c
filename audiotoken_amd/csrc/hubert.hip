// semantic_s tokenizer (mHuBERT-base -> LayerNorm -> k-means assignment) — host side. C ABI in
// include/audiotoken_hip.h. Replaces reference HubertEncoder (audiotoken/encoder.py:60-108): HF HubertModel
// hidden_states[output_layer = 11], non-affine LayerNorm(768), torch.cdist to 1000 centres + argmin.
// Arithmetic per SURVEY.md Appendix A.4 (HF modeling_hubert.py). fp32 on the f32 matrix cores throughout.
//
// Weight repacking at finalize():
//   feature-extractor convs [512][Cin][k] -> [512][k*Cin] (tap-major, channels-last windows); conv 0 keeps [512][10]
//   positional conv (weight-norm folded by the caller) [768][48][128], groups 16 -> 16 x [48][128*48]
//   q,k,v Linear -> one [2304][768]
// The encode entry point is checks, plan, the Call struct (make_call; the test tap at_hubert_features stops after the first stage), then one call per stage: feature_extractor, projection_posconv, transformer_layer per
// layer, quantise. Every split GEMM, the windowed conv chain included, goes through split_gemm_args (semantic_handle.h), which owns the f16x2 scale rule.
#include <string>
#include <vector>
#include <cstring>

#include "../../include/audiotoken_hip.h"
#include "semantic_handle.h"
#include "hubert_kernels.h"
#include "w2vbert_kernels.h"

using namespace at;

namespace {
constexpr int kCd = 512, kHid = 768, kFfn = 3072, kHeads = 12, kPosK = 128, kGroups = 16, kGc = 48, kCenters = 1000, kCentersPad = 1024;
constexpr int kKs[7] = {10, 3, 3, 3, 3, 2, 2}, kSt[7] = {5, 2, 2, 2, 2, 2, 2};

enum { HW_QKV = 0, HW_O, HW_1, HW_2, HW_NLINEAR };
// output x input width of the four linear layers
constexpr int kWN[HW_NLINEAR] = {3 * kHid, kHid, kFfn, kHid}, kWK[HW_NLINEAR] = {kHid, kHid, kHid, kFfn};

struct LayerW {
    const float *wqkv, *bqkv, *wo, *bo, *ln1_g, *ln1_b, *w1, *b1, *w2, *b2, *ln2_g, *ln2_b;
    SplitW ws[2][HW_NLINEAR];   // the four linear layers as operand pieces per scheme [XB_SCHEME_*][HW_*] (gemm_bf16x3.h)
    // f16x2: the activation scales of the two LayerNorm-fed split sites of this layer — the input of the q/k/v projection (written by the previous
    // layer's final_layer_norm, or encoder.layer_norm for layer 0) and the input of the first FFN GEMM (this layer's layer_norm): 16 unless the
    // LayerNorm's gains force the provable scale below that (xb_ln_site_scale, gemm_bf16x3.h)
    float xs_qkv = XB_F16_ACT_SCALE, xs_ffn = XB_F16_ACT_SCALE;
};

// Sites of the handle's range table (semantic_handle.h, RangeTable): where activations become fp16 pieces
enum HSite { HS_CONV0 = 0, HS_FE_CONV, HS_X_IN, HS_QKV_KV, HS_ATTENTION, HS_FFN_HIDDEN, HS_OTHER, H_NSITES };
static const char* const kHSiteNames[H_NSITES] = {"conv0_out", "feature_convs", "layer_input", "qkv_kv", "attention", "ffn_hidden", "other"};
// rows of the range table: row 0 = conv feature encoder + positional conv, row 1 + l = transformer layer l, up to 32 layers
constexpr int kRangeRows = 33, kRangeLayer0 = 1;

// what finalize builds on the device
struct HubertW {
    const float* conv_w[7] = {};
    const float *gn_g = nullptr, *gn_b = nullptr, *fp_ln_g = nullptr, *fp_ln_b = nullptr, *fp_w = nullptr, *fp_b = nullptr;
    const float *pos_w = nullptr, *pos_b = nullptr, *enc_ln_g = nullptr, *enc_ln_b = nullptr;
    std::vector<LayerW> layers;
    const float *centers = nullptr, *c2 = nullptr;
    SplitW conv_s[2][7];   // conv weights of layers 1..6 as operand pieces, per scheme
    SplitW pos_s;          // positional-conv weights as fp16 pieces in the per-K-step layout of hubert_posconv.hip (f16x2 scheme only)
    SplitW cen_s[2];       // the k-means centres as operand pieces per scheme, rows padded 1000 -> 1024 (zero rows): the score GEMM on the split kernel
};
}  // namespace

struct at_hubert : SemanticHandle, HubertW {
    bool kmeans_split = true;            // option "kmeans_split": the score GEMM on the split kernel instead of the fp32 MFMA (as at_w2vbert's "vq_split")
    bool ln_split = true;                // option "ln_split" (round 5): the post-LN LayerNorms write the fp32 residual stream AND the next GEMM's operand pieces in one pass (launch_layernorm_split, D = 768) instead of LayerNorm + a separate split pass; bit-identical
    bool posconv_split = true;           // option "posconv_split": the LDS-resident grouped conv kernel (hubert_posconv.hip) instead of 16 fp32 windowed GEMMs
    explicit at_hubert(int device_id) : SemanticHandle(PACKED_MODEL_HUBERT, device_id, RangeTable{kRangeRows, (int)H_NSITES, kRangeLayer0}) {
        bool_opts = {{"posconv_split", &posconv_split}, {"ln_split", &ln_split}, {"kmeans_split", &kmeans_split}};
    }
    int finalize_model() override;
    int split_model(int scheme) override;
    void forget_model() override { static_cast<HubertW&>(*this) = HubertW{}; }
    int num_layers() const override { return (int)layers.size(); }
    bool has_codes() const override { return centers != nullptr; }
};

namespace {

struct Plan {
    int L[8];   // L[0] = N, L[i+1] = frames after conv i
    size_t off_a, off_b, off_part, off_ss, off_fmask, off_x, off_t1, off_big, off_pos, off_xs, off_bigs, off_kvs;
    size_t Mpad;
    int Lp[8];              // rows per phase plane of the split-bf16 input of conv i (i = 1..6)
    int Mp[8];              // padded output rows per clip of conv i
    size_t off_sa, off_sb;  // split-bf16 ping / pong buffers of the conv chain
    size_t total_floats;
};
Plan make_plan(int B, int N) {
    Plan p;
    p.L[0] = N;
    for (int i = 0; i < 7; ++i) p.L[i + 1] = p.L[i] >= kKs[i] ? (p.L[i] - kKs[i]) / kSt[i] + 1 : 0;
    size_t cur = 0;
    auto takef = [&](size_t n) { size_t o = cur; cur += (n + 63) / 64 * 64; return o; };
    const size_t T = p.L[7], M = (size_t)B * T;
    p.off_a = takef((size_t)B * p.L[1] * kCd);     // ping: conv 0, 2, 4, 6 outputs
    p.off_b = takef((size_t)B * p.L[2] * kCd);     // pong: conv 1, 3, 5 outputs
    p.off_part = takef((size_t)B * hub_ws_nchunk(p.L[1] > 0 ? p.L[1] : 1) * 65 * 2);   // doubles
    p.off_ss = takef((size_t)B * kCd * 2);
    p.off_fmask = takef(M);
    p.off_x = takef(M * kHid);
    p.off_t1 = takef(M * kHid);
    p.off_pos = takef(M * kHid);
    p.off_big = takef(M * kFfn);
    p.Mpad = (M + 255) / 256 * 256;                 // split-bf16 operands: 3 pieces x 2 bytes = 1.5 floats per element
    {
        size_t need[2] = {0, 0};
        for (int i = 1; i < 7; ++i) {
            p.Mp[i] = (p.L[i + 1] + 255) / 256 * 256;
            // phase-major time axis: kSt planes of Lp rows each; the last tile of tap j reads rows up to Mp + (k - 1) / stride
            const int reach = p.Mp[i] + (kKs[i] - 1) / kSt[i], have = (p.L[i] + kSt[i] - 1) / kSt[i];
            p.Lp[i] = ((have > reach ? have : reach) + 63) / 64 * 64;
            const size_t fl = (size_t)B * kSt[i] * p.Lp[i] * kCd * 3 / 2 + 64;   // 3 pieces x 2 bytes per element, in floats
            if (fl > need[i & 1]) need[i & 1] = fl;
        }
        p.off_sa = takef(need[1]);   // inputs of conv 1, 3, 5
        p.off_sb = takef(need[0]);   // inputs of conv 2, 4, 6
    }
    p.off_xs = takef(p.Mpad * kHid * 3 / 2);
    p.off_bigs = takef(p.Mpad * kFfn * 3 / 2);
    p.off_kvs = takef(p.Mpad * kHid * 2);           // k and v as two fp16 pieces each (XB_EPI_QKV)
    p.total_floats = cur;
    return p;
}

// ---- finalize: the staged tensors of one part of the model -> device, in the order the packed blob records ---------------------------------------
// feature-extractor conv i [512][Cin][k] -> [512][k * Cin] (tap-major, channels-last windows)
int take_conv(at_hubert* h, int i) {
    const int cin = i == 0 ? 1 : kCd, k = kKs[i];
    if (int rc = take_repacked(h, (size_t)kCd * k * cin, &h->conv_w[i], [&](std::vector<float>& w) {
            const std::string key = "feature_extractor.conv_layers." + std::to_string(i) + ".conv.weight";
            const HostTensor* t = find(h, key);
            AT_REQUIRE(t && t->shape == (std::vector<int64_t>{kCd, cin, k}), "missing / mis-shaped " + key);
            for (int co = 0; co < kCd; ++co)
                for (int ci = 0; ci < cin; ++ci)
                    for (int tp = 0; tp < k; ++tp) w[((size_t)co * k + tp) * cin + ci] = t->data[((size_t)co * cin + ci) * k + tp];
            return 0;
        }))
        return rc;
    AT_REQUIRE(h->conv_w[i] != nullptr, h->arena.importing ? "import_packed: feature-extractor weights" : "device allocation failed");
    return 0;
}

// grouped positional conv: folded weight [768][48][128] -> per group [48 out][128 taps][48 in]
int take_posconv(at_hubert* h) {
    if (int rc = take_repacked(h, (size_t)kHid * kPosK * kGc, &h->pos_w, [&](std::vector<float>& w) {
            const HostTensor* t = find(h, "encoder.pos_conv_embed.conv.weight");
            AT_REQUIRE(t && t->shape == (std::vector<int64_t>{kHid, kGc, kPosK}), "encoder.pos_conv_embed.conv.weight [768,48,128] (weight-norm folded) missing");
            for (int co = 0; co < kHid; ++co)
                for (int ci = 0; ci < kGc; ++ci)
                    for (int tp = 0; tp < kPosK; ++tp) w[((size_t)co * kPosK + tp) * kGc + ci] = t->data[((size_t)co * kGc + ci) * kPosK + tp];
            return 0;
        }))
        return rc;
    AT_REQUIRE(h->pos_w != nullptr, h->arena.importing ? "import_packed: positional conv" : "device allocation failed");
    return 0;
}

// transformer layer i; its q/k/v input site is fed by the LayerNorm before it (the previous layer's final_layer_norm, or encoder.layer_norm)
int take_layer(at_hubert* h, int i, LayerW& L) {
    static const char* const kQkv[3] = {"q_proj", "k_proj", "v_proj"};
    const std::string p = "encoder.layers." + std::to_string(i);
    bool ok = true;
    if (int rc = take_qkv(h, p + ".attention.", kQkv, kHid, &L.wqkv, &L.bqkv)) return rc;
    AT_REQUIRE(L.wqkv && L.bqkv, "device allocation failed");
    L.wo = take(h, p + ".attention.out_proj.weight", {kHid, kHid}, ok);
    L.bo = take(h, p + ".attention.out_proj.bias", {kHid}, ok);
    L.ln1_g = take(h, p + ".layer_norm.weight", {kHid}, ok);
    L.ln1_b = take(h, p + ".layer_norm.bias", {kHid}, ok);
    L.w1 = take(h, p + ".feed_forward.intermediate_dense.weight", {kFfn, kHid}, ok);
    L.b1 = take(h, p + ".feed_forward.intermediate_dense.bias", {kFfn}, ok);
    L.w2 = take(h, p + ".feed_forward.output_dense.weight", {kHid, kFfn}, ok);
    L.b2 = take(h, p + ".feed_forward.output_dense.bias", {kHid}, ok);
    L.ln2_g = take(h, p + ".final_layer_norm.weight", {kHid}, ok);
    L.ln2_b = take(h, p + ".final_layer_norm.bias", {kHid}, ok);
    if (!ok) return -1;
    const bool first = h->layers.empty();
    L.xs_qkv = ln_site_scale(h, first ? h->enc_ln_g : h->layers.back().ln2_g, first ? h->enc_ln_b : h->layers.back().ln2_b, kHid);
    L.xs_ffn = ln_site_scale(h, L.ln1_g, L.ln1_b, kHid);
    return 0;
}

// k-means centres [1000][768] and their squared norms
int take_centres(at_hubert* h) {
    if (h->arena.importing) {
        if (h->imp.flags & 1) {
            h->centers = reserve(h, (size_t)kCenters * kHid);
            h->c2 = reserve(h, kCenters);
            AT_REQUIRE(h->centers && h->c2, "import_packed: k-means centres");
        }
        return 0;
    }
    const HostTensor* c = find(h, "kmeans.cluster_centers_");
    if (!c) return 0;
    AT_REQUIRE(c->shape.size() == 2 && c->shape[1] == kHid && c->shape[0] % 4 == 0, "kmeans.cluster_centers_ must be [C,768], C % 4 == 0");
    h->centers = upload(h, c->data);
    const int C = (int)c->shape[0];
    AT_REQUIRE(C == kCenters, "this build is sized for 1000 centres");
    const HostTensor* e = find(h, "kmeans.c2");
    if (e) AT_REQUIRE(e->data.size() == (size_t)C, "bad kmeans.c2 shape");
    h->c2 = upload(h, e ? e->data : code_norms(c->data, C, kHid));
    AT_REQUIRE(h->centers && h->c2, "device allocation failed");
    return 0;
}

}  // namespace

// Split the conv chain's and the transformer's weights into the 16-bit pieces of `scheme`
int at_hubert::split_model(int scheme) {
    for (int i = 1; i < 7; ++i)
        if (int rc = split_one(this, scheme, conv_w[i], kCd, kKs[i] * kCd, &conv_s[scheme][i], 0, kCd / 16, kSt[i])) return rc;   // window order
    if (scheme == XB_SCHEME_F16X2) {   // the positional conv's weights in hubert_posconv.hip's layout ([group][K step][piece][k-block][48][16])
        piece_t* d = static_cast<piece_t*>(arena.alloc(posconv_weight_pieces_bytes()));
        if (!d) return -1;
        float s = 1.f;
        if (int rc = weight_scale(this, pos_w, &s)) return rc;
        if (!arena.importing)
            if (int rc = launch_posconv_weight_split(pos_w, d, s, nullptr)) return rc;
        pos_s = SplitW{d, s};
    }
    for (LayerW& L : layers) {
        const float* src[HW_NLINEAR] = {L.wqkv, L.wo, L.w1, L.w2};
        for (int j = 0; j < HW_NLINEAR; ++j)
            if (int rc = split_one(this, scheme, src[j], kWN[j], kWK[j], &L.ws[scheme][j])) return rc;
    }
    if (centers)   // k-means centres [1000][768] -> pieces of 1024 rows (the last 24 zero: their scores are never read)
        if (int rc = split_one(this, scheme, centers, kCenters, kHid, &cen_s[scheme], kCentersPad)) return rc;
    return 0;
}

// The model part of finalize(): staged host tensors -> device (semantic_handle.h, finalize_model)
int at_hubert::finalize_model() {
    for (int i = 0; i < 7; ++i)
        if (int rc = take_conv(this, i)) return rc;
    bool ok = true;
    gn_g = take(this, "feature_extractor.conv_layers.0.layer_norm.weight", {kCd}, ok);
    gn_b = take(this, "feature_extractor.conv_layers.0.layer_norm.bias", {kCd}, ok);
    fp_ln_g = take(this, "feature_projection.layer_norm.weight", {kCd}, ok);
    fp_ln_b = take(this, "feature_projection.layer_norm.bias", {kCd}, ok);
    fp_w = take(this, "feature_projection.projection.weight", {kHid, kCd}, ok);
    fp_b = take(this, "feature_projection.projection.bias", {kHid}, ok);
    pos_b = take(this, "encoder.pos_conv_embed.conv.bias", {kHid}, ok);
    enc_ln_g = take(this, "encoder.layer_norm.weight", {kHid}, ok);
    enc_ln_b = take(this, "encoder.layer_norm.bias", {kHid}, ok);
    if (!ok) return -1;
    if (int rc = take_posconv(this)) return rc;
    int nl = arena.importing ? imp.n_layers : 0;
    while (!arena.importing && find(this, "encoder.layers." + std::to_string(nl) + ".layer_norm.weight")) ++nl;
    for (int i = 0; i < nl; ++i) {
        LayerW L{};
        if (int rc = take_layer(this, i, L)) return rc;
        layers.push_back(L);
    }
    return take_centres(this);
}

extern "C" {

at_hubert_t* at_hubert_create(int device_id) { return device_exists("at_hubert_create", device_id) ? new at_hubert(device_id) : nullptr; }
int at_hubert_set_tensor(at_hubert_t* h, const char* name, const float* host_data, const int64_t* shape, int ndim) {
    return stage_tensor(h, name, host_data, shape, ndim);
}
int at_hubert_finalize(at_hubert_t* h) { return sem_finalize(h); }
int64_t at_hubert_packed_bytes(at_hubert_t* h) { return sem_packed_bytes(h, "at_hubert_packed_bytes"); }
int64_t at_hubert_packed_meta(at_hubert_t* h, void* host_dst, int64_t cap) { return sem_packed_meta(h, "at_hubert_packed_meta", host_dst, cap); }
int at_hubert_export_packed(at_hubert_t* h, void* device_dst, int64_t bytes, void* stream) {
    return sem_export_packed(h, "at_hubert_export_packed", device_dst, bytes, stream);
}
int at_hubert_import_packed(at_hubert_t* h, const void* host_meta, int64_t meta_bytes, const void* device_src, int64_t bytes, void* stream) {
    return sem_import_packed(h, "at_hubert_import_packed", host_meta, meta_bytes, device_src, bytes, stream);
}
void at_hubert_destroy(at_hubert_t* h) { sem_destroy(h); }

int at_hubert_num_layers(const at_hubert_t* h) { return h ? (int)h->layers.size() : 0; }

int at_hubert_num_tokens(int N) {
    int L = N;
    for (int i = 0; i < 7; ++i) L = L >= kKs[i] ? (L - kKs[i]) / kSt[i] + 1 : 0;
    return L;
}

size_t at_hubert_workspace_bytes(const at_hubert_t* h, int B, int N) {
    if (B <= 0 || at_hubert_num_tokens(N) <= 0) return 0;
    return make_plan(B, N).total_floats * sizeof(float);
}

int at_hubert_set_option(at_hubert_t* h, const char* name, int value) { return sem_set_option(h, "at_hubert_set_option", name, value); }
int at_hubert_get_option(const at_hubert_t* h, const char* name) { return sem_get_option(h, name); }

}  // extern "C"

// ---- encode -------------------------------------------------------------------------------------------------------------------------------------
namespace {

// One encode call: the model, the shapes, the stream and the workspace the plan carved
struct Call {
    at_hubert* h;
    const Plan* p;
    hipStream_t stream;
    int B, N, T, n_layers;
    long long M, Mpad;   // token rows, and padded for the split operands
    int* status;         // the caller's status word (nullable)
    bool split;          // the linear layers and the conv chain run on the split kernels (arith != f32)
    // The LayerNorm that writes x also writes the pieces of x its consumer's first GEMM reads (option "ln_split"): true for every LayerNorm whose consumer
    // is one of the n_layers layers that run, so inside a layer "xs holds split(x)" is this value, at the q/k/v projection and at the first FFN GEMM alike
    bool ln_pieces;
    float *conv_a, *conv_b, *part, *ss, *fmask, *x, *t1, *pos, *big;   // conv_a / conv_b: ping (conv 0, 2, 4, 6 outputs) / pong
    piece_t *conv_sa, *conv_sb, *xs, *bigs, *kvs;                       // conv_sa / conv_sb: pieces in of conv 1, 3, 5 / conv 2, 4, 6
    const float* feats() const { return conv_a; }                       // [B][T][512], the last conv's output
    SplitCtx front() const { return SplitCtx{scheme_of(h->arith), h->range.dev}; }   // the front end (row 0) and the k-means GEMM
    // transformer layer l: its own row of the range table and, when the range fallback has pinned it (option "layer_arith:<l>"), its own arithmetic
    SplitCtx ctx_of(int li) const { return SplitCtx{scheme_of(h->arith_of(li)), h->range.layer_row(li)}; }
};

// The Call of one entry into the model: shapes from the plan, every buffer a slice of the caller's workspace (make_plan's offsets)
Call make_call(at_hubert* h, const Plan& p, int B, int N, int n_layers, void* workspace, hipStream_t stream, int32_t* status_dev) {
    float* ws = (float*)workspace;
    Call c{};
    c.h = h; c.p = &p; c.stream = stream; c.B = B; c.N = N; c.T = p.L[7]; c.n_layers = n_layers;
    c.M = (long long)B * c.T; c.Mpad = (long long)p.Mpad;
    c.status = reinterpret_cast<int*>(status_dev);
    c.split = h->arith != ARITH_F32;
    c.ln_pieces = c.split && h->ln_split;
    c.conv_a = ws + p.off_a; c.conv_b = ws + p.off_b; c.part = ws + p.off_part; c.ss = ws + p.off_ss;
    c.fmask = ws + p.off_fmask; c.x = ws + p.off_x; c.t1 = ws + p.off_t1; c.pos = ws + p.off_pos; c.big = ws + p.off_big;
    c.conv_sa = reinterpret_cast<piece_t*>(ws + p.off_sa);
    c.conv_sb = reinterpret_cast<piece_t*>(ws + p.off_sb);
    c.xs = reinterpret_cast<piece_t*>(ws + p.off_xs);
    c.bigs = reinterpret_cast<piece_t*>(ws + p.off_bigs);
    c.kvs = reinterpret_cast<piece_t*>(ws + p.off_kvs);
    return c;
}

int linear(const Call& c, const float* X, int K, const float* W, const float* bias, float* C, int N, int epi, const float* R, const float* row_mask, int ldc) {
    GemmArgs a;
    a.X = X; a.Tin = (int)c.M; a.Cin = K; a.ldx = K;
    a.W = W; a.bias = bias; a.C = C; a.ldc = ldc; a.R = R; a.ldr = ldc;
    a.M = (int)c.M; a.N = N; a.K = K; a.batch = 1; a.epi = epi; a.row_mask = row_mask;
    return launch_gemm(a, c.stream);
}

// C / S = epi(A . W^T) of linear layer w on the split GEMM. A = the pieces in c.xs (or c.bigs for the second FFN GEMM), split with the f16x2 scale
// a_f16; X != nullptr: c.xs does not hold them yet — the fp32 rows X are split into it first
int linear_split(const Call& c, const SplitCtx& sc, const LayerW& L, int w, const float* X, float a_f16, const float* bias, int epi, float* C, const float* R,
                 piece_t* S) {
    const int N = kWN[w], K = kWK[w];
    // HS_X_IN is also this site: a context or hidden row split on the way into a GEMM reports where the LayerNorm-written layer input does
    if (X)
        if (int rc = launch_split_blocked(X, K, c.M, c.Mpad, K, c.xs, c.stream, sc.scheme, sc.act(a_f16), sc.site(HS_X_IN))) return rc;
    Bf16x3Args a = split_gemm_args(sc.scheme, w == HW_2 ? c.bigs : c.xs, sc.act(a_f16), L.ws[sc.scheme][w], c.M, N, K, c.Mpad, epi,
                                   sc.site(w == HW_1 ? HS_FFN_HIDDEN : HS_OTHER), sc.act());
    a.bias = bias; a.C = C; a.ldc = N; a.R = R; a.ldr = N; a.alpha = 1.0f; a.S = S; a.Spad = (int)c.Mpad;
    return launch_gemm_bf16x3(a, c.stream);
}

// x = LayerNorm(src) and, when layer `consumer` runs and ln_pieces, xs = split(x) in the same pass. The pieces are the CONSUMING layer's operand: its
// scheme, its site scale (for_qkv: the q/k/v projection's input, else the first FFN GEMM's) and its range row
int ln_to(const Call& c, const float* src, const float* g, const float* b, int consumer, bool for_qkv) {
    if (c.ln_pieces && consumer < c.n_layers) {
        const SplitCtx sc = c.ctx_of(consumer);
        const LayerW& Lc = c.h->layers[consumer];
        return launch_layernorm_split(src, g, b, nullptr, c.x, c.M, kHid, sc.out(c.xs, c.Mpad, for_qkv ? Lc.xs_qkv : Lc.xs_ffn, sc.site(HS_X_IN)), c.stream);
    }
    return launch_layernorm(src, g, b, nullptr, c.x, c.M, kHid, c.stream);
}

// the six 512 -> 512 convs as windowed split GEMMs (gemm_bf16x3.hip): conv0 writes the K-blocked pieces of its output, every conv's GELU epilogue
// writes the next conv's input the same way, the last one writes fp32 features. The common fields and the scale rule come from split_gemm_args.
int conv_chain_split(const Call& c, const float* wav) {
    const at_hubert* h = c.h;
    const Plan& p = *c.p;
    const SplitCtx sc = c.front();
    piece_t* sb[2] = {c.conv_sb, c.conv_sa};   // [i & 1]: the input of conv i
    if (int rc = launch_hub_conv0_gn_gelu(wav, h->conv_w[0], h->gn_g, h->gn_b, c.part, c.ss, nullptr, c.B, c.N, p.L[1], c.stream, sb[1], p.Lp[1], sc.scheme,
                                          sc.act(), sc.site(HS_CONV0)))
        return rc;
    for (int i = 1; i < 7; ++i) {
        Bf16x3Args a = split_gemm_args(sc.scheme, sb[i & 1], sc.act(), h->conv_s[sc.scheme][i], p.L[i + 1], kCd, kKs[i] * kCd, p.Mp[i],
                                       i < 6 ? XB_EPI_GELU_SPLIT : XB_EPI_GELU, sc.site(HS_FE_CONV), sc.act());
        a.batch = c.B; a.stride = kSt[i]; a.cblocks = kCd / 16; a.Lp = p.Lp[i];
        if (i < 6) { a.S = sb[(i + 1) & 1]; a.Spad = p.Lp[i + 1]; a.Sphases = kSt[i + 1]; }
        else { a.C = c.conv_a; a.ldc = kCd; }
        if (int rc = launch_gemm_bf16x3(a, c.stream)) return rc;
    }
    return 0;
}

int conv_chain_f32(const Call& c, const float* wav) {
    const at_hubert* h = c.h;
    const Plan& p = *c.p;
    float* bufs[2] = {c.conv_a, c.conv_b};
    if (int rc = launch_hub_conv0_gn_gelu(wav, h->conv_w[0], h->gn_g, h->gn_b, c.part, c.ss, bufs[0], c.B, c.N, p.L[1], c.stream)) return rc;
    for (int i = 1; i < 7; ++i) {
        GemmArgs a;
        a.X = bufs[(i - 1) & 1]; a.x_bstride = (long long)p.L[i] * kCd; a.Tin = p.L[i]; a.Cin = kCd; a.ldx = kCd;
        a.ktaps = kKs[i]; a.stride = kSt[i]; a.pad_left = 0; a.pad_mode = 0;
        a.W = h->conv_w[i];
        a.C = bufs[i & 1]; a.c_bstride = (long long)p.L[i + 1] * kCd; a.ldc = kCd;
        a.M = p.L[i + 1]; a.N = kCd; a.K = kKs[i] * kCd; a.batch = c.B; a.epi = EPI_GELU;
        if (int rc = launch_gemm(a, c.stream)) return rc;
    }
    return 0;
}

// conv feature encoder (7 valid strided convs, GroupNorm after the first, GELU). conv0 + GroupNorm + GELU: statistics from float64 waveform moments,
// one pass over the output (hubert_kernels.hip)
int feature_extractor(const Call& c, const float* wav) {
    c.h->prof.begin("feature_extractor", 9, c.stream);
    if (int rc = c.split ? conv_chain_split(c, wav) : conv_chain_f32(c, wav)) return rc;
    c.h->prof.end(c.stream);
    return 0;
}

// feature projection, zero padded frames, positional conv, LayerNorm (HF encoder entry)
int projection_posconv(const Call& c, const float* mask) {
    const at_hubert* h = c.h;
    const SplitCtx sc = c.front();
    c.h->prof.begin("projection_posconv", 20, c.stream);
    if (int rc = launch_hub_frame_mask(mask, c.fmask, c.B, c.N, c.T, c.stream)) return rc;
    if (int rc = launch_layernorm(c.feats(), h->fp_ln_g, h->fp_ln_b, nullptr, c.t1, c.M, kCd, c.stream)) return rc;
    if (int rc = linear(c, c.t1, kCd, h->fp_w, h->fp_b, c.x, kHid, EPI_NONE, nullptr, c.fmask, kHid)) return rc;
    if (c.split && sc.scheme == XB_SCHEME_F16X2 && h->pos_s.p && h->posconv_split) {
        // all 16 groups in one launch on the split scheme, the input tile resident in LDS (hubert_posconv.hip)
        if (int rc = launch_hubert_posconv(c.x, h->pos_s.p, h->pos_b, c.pos, c.B, c.T, h->pos_s.s, sc.site(HS_X_IN), c.stream)) return rc;
    } else {
        for (int g = 0; g < kGroups; ++g) {   // pos[b][t][g*48 + co] = x + gelu(conv_g(x) + bias)
            GemmArgs a;
            a.X = c.x + g * kGc; a.x_bstride = (long long)c.T * kHid; a.Tin = c.T; a.Cin = kGc; a.ldx = kHid;
            a.ktaps = kPosK; a.stride = 1; a.pad_left = kPosK / 2; a.pad_mode = 0;
            a.W = h->pos_w + (size_t)g * kGc * kPosK * kGc; a.bias = h->pos_b + g * kGc;
            a.C = c.pos + g * kGc; a.c_bstride = (long long)c.T * kHid; a.ldc = kHid;
            a.R = c.x + g * kGc; a.r_bstride = (long long)c.T * kHid; a.ldr = kHid;
            a.M = c.T; a.N = kGc; a.K = kPosK * kGc; a.batch = c.B; a.epi = EPI_GELU;
            if (int rc = launch_gemm(a, c.stream)) return rc;
        }
    }
    if (int rc = ln_to(c, c.pos, h->enc_ln_g, h->enc_ln_b, 0, true)) return rc;
    c.h->prof.end(c.stream);
    return 0;
}

// Transformer layer li (post-LN), on the split kernels or the fp32 MFMA. On entry x is the layer input; xs holds split(x) iff c.ln_pieces.
int transformer_layer(const Call& c, int li) {
    at_hubert* const h = c.h;
    Profiler& prof = h->prof;
    const LayerW& L = h->layers[li];
    const SplitCtx sc = c.ctx_of(li);   // this layer's scheme and range row
    const float* unsplit_x = c.ln_pieces ? nullptr : c.x;
    prof.begin("attn_proj", 3, c.stream);
    // f16x2: the projection's epilogue writes k / v as fp16 pieces, the attention kernel stages them unsplit and writes its context as the
    // output projection's operand pieces (as in w2vbert.hip)
    const bool kvp = c.split && sc.scheme == XB_SCHEME_F16X2;
    if (kvp) {
        if (unsplit_x)
            if (int rc = launch_split_blocked(c.x, kHid, c.M, c.Mpad, kHid, c.xs, c.stream, sc.scheme, L.xs_qkv, sc.site(HS_X_IN))) return rc;
        if (int rc = qkv_split_gemm(sc, HS_QKV_KV, c.xs, L.xs_qkv, L.ws[sc.scheme][HW_QKV], L.bqkv, kHid, c.M, c.Mpad, c.big, c.kvs, c.stream)) return rc;
    } else if (c.split) {
        if (int rc = linear_split(c, sc, L, HW_QKV, unsplit_x, L.xs_qkv, L.bqkv, XB_EPI_LINEAR, c.big, nullptr, nullptr)) return rc;
    } else if (int rc = linear(c, c.x, kHid, L.wqkv, L.bqkv, c.big, 3 * kHid, EPI_NONE, nullptr, nullptr, 3 * kHid)) {
        return rc;
    }
    prof.end(c.stream);
    prof.begin("attention", 1, c.stream);
    AttnArgs at;   // split: the context is written as the output projection's operand pieces; attention follows the layer's arithmetic
    at.qkv = c.big; at.amask = c.fmask; at.ctx = c.split ? nullptr : c.t1; at.B = c.B; at.T = c.T; at.heads = kHeads;
    at.arith = c.split ? h->arith_of(li) : ARITH_F32;
    at.status = sc.site(HS_ATTENTION); at.ctx_pieces = c.split ? c.xs : nullptr; at.rows_pad = c.Mpad; at.kv_pieces = kvp ? c.kvs : nullptr; at.w8 = h->attn_w8;
    if (int rc = launch_relpos_attention(at, c.stream)) return rc;
    prof.end(c.stream);
    prof.begin("attn_proj", 0, c.stream);
    if (c.split) {
        if (int rc = linear_split(c, sc, L, HW_O, nullptr, XB_F16_ACT_SCALE, L.bo, XB_EPI_LINEAR, c.x, c.x, nullptr)) return rc;
    } else if (int rc = linear(c, c.t1, kHid, L.wo, L.bo, c.x, kHid, EPI_NONE, c.x, nullptr, kHid)) {
        return rc;
    }
    if (int rc = ln_to(c, c.x, L.ln1_g, L.ln1_b, li, false)) return rc;
    prof.end(c.stream);
    prof.begin("ffn", 3, c.stream);
    if (c.split) {   // hidden activation written split by the first GEMM's epilogue
        if (int rc = linear_split(c, sc, L, HW_1, unsplit_x, L.xs_ffn, L.b1, XB_EPI_GELU_SPLIT, nullptr, nullptr, c.bigs)) return rc;
        if (int rc = linear_split(c, sc, L, HW_2, nullptr, XB_F16_ACT_SCALE, L.b2, XB_EPI_LINEAR, c.x, c.x, nullptr)) return rc;
    } else {
        if (int rc = linear(c, c.x, kHid, L.w1, L.b1, c.big, kFfn, EPI_GELU, nullptr, nullptr, kFfn)) return rc;
        if (int rc = linear(c, c.big, kFfn, L.w2, L.b2, c.x, kHid, EPI_NONE, c.x, nullptr, kHid)) return rc;
    }
    if (int rc = ln_to(c, c.x, L.ln2_g, L.ln2_b, li + 1, true)) return rc;     // (the last layer: plain LayerNorm, nothing consumes pieces)
    prof.end(c.stream);
    return 0;
}

// non-affine LayerNorm, then the nearest of the 1000 centres
int quantise(const Call& c, int16_t* tokens) {
    const at_hubert* h = c.h;
    const SplitCtx sc = c.front();
    const float* refine = h->vq_refine ? h->centers : nullptr;
    c.h->prof.begin("kmeans", 3, c.stream);
    if (int rc = launch_layernorm(c.x, nullptr, nullptr, nullptr, c.t1, c.M, kHid, c.stream)) return rc;
    if (c.split && h->kmeans_split && h->cen_s[sc.scheme].p) {
        // the score GEMM on the split kernel against the centres padded to 1024 rows; no range site (see score_split_gemm)
        if (int rc = launch_split_blocked(c.t1, kHid, c.M, c.Mpad, kHid, c.xs, c.stream, sc.scheme, sc.act(), nullptr)) return rc;
        if (int rc = score_split_gemm(sc, c.xs, h->cen_s[sc.scheme], kCentersPad, kHid, c.M, c.Mpad, c.big, c.stream)) return rc;
        if (int rc = launch_vq_argmax(c.t1, c.big, h->c2, tokens, c.M, kHid, kCenters, c.stream, c.status, kCentersPad, refine)) return rc;
    } else {
        if (int rc = linear(c, c.t1, kHid, h->centers, nullptr, c.big, kCenters, EPI_NONE, nullptr, nullptr, kCenters)) return rc;
        if (int rc = launch_vq_argmax(c.t1, c.big, h->c2, tokens, c.M, kHid, kCenters, c.stream, c.status, 0, refine)) return rc;
    }
    c.h->prof.end(c.stream);
    return 0;
}

}  // namespace

extern "C" {

int at_hubert_encode(at_hubert_t* h, const float* wav, const float* mask, int B, int N, int n_layers, int16_t* tokens, int* T_out,
                     float* hidden_out, void* workspace, size_t workspace_bytes, at_stream_t stream_) {
    return at_hubert_encode_checked(h, wav, mask, B, N, n_layers, tokens, T_out, hidden_out, workspace, workspace_bytes, stream_, nullptr);
}

int at_hubert_encode_checked(at_hubert_t* h, const float* wav, const float* mask, int B, int N, int n_layers, int16_t* tokens, int* T_out,
                             float* hidden_out, void* workspace, size_t workspace_bytes, at_stream_t stream_, int32_t* status_dev) {
    AT_REQUIRE(h && h->finalized, "model not finalized");
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    AT_REQUIRE(wav && workspace, "null pointer");
    AT_REQUIRE(n_layers >= 0 && n_layers <= (int)h->layers.size(), "n_layers exceeds the loaded layers");
    AT_REQUIRE(tokens == nullptr || h->centers != nullptr, "tokens requested but no k-means centres loaded");
    const Plan p = make_plan(B, N);
    AT_REQUIRE(B >= 1 && p.L[7] >= 1, "clip too short (needs at least 400 samples)");
    AT_REQUIRE(workspace_bytes >= p.total_floats * sizeof(float), "workspace too small");
    hipStream_t stream = (hipStream_t)stream_;
    if (T_out) *T_out = p.L[7];
    if (status_dev) AT_CHECK_HIP(hipMemsetAsync(status_dev, 0, sizeof(int32_t), stream));
    AT_REQUIRE(kRangeLayer0 + n_layers <= kRangeRows, "more transformer layers than range-table rows");
    if (int rc = h->range.reset(stream)) return rc;

    const Call c = make_call(h, p, B, N, n_layers, workspace, stream, status_dev);

    if (int rc = feature_extractor(c, wav)) return rc;
    if (int rc = projection_posconv(c, mask)) return rc;
    for (int li = 0; li < n_layers; ++li)
        if (int rc = transformer_layer(c, li)) return rc;
    if (status_dev)   // every site's range verdict of this call -> the caller's status word
        if (int rc = launch_range_combine(h->range.dev, (kRangeLayer0 + n_layers) * (int)H_NSITES, c.status, stream)) return rc;
    if (hidden_out) AT_CHECK_HIP(hipMemcpyAsync(hidden_out, c.x, (size_t)c.M * kHid * sizeof(float), hipMemcpyDeviceToDevice, stream));
    if (tokens)
        if (int rc = quantise(c, tokens)) return rc;
    return 0;
}

// Test tap: the conv features alone. The same feature_extractor() the encode runs, on the handle's current arithmetic, over the same plan and
// workspace slices (make_call); feats() copied out. status_dev: the front end's range sites (row 0 of the table) only.
int at_hubert_features(at_hubert_t* h, const float* wav, int B, int N, float* feats_out, void* workspace, size_t workspace_bytes, at_stream_t stream_,
                       int32_t* status_dev) {
    AT_REQUIRE(h && h->finalized, "model not finalized");
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    AT_REQUIRE(wav && feats_out && workspace, "null pointer");
    const Plan p = make_plan(B, N);
    AT_REQUIRE(B >= 1 && p.L[7] >= 1, "clip too short (needs at least 400 samples)");
    AT_REQUIRE(workspace_bytes >= p.total_floats * sizeof(float), "workspace too small");
    hipStream_t stream = (hipStream_t)stream_;
    if (status_dev) AT_CHECK_HIP(hipMemsetAsync(status_dev, 0, sizeof(int32_t), stream));
    if (int rc = h->range.reset(stream)) return rc;
    const Call c = make_call(h, p, B, N, 0, workspace, stream, status_dev);
    if (int rc = feature_extractor(c, wav)) return rc;
    if (status_dev)
        if (int rc = launch_range_combine(h->range.dev, kRangeLayer0 * (int)H_NSITES, c.status, stream)) return rc;
    AT_CHECK_HIP(hipMemcpyAsync(feats_out, c.feats(), (size_t)c.M * kCd * sizeof(float), hipMemcpyDeviceToDevice, stream));
    return 0;
}

int at_hubert_range_report(at_hubert_t* h, float* max_scaled, int cap) { return sem_range_report(h, "at_hubert_range_report", max_scaled, cap); }
// flags[0] = conv feature encoder + positional conv, flags[1 + l] = transformer layer l: 1 + layers entries
int at_hubert_layer_status(at_hubert_t* h, int32_t* flags, int cap) { return sem_layer_status(h, "at_hubert_layer_status", flags, cap); }
// The activation scales of the two LayerNorm-fed split sites of every transformer layer: scales[2 l] = the q/k/v projection's input, scales[2 l + 1] = the
// first FFN GEMM's input (16 unless a LayerNorm's gains force the provable scale below that). Returns the number of floats written. Host-only.
int at_hubert_site_scales(const at_hubert_t* h, float* scales, int cap) {
    AT_REQUIRE(h && h->finalized && scales, "at_hubert_site_scales: bad arguments");
    const int n = 2 * (int)h->layers.size();
    AT_REQUIRE(cap >= n, "at_hubert_site_scales: buffer too small");
    for (size_t l = 0; l < h->layers.size(); ++l) { scales[2 * l] = h->layers[l].xs_qkv; scales[2 * l + 1] = h->layers[l].xs_ffn; }
    return n;
}
int at_hubert_range_sites(char* names, size_t cap) { return range_sites(kHSiteNames, (int)H_NSITES, names, cap); }

int at_hubert_profile(at_hubert_t* h, int enable) { return profile_enable(h, enable); }
int at_hubert_profile_read(at_hubert_t* h, char* names, size_t names_cap, float* total_ms, int* launches, int max_groups) {
    return profile_read(h, names, names_cap, total_ms, launches, max_groups);
}

}  // extern "C"
