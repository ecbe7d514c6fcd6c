// What the handles of the two semantic tokenizers (at_hubert in hubert.hip, at_w2vbert in w2vbert.hip) have in common, stated once: tensor staging, the
// device arena and its packed export / import replay (packed_model.h), the lazy weight splits per scheme, the range table, the common options, the
// reports, the split-GEMM helper that owns the f16x2 scale rule (split_gemm_args) and the finalize helpers. A model file keeps what is its own: weight
// pointers, LayerW, Plan, the site names, the model part of finalize, the list of weights it splits and the encode stages. stage_tensor also serves the acoustic handle (encodec_handle.h); HostTensor and device_exists come from model_handle.h.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "at_common.h"
#include "gemm_bf16x3.h"
#include "model_handle.h"   // HostTensor, device_exists
#include "packed_model.h"

namespace at {

// at_*_set_tensor of every handle: one host tensor copied into h->staged until finalize()
template <class H>
int stage_tensor(H* h, const char* name, const float* host_data, const int64_t* shape, int ndim) {
    AT_REQUIRE(h && name && host_data && shape && ndim >= 1 && ndim <= 4, "bad arguments");
    AT_REQUIRE(!h->finalized, "model already finalized");
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    t.data.assign(host_data, host_data + n);
    h->staged[name] = std::move(t);
    return 0;
}

// at_*_profile / at_*_profile_read of every handle (Profiler, at_common.h)
template <class H>
int profile_enable(H* h, int enable) {
    AT_REQUIRE(h != nullptr, "null handle");
    h->prof.restart(enable != 0);
    return 0;
}
template <class H>
int profile_read(H* h, char* names, size_t names_cap, float* total_ms, int* launches, int max_groups) {
    AT_REQUIRE(h && names && total_ms && launches, "null pointer");
    return h->prof.read_groups(names, names_cap, total_ms, launches, max_groups);
}

// arithmetic of the linear layers: the fp32 MFMA, or operand splits on the 16-bit matrix cores (gemm_bf16x3.h)
enum { ARITH_F32 = 0, ARITH_BF16X3 = 1, ARITH_F16X2 = 2 };

// Device table of {flag, census} per (row, site) where activations become fp16 pieces (gemm_bf16x3.h, launch_range_combine) and, behind it, its per-encode
// initial image: row 0 = {flag 0, census 0} per site; every further row {flag 0, LINK to row 0's census word of that site} (split_scheme.h, range_publish):
// one flag word per (row, site), one census word per site. Run-time state, not part of the packed model.
struct RangeTable {
    int rows, sites, layer0;   // layer l of the model is row layer0 + l; the rows below layer0 belong to the front end
    int* dev = nullptr;
    int ints() const { return rows * 2 * sites; }
    int* layer_row(int l) const { return dev + (layer0 + l) * 2 * sites; }
    int alloc();                        // the table and its initial image (nothing when it exists)
    int reset(hipStream_t stream);      // at the start of every encode: flags 0, census 0 / links
    int read(std::vector<int>& host);   // the last encode's table; synchronises the device
    void free();
};

struct SemanticHandle {
    const uint32_t model;       // PACKED_MODEL_*
    int device;
    bool finalized = false;
    std::map<std::string, HostTensor> staged;
    DeviceArena arena;          // every device allocation of finalize(), in order (packed_model.h: export / import of the finalized model)
    PackedHeader imp{};         // import_packed: the exporter's record (layer count, flags) while finalize is replayed
    std::vector<int> split_seq; // the schemes whose weight pieces exist, in the order they were split (= their order in the arena)
    bool split_done[2] = {false, false};
    std::map<const float*, float> wmax;   // max |w| of every uploaded tensor (the fp16 scheme's weight scales)
    RangeTable range;           // zeroed per encode; the range reports read it
    int arith = ARITH_F16X2;    // linear layers (HuBERT: + conv chain): ARITH_* ($AUDIOTOKEN_SEMANTIC_ARITH = f32 | bf16x3 | f16x2; option "arith")
    std::vector<int> layer_arith;   // per layer: -1 = the handle's arithmetic, else ARITH_BF16X3 / ARITH_F16X2 for that layer only (option "layer_arith:<i>")
    int attn_w8 = -1;           // option "attn_w8": 1 / 0 = the 8-wave 64-key LDS-DMA attention (attention_f16x2_w8.hip) / its round-3 twin; -1 = $AUDIOTOKEN_ATTN_W8, default 1
    bool vq_refine = true;      // option "vq_refine" (round 5): near-tie codes re-evaluated exactly (vq_argmax_kernel); 0 = the expanded fp32 form alone, as rounds 1-4
    struct BoolOption { const char* name; bool* value; };
    std::vector<BoolOption> bool_opts;   // the model's own plain boolean options (its constructor lists them)
    Profiler prof;

    SemanticHandle(uint32_t model_, int device_, RangeTable range_) : model(model_), device(device_), range(range_) {}
    virtual ~SemanticHandle() = default;
    // The three places where the shared code calls the model's. finalize_model(): staged host tensors -> device, up to and including the code book. With the
    // arena in import mode the same code REPLAYS the allocation order over the packed blob: no host tensor is read, nothing is uploaded or split — only the
    // pointers and scales are rebuilt
    virtual int finalize_model() = 0;
    virtual int split_model(int scheme) = 0;   // every weight the model runs on the split kernels as the 16-bit pieces of `scheme` (split_one)
    virtual void forget_model() = 0;           // after a failed import: no layers, every weight pointer null
    virtual int num_layers() const = 0;
    virtual bool has_codes() const = 0;        // a code book / k-means centres are loaded (bit 0 of the packed flags)

    // layer li's arithmetic: the handle's, unless the range fallback has pinned that layer to another split scheme (option "layer_arith:<i>")
    int arith_of(int li) const { return (arith != ARITH_F32 && li < (int)layer_arith.size() && layer_arith[li] > 0) ? layer_arith[li] : arith; }
};

// ---- staging, for the model's finalize_model() ---------------------------------------------------------------------------------------------
const HostTensor* find(const SemanticHandle* h, const std::string& name);
// upload one packed tensor into its own device allocation (the conformer is ~1.8 GB: no second full host copy) and record its max |w|
const float* upload(SemanticHandle* h, const std::vector<float>& v);
// import_packed: the tensor's bytes are already in the blob — take the next slice and the recorded max |w|
const float* reserve(SemanticHandle* h, size_t n_floats);
// the staged tensor `name` of exactly `shape` uploaded (import: reserved); on failure nullptr, the error set and ok = false
const float* take(SemanticHandle* h, const std::string& name, std::vector<int64_t> shape, bool& ok);

// a tensor that finalize repacks on the host. `fill(v)` writes the repacked floats into v (n zeros) and returns 0, or sets the error and returns non-zero
// (the staged tensor is missing); import: the next n floats of the blob, `fill` is not called. *dst = nullptr when the device allocation failed: the caller
// names that error.
template <class Fill>
int take_repacked(SemanticHandle* h, size_t n, const float** dst, Fill&& fill) {
    if (h->arena.importing) { *dst = reserve(h, n); return 0; }
    std::vector<float> v(n, 0.f);
    if (int rc = fill(v)) return rc;
    *dst = upload(h, v);
    return 0;
}
// the three [hid][hid] projections prefix + names[j] + ".weight" / ".bias" as ONE [3 hid][hid] weight and [3 hid] bias (one GEMM, one pass over the
// LayerNorm output): two allocations, weight then bias. *w / *b = nullptr when a device allocation failed.
int take_qkv(SemanticHandle* h, const std::string& prefix, const char* const names[3], int hid, const float** w, const float** b);
// |row|^2 of the n rows of a code book [n][d], summed in fp32 in index order (the e2 / c2 term of the quantisers' expanded distance)
std::vector<float> code_norms(const std::vector<float>& codes, int n, int d);
// the provable f16x2 scale of the split site fed by LayerNorm(D; gamma, beta), from the recorded max |gamma|, max |beta| (xb_ln_site_scale, gemm_bf16x3.h)
float ln_site_scale(const SemanticHandle* h, const float* gamma, const float* beta, int D);

// ---- weight splits, for the model's split_model() ------------------------------------------------------------------------------------------
// the fp16 scheme's power-of-two scale of the uploaded tensor `src`, from its recorded max |w|
int weight_scale(SemanticHandle* h, const float* src, float* scale_out);
// W [n][k] as pieces of `scheme`, rows padded to n_pad (0: n) with zeros: allocate, set dst->s (f16x2 only; bf16x3 keeps 1), split unless importing (the
// pieces are in the blob)
int split_one(SemanticHandle* h, int scheme, const float* src, int n, int k, SplitW* dst, int n_pad = 0, int win_cblocks = 0, int win_stride = 1);
int split_weights(SemanticHandle* h, int scheme);   // split_model() once per scheme, recorded in split_seq

// ---- split GEMMs, for the model's encode stages ---------------------------------------------------------------------------------------------
inline int scheme_of(int arith) { return arith == ARITH_F16X2 ? XB_SCHEME_F16X2 : XB_SCHEME_BF16X3; }
// The split arithmetic of one part of a model (a layer, or the front end / quantiser): its scheme and its row of the range table (nullptr: no range sites)
struct SplitCtx {
    int scheme;
    int* row;
    int* site(int k) const { return row ? row + 2 * k : nullptr; }
    // the scale activations are multiplied by before they are split: `f16` on the fp16 scheme, 1 on bf16x3 (full fp32 exponent range)
    float act(float f16 = XB_F16_ACT_SCALE) const { return scheme == XB_SCHEME_F16X2 ? f16 : 1.0f; }
    SplitOut out(piece_t* pieces, long long rows_pad, float f16_scale, int* status) const { return SplitOut{pieces, rows_pad, scheme, act(f16_scale), status}; }
};
// A plain linear layer acc = A . W^T on the split GEMM (gemm_bf16x3.hip): A as pieces that were split with a_scale, W with its scale; values the epilogue
// splits again are multiplied by out_scale and their range verdict goes to `status`. THE place of the f16x2 scale rule: acc_scale = 1 / (s_a s_w),
// split_scale = s_out. Every scale is 1 on bf16x3 (SplitCtx::act, SplitW::s), where 1 / (1 * 1) is exact: no scheme branch. The caller adds the bias and
// where the output goes (C / R / S) and, for a windowed conv, the window description.
Bf16x3Args split_gemm_args(int scheme, const piece_t* A, float a_scale, const SplitW& w, long long M, int N, int K, long long Mpad, int epi, int* status,
                           float out_scale);
// The fused q / k / v projection of an f16x2 layer (XB_EPI_QKV): q as fp32 rows of C [M][3 hid], k and v as row-major fp16 pieces in kvs
int qkv_split_gemm(const SplitCtx& c, int kv_site, const piece_t* A, float a_scale, const SplitW& w, const float* bias, int hid, long long M, long long Mpad,
                   float* C, piece_t* kvs, hipStream_t stream);
// The quantisers' score GEMM dots [M][n_codes] = LN(x) . E^T against a code book split into n_codes rows of pieces
int score_split_gemm(const SplitCtx& c, const piece_t* A, const SplitW& codes, int n_codes, int K, long long M, long long Mpad, float* dots, hipStream_t stream);

// ---- bodies of the exported at_<model>_* functions; `fn` is the exported function's name where an error text carries it -------------------------------
int sem_finalize(SemanticHandle* h);
int64_t sem_packed_bytes(SemanticHandle* h, const char* fn);
int64_t sem_packed_meta(SemanticHandle* h, const char* fn, void* host_dst, int64_t cap);
int sem_export_packed(SemanticHandle* h, const char* fn, void* device_dst, int64_t bytes, void* stream);
int sem_import_packed(SemanticHandle* h, const char* fn, const void* host_meta, int64_t meta_bytes, const void* device_src, int64_t bytes, void* stream);
void sem_destroy(SemanticHandle* h);
int sem_set_option(SemanticHandle* h, const char* fn, const char* name, int value);
int sem_get_option(const SemanticHandle* h, const char* name);
// The measured fp16 headroom of the LAST encode: per site the largest |x * scale| a split writer saw over all rows (0: the site did not run on the fp16
// scheme); the scheme overflows at 65504. Synchronises the device.
int sem_range_report(SemanticHandle* h, const char* fn, float* max_scaled, int cap);
// Per row of the range table that the model uses (range.layer0 + layers), the OR of its sites' status flags in the LAST encode (bit 1 = an activation left
// the fp16 range; the FIRST flagged entry is the cause, later ones inherit its infinities). Returns the number of entries written. Synchronises the device.
int sem_layer_status(SemanticHandle* h, const char* fn, int32_t* flags, int cap);
// n site names, newline-terminated each, into `out`; -(needed size) when cap is too small
int range_sites(const char* const* site_names, int n, char* out, size_t cap);

}  // namespace at
