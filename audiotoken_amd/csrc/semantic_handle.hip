// The shared half of the semantic tokenizers' handles (semantic_handle.h). Host code only.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "semantic_handle.h"

namespace at {

// ---- range table ----------------------------------------------------------------------------------------------------------------------------
int RangeTable::alloc() {
    if (dev) return 0;
    AT_CHECK_HIP(hipMalloc((void**)&dev, 2 * ints() * sizeof(int)));
    std::vector<int> init(ints(), 0);
    for (int r = 1; r < rows; ++r)
        for (int k = 0; k < sites; ++k) init[(r * sites + k) * 2 + 1] = -(r * sites * 2);
    AT_CHECK_HIP(hipMemcpy(dev + ints(), init.data(), ints() * sizeof(int), hipMemcpyHostToDevice));
    AT_CHECK_HIP(hipMemcpy(dev, init.data(), ints() * sizeof(int), hipMemcpyHostToDevice));
    return 0;
}
int RangeTable::reset(hipStream_t stream) {
    AT_CHECK_HIP(hipMemcpyAsync(dev, dev + ints(), ints() * sizeof(int), hipMemcpyDeviceToDevice, stream));
    return 0;
}
int RangeTable::read(std::vector<int>& host) {
    host.resize(ints());
    AT_CHECK_HIP(hipDeviceSynchronize());
    AT_CHECK_HIP(hipMemcpy(host.data(), dev, ints() * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}
void RangeTable::free() {
    if (dev) (void)hipFree(dev);
    dev = nullptr;
}

// ---- staging ----------------------------------------------------------------------------------------------------------------------------------
const HostTensor* find(const SemanticHandle* h, const std::string& name) {
    auto it = h->staged.find(name);
    return it == h->staged.end() ? nullptr : &it->second;
}
const float* upload(SemanticHandle* h, const std::vector<float>& v) {
    const size_t n = (v.size() + 3) / 4 * 4;
    float* d = static_cast<float*>(h->arena.alloc(n * sizeof(float)));
    if (!d) return nullptr;
    if (hipMemcpy(d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    float mx = 0.f;
    for (float x : v) mx = std::fmax(mx, std::fabs(x));
    h->arena.blocks.back().wmax = mx;
    h->wmax[d] = mx;
    return d;
}
const float* reserve(SemanticHandle* h, size_t n_floats) {
    float* d = static_cast<float*>(h->arena.alloc((n_floats + 3) / 4 * 4 * sizeof(float)));
    if (d) h->wmax[d] = h->arena.blocks.back().wmax;
    return d;
}
const float* take(SemanticHandle* h, const std::string& name, std::vector<int64_t> shape, bool& ok) {
    if (h->arena.importing) {
        size_t n = 1;
        for (int64_t d : shape) n *= (size_t)d;
        const float* d = reserve(h, n);
        if (!d) ok = false;
        return d;
    }
    const HostTensor* t = find(h, name);
    if (!t) { set_error("missing tensor " + name); ok = false; return nullptr; }
    if (t->shape != shape) { set_error("bad shape for " + name); ok = false; return nullptr; }
    const float* d = upload(h, t->data);
    if (!d) { set_error("device allocation/copy failed for " + name); ok = false; }
    return d;
}

int take_qkv(SemanticHandle* h, const std::string& prefix, const char* const names[3], int hid, const float** w, const float** b) {
    const size_t hh = (size_t)hid * hid;
    if (h->arena.importing) {
        *w = reserve(h, 3 * hh);
        *b = reserve(h, (size_t)3 * hid);
        return 0;
    }
    std::vector<float> wv(3 * hh), bv((size_t)3 * hid);
    for (int j = 0; j < 3; ++j) {
        const HostTensor* wt = find(h, prefix + names[j] + ".weight");
        const HostTensor* bt = find(h, prefix + names[j] + ".bias");
        AT_REQUIRE(wt && bt && wt->shape == (std::vector<int64_t>{hid, hid}) && bt->shape == (std::vector<int64_t>{hid}),
                   "attention projection tensors missing or mis-shaped");
        std::memcpy(&wv[j * hh], wt->data.data(), hh * sizeof(float));
        std::memcpy(&bv[(size_t)j * hid], bt->data.data(), hid * sizeof(float));
    }
    *w = upload(h, wv);
    *b = upload(h, bv);
    return 0;
}
std::vector<float> code_norms(const std::vector<float>& codes, int n, int d) {
    std::vector<float> e2(n);
    for (int i = 0; i < n; ++i) {
        float acc = 0.f;
        for (int k = 0; k < d; ++k) { const float v = codes[(size_t)i * d + k]; acc += v * v; }
        e2[i] = acc;
    }
    return e2;
}
float ln_site_scale(const SemanticHandle* h, const float* gamma, const float* beta, int D) {
    auto mx = [&](const float* d) { auto it = h->wmax.find(d); return it == h->wmax.end() ? 0.f : it->second; };
    return xb_ln_site_scale(mx(gamma), mx(beta), D);
}

// ---- weight splits ----------------------------------------------------------------------------------------------------------------------------
int weight_scale(SemanticHandle* h, const float* src, float* scale_out) {
    auto it = h->wmax.find(src);
    AT_REQUIRE(it != h->wmax.end(), "weight maximum not recorded");
    *scale_out = xb_weight_scale(it->second);
    return 0;
}
int split_one(SemanticHandle* h, int scheme, const float* src, int n, int k, SplitW* dst, int n_pad, int win_cblocks, int win_stride) {
    if (!n_pad) n_pad = n;
    piece_t* d = static_cast<piece_t*>(h->arena.alloc((size_t)xb_pieces(scheme) * n_pad * k * sizeof(piece_t)));
    if (!d) return -1;
    float s = 1.0f;
    if (scheme == XB_SCHEME_F16X2)
        if (int rc = weight_scale(h, src, &s)) return rc;
    if (!h->arena.importing)
        if (int rc = launch_split_blocked(src, k, n, n_pad, k, d, nullptr, scheme, s, nullptr, win_cblocks, win_stride)) return rc;
    *dst = SplitW{d, s};
    return 0;
}
int split_weights(SemanticHandle* h, int scheme) {
    if (h->split_done[scheme]) return 0;
    if (int rc = h->split_model(scheme)) return rc;
    AT_CHECK_HIP(hipDeviceSynchronize());
    h->split_done[scheme] = true;
    h->split_seq.push_back(scheme);
    return 0;
}

// ---- split GEMMs --------------------------------------------------------------------------------------------------------------------------------
Bf16x3Args split_gemm_args(int scheme, const piece_t* A, float a_scale, const SplitW& w, long long M, int N, int K, long long Mpad, int epi, int* status,
                           float out_scale) {
    Bf16x3Args a;
    a.A = A; a.W = w.p; a.M = (int)M; a.N = N; a.K = K; a.Mpad = (int)Mpad; a.epi = epi;
    a.scheme = scheme; a.status = status;
    a.acc_scale = 1.0f / (a_scale * w.s); a.split_scale = out_scale;
    return a;
}
int qkv_split_gemm(const SplitCtx& c, int kv_site, const piece_t* A, float a_scale, const SplitW& w, const float* bias, int hid, long long M, long long Mpad,
                   float* C, piece_t* kvs, hipStream_t stream) {
    // the k / v pieces always use XB_F16_ACT_SCALE, whatever the layer's site scales: the attention kernels divide by that fixed 16
    Bf16x3Args a = split_gemm_args(c.scheme, A, a_scale, w, M, 3 * hid, hid, Mpad, XB_EPI_QKV, c.site(kv_site), XB_F16_ACT_SCALE);
    a.bias = bias; a.C = C; a.ldc = 3 * hid; a.S = kvs; a.Spad = (int)Mpad; a.qkv_hid = hid;
    return launch_gemm_bf16x3(a, stream);
}
int score_split_gemm(const SplitCtx& c, const piece_t* A, const SplitW& codes, int n_codes, int K, long long M, long long Mpad, float* dots, hipStream_t stream) {
    // the VQ / k-means operand has no range site: a non-affine LayerNorm row is bounded by sqrt(D) <= 32, and x 16 cannot leave the fp16 range
    Bf16x3Args a = split_gemm_args(c.scheme, A, c.act(), codes, M, n_codes, K, Mpad, XB_EPI_LINEAR, nullptr, c.act());
    a.C = dots; a.ldc = n_codes; a.ldr = n_codes;
    return launch_gemm_bf16x3(a, stream);
}

// ---- finalize, and the finalized model as one device blob (packed_model.h) ---------------------------------------------------------------------
// The arena's allocations are the packed format: the model's tensors, then the pieces of every split scheme in split_seq order. Import replays exactly that.
static int finalize_impl(SemanticHandle* h) {
    if (int rc = h->finalize_model()) return rc;
    h->staged.clear();
    if (h->arena.importing) {
        h->arith = h->imp.arith;
        // the exporter's splits in ITS order (flags bits 1-2 = count, bits 3.. = one bit per split: 1 = bf16x3). Normally one: the default scheme at
        // finalize; two when the per-batch range fallback had run there (the other scheme is split lazily, and the handle's current arithmetic may be either)
        const int n = (h->imp.flags >> 1) & 3;
        for (int i = 0; i < n; ++i)
            if (int rc = split_weights(h, ((h->imp.flags >> (3 + i)) & 1) ? XB_SCHEME_BF16X3 : XB_SCHEME_F16X2)) return rc;
    } else {
        h->arith = ARITH_F16X2;
        if (const char* e = std::getenv("AUDIOTOKEN_SEMANTIC_ARITH")) {
            const std::string v(e);
            AT_REQUIRE(v == "f32" || v == "bf16x3" || v == "f16x2", "AUDIOTOKEN_SEMANTIC_ARITH must be f32, bf16x3 or f16x2");
            h->arith = v == "f32" ? ARITH_F32 : v == "bf16x3" ? ARITH_BF16X3 : ARITH_F16X2;
        }
        if (h->arith != ARITH_F32)
            if (int rc = split_weights(h, scheme_of(h->arith))) return rc;
    }
    if (!host_only_test())
        if (int rc = h->range.alloc()) return rc;
    h->finalized = true;
    return 0;
}
int sem_finalize(SemanticHandle* h) {
    AT_REQUIRE(h && !h->finalized, "bad handle");
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    return finalize_impl(h);
}

static int packed_flags(const SemanticHandle* h) {
    int f = (h->has_codes() ? 1 : 0) | ((int)h->split_seq.size() << 1);
    for (size_t i = 0; i < h->split_seq.size(); ++i) f |= (h->split_seq[i] == XB_SCHEME_BF16X3 ? 1 : 0) << (3 + i);
    return f;
}
int64_t sem_packed_bytes(SemanticHandle* h, const char* fn) {
    if (!h || !h->finalized) { set_error(std::string(fn) + ": model not finalized"); return -1; }
    return (int64_t)h->arena.packed_bytes();
}
int64_t sem_packed_meta(SemanticHandle* h, const char* fn, void* host_dst, int64_t cap) {
    if (!h || !h->finalized) { set_error(std::string(fn) + ": model not finalized"); return -1; }
    return packed_write_meta(h->arena, h->model, h->num_layers(), packed_flags(h), h->arith, host_dst, cap);
}
int sem_export_packed(SemanticHandle* h, const char* fn, void* device_dst, int64_t bytes, void* stream) {
    AT_REQUIRE(h && h->finalized, std::string(fn) + ": model not finalized");
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    return packed_export(h->arena, device_dst, bytes, (hipStream_t)stream);
}
int sem_import_packed(SemanticHandle* h, const char* fn, const void* host_meta, int64_t meta_bytes, const void* device_src, int64_t bytes, void* stream) {
    AT_REQUIRE(h && !h->finalized && h->staged.empty(), std::string(fn) + " needs a fresh handle (no set_tensor, no finalize)");
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    if (int rc = packed_begin_import(h->arena, h->model, host_meta, meta_bytes, device_src, bytes, (hipStream_t)stream, &h->imp)) return rc;
    int rc = finalize_impl(h);
    if (!rc) rc = packed_end_import(h->arena);
    if (rc) {
        // A failed import leaves an EMPTY handle that can only be destroyed (or imported into again): it owns no device memory, reports not finalized, and has
        // no layers, no recorded splits, no recorded weight maxima and no model pointer into the freed blob (the union of what the two models used to clear).
        h->finalized = false;
        h->arena.importing = false;
        h->arena.free_all();
        h->range.free();
        h->split_seq.clear();
        h->split_done[0] = h->split_done[1] = false;
        h->wmax.clear();
        h->forget_model();
    }
    return rc;
}
void sem_destroy(SemanticHandle* h) {
    if (!h) return;
    DeviceGuard guard(h->device);   // restores the caller's current device (destroy runs from garbage collection in Python)
    h->arena.free_all();
    h->range.free();
    delete h;
}

// ---- options ----------------------------------------------------------------------------------------------------------------------------------
int sem_set_option(SemanticHandle* h, const char* fn, const char* name, int value) {
    AT_REQUIRE(h && h->finalized && name, "bad handle");
    const std::string n(name);
    if (n == "arith") {
        AT_REQUIRE(value == ARITH_F32 || value == ARITH_BF16X3 || value == ARITH_F16X2, "arith: 0 = f32 MFMA, 1 = bf16x3, 2 = f16x2");
        DeviceGuard guard(h->device);
        AT_REQUIRE(guard.ok, "cannot select the handle's device");
        if (value != ARITH_F32)
            if (int rc = split_weights(h, scheme_of(value))) return rc;
        h->arith = value;
        return 0;
    }
    if (n.rfind("layer_arith:", 0) == 0) {   // "layer_arith:<i>": -1 = follow "arith", 1 = bf16x3, 2 = f16x2 for layer i only
        const int li = std::atoi(n.c_str() + 12);
        AT_REQUIRE(li >= 0 && li < h->num_layers(), "layer_arith: no such layer");
        AT_REQUIRE(value == -1 || value == ARITH_BF16X3 || value == ARITH_F16X2, "layer_arith:<i>: -1 = the handle's arithmetic, 1 = bf16x3, 2 = f16x2");
        if (value > 0) {
            DeviceGuard guard(h->device);
            AT_REQUIRE(guard.ok, "cannot select the handle's device");
            if (int rc = split_weights(h, scheme_of(value))) return rc;
        }
        if ((int)h->layer_arith.size() < h->num_layers()) h->layer_arith.resize(h->num_layers(), -1);
        h->layer_arith[li] = value;
        return 0;
    }
    if (n == "attn_w8") { h->attn_w8 = value < 0 ? -1 : (value != 0); return 0; }
    if (n == "vq_refine") { h->vq_refine = value != 0; return 0; }
    for (const auto& o : h->bool_opts)
        if (n == o.name) { *o.value = value != 0; return 0; }
    set_error(std::string(fn) + ": unknown option " + n);
    return -1;
}
int sem_get_option(const SemanticHandle* h, const char* name) {
    if (!h || !name) return -1;
    const std::string n(name);
    if (n == "arith") return h->arith;
    if (n.rfind("layer_arith:", 0) == 0) {
        const int li = std::atoi(name + 12);
        return (li >= 0 && li < (int)h->layer_arith.size()) ? h->layer_arith[li] : -1;
    }
    if (n == "attn_w8") return h->attn_w8;
    if (n == "vq_refine") return h->vq_refine ? 1 : 0;
    for (const auto& o : h->bool_opts)
        if (n == o.name) return *o.value ? 1 : 0;
    return -1;
}

// ---- range reports ------------------------------------------------------------------------------------------------------------------------------
int sem_range_report(SemanticHandle* h, const char* fn, float* max_scaled, int cap) {
    AT_REQUIRE(h && h->finalized && h->range.dev && max_scaled && cap >= h->range.sites, std::string(fn) + ": bad arguments");
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    std::vector<int> host;
    if (int rc = h->range.read(host)) return rc;
    // row 0 holds the one census word of the site; the other rows' second words are links to it (split_scheme.h)
    for (int k = 0; k < h->range.sites; ++k) std::memcpy(&max_scaled[k], &host[k * 2 + 1], sizeof(float));
    return h->range.sites;
}
int sem_layer_status(SemanticHandle* h, const char* fn, int32_t* flags, int cap) {
    AT_REQUIRE(h && h->finalized && h->range.dev && flags && cap >= 1, std::string(fn) + ": bad arguments");
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    std::vector<int> host;
    if (int rc = h->range.read(host)) return rc;
    const int n = std::min<int>({cap, h->range.layer0 + h->num_layers(), h->range.rows});
    for (int r = 0; r < n; ++r) {
        int v = 0;
        for (int k = 0; k < h->range.sites; ++k) v |= host[(r * h->range.sites + k) * 2];
        flags[r] = v;
    }
    return n;
}
int range_sites(const char* const* site_names, int n, char* out, size_t cap) {
    std::string s;
    for (int k = 0; k < n; ++k) { s += site_names[k]; s += "\n"; }
    if (!out || cap < s.size() + 1) return -(int)(s.size() + 1);
    std::memcpy(out, s.c_str(), s.size() + 1);
    return n;
}

}  // namespace at
