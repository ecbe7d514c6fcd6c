// The semantic decoder's second stage: bark's non-causal "fine" transformer fills code books 3 to 8 of a [2][T] coarse row, window by window.
// The model: 8 embedding tables summed up to the code book being predicted, learned positions, pre-LN blocks (LayerNorm with gain and bias, linears with or
// without bias, E / 64 heads of 64, attention over the whole window without a mask, erf-GELU MLP), a final LayerNorm and 7 heads.
// The matrix products, the attention and the LayerNorm are the library's own fp32 launchers (launch_gemm, launch_relpos_attention with its arithmetic set to
// fp32, launch_layernorm). New here, all fp32:
//   fine_init_kernel     the rows' work arrays [L][8]: the coarse codes, 1024 everywhere else
//   fine_embed_kernel    x[t] = sum_{i <= c} wtes[i][cell[t][i]] + wpe[t], read straight from the work arrays at each row's window (no batch copy of the ids)
//   fine_gather_kernel   the rows the head needs (positions >= rel of every window of the pass), where a window has rel > 0
//   fine_sample_kernel   one wave per position over its 1024 logits: the argmax or the inverse-CDF draw, written straight into the work array
//   fine_finish_kernel   the first T positions as [8][T]
// A call enqueues every window of every row without looking at the device: the host knows the schedule from the lengths. No float is added atomically.
#include <cmath>
#include <cstring>

#include "../../include/audiotoken_hip.h"
#include "fine.h"
#include "w2vbert_kernels.h"

using namespace at;

namespace {

constexpr int SAMPLE_WAVES = 4;

// ---- caller-owned state --------------------------------------------------------------------------------------------------------------------
struct FineState {
    int* work;       // [B][Lmax][8]
    float *ones, *x, *xn, *qkv, *h, *logits;
    int Lmax;
    size_t bytes;
};

size_t round256(size_t n) { return (n + 255) / 256 * 256; }

FineState carve_state(void* base, int B, int max_T, int W, int E) {
    FineState s{};
    char* p = static_cast<char*>(base);
    size_t off = 0;
    auto take = [&](size_t bytes) { char* r = p ? p + off : nullptr; off += round256(bytes); return r; };
    const size_t R = (size_t)B * W;
    s.Lmax = max_T > W ? max_T : W;
    s.work = (int*)take((size_t)B * s.Lmax * FINE_CODES * 4);
    s.ones = (float*)take(R * 4);
    s.x = (float*)take(R * E * 4);
    s.xn = (float*)take(R * E * 4);
    s.qkv = (float*)take(R * 3 * E * 4);
    s.h = (float*)take(R * 4 * E * 4);       // the MLP's hidden rows; before the head, the gathered rows
    s.logits = (float*)take(R * FINE_VOCAB * 4);
    s.bytes = off;
    return s;
}

// ---- the schedule of one pass, by value into the kernels ------------------------------------------------------------------------------------
struct FinePass {
    int n;                             // windows in the batch
    int row[FINE_MAX_B];               // the call's row each belongs to
    int start[FINE_MAX_B];             // first position of the window in the row's work array
    int rel[FINE_MAX_B];               // first buffer position that is predicted
    int head_off[FINE_MAX_B + 1];      // the window's predicted positions are head rows [head_off[j], head_off[j + 1])
};
struct RowLens { int T[FINE_MAX_B]; };
struct FineTables { const float* t[FINE_CODES]; };

__device__ __forceinline__ int slot_of(const FinePass& p, int r) {
    int j = 0;
    while (j + 1 < p.n && p.head_off[j + 1] <= r) ++j;
    return j;
}

// start of a call: thread i = (row, position). A coarse code outside [0, 1024) is clamped and reported in bit 0 of *status.
__global__ __launch_bounds__(256) void fine_init_kernel(RowLens lens, int B, int Lmax, int n_ones, const int* coarse, int t_stride, int* work, float* ones, int* status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * Lmax) return;
    if (i < (size_t)n_ones) ones[i] = 1.0f;
    const int b = (int)(i / Lmax), t = (int)(i % Lmax);
    int c0 = FINE_VOCAB, c1 = FINE_VOCAB;
    if (t < lens.T[b]) {
        c0 = coarse[((size_t)b * 2 + 0) * t_stride + t];
        c1 = coarse[((size_t)b * 2 + 1) * t_stride + t];
        if (c0 < 0 || c0 >= FINE_VOCAB || c1 < 0 || c1 >= FINE_VOCAB) {
            if (status) atomicOr(status, 1);
            c0 = min(max(c0, 0), FINE_VOCAB - 1);
            c1 = min(max(c1, 0), FINE_VOCAB - 1);
        }
    }
    int4* cell = reinterpret_cast<int4*>(work + i * FINE_CODES);
    cell[0] = make_int4(c0, c1, FINE_VOCAB, FINE_VOCAB);
    cell[1] = make_int4(FINE_VOCAB, FINE_VOCAB, FINE_VOCAB, FINE_VOCAB);
}

// Token i = (window i / W of the pass, buffer position i % W), E / 4 threads of 16 bytes each. Tables 0 to c in that order, the position last.
__global__ __launch_bounds__(256) void fine_embed_kernel(FinePass p, FineTables tab, const float* wpe, const int* work, int Lmax, int W, int E, int c, float* x) {
    const int i = blockIdx.x, tid = threadIdx.x;
    const int j = i / W, t = i % W;
    const int4* cell = reinterpret_cast<const int4*>(work + ((size_t)p.row[j] * Lmax + p.start[j] + t) * FINE_CODES);
    const int4 lo = cell[0], hi = cell[1];
    const int ids[FINE_CODES] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    float4 a = reinterpret_cast<const float4*>(tab.t[0] + (size_t)ids[0] * E)[tid];
#pragma unroll
    for (int ch = 1; ch < FINE_CODES; ++ch) {
        if (ch <= c) {   // uniform
            const float4 v = reinterpret_cast<const float4*>(tab.t[ch] + (size_t)ids[ch] * E)[tid];
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
    }
    const float4 q = reinterpret_cast<const float4*>(wpe + (size_t)t * E)[tid];
    reinterpret_cast<float4*>(x + (size_t)i * E)[tid] = make_float4(a.x + q.x, a.y + q.y, a.z + q.z, a.w + q.w);
}

// head row r = position rel + (r - head_off) of its window: a copy of that token's row
__global__ __launch_bounds__(256) void fine_gather_kernel(FinePass p, int W, int E, const float* x, float* dst) {
    const int r = blockIdx.x, tid = threadIdx.x;
    const int j = slot_of(p, r);
    const size_t tok = (size_t)j * W + p.rel[j] + (r - p.head_off[j]);
    reinterpret_cast<float4*>(dst + (size_t)r * E)[tid] = reinterpret_cast<const float4*>(x + tok * E)[tid];
}

struct FineSampleArgs {
    const float* logits;      // [head rows][1024]
    int total;                // head rows of the pass
    int W, Lmax, k, c, n_max;
    int greedy;
    float temperature;
    const float* uniforms;    // [B][n_max][6][W]
    int* work;
    float* logits_out;        // nullable [B][n_max][6][W][1024]
    int* ids_out;             // nullable [B][n_max][6][W]
};

// One wave per head row; lane l owns ids [16 l, 16 l + 16). The rule: zt = z / temperature, m = max zt, p = expf(zt - m); the running sum of
// id i is (the lanes before l, added by an inclusive shuffle scan of the lanes' totals) + (the lane's own ids up to i, added in id order); S is lane 63's
// inclusive total. The token is the lowest id whose running sum exceeds u * S, else the highest id with p > 0. greedy: the largest z, the lowest id among equals.
__global__ __launch_bounds__(64 * SAMPLE_WAVES) void fine_sample_kernel(FinePass p, FineSampleArgs a) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * SAMPLE_WAVES + (threadIdx.x >> 6);
    if (r >= a.total) return;   // uniform over the wave
    const int j = slot_of(p, r);
    const int t = p.rel[j] + (r - p.head_off[j]), b = p.row[j];
    const float4* zr = reinterpret_cast<const float4*>(a.logits + (size_t)r * FINE_VOCAB) + 4 * lane;
    float z[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v = zr[q];
        z[4 * q] = v.x; z[4 * q + 1] = v.y; z[4 * q + 2] = v.z; z[4 * q + 3] = v.w;
    }
    const size_t cell = (((size_t)b * a.n_max + a.k) * FINE_PASSES + (a.c - FINE_COARSE)) * a.W + t;
    if (a.logits_out) {
        float4* dst = reinterpret_cast<float4*>(a.logits_out + cell * FINE_VOCAB) + 4 * lane;
#pragma unroll
        for (int q = 0; q < 4; ++q) dst[q] = make_float4(z[4 * q], z[4 * q + 1], z[4 * q + 2], z[4 * q + 3]);
    }
    int tok;
    if (a.greedy) {
        float best = z[0];
        int at_ = 16 * lane;
#pragma unroll
        for (int i = 1; i < 16; ++i)
            if (z[i] > best) { best = z[i]; at_ = 16 * lane + i; }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(best, o);
            const int oi = __shfl_xor(at_, o);
            if (ov > best || (ov == best && oi < at_)) { best = ov; at_ = oi; }
        }
        tok = at_;
    } else {
        float m = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) { z[i] = z[i] / a.temperature; m = fmaxf(m, z[i]); }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        int top = -1;
        float run = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {   // z[i] becomes the lane's own running sum up to id i
            const float w = expf(z[i] - m);
            if (w > 0.f) top = 16 * lane + i;
            run = i == 0 ? w : run + w;
            z[i] = run;
        }
        float incl = run;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        const float before = __shfl_up(incl, 1);
        const float S = __shfl(incl, 63);
        const float target = a.uniforms[cell] * S;
        int first = FINE_VOCAB;
#pragma unroll
        for (int i = 15; i >= 0; --i) {
            const float cum = lane == 0 ? z[i] : before + z[i];
            if (cum > target) first = 16 * lane + i;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            first = min(first, __shfl_xor(first, o));
            top = max(top, __shfl_xor(top, o));
        }
        tok = first < FINE_VOCAB ? first : max(top, 0);
    }
    if (lane == 0) {
        a.work[((size_t)b * a.Lmax + p.start[j] + t) * FINE_CODES + a.c] = tok;
        if (a.ids_out) a.ids_out[cell] = tok;
    }
}

// out[b][ch][t] = work[b][t][ch] for t < T_b; the rest of out is left as it was
__global__ __launch_bounds__(256) void fine_finish_kernel(RowLens lens, int B, int Lmax, int max_T, const int* work, int* out, int t_stride) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * max_T) return;
    const int b = (int)(i / max_T), t = (int)(i % max_T);
    if (t >= lens.T[b]) return;
    const int4* cell = reinterpret_cast<const int4*>(work + ((size_t)b * Lmax + t) * FINE_CODES);
    const int4 lo = cell[0], hi = cell[1];
    const int ids[FINE_CODES] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int ch = 0; ch < FINE_CODES; ++ch) out[((size_t)b * FINE_CODES + ch) * t_stride + t] = ids[ch];
}

// ---- the forward of one pass for code book c: logits of the pass's head rows ----------------------------------------------------------------
int run_forward(const at_fine* h, const FineState& s, const FinePass& p, int c, hipStream_t stream) {
    const int W = h->block, E = h->embd, M = p.n * W, total = p.head_off[p.n];
    FineTables tab;
    for (int i = 0; i < FINE_CODES; ++i) tab.t[i] = h->wtes[i];
    hipLaunchKernelGGL(fine_embed_kernel, dim3(M), dim3(E / 4), 0, stream, p, tab, h->wpe, s.work, s.Lmax, W, E, c, s.x);
    AT_CHECK_HIP(hipGetLastError());
    auto dense = [&](const float* X, int rows, int K, const float* Wt, const float* bias, int N, float* C, const float* Res, int epi) {
        GemmArgs g;
        g.X = X; g.Tin = rows; g.Cin = K; g.ldx = K; g.W = Wt; g.bias = bias; g.C = C; g.ldc = N; g.R = Res; g.ldr = N; g.M = rows; g.N = N; g.K = K; g.epi = epi;
        return launch_gemm(g, stream);
    };
    for (int l = 0; l < h->n_layer; ++l) {
        const FineLayer& w = h->layers[l];
        if (int rc = launch_layernorm(s.x, w.ln1_g, w.ln1_b, nullptr, s.xn, M, E, stream)) return rc;
        if (int rc = dense(s.xn, M, E, w.qkv, w.qkv_b, 3 * E, s.qkv, nullptr, EPI_NONE)) return rc;
        AttnArgs at;   // the whole window, no mask (every key's entry is 1), no relative positions; fp32 stated, never the environment's default
        at.qkv = s.qkv; at.amask = s.ones; at.dist_emb = nullptr; at.ctx = s.xn; at.B = p.n; at.T = W; at.heads = E / 64; at.arith = 0;
        if (int rc = launch_relpos_attention(at, stream)) return rc;
        if (int rc = dense(s.xn, M, E, w.proj, w.proj_b, E, s.x, s.x, EPI_NONE)) return rc;
        if (int rc = launch_layernorm(s.x, w.ln2_g, w.ln2_b, nullptr, s.xn, M, E, stream)) return rc;
        if (int rc = dense(s.xn, M, E, w.fc, w.fc_b, 4 * E, s.h, nullptr, EPI_GELU)) return rc;
        if (int rc = dense(s.h, M, 4 * E, w.fc_proj, w.fc_proj_b, E, s.x, s.x, EPI_NONE)) return rc;
    }
    // the final LayerNorm and the head on the predicted positions only; columns [0, 1024) of the head: its first 1024 rows
    const float* rows = s.x;
    if (total < M) {
        hipLaunchKernelGGL(fine_gather_kernel, dim3(total), dim3(E / 4), 0, stream, p, W, E, s.x, s.h);
        AT_CHECK_HIP(hipGetLastError());
        rows = s.h;
    }
    if (int rc = launch_layernorm(rows, h->lnf_g, h->lnf_b, nullptr, s.xn, total, E, stream)) return rc;
    return dense(s.xn, total, E, h->heads[c - 1], nullptr, FINE_VOCAB, s.logits, nullptr, EPI_NONE);
}

const FineHostTensor* staged(const at_fine* h, const std::string& name) {
    auto it = h->staged.find(name);
    return it == h->staged.end() ? nullptr : &it->second;
}

int upload(at_fine* h, const std::string& name, std::vector<int64_t> shape, const float** dst) {
    const FineHostTensor* t = staged(h, name);
    if (!t) { set_error("at_fine_finalize: missing tensor " + name); return -1; }
    if (t->shape != shape) { set_error("at_fine_finalize: tensor " + name + " has an unexpected shape"); return -1; }
    void* d = nullptr;
    AT_CHECK_HIP(hipMalloc(&d, t->data.size() * sizeof(float)));
    h->allocs.push_back(d);
    AT_CHECK_HIP(hipMemcpy(d, t->data.data(), t->data.size() * sizeof(float), hipMemcpyHostToDevice));
    *dst = static_cast<const float*>(d);
    return 0;
}

void release(at_fine* h) {
    for (void* p : h->allocs) (void)hipFree(p);
    h->allocs.clear();
    h->layers.clear();
    for (auto& t : h->wtes) t = nullptr;
    for (auto& t : h->heads) t = nullptr;
    h->wpe = h->lnf_g = h->lnf_b = nullptr;
}

const char* const kLinears[4] = {".attn.c_attn", ".attn.c_proj", ".mlp.c_fc", ".mlp.c_proj"};

}  // namespace

extern "C" {

at_fine_t* at_fine_create(int device_id) {
    int n = 0;
    if (!host_only_test() && (hipGetDeviceCount(&n) != hipSuccess || device_id < 0 || device_id >= n)) {
        set_error("at_fine_create: no such HIP device " + std::to_string(device_id));
        return nullptr;
    }
    at_fine* h = new at_fine();
    h->device = device_id;
    return h;
}

int at_fine_set_tensor(at_fine_t* h, const char* name, const float* host_data, const int64_t* shape, int ndim) {
    AT_REQUIRE(h && name && host_data && shape && ndim >= 1 && ndim <= 4, "bad arguments");
    AT_REQUIRE(!h->finalized, "model already finalized");
    FineHostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        AT_REQUIRE(shape[i] >= 1 && shape[i] <= (int64_t)1 << 32, "bad dimension");
        t.shape.push_back(shape[i]);
        n *= (size_t)shape[i];
    }
    t.data.assign(host_data, host_data + n);
    h->staged[name] = std::move(t);
    return 0;
}

int at_fine_finalize(at_fine_t* h) {
    AT_REQUIRE(h != nullptr, "null handle");
    AT_REQUIRE(!h->finalized, "model already finalized");
    const FineHostTensor* wpe = staged(h, "transformer.wpe.weight");
    AT_REQUIRE(wpe && wpe->shape.size() == 2, "transformer.wpe.weight [block][n_embd] is needed");
    const int64_t W = wpe->shape[0], E = wpe->shape[1];
    AT_REQUIRE(E == 768 || E == 1024, "n_embd must be 768 or 1024 (heads of 64): what the kernels implement");
    AT_REQUIRE(W >= 128 && W % 128 == 0 && W <= FINE_MAX_BLOCK, "the block size must be a multiple of 128, from 128 to 1024");
    int n_layer = 0;
    while (staged(h, "transformer.h." + std::to_string(n_layer) + ".ln_1.weight")) ++n_layer;
    AT_REQUIRE(n_layer >= 1 && n_layer <= FINE_MAX_LAYERS, "1 to 48 layers (transformer.h.<i>.ln_1.weight, ...)");
    int biases = 0;
    for (int l = 0; l < n_layer; ++l)
        for (const char* lin : kLinears) biases += staged(h, "transformer.h." + std::to_string(l) + lin + ".bias") ? 1 : 0;
    AT_REQUIRE(biases == 0 || biases == 4 * n_layer, "the linears carry a bias in every block or in none");
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    h->embd = (int)E;
    h->block = (int)W;
    h->n_layer = n_layer;
    h->bias = biases != 0;
    h->layers.resize(n_layer);
    int rc = upload(h, "transformer.wpe.weight", {W, E}, &h->wpe);
    for (int i = 0; i < FINE_CODES && !rc; ++i) rc = upload(h, "transformer.wtes." + std::to_string(i) + ".weight", {FINE_TABLE, E}, &h->wtes[i]);
    for (int j = 0; j < FINE_HEADS && !rc; ++j) rc = upload(h, "lm_heads." + std::to_string(j) + ".weight", {FINE_TABLE, E}, &h->heads[j]);
    if (!rc) rc = upload(h, "transformer.ln_f.weight", {E}, &h->lnf_g);
    if (!rc) rc = upload(h, "transformer.ln_f.bias", {E}, &h->lnf_b);
    for (int l = 0; l < n_layer && !rc; ++l) {
        const std::string p = "transformer.h." + std::to_string(l);
        FineLayer& w = h->layers[l];
        rc = upload(h, p + ".ln_1.weight", {E}, &w.ln1_g);
        if (!rc) rc = upload(h, p + ".ln_1.bias", {E}, &w.ln1_b);
        if (!rc) rc = upload(h, p + ".attn.c_attn.weight", {3 * E, E}, &w.qkv);
        if (!rc) rc = upload(h, p + ".attn.c_proj.weight", {E, E}, &w.proj);
        if (!rc) rc = upload(h, p + ".ln_2.weight", {E}, &w.ln2_g);
        if (!rc) rc = upload(h, p + ".ln_2.bias", {E}, &w.ln2_b);
        if (!rc) rc = upload(h, p + ".mlp.c_fc.weight", {4 * E, E}, &w.fc);
        if (!rc) rc = upload(h, p + ".mlp.c_proj.weight", {E, 4 * E}, &w.fc_proj);
        if (h->bias) {
            if (!rc) rc = upload(h, p + ".attn.c_attn.bias", {3 * E}, &w.qkv_b);
            if (!rc) rc = upload(h, p + ".attn.c_proj.bias", {E}, &w.proj_b);
            if (!rc) rc = upload(h, p + ".mlp.c_fc.bias", {4 * E}, &w.fc_b);
            if (!rc) rc = upload(h, p + ".mlp.c_proj.bias", {E}, &w.fc_proj_b);
        }
    }
    if (rc) { release(h); return rc; }
    h->staged.clear();
    h->finalized = true;
    return 0;
}

void at_fine_destroy(at_fine_t* h) {
    if (!h) return;
    {
        DeviceGuard guard(h->device);
        release(h);
    }
    delete h;
}

int at_fine_num_layers(const at_fine_t* h) { return h && h->finalized ? h->n_layer : 0; }
int at_fine_hidden(const at_fine_t* h) { return h && h->finalized ? h->embd : 0; }
int at_fine_block_size(const at_fine_t* h) { return h && h->finalized ? h->block : 0; }
int at_fine_has_bias(const at_fine_t* h) { return h && h->finalized && h->bias ? 1 : 0; }

int at_fine_num_windows(const at_fine_t* h, int T) {
    if (!(h && h->finalized)) { set_error("at_fine_num_windows: the model is not finalized"); return 0; }
    if (!(T >= 1 && T <= FINE_MAX_T)) { set_error("at_fine_num_windows: T must be 1 to 262144"); return 0; }
    return fine_windows(T, h->block);
}

size_t at_fine_state_bytes(const at_fine_t* h, int B, int max_T) {
    if (!(h && h->finalized)) { set_error("at_fine_state_bytes: the model is not finalized"); return 0; }
    if (!(B >= 1 && B <= FINE_MAX_B)) { set_error("at_fine_state_bytes: B must be 1 to 64"); return 0; }
    if (!(max_T >= 1 && max_T <= FINE_MAX_T)) { set_error("at_fine_state_bytes: max_T must be 1 to 262144"); return 0; }
    return carve_state(nullptr, B, max_T, h->block, h->embd).bytes;
}

int at_fine_generate(at_fine_t* h, const int32_t* coarse_dev, int t_stride, const int32_t* lens, int B, float temperature, int greedy,
                     const float* uniforms_dev, int n_max, int32_t* out_dev, float* logits_out_dev, int32_t* window_ids_dev, void* state_dev, size_t state_bytes,
                     int max_T, at_stream_t stream_, int32_t* status_dev) {
    AT_REQUIRE(h && h->finalized, "the model is not finalized");
    AT_REQUIRE(B >= 1 && B <= FINE_MAX_B, "B must be 1 to 64");
    AT_REQUIRE(coarse_dev && lens && out_dev, "null pointer");
    AT_REQUIRE(greedy == 0 || greedy == 1, "greedy must be 0 or 1");
    AT_REQUIRE(greedy || uniforms_dev, "null pointer: sampling needs the uniforms");
    AT_REQUIRE(greedy || (std::isfinite(temperature) && temperature > 0.0f), "temperature must be a positive finite number");
    AT_REQUIRE(state_dev != nullptr, "null state");
    AT_REQUIRE(max_T >= 1 && max_T <= FINE_MAX_T, "max_T must be 1 to 262144");
    AT_REQUIRE(t_stride >= 1 && t_stride <= FINE_MAX_T, "t_stride must be 1 to 262144");
    const int W = h->block, H = W / 2;
    RowLens rl{};
    int n_b[FINE_MAX_B], n_most = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 1 || lens[b] > t_stride || lens[b] > max_T) {
            set_error("at_fine_generate: the length of row " + std::to_string(b) + " must be 1 to min(t_stride, max_T)");
            return -1;
        }
        rl.T[b] = lens[b];
        n_b[b] = fine_windows(lens[b], W);
        n_most = n_b[b] > n_most ? n_b[b] : n_most;
    }
    AT_REQUIRE(n_max >= n_most, "n_max must hold the windows of the longest row: at_fine_num_windows(h, T)");
    const FineState s = carve_state(state_dev, B, max_T, W, h->embd);
    AT_REQUIRE(state_bytes >= s.bytes, "state too small: at_fine_state_bytes(h, B, max_T)");
    // ---- nothing above touched the device
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t cells = (size_t)B * s.Lmax;
    hipLaunchKernelGGL(fine_init_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream, rl, B, s.Lmax, B * W, coarse_dev, t_stride, s.work, s.ones,
                       status_dev);
    AT_CHECK_HIP(hipGetLastError());
    FineSampleArgs sa{};
    sa.logits = s.logits; sa.W = W; sa.Lmax = s.Lmax; sa.n_max = n_max; sa.greedy = greedy; sa.temperature = greedy ? 1.0f : temperature;
    sa.uniforms = uniforms_dev; sa.work = s.work; sa.logits_out = logits_out_dev; sa.ids_out = window_ids_dev;
    for (int k = 0; k < n_most; ++k) {
        FinePass p{};
        for (int b = 0; b < B; ++b) {
            if (n_b[b] <= k) continue;
            const int L = rl.T[b] > W ? rl.T[b] : W, j = p.n++;
            const int start = k * H < L - W ? k * H : L - W, fill = k * H < L - H ? k * H : L - H;
            p.row[j] = b;
            p.start[j] = start;
            p.rel[j] = fill - start;
            p.head_off[j + 1] = p.head_off[j] + W - p.rel[j];
        }
        sa.k = k;
        sa.total = p.head_off[p.n];
        for (int c = FINE_COARSE; c < FINE_CODES; ++c) {
            if (int rc = run_forward(h, s, p, c, stream)) return rc;
            sa.c = c;
            hipLaunchKernelGGL(fine_sample_kernel, dim3((sa.total + SAMPLE_WAVES - 1) / SAMPLE_WAVES), dim3(64 * SAMPLE_WAVES), 0, stream, p, sa);
            AT_CHECK_HIP(hipGetLastError());
        }
    }
    const size_t outs = (size_t)B * max_T;
    hipLaunchKernelGGL(fine_finish_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, stream, rl, B, s.Lmax, max_T, s.work, out_dev, t_stride);
    AT_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
