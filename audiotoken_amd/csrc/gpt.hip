// The semantic-to-acoustic decoder's first stage: a nanoGPT-style model (pre-LN, gain-only LayerNorm, bias-free linears, 12 heads of 64,
// learned positions, tied head) generating with a KV cache. One call prefills every row's prompt and then enqueues one step per new token without waiting
// for the host; the rows' lengths, last tokens and finish flags live on the device. Kernels, all fp32:
//   gpt_embed_kernel    token + position rows
//   gpt_ln_kernel       LayerNorm (two-pass, one wave per row), optionally gathering the rows the head needs
//   gpt_linear_kernel   out[R][N] = A[R][K] . W[N][K]^T for few rows: weights straight from global memory to registers in 16-byte loads, 16 activation rows per
//                       pass, fp32 FMA, a fixed-order reduction; epilogues: none / GELU / residual add / q + K,V scattered into the cache
//                       A prefill of more than 64 tokens runs its four linears per layer on the fp32 matrix-core GEMM instead (gemm_f32.hip, launch_gemm).
//   gpt_attn_kernel     causal attention of one query over its row's cache, one workgroup of 4 waves per (token, head)
//   gpt_sample_kernel   temperature, allow ranges, exact top-k threshold (radix select), softmax weights and the inverse-CDF draw, one workgroup per row
//   gpt_window_kernel   the long form: the prompts of one window of every row, from the source ids and the row's own output stream
//   gpt_tick_kernel     the queue: one tick's token list, step tokens of the rows that are mid-window and the prompts of the windows that begin,
//                       with gpt_embed_list_kernel, the embedding that reads it
// Nothing here adds floats atomically: every sum has one order, so a call repeated gives the same tokens.
#include <cmath>
#include <cstring>

#include "../../include/audiotoken_hip.h"
#include "gpt.h"

using namespace at;

namespace {

constexpr int E = GPT_EMBD, HD = GPT_HEAD_DIM, NH = GPT_HEADS, FF = GPT_FF;
constexpr int LIN_COLS = 4;            // output columns of one workgroup of the linear kernel
constexpr int SAMPLE_THREADS = 1024;

// ---- caller-owned state --------------------------------------------------------------------------------------------------------------------
struct GptState {
    int *len, *done, *cur, *last_row, *tok_row, *tok_pos;
    float *x, *xn, *q, *h, *xh, *logits, *kc, *vc;
    size_t layer_stride;   // floats of one layer's K (or V) cache: B * 12 * cap * 64
    size_t bytes;
};

size_t round256(size_t n) { return (n + 255) / 256 * 256; }

GptState carve_state(void* base, int B, int cap, int vocab, int n_layer) {
    GptState s{};
    char* p = static_cast<char*>(base);
    size_t off = 0;
    auto take = [&](size_t bytes) { char* r = p ? p + off : nullptr; off += round256(bytes); return r; };
    const size_t R = (size_t)B * cap;
    s.len = (int*)take(GPT_MAX_B * 4);
    s.done = (int*)take(GPT_MAX_B * 4);
    s.cur = (int*)take(GPT_MAX_B * 4);
    s.last_row = (int*)take(GPT_MAX_B * 4);
    s.tok_row = (int*)take(R * 4);
    s.tok_pos = (int*)take(R * 4);
    s.x = (float*)take(R * E * 4);
    s.xn = (float*)take(R * E * 4);
    s.q = (float*)take(R * 3 * E * 4);   // steps: q [R][768]; prefill on the GEMM: q | k | v [R][2304]
    s.h = (float*)take(R * FF * 4);
    s.xh = (float*)take((size_t)GPT_MAX_B * E * 4);
    s.logits = (float*)take((size_t)B * vocab * 4);
    s.layer_stride = R * NH * HD;
    s.kc = (float*)take(s.layer_stride * n_layer * 4);
    s.vc = (float*)take(s.layer_stride * n_layer * 4);
    s.bytes = off;
    return s;
}

// ---- small device helpers ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
// 64 per-lane values summed over the 64 lanes of a wave in 63 exchanges: at step s a lane keeps the half of its values that its bit s selects and adds
// its partner's copy of that half. Lane l ends with the wave's sum of value number bitrev6(l) in v[0]. One order of additions per value.
__device__ __forceinline__ void wave_transpose_sum64(float (&v)[64], int lane) {
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const int half = 32 >> s;
        // the choice as a bit mask on the values: a select between two array elements becomes a run-time index, and the array then lives in scratch
        const unsigned up = 0u - ((unsigned)(lane >> s) & 1u);
#pragma unroll
        for (int i = 0; i < half; ++i) {
            const unsigned lo = __float_as_uint(v[i]), hi = __float_as_uint(v[i + half]);
            const float keep = __uint_as_float((hi & up) | (lo & ~up));
            const float send = __uint_as_float((lo & up) | (hi & ~up));
            v[i] = keep + __shfl_xor(send, 1 << s);
        }
    }
}
__device__ __forceinline__ int bitrev6(int lane) { return (int)(__brev((unsigned)lane) >> 26); }

// ---- bookkeeping ---------------------------------------------------------------------------------------------------------------------------
struct PromptLens {
    int off[GPT_MAX_B + 1];   // row b's prompt tokens are the pass's tokens [off[b], off[b + 1])
};

// start of a call: the prefill's token list and the rows' state
__global__ void gpt_init_kernel(PromptLens pl, int B, int R, int block, int* len, int* done, int* cur, int* last_row, int* tok_row, int* tok_pos,
                                int* out_len, int* finish) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < R) {
        int b = 0;
        while (b + 1 < B && pl.off[b + 1] <= i) ++b;
        tok_row[i] = b;
        tok_pos[i] = i - pl.off[b];
    }
    if (i < B) {
        const int P = pl.off[i + 1] - pl.off[i];
        len[i] = P;
        const int d = P >= block ? GPT_FINISH_BLOCK : GPT_RUNNING;   // no room for a single new token
        done[i] = d;
        finish[i] = d;
        out_len[i] = 0;
        cur[i] = 0;
        last_row[i] = pl.off[i + 1] - 1;
    }
}

// x[i] = wte[id] + wpe[pos]. Prefill (prompts != nullptr): token i of the list made by gpt_init_kernel. Step: token i is row i's last sampled id at position
// len - 1; the kernel writes the list itself. An id outside [0, V) is clamped and reported in bit 0 of *status.
__global__ __launch_bounds__(E / 4) void gpt_embed_kernel(const int* prompts, int prompt_stride, const float* wte, const float* wpe, int V, int block,
                                                           const int* len, const int* cur, int* last_row, int* tok_row, int* tok_pos, float* x, int* status) {
    const int i = blockIdx.x, t = threadIdx.x;
    int b, p, id;
    if (prompts) {
        b = tok_row[i];
        p = tok_pos[i];
        id = prompts[(size_t)b * prompt_stride + p];
    } else {
        b = i;
        p = min(max(len[b] - 1, 0), block - 1);
        id = cur[b];
        if (t == 0) { tok_row[i] = b; tok_pos[i] = p; last_row[b] = b; }
    }
    if (id < 0 || id >= V) {
        if (t == 0 && status) atomicOr(status, 1);
        id = min(max(id, 0), V - 1);
    }
    const float4 a = reinterpret_cast<const float4*>(wte + (size_t)id * E)[t];
    const float4 c = reinterpret_cast<const float4*>(wpe + (size_t)p * E)[t];
    reinterpret_cast<float4*>(x + (size_t)i * E)[t] = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w);
}

// The queue's form: token i of a list that gpt_tick_kernel resolved, prompt tokens and step tokens alike: x[i] = wte[tok_id[i]] + wpe[tok_pos[i]].
// The list's ids are the model's own (sampled, or clamped when the prompt was written); the clamp here only keeps a corrupted list inside the tables.
__global__ __launch_bounds__(E / 4) void gpt_embed_list_kernel(const int* tok_id, const int* tok_pos, const float* wte, const float* wpe, int V, int block, float* x,
                                                                int* status) {
    const int i = blockIdx.x, t = threadIdx.x;
    int id = tok_id[i];
    const int p = min(max(tok_pos[i], 0), block - 1);
    if (id < 0 || id >= V) {
        if (t == 0 && status) atomicOr(status, 1);
        id = min(max(id, 0), V - 1);
    }
    const float4 a = reinterpret_cast<const float4*>(wte + (size_t)id * E)[t];
    const float4 c = reinterpret_cast<const float4*>(wpe + (size_t)p * E)[t];
    reinterpret_cast<float4*>(x + (size_t)i * E)[t] = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w);
}

// y[r] = (x[src] - mean) * rstd * gain, eps 1e-5, no bias; src = gather ? gather[r] : r. One wave per row, the row in registers, variance from the centred values.
__global__ __launch_bounds__(256) void gpt_ln_kernel(const float* x, const float* gain, const int* gather, float* y, int R) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int src = gather ? gather[r] : r;
    const float4* xr = reinterpret_cast<const float4*>(x + (size_t)src * E);
    float4 v[3];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) { v[j] = xr[lane + 64 * j]; s += (v[j].x + v[j].y) + (v[j].z + v[j].w); }
    const float mean = wave_sum(s) * (1.0f / E);
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        v[j].x -= mean; v[j].y -= mean; v[j].z -= mean; v[j].w -= mean;
        ss += (v[j].x * v[j].x + v[j].y * v[j].y) + (v[j].z * v[j].z + v[j].w * v[j].w);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(ss) * (1.0f / E) + 1e-5f);
    const float4* g = reinterpret_cast<const float4*>(gain);
    float4* yr = reinterpret_cast<float4*>(y + (size_t)r * E);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float4 gg = g[lane + 64 * j];
        yr[lane + 64 * j] = make_float4(v[j].x * rstd * gg.x, v[j].y * rstd * gg.y, v[j].z * rstd * gg.z, v[j].w * rstd * gg.w);
    }
}

// ---- linear layers -------------------------------------------------------------------------------------------------------------------------
enum { LIN_NONE = 0, LIN_GELU = 1, LIN_RESID = 2, LIN_QKV = 3 };
struct LinArgs {
    const float* A;   // [R][K]
    const float* W;   // [N][K]
    float* out;       // [R][N] (LIN_QKV: q [R][768]); LIN_RESID adds into it
    int R, N;
    // LIN_QKV: where K and V rows go
    const int *tok_row, *tok_pos, *done;
    float *kc, *vc;   // this layer's caches [B][12][cap][64]
    int cap;
};

// One workgroup: LIN_COLS output columns for the GPT_ROW_TILE rows of tile blockIdx.y. Every thread loads its 16-byte pieces of the LIN_COLS weight rows first
// (all loads in flight before the first use; no LDS round trip), then streams the activation rows (a few hundred KB that stay in L2) against them.
// The THREADS * ITERS pieces cover K exactly. Per (row, column): a lane's partial in k order, the lanes by wave_transpose_sum64, the waves in index order.
template <int K, int THREADS, int EPI>
__global__ __launch_bounds__(THREADS) void gpt_linear_kernel(LinArgs a) {
    constexpr int ITERS = K / 4 / THREADS, WAVES = THREADS / 64;
    static_assert(ITERS * THREADS * 4 == K && THREADS % 64 == 0, "the threads' 16-byte pieces tile K");
    static_assert(GPT_ROW_TILE * LIN_COLS == 64, "one value per lane after the reduction");
    __shared__ float red[WAVES][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * LIN_COLS, r0 = blockIdx.y * GPT_ROW_TILE;
    float4 w[ITERS][LIN_COLS];
#pragma unroll
    for (int it = 0; it < ITERS; ++it)
#pragma unroll
        for (int c = 0; c < LIN_COLS; ++c) w[it][c] = reinterpret_cast<const float4*>(a.W + (size_t)(n0 + c) * K)[it * THREADS + tid];
    float acc[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) acc[i] = 0.f;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
#pragma unroll
        for (int r = 0; r < GPT_ROW_TILE; ++r) {
            const int row = min(r0 + r, a.R - 1);   // rows past the end repeat the last one and are not written
            const float4 x = reinterpret_cast<const float4*>(a.A + (size_t)row * K)[it * THREADS + tid];
#pragma unroll
            for (int c = 0; c < LIN_COLS; ++c) {
                float s = acc[r * LIN_COLS + c];
                s = fmaf(x.x, w[it][c].x, s);
                s = fmaf(x.y, w[it][c].y, s);
                s = fmaf(x.z, w[it][c].z, s);
                s = fmaf(x.w, w[it][c].w, s);
                acc[r * LIN_COLS + c] = s;
            }
        }
    }
    wave_transpose_sum64(acc, lane);
    red[wave][bitrev6(lane)] = acc[0];
    __syncthreads();
    if (tid >= 64) return;
    float v = red[0][tid];
#pragma unroll
    for (int wv = 1; wv < WAVES; ++wv) v += red[wv][tid];
    const int row = r0 + tid / LIN_COLS, n = n0 + tid % LIN_COLS;
    if (row >= a.R) return;
    if (EPI == LIN_NONE) {
        a.out[(size_t)row * a.N + n] = v;
    } else if (EPI == LIN_GELU) {
        a.out[(size_t)row * a.N + n] = gelu_erf(v);
    } else if (EPI == LIN_RESID) {
        a.out[(size_t)row * a.N + n] += v;
    } else {
        const int part = n / E, col = n % E;
        if (part == 0) {
            a.out[(size_t)row * E + col] = v;
        } else {
            const int b = a.tok_row[row], p = a.tok_pos[row];
            if (a.done[b] == GPT_RUNNING && p < a.cap)   // a finished row leaves its cache as it is
                (part == 1 ? a.kc : a.vc)[(((size_t)b * NH + col / HD) * a.cap + p) * HD + col % HD] = v;
        }
    }
}

template <int K, int THREADS, int EPI>
int launch_linear(const LinArgs& a, hipStream_t stream) {
    const dim3 grid(a.N / LIN_COLS, (a.R + GPT_ROW_TILE - 1) / GPT_ROW_TILE);
    hipLaunchKernelGGL((gpt_linear_kernel<K, THREADS, EPI>), grid, dim3(THREADS), 0, stream, a);
    AT_CHECK_HIP(hipGetLastError());
    return 0;
}

// The prefill on the GEMM leaves q | k | v rows [R][2304]: the K and V parts into the cache (what LIN_QKV's epilogue does for a step)
__global__ __launch_bounds__(E / 4) void gpt_kv_scatter_kernel(const float* qkv, const int* tok_row, const int* tok_pos, const int* done, float* kc, float* vc, int cap) {
    const int i = blockIdx.x, t = threadIdx.x;
    const int b = tok_row[i], p = tok_pos[i];
    if (done[b] != GPT_RUNNING || p >= cap) return;
    const int col = 4 * t;
    const size_t dst = (((size_t)b * NH + col / HD) * cap + p) * HD + col % HD;
    const float4* src = reinterpret_cast<const float4*>(qkv + (size_t)i * 3 * E);
    *reinterpret_cast<float4*>(kc + dst) = src[E / 4 + t];
    *reinterpret_cast<float4*>(vc + dst) = src[2 * (E / 4) + t];
}

// ---- attention -----------------------------------------------------------------------------------------------------------------------------
// Token i (row b, position p), head blockIdx.y: softmax(q . K[0..p] / 8) . V[0..p] over the row's cache, one workgroup of 4 waves. A thread owns keys tid, tid + 256,
// ...: at most 4 of them (block <= 1024), so its scores stay in registers and the softmax is the plain max / exp / sum form, with nothing to rescale. Loads are
// unconditional (a key past the end repeats the last one and gets weight 0), so the loads of all of a thread's keys can be in flight together. The lanes' partial
// outputs meet in wave_transpose_sum64, the waves through LDS in index order. Prefill tokens and step tokens differ only in p.
constexpr int ATTN_THREADS = 256;
__global__ __launch_bounds__(ATTN_THREADS) void gpt_attn_kernel(const float* q, int ldq, const float* kc, const float* vc, const int* tok_row, const int* tok_pos,
                                                                float* ctx, int cap) {
    constexpr int WAVES = ATTN_THREADS / 64, MAXJ = GPT_MAX_BLOCK / ATTN_THREADS;
    __shared__ float red[WAVES][64];
    __shared__ float part[WAVES];
    const int i = blockIdx.x, h = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = tok_row[i], n = min(tok_pos[i], cap - 1) + 1;
    const float4* qr = reinterpret_cast<const float4*>(q + (size_t)i * ldq + h * HD);
    float4 qv[HD / 4];
#pragma unroll
    for (int d = 0; d < HD / 4; ++d) qv[d] = qr[d];
    const size_t base = ((size_t)b * NH + h) * cap * HD;
    const float4* K4 = reinterpret_cast<const float4*>(kc + base);
    const float4* V4 = reinterpret_cast<const float4*>(vc + base);
    float s[MAXJ];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        s[j] = -INFINITY;
        if (ATTN_THREADS * j < n) {   // uniform over the workgroup
            const int key = tid + ATTN_THREADS * j, kk = min(key, n - 1);
            float dot = 0.f;
#pragma unroll
            for (int d = 0; d < HD / 4; ++d) {
                const float4 k = K4[(size_t)kk * (HD / 4) + d];
                dot = fmaf(qv[d].x, k.x, dot);
                dot = fmaf(qv[d].y, k.y, dot);
                dot = fmaf(qv[d].z, k.z, dot);
                dot = fmaf(qv[d].w, k.w, dot);
            }
            if (key < n) s[j] = dot * 0.125f;
            m = fmaxf(m, s[j]);
        }
    }
    m = wave_max(m);
    if (lane == 0) part[wave] = m;
    __syncthreads();
    m = part[0];
#pragma unroll
    for (int wv = 1; wv < WAVES; ++wv) m = fmaxf(m, part[wv]);
    __syncthreads();
    float o[64];
#pragma unroll
    for (int d = 0; d < 64; ++d) o[d] = 0.f;
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        if (ATTN_THREADS * j < n) {
            const int key = tid + ATTN_THREADS * j, kk = min(key, n - 1);
            const float p = key < n ? expf(s[j] - m) : 0.f;
            l += p;
#pragma unroll
            for (int d = 0; d < HD / 4; ++d) {
                const float4 v = V4[(size_t)kk * (HD / 4) + d];
                o[4 * d + 0] = fmaf(p, v.x, o[4 * d + 0]);
                o[4 * d + 1] = fmaf(p, v.y, o[4 * d + 1]);
                o[4 * d + 2] = fmaf(p, v.z, o[4 * d + 2]);
                o[4 * d + 3] = fmaf(p, v.w, o[4 * d + 3]);
            }
        }
    }
    l = wave_sum(l);
    wave_transpose_sum64(o, lane);
    red[wave][bitrev6(lane)] = o[0];
    if (lane == 0) part[wave] = l;
    __syncthreads();
    if (tid >= 64) return;
    float v = red[0][tid], L = part[0];
#pragma unroll
    for (int wv = 1; wv < WAVES; ++wv) { v += red[wv][tid]; L += part[wv]; }
    ctx[(size_t)i * E + h * HD + tid] = v / L;
}

// ---- the sampler ---------------------------------------------------------------------------------------------------------------------------
struct Allow {
    int on;
    int lo0, hi0, lo1, hi1;   // ids in [lo0, hi0) or [lo1, hi1) are allowed
};
// One row of one pass of the long form (at_gpt_generate_long): which row of the caller's arrays it is, where in that row's stream its step 0 lies (out_ids,
// uniforms and logits_out are indexed by stream position), how many steps it has, what it may produce on even / odd steps and which id stops it (-1: none).
struct SampleRow {
    int out_row, base, budget, stop_token, final_window;
    Allow allow[2];
};
struct SampleArgs {
    const float* logits;      // [B][V]
    int V, top_k;
    float temperature;
    const float* uniforms;    // row b's draw is uniforms[b * u_stride + step]
    int u_stride, step;
    Allow allow;
    int* out;                 // the op alone: out[b] = token; generation: nullptr
    // generation
    int *len, *done, *cur, *out_ids, *out_len, *finish;
    float* logits_out;        // nullable [B][out_stride][V]
    int max_new, stop_token, block;
    int out_stride;           // ids of one row of out_ids (at_gpt_generate: max_new)
    const SampleRow* rows;    // nullable [B]: the long form's per-row rules; nullptr: the call's own scalars
    // the queue (at_gpt_generate_queue; needs rows): workgroup j samples for cache row samp_slot[j] from logits row j, at that row's own step
    int* step_ctr;            // nullable [slots]: steps sampled in the row's window so far; replaces `step`
    const int* samp_slot;     // [gridDim.x]
};

// floats as unsigned keys in the same order
__device__ __forceinline__ unsigned order_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
// step 1 and 2 of the rule: one IEEE division, then the allow ranges
__device__ __forceinline__ float tempered(const float* z, int i, float temperature, const Allow& a) {
    const float v = z[i] / temperature;
    if (a.on && !((i >= a.lo0 && i < a.hi0) || (i >= a.lo1 && i < a.hi1))) return -INFINITY;
    return v;
}

__global__ __launch_bounds__(SAMPLE_THREADS) void gpt_sample_kernel(SampleArgs a) {
    __shared__ unsigned hist[256];
    __shared__ unsigned sel_prefix, sel_k;
    __shared__ float wave_part[SAMPLE_THREADS / 64];
    __shared__ int best_id, high_id;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool queued = a.rows && a.step_ctr;
    const int b = queued ? a.samp_slot[blockIdx.x] : blockIdx.x;
    const bool generating = a.out == nullptr;
    if (generating && a.done[b] != GPT_RUNNING) return;   // a finished row writes nothing more (uniform over the workgroup)
    const int V = a.V;
    const float* z = a.logits + (size_t)blockIdx.x * V;
    // where the step's id, draw and logits live: row b at a.step, or the long form's row and stream position; the queue's rows count their own steps
    // (every thread reads the counter here, thread 0 advances it after the last barrier)
    const int step = queued ? a.step_ctr[b] : a.step;
    const SampleRow* pr = a.rows ? a.rows + b : nullptr;
    if (pr && step >= pr->budget) return;
    const int orow = pr ? pr->out_row : b, pos = (pr ? pr->base : 0) + step;
    const Allow allow = pr ? pr->allow[step & 1] : a.allow;
    if (generating && a.logits_out) {
        float* dst = a.logits_out + ((size_t)orow * a.out_stride + pos) * V;
        for (int i = tid; i < V; i += SAMPLE_THREADS) dst[i] = z[i];
    }
    // ---- the k-th largest tempered value, exactly: radix select over the order keys, 8 bits a pass, and the maximum on the way
    float mx = -INFINITY;
    if (tid == 0) { sel_prefix = 0; sel_k = (unsigned)min(a.top_k, V); best_id = V; high_id = -1; }
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        const unsigned prefix = sel_prefix, need = sel_k, mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
        for (int i = tid; i < V; i += SAMPLE_THREADS) {
            const float v = tempered(z, i, a.temperature, allow);
            if (pass == 0) mx = fmaxf(mx, v);
            const unsigned k = order_key(v);
            if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 256) {   // the one bin that holds the need-th largest of the keys that are left: every bin counts what lies above it
            unsigned above = 0;
            for (int bin = 255; bin > tid; --bin) above += hist[bin];
            if (above < need && need <= above + hist[tid]) {
                sel_k = need - above;
                sel_prefix = prefix | ((unsigned)tid << shift);
            }
        }
        __syncthreads();
    }
    const float thresh = key_value(sel_prefix);
    // ---- m = the largest kept value (the largest of all: it is always kept)
    mx = wave_max(mx);
    if (lane == 0) wave_part[wave] = mx;
    __syncthreads();
    float m = wave_part[0];
#pragma unroll
    for (int wv = 1; wv < SAMPLE_THREADS / 64; ++wv) m = fmaxf(m, wave_part[wv]);
    __syncthreads();
    // ---- S and the running sums in ascending id order. A wave owns a contiguous run of ids and walks it 64 at a time (coalesced): within a group the lanes'
    // weights are scanned (shuffle scan), the groups chain through a carry, the waves' totals are added in wave order. The first walk gives the waves' totals and S,
    // the second the running sums, its carry starting from the total of the waves before.
    const int per_wave = ((V + SAMPLE_THREADS / 64 - 1) / (SAMPLE_THREADS / 64) + 63) / 64 * 64, first = wave * per_wave;
    const float u = a.uniforms[(size_t)orow * a.u_stride + pos];
    float before = 0.f, target = 0.f;
    bool found = false;
    int top = -1;
    for (int walk = 0; walk < 2; ++walk) {
        float carry = before;
        for (int g = 0; g < per_wave; g += 64) {
            const int i = first + g + lane;
            float v = -INFINITY;
            if (i < V) v = tempered(z, i, a.temperature, allow);
            const bool kept = i < V && v >= thresh;
            float incl = kept ? expf(v - m) : 0.f;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const float up = __shfl_up(incl, o);
                if (lane >= o) incl += up;
            }
            if (walk == 1 && kept) {
                if (v > -INFINITY) top = i;   // the fallback never returns an id of weight zero (a threshold of -inf keeps every id)
                if (!found && carry + incl > target) { found = true; atomicMin(&best_id, i); }
            }
            carry += __shfl(incl, 63);
        }
        if (walk == 1) break;
        if (lane == 0) wave_part[wave] = carry;
        __syncthreads();
        float S = 0.f;
#pragma unroll
        for (int wv = 0; wv < SAMPLE_THREADS / 64; ++wv) {
            if (wv == wave) before = S;
            S += wave_part[wv];
        }
        target = u * S;
    }
    if (top >= 0) atomicMax(&high_id, top);
    __syncthreads();
    if (tid != 0) return;
    const int tok = best_id < V ? best_id : max(high_id, 0);
    if (!generating) { a.out[b] = tok; return; }
    // ---- the row's bookkeeping: stop, max_new_tokens, block_size in that order
    if (queued) a.step_ctr[b] = step + 1;
    if (tok == (pr ? pr->stop_token : a.stop_token)) {
        a.done[b] = a.finish[orow] = GPT_FINISH_STOP;
        return;
    }
    a.out_ids[(size_t)orow * a.out_stride + pos] = tok;
    a.out_len[orow] = pos + 1;
    a.cur[b] = tok;
    const int total = a.len[b] + 1;
    a.len[b] = total;
    if (pr && !pr->final_window) {   // the window's count is exact; the row is done for this pass, not for the call
        if (step + 1 >= pr->budget) a.done[b] = GPT_PASS_DONE;
        return;
    }
    if (step + 1 >= a.max_new) a.done[b] = a.finish[orow] = GPT_FINISH_MAX_NEW;
    else if (total >= a.block) a.done[b] = a.finish[orow] = GPT_FINISH_BLOCK;
}

int check_allow(const int32_t* r, int V, Allow* out) {
    out->on = 0;
    out->lo0 = out->hi0 = out->lo1 = out->hi1 = 0;
    if (!r) return 0;
    AT_REQUIRE(r[0] >= 0 && r[0] <= r[1] && r[1] <= V && r[2] >= 0 && r[2] <= r[3] && r[3] <= V, "allow ranges must satisfy 0 <= lo <= hi <= vocab");
    AT_REQUIRE(r[1] > r[0] || r[3] > r[2], "allow ranges are both empty");
    *out = Allow{1, r[0], r[1], r[2], r[3]};
    return 0;
}

int check_sampling(float temperature, int top_k) {
    AT_REQUIRE(std::isfinite(temperature) && temperature > 0.0f, "temperature must be a positive finite number");
    AT_REQUIRE(top_k >= 1, "top_k must be at least 1");
    return 0;
}

// ---- the long form: one window of every row that has one --------------------------------------------------------------------
struct LongPass {
    int off[GPT_MAX_B + 1];          // pass row j's prompt tokens are the pass's tokens [off[j], off[j + 1])
    int row[GPT_MAX_B];              // the caller's row that pass row j is
    unsigned long long final_mask;   // bit j: this is the row's last window
};
struct LongRules {
    int k, S, H, r, semantic_offset, semantic_vocab, infer_token, stop_token, max_new, block;
    Allow mid[2], last[2];           // even / odd steps of a non-final and of a final window
};

// Start of pass k: the prompt rows (source ids + the offset, INFER, the carry out of the row's own stream), the prefill's token list, the rows' state and
// their rules for the sampler. A source id outside [0, semantic_vocab) is clamped and reported in bit 0 of *status.
__global__ void gpt_window_kernel(LongPass p, LongRules q, int Bk, int R, const int* src, int src_stride, const int* out_ids, int out_stride, int* prompts,
                                  int prompt_stride, int* len, int* done, int* cur, int* last_row, int* tok_row, int* tok_pos, SampleRow* rows, int* out_len,
                                  int* finish, int* status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int carry = q.k > 0 ? q.r * (q.S - q.H) : 0;
    if (i < R) {
        int j = 0;
        while (j + 1 < Bk && p.off[j + 1] <= i) ++j;
        const int b = p.row[j], pos = i - p.off[j], n_src = p.off[j + 1] - p.off[j] - 1 - carry;
        int id;
        if (pos < n_src) {
            id = src[(size_t)b * src_stride + q.k * q.H + pos];
            if (id < 0 || id >= q.semantic_vocab) {
                if (status) atomicOr(status, 1);
                id = min(max(id, 0), q.semantic_vocab - 1);
            }
            id += q.semantic_offset;
        } else if (pos == n_src) {
            id = q.infer_token;
        } else {
            id = out_ids[(size_t)b * out_stride + q.r * q.k * q.H + (pos - n_src - 1)];
        }
        prompts[(size_t)j * prompt_stride + pos] = id;
        tok_row[i] = j;
        tok_pos[i] = pos;
    }
    if (i < Bk) {
        const int P = p.off[i + 1] - p.off[i], b = p.row[i];
        const bool last = (p.final_mask >> i) & 1ull;
        len[i] = P;
        done[i] = GPT_RUNNING;
        cur[i] = 0;
        last_row[i] = p.off[i + 1] - 1;
        SampleRow s;
        s.out_row = b;
        s.base = q.r * q.k * q.H + carry;
        s.budget = last ? min(q.max_new, q.block - P) : q.r * q.S - carry;
        s.stop_token = last ? q.stop_token : -1;
        s.final_window = last ? 1 : 0;
        s.allow[0] = last ? q.last[0] : q.mid[0];
        s.allow[1] = last ? q.last[1] : q.mid[1];
        rows[i] = s;
        if (q.k == 0) { out_len[b] = 0; finish[b] = GPT_RUNNING; }
    }
}

struct LongState {
    GptState g;
    int* prompts;      // [B][cap]
    SampleRow* rows;   // [GPT_MAX_B]
    size_t bytes;
};

LongState carve_long_state(void* base, int B, int cap, int vocab, int n_layer) {
    LongState s{};
    s.g = carve_state(base, B, cap, vocab, n_layer);
    char* p = static_cast<char*>(base);
    size_t off = s.g.bytes;
    auto take = [&](size_t bytes) { char* r = p ? p + off : nullptr; off += round256(bytes); return r; };
    s.prompts = (int*)take((size_t)B * cap * 4);
    s.rows = (SampleRow*)take(GPT_MAX_B * sizeof(SampleRow));
    s.bytes = off;
    return s;
}

// What at_gpt_generate_long and at_gpt_generate_queue share: the checks of the geometry, the token space and the sampling arguments, and the rules they make
int check_long_rules(const at_gpt* h, int S, int H, int r, int src_stride, int semantic_offset, int semantic_vocab, int infer_token, int acoustic_offset,
                     int codebook_size, int stop_token, int max_new, float temperature, int top_k, LongRules* out) {
    const int V = h->vocab, block = h->block;
    AT_REQUIRE(S >= 2 && S % 2 == 0 && H >= 2 && H % 2 == 0, "the window S and the hop H must be even, at least 2");
    AT_REQUIRE(H <= S, "the hop H must not exceed the window S");
    AT_REQUIRE(r >= 1 && r <= GPT_MAX_BLOCK, "r (acoustic ids per source id) must be 1 to 1024");
    AT_REQUIRE((int64_t)S + 1 + (int64_t)r * S <= block, "a window does not fit: S + 1 + r S must not exceed the model's block size");
    AT_REQUIRE(src_stride >= 1, "src_stride must be at least 1");
    AT_REQUIRE(max_new >= 1 && max_new <= GPT_MAX_BLOCK, "max_new must be 1 to 1024");
    if (int rc = check_sampling(temperature, top_k)) return rc;
    AT_REQUIRE(semantic_offset >= 0 && semantic_vocab >= 1 && (int64_t)semantic_offset + semantic_vocab <= V, "the semantic ids must lie inside the vocabulary");
    AT_REQUIRE(infer_token >= 0 && infer_token < V, "infer_token is not in the vocabulary");
    AT_REQUIRE(acoustic_offset >= 0 && codebook_size >= 1 && (int64_t)acoustic_offset + 2 * (int64_t)codebook_size <= V,
               "the two code books must lie inside the vocabulary");
    AT_REQUIRE(stop_token < V, "stop_token is not in the vocabulary (negative: none)");
    LongRules q{};
    q.S = S; q.H = H; q.r = r; q.semantic_offset = semantic_offset; q.semantic_vocab = semantic_vocab; q.infer_token = infer_token;
    q.stop_token = stop_token < 0 ? -1 : stop_token; q.max_new = max_new; q.block = block;
    q.mid[0] = Allow{1, acoustic_offset, acoustic_offset + codebook_size, 0, 0};
    q.mid[1] = Allow{1, acoustic_offset + codebook_size, acoustic_offset + 2 * codebook_size, 0, 0};
    q.last[0] = q.mid[0];
    q.last[1] = q.mid[1];
    if (stop_token >= 0) { q.last[0].lo1 = stop_token; q.last[0].hi1 = stop_token + 1; }
    *out = q;
    return 0;
}

// ---- the queue: one tick of any mix of windows that begin and rows that step -----------------------------------------------------
struct TickPlan {
    int n_step, n_start, R;               // the list: n_step step tokens, then the prompts; R tokens in all
    int off[GPT_MAX_B + 1];               // start j's prompt tokens are the list's [off[j], off[j + 1])
    int src[GPT_MAX_B], k[GPT_MAX_B];     // start j: window k[j] of source src[j]
    unsigned char slot[GPT_MAX_B];        //          in cache row slot[j]
    unsigned char step_slot[GPT_MAX_B];   // the cache row of step token i
    unsigned long long final_mask;        // bit j: start j is its source's last window
};

// Start of a tick: the resolved token list (row, position, id of every token), the sampling list (which token's logits each sampling row draws from and
// whose cache row that is) and, for every window that begins, what gpt_window_kernel writes for a row of a pass, plus its zeroed step counter. A step
// token is its row's last sampled id at position len - 1; the samplers before this launch wrote both, and the carry ids in out_ids, in stream order.
// A slot either steps or begins in a tick, never both, so no word is read and written here. A source id outside [0, semantic_vocab) is clamped and reported.
__global__ void gpt_tick_kernel(TickPlan p, LongRules q, const int* src, int src_stride, const int* out_ids, int out_stride, int* len, int* done, int* cur,
                                int* step_ctr, int* last_row, int* samp_slot, int* tok_row, int* tok_pos, int* tok_id, SampleRow* rows, int* out_len,
                                int* finish, int* status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < p.n_step) {
        const int slot = p.step_slot[i];
        tok_row[i] = slot;
        tok_pos[i] = min(max(len[slot] - 1, 0), q.block - 1);
        tok_id[i] = cur[slot];
        last_row[i] = i;
        samp_slot[i] = slot;
    } else if (i < p.R) {
        int j = 0;
        while (j + 1 < p.n_start && p.off[j + 1] <= i) ++j;
        const int b = p.src[j], k = p.k[j], carry = k > 0 ? q.r * (q.S - q.H) : 0;
        const int pos = i - p.off[j], n_src = p.off[j + 1] - p.off[j] - 1 - carry;
        int id;
        if (pos < n_src) {
            id = src[(size_t)b * src_stride + k * q.H + pos];
            if (id < 0 || id >= q.semantic_vocab) {
                if (status) atomicOr(status, 1);
                id = min(max(id, 0), q.semantic_vocab - 1);
            }
            id += q.semantic_offset;
        } else if (pos == n_src) {
            id = q.infer_token;
        } else {
            id = out_ids[(size_t)b * out_stride + q.r * k * q.H + (pos - n_src - 1)];
        }
        tok_row[i] = p.slot[j];
        tok_pos[i] = pos;
        tok_id[i] = id;
    }
    if (i < p.n_start) {
        const int P = p.off[i + 1] - p.off[i], b = p.src[i], k = p.k[i], slot = p.slot[i], carry = k > 0 ? q.r * (q.S - q.H) : 0;
        const bool last = (p.final_mask >> i) & 1ull;
        len[slot] = P;
        done[slot] = GPT_RUNNING;
        cur[slot] = 0;
        step_ctr[slot] = 0;
        last_row[p.n_step + i] = p.off[i + 1] - 1;
        samp_slot[p.n_step + i] = slot;
        SampleRow s;
        s.out_row = b;
        s.base = q.r * k * q.H + carry;
        s.budget = last ? min(q.max_new, q.block - P) : q.r * q.S - carry;
        s.stop_token = last ? q.stop_token : -1;
        s.final_window = last ? 1 : 0;
        s.allow[0] = last ? q.last[0] : q.mid[0];
        s.allow[1] = last ? q.last[1] : q.mid[1];
        rows[slot] = s;
        if (k == 0) { out_len[b] = 0; finish[b] = GPT_RUNNING; }
    }
}

// K / V for `slots` rows of `cap` positions, activations for `T` token rows, nothing per source
struct QueueState {
    GptState g;
    int *tok_id, *samp_slot, *step_ctr;
    SampleRow* rows;   // [GPT_MAX_B], by slot
    size_t bytes;
};

QueueState carve_queue_state(void* base, int slots, int cap, int T, int vocab, int n_layer) {
    QueueState q{};
    GptState& s = q.g;
    char* p = static_cast<char*>(base);
    size_t off = 0;
    auto take = [&](size_t bytes) { char* r = p ? p + off : nullptr; off += round256(bytes); return r; };
    const size_t R = (size_t)T;
    s.len = (int*)take(GPT_MAX_B * 4);
    s.done = (int*)take(GPT_MAX_B * 4);
    s.cur = (int*)take(GPT_MAX_B * 4);
    s.last_row = (int*)take(GPT_MAX_B * 4);
    q.samp_slot = (int*)take(GPT_MAX_B * 4);
    q.step_ctr = (int*)take(GPT_MAX_B * 4);
    q.rows = (SampleRow*)take(GPT_MAX_B * sizeof(SampleRow));
    s.tok_row = (int*)take(R * 4);
    s.tok_pos = (int*)take(R * 4);
    q.tok_id = (int*)take(R * 4);
    s.x = (float*)take(R * E * 4);
    s.xn = (float*)take(R * E * 4);
    s.q = (float*)take(R * 3 * E * 4);
    s.h = (float*)take(R * FF * 4);
    s.xh = (float*)take((size_t)GPT_MAX_B * E * 4);
    s.logits = (float*)take((size_t)slots * vocab * 4);
    s.layer_stride = (size_t)slots * cap * NH * HD;
    s.kc = (float*)take(s.layer_stride * n_layer * 4);
    s.vc = (float*)take(s.layer_stride * n_layer * 4);
    s.bytes = q.bytes = off;
    return q;
}

// ---- one pass of the model over R tokens: the prefill of every prompt (prompts != nullptr) or one step of every row (R = B) -----------------------------
// The model over the R embedded tokens of s.x, each at (tok_row, tok_pos), then the head for the B tokens that s.last_row names: logits row j belongs to token last_row[j].
int run_layers(const at_gpt* h, const GptState& s, int B, int R, int cap, hipStream_t stream) {
    const dim3 ln_grid((R + 3) / 4);
    // More rows than a step can have (a prefill of more than 64 tokens): the four linears on the fp32 matrix-core GEMM (gemm_f32.hip, an exact k-ordered fp32
    // chain). Otherwise the register-streaming kernel, in ceil(R / 16) passes.
    const bool gemm = R > GPT_GEMM_ABOVE;
    auto dense = [&](const float* X, int K, const float* Wt, int N, float* C, const float* Res, int epi) {
        GemmArgs g;
        g.X = X; g.Tin = R; g.Cin = K; g.ldx = K; g.W = Wt; g.C = C; g.ldc = N; g.R = Res; g.ldr = N; g.M = R; g.N = N; g.K = K; g.epi = epi;
        return launch_gemm(g, stream);
    };
    for (int l = 0; l < h->n_layer; ++l) {
        const GptLayer& w = h->layers[l];
        float* kc = s.kc + s.layer_stride * l;
        float* vc = s.vc + s.layer_stride * l;
        hipLaunchKernelGGL(gpt_ln_kernel, ln_grid, dim3(256), 0, stream, s.x, w.ln1, (const int*)nullptr, s.xn, R);
        AT_CHECK_HIP(hipGetLastError());
        if (gemm) {
            if (int rc = dense(s.xn, E, w.qkv, 3 * E, s.q, nullptr, EPI_NONE)) return rc;
            hipLaunchKernelGGL(gpt_kv_scatter_kernel, dim3(R), dim3(E / 4), 0, stream, s.q, s.tok_row, s.tok_pos, s.done, kc, vc, cap);
            AT_CHECK_HIP(hipGetLastError());
        } else {
            LinArgs a{};
            a.A = s.xn; a.W = w.qkv; a.out = s.q; a.R = R; a.N = 3 * E;
            a.tok_row = s.tok_row; a.tok_pos = s.tok_pos; a.done = s.done; a.cap = cap; a.kc = kc; a.vc = vc;
            if (int rc = launch_linear<E, 192, LIN_QKV>(a, stream)) return rc;
        }
        hipLaunchKernelGGL(gpt_attn_kernel, dim3(R, NH), dim3(ATTN_THREADS), 0, stream, s.q, gemm ? 3 * E : E, kc, vc, s.tok_row, s.tok_pos, s.xn, cap);   // the context overwrites LN1's output
        AT_CHECK_HIP(hipGetLastError());
        if (gemm) {
            if (int rc = dense(s.xn, E, w.proj, E, s.x, s.x, EPI_NONE)) return rc;
        } else {
            LinArgs p{};
            p.A = s.xn; p.W = w.proj; p.out = s.x; p.R = R; p.N = E;
            if (int rc = launch_linear<E, 192, LIN_RESID>(p, stream)) return rc;
        }
        hipLaunchKernelGGL(gpt_ln_kernel, ln_grid, dim3(256), 0, stream, s.x, w.ln2, (const int*)nullptr, s.xn, R);
        AT_CHECK_HIP(hipGetLastError());
        if (gemm) {
            if (int rc = dense(s.xn, E, w.fc, FF, s.h, nullptr, EPI_GELU)) return rc;
            if (int rc = dense(s.h, FF, w.fc_proj, E, s.x, s.x, EPI_NONE)) return rc;
        } else {
            LinArgs f{};
            f.A = s.xn; f.W = w.fc; f.out = s.h; f.R = R; f.N = FF;
            if (int rc = launch_linear<E, 192, LIN_GELU>(f, stream)) return rc;
            LinArgs g{};
            g.A = s.h; g.W = w.fc_proj; g.out = s.x; g.R = R; g.N = E;
            if (int rc = launch_linear<FF, 256, LIN_RESID>(g, stream)) return rc;
        }
    }
    // the head, for the last token of every row only
    hipLaunchKernelGGL(gpt_ln_kernel, dim3((B + 3) / 4), dim3(256), 0, stream, s.x, h->ln_f, (const int*)s.last_row, s.xh, B);
    AT_CHECK_HIP(hipGetLastError());
    LinArgs o{};
    o.A = s.xh; o.W = h->wte; o.out = s.logits; o.R = B; o.N = h->vocab;
    return launch_linear<E, 192, LIN_NONE>(o, stream);
}

int run_pass(const at_gpt* h, const GptState& s, const int* prompts, int prompt_stride, int B, int R, int cap, int* status, hipStream_t stream) {
    hipLaunchKernelGGL(gpt_embed_kernel, dim3(R), dim3(E / 4), 0, stream, prompts, prompt_stride, h->wte, h->wpe, h->vocab, h->block, s.len, s.cur, s.last_row,
                       s.tok_row, s.tok_pos, s.x, status);
    AT_CHECK_HIP(hipGetLastError());
    return run_layers(h, s, B, R, cap, stream);
}

const GptHostTensor* staged(const at_gpt* h, const std::string& name) {
    auto it = h->staged.find(name);
    return it == h->staged.end() ? nullptr : &it->second;
}

int upload(at_gpt* h, const std::string& name, std::vector<int64_t> shape, const float** dst) {
    const GptHostTensor* t = staged(h, name);
    if (!t) { set_error("at_gpt_finalize: missing tensor " + name); return -1; }
    if (t->shape != shape) { set_error("at_gpt_finalize: tensor " + name + " has an unexpected shape"); return -1; }
    void* d = nullptr;
    AT_CHECK_HIP(hipMalloc(&d, t->data.size() * sizeof(float)));
    h->allocs.push_back(d);
    AT_CHECK_HIP(hipMemcpy(d, t->data.data(), t->data.size() * sizeof(float), hipMemcpyHostToDevice));
    *dst = static_cast<const float*>(d);
    return 0;
}

void release(at_gpt* h) {
    for (void* p : h->allocs) (void)hipFree(p);
    h->allocs.clear();
    if (h->flags_host) { (void)hipHostFree(h->flags_host); h->flags_host = nullptr; }
    h->layers.clear();
    h->wte = h->wpe = h->ln_f = nullptr;
}

}  // namespace

extern "C" {

at_gpt_t* at_gpt_create(int device_id) {
    int n = 0;
    if (!host_only_test() && (hipGetDeviceCount(&n) != hipSuccess || device_id < 0 || device_id >= n)) {
        set_error("at_gpt_create: no such HIP device " + std::to_string(device_id));
        return nullptr;
    }
    at_gpt* h = new at_gpt();
    h->device = device_id;
    return h;
}

int at_gpt_set_tensor(at_gpt_t* h, const char* name, const float* host_data, const int64_t* shape, int ndim) {
    AT_REQUIRE(h && name && host_data && shape && ndim >= 1 && ndim <= 4, "bad arguments");
    AT_REQUIRE(!h->finalized, "model already finalized");
    GptHostTensor t;
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

int at_gpt_finalize(at_gpt_t* h) {
    AT_REQUIRE(h != nullptr, "null handle");
    AT_REQUIRE(!h->finalized, "model already finalized");
    for (const auto& kv : h->staged)
        if (kv.first.size() > 5 && kv.first.compare(kv.first.size() - 5, 5, ".bias") == 0) {
            set_error("at_gpt_finalize: " + kv.first + ": the kernels implement the bias-free model only");
            return -1;
        }
    const GptHostTensor* wte = staged(h, "transformer.wte.weight");
    const GptHostTensor* wpe = staged(h, "transformer.wpe.weight");
    AT_REQUIRE(wte && wpe, "transformer.wte.weight and transformer.wpe.weight are needed");
    AT_REQUIRE(wte->shape.size() == 2 && wpe->shape.size() == 2 && wte->shape[1] == E && wpe->shape[1] == E, "n_embd must be 768 (12 heads of 64): what the kernels implement");
    const int64_t V = wte->shape[0], block = wpe->shape[0];
    AT_REQUIRE(V >= 64 && V % 64 == 0 && V <= GPT_MAX_VOCAB, "the vocabulary must be a multiple of 64, at most 65536");
    AT_REQUIRE(block >= 64 && block % 64 == 0 && block <= GPT_MAX_BLOCK, "the block size must be a multiple of 64, at most 1024");
    int n_layer = 0;
    while (staged(h, "transformer.h." + std::to_string(n_layer) + ".ln_1.weight")) ++n_layer;
    AT_REQUIRE(n_layer >= 1 && n_layer <= GPT_MAX_LAYERS, "1 to 48 layers (transformer.h.<i>.ln_1.weight, ...)");
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    h->vocab = (int)V;
    h->block = (int)block;
    h->n_layer = n_layer;
    h->layers.resize(n_layer);
    int rc = upload(h, "transformer.wte.weight", {V, E}, &h->wte);
    if (!rc) rc = upload(h, "transformer.wpe.weight", {block, E}, &h->wpe);
    if (!rc) rc = upload(h, "transformer.ln_f.weight", {E}, &h->ln_f);
    for (int l = 0; l < n_layer && !rc; ++l) {
        const std::string p = "transformer.h." + std::to_string(l);
        GptLayer& w = h->layers[l];
        rc = upload(h, p + ".ln_1.weight", {E}, &w.ln1);
        if (!rc) rc = upload(h, p + ".attn.c_attn.weight", {3 * E, E}, &w.qkv);
        if (!rc) rc = upload(h, p + ".attn.c_proj.weight", {E, E}, &w.proj);
        if (!rc) rc = upload(h, p + ".ln_2.weight", {E}, &w.ln2);
        if (!rc) rc = upload(h, p + ".mlp.c_fc.weight", {FF, E}, &w.fc);
        if (!rc) rc = upload(h, p + ".mlp.c_proj.weight", {E, FF}, &w.fc_proj);
    }
    if (!rc && hipHostMalloc((void**)&h->flags_host, GPT_MAX_B * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) {
        set_error("at_gpt_finalize: hipHostMalloc failed");
        rc = -2;
    }
    if (rc) { release(h); return rc; }
    h->staged.clear();
    h->finalized = true;
    return 0;
}

void at_gpt_destroy(at_gpt_t* h) {
    if (!h) return;
    {
        DeviceGuard guard(h->device);
        release(h);
    }
    delete h;
}

int at_gpt_num_layers(const at_gpt_t* h) { return h && h->finalized ? h->n_layer : 0; }
int at_gpt_vocab(const at_gpt_t* h) { return h && h->finalized ? h->vocab : 0; }
int at_gpt_block_size(const at_gpt_t* h) { return h && h->finalized ? h->block : 0; }

size_t at_gpt_state_bytes(const at_gpt_t* h, int B, int max_len) {
    if (!(h && h->finalized)) { set_error("at_gpt_state_bytes: the model is not finalized"); return 0; }
    if (!(B >= 1 && B <= GPT_MAX_B)) { set_error("at_gpt_state_bytes: B must be 1 to 64"); return 0; }
    if (!(max_len >= 1 && max_len <= h->block)) { set_error("at_gpt_state_bytes: max_len must be 1 to the model's block size"); return 0; }
    return carve_state(nullptr, B, max_len, h->vocab, h->n_layer).bytes;
}

int at_gpt_generate(at_gpt_t* h, const int32_t* prompts_dev, int prompt_stride, const int32_t* prompt_len, int B, int max_new, float temperature, int top_k,
                    int stop_token, const float* uniforms_dev, const int32_t* allow, int32_t* out_ids_dev, int32_t* out_len_dev, int32_t* finish_dev,
                    float* logits_out_dev, void* state_dev, size_t state_bytes, int max_len, at_stream_t stream_, int32_t* status_dev) {
    AT_REQUIRE(h && h->finalized, "the model is not finalized");
    AT_REQUIRE(B >= 1 && B <= GPT_MAX_B, "B must be 1 to 64");
    AT_REQUIRE(prompts_dev && prompt_len && uniforms_dev && out_ids_dev && out_len_dev && finish_dev, "null pointer");
    AT_REQUIRE(state_dev != nullptr, "null state");
    AT_REQUIRE(prompt_stride >= 1 && prompt_stride <= h->block, "prompt_stride must be 1 to the model's block size");
    AT_REQUIRE(max_new >= 1 && max_new <= GPT_MAX_BLOCK, "max_new must be 1 to 1024");
    if (int rc = check_sampling(temperature, top_k)) return rc;
    AT_REQUIRE(stop_token < h->vocab, "stop_token is not in the vocabulary (negative: none)");
    PromptLens pl{};
    int longest = 0;
    for (int b = 0; b < B; ++b) {
        if (prompt_len[b] > h->block) { set_error("at_gpt_generate: prompt of row " + std::to_string(b) + " is longer than the model's block size"); return -1; }
        if (prompt_len[b] < 1 || prompt_len[b] > prompt_stride) { set_error("at_gpt_generate: prompt_len of row " + std::to_string(b) + " must be 1 to prompt_stride"); return -1; }
        pl.off[b + 1] = pl.off[b] + prompt_len[b];
        longest = prompt_len[b] > longest ? prompt_len[b] : longest;
    }
    const int need_len = longest + max_new < h->block ? longest + max_new : h->block;
    AT_REQUIRE(max_len >= need_len && max_len <= h->block, "max_len must hold the longest prompt and max_new (or the block size) and not exceed the block size");
    Allow al[2];
    if (int rc = check_allow(allow, h->vocab, &al[0])) return rc;
    if (int rc = check_allow(allow ? allow + 4 : nullptr, h->vocab, &al[1])) return rc;
    const GptState s = carve_state(state_dev, B, max_len, h->vocab, h->n_layer);
    AT_REQUIRE(state_bytes >= s.bytes, "state too small: at_gpt_state_bytes(h, B, max_len)");
    // ---- nothing above touched the device
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    hipStream_t stream = (hipStream_t)stream_;
    const int R = pl.off[B];
    hipLaunchKernelGGL(gpt_init_kernel, dim3((R + 255) / 256), dim3(256), 0, stream, pl, B, R, h->block, s.len, s.done, s.cur, s.last_row, s.tok_row, s.tok_pos,
                       out_len_dev, finish_dev);
    AT_CHECK_HIP(hipGetLastError());
    if (int rc = run_pass(h, s, prompts_dev, prompt_stride, B, R, max_len, status_dev, stream)) return rc;
    SampleArgs sa{};
    sa.logits = s.logits; sa.V = h->vocab; sa.top_k = top_k; sa.temperature = temperature; sa.uniforms = uniforms_dev; sa.u_stride = max_new;
    sa.len = s.len; sa.done = s.done; sa.cur = s.cur; sa.out_ids = out_ids_dev; sa.out_len = out_len_dev; sa.finish = finish_dev;
    sa.logits_out = logits_out_dev; sa.max_new = max_new; sa.stop_token = stop_token; sa.block = h->block; sa.out_stride = max_new;
    for (int step = 0; step < max_new; ++step) {
        if (step > 0)
            if (int rc = run_pass(h, s, nullptr, 0, B, B, max_len, status_dev, stream)) return rc;
        sa.step = step;
        sa.allow = al[step & 1];
        hipLaunchKernelGGL(gpt_sample_kernel, dim3(B), dim3(SAMPLE_THREADS), 0, stream, sa);
        AT_CHECK_HIP(hipGetLastError());
        if ((step + 1) % GPT_CHECK_EVERY == 0 && step + 1 < max_new) {   // the host's only look at the device during the call
            AT_CHECK_HIP(hipMemcpyAsync(h->flags_host, s.done, B * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
            AT_CHECK_HIP(hipStreamSynchronize(stream));
            bool all = true;
            for (int b = 0; b < B; ++b) all = all && h->flags_host[b] != GPT_RUNNING;
            if (all) break;
        }
    }
    return 0;
}

int at_gpt_long_num_windows(int N, int S, int H) {
    if (!(S >= 2 && S % 2 == 0 && H >= 2 && H % 2 == 0 && H <= S && N >= 1 && N <= GPT_MAX_SOURCE)) {
        set_error("at_gpt_long_num_windows: S and H must be even with 2 <= H <= S, N 1 to 65536");
        return 0;
    }
    return gpt_long_windows(N, S, H);
}

size_t at_gpt_long_state_bytes(const at_gpt_t* h, int B, int max_len) {
    if (!(h && h->finalized)) { set_error("at_gpt_long_state_bytes: the model is not finalized"); return 0; }
    if (!(B >= 1 && B <= GPT_MAX_B)) { set_error("at_gpt_long_state_bytes: B must be 1 to 64"); return 0; }
    if (!(max_len >= 1 && max_len <= h->block)) { set_error("at_gpt_long_state_bytes: max_len must be 1 to the model's block size"); return 0; }
    return carve_long_state(nullptr, B, max_len, h->vocab, h->n_layer).bytes;
}

int at_gpt_generate_long(at_gpt_t* h, const int32_t* src_dev, int src_stride, const int32_t* src_len, int B, int S, int H, int r, int semantic_offset,
                         int semantic_vocab, int infer_token, int acoustic_offset, int codebook_size, int stop_token, int max_new, float temperature, int top_k,
                         const float* uniforms_dev, int u_stride, int32_t* out_ids_dev, int out_stride, int32_t* out_len_dev, int32_t* finish_dev,
                         float* logits_out_dev, void* state_dev, size_t state_bytes, int max_len, at_stream_t stream_, int32_t* status_dev) {
    AT_REQUIRE(h && h->finalized, "the model is not finalized");
    AT_REQUIRE(B >= 1 && B <= GPT_MAX_B, "B must be 1 to 64");
    AT_REQUIRE(src_dev && src_len && uniforms_dev && out_ids_dev && out_len_dev && finish_dev, "null pointer");
    AT_REQUIRE(state_dev != nullptr, "null state");
    const int V = h->vocab, block = h->block;
    LongRules q{};
    if (int rc = check_long_rules(h, S, H, r, src_stride, semantic_offset, semantic_vocab, infer_token, acoustic_offset, codebook_size, stop_token, max_new,
                                  temperature, top_k, &q))
        return rc;
    // ---- the schedule: rows in descending order of their window counts, so that the rows of pass k are the first Bk of them
    int n_win[GPT_MAX_B], order[GPT_MAX_B];
    int n_max = 0, need_len = 0;
    int64_t need_stride = 0;
    const int carry = r * (S - H);
    for (int b = 0; b < B; ++b) {
        if (src_len[b] < 1 || src_len[b] > src_stride || src_len[b] > GPT_MAX_SOURCE) {
            set_error("at_gpt_generate_long: src_len of row " + std::to_string(b) + " must be 1 to min(src_stride, 65536)");
            return -1;
        }
        const int n = gpt_long_windows(src_len[b], S, H);
        n_win[b] = n;
        n_max = n > n_max ? n : n_max;
        const int P = src_len[b] - (n - 1) * H + 1 + (n > 1 ? carry : 0);   // the final window's prompt
        const int budget = max_new < block - P ? max_new : block - P;
        const int64_t end = (n > 1 ? (int64_t)r * (n - 1) * H + carry : 0) + budget;
        need_stride = end > need_stride ? end : need_stride;
        need_len = P + budget > need_len ? P + budget : need_len;
        if (n > 1 && S + 1 + r * S > need_len) need_len = S + 1 + r * S;
        int at = b;
        while (at > 0 && n_win[order[at - 1]] < n) { order[at] = order[at - 1]; --at; }
        order[at] = b;
    }
    AT_REQUIRE(out_stride >= need_stride && u_stride >= need_stride, "out_stride and u_stride must hold the longest row's stream");
    AT_REQUIRE(max_len >= need_len && max_len <= block, "max_len must hold the longest window with its new ids and not exceed the block size");
    const LongState ls = carve_long_state(state_dev, B, max_len, V, h->n_layer);
    const GptState& s = ls.g;
    AT_REQUIRE(state_bytes >= ls.bytes, "state too small: at_gpt_long_state_bytes(h, B, max_len)");
    // ---- nothing above touched the device
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    hipStream_t stream = (hipStream_t)stream_;
    SampleArgs sa{};
    sa.logits = s.logits; sa.V = V; sa.top_k = top_k; sa.temperature = temperature; sa.uniforms = uniforms_dev; sa.u_stride = u_stride;
    sa.len = s.len; sa.done = s.done; sa.cur = s.cur; sa.out_ids = out_ids_dev; sa.out_len = out_len_dev; sa.finish = finish_dev;
    sa.logits_out = logits_out_dev; sa.max_new = max_new; sa.stop_token = -1; sa.block = block; sa.out_stride = out_stride; sa.rows = ls.rows;
    for (int k = 0; k < n_max; ++k) {
        LongPass p{};
        int Bk = 0, steps = 0, mid_steps = 0;
        while (Bk < B && n_win[order[Bk]] > k) {
            const int b = order[Bk];
            const bool last = k == n_win[b] - 1;
            const int n_src = last ? src_len[b] - k * H : S, P = n_src + 1 + (k > 0 ? carry : 0);
            const int budget = last ? (max_new < block - P ? max_new : block - P) : r * S - (k > 0 ? carry : 0);
            p.off[Bk + 1] = p.off[Bk] + P;
            p.row[Bk] = b;
            if (last) p.final_mask |= 1ull << Bk;
            else mid_steps = budget > mid_steps ? budget : mid_steps;
            steps = budget > steps ? budget : steps;
            ++Bk;
        }
        const int R = p.off[Bk];
        q.k = k;
        hipLaunchKernelGGL(gpt_window_kernel, dim3(((R > Bk ? R : Bk) + 255) / 256), dim3(256), 0, stream, p, q, Bk, R, src_dev, src_stride, out_ids_dev, out_stride,
                           ls.prompts, max_len, s.len, s.done, s.cur, s.last_row, s.tok_row, s.tok_pos, ls.rows, out_len_dev, finish_dev, status_dev);
        AT_CHECK_HIP(hipGetLastError());
        if (int rc = run_pass(h, s, ls.prompts, max_len, Bk, R, max_len, status_dev, stream)) return rc;
        for (int step = 0; step < steps; ++step) {
            if (step > 0)
                if (int rc = run_pass(h, s, nullptr, 0, Bk, Bk, max_len, status_dev, stream)) return rc;
            sa.step = step;
            hipLaunchKernelGGL(gpt_sample_kernel, dim3(Bk), dim3(SAMPLE_THREADS), 0, stream, sa);
            AT_CHECK_HIP(hipGetLastError());
            // the host's only look at the device; a non-final window never ends early, so there is nothing to see before the last of them is complete
            if ((step + 1) % GPT_CHECK_EVERY == 0 && step + 1 < steps && step + 1 >= mid_steps) {
                AT_CHECK_HIP(hipMemcpyAsync(h->flags_host, s.done, Bk * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
                AT_CHECK_HIP(hipStreamSynchronize(stream));
                bool all = true;
                for (int j = 0; j < Bk; ++j) all = all && h->flags_host[j] != GPT_RUNNING;
                if (all) break;
            }
        }
    }
    return 0;
}

size_t at_gpt_queue_state_bytes(const at_gpt_t* h, int slots, int max_len, int tick_tokens) {
    if (!(h && h->finalized)) { set_error("at_gpt_queue_state_bytes: the model is not finalized"); return 0; }
    if (!(slots >= 1 && slots <= GPT_MAX_B)) { set_error("at_gpt_queue_state_bytes: slots must be 1 to 64"); return 0; }
    if (!(max_len >= 1 && max_len <= h->block)) { set_error("at_gpt_queue_state_bytes: max_len must be 1 to the model's block size"); return 0; }
    if (!(tick_tokens >= slots + max_len && tick_tokens <= GPT_MAX_TICK_TOKENS)) {
        set_error("at_gpt_queue_state_bytes: tick_tokens must be slots + max_len to " + std::to_string(GPT_MAX_TICK_TOKENS));
        return 0;
    }
    return carve_queue_state(nullptr, slots, max_len, tick_tokens, h->vocab, h->n_layer).bytes;
}

int at_gpt_generate_queue(at_gpt_t* h, const int32_t* src_dev, int src_stride, const int32_t* src_len, int n_src, int S, int H, int r, int semantic_offset,
                          int semantic_vocab, int infer_token, int acoustic_offset, int codebook_size, int stop_token, int max_new, float temperature, int top_k,
                          const float* uniforms_dev, int u_stride, int32_t* out_ids_dev, int out_stride, int32_t* out_len_dev, int32_t* finish_dev,
                          float* logits_out_dev, void* state_dev, size_t state_bytes, int max_len, int slots, int tick_tokens, int32_t* trace, int trace_cap,
                          int32_t* n_ticks, int32_t* placement, at_stream_t stream_, int32_t* status_dev) {
    AT_REQUIRE(h && h->finalized, "the model is not finalized");
    AT_REQUIRE(n_src >= 1 && n_src <= GPT_MAX_QUEUE, "n_src must be 1 to 4096");
    AT_REQUIRE(slots >= 1 && slots <= GPT_MAX_B, "slots must be 1 to 64");
    AT_REQUIRE(src_dev && src_len && uniforms_dev && out_ids_dev && out_len_dev && finish_dev, "null pointer");
    AT_REQUIRE(state_dev != nullptr, "null state");
    AT_REQUIRE(trace_cap >= 0 && (trace != nullptr || trace_cap == 0), "trace_cap must be 0 without a trace and never negative");
    const int V = h->vocab, block = h->block;
    LongRules q{};
    if (int rc = check_long_rules(h, S, H, r, src_stride, semantic_offset, semantic_vocab, infer_token, acoustic_offset, codebook_size, stop_token, max_new,
                                  temperature, top_k, &q))
        return rc;
    // ---- the schedule's extent: every source's stream and its longest window
    const GptQueueSchedule geometry(src_len, n_src, S, H, r, max_new, block, slots, tick_tokens);
    int need_len = 0;
    int64_t need_stride = 0;
    for (int i = 0; i < n_src; ++i) {
        if (src_len[i] < 1 || src_len[i] > src_stride || src_len[i] > GPT_MAX_SOURCE) {
            set_error("at_gpt_generate_queue: src_len of source " + std::to_string(i) + " must be 1 to min(src_stride, 65536)");
            return -1;
        }
        const int n = gpt_long_windows(src_len[i], S, H);
        int n_ids, P, budget;
        bool fin;
        geometry.window(src_len[i], n - 1, &n_ids, &P, &budget, &fin);
        const int64_t end = (n > 1 ? (int64_t)r * (n - 1) * H + r * (S - H) : 0) + budget;
        need_stride = end > need_stride ? end : need_stride;
        need_len = P + budget > need_len ? P + budget : need_len;
        if (n > 1 && S + 1 + r * S > need_len) need_len = S + 1 + r * S;
    }
    AT_REQUIRE(out_stride >= need_stride && u_stride >= need_stride, "out_stride and u_stride must hold the longest source's stream");
    AT_REQUIRE(max_len >= need_len && max_len <= block, "max_len must hold the longest window with its new ids and not exceed the block size");
    AT_REQUIRE(tick_tokens >= slots + max_len && tick_tokens <= GPT_MAX_TICK_TOKENS, "tick_tokens must be at least slots + max_len (one window always fits) and at most 65600");
    const QueueState qs = carve_queue_state(state_dev, slots, max_len, tick_tokens, V, h->n_layer);
    const GptState& s = qs.g;
    AT_REQUIRE(state_bytes >= qs.bytes, "state too small: at_gpt_queue_state_bytes(h, slots, max_len, tick_tokens)");
    // ---- nothing above touched the device
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    hipStream_t stream = (hipStream_t)stream_;
    SampleArgs sa{};
    sa.logits = s.logits; sa.V = V; sa.top_k = top_k; sa.temperature = temperature; sa.uniforms = uniforms_dev; sa.u_stride = u_stride;
    sa.len = s.len; sa.done = s.done; sa.cur = s.cur; sa.out_ids = out_ids_dev; sa.out_len = out_len_dev; sa.finish = finish_dev;
    sa.logits_out = logits_out_dev; sa.max_new = max_new; sa.stop_token = -1; sa.block = block; sa.out_stride = out_stride; sa.rows = qs.rows;
    sa.step_ctr = qs.step_ctr; sa.samp_slot = qs.samp_slot;
    GptQueueSchedule schedule(src_len, n_src, S, H, r, max_new, block, slots, tick_tokens);
    GptQueueTick t;
    while (schedule.next(&t)) {
        TickPlan p{};
        p.n_step = t.n_step; p.n_start = t.n_start; p.R = t.tokens();
        for (int i = 0; i < t.n_step; ++i) p.step_slot[i] = (unsigned char)t.step_slot[i];
        p.off[0] = t.n_step;
        for (int j = 0; j < t.n_start; ++j) {
            const GptQueueStart& w = t.start[j];
            p.off[j + 1] = p.off[j] + w.P;
            p.src[j] = w.src; p.k[j] = w.k; p.slot[j] = (unsigned char)w.slot;
            if (w.final_window) p.final_mask |= 1ull << j;
        }
        const int ns = t.n_step + t.n_start;   // sampling rows: every slot with a token in the tick
        hipLaunchKernelGGL(gpt_tick_kernel, dim3((p.R + 255) / 256), dim3(256), 0, stream, p, q, src_dev, src_stride, out_ids_dev, out_stride, s.len, s.done, s.cur,
                           qs.step_ctr, s.last_row, qs.samp_slot, s.tok_row, s.tok_pos, qs.tok_id, qs.rows, out_len_dev, finish_dev, status_dev);
        AT_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(gpt_embed_list_kernel, dim3(p.R), dim3(E / 4), 0, stream, qs.tok_id, s.tok_pos, h->wte, h->wpe, V, block, s.x, status_dev);
        AT_CHECK_HIP(hipGetLastError());
        if (int rc = run_layers(h, s, ns, p.R, max_len, stream)) return rc;
        hipLaunchKernelGGL(gpt_sample_kernel, dim3(ns), dim3(SAMPLE_THREADS), 0, stream, sa);
        AT_CHECK_HIP(hipGetLastError());
        const int at = schedule.ticks() - 1;
        if (at < trace_cap) {   // a trace too small loses its tail, the run goes on
            int32_t* row = trace + 4 * (size_t)at;
            row[0] = t.n_step; row[1] = t.n_start; row[2] = t.prefill_tokens; row[3] = t.route();
        }
        if (t.poll) {   // the host's only look at the device: some slot is in a final window, and when that ends only the device knows
            AT_CHECK_HIP(hipMemcpyAsync(h->flags_host, s.done, slots * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
            AT_CHECK_HIP(hipStreamSynchronize(stream));
            schedule.seen(h->flags_host);
        }
    }
    if (n_ticks) *n_ticks = schedule.ticks();
    if (placement) std::memcpy(placement, schedule.placement().data(), (size_t)n_src * 3 * sizeof(int32_t));
    return 0;
}

int at_op_topk_sample(const float* logits_dev, int B, int V, float temperature, int top_k, const float* uniforms_dev, const int32_t* allow, int32_t* out_dev,
                      at_stream_t stream) {
    AT_REQUIRE(logits_dev && uniforms_dev && out_dev, "null pointer");
    AT_REQUIRE(B >= 1 && B <= 65535, "B must be 1 to 65535");
    AT_REQUIRE(V >= 1 && V <= GPT_MAX_VOCAB, "V must be 1 to 65536");
    if (int rc = check_sampling(temperature, top_k)) return rc;
    SampleArgs sa{};
    if (int rc = check_allow(allow, V, &sa.allow)) return rc;
    sa.logits = logits_dev; sa.V = V; sa.top_k = top_k; sa.temperature = temperature; sa.uniforms = uniforms_dev; sa.u_stride = 1; sa.step = 0;
    sa.out = out_dev;
    hipLaunchKernelGGL(gpt_sample_kernel, dim3(B), dim3(SAMPLE_THREADS), 0, (hipStream_t)stream, sa);
    AT_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
