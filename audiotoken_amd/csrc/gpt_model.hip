// The model pass and the sampler of the semantic-to-acoustic GPT: a nanoGPT-style model (pre-LN, gain-only LayerNorm, bias-free linears,
// 12 heads of 64, learned positions, tied head) over a token list, with a KV cache. gpt.hip holds the handle and the entry points that drive it. Kernels, all fp32:
//   gpt_embed_kernel    token + position rows: the list's prompt tokens as the begin kernel (gpt.hip) wrote them, its step tokens resolved here
//   gpt_ln_kernel       LayerNorm (two-pass, one wave per row), optionally gathering the rows the head needs
//   gpt_linear_kernel   out[R][N] = A[R][K] . W[N][K]^T for few rows: weights straight from global memory to registers in 16-byte loads, 16 activation rows per
//                       pass, fp32 FMA, a fixed-order reduction; epilogues: none / GELU / residual add / q + K,V scattered into the cache
//                       A pass of more than 64 tokens runs its four linears per layer on the fp32 matrix-core GEMM instead (gemm_f32.hip, launch_gemm).
//   gpt_attn_kernel     causal attention of one query over its row's cache, one workgroup of 4 waves per (token, head)
//   gpt_sample_kernel   temperature, allow ranges, exact top-k threshold (radix select), softmax weights and the inverse-CDF draw, one workgroup per row
// Nothing here adds floats atomically: every sum has one order, so a call repeated gives the same tokens.
#include <cmath>

#include "../../include/audiotoken_hip.h"
#include "gpt_kernels.h"

using namespace at;

namespace {

constexpr int E = GPT_EMBD, HD = GPT_HEAD_DIM, NH = GPT_HEADS, FF = GPT_FF;
constexpr int LIN_COLS = 4;            // output columns of one workgroup of the linear kernel
constexpr int SAMPLE_THREADS = 1024;

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

// x[i] = wte[id] + wpe[pos] for token i of the pass's list. A step token (i < st.n) is cache row st.slot[i]'s last sampled id at position len - 1; the kernel
// writes its entry of the token list and of the sampling list itself. A prompt token is what the begin kernel wrote. An id outside [0, V) is clamped and
// reported in bit 0 of *status: a caller's raw prompt id (every other id is the model's own, or was clamped when the prompt was written).
__global__ __launch_bounds__(E / 4) void gpt_embed_kernel(StepSlots st, const float* wte, const float* wpe, int V, int block, GptState s, int* status) {
    const int i = blockIdx.x, t = threadIdx.x;
    int p, id;
    if (i < st.n) {
        const int slot = st.slot[i];
        p = min(max(s.len[slot] - 1, 0), block - 1);
        id = s.cur[slot];
        if (t == 0) { s.tok_row[i] = slot; s.tok_pos[i] = p; s.last_row[i] = i; s.samp_slot[i] = slot; }
    } else {
        p = min(max(s.tok_pos[i], 0), block - 1);
        id = s.tok_id[i];
    }
    if (id < 0 || id >= V) {
        if (t == 0 && status) atomicOr(status, 1);
        id = min(max(id, 0), V - 1);
    }
    const float4 a = reinterpret_cast<const float4*>(wte + (size_t)id * E)[t];
    const float4 c = reinterpret_cast<const float4*>(wpe + (size_t)p * E)[t];
    reinterpret_cast<float4*>(s.x + (size_t)i * E)[t] = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w);
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

// ---- truncation: the pieces gpt_sample_kernel<true> adds between the radix select and the walk
constexpr int NUCLEUS_LIST = 1024;   // a top-k set of at most this many values is compacted into LDS and finished there
// the integer mass of one id: floor(p 2^40), p = expf(v - m) in [0, 1] (the product is exact: a power of two scales it)
__device__ __forceinline__ unsigned long long mass_of(float v, float m) { return (unsigned long long)(expf(v - m) * 1099511627776.0f); }
// an id stays in the nucleus iff the integer mass strictly above it is below this: ceil(top_p total), at least 1 (the maximum always stays)
__device__ __forceinline__ unsigned long long cut_mass(float top_p, unsigned long long total) {
    const unsigned long long t = (unsigned long long)ceil((double)top_p * (double)total);
    return t < 1 ? 1 : (t > total ? total : t);
}

// TRUNC = false is the sampler of 17 alone. TRUNC = true adds min_p, the nucleus and the op's kept / thresh outputs; its extra LDS exists in that instance only.
template <bool TRUNC>
__global__ __launch_bounds__(SAMPLE_THREADS) void gpt_sample_kernel(SampleArgs a) {
    __shared__ unsigned hist[256];
    __shared__ unsigned sel_prefix, sel_k;
    __shared__ float wave_part[SAMPLE_THREADS / 64];
    __shared__ int best_id, high_id;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the op alone: row blockIdx.x at step 0 from the call's allow set; generation: the cache row this sampling row belongs to, by its SampleRow at its own
    // step (every thread reads the counter here, thread 0 advances it after the last barrier)
    const bool generating = a.out == nullptr;
    const int b = generating ? a.samp_slot[blockIdx.x] : blockIdx.x;
    if (generating && a.done[b] != GPT_RUNNING) return;   // a finished row writes nothing more (uniform over the workgroup)
    const int V = a.V;
    const float* z = a.logits + (size_t)blockIdx.x * V;
    const int step = generating ? a.step_ctr[b] : 0;
    const SampleRow* pr = generating ? a.rows + b : nullptr;
    if (pr && step >= pr->budget) return;
    // where the step's id, draw and logits live: the caller's row and the stream position
    const int orow = pr ? pr->out_row : b, pos = (pr ? pr->base : 0) + step, out_at = pos - (pr ? pr->out_org : 0), u_at = pos - (pr ? pr->u_org : 0);
    const Allow allow = pr ? pr->allow[step & 1] : a.allow;
    if (generating && a.logits_out) {
        float* dst = a.logits_out + ((size_t)orow * a.out_stride + out_at) * V;
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
    float thresh = key_value(sel_prefix);
    // ---- m = the largest kept value (the largest of all: it is always kept)
    mx = wave_max(mx);
    if (lane == 0) wave_part[wave] = mx;
    __syncthreads();
    float m = wave_part[0];
#pragma unroll
    for (int wv = 1; wv < SAMPLE_THREADS / 64; ++wv) m = fmaxf(m, wave_part[wv]);
    __syncthreads();
    if constexpr (TRUNC) {
        // ---- steps 3a and 3b on K = {zt >= thresh}: both are value thresholds, found as order keys (of v + 0, so that -0 and +0 are one value as they are
        // for >=). Every sum is of integers through integer atomics, so nothing depends on the order in which threads arrive.
        __shared__ unsigned long long mhist[256], list_q[NUCLEUS_LIST];
        __shared__ unsigned list_key[NUCLEUS_LIST];
        __shared__ unsigned long long nuc_above;
        __shared__ unsigned nuc_prefix, nuc_key, minp_key, n_list;
        __shared__ int n_kept;
        const bool nucleus = a.top_p < 1.0f, min_p = a.lmin > -INFINITY;
        const bool compact = nucleus && min(a.top_k, V) <= NUCLEUS_LIST;   // K has at least that many values; ties can still overflow the list
        if (tid == 0) { nuc_above = 0; nuc_prefix = 0; nuc_key = minp_key = 0xffffffffu; n_list = 0; n_kept = 0; }
        __syncthreads();
        if (compact || min_p) {   // one walk: the lowest value of K that passes min_p, and K's (key, mass) pairs into the list
            unsigned lo = 0xffffffffu;
            for (int i = tid; i < V; i += SAMPLE_THREADS) {
                const float v = tempered(z, i, a.temperature, allow);
                if (!(v >= thresh)) continue;
                const unsigned k = order_key(v + 0.0f);
                if (v - m >= a.lmin) lo = min(lo, k);
                if (compact) {
                    const unsigned at = atomicAdd(&n_list, 1u);
                    if (at < (unsigned)NUCLEUS_LIST) { list_key[at] = k; list_q[at] = mass_of(v, m); }
                }
            }
            if (min_p && lo != 0xffffffffu) atomicMin(&minp_key, lo);
            __syncthreads();
        }
        const unsigned n = n_list;   // uniform over the workgroup
        if (compact && n <= (unsigned)NUCLEUS_LIST) {
            // thread t owns list entry t: the mass of the entries strictly above it, and the total, in one loop over the list (LDS broadcast reads)
            const unsigned mine = tid < (int)n ? list_key[tid] : 0u;
            unsigned long long total = 0, above = 0;
            for (unsigned j = 0; j < n; ++j) {
                const unsigned long long q = list_q[j];
                total += q;
                if (list_key[j] > mine) above += q;
            }
            if (tid < (int)n && above < cut_mass(a.top_p, total)) atomicMin(&nuc_key, mine);
            __syncthreads();
        } else if (nucleus) {
            // the radix descent of the select above, on masses: in every pass the one bin with (mass above it) < cut <= (mass above it) + (its own)
            unsigned long long cut = 0;
            for (int pass = 0; pass < 4; ++pass) {
                const int shift = 24 - 8 * pass;
                if (tid < 256) mhist[tid] = 0;
                __syncthreads();
                const unsigned prefix = nuc_prefix, mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
                const unsigned long long base = nuc_above;
                for (int i = tid; i < V; i += SAMPLE_THREADS) {
                    const float v = tempered(z, i, a.temperature, allow);
                    if (!(v >= thresh)) continue;
                    const unsigned k = order_key(v + 0.0f);
                    if ((k & mask) == prefix) atomicAdd(&mhist[(k >> shift) & 255u], mass_of(v, m));
                }
                __syncthreads();
                if (tid < 256) {
                    unsigned long long above = base;
                    for (int bin = 255; bin > tid; --bin) above += mhist[bin];
                    if (pass == 0) {   // the total is every bin of the first pass
                        unsigned long long total = above;
                        for (int bin = tid; bin >= 0; --bin) total += mhist[bin];
                        cut = cut_mass(a.top_p, total);
                    }
                    if (above < cut && cut <= above + mhist[tid]) {
                        nuc_above = above;
                        nuc_prefix = prefix | ((unsigned)tid << shift);
                        if (pass == 3) nuc_key = prefix | (unsigned)tid;
                    }
                }
                __syncthreads();
            }
        }
        unsigned final_key = order_key(thresh + 0.0f);
        if (minp_key != 0xffffffffu) final_key = max(final_key, minp_key);
        if (nuc_key != 0xffffffffu) final_key = max(final_key, nuc_key);
        thresh = key_value(final_key);
        if (a.kept_out) {   // the op alone: the size of the final set
            int c = 0;
            for (int i = tid; i < V; i += SAMPLE_THREADS) c += tempered(z, i, a.temperature, allow) >= thresh ? 1 : 0;
            if (c) atomicAdd(&n_kept, c);
            __syncthreads();
            if (tid == 0) a.kept_out[b] = n_kept;
        }
        if (a.thresh_out && tid == 0) a.thresh_out[b] = thresh;
    }
    // ---- S and the running sums in ascending id order. A wave owns a contiguous run of ids and walks it 64 at a time (coalesced): within a group the lanes'
    // weights are scanned (shuffle scan), the groups chain through a carry, the waves' totals are added in wave order. The first walk gives the waves' totals and S,
    // the second the running sums, its carry starting from the total of the waves before.
    const int per_wave = ((V + SAMPLE_THREADS / 64 - 1) / (SAMPLE_THREADS / 64) + 63) / 64 * 64, first = wave * per_wave;
    const float u = a.uniforms[(size_t)orow * a.u_stride + u_at];
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
    a.step_ctr[b] = step + 1;
    if (tok == pr->stop_token) {
        a.done[b] = a.finish[orow] = GPT_FINISH_STOP;
        return;
    }
    a.out_ids[(size_t)orow * a.out_stride + out_at] = tok;
    a.out_len[orow] = pos + 1;
    a.cur[b] = tok;
    const int total = a.len[b] + 1;
    a.len[b] = total;
    if (!pr->final_window) {   // the window's count is exact; the row is done for this pass, not for the call
        if (step + 1 >= pr->budget) a.done[b] = GPT_PASS_DONE;
        return;
    }
    if (step + 1 >= a.max_new) a.done[b] = a.finish[orow] = GPT_FINISH_MAX_NEW;
    else if (total >= a.block) a.done[b] = a.finish[orow] = GPT_FINISH_BLOCK;
}

// ---- one pass of the model ------------------------------------------------------------------------------------------------------------------
// The model over the R embedded tokens of s.x, each at (tok_row, tok_pos), then the head for the B tokens that s.last_row names: logits row j belongs to token last_row[j].
// Without with_head the pass ends after the last layer (the scorer, gpt_score.hip, applies the head to every scored position itself).
int run_layers(const at_gpt* h, const GptState& s, int B, int R, int cap, hipStream_t stream, bool with_head) {
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
    if (!with_head) return 0;
    // the head, for the last token of every row only; its B <= R input rows take the place of LN2's output, which the last layer has consumed
    hipLaunchKernelGGL(gpt_ln_kernel, dim3((B + 3) / 4), dim3(256), 0, stream, s.x, h->ln_f, (const int*)s.last_row, s.xn, B);
    AT_CHECK_HIP(hipGetLastError());
    LinArgs o{};
    o.A = s.xn; o.W = h->wte; o.out = s.logits; o.R = B; o.N = h->vocab;
    return launch_linear<E, 192, LIN_NONE>(o, stream);
}

}  // namespace

namespace at {

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

int gpt_forward(const at_gpt* h, const GptState& s, const StepSlots& steps, int ns, int R, int* status, hipStream_t stream, bool with_head) {
    hipLaunchKernelGGL(gpt_embed_kernel, dim3(R), dim3(E / 4), 0, stream, steps, h->wte, h->wpe, h->vocab, h->block, s, status);
    AT_CHECK_HIP(hipGetLastError());
    return run_layers(h, s, ns, R, s.cap, stream, with_head);
}

int gpt_final_ln(const at_gpt* h, const float* x, const int* gather, float* y, int n, hipStream_t stream) {
    hipLaunchKernelGGL(gpt_ln_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, x, h->ln_f, gather, y, n);
    AT_CHECK_HIP(hipGetLastError());
    return 0;
}

int check_truncation(float top_p, float min_p, float* lmin) {
    AT_REQUIRE(top_p > 0.0f && top_p <= 1.0f, "top_p must lie in (0, 1] (1: off) and not be NaN");
    AT_REQUIRE(min_p >= 0.0f && min_p < 1.0f, "min_p must lie in [0, 1) (0: off) and not be NaN");
    *lmin = min_p > 0.0f ? (float)std::log((double)min_p) : -INFINITY;
    return 0;
}

int gpt_sample(const SampleArgs& a, int rows, hipStream_t stream) {
    // both cuts off and nothing but the token asked for: the instance without truncation, the launch of 17
    if (a.top_p < 1.0f || a.lmin > -INFINITY || a.kept_out || a.thresh_out)
        hipLaunchKernelGGL(gpt_sample_kernel<true>, dim3(rows), dim3(SAMPLE_THREADS), 0, stream, a);
    else
        hipLaunchKernelGGL(gpt_sample_kernel<false>, dim3(rows), dim3(SAMPLE_THREADS), 0, stream, a);
    AT_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace at

extern "C" {

int at_op_topk_sample(const float* logits_dev, int B, int V, float temperature, int top_k, const float* uniforms_dev, const int32_t* allow, int32_t* out_dev,
                      at_stream_t stream) {
    AT_REQUIRE(logits_dev && uniforms_dev && out_dev, "null pointer");
    AT_REQUIRE(B >= 1 && B <= 65535, "B must be 1 to 65535");
    AT_REQUIRE(V >= 1 && V <= GPT_MAX_VOCAB, "V must be 1 to 65536");
    if (int rc = check_sampling(temperature, top_k)) return rc;
    SampleArgs sa{};
    if (int rc = check_allow(allow, V, &sa.allow)) return rc;
    sa.logits = logits_dev; sa.V = V; sa.top_k = top_k; sa.temperature = temperature; sa.uniforms = uniforms_dev; sa.u_stride = 1;
    sa.out = out_dev;
    return gpt_sample(sa, B, (hipStream_t)stream);
}

int at_op_nucleus_sample(const float* logits_dev, int B, int V, float temperature, int top_k, float top_p, float min_p, const float* uniforms_dev,
                         const int32_t* allow, int32_t* out_dev, int32_t* kept_out_dev, float* thresh_out_dev, at_stream_t stream) {
    AT_REQUIRE(logits_dev && uniforms_dev && out_dev, "null pointer");
    AT_REQUIRE(B >= 1 && B <= 65535, "B must be 1 to 65535");
    AT_REQUIRE(V >= 1 && V <= GPT_MAX_VOCAB, "V must be 1 to 65536");
    if (int rc = check_sampling(temperature, top_k)) return rc;
    SampleArgs sa{};
    if (int rc = check_truncation(top_p, min_p, &sa.lmin)) return rc;
    if (int rc = check_allow(allow, V, &sa.allow)) return rc;
    sa.logits = logits_dev; sa.V = V; sa.top_k = top_k; sa.temperature = temperature; sa.uniforms = uniforms_dev; sa.u_stride = 1;
    sa.top_p = top_p;
    sa.out = out_dev; sa.kept_out = kept_out_dev; sa.thresh_out = thresh_out_dev;
    return gpt_sample(sa, B, (hipStream_t)stream);
}

}  // extern "C"
