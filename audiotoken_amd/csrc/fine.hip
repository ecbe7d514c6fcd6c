// The semantic decoder's second stage: bark's non-causal "fine" transformer fills code books 3 to 8 of a [2][T] coarse row, window by window.
// The model: 8 embedding tables summed up to the code book being predicted, learned positions, pre-LN blocks (LayerNorm with gain and bias, linears with or
// without bias, E / 64 heads of 64, attention over the whole window without a mask, erf-GELU MLP), a final LayerNorm and 7 heads.
// The matrix products, the attention and the LayerNorm are the library's own fp32 launchers (launch_gemm, launch_relpos_attention with its arithmetic set to
// fp32, launch_layernorm). New here, all fp32:
//   fine_init_kernel     the work arrays [L][8] of the rows that enter a slot: a history's last frames, the coarse codes, 1024 everywhere else
//   fine_embed_kernel    x[t] = sum_{i <= c} wtes[i][cell[t][i]] + wpe[t], read straight from the work arrays at each row's window (no batch copy of the ids)
//   fine_gather_kernel   the rows the head needs (positions >= rel of every window of the pass), where a window has rel > 0
//   fine_sample_kernel   one wave per position over its 1024 logits: the argmax or the inverse-CDF draw, written straight into the work array
//   fine_finish_kernel   the T cells after the history of the rows that leave a slot, as [8][T]
// The stream and the stream pool share fine_pool_handover_kernel / fine_pool_emit_kernel / fine_pool_shift_kernel, which take
// their work by table: a stream of its own is the one-piece case.
// A call enqueues every window of every row without looking at the device: the host knows the schedule from the lengths. No float is added atomically.
// Both generators are one function (generate) and one loop (run_passes) over the passes of FineQueueSchedule (fine.h): at_fine_generate is
// the queue with a slot per row. A pass's six code books are run_codebooks, which the stream's windows use as well. The handle's plumbing
// and the state carver are model_handle.h's, shared with the GPT.
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

// max_hist: the longest history of the call (0 = none); a work array then holds min(H, max_hist) + max_T cells
FineState carve_state(void* base, int B, int max_T, int max_hist, int W, int E) {
    FineState s{};
    StateCarver c(base);
    const size_t R = (size_t)B * W;
    s.Lmax = fine_cells(max_T, W, fine_history(max_hist, W));
    s.work = c.take<int>((size_t)B * s.Lmax * FINE_CODES);
    s.ones = c.take<float>(R);
    s.x = c.take<float>(R * E);
    s.xn = c.take<float>(R * E);
    s.qkv = c.take<float>(R * 3 * E);
    s.h = c.take<float>(R * 4 * E);          // the MLP's hidden rows; before the head, the gathered rows
    s.logits = c.take<float>(R * FINE_VOCAB);
    s.bytes = c.off;
    return s;
}

// ---- the schedule of one pass, by value into the kernels ------------------------------------------------------------------------------------
// A pass may hold windows of different rows AND of different k (the window queue), so everything a kernel needs of a window travels with it.
struct FinePass {
    int n;                             // windows in the batch
    int cell0[FINE_MAX_B];             // the cell, in the state's work arrays, of the window's first position: the slot's base + start
    int draw[FINE_MAX_B];              // the window's draw cell: uniforms, logits_out and window_ids hold [6][W] per cell
    int rel[FINE_MAX_B];               // first buffer position that is predicted
    int head_off[FINE_MAX_B + 1];      // the window's predicted positions are head rows [head_off[j], head_off[j + 1])
};
// the rows that enter (fine_init_kernel) or leave (fine_finish_kernel) their slots in one pass: at most one per slot, so they go by value
struct FineRows {
    int n;
    int T[FINE_MAX_B];                 // frames of the row
    int cell0[FINE_MAX_B];             // the slot's base, in cells of the state's work arrays
    int stride[FINE_MAX_B];            // distance between the row's planes in coarse_dev / out_dev
    long long at[FINE_MAX_B];          // the row's first element in coarse_dev / out_dev
    int h[FINE_MAX_B];                 // history cells in front of the row's own; 0 = none
    long long hat[FINE_MAX_B];         // the first of the history's last h frames, in plane 0 of its table entry
};
static_assert(sizeof(FineRows) + 64 <= 4096, "fine_init_kernel's arguments must stay under the launch limit");
struct FineTables { const float* t[FINE_CODES]; };

__device__ __forceinline__ int slot_of(const FinePass& p, int r) {
    int j = 0;
    while (j + 1 < p.n && p.head_off[j + 1] <= r) ++j;
    return j;
}

// A row enters its slot: blockIdx.y = the row of the list, thread = cell. Every one of the row's max(h + T, W) cells is rewritten (the last h history
// frames in all 8 channels, the coarse codes, 1024 everywhere else), which is all a window of the row can read: whatever the slot's previous row left behind
// lies past them or is overwritten. A coarse code outside [0, 1024) is clamped and reported in bit 0 of *status, a history id in bit 1. ones: the
// attention's key mask, written by the call's first launch. hist: the call's history table, planes hstride apart (null and 0 where no row has one).
__global__ __launch_bounds__(256) void fine_init_kernel(FineRows rows, int W, const int* coarse, const int* hist, int hstride, int* work, float* ones, int* status) {
    const int j = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    const int T = rows.T[j], h = rows.h[j];
    if (t >= max(h + T, W)) return;
    if (ones && t < W) ones[(size_t)j * W + t] = 1.0f;
    int4* cell = reinterpret_cast<int4*>(work + ((size_t)rows.cell0[j] + t) * FINE_CODES);
    if (t < h) {
        const int* src = hist + rows.hat[j] + t;
        int id[FINE_CODES];
        bool bad = false;
#pragma unroll
        for (int ch = 0; ch < FINE_CODES; ++ch) {
            const int v = src[(size_t)ch * hstride];
            bad |= v < 0 || v >= FINE_VOCAB;
            id[ch] = min(max(v, 0), FINE_VOCAB - 1);
        }
        if (bad && status) atomicOr(status, 2);
        cell[0] = make_int4(id[0], id[1], id[2], id[3]);
        cell[1] = make_int4(id[4], id[5], id[6], id[7]);
        return;
    }
    int c0 = FINE_VOCAB, c1 = FINE_VOCAB;
    if (t < h + T) {
        const int* src = coarse + rows.at[j] + (t - h);
        c0 = src[0];
        c1 = src[(size_t)rows.stride[j]];
        if (c0 < 0 || c0 >= FINE_VOCAB || c1 < 0 || c1 >= FINE_VOCAB) {
            if (status) atomicOr(status, 1);
            c0 = min(max(c0, 0), FINE_VOCAB - 1);
            c1 = min(max(c1, 0), FINE_VOCAB - 1);
        }
    }
    cell[0] = make_int4(c0, c1, FINE_VOCAB, FINE_VOCAB);
    cell[1] = make_int4(FINE_VOCAB, FINE_VOCAB, FINE_VOCAB, FINE_VOCAB);
}

// Token i = (window i / W of the pass, buffer position i % W), E / 4 threads of 16 bytes each. Tables 0 to c in that order, the position last.
__global__ __launch_bounds__(256) void fine_embed_kernel(FinePass p, FineTables tab, const float* wpe, const int* work, int W, int E, int c, float* x) {
    const int i = blockIdx.x, tid = threadIdx.x;
    const int j = i / W, t = i % W;
    const int4* cell = reinterpret_cast<const int4*>(work + ((size_t)p.cell0[j] + t) * FINE_CODES);
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
    int W, c;
    int greedy;
    float temperature;
    const float* uniforms;    // [draw cells][6][W]
    int* work;
    float* logits_out;        // nullable [draw cells][6][W][1024]
    int* ids_out;             // nullable [draw cells][6][W]
};

// One wave per head row; lane l owns ids [16 l, 16 l + 16). The rule: zt = z / temperature, m = max zt, p = expf(zt - m); the running sum of
// id i is (the lanes before l, added by an inclusive shuffle scan of the lanes' totals) + (the lane's own ids up to i, added in id order); S is lane 63's
// inclusive total. The token is the lowest id whose running sum exceeds u * S, else the highest id with p > 0. greedy: the largest z, the lowest id among equals.
__global__ __launch_bounds__(64 * SAMPLE_WAVES) void fine_sample_kernel(FinePass p, FineSampleArgs a) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * SAMPLE_WAVES + (threadIdx.x >> 6);
    if (r >= a.total) return;   // uniform over the wave
    const int j = slot_of(p, r);
    const int t = p.rel[j] + (r - p.head_off[j]);
    const float4* zr = reinterpret_cast<const float4*>(a.logits + (size_t)r * FINE_VOCAB) + 4 * lane;
    float z[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v = zr[q];
        z[4 * q] = v.x; z[4 * q + 1] = v.y; z[4 * q + 2] = v.z; z[4 * q + 3] = v.w;
    }
    const size_t cell = ((size_t)p.draw[j] * FINE_PASSES + (a.c - FINE_COARSE)) * a.W + t;
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
        a.work[((size_t)p.cell0[j] + t) * FINE_CODES + a.c] = tok;
        if (a.ids_out) a.ids_out[cell] = tok;
    }
}

// A row leaves its slot: out[ch][t] = work[h + t][ch] for t < T (the history cells stay behind), at the row's place in out; the rest of out is left as it was
__global__ __launch_bounds__(256) void fine_finish_kernel(FineRows rows, const int* work, int* out) {
    const int j = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows.T[j]) return;
    const int4* cell = reinterpret_cast<const int4*>(work + ((size_t)rows.cell0[j] + rows.h[j] + t) * FINE_CODES);
    const int4 lo = cell[0], hi = cell[1];
    const int ids[FINE_CODES] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    int* dst = out + rows.at[j];
#pragma unroll
    for (int ch = 0; ch < FINE_CODES; ++ch) dst[(size_t)ch * rows.stride[j] + t] = ids[ch];
}

// ---- the forward of one pass for code book c: logits of the pass's head rows ----------------------------------------------------------------
int run_forward(const at_fine* h, const FineState& s, const FinePass& p, int c, hipStream_t stream) {
    const int W = h->block, E = h->embd, M = p.n * W, total = p.head_off[p.n];
    FineTables tab;
    for (int i = 0; i < FINE_CODES; ++i) tab.t[i] = h->wtes[i];
    hipLaunchKernelGGL(fine_embed_kernel, dim3(M), dim3(E / 4), 0, stream, p, tab, h->wpe, s.work, W, E, c, s.x);
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

// the six code books of one pass: for each the forward, then the sampler, which writes the code book's ids into the work arrays the next forward reads
int run_codebooks(const at_fine* h, const FineState& s, const FinePass& p, FineSampleArgs sa, hipStream_t stream) {
    sa.total = p.head_off[p.n];
    for (int cb = FINE_COARSE; cb < FINE_CODES; ++cb) {
        if (int rc = run_forward(h, s, p, cb, stream)) return rc;
        sa.c = cb;
        hipLaunchKernelGGL(fine_sample_kernel, dim3((sa.total + SAMPLE_WAVES - 1) / SAMPLE_WAVES), dim3(64 * SAMPLE_WAVES), 0, stream, p, sa);
        AT_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

// what a call fixes of the sampler's arguments; run_codebooks adds the pass's head rows and the code book
FineSampleArgs sample_args(const FineState& s, int W, int greedy, float temperature, const float* uniforms, float* logits_out, int32_t* ids_out) {
    FineSampleArgs sa{};
    sa.logits = s.logits; sa.W = W; sa.greedy = greedy; sa.temperature = greedy ? 1.0f : temperature;
    sa.uniforms = uniforms; sa.work = s.work; sa.logits_out = logits_out; sa.ids_out = ids_out;
    return sa;
}

int upload(at_fine* h, const std::string& name, std::vector<int64_t> shape, const float** dst) { return upload_staged(h, "at_fine_finalize", name, shape, dst); }

void release(at_fine* h) {
    free_allocs(h);
    h->layers.clear();
    for (auto& t : h->wtes) t = nullptr;
    for (auto& t : h->heads) t = nullptr;
    h->wpe = h->lnf_g = h->lnf_b = nullptr;
}

const char* const kLinears[4] = {".attn.c_attn", ".attn.c_proj", ".mlp.c_fc", ".mlp.c_proj"};

// ---- the passes of a call: the one loop behind at_fine_generate and at_fine_generate_queue ---------------------------------------------------------
// Where a row's data lies: its first element in coarse_dev and in out_dev, the distance between its planes, and the draw cell of its window 0.
struct FineRowMap {
    long long src, dst;
    int stride, draw0;
    int h = 0;             // history cells and where the first of them lies in the history table
    long long hat = 0;
};
struct FineCall {
    const int32_t* coarse;
    int32_t* out;
    float temperature;
    int greedy;
    const float* uniforms;
    float* logits_out;
    int32_t* window_ids;
    int32_t* status;
    int32_t* trace;        // the queue alone: nullable HOST arrays
    int trace_cap;
    int32_t *n_passes, *placement;
    const int32_t* hist;   // the history table; null where no row has a history
    int hstride;
};

int launch_rows(bool init, const FineRows& rows, int span, int W, const FineState& s, const FineCall& c, bool first, hipStream_t stream) {
    if (rows.n == 0) return 0;   // nothing enters or leaves in this pass
    const dim3 grid((unsigned)((span + 255) / 256), (unsigned)rows.n);
    if (init) hipLaunchKernelGGL(fine_init_kernel, grid, dim3(256), 0, stream, rows, W, c.coarse, c.hist, c.hstride, s.work, first ? s.ones : nullptr, c.status);
    else hipLaunchKernelGGL(fine_finish_kernel, grid, dim3(256), 0, stream, rows, s.work, c.out);
    AT_CHECK_HIP(hipGetLastError());
    return 0;
}

// lens and map are indexed by row; everything has been checked. Slot j's work array is cells [j Lmax, (j + 1) Lmax) of the state.
int run_passes(const at_fine* h, const FineState& s, const int32_t* lens, int n_rows, int slots, const FineRowMap* map, const FineCall& c, hipStream_t stream) {
    const int W = h->block;
    const FineSampleArgs sa = sample_args(s, W, c.greedy, c.temperature, c.uniforms, c.logits_out, c.window_ids);
    std::vector<int32_t> hcells((size_t)n_rows);
    for (int b = 0; b < n_rows; ++b) hcells[b] = map[b].h;
    FineQueueSchedule schedule(lens, n_rows, W, slots, hcells.data());
    FineQueuePass q;
    while (schedule.next(&q)) {
        const int at = schedule.passes() - 1;
        if (c.trace && at < c.trace_cap) {
            c.trace[3 * at] = q.n;
            c.trace[3 * at + 1] = q.n_admit;
            c.trace[3 * at + 2] = q.n_retire;
        }
        FinePass p{};
        FineRows in{}, outr{};
        int span_in = 0, span_out = 0;
        auto add = [&](FineRows& rows, int& span, int i, bool init) {
            const int b = q.row[i], j = rows.n++, T = lens[b];
            rows.T[j] = T;
            rows.cell0[j] = q.slot[i] * s.Lmax;
            rows.stride[j] = map[b].stride;
            rows.at[j] = init ? map[b].src : map[b].dst;
            rows.h[j] = map[b].h;
            rows.hat[j] = map[b].hat;
            const int cells = init ? fine_cells(T, W, map[b].h) : T;
            span = cells > span ? cells : span;
        };
        for (int a = 0; a < q.n_admit; ++a) add(in, span_in, q.admit[a], true);
        for (int a = 0; a < q.n_retire; ++a) add(outr, span_out, q.retire[a], false);
        for (int i = 0; i < q.n; ++i) {
            const int b = q.row[i], k = q.k[i];
            int start, fill;
            fine_window(k, lens[b], W, map[b].h, &start, &fill);
            p.cell0[i] = q.slot[i] * s.Lmax + start;
            p.draw[i] = map[b].draw0 + k;
            p.rel[i] = fill - start;
            p.head_off[i + 1] = p.head_off[i] + W - p.rel[i];
        }
        p.n = q.n;
        if (int rc = launch_rows(true, in, span_in, W, s, c, at == 0, stream)) return rc;
        if (int rc = run_codebooks(h, s, p, sa, stream)) return rc;
        if (int rc = launch_rows(false, outr, span_out, W, s, c, false, stream)) return rc;
    }
    if (c.n_passes) *c.n_passes = schedule.passes();
    if (c.placement) std::memcpy(c.placement, schedule.placement().data(), 3 * (size_t)n_rows * sizeof(int32_t));
    return 0;
}

}  // namespace

extern "C" {

at_fine_t* at_fine_create(int device_id) {
    if (!device_exists("at_fine_create", device_id)) return nullptr;
    at_fine* h = new at_fine();
    h->device = device_id;
    return h;
}

int at_fine_set_tensor(at_fine_t* h, const char* name, const float* host_data, const int64_t* shape, int ndim) {
    return stage_model_tensor(h, name, host_data, shape, ndim);
}

int at_fine_finalize(at_fine_t* h) {
    AT_REQUIRE(h != nullptr, "null handle");
    AT_REQUIRE(!h->finalized, "model already finalized");
    const HostTensor* wpe = staged_tensor(h, "transformer.wpe.weight");
    AT_REQUIRE(wpe && wpe->shape.size() == 2, "transformer.wpe.weight [block][n_embd] is needed");
    const int64_t W = wpe->shape[0], E = wpe->shape[1];
    AT_REQUIRE(E == 768 || E == 1024, "n_embd must be 768 or 1024 (heads of 64): what the kernels implement");
    AT_REQUIRE(W >= 128 && W % 128 == 0 && W <= FINE_MAX_BLOCK, "the block size must be a multiple of 128, from 128 to 1024");
    int n_layer = 0;
    while (staged_tensor(h, "transformer.h." + std::to_string(n_layer) + ".ln_1.weight")) ++n_layer;
    AT_REQUIRE(n_layer >= 1 && n_layer <= FINE_MAX_LAYERS, "1 to 48 layers (transformer.h.<i>.ln_1.weight, ...)");
    int biases = 0;
    for (int l = 0; l < n_layer; ++l)
        for (const char* lin : kLinears) biases += staged_tensor(h, "transformer.h." + std::to_string(l) + lin + ".bias") ? 1 : 0;
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

// the three size queries behind their two names each: `who` is the entry point the caller called
static int num_windows(const char* who, const at_fine_t* h, int T, int Th) {
    const std::string w(who);
    if (!(h && h->finalized)) { set_error(w + ": the model is not finalized"); return 0; }
    if (!(T >= 1 && T <= FINE_MAX_T)) { set_error(w + ": T must be 1 to 262144"); return 0; }
    if (!(Th >= 0 && Th <= FINE_MAX_T)) { set_error(w + ": the history must be 0 to 262144 frames"); return 0; }
    return fine_windows(T, h->block, fine_history(Th, h->block));
}
static size_t state_bytes_of(const char* who, const char* rows, const at_fine_t* h, int B, int max_T, int max_hist) {
    const std::string w(who);
    if (!(h && h->finalized)) { set_error(w + ": the model is not finalized"); return 0; }
    if (!(B >= 1 && B <= FINE_MAX_B)) { set_error(w + ": " + rows + " must be 1 to 64"); return 0; }
    if (!(max_T >= 1 && max_T <= FINE_MAX_T)) { set_error(w + ": max_T must be 1 to 262144"); return 0; }
    if (!(max_hist >= 0 && max_hist <= FINE_MAX_T)) { set_error(w + ": max_hist must be 0 to 262144"); return 0; }
    return carve_state(nullptr, B, max_T, max_hist, h->block, h->embd).bytes;
}

int at_fine_num_windows(const at_fine_t* h, int T) { return num_windows("at_fine_num_windows", h, T, 0); }
int at_fine_num_windows_hist(const at_fine_t* h, int T, int Th) { return num_windows("at_fine_num_windows_hist", h, T, Th); }
size_t at_fine_state_bytes(const at_fine_t* h, int B, int max_T) { return state_bytes_of("at_fine_state_bytes", "B", h, B, max_T, 0); }
size_t at_fine_state_bytes_hist(const at_fine_t* h, int B, int max_T, int max_hist) { return state_bytes_of("at_fine_state_bytes_hist", "B", h, B, max_T, max_hist); }
size_t at_fine_queue_state_bytes(const at_fine_t* h, int slots, int max_T) { return state_bytes_of("at_fine_queue_state_bytes", "slots", h, slots, max_T, 0); }
size_t at_fine_queue_state_bytes_hist(const at_fine_t* h, int slots, int max_T, int max_hist) {
    return state_bytes_of("at_fine_queue_state_bytes_hist", "slots", h, slots, max_T, max_hist);
}

}  // extern "C"

namespace {

// The history table of a call, as the caller gave it; n = 0 and null pointers where the call has none.
struct FineHistory {
    const int32_t* dev;     // device int32 [n][8][stride]
    int stride;
    const int32_t* lens;    // HOST [n]
    int n;
    const int32_t* of_row;  // HOST [rows]: the entry of each row, -1 for none
    int max_hist;
};

// Checks the table and writes every row's history cells and their place into map[b].h / map[b].hat. Touches no device.
int place_history(const char* who, const FineHistory& hi, int n_rows, int W, FineRowMap* map) {
    const std::string fn(who);
    auto fail = [&](const std::string& msg) { set_error(fn + ": " + msg); return -1; };
    if (hi.n < 0 || hi.n > FINE_MAX_QUEUE) return fail("n_hist must be 0 to 4096");
    if (hi.max_hist < 0 || hi.max_hist > FINE_MAX_T) return fail("max_hist must be 0 to 262144");
    if (hi.n == 0) {
        if (hi.of_row)
            for (int b = 0; b < n_rows; ++b)
                if (hi.of_row[b] != -1) return fail("the history of row " + std::to_string(b) + " must be -1: the table is empty");
        return 0;
    }
    if (!(hi.dev && hi.lens && hi.of_row)) return fail("null pointer: a history table needs its ids, its lengths and the history of every row");
    if (hi.stride < 1 || hi.stride > FINE_MAX_T) return fail("h_stride must be 1 to 262144");
    for (int i = 0; i < hi.n; ++i)
        if (hi.lens[i] < 1 || hi.lens[i] > hi.stride || hi.lens[i] > hi.max_hist)
            return fail("the length of history " + std::to_string(i) + " must be 1 to min(h_stride, max_hist)");
    for (int b = 0; b < n_rows; ++b) {
        const int i = hi.of_row[b];
        if (i < -1 || i >= hi.n) return fail("the history of row " + std::to_string(b) + " must be -1 or an entry of the table");
        if (i < 0) continue;
        map[b].h = fine_history(hi.lens[i], W);
        map[b].hat = (long long)i * FINE_CODES * hi.stride + (hi.lens[i] - map[b].h);
    }
    return 0;
}

// The one generator behind the four entry points. `c` holds the caller's arrays; the history table is added here. The lockstep form (queue = false) is the
// queue with a slot per row (slots = n_rows = B) over rows t_stride apart with n_max draw cells each; the queue's rows are packed and may be traced.
int generate(const char* who, bool queue, at_fine_t* h, FineCall c, const FineHistory& hi, const int32_t* lens, int n_rows, int slots, int t_stride, int n_max,
             void* state_dev, size_t state_bytes, int max_T, at_stream_t stream_) {
    AT_REQUIRE(h && h->finalized, "the model is not finalized");
    if (queue) {
        AT_REQUIRE(n_rows >= 1 && n_rows <= FINE_MAX_QUEUE, "n_rows must be 1 to 4096");
        AT_REQUIRE(slots >= 1 && slots <= FINE_MAX_B, "slots must be 1 to 64");
    } else {
        AT_REQUIRE(n_rows >= 1 && n_rows <= FINE_MAX_B, "B must be 1 to 64");
    }
    AT_REQUIRE(c.coarse && lens && c.out, "null pointer");
    AT_REQUIRE(c.greedy == 0 || c.greedy == 1, "greedy must be 0 or 1");
    AT_REQUIRE(c.greedy || c.uniforms, "null pointer: sampling needs the uniforms");
    AT_REQUIRE(c.greedy || (std::isfinite(c.temperature) && c.temperature > 0.0f), "temperature must be a positive finite number");
    AT_REQUIRE(state_dev != nullptr, "null state");
    AT_REQUIRE(max_T >= 1 && max_T <= FINE_MAX_T, "max_T must be 1 to 262144");
    if (queue) AT_REQUIRE(c.trace_cap >= 0 && (c.trace != nullptr || c.trace_cap == 0), "trace_cap must be 0 without a trace, and never negative");
    else AT_REQUIRE(t_stride >= 1 && t_stride <= FINE_MAX_T, "t_stride must be 1 to 262144");
    const int W = h->block;
    for (int b = 0; b < n_rows; ++b)
        if (lens[b] < 1 || lens[b] > max_T || (!queue && lens[b] > t_stride)) {
            set_error(std::string(who) + ": the length of row " + std::to_string(b) + " must be 1 to " + (queue ? "max_T" : "min(t_stride, max_T)"));
            return -1;
        }
    std::vector<FineRowMap> map((size_t)n_rows);
    if (int rc = place_history(who, hi, n_rows, W, map.data())) return rc;
    long long off = 0, woff = 0;   // the queue: frames and windows of the rows before
    int n_most = 0;
    for (int b = 0; b < n_rows; ++b) {
        const int n = fine_windows(lens[b], W, map[b].h);
        map[b].src = queue ? 2 * off : (long long)b * 2 * t_stride;
        map[b].dst = queue ? FINE_CODES * off : (long long)b * FINE_CODES * t_stride;
        map[b].stride = queue ? lens[b] : t_stride;
        map[b].draw0 = queue ? (int)woff : (int)((long long)b * n_max);
        off += lens[b];
        woff += n;
        n_most = n > n_most ? n : n_most;
    }
    if (queue) {
        AT_REQUIRE(woff <= INT32_MAX, "the rows' windows must number fewer than 2^31");
    } else {
        AT_REQUIRE(n_max >= n_most, "n_max must hold the windows of the longest row: at_fine_num_windows(h, T)");
        AT_REQUIRE((long long)n_rows * n_max <= INT32_MAX, "B * n_max must fit 31 bits");
    }
    const FineState s = carve_state(state_dev, slots, max_T, hi.max_hist, W, h->embd);
    AT_REQUIRE(state_bytes >= s.bytes, queue ? "state too small: at_fine_queue_state_bytes(h, slots, max_T)" : "state too small: at_fine_state_bytes(h, B, max_T)");
    // ---- nothing above touched the device
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    c.hist = hi.dev;
    c.hstride = hi.stride;
    return run_passes(h, s, lens, n_rows, slots, map.data(), c, (hipStream_t)stream_);
}

}  // namespace

extern "C" {

// The queue with slots = B: every row is admitted in pass 0, and pass k is window k of every row that has one, in row order.
int at_fine_generate(at_fine_t* h, const int32_t* coarse_dev, int t_stride, const int32_t* lens, int B, float temperature, int greedy,
                     const float* uniforms_dev, int n_max, int32_t* out_dev, float* logits_out_dev, int32_t* window_ids_dev, void* state_dev, size_t state_bytes,
                     int max_T, at_stream_t stream_, int32_t* status_dev) {
    return generate("at_fine_generate", false, h, FineCall{coarse_dev, out_dev, temperature, greedy, uniforms_dev, logits_out_dev, window_ids_dev, status_dev},
                    FineHistory{}, lens, B, B, t_stride, n_max, state_dev, state_bytes, max_T, stream_);
}

int at_fine_generate_hist(at_fine_t* h, const int32_t* coarse_dev, int t_stride, const int32_t* lens, int B, const int32_t* hist_dev, int h_stride,
                          const int32_t* hist_lens, int n_hist, const int32_t* hist_of_row, int max_hist, float temperature, int greedy,
                          const float* uniforms_dev, int n_max, int32_t* out_dev, float* logits_out_dev, int32_t* window_ids_dev, void* state_dev,
                          size_t state_bytes, int max_T, at_stream_t stream_, int32_t* status_dev) {
    return generate("at_fine_generate_hist", false, h, FineCall{coarse_dev, out_dev, temperature, greedy, uniforms_dev, logits_out_dev, window_ids_dev, status_dev},
                    FineHistory{hist_dev, h_stride, hist_lens, n_hist, hist_of_row, max_hist}, lens, B, B, t_stride, n_max, state_dev, state_bytes, max_T, stream_);
}

int at_fine_generate_queue(at_fine_t* h, const int32_t* coarse_dev, const int32_t* lens, int n_rows, float temperature, int greedy, const float* uniforms_dev,
                           int32_t* out_dev, float* logits_out_dev, int32_t* window_ids_dev, void* state_dev, size_t state_bytes, int max_T, int slots,
                           int32_t* trace, int trace_cap, int32_t* n_passes, int32_t* placement, at_stream_t stream_, int32_t* status_dev) {
    return generate("at_fine_generate_queue", true, h,
                    FineCall{coarse_dev, out_dev, temperature, greedy, uniforms_dev, logits_out_dev, window_ids_dev, status_dev, trace, trace_cap, n_passes, placement},
                    FineHistory{}, lens, n_rows, slots, 0, 0, state_dev, state_bytes, max_T, stream_);
}

int at_fine_generate_queue_hist(at_fine_t* h, const int32_t* coarse_dev, const int32_t* lens, int n_rows, const int32_t* hist_dev, int h_stride,
                                const int32_t* hist_lens, int n_hist, const int32_t* hist_of_row, int max_hist, float temperature, int greedy,
                                const float* uniforms_dev, int32_t* out_dev, float* logits_out_dev, int32_t* window_ids_dev, void* state_dev, size_t state_bytes,
                                int max_T, int slots, int32_t* trace, int trace_cap, int32_t* n_passes, int32_t* placement, at_stream_t stream_,
                                int32_t* status_dev) {
    return generate("at_fine_generate_queue_hist", true, h,
                    FineCall{coarse_dev, out_dev, temperature, greedy, uniforms_dev, logits_out_dev, window_ids_dev, status_dev, trace, trace_cap, n_passes, placement},
                    FineHistory{hist_dev, h_stride, hist_lens, n_hist, hist_of_row, max_hist}, lens, n_rows, slots, 0, 0, state_dev, state_bytes, max_T, stream_);
}

}  // extern "C"

// ---- the stream: one row whose coarse frames arrive in pushes -----------------------------------------------------------------
namespace {

constexpr int HANDOVER_BAD_ID = 4;   // status bit 2

// The stream's three kernels take their work by table, by value: up to FINE_POOL_CHUNK pieces a launch (blockIdx.y or blockIdx.x = the piece), as FineRows
// goes to the init kernel. A stream of its own is the one-piece case; a pool names a piece per stream of the call.
//   hand-over  The GPT's new ids into the work array: thread t of piece e = cell cell[e] + t. A frame's two ids are one 8-byte load (interleaved; code book 0
//              carries `offset`, code book 1 offset + codebook_size), its cell two 16-byte stores: channels 0 and 1, and 1024 ("nothing yet") in channels 2
//              to 7. A frame with an id outside its code book (or past the fine model's 1024 ids) is reported in bit 2 of *status and not written. The aux[e]
//              cells behind the frames get 1024 in all 8 channels: the padding of a row shorter than the window.
//   emit       The frames that just turned final, cells [cell[e], cell[e] + len[e]), as int64 columns from out[at[e]] on, planes `stride` apart: what
//              AcousticDecodeStream.push takes on the device. Two 16-byte loads a frame, eight 8-byte stores that are contiguous across the wave.
//   shift      cells [cell[e], cell[e] + len[e]) = the cells aux[e] further on: one workgroup a piece, every cell read before any is written.
constexpr int FINE_POOL_CHUNK = 128;
struct FinePieces {
    int n;
    int cell[FINE_POOL_CHUNK];   // the piece's first cell in the state's work arrays
    int len[FINE_POOL_CHUNK];    // hand-over: frames; emit: frames; shift: cells kept
    int aux[FINE_POOL_CHUNK];    // hand-over: cells of padding behind the frames; shift: cells dropped
    int at[FINE_POOL_CHUNK];     // hand-over: the first id in ids; emit: the first element in out
};
static_assert(sizeof(FinePieces) + 64 <= 4096, "the pool kernels' arguments must stay under the launch limit");

// ones: NULL, or the key masks of the call's windows [n_ones], written by the call's first launch
__global__ __launch_bounds__(256) void fine_pool_handover_kernel(FinePieces p, const int* ids, int offset, int codebook_size, int* work, float* ones, int n_ones, int* status) {
    const int e = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (ones && e == 0 && t < n_ones) ones[t] = 1.0f;
    if (e >= p.n) return;
    const int n = p.len[e];
    if (t >= n + p.aux[e]) return;
    int4* cell = reinterpret_cast<int4*>(work + ((size_t)p.cell[e] + t) * FINE_CODES);
    int c0 = FINE_VOCAB, c1 = FINE_VOCAB;
    if (t < n) {
        const int2 id = reinterpret_cast<const int2*>(ids + p.at[e])[t];
        const int top = min(codebook_size, FINE_VOCAB);
        c0 = id.x - offset;
        c1 = id.y - offset - codebook_size;
        if (c0 < 0 || c0 >= top || c1 < 0 || c1 >= top) {
            if (status) atomicOr(status, HANDOVER_BAD_ID);
            return;
        }
    }
    cell[0] = make_int4(c0, c1, FINE_VOCAB, FINE_VOCAB);
    cell[1] = make_int4(FINE_VOCAB, FINE_VOCAB, FINE_VOCAB, FINE_VOCAB);
}

// frame t of piece e goes to out[at[e] + ch * stride + t]
__global__ __launch_bounds__(256) void fine_pool_emit_kernel(FinePieces p, const int* work, long long* out, int stride) {
    const int e = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= p.len[e]) return;
    const int4* cell = reinterpret_cast<const int4*>(work + ((size_t)p.cell[e] + t) * FINE_CODES);
    const int4 lo = cell[0], hi = cell[1];
    const int ids[FINE_CODES] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int ch = 0; ch < FINE_CODES; ++ch) out[(size_t)p.at[e] + (size_t)ch * stride + t] = ids[ch];
}

// len is at most 2 W <= 2048: two cells a thread
__global__ __launch_bounds__(1024) void fine_pool_shift_kernel(FinePieces p, int* work) {
    const int e = blockIdx.x, n = p.len[e];
    int* base = work + (size_t)p.cell[e] * FINE_CODES;
    int4 v[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int t = threadIdx.x + 1024 * i;
        if (t < n) {
            const int4* src = reinterpret_cast<const int4*>(base + ((size_t)p.aux[e] + t) * FINE_CODES);
            v[i][0] = src[0]; v[i][1] = src[1];
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int t = threadIdx.x + 1024 * i;
        if (t < n) {
            int4* dst = reinterpret_cast<int4*>(base + (size_t)t * FINE_CODES);
            dst[0] = v[i][0]; dst[1] = v[i][1];
        }
    }
}

// one piece: n frames of ids into cells [0, n + n_pad) of work; ones: NULL, or the attention's key mask [W], written by the call's first launch
int launch_handover(const int32_t* ids, int n, int n_pad, int offset, int codebook_size, int* work, float* ones, int W, int32_t* status, hipStream_t stream) {
    const int mask = ones ? W : 0, span = n + n_pad > mask ? n + n_pad : mask;
    if (span <= 0) return 0;
    FinePieces p{};
    p.n = 1;
    p.len[0] = n;
    p.aux[0] = n_pad;
    hipLaunchKernelGGL(fine_pool_handover_kernel, dim3((span + 255) / 256, 1), dim3(256), 0, stream, p, ids, offset, codebook_size, work, ones, mask, status);
    AT_CHECK_HIP(hipGetLastError());
    return 0;
}

int check_handover(const int32_t* ids_dev, int n_frames, int acoustic_offset, int codebook_size) {
    AT_REQUIRE(n_frames >= 0 && (ids_dev != nullptr || n_frames == 0), "n_frames must not be negative, and frames need a pointer");
    AT_REQUIRE((reinterpret_cast<uintptr_t>(ids_dev) & 7) == 0, "ids_dev must be 8-byte aligned: a frame is one load");
    AT_REQUIRE(acoustic_offset >= 0 && codebook_size >= 1 && (int64_t)acoustic_offset + 2 * (int64_t)codebook_size <= INT32_MAX, "the two code books must be ranges of int32 ids");
    return 0;
}

}  // namespace

extern "C" {

size_t at_fine_stream_state_bytes(const at_fine_t* h) {
    if (!(h && h->finalized)) { set_error("at_fine_stream_state_bytes: the model is not finalized"); return 0; }
    return carve_state(nullptr, 1, fine_stream_cells(h->block), 0, h->block, h->embd).bytes;
}

int at_op_fine_handover(const int32_t* ids_dev, int n_frames, int n_pad, int acoustic_offset, int codebook_size, int32_t* work_dev, at_stream_t stream,
                        int32_t* status_dev) {
    if (int rc = check_handover(ids_dev, n_frames, acoustic_offset, codebook_size)) return rc;
    AT_REQUIRE(work_dev != nullptr && n_pad >= 0 && (int64_t)n_frames + n_pad <= FINE_MAX_T, "a work array of n_frames + n_pad cells, at most 262144");
    AT_REQUIRE((reinterpret_cast<uintptr_t>(work_dev) & 15) == 0, "work_dev must be 16-byte aligned");
    return launch_handover(ids_dev, n_frames, n_pad, acoustic_offset, codebook_size, work_dev, nullptr, 0, status_dev, (hipStream_t)stream);
}

int at_fine_stream_push(at_fine_t* h, void* state_dev, size_t state_bytes, int64_t* pos, const int32_t* ids_dev, int n_frames, int final, int acoustic_offset,
                        int codebook_size, float temperature, int greedy, const float* uniforms_dev, int u_win0, int u_windows, int64_t* emit_dev,
                        int emit_stride, int32_t* n_emitted, int32_t* windows_run, at_stream_t stream_, int32_t* status_dev) {
    AT_REQUIRE(h && h->finalized, "the model is not finalized");
    AT_REQUIRE(state_dev != nullptr, "null state");
    AT_REQUIRE(pos && n_emitted, "null pointer");
    AT_REQUIRE(final == 0 || final == 1, "final must be 0 or 1");
    AT_REQUIRE(greedy == 0 || greedy == 1, "greedy must be 0 or 1");
    AT_REQUIRE(greedy || (std::isfinite(temperature) && temperature > 0.0f), "temperature must be a positive finite number");
    if (int rc = check_handover(ids_dev, n_frames, acoustic_offset, codebook_size)) return rc;
    AT_REQUIRE(pos[1] == 0, "the stream is finished: a push after the final call");
    AT_REQUIRE(pos[0] >= 0 && pos[0] + n_frames <= FINE_MAX_T, "a stream takes at most 262144 frames");
    AT_REQUIRE(!final || pos[0] + n_frames >= 1, "a final call with nothing pushed");
    AT_REQUIRE(u_win0 >= 0 && u_windows >= 0 && emit_stride >= 0, "u_win0, u_windows and emit_stride must not be negative");
    const int W = h->block, H = W / 2;
    // ---- a dry run of the schedule: the windows and the frames of this call against the caller's arrays
    int n_win = 0, j_lo = -1, j_hi = -1;
    long long emitted = 0;
    {
        FineStreamSchedule dry(pos[0], n_frames, final != 0, W);
        FineStreamRound rd;
        while (dry.next(&rd)) {
            const int n = rd.n_win + (rd.last_window ? 1 : 0);
            if (n > 0) { if (j_lo < 0) j_lo = rd.j_first; j_hi = rd.j_first + n; }
            n_win += n;
            emitted += rd.emit_to - rd.emit_from;
        }
    }
    AT_REQUIRE(greedy || n_win == 0 || (uniforms_dev != nullptr && j_lo >= u_win0 && j_hi <= u_win0 + u_windows), "the uniforms do not cover the windows this call runs");
    AT_REQUIRE(emitted == 0 || (emit_dev != nullptr && emitted <= emit_stride), "emit_dev must hold the frames that turn final in this call");
    const FineState s = carve_state(state_dev, 1, fine_stream_cells(W), 0, W, h->embd);
    AT_REQUIRE(state_bytes >= s.bytes, "state too small: at_fine_stream_state_bytes(h)");
    // ---- nothing above touched the device
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    hipStream_t stream = (hipStream_t)stream_;
    const FineSampleArgs sa = sample_args(s, W, greedy, temperature, uniforms_dev, nullptr, nullptr);
    auto run_window = [&](int cell, int j, int rel) -> int {
        FinePass p{};
        p.n = 1;
        p.cell0[0] = cell;
        p.draw[0] = j - u_win0;
        p.rel[0] = rel;
        p.head_off[1] = W - rel;
        return run_codebooks(h, s, p, sa, stream);
    };
    FineStreamSchedule schedule(pos[0], n_frames, final != 0, W);
    FineStreamRound rd;
    int taken = 0, col = 0;
    bool first = true;
    const long long T = pos[0] + n_frames;
    while (schedule.next(&rd)) {
        if (rd.take > 0 || rd.pad > 0 || (first && n_win > 0))
            if (int rc = launch_handover(ids_dev + 2 * (size_t)taken, rd.take, rd.pad, acoustic_offset, codebook_size, s.work + (size_t)rd.held * FINE_CODES,
                                         first ? s.ones : nullptr, W, status_dev, stream))
                return rc;
        first = false;
        taken += rd.take;
        const int plain = rd.pad ? 1 : rd.n_win;
        for (int i = 0; i < plain; ++i)
            if (int rc = run_window((int)((long long)(rd.j_first + i) * H - rd.first), rd.j_first + i, 0)) return rc;
        if (rd.last_window)
            if (int rc = run_window((int)(T - W - rd.first), rd.j_first + rd.n_win, rd.last_rel)) return rc;
        const int n = (int)(rd.emit_to - rd.emit_from);
        if (n > 0) {
            FinePieces p{};
            p.n = 1;
            p.cell[0] = (int)(rd.emit_from - rd.first);
            p.len[0] = n;
            p.at[0] = col;
            hipLaunchKernelGGL(fine_pool_emit_kernel, dim3((n + 255) / 256, 1), dim3(256), 0, stream, p, s.work, reinterpret_cast<long long*>(emit_dev), emit_stride);
            AT_CHECK_HIP(hipGetLastError());
            col += n;
        }
        if (rd.shift > 0) {
            FinePieces p{};
            p.n = 1;
            p.aux[0] = rd.shift;
            p.len[0] = rd.held + rd.take - rd.shift;
            hipLaunchKernelGGL(fine_pool_shift_kernel, dim3(1), dim3(1024), 0, stream, p, s.work);
            AT_CHECK_HIP(hipGetLastError());
        }
    }
    pos[0] = T;
    pos[1] = final;
    *n_emitted = (int)emitted;
    if (windows_run) *windows_run = n_win;
    return 0;
}

}  // extern "C"

// ---- the stream pool: many rows whose coarse frames arrive in pushes share the passes ----------------------------------------------
namespace {

// per stream 2 W cells [8]; shared, the activations of fine_slots windows
FineState carve_pool(void* base, int streams, int fine_slots, int W, int E) {
    FineState s{};
    StateCarver c(base);
    const size_t R = (size_t)fine_slots * W;
    s.Lmax = fine_stream_cells(W);
    s.work = c.take<int>((size_t)streams * s.Lmax * FINE_CODES);
    s.ones = c.take<float>(R);
    s.x = c.take<float>(R * E);
    s.xn = c.take<float>(R * E);
    s.qkv = c.take<float>(R * 3 * E);
    s.h = c.take<float>(R * 4 * E);
    s.logits = c.take<float>(R * FINE_VOCAB);
    s.bytes = c.off;
    return s;
}

// the pieces gathered for one kernel, launched FINE_POOL_CHUNK at a time
struct FinePoolLaunch {
    std::vector<FinePieces> chunks;
    int span = 0;   // the longest piece, in threads
    void add(long long cell, int len, int aux, long long at, int threads) {
        if (chunks.empty() || chunks.back().n == FINE_POOL_CHUNK) chunks.push_back(FinePieces{});
        FinePieces& c = chunks.back();
        c.cell[c.n] = (int)cell; c.len[c.n] = len; c.aux[c.n] = aux; c.at[c.n] = (int)at; ++c.n;
        span = threads > span ? threads : span;
    }
};

}  // namespace

extern "C" {

size_t at_fine_pool_state_bytes(const at_fine_t* h, int streams, int fine_slots) {
    if (!(h && h->finalized)) { set_error("at_fine_pool_state_bytes: the model is not finalized"); return 0; }
    if (!(streams >= 1 && streams <= FINE_MAX_POOL_STREAMS)) { set_error("at_fine_pool_state_bytes: streams must be 1 to 1024"); return 0; }
    if (!(fine_slots >= 1 && fine_slots <= FINE_MAX_B)) { set_error("at_fine_pool_state_bytes: fine_slots must be 1 to 64"); return 0; }
    return carve_pool(nullptr, streams, fine_slots, h->block, h->embd).bytes;
}

int at_fine_pool_push(at_fine_t* h, void* state_dev, size_t state_bytes, int streams, int fine_slots, int64_t* pos, int n, const int32_t* place,
                      const int32_t* ids_dev, const int64_t* id_off, const int32_t* n_frames, const int32_t* final, int acoustic_offset, int codebook_size,
                      float temperature, int greedy, const float* uniforms_dev, const int32_t* u_cell0, const int32_t* u_win0, const int32_t* u_windows,
                      int64_t* emit_dev, int emit_stride, int32_t* n_emitted, int32_t* windows_run, int32_t* trace, int trace_cap, int32_t* n_passes,
                      at_stream_t stream_, int32_t* status_dev) {
    const char* who = "at_fine_pool_push";
    AT_REQUIRE(h && h->finalized, "the model is not finalized");
    AT_REQUIRE(streams >= 1 && streams <= FINE_MAX_POOL_STREAMS, "streams must be 1 to 1024");
    AT_REQUIRE(fine_slots >= 1 && fine_slots <= FINE_MAX_B, "fine_slots must be 1 to 64");
    AT_REQUIRE(state_dev != nullptr, "null state");
    AT_REQUIRE(n >= 0 && n <= streams, "n (the call's streams) must be 0 to streams");
    AT_REQUIRE(pos != nullptr, "null pointer");
    AT_REQUIRE(n == 0 || (place && id_off && n_frames && final && u_cell0 && u_win0 && u_windows && n_emitted), "null pointer");
    AT_REQUIRE(greedy == 0 || greedy == 1, "greedy must be 0 or 1");
    AT_REQUIRE(greedy || (std::isfinite(temperature) && temperature > 0.0f), "temperature must be a positive finite number");
    AT_REQUIRE(trace_cap >= 0 && (trace != nullptr || trace_cap == 0), "trace_cap must be 0 without a trace and never negative");
    AT_REQUIRE(emit_stride >= 0, "emit_stride must not be negative");
    AT_REQUIRE((int64_t)n * FINE_CODES * emit_stride <= INT32_MAX, "n * 8 * emit_stride must fit 31 bits: the pieces are addressed by int");
    if (int rc = check_handover(ids_dev, 0, acoustic_offset, codebook_size)) return rc;
    const int W = h->block;
    // ---- every stream of the call, checked before any is changed: its place, its record, and a dry run of its schedule against the caller's arrays
    std::vector<char> named((size_t)streams, 0);
    std::vector<int64_t> T_before((size_t)n);
    std::vector<long long> emitted((size_t)n, 0);
    std::vector<int32_t> ran((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        const std::string at = std::string(who) + ": stream " + std::to_string(i) + " of the call: ";
        if (place[i] < 0 || place[i] >= streams || named[place[i]]) { set_error(at + "its place must be 0 to streams - 1 and named once"); return -1; }
        named[place[i]] = 1;
        const int64_t* ps = pos + 2 * (size_t)place[i];
        if (final[i] != 0 && final[i] != 1) { set_error(at + "final must be 0 or 1"); return -1; }
        if (n_frames[i] < 0 || (n_frames[i] > 0 && ids_dev == nullptr)) { set_error(at + "n_frames must not be negative, and frames need a pointer"); return -1; }
        if (id_off[i] < 0 || (id_off[i] & 1)) { set_error(at + "id_off must be even and not negative: a frame is one 8-byte load"); return -1; }
        if (id_off[i] + 2 * (int64_t)n_frames[i] > INT32_MAX) { set_error(at + "its ids must lie below 2^31 in ids_dev"); return -1; }
        if (ps[1] != 0) { set_error(at + "the stream is finished: a push after the final call"); return -1; }
        if (ps[0] < 0 || ps[0] + n_frames[i] > FINE_MAX_T) { set_error(at + "a stream takes at most 262144 frames"); return -1; }
        if (final[i] && ps[0] + n_frames[i] < 1) { set_error(at + "a final call with nothing pushed"); return -1; }
        if (u_cell0[i] < 0 || u_win0[i] < 0 || u_windows[i] < 0) { set_error(at + "u_cell0, u_win0 and u_windows must not be negative"); return -1; }
        T_before[i] = ps[0];
        int j_lo = -1, j_hi = -1;
        FineStreamSchedule dry(ps[0], n_frames[i], final[i] != 0, W);
        FineStreamRound rd;
        while (dry.next(&rd)) {
            const int m = rd.n_win + (rd.last_window ? 1 : 0);
            if (m > 0) { if (j_lo < 0) j_lo = rd.j_first; j_hi = rd.j_first + m; }
            ran[i] += m;
            emitted[i] += rd.emit_to - rd.emit_from;
        }
        if (!(greedy || ran[i] == 0 || (uniforms_dev != nullptr && j_lo >= u_win0[i] && j_hi <= u_win0[i] + u_windows[i]))) {
            set_error(at + "the uniforms do not cover the windows this call runs");
            return -1;
        }
        if (!(emitted[i] == 0 || (emit_dev != nullptr && emitted[i] <= emit_stride))) { set_error(at + "emit_dev must hold the frames that turn final in this call"); return -1; }
    }
    const FineState s = carve_pool(state_dev, streams, fine_slots, W, h->embd);
    AT_REQUIRE(state_bytes >= s.bytes, "state too small: at_fine_pool_state_bytes(h, streams, fine_slots)");
    if (n_passes) *n_passes = 0;
    if (n == 0) return 0;
    // ---- nothing above touched the device or the host record
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    hipStream_t stream = (hipStream_t)stream_;
    const FineSampleArgs sa = sample_args(s, W, greedy, temperature, uniforms_dev, nullptr, nullptr);
    FinePoolSchedule schedule(T_before.data(), n_frames, final, n, W, fine_slots);
    std::vector<int> taken((size_t)n, 0), col((size_t)n, 0);
    bool first = true;
    while (schedule.next_round()) {
        FinePoolLaunch handover, emit, shift;
        for (int i = 0; i < n; ++i) {
            const FineStreamRound* rd = schedule.round(i);
            if (!rd) continue;
            const long long base = (long long)place[i] * s.Lmax;
            if (rd->take > 0 || rd->pad > 0) handover.add(base + rd->held, rd->take, rd->pad, id_off[i] + 2 * (long long)taken[i], rd->take + rd->pad);
            taken[i] += rd->take;
            const int m = (int)(rd->emit_to - rd->emit_from);
            if (m > 0) {
                emit.add(base + (rd->emit_from - rd->first), m, 0, (long long)i * FINE_CODES * emit_stride + col[i], m);
                col[i] += m;
            }
            if (rd->shift > 0) shift.add(base, rd->held + rd->take - rd->shift, rd->shift, 0, 0);
        }
        // the hand-over; the call's first launch also writes the key masks, so it happens even when no stream hands anything over
        if (first && handover.chunks.empty()) handover.chunks.push_back(FinePieces{});
        for (const FinePieces& c : handover.chunks) {
            const int n_ones = first ? fine_slots * W : 0, span = handover.span > n_ones ? handover.span : n_ones;
            hipLaunchKernelGGL(fine_pool_handover_kernel, dim3((span + 255) / 256, c.n > 0 ? c.n : 1), dim3(256), 0, stream, c, ids_dev, acoustic_offset, codebook_size,
                               s.work, first ? s.ones : nullptr, n_ones, status_dev);
            AT_CHECK_HIP(hipGetLastError());
            first = false;
        }
        FinePoolPass ps;
        while (schedule.next(&ps)) {
            FinePass p{};
            p.n = ps.n;
            for (int w = 0; w < ps.n; ++w) {
                const int i = ps.stream[w];
                p.cell0[w] = (int)((long long)place[i] * s.Lmax + ps.cell[w]);
                p.draw[w] = u_cell0[i] + ps.j[w] - u_win0[i];
                p.rel[w] = ps.rel[w];
                p.head_off[w + 1] = p.head_off[w] + W - ps.rel[w];
            }
            if (int rc = run_codebooks(h, s, p, sa, stream)) return rc;
            const int at = schedule.passes() - 1;
            if (at < trace_cap) {   // a trace too small loses its tail, the run goes on
                int32_t* row = trace + 3 * (size_t)at;
                row[0] = schedule.rounds() - 1; row[1] = ps.wave; row[2] = ps.n;
            }
        }
        for (const FinePieces& c : emit.chunks) {
            hipLaunchKernelGGL(fine_pool_emit_kernel, dim3((emit.span + 255) / 256, c.n), dim3(256), 0, stream, c, s.work, reinterpret_cast<long long*>(emit_dev), emit_stride);
            AT_CHECK_HIP(hipGetLastError());
        }
        for (const FinePieces& c : shift.chunks) {
            hipLaunchKernelGGL(fine_pool_shift_kernel, dim3(c.n), dim3(1024), 0, stream, c, s.work);
            AT_CHECK_HIP(hipGetLastError());
        }
    }
    for (int i = 0; i < n; ++i) {
        pos[2 * (size_t)place[i]] += n_frames[i];
        pos[2 * (size_t)place[i] + 1] = final[i];
        n_emitted[i] = (int)emitted[i];
        if (windows_run) windows_run[i] = ran[i];
    }
    if (n_passes) *n_passes = schedule.passes();
    return 0;
}

}  // extern "C"
