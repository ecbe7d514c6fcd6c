// Teacher-forced scoring under the semantic-to-acoustic GPT: the log-probability and the rank of given ids, where gpt.hip's generators
// draw ids. One pass is one prefill of gpt_model.hip's model over a token list, without its head; the head is applied here to every scored position, in
// chunks whose logits are reduced as they are produced and never stored whole. Kernels:
//   gpt_score_begin_kernel   a pass's token list (cache row, position, id) and its scored positions (the token whose logits are scored, the target, the
//                            allow set's parity, where the result goes)
//   gpt_score_kernel         the row rule: temperature, allow ranges, max, the sum of exponentials in one fixed order, the target's rank; one workgroup per row
// Nothing here adds floats atomically: a call repeated gives the same bits.
#include <cmath>
#include <cstdint>

#include "../../include/audiotoken_hip.h"
#include "gpt_kernels.h"

using namespace at;

namespace {

constexpr int E = GPT_EMBD, HD = GPT_HEAD_DIM, NH = GPT_HEADS, FF = GPT_FF;
constexpr int SCORE_THREADS = 1024, SCORE_WAVES = SCORE_THREADS / 64;
constexpr int SCORE_GROUP = 256;       // ids one wave takes at a time: 4 consecutive ids per lane, one 16-byte load where the row allows
constexpr int SCORE_MAX_ROWS = 65536;  // rows of one at_gpt_score or at_op_score_rows call
constexpr int HEAD_ROWS_MAX = 4096;

__device__ __forceinline__ bool allowed(const Allow& a, int i) { return !a.on || (i >= a.lo0 && i < a.hi0) || (i >= a.lo1 && i < a.hi1); }

// Steps 1 and 2 of the rule for ids i .. i + 3 of row z (i a multiple of 4): one IEEE division each, -inf outside the allow ranges and past the row's end
__device__ __forceinline__ float4 tempered4(const float* z, int i, int V, bool vec, float temperature, const Allow& a) {
    float4 v;
    if (vec && i + 3 < V) {
        v = *reinterpret_cast<const float4*>(z + i);
    } else {
        v.x = i < V ? z[i] : 0.f;
        v.y = i + 1 < V ? z[i + 1] : 0.f;
        v.z = i + 2 < V ? z[i + 2] : 0.f;
        v.w = i + 3 < V ? z[i + 3] : 0.f;
    }
    v.x = i < V && allowed(a, i) ? v.x / temperature : -INFINITY;
    v.y = i + 1 < V && allowed(a, i + 1) ? v.y / temperature : -INFINITY;
    v.z = i + 2 < V && allowed(a, i + 2) ? v.z / temperature : -INFINITY;
    v.w = i + 3 < V && allowed(a, i + 3) ? v.w / temperature : -INFINITY;
    return v;
}

// The row rule. Wave w owns the ids [w per_wave, (w + 1) per_wave), per_wave a multiple of 256, and walks them 256 at a time: lane l takes the
// four ids 256 g + 4 l .. + 3 of group g. The order of additions of S: a lane's four weights as (e0 + e1) + (e2 + e3), added to the lane's running sum group
// after group; the 64 lanes by the xor butterfly, distances 32 down to 1; the 16 waves in index order. The load width does not enter that order, so a row gives
// the same bits wherever it lies. m and S take one walk each; the rank (ids above the target's value, ties not counted) is an integer and rides on the second.
__global__ __launch_bounds__(SCORE_THREADS) void gpt_score_kernel(ScoreArgs a) {
    __shared__ float part[SCORE_WAVES];
    __shared__ int above[SCORE_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x, V = a.V;
    const float* z = a.logits + (size_t)row * V;
    const Allow allow = a.allow[a.parity ? a.parity[row] & 1 : 0];
    const size_t o = a.out_index ? (size_t)a.out_index[row] : (size_t)row;
    const bool vec = (reinterpret_cast<uintptr_t>(z) & 15) == 0;
    if (a.logits_out) {
        float* dst = a.logits_out + o * V;
        for (int i = tid; i < V; i += SCORE_THREADS) dst[i] = z[i];
    }
    const int t = a.targets[row];
    const bool scored = t >= 0 && t < V && allowed(allow, t);   // uniform over the workgroup
    const float zt = scored ? z[t] / a.temperature : -INFINITY;
    const int per_wave = ((V + SCORE_WAVES - 1) / SCORE_WAVES + SCORE_GROUP - 1) / SCORE_GROUP * SCORE_GROUP, first = wave * per_wave;
    float m = -INFINITY;
    for (int g = 0; g < per_wave; g += SCORE_GROUP) {
        const float4 v = tempered4(z, first + g + 4 * lane, V, vec, a.temperature, allow);
        m = fmaxf(m, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
    if (lane == 0) part[wave] = m;
    __syncthreads();
    m = part[0];
#pragma unroll
    for (int w = 1; w < SCORE_WAVES; ++w) m = fmaxf(m, part[w]);
    __syncthreads();
    float s = 0.f;
    int n = 0;
    for (int g = 0; g < per_wave; g += SCORE_GROUP) {
        const float4 v = tempered4(z, first + g + 4 * lane, V, vec, a.temperature, allow);
        s += (expf(v.x - m) + expf(v.y - m)) + (expf(v.z - m) + expf(v.w - m));
        n += (v.x > zt) + (v.y > zt) + (v.z > zt) + (v.w > zt);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { s += __shfl_xor(s, d); n += __shfl_xor(n, d); }
    if (lane == 0) { part[wave] = s; above[wave] = n; }
    __syncthreads();
    if (tid != 0) return;
    float S = part[0];
    int cnt = above[0];
#pragma unroll
    for (int w = 1; w < SCORE_WAVES; ++w) { S += part[w]; cnt += above[w]; }
    a.logprob[o] = scored ? (zt - m) - logf(S) : -INFINITY;
    a.rank[o] = scored ? cnt : V;
}

// ---- a pass --------------------------------------------------------------------------------------------------------------------------------
// The caller's rows row0 .. row0 + n - 1 in cache rows 0 .. n - 1: row j's tokens are the list's [off[j], off[j + 1]), its scored positions the pass's
// [cum[j], cum[j + 1]), the first of them position from[j]
struct ScorePlan {
    int n, row0;
    int off[GPT_MAX_B + 1], cum[GPT_MAX_B + 1], from[GPT_MAX_B];
};

// The scorer's state: what carve_state (gpt.hip) gives a generator, with the scored positions' lists in place of the rows' bookkeeping and one chunk of
// logits in place of a row of them per cache row
struct ScoreState {
    GptState g;
    int *gather, *target, *parity, *out_index;   // per scored position of a pass
};

ScoreState carve_score_state(void* base, int rows, int cap, int tokens, int head_rows, int vocab, int n_layer) {
    ScoreState s{};
    StateCarver c(base);
    const size_t R = (size_t)tokens;
    s.g.done = c.take<int>(GPT_MAX_B);
    s.g.tok_row = c.take<int>(R);
    s.g.tok_pos = c.take<int>(R);
    s.gather = c.take<int>(R);
    s.target = c.take<int>(R);
    s.parity = c.take<int>(R);
    s.out_index = c.take<int>(R);
    s.g.x = c.take<float>(R * E);
    s.g.xn = c.take<float>(R * E);
    s.g.q = c.take<float>(R * 3 * E);
    s.g.h = c.take<float>(R * FF);
    s.g.tok_id = (int*)s.g.h;   // as in carve_state: read by the embedding before the first layer's MLP writes h
    s.g.logits = c.take<float>((size_t)head_rows * vocab);
    s.g.layer_stride = (size_t)rows * cap * NH * HD;
    s.g.kc = c.take<float>(s.g.layer_stride * n_layer);
    s.g.vc = c.take<float>(s.g.layer_stride * n_layer);
    s.g.cap = cap;
    s.g.bytes = c.off;
    return s;
}

// Token i of the pass: cache row j, position pos, the caller's id as it is (the embedding clamps it and reports it). A row's list holds all its ids but the
// last, which is a target only: nothing reads its logits or its K and V. The id after token i, at position pos + 1, is a target when that position is at or
// past the row's first scored one: scored position c takes token i's logits. A target is clamped and reported here (the last id meets no embedding). Every
// cache row of the pass is marked running, which is what lets the prefill write its K and V.
__global__ void gpt_score_begin_kernel(ScorePlan p, const int* seq, int seq_stride, int out_stride, int V, ScoreState s, int* status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < p.n) s.g.done[i] = GPT_RUNNING;
    if (i >= p.off[p.n]) return;
    int j = 0;
    while (j + 1 < p.n && p.off[j + 1] <= i) ++j;
    const int pos = i - p.off[j];
    const int* row = seq + (size_t)(p.row0 + j) * seq_stride;
    s.g.tok_row[i] = j;
    s.g.tok_pos[i] = pos;
    s.g.tok_id[i] = row[pos];
    const int at = pos + 1 - p.from[j];   // the target's index among the row's scored positions
    if (at < 0) return;
    int id = row[pos + 1];
    if (id < 0 || id >= V) {
        if (status) atomicOr(status, 1);
        id = min(max(id, 0), V - 1);
    }
    const int c = p.cum[j] + at;
    s.gather[c] = i;
    s.target[c] = id;
    s.parity[c] = at & 1;
    s.out_index[c] = (p.row0 + j) * out_stride + at;
}

bool score_dims_ok(const char* who, const at_gpt* h, int rows, int max_len, int pass_tokens, int head_rows) {
    std::string bad;
    if (!(h && h->finalized)) bad = "the model is not finalized";
    else if (!(rows >= 1 && rows <= GPT_MAX_B)) bad = "rows must be 1 to 64";
    else if (!(max_len >= 2 && max_len <= h->block)) bad = "max_len must be 2 to the model's block size";
    else if (!(pass_tokens >= max_len && pass_tokens <= GPT_MAX_TICK_TOKENS)) bad = "pass_tokens must be max_len (one row always fits) to 65600";
    else if (!(head_rows >= 16 && head_rows <= HEAD_ROWS_MAX && head_rows % 16 == 0)) bad = "head_rows must be a multiple of 16, 16 to 4096";
    if (bad.empty()) return true;
    set_error(std::string(who) + ": " + bad);
    return false;
}

}  // namespace

namespace at {

int gpt_score_rows(const ScoreArgs& a, int rows, hipStream_t stream) {
    hipLaunchKernelGGL(gpt_score_kernel, dim3(rows), dim3(SCORE_THREADS), 0, stream, a);
    AT_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace at

extern "C" {

int at_op_score_rows(const float* logits_dev, int R, int V, const int32_t* targets_dev, float temperature, const int32_t* allow, float* logprob_out_dev,
                     int32_t* rank_out_dev, at_stream_t stream) {
    AT_REQUIRE(logits_dev && targets_dev && logprob_out_dev && rank_out_dev, "null pointer");
    AT_REQUIRE(R >= 1 && R <= SCORE_MAX_ROWS, "R must be 1 to 65536");
    AT_REQUIRE(V >= 1 && V <= GPT_MAX_VOCAB, "V must be 1 to 65536");
    AT_REQUIRE(std::isfinite(temperature) && temperature > 0.0f, "temperature must be a positive finite number");
    ScoreArgs sa{};
    if (int rc = check_allow(allow, V, &sa.allow[0])) return rc;
    sa.logits = logits_dev; sa.V = V; sa.temperature = temperature; sa.targets = targets_dev; sa.logprob = logprob_out_dev; sa.rank = rank_out_dev;
    return gpt_score_rows(sa, R, (hipStream_t)stream);
}

size_t at_gpt_score_state_bytes(const at_gpt_t* h, int rows, int max_len, int pass_tokens, int head_rows) {
    if (!score_dims_ok("at_gpt_score_state_bytes", h, rows, max_len, pass_tokens, head_rows)) return 0;
    return carve_score_state(nullptr, rows, max_len, pass_tokens, head_rows, h->vocab, h->n_layer).g.bytes;
}

int at_gpt_score(at_gpt_t* h, const int32_t* seq_dev, int seq_stride, const int32_t* seq_len, const int32_t* score_from, int n_rows, float temperature,
                 const int32_t* allow, float* logprob_out_dev, int32_t* rank_out_dev, int out_stride, float* logits_out_dev, void* state_dev, size_t state_bytes,
                 int rows, int max_len, int pass_tokens, int head_rows, at_stream_t stream_, int32_t* status_dev) {
    if (!score_dims_ok("at_gpt_score", h, rows, max_len, pass_tokens, head_rows)) return -1;
    AT_REQUIRE(n_rows >= 1 && n_rows <= SCORE_MAX_ROWS, "n_rows must be 1 to 65536");
    AT_REQUIRE(seq_dev && seq_len && score_from && logprob_out_dev && rank_out_dev, "null pointer");
    AT_REQUIRE(state_dev != nullptr, "null state");
    AT_REQUIRE(seq_stride >= 2 && out_stride >= 1, "seq_stride must be at least 2, out_stride at least 1");
    AT_REQUIRE((int64_t)n_rows * out_stride <= INT32_MAX, "n_rows * out_stride must stay below 2^31");
    AT_REQUIRE(std::isfinite(temperature) && temperature > 0.0f, "temperature must be a positive finite number");
    const int V = h->vocab;
    ScoreArgs sa{};
    if (int rc = check_allow(allow, V, &sa.allow[0])) return rc;
    if (int rc = check_allow(allow ? allow + 4 : nullptr, V, &sa.allow[1])) return rc;
    for (int b = 0; b < n_rows; ++b) {
        if (seq_len[b] < 2 || seq_len[b] > max_len || seq_len[b] > seq_stride) {
            set_error("at_gpt_score: seq_len of row " + std::to_string(b) + " must be 2 to min(max_len, seq_stride)");
            return -1;
        }
        if (score_from[b] < 1 || score_from[b] >= seq_len[b]) {
            set_error("at_gpt_score: score_from of row " + std::to_string(b) + " must be 1 to seq_len - 1");
            return -1;
        }
        if (seq_len[b] - score_from[b] > out_stride) {
            set_error("at_gpt_score: row " + std::to_string(b) + " scores more positions than out_stride holds");
            return -1;
        }
    }
    const ScoreState s = carve_score_state(state_dev, rows, max_len, pass_tokens, head_rows, V, h->n_layer);
    AT_REQUIRE(state_bytes >= s.g.bytes, "state too small: at_gpt_score_state_bytes(h, rows, max_len, pass_tokens, head_rows)");
    // ---- nothing above touched the device
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    hipStream_t stream = (hipStream_t)stream_;
    sa.V = V; sa.temperature = temperature; sa.logits = s.g.logits;
    sa.logprob = logprob_out_dev; sa.rank = rank_out_dev; sa.logits_out = logits_out_dev;
    const StepSlots no_steps{};
    for (int next = 0; next < n_rows;) {
        // a pass: the caller's next rows while a cache row and room in the token list are left; a row's last id is a target only and takes no room
        ScorePlan p{};
        p.row0 = next;
        while (next < n_rows && p.n < rows && p.off[p.n] + seq_len[next] - 1 <= pass_tokens) {
            p.from[p.n] = score_from[next];
            p.off[p.n + 1] = p.off[p.n] + seq_len[next] - 1;
            p.cum[p.n + 1] = p.cum[p.n] + seq_len[next] - score_from[next];
            ++p.n;
            ++next;
        }
        const int R = p.off[p.n], scored = p.cum[p.n];
        hipLaunchKernelGGL(gpt_score_begin_kernel, dim3((R + 255) / 256), dim3(256), 0, stream, p, seq_dev, seq_stride, out_stride, V, s, status_dev);
        AT_CHECK_HIP(hipGetLastError());
        if (int rc = gpt_forward(h, s.g, no_steps, 0, R, status_dev, stream, false)) return rc;
        // the head, head_rows scored positions at a time: the final LayerNorm of their tokens, the logits on the fp32 GEMM, the row rule
        for (int c0 = 0; c0 < scored; c0 += head_rows) {
            const int n = scored - c0 < head_rows ? scored - c0 : head_rows;
            if (int rc = gpt_final_ln(h, s.g.x, s.gather + c0, s.g.xn, n, stream)) return rc;
            GemmArgs g;
            g.X = s.g.xn; g.Tin = n; g.Cin = E; g.ldx = E; g.W = h->wte; g.C = s.g.logits; g.ldc = V; g.M = n; g.N = V; g.K = E;
            if (int rc = launch_gemm(g, stream)) return rc;
            sa.targets = s.target + c0; sa.parity = s.parity + c0; sa.out_index = s.out_index + c0;
            if (int rc = gpt_score_rows(sa, n, stream)) return rc;
        }
    }
    return 0;
}

}  // extern "C"
