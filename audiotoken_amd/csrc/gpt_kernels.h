// What gpt.hip (the handle, the plans and the three entry points) and gpt_model.hip (the model pass and the sampler) share: the caller-owned state,
// the sampler's arguments and the two launch sequences of a tick.
#pragma once
#include "gpt.h"

namespace at {

struct Allow {
    int on;
    int lo0, hi0, lo1, hi1;   // ids in [lo0, hi0) or [lo1, hi1) are allowed
};
// The sampler's rule for one cache row while a window runs in it: which row of the caller's arrays it is, where in that row's stream its step 0 lies (out_ids,
// uniforms and logits_out are indexed by stream position), how many steps it has, what it may produce on even / odd steps and which id stops it (-1: none).
// out_org / u_org: the stream position of element 0 of the row's out_ids (and logits_out) and of its uniforms: 0 everywhere but in a stream pool
// (DESIGN.md 26), whose streams stand at different positions in one call.
struct SampleRow {
    int out_row, base, budget, stop_token, final_window, out_org, u_org;
    Allow allow[2];
};

// The caller-owned state: K / V for `rows` cache rows of `cap` positions, activations for the `tokens` token rows of one pass (carve_state in gpt.hip)
struct GptState {
    int *len, *done, *cur, *step_ctr;   // per cache row: tokens in the cache, finish flag, last sampled id, steps sampled in its window so far
    SampleRow* rows;                    // per cache row
    int *last_row, *samp_slot;          // per sampling row of a pass: the token whose logits it draws from, and its cache row
    int *tok_row, *tok_pos, *tok_id;    // the pass's token list: cache row, position and id (tok_id shares h's memory: the embedding has read it before a layer writes h)
    float *x, *xn, *q, *h, *logits, *kc, *vc;   // xn: LayerNorm output / attention context, and at the end the head's rows
    size_t layer_stride;                // floats of one layer's K (or V) cache: rows * 12 * cap * 64
    int cap;
    size_t bytes;
};

// The cache rows whose step tokens lead a pass's list, by value: the embedding resolves them itself (the row's last sampled id at position len - 1)
struct StepSlots {
    int n;
    unsigned char slot[GPT_MAX_B];
};

struct SampleArgs {
    const float* logits;      // [sampling rows][V]
    int V, top_k;
    float temperature;
    const float* uniforms;    // the op alone: [B]; generation: the draw of stream position p of caller's row o is uniforms[o * u_stride + p]
    int u_stride;
    // the op alone (at_op_topk_sample): out[b] = token, from the call's allow set
    int* out;
    Allow allow;
    // generation (out == nullptr): workgroup j samples for cache row samp_slot[j] from logits row j, by that row's SampleRow at that row's own step
    int *len, *done, *cur, *step_ctr;
    const SampleRow* rows;
    const int* samp_slot;
    int *out_ids, *out_len, *finish;
    float* logits_out;        // nullable [caller's rows][out_stride][V]
    int max_new, block, out_stride;
    // truncation: the nucleus' mass (1: off) and log(min_p) rounded to fp32 (-inf: off). With both off and no kept_out / thresh_out the
    // launch is the sampler as it was before truncation existed.
    float top_p = 1.0f, lmin = -__builtin_huge_valf();
    // the op alone (at_op_nucleus_sample): the final kept count and threshold value of row b
    int* kept_out = nullptr;
    float* thresh_out = nullptr;
};

int check_allow(const int32_t* r, int V, Allow* out);
int check_sampling(float temperature, int top_k);
// top_p in (0, 1] and min_p in [0, 1), neither NaN; *lmin = float32(log(min_p)) computed in double and rounded once, -inf for 0
int check_truncation(float top_p, float min_p, float* lmin);

// One pass of the model over the R tokens of the state's list: the `steps.n` step tokens, which the embedding resolves, then the prompt tokens the begin
// kernel wrote; then the head for the `ns` sampling rows that s.last_row names. An id outside [0, V) is clamped and reported in bit 0 of *status.
// with_head = false ends after the last layer and leaves the residual stream in s.x: the scorer applies the head itself, to every scored position.
int gpt_forward(const at_gpt* h, const GptState& s, const StepSlots& steps, int ns, int R, int* status, hipStream_t stream, bool with_head = true);
int gpt_sample(const SampleArgs& a, int rows, hipStream_t stream);
// The final LayerNorm alone (gpt_ln_kernel with ln_f): y[r] = LN(x[gather[r]]) for n rows
int gpt_final_ln(const at_gpt* h, const float* x, const int* gather, float* y, int n, hipStream_t stream);

// Teacher-forced scoring (gpt_score.hip): workgroup j scores logits row j against targets[j] under allow[parity ? parity[j] & 1 : 0] and
// writes logprob / rank (and the row itself into logits_out, when given) at index out_index ? out_index[j] : j.
struct ScoreArgs {
    const float* logits;      // [rows][V]
    int V;
    float temperature;
    const int *targets, *parity, *out_index;
    Allow allow[2];
    float* logprob;
    int* rank;
    float* logits_out;        // nullable [.][V]
};
int gpt_score_rows(const ScoreArgs& a, int rows, hipStream_t stream);

}  // namespace at
