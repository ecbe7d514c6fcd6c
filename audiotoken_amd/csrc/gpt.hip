// The semantic-to-acoustic decoder's first stage: the handle of the KV-cached GPT and its three generators. All three drive one
// tick (run_tick): gpt_begin_kernel for the cache rows in which a prompt begins, then the model pass over the tick's token list and the sampler
// (gpt_model.hip). A tick's list is one step token of every stepping row, then the whole prompt of every beginning one. The generators differ in their
// schedules and in when the host looks at the rows' flags:
//   at_gpt_generate        the caller's prompts begin in tick 0, then every row steps; a look every 16 steps
//   at_gpt_generate_long   lockstep passes: window k of every row that has one begins, then those rows step
//   at_gpt_generate_queue  GptQueueSchedule's ticks: any mix of rows that step and windows that begin
//   at_gpt_stream_push     one source whose ids arrive in pushes: GptStreamSchedule's rounds of windows
//   at_gpt_pool_push       many such sources in one call: GptPoolSchedule's rounds, each round the queue's ticks over the streams' windows
// Nothing waits for the host between those looks: the rows' lengths, last tokens, step counters and finish flags live on the device.
// The host side: the handle's plumbing and the state carver are model_handle.h's; the windowed entry points fill one GenRequest, which generate_long and
// generate_queue take and check_request checks; the lockstep generators' step loop is run_steps (at_gpt_generate, a pass of the long form, a stream window).
#include <cmath>
#include <cstring>

#include "../../include/audiotoken_hip.h"
#include "gpt_kernels.h"

using namespace at;

namespace {

constexpr int E = GPT_EMBD, HD = GPT_HEAD_DIM, NH = GPT_HEADS, FF = GPT_FF;

GptState carve_state(void* base, int rows, int cap, int tokens, int vocab, int n_layer) {
    GptState s{};
    StateCarver c(base);
    const size_t R = (size_t)tokens;
    s.len = c.take<int>(GPT_MAX_B);
    s.done = c.take<int>(GPT_MAX_B);
    s.cur = c.take<int>(GPT_MAX_B);
    s.step_ctr = c.take<int>(GPT_MAX_B);
    s.last_row = c.take<int>(GPT_MAX_B);
    s.samp_slot = c.take<int>(GPT_MAX_B);
    s.rows = c.take<SampleRow>(rows);
    s.tok_row = c.take<int>(R);
    s.tok_pos = c.take<int>(R);
    s.x = c.take<float>(R * E);
    s.xn = c.take<float>(R * E);
    s.q = c.take<float>(R * 3 * E);      // up to 64 tokens: q [R][768]; more, on the GEMM: q | k | v [R][2304]
    s.h = c.take<float>(R * FF);
    s.tok_id = (int*)s.h;                // [R]: written by the begin kernel, read by the embedding, dead before the first layer's MLP writes h
    s.logits = c.take<float>((size_t)rows * vocab);
    s.layer_stride = (size_t)rows * cap * NH * HD;
    s.kc = c.take<float>(s.layer_stride * n_layer);
    s.vc = c.take<float>(s.layer_stride * n_layer);
    s.cap = cap;
    s.bytes = c.off;
    return s;
}

// ---- a tick --------------------------------------------------------------------------------------------------------------------------------
// What a call fixes for all its ticks: where prompts come from and the rules of the windows that begin
struct Rules {
    const int* src;                  // [.][src_stride]: source ids (the prompt is ids + semantic_offset, INFER, the carry), or with `raw` the prompt itself
    int src_stride, raw;
    int S, H, r, semantic_offset, semantic_vocab, infer_token, stop_token, max_new, block;
    Allow mid[2], last[2];           // even / odd steps of a non-final and of a final window
    int* status;
    // the voice prompt table, NULL without one: entry e has semantic ids vp_sem[e][vp_stride] and coarse codes vp_codes[e][2][vf_stride]
    const int *vp_sem, *vp_codes;
    int vp_stride, vf_stride, acoustic_offset, codebook_size;
};
struct TickPlan {
    StepSlots steps;                      // the list: steps.n step tokens, then the prompts; R tokens in all
    int n_start, R;
    int off[GPT_MAX_B + 1];               // start j's prompt tokens are the list's [off[j], off[j + 1]); off[0] = steps.n
    int src[GPT_MAX_B], k[GPT_MAX_B];     // start j: window k[j] of source src[j]
    unsigned char slot[GPT_MAX_B];        //          in cache row slot[j]
    unsigned short pv[GPT_MAX_B];         //          after a voice prompt of pv[j] ids (0: none),
    short entry[GPT_MAX_B];               //          entry[j] of the prompt table
    unsigned long long final_mask;        // bit j: start j is its source's last window
    // Per-row origins, all 0 outside a stream pool: start j's source id c is q.src[src[j] * src_stride + src_org[j] + c], and element 0
    // of its row of out_ids (and logits_out) and of its row of the uniforms lie at stream positions out_org[j] and u_org[j]
    int src_org[GPT_MAX_B], out_org[GPT_MAX_B], u_org[GPT_MAX_B];
    void start(int slot_, int src_, int k_, int P, bool final_window, int pv_ = 0, int entry_ = 0) {
        const int j = n_start++;
        if (j == 0) off[0] = steps.n;
        off[j + 1] = off[j] + P;
        src[j] = src_; k[j] = k_; slot[j] = (unsigned char)slot_; pv[j] = (unsigned short)pv_; entry[j] = (short)entry_;
        if (final_window) final_mask |= 1ull << j;
        R = off[j + 1];
    }
};
constexpr int GPT_MAX_VOICE_PROMPTS = 4096;   // entries of a prompt table: what TickPlan::entry holds (a prompt's length is below GPT_MAX_BLOCK)
// rows 0 .. B - 1 step: every tick of a lockstep generator after the one in which they began
TickPlan lockstep_steps(int B) {
    TickPlan p{};
    p.steps.n = p.R = B;
    for (int b = 0; b < B; ++b) p.steps.slot[b] = (unsigned char)b;
    return p;
}

// The rows that begin in a tick: prompt token i of the list (cache row, position, id: a source id + the offset, INFER, or a carry id out of the source's
// own stream, which the samplers before this launch wrote in stream order; with q.raw the caller's id as it is), and per row len / done / cur, a zeroed step
// counter, its entry of the sampling list and its rule for the sampler. A prompt that fills the block leaves no room for a new token: the row is born
// finished. A row either steps or begins in a tick, never both, and the step tokens are the embedding's, so no word is read by one thread and written
// by another. A source id outside [0, semantic_vocab) is clamped and reported in bit 0 of *status (a raw id: by the embedding, against the vocabulary).
// A start with a voice prompt (p.pv[j] ids of table entry p.entry[j]) walks the concatenated source: index c below pv is the prompt's id,
// above it src[c - pv]; a carry id at stream position sp below r pv is the prompt's code (sp & 1 its code book, sp >> 1 its frame; outside
// [0, codebook_size) clamped, bit 1 of *status), above it the row's own out_ids[sp - r pv]. The sampler's base is the result position.
// A start's origins (p.src_org, p.out_org, p.u_org) move where its row's source ids, output and draws begin; they are 0 everywhere but in a
// stream pool.
static_assert(sizeof(TickPlan) + sizeof(Rules) + sizeof(GptState) + 4 * sizeof(void*) <= 4096, "gpt_begin_kernel's arguments must stay under the launch limit");
__global__ void gpt_begin_kernel(TickPlan p, Rules q, GptState s, const int* out_ids, int out_stride, int* out_len, int* finish) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x, i = p.steps.n + t;
    if (i < p.R) {
        int j = 0;
        while (j + 1 < p.n_start && p.off[j + 1] <= i) ++j;
        const int b = p.src[j], k = p.k[j], pv = p.pv[j], carry = k > 0 ? q.r * (q.S - q.H) : q.r * pv;
        const int pos = i - p.off[j], P = p.off[j + 1] - p.off[j], n_src = q.raw ? P : P - 1 - carry;
        int id;
        if (pos < n_src) {
            const int c = k * q.H + pos;
            id = c < pv ? q.vp_sem[(size_t)p.entry[j] * q.vp_stride + c] : q.src[(int64_t)b * q.src_stride + p.src_org[j] + c - pv];
            if (!q.raw) {
                if (id < 0 || id >= q.semantic_vocab) {
                    if (q.status) atomicOr(q.status, 1);
                    id = min(max(id, 0), q.semantic_vocab - 1);
                }
                id += q.semantic_offset;
            }
        } else if (pos == n_src) {
            id = q.infer_token;
        } else {
            const int sp = q.r * k * q.H + (pos - n_src - 1);
            if (sp < q.r * pv) {
                id = q.vp_codes[((size_t)p.entry[j] * 2 + (sp & 1)) * q.vf_stride + (sp >> 1)];
                if (id < 0 || id >= q.codebook_size) {
                    if (q.status) atomicOr(q.status, 2);
                    id = min(max(id, 0), q.codebook_size - 1);
                }
                id += q.acoustic_offset + (sp & 1) * q.codebook_size;
            } else {
                id = out_ids[(int64_t)b * out_stride + sp - q.r * pv - p.out_org[j]];
            }
        }
        s.tok_row[i] = p.slot[j];
        s.tok_pos[i] = pos;
        s.tok_id[i] = id;
    }
    if (t < p.n_start) {
        const int P = p.off[t + 1] - p.off[t], b = p.src[t], k = p.k[t], slot = p.slot[t], carry = k > 0 ? q.r * (q.S - q.H) : q.r * p.pv[t];
        const bool last = (p.final_mask >> t) & 1ull;
        const int born = P >= q.block ? GPT_FINISH_BLOCK : GPT_RUNNING;
        s.len[slot] = P;
        s.done[slot] = born;
        s.cur[slot] = 0;
        s.step_ctr[slot] = 0;
        s.last_row[p.steps.n + t] = p.off[t + 1] - 1;
        s.samp_slot[p.steps.n + t] = slot;
        SampleRow w;
        w.out_row = b;
        w.base = q.r * k * q.H + carry - q.r * p.pv[t];
        w.budget = last ? min(q.max_new, q.block - P) : q.r * q.S - carry;
        w.stop_token = last ? q.stop_token : -1;
        w.final_window = last ? 1 : 0;
        w.out_org = p.out_org[t];
        w.u_org = p.u_org[t];
        w.allow[0] = last ? q.last[0] : q.mid[0];
        w.allow[1] = last ? q.last[1] : q.mid[1];
        s.rows[slot] = w;
        if (k == 0) { out_len[b] = 0; finish[b] = born; }
    }
}

// One tick: the begin kernel when rows begin, the model pass over the list, one sampler launch for every row with a token in it
int run_tick(const at_gpt* h, const GptState& s, const TickPlan& p, const Rules& q, const SampleArgs& sa, hipStream_t stream) {
    const int ns = p.steps.n + p.n_start;
    if (p.n_start > 0) {
        hipLaunchKernelGGL(gpt_begin_kernel, dim3((p.R - p.steps.n + 255) / 256), dim3(256), 0, stream, p, q, s, sa.out_ids, sa.out_stride, sa.out_len, sa.finish);
        AT_CHECK_HIP(hipGetLastError());
    }
    if (int rc = gpt_forward(h, s, p.steps, ns, p.R, q.status, stream)) return rc;
    return gpt_sample(sa, ns, stream);
}

// the host's look at the device: true when none of the first n rows' flags says running
int all_done(at_gpt* h, const GptState& s, int n, hipStream_t stream, bool* all) {
    AT_CHECK_HIP(hipMemcpyAsync(h->flags_host, s.done, n * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    AT_CHECK_HIP(hipStreamSynchronize(stream));
    *all = true;
    for (int j = 0; j < n; ++j) *all = *all && h->flags_host[j] != GPT_RUNNING;
    return 0;
}

// The step loop of the lockstep generators: the tick in which `begin`'s windows begin in cache rows 0 .. n_rows - 1, then step ticks of those rows, `steps`
// ticks in all. After every GPT_CHECK_EVERY ticks, from tick poll_from on and not after the last, the host looks at the rows' flags and ends the loop when
// none is running: its only look at the device. (poll_from = steps: never, which is right for windows that cannot end early.)
int run_steps(at_gpt* h, const GptState& s, const TickPlan& begin, int n_rows, int steps, int poll_from, const Rules& q, const SampleArgs& sa, hipStream_t stream) {
    const TickPlan step_plan = lockstep_steps(n_rows);
    for (int step = 0; step < steps; ++step) {
        if (int rc = run_tick(h, s, step == 0 ? begin : step_plan, q, sa, stream)) return rc;
        if ((step + 1) % GPT_CHECK_EVERY == 0 && step + 1 < steps && step + 1 >= poll_from) {
            bool all;
            if (int rc = all_done(h, s, n_rows, stream, &all)) return rc;
            if (all) break;
        }
    }
    return 0;
}

// ---- a call of the windowed generators, as its entry point hands it over ------------------------------------------------------------------------
struct Sources { const int32_t* dev; int stride; const int32_t* len; int n; };   // device ids [n][stride], HOST lengths
struct Geometry { int S, H, r; };
struct TokenSpace { int semantic_offset, semantic_vocab, infer_token, acoustic_offset, codebook_size, stop_token; };
struct Sampling { int max_new; float temperature; int top_k; const float* uniforms; int u_stride; };
struct Outputs { int32_t* ids; int stride; int32_t *len, *finish; float* logits; };
struct StateBuf { void* dev; size_t bytes; int max_len; };
struct QueueExtras { int slots, tick_tokens; int32_t* trace; int trace_cap; int32_t *n_ticks, *placement; };
// A call's voice prompts as the caller hands them over: the table on the device, the lengths and each source's entry (-1: none) on the host
struct VoiceTable {
    const int32_t* sem; int p_stride; const int32_t* codes; int f_stride; const int32_t* len; int n; const int32_t* of_src;
    bool on;   // a prompted entry point was called
};
struct GenRequest {
    const char* who;   // the entry point the caller called
    at_gpt* h;
    Sources src;
    Geometry geo;
    TokenSpace tok;
    Sampling samp;
    Outputs out;
    StateBuf state;
    at_stream_t stream;
    int32_t* status;
    VoiceTable voice;
    QueueExtras queue;
};

SampleArgs generation_args(const at_gpt* h, const GptState& s, const Sampling& g, const Outputs& o) {
    SampleArgs sa{};
    sa.logits = s.logits; sa.V = h->vocab; sa.top_k = g.top_k; sa.temperature = g.temperature; sa.uniforms = g.uniforms; sa.u_stride = g.u_stride;
    sa.len = s.len; sa.done = s.done; sa.cur = s.cur; sa.step_ctr = s.step_ctr; sa.rows = s.rows; sa.samp_slot = s.samp_slot;
    sa.out_ids = o.ids; sa.out_len = o.len; sa.finish = o.finish; sa.logits_out = o.logits; sa.max_new = g.max_new; sa.block = h->block; sa.out_stride = o.stride;
    sa.top_p = h->top_p; sa.lmin = h->lmin;
    return sa;
}

// the window geometry against the model's block size: what every windowed entry point and the stream's size query check first
int check_geometry(const at_gpt* h, const Geometry& g) {
    AT_REQUIRE(g.S >= 2 && g.S % 2 == 0 && g.H >= 2 && g.H % 2 == 0, "the window S and the hop H must be even, at least 2");
    AT_REQUIRE(g.H <= g.S, "the hop H must not exceed the window S");
    AT_REQUIRE(g.r >= 1 && g.r <= GPT_MAX_BLOCK, "r (acoustic ids per source id) must be 1 to 1024");
    AT_REQUIRE((int64_t)g.S + 1 + (int64_t)g.r * g.S <= h->block, "a window does not fit: S + 1 + r S must not exceed the model's block size");
    return 0;
}

// What the windowed generators and the stream share: the checks of the geometry, the token space and the sampling arguments, and the rules they make
int check_long_rules(const GenRequest& rq, Rules* out) {
    const int V = rq.h->vocab;
    const TokenSpace& t = rq.tok;
    if (int rc = check_geometry(rq.h, rq.geo)) return rc;
    AT_REQUIRE(rq.src.stride >= 1, "src_stride must be at least 1");
    AT_REQUIRE(rq.samp.max_new >= 1 && rq.samp.max_new <= GPT_MAX_BLOCK, "max_new must be 1 to 1024");
    if (int rc = check_sampling(rq.samp.temperature, rq.samp.top_k)) return rc;
    AT_REQUIRE(t.semantic_offset >= 0 && t.semantic_vocab >= 1 && (int64_t)t.semantic_offset + t.semantic_vocab <= V, "the semantic ids must lie inside the vocabulary");
    AT_REQUIRE(t.infer_token >= 0 && t.infer_token < V, "infer_token is not in the vocabulary");
    AT_REQUIRE(t.acoustic_offset >= 0 && t.codebook_size >= 1 && (int64_t)t.acoustic_offset + 2 * (int64_t)t.codebook_size <= V,
               "the two code books must lie inside the vocabulary");
    AT_REQUIRE(t.stop_token < V, "stop_token is not in the vocabulary (negative: none)");
    Rules q{};
    q.src = rq.src.dev; q.src_stride = rq.src.stride; q.status = rq.status;
    q.S = rq.geo.S; q.H = rq.geo.H; q.r = rq.geo.r; q.semantic_offset = t.semantic_offset; q.semantic_vocab = t.semantic_vocab; q.infer_token = t.infer_token;
    q.stop_token = t.stop_token < 0 ? -1 : t.stop_token; q.max_new = rq.samp.max_new; q.block = rq.h->block;
    q.acoustic_offset = t.acoustic_offset; q.codebook_size = t.codebook_size;
    q.mid[0] = Allow{1, t.acoustic_offset, t.acoustic_offset + t.codebook_size, 0, 0};
    q.mid[1] = Allow{1, t.acoustic_offset + t.codebook_size, t.acoustic_offset + 2 * t.codebook_size, 0, 0};
    q.last[0] = q.mid[0];
    q.last[1] = q.mid[1];
    if (t.stop_token >= 0) { q.last[0].lo1 = t.stop_token; q.last[0].hi1 = t.stop_token + 1; }
    q.vp_sem = rq.voice.sem; q.vp_codes = rq.voice.codes; q.vp_stride = rq.voice.p_stride; q.vf_stride = rq.voice.f_stride;
    *out = q;
    return 0;
}

// The sources' lengths (`unit`: what the entry point calls a source in its error texts), then the checks of a prompted call, and per source its prompt's
// length (0: none) and entry: pv and entry are left empty when no source has a prompt
int check_sources(const GenRequest& rq, const char* unit, std::vector<int32_t>* pv, std::vector<int32_t>* entry) {
    const char* who = rq.who;
    const VoiceTable& vt = rq.voice;
    const int32_t* src_len = rq.src.len;
    const int n_src = rq.src.n, S = rq.geo.S, H = rq.geo.H, r = rq.geo.r;
    for (int i = 0; i < n_src; ++i)
        if (src_len[i] < 1 || src_len[i] > rq.src.stride || src_len[i] > GPT_MAX_SOURCE) {
            set_error(std::string(who) + ": src_len of " + unit + " " + std::to_string(i) + " must be 1 to min(src_stride, 65536)");
            return -1;
        }
    if (!vt.on) return 0;
    AT_REQUIRE(vt.n >= 0 && vt.n <= GPT_MAX_VOICE_PROMPTS, "n_prompts must be 0 to 4096");
    AT_REQUIRE(vt.of_src != nullptr, "null prompt_of_src");
    AT_REQUIRE(vt.n == 0 || (vt.sem && vt.codes && vt.len), "null prompt table");
    AT_REQUIRE(vt.n == 0 || (vt.p_stride >= 1 && vt.f_stride >= 1), "p_stride and f_stride must be at least 1");
    for (int e = 0; e < vt.n; ++e) {
        const int P = vt.len[e];
        if (!(P >= 2 && P % 2 == 0 && P <= S - H)) {
            set_error(std::string(who) + ": the length of prompt " + std::to_string(e) + " must be even, 2 to S - H");
            return -1;
        }
        if (P > vt.p_stride || (int64_t)r * P / 2 > vt.f_stride) {
            set_error(std::string(who) + ": prompt " + std::to_string(e) + " does not fit p_stride ids and f_stride frames (r P / 2)");
            return -1;
        }
    }
    bool any = false;
    for (int i = 0; i < n_src; ++i) {
        const int e = vt.of_src[i];
        if (e < -1 || e >= vt.n) {
            set_error(std::string(who) + ": prompt_of_src of source " + std::to_string(i) + " must be -1 or an entry of the table");
            return -1;
        }
        if (e >= 0 && !gpt_voice_prompt_ok(vt.len[e], src_len[i], S, H)) {
            set_error(std::string(who) + ": source " + std::to_string(i) + " with its prompt exceeds 65536 ids");
            return -1;
        }
        any = any || e >= 0;
    }
    if (!any) return 0;
    pv->assign(n_src, 0);
    entry->assign(n_src, 0);
    for (int i = 0; i < n_src; ++i)
        if (vt.of_src[i] >= 0) { (*pv)[i] = vt.len[vt.of_src[i]]; (*entry)[i] = vt.of_src[i]; }
    return 0;
}

int upload(at_gpt* h, const std::string& name, std::vector<int64_t> shape, const float** dst) { return upload_staged(h, "at_gpt_finalize", name, shape, dst); }

void release(at_gpt* h) {
    free_allocs(h);
    if (h->flags_host) { (void)hipHostFree(h->flags_host); h->flags_host = nullptr; }
    h->layers.clear();
    h->wte = h->wpe = h->ln_f = nullptr;
}

}  // namespace

extern "C" {

at_gpt_t* at_gpt_create(int device_id) {
    if (!device_exists("at_gpt_create", device_id)) return nullptr;
    at_gpt* h = new at_gpt();
    h->device = device_id;
    return h;
}

int at_gpt_set_tensor(at_gpt_t* h, const char* name, const float* host_data, const int64_t* shape, int ndim) {
    return stage_model_tensor(h, name, host_data, shape, ndim);
}

int at_gpt_finalize(at_gpt_t* h) {
    AT_REQUIRE(h != nullptr, "null handle");
    AT_REQUIRE(!h->finalized, "model already finalized");
    for (const auto& kv : h->staged)
        if (kv.first.size() > 5 && kv.first.compare(kv.first.size() - 5, 5, ".bias") == 0) {
            set_error("at_gpt_finalize: " + kv.first + ": the kernels implement the bias-free model only");
            return -1;
        }
    const HostTensor* wte = staged_tensor(h, "transformer.wte.weight");
    const HostTensor* wpe = staged_tensor(h, "transformer.wpe.weight");
    AT_REQUIRE(wte && wpe, "transformer.wte.weight and transformer.wpe.weight are needed");
    AT_REQUIRE(wte->shape.size() == 2 && wpe->shape.size() == 2 && wte->shape[1] == E && wpe->shape[1] == E, "n_embd must be 768 (12 heads of 64): what the kernels implement");
    const int64_t V = wte->shape[0], block = wpe->shape[0];
    AT_REQUIRE(V >= 64 && V % 64 == 0 && V <= GPT_MAX_VOCAB, "the vocabulary must be a multiple of 64, at most 65536");
    AT_REQUIRE(block >= 64 && block % 64 == 0 && block <= GPT_MAX_BLOCK, "the block size must be a multiple of 64, at most 1024");
    int n_layer = 0;
    while (staged_tensor(h, "transformer.h." + std::to_string(n_layer) + ".ln_1.weight")) ++n_layer;
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

int at_gpt_set_truncation(at_gpt_t* h, float top_p, float min_p) {
    AT_REQUIRE(h != nullptr, "null handle");
    float lmin;
    if (int rc = check_truncation(top_p, min_p, &lmin)) return rc;   // a refused call leaves the handle as it was
    h->top_p = top_p;
    h->lmin = lmin;
    return 0;
}

// the size of a lockstep generator's state, behind its two names: `who` is the entry point the caller called
static size_t lockstep_state_bytes(const char* who, const at_gpt_t* h, int B, int max_len) {
    const std::string w(who);
    if (!(h && h->finalized)) { set_error(w + ": the model is not finalized"); return 0; }
    if (!(B >= 1 && B <= GPT_MAX_B)) { set_error(w + ": B must be 1 to 64"); return 0; }
    if (!(max_len >= 1 && max_len <= h->block)) { set_error(w + ": max_len must be 1 to the model's block size"); return 0; }
    return carve_state(nullptr, B, max_len, B * max_len, h->vocab, h->n_layer).bytes;
}
size_t at_gpt_state_bytes(const at_gpt_t* h, int B, int max_len) { return lockstep_state_bytes("at_gpt_state_bytes", h, B, max_len); }
size_t at_gpt_long_state_bytes(const at_gpt_t* h, int B, int max_len) { return lockstep_state_bytes("at_gpt_long_state_bytes", h, B, max_len); }

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
    // ---- tick 0: every row's prompt begins in its own cache row, as a source's only window would
    TickPlan begin{};
    int longest = 0;
    for (int b = 0; b < B; ++b) {
        if (prompt_len[b] > h->block) { set_error("at_gpt_generate: prompt of row " + std::to_string(b) + " is longer than the model's block size"); return -1; }
        if (prompt_len[b] < 1 || prompt_len[b] > prompt_stride) { set_error("at_gpt_generate: prompt_len of row " + std::to_string(b) + " must be 1 to prompt_stride"); return -1; }
        begin.start(b, b, 0, prompt_len[b], true);
        longest = prompt_len[b] > longest ? prompt_len[b] : longest;
    }
    const int need_len = longest + max_new < h->block ? longest + max_new : h->block;
    AT_REQUIRE(max_len >= need_len && max_len <= h->block, "max_len must hold the longest prompt and max_new (or the block size) and not exceed the block size");
    Rules q{};
    q.src = prompts_dev; q.src_stride = prompt_stride; q.raw = 1; q.status = status_dev;
    q.stop_token = stop_token < 0 ? -1 : stop_token; q.max_new = max_new; q.block = h->block;
    if (int rc = check_allow(allow, h->vocab, &q.last[0])) return rc;
    if (int rc = check_allow(allow ? allow + 4 : nullptr, h->vocab, &q.last[1])) return rc;
    const GptState s = carve_state(state_dev, B, max_len, B * max_len, h->vocab, h->n_layer);
    AT_REQUIRE(state_bytes >= s.bytes, "state too small: at_gpt_state_bytes(h, B, max_len)");
    // ---- nothing above touched the device
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    hipStream_t stream = (hipStream_t)stream_;
    const SampleArgs sa = generation_args(h, s, Sampling{max_new, temperature, top_k, uniforms_dev, max_new}, Outputs{out_ids_dev, max_new, out_len_dev, finish_dev, logits_out_dev});
    return run_steps(h, s, begin, B, max_new, 0, q, sa, stream);
}

int at_gpt_long_num_windows(int N, int S, int H) {
    if (!(S >= 2 && S % 2 == 0 && H >= 2 && H % 2 == 0 && H <= S && N >= 1 && N <= GPT_MAX_SOURCE)) {
        set_error("at_gpt_long_num_windows: S and H must be even with 2 <= H <= S, N 1 to 65536");
        return 0;
    }
    return gpt_long_windows(N, S, H);
}

int at_gpt_long_num_windows_prompted(int P, int N, int S, int H) {
    if (!(S >= 2 && S % 2 == 0 && H >= 2 && H % 2 == 0 && H <= S && gpt_voice_prompt_ok(P, N, S, H))) {
        set_error("at_gpt_long_num_windows_prompted: S and H must be even with 2 <= H <= S, P even with 2 <= P <= S - H, N at least 1, P + N at most 65536");
        return 0;
    }
    return gpt_long_windows(N, S, H, P);
}

// What at_gpt_generate_long and at_gpt_generate_queue check alike once the counts are known to be in range, in this order: the pointers, the rules, the
// sources with their voice prompts, and the caller's arrays against the sources' extent. `unit`: what the entry point calls a source in its error texts.
static int check_request(const GenRequest& rq, const char* unit, Rules* q, std::vector<int32_t>* pv, std::vector<int32_t>* entry) {
    AT_REQUIRE(rq.src.dev && rq.src.len && rq.samp.uniforms && rq.out.ids && rq.out.len && rq.out.finish, "null pointer");
    AT_REQUIRE(rq.state.dev != nullptr, "null state");
    AT_REQUIRE(rq.queue.trace_cap >= 0 && (rq.queue.trace != nullptr || rq.queue.trace_cap == 0), "trace_cap must be 0 without a trace and never negative");
    if (int rc = check_long_rules(rq, q)) return rc;
    if (int rc = check_sources(rq, unit, pv, entry)) return rc;
    const auto [need_len, need_stride] = gpt_extent(rq.src.len, rq.src.n, rq.geo.S, rq.geo.H, rq.geo.r, rq.samp.max_new, rq.h->block, pv->empty() ? nullptr : pv->data());
    AT_REQUIRE(rq.out.stride >= need_stride && rq.samp.u_stride >= need_stride, std::string("out_stride and u_stride must hold the longest ") + unit + "'s stream");
    AT_REQUIRE(rq.state.max_len >= need_len && rq.state.max_len <= rq.h->block, "max_len must hold the longest window with its new ids and not exceed the block size");
    return 0;
}

static int generate_long(const GenRequest& rq) {
    at_gpt* h = rq.h;
    const int B = rq.src.n, S = rq.geo.S, H = rq.geo.H, r = rq.geo.r, max_new = rq.samp.max_new;
    AT_REQUIRE(h && h->finalized, "the model is not finalized");
    AT_REQUIRE(B >= 1 && B <= GPT_MAX_B, "B must be 1 to 64");
    Rules q{};
    std::vector<int32_t> pv, entry;
    if (int rc = check_request(rq, "row", &q, &pv, &entry)) return rc;
    const bool voiced = !pv.empty();
    // ---- the schedule: rows in descending order of their window counts, so that the rows of pass k are the first Bk of them
    int n_win[GPT_MAX_B], order[GPT_MAX_B];
    int n_max = 0;
    for (int b = 0; b < B; ++b) {
        const int n = n_win[b] = gpt_long_windows(rq.src.len[b], S, H, voiced ? pv[b] : 0);
        n_max = n > n_max ? n : n_max;
        int at = b;
        while (at > 0 && n_win[order[at - 1]] < n) { order[at] = order[at - 1]; --at; }
        order[at] = b;
    }
    const GptState s = carve_state(rq.state.dev, B, rq.state.max_len, B * rq.state.max_len, h->vocab, h->n_layer);
    AT_REQUIRE(rq.state.bytes >= s.bytes, "state too small: at_gpt_long_state_bytes(h, B, max_len)");
    // ---- nothing above touched the device
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    hipStream_t stream = (hipStream_t)rq.stream;
    const SampleArgs sa = generation_args(h, s, rq.samp, rq.out);
    for (int k = 0; k < n_max; ++k) {
        // pass k: window k of every row that has one begins in cache row 0 .. Bk - 1, then those rows step up to the largest budget among them
        TickPlan begin{};
        int Bk = 0, steps = 0, mid_steps = 0;
        while (Bk < B && n_win[order[Bk]] > k) {
            const int b = order[Bk];
            const GptWindow w = gpt_window(rq.src.len[b], k, S, H, r, max_new, h->block, voiced ? pv[b] : 0);
            begin.start(Bk, b, k, w.P, w.final_window, voiced ? pv[b] : 0, voiced ? entry[b] : 0);
            if (!w.final_window) mid_steps = w.budget > mid_steps ? w.budget : mid_steps;
            steps = w.budget > steps ? w.budget : steps;
            ++Bk;
        }
        // a non-final window never ends early, so there is nothing to see before the last of them is complete
        if (int rc = run_steps(h, s, begin, Bk, steps, mid_steps, q, sa, stream)) return rc;
    }
    return 0;
}

int at_gpt_generate_long(at_gpt_t* h, const int32_t* src_dev, int src_stride, const int32_t* src_len, int B, int S, int H, int r, int semantic_offset,
                         int semantic_vocab, int infer_token, int acoustic_offset, int codebook_size, int stop_token, int max_new, float temperature, int top_k,
                         const float* uniforms_dev, int u_stride, int32_t* out_ids_dev, int out_stride, int32_t* out_len_dev, int32_t* finish_dev,
                         float* logits_out_dev, void* state_dev, size_t state_bytes, int max_len, at_stream_t stream, int32_t* status_dev) {
    return generate_long(GenRequest{"at_gpt_generate_long", h, {src_dev, src_stride, src_len, B}, {S, H, r},
                                    {semantic_offset, semantic_vocab, infer_token, acoustic_offset, codebook_size, stop_token},
                                    {max_new, temperature, top_k, uniforms_dev, u_stride}, {out_ids_dev, out_stride, out_len_dev, finish_dev, logits_out_dev},
                                    {state_dev, state_bytes, max_len}, stream, status_dev});
}

int at_gpt_generate_long_prompted(at_gpt_t* h, const int32_t* src_dev, int src_stride, const int32_t* src_len, int B, const int32_t* prompt_sem_dev, int p_stride,
                                  const int32_t* prompt_codes_dev, int f_stride, const int32_t* prompt_len, int n_prompts, const int32_t* prompt_of_src, int S, int H,
                                  int r, int semantic_offset, int semantic_vocab, int infer_token, int acoustic_offset, int codebook_size, int stop_token, int max_new,
                                  float temperature, int top_k, const float* uniforms_dev, int u_stride, int32_t* out_ids_dev, int out_stride, int32_t* out_len_dev,
                                  int32_t* finish_dev, float* logits_out_dev, void* state_dev, size_t state_bytes, int max_len, at_stream_t stream, int32_t* status_dev) {
    return generate_long(GenRequest{"at_gpt_generate_long_prompted", h, {src_dev, src_stride, src_len, B}, {S, H, r},
                                    {semantic_offset, semantic_vocab, infer_token, acoustic_offset, codebook_size, stop_token},
                                    {max_new, temperature, top_k, uniforms_dev, u_stride}, {out_ids_dev, out_stride, out_len_dev, finish_dev, logits_out_dev},
                                    {state_dev, state_bytes, max_len}, stream, status_dev,
                                    {prompt_sem_dev, p_stride, prompt_codes_dev, f_stride, prompt_len, n_prompts, prompt_of_src, true}});
}

size_t at_gpt_queue_state_bytes(const at_gpt_t* h, int slots, int max_len, int tick_tokens) {
    if (!(h && h->finalized)) { set_error("at_gpt_queue_state_bytes: the model is not finalized"); return 0; }
    if (!(slots >= 1 && slots <= GPT_MAX_B)) { set_error("at_gpt_queue_state_bytes: slots must be 1 to 64"); return 0; }
    if (!(max_len >= 1 && max_len <= h->block)) { set_error("at_gpt_queue_state_bytes: max_len must be 1 to the model's block size"); return 0; }
    if (!(tick_tokens >= slots + max_len && tick_tokens <= GPT_MAX_TICK_TOKENS)) {
        set_error("at_gpt_queue_state_bytes: tick_tokens must be slots + max_len to " + std::to_string(GPT_MAX_TICK_TOKENS));
        return 0;
    }
    return carve_state(nullptr, slots, max_len, tick_tokens, h->vocab, h->n_layer).bytes;
}

static int generate_queue(const GenRequest& rq) {
    at_gpt* h = rq.h;
    const QueueExtras& x = rq.queue;
    const int n_src = rq.src.n, slots = x.slots, tick_tokens = x.tick_tokens, max_len = rq.state.max_len;
    AT_REQUIRE(h && h->finalized, "the model is not finalized");
    AT_REQUIRE(n_src >= 1 && n_src <= GPT_MAX_QUEUE, "n_src must be 1 to 4096");
    AT_REQUIRE(slots >= 1 && slots <= GPT_MAX_B, "slots must be 1 to 64");
    Rules q{};
    std::vector<int32_t> pv, entry;
    if (int rc = check_request(rq, "source", &q, &pv, &entry)) return rc;
    const bool voiced = !pv.empty();
    AT_REQUIRE(tick_tokens >= slots + max_len && tick_tokens <= GPT_MAX_TICK_TOKENS, "tick_tokens must be at least slots + max_len (one window always fits) and at most 65600");
    const GptState s = carve_state(rq.state.dev, slots, max_len, tick_tokens, h->vocab, h->n_layer);
    AT_REQUIRE(rq.state.bytes >= s.bytes, "state too small: at_gpt_queue_state_bytes(h, slots, max_len, tick_tokens)");
    // ---- nothing above touched the device
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    hipStream_t stream = (hipStream_t)rq.stream;
    const SampleArgs sa = generation_args(h, s, rq.samp, rq.out);
    GptQueueSchedule schedule(rq.src.len, n_src, rq.geo.S, rq.geo.H, rq.geo.r, rq.samp.max_new, h->block, slots, tick_tokens, voiced ? pv.data() : nullptr);
    GptQueueTick t;
    while (schedule.next(&t)) {
        TickPlan p{};
        p.steps.n = p.R = t.n_step;
        for (int i = 0; i < t.n_step; ++i) p.steps.slot[i] = (unsigned char)t.step_slot[i];
        for (int j = 0; j < t.n_start; ++j) {
            const GptQueueStart& st = t.start[j];
            p.start(st.slot, st.src, st.k, st.P, st.final_window != 0, voiced ? pv[st.src] : 0, voiced ? entry[st.src] : 0);
        }
        if (int rc = run_tick(h, s, p, q, sa, stream)) return rc;
        const int at = schedule.ticks() - 1;
        if (at < x.trace_cap) {   // a trace too small loses its tail, the run goes on
            int32_t* row = x.trace + 4 * (size_t)at;
            row[0] = t.n_step; row[1] = t.n_start; row[2] = t.prefill_tokens; row[3] = t.route();
        }
        if (t.poll) {   // the host's only look at the device: some slot is in a final window, and when that ends only the device knows
            AT_CHECK_HIP(hipMemcpyAsync(h->flags_host, s.done, slots * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
            AT_CHECK_HIP(hipStreamSynchronize(stream));
            schedule.seen(h->flags_host);
        }
    }
    if (x.n_ticks) *x.n_ticks = schedule.ticks();
    if (x.placement) std::memcpy(x.placement, schedule.placement().data(), (size_t)n_src * 3 * sizeof(int32_t));
    return 0;
}

int at_gpt_generate_queue(at_gpt_t* h, const int32_t* src_dev, int src_stride, const int32_t* src_len, int n_src, int S, int H, int r, int semantic_offset,
                          int semantic_vocab, int infer_token, int acoustic_offset, int codebook_size, int stop_token, int max_new, float temperature, int top_k,
                          const float* uniforms_dev, int u_stride, int32_t* out_ids_dev, int out_stride, int32_t* out_len_dev, int32_t* finish_dev,
                          float* logits_out_dev, void* state_dev, size_t state_bytes, int max_len, int slots, int tick_tokens, int32_t* trace, int trace_cap,
                          int32_t* n_ticks, int32_t* placement, at_stream_t stream, int32_t* status_dev) {
    return generate_queue(GenRequest{"at_gpt_generate_queue", h, {src_dev, src_stride, src_len, n_src}, {S, H, r},
                                     {semantic_offset, semantic_vocab, infer_token, acoustic_offset, codebook_size, stop_token},
                                     {max_new, temperature, top_k, uniforms_dev, u_stride}, {out_ids_dev, out_stride, out_len_dev, finish_dev, logits_out_dev},
                                     {state_dev, state_bytes, max_len}, stream, status_dev, {}, {slots, tick_tokens, trace, trace_cap, n_ticks, placement}});
}

int at_gpt_generate_queue_prompted(at_gpt_t* h, const int32_t* src_dev, int src_stride, const int32_t* src_len, int n_src, const int32_t* prompt_sem_dev, int p_stride,
                                   const int32_t* prompt_codes_dev, int f_stride, const int32_t* prompt_len, int n_prompts, const int32_t* prompt_of_src, int S, int H,
                                   int r, int semantic_offset, int semantic_vocab, int infer_token, int acoustic_offset, int codebook_size, int stop_token, int max_new,
                                   float temperature, int top_k, const float* uniforms_dev, int u_stride, int32_t* out_ids_dev, int out_stride, int32_t* out_len_dev,
                                   int32_t* finish_dev, float* logits_out_dev, void* state_dev, size_t state_bytes, int max_len, int slots, int tick_tokens,
                                   int32_t* trace, int trace_cap, int32_t* n_ticks, int32_t* placement, at_stream_t stream, int32_t* status_dev) {
    return generate_queue(GenRequest{"at_gpt_generate_queue_prompted", h, {src_dev, src_stride, src_len, n_src}, {S, H, r},
                                     {semantic_offset, semantic_vocab, infer_token, acoustic_offset, codebook_size, stop_token},
                                     {max_new, temperature, top_k, uniforms_dev, u_stride}, {out_ids_dev, out_stride, out_len_dev, finish_dev, logits_out_dev},
                                     {state_dev, state_bytes, max_len}, stream, status_dev,
                                     {prompt_sem_dev, p_stride, prompt_codes_dev, f_stride, prompt_len, n_prompts, prompt_of_src, true},
                                     {slots, tick_tokens, trace, trace_cap, n_ticks, placement}});
}

}  // extern "C"

// ---- the stream: one source whose ids arrive in pushes ------------------------------------------------------------------------
namespace {

// The stream's own buffers behind the one-row generation state: the source ids no window has left behind (2 S), and the last r (S - H) stream ids
struct GptStreamState {
    GptState g;
    int *src, *carry;
    size_t bytes;
};
GptStreamState carve_stream(void* base, const at_gpt* h, int S, int H, int r) {
    GptStreamState st{};
    st.g = carve_state(base, 1, h->block, h->block, h->vocab, h->n_layer);
    StateCarver c(base, st.g.bytes);
    st.src = c.take<int>((size_t)2 * S);
    st.carry = c.take<int>((size_t)r * (S - H) + 1);
    st.bytes = c.off;
    return st;
}

// buf[0 .. n) = buf[shift .. shift + n): one workgroup, every id read before any is written (n is at most 2 S <= 1024)
__global__ __launch_bounds__(1024) void gpt_stream_shift_kernel(int* buf, int shift, int n) {
    const int t = threadIdx.x;
    const int v = t < n ? buf[shift + t] : 0;
    __syncthreads();
    if (t < n) buf[t] = v;
}

}  // namespace

extern "C" {

size_t at_gpt_stream_state_bytes(const at_gpt_t* h, int S, int H, int r) {
    if (!(h && h->finalized)) { set_error("at_gpt_stream_state_bytes: the model is not finalized"); return 0; }
    if (check_geometry(h, Geometry{S, H, r})) return 0;
    return carve_stream(nullptr, h, S, H, r).bytes;
}

int at_gpt_stream_push(at_gpt_t* h, void* state_dev, size_t state_bytes, int64_t* pos, const int32_t* ids_dev, int n_new, int final, int S, int H, int r,
                       int semantic_offset, int semantic_vocab, int infer_token, int acoustic_offset, int codebook_size, int stop_token, int max_new,
                       float temperature, int top_k, const float* uniforms_dev, int64_t u_pos0, int64_t u_len, int32_t* out_ids_dev, int out_cap,
                       int32_t* out_len_dev, int32_t* finish_dev, int32_t* windows_run, at_stream_t stream_, int32_t* status_dev) {
    AT_REQUIRE(h && h->finalized, "the model is not finalized");
    AT_REQUIRE(state_dev != nullptr, "null state");
    AT_REQUIRE(pos && uniforms_dev && out_ids_dev && out_len_dev && finish_dev, "null pointer");
    AT_REQUIRE(final == 0 || final == 1, "final must be 0 or 1");
    AT_REQUIRE(n_new >= 0 && (ids_dev != nullptr || n_new == 0), "n_new must not be negative, and ids need a pointer");
    AT_REQUIRE(pos[1] == 0, "the stream is finished: a push after the final call");
    AT_REQUIRE(pos[0] >= 0 && pos[0] + n_new <= GPT_MAX_SOURCE, "a stream takes at most 65536 ids");
    AT_REQUIRE(!final || pos[0] + n_new >= 1, "a final call with nothing pushed");
    const int block = h->block;
    Rules q{};
    // one source of stride 1; the sampler's view of the caller's arrays replaces them below, once the geometry is known to be sound
    GenRequest rq{"at_gpt_stream_push", h, {ids_dev, 1, nullptr, 1}, {S, H, r}, {semantic_offset, semantic_vocab, infer_token, acoustic_offset, codebook_size, stop_token},
                        {max_new, temperature, top_k, uniforms_dev, 0}, {out_ids_dev, 0, out_len_dev, finish_dev, nullptr}, {state_dev, state_bytes, block}, stream_, status_dev};
    if (int rc = check_long_rules(rq, &q)) return rc;
    AT_REQUIRE(u_pos0 >= 0 && u_len >= 0 && out_cap >= 0, "u_pos0, u_len and out_cap must not be negative");
    // ---- the windows this call runs and what they need of the caller's arrays
    const int k0 = gpt_stream_windows_run(pos[0], S, H), k1 = gpt_stream_windows_run(pos[0] + n_new, S, H);
    const int carry = r * (S - H);
    const int64_t p_base = k0 > 0 ? (int64_t)r * k0 * H : 0;   // the stream position of out_ids_dev[0]
    if (k1 > k0 || final) {
        const int64_t N = pos[0] + n_new;
        const GptWindow first = gpt_window((int)(final && k0 == k1 ? N : (int64_t)k0 * H + S + 1), k0, S, H, r, max_new, block);
        const GptWindow last = gpt_window((int)(final ? N : (int64_t)(k1 - 1) * H + S + 1), final ? k1 : k1 - 1, S, H, r, max_new, block);
        const int64_t end = (int64_t)last.stream_base + last.budget;
        AT_REQUIRE(first.stream_base >= u_pos0 && end <= u_pos0 + u_len, "the uniforms do not cover the stream positions this call draws");
        AT_REQUIRE(end - p_base <= out_cap, "out_cap must hold the carry and the ids this call can produce");
    }
    const GptStreamState st = carve_stream(state_dev, h, S, H, r);
    AT_REQUIRE(state_bytes >= st.bytes, "state too small: at_gpt_stream_state_bytes(h, S, H, r)");
    // ---- nothing above touched the device
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    hipStream_t stream = (hipStream_t)stream_;
    // the sampler and the begin kernel index the stream by absolute position: the call's arrays are addressed from the position of their first element
    int32_t* out_abs = reinterpret_cast<int32_t*>(reinterpret_cast<intptr_t>(out_ids_dev) - (intptr_t)p_base * 4);
    const float* u_abs = reinterpret_cast<const float*>(reinterpret_cast<intptr_t>(uniforms_dev) - (intptr_t)u_pos0 * 4);
    rq.samp.uniforms = u_abs;
    rq.out.ids = out_abs;
    const SampleArgs sa = generation_args(h, st.g, rq.samp, rq.out);
    if ((k1 > k0 || final) && k0 > 0) AT_CHECK_HIP(hipMemcpyAsync(out_ids_dev, st.carry, (size_t)carry * 4, hipMemcpyDeviceToDevice, stream));
    auto run_window = [&](int k, int n_src_ids, bool last) -> int {
        const GptWindow w = gpt_window(last ? k * H + n_src_ids : k * H + S + 1, k, S, H, r, max_new, block);
        TickPlan begin{};
        begin.start(0, 0, k, w.P, last);
        return run_steps(h, st.g, begin, 1, w.budget, last ? 0 : w.budget, q, sa, stream);   // only the final window's flag is worth a look
    };
    GptStreamSchedule schedule(pos[0], n_new, final != 0, S, H);
    GptStreamRound rd;
    int taken = 0, ran = 0;
    while (schedule.next(&rd)) {
        if (rd.take > 0) AT_CHECK_HIP(hipMemcpyAsync(st.src + rd.held, ids_dev + taken, (size_t)rd.take * 4, hipMemcpyDeviceToDevice, stream));
        taken += rd.take;
        // the begin kernel reads source id k H + i of window k: the buffer is addressed from the source position of its first id
        q.src = reinterpret_cast<const int*>(reinterpret_cast<intptr_t>(st.src) - (intptr_t)rd.k_first * H * 4);
        for (int k = rd.k_first; k < rd.k_first + rd.n_win; ++k)
            if (int rc = run_window(k, S, false)) return rc;
        if (rd.final_window)
            if (int rc = run_window(rd.k_first + rd.n_win, rd.final_ids, true)) return rc;
        ran += rd.n_win + (rd.final_window ? 1 : 0);
        if (rd.n_win > 0 && !rd.final_window) {
            hipLaunchKernelGGL(gpt_stream_shift_kernel, dim3(1), dim3(1024), 0, stream, st.src, rd.n_win * H, rd.held + rd.take - rd.n_win * H);
            AT_CHECK_HIP(hipGetLastError());
        }
    }
    // the carry of the next call's first window: the last r (S - H) ids of what has been produced
    if (k1 > k0 && !final && carry > 0)
        AT_CHECK_HIP(hipMemcpyAsync(st.carry, out_abs + (int64_t)r * k1 * H, (size_t)carry * 4, hipMemcpyDeviceToDevice, stream));
    pos[0] += n_new;
    pos[1] = final;
    if (windows_run) *windows_run = ran;
    return 0;
}

}  // extern "C"

// ---- the stream pool: many streams whose ids arrive in pushes share the cache rows and the ticks --------------------------------------
namespace {

// Behind the queue's state (slots cache rows, tick_tokens token rows), per stream: its source ring (2 S ids) and its carry. Nothing else is kept per stream.
struct GptPoolState {
    GptState g;
    int *src, *carry;   // [streams][2 S], [streams][r (S - H) + 1]
    int carry_stride;
    size_t bytes;
};
GptPoolState carve_pool(void* base, const at_gpt* h, int streams, int slots, int max_len, int tick_tokens, int S, int H, int r) {
    GptPoolState st{};
    st.g = carve_state(base, slots, max_len, tick_tokens, h->vocab, h->n_layer);
    StateCarver c(base, st.g.bytes);
    st.carry_stride = r * (S - H) + 1;
    st.src = c.take<int>((size_t)streams * 2 * S);
    st.carry = c.take<int>((size_t)streams * st.carry_stride);
    st.bytes = c.off;
    return st;
}

// Up to GPT_POOL_CHUNK streams' pieces of one launch, by value: no table on the device that could disagree with the host's record
constexpr int GPT_POOL_CHUNK = 128;
struct PoolPieces {
    int n;
    int dst[GPT_POOL_CHUNK], src[GPT_POOL_CHUNK], len[GPT_POOL_CHUNK];   // piece e: len[e] ids from index src[e] of one array to index dst[e] of another (or, the shift, the same)
    void add(int64_t d, int64_t s, int l) { dst[n] = (int)d; src[n] = (int)s; len[n] = l; ++n; }
};
// to[dst[e] + t] = from[src[e] + t]: the copy-in behind each ring's held ids, and the carries into and out of the call's pieces. The two arrays are distinct.
__global__ __launch_bounds__(256) void gpt_pool_copy_kernel(PoolPieces p, int* to, const int* from) {
    const int e = blockIdx.x;
    for (int t = threadIdx.x; t < p.len[e]; t += 256) to[p.dst[e] + t] = from[p.src[e] + t];
}
// ring e: buf[dst[e] + t] = buf[src[e] + t] for t < len[e] <= 2 S <= 1024: one workgroup a ring, every id read before any is written
__global__ __launch_bounds__(1024) void gpt_pool_shift_kernel(PoolPieces p, int* buf) {
    const int e = blockIdx.x, t = threadIdx.x, n = p.len[e];
    const int v = t < n ? buf[p.src[e] + t] : 0;
    __syncthreads();
    if (t < n) buf[p.dst[e] + t] = v;
}
// the pieces gathered for one kernel, launched GPT_POOL_CHUNK at a time
struct PoolLaunch {
    std::vector<PoolPieces> chunks;
    void add(int64_t d, int64_t s, int l) {
        if (l <= 0) return;
        if (chunks.empty() || chunks.back().n == GPT_POOL_CHUNK) chunks.push_back(PoolPieces{});
        chunks.back().add(d, s, l);
    }
    int copy(int* to, const int* from, hipStream_t stream) const {
        for (const PoolPieces& c : chunks) {
            hipLaunchKernelGGL(gpt_pool_copy_kernel, dim3(c.n), dim3(256), 0, stream, c, to, from);
            AT_CHECK_HIP(hipGetLastError());
        }
        return 0;
    }
    int shift(int* buf, hipStream_t stream) const {
        for (const PoolPieces& c : chunks) {
            hipLaunchKernelGGL(gpt_pool_shift_kernel, dim3(c.n), dim3(1024), 0, stream, c, buf);
            AT_CHECK_HIP(hipGetLastError());
        }
        return 0;
    }
};

int check_pool_capacity(const char* who, const at_gpt* h, int streams, int slots, int max_len, int tick_tokens, int S, int H, int r, int max_new) {
    const std::string w(who);
    if (!(h && h->finalized)) { set_error(w + ": the model is not finalized"); return -1; }
    if (!(streams >= 1 && streams <= GPT_MAX_POOL_STREAMS)) { set_error(w + ": streams must be 1 to 1024"); return -1; }
    if (!(slots >= 1 && slots <= GPT_MAX_B)) { set_error(w + ": slots must be 1 to 64"); return -1; }
    if (check_geometry(h, Geometry{S, H, r})) return -1;
    // a non-final window fills S + 1 + r S positions, a final one its prompt and at most max_new more (max_new < 0: the size query, which cannot know it)
    const int final_len = S + 1 + r * (S - H) + (max_new < 0 ? 0 : max_new);
    const int need = std::max(S + 1 + r * S, std::min(h->block, final_len));
    if (!(max_len >= need && max_len <= h->block)) { set_error(w + ": max_len must hold the longest window with its new ids and not exceed the block size"); return -1; }
    if (!(tick_tokens >= slots + max_len && tick_tokens <= GPT_MAX_TICK_TOKENS)) {
        set_error(w + ": tick_tokens must be slots + max_len to " + std::to_string(GPT_MAX_TICK_TOKENS));
        return -1;
    }
    return 0;
}

}  // namespace

extern "C" {

size_t at_gpt_pool_state_bytes(const at_gpt_t* h, int streams, int slots, int max_len, int tick_tokens, int S, int H, int r) {
    if (check_pool_capacity("at_gpt_pool_state_bytes", h, streams, slots, max_len, tick_tokens, S, H, r, -1)) return 0;
    return carve_pool(nullptr, h, streams, slots, max_len, tick_tokens, S, H, r).bytes;
}

int at_gpt_pool_push(at_gpt_t* h, void* state_dev, size_t state_bytes, int streams, int slots, int max_len, int tick_tokens, int64_t* pos, int n,
                     const int32_t* place, const int32_t* ids_dev, const int32_t* n_new, const int32_t* final, int S, int H, int r, int semantic_offset,
                     int semantic_vocab, int infer_token, int acoustic_offset, int codebook_size, int stop_token, int max_new, float temperature, int top_k,
                     const float* uniforms_dev, int u_stride, const int64_t* u_pos0, int32_t* out_ids_dev, int out_stride, int32_t* out_len_dev,
                     int32_t* finish_dev, float* logits_out_dev, int32_t* windows_run, int32_t* trace, int trace_cap, int32_t* n_ticks, int32_t* n_rounds,
                     int32_t* placement, at_stream_t stream_, int32_t* status_dev) {
    const char* who = "at_gpt_pool_push";
    AT_REQUIRE(max_new >= 1 && max_new <= GPT_MAX_BLOCK, "max_new must be 1 to 1024");
    if (int rc = check_pool_capacity(who, h, streams, slots, max_len, tick_tokens, S, H, r, max_new)) return rc;
    AT_REQUIRE(state_dev != nullptr, "null state");
    AT_REQUIRE(n >= 0 && n <= streams, "n (the call's streams) must be 0 to streams");
    AT_REQUIRE(pos != nullptr, "null pointer");
    AT_REQUIRE(n == 0 || (place && n_new && final && u_pos0 && uniforms_dev && out_ids_dev && out_len_dev && finish_dev), "null pointer");
    AT_REQUIRE(trace_cap >= 0 && (trace != nullptr || trace_cap == 0), "trace_cap must be 0 without a trace and never negative");
    AT_REQUIRE(u_stride >= 0 && out_stride >= 0, "u_stride and out_stride must not be negative");
    AT_REQUIRE((int64_t)n * out_stride <= INT32_MAX, "n * out_stride must fit 31 bits: the pieces and the origins are addressed by int");
    Rules q{};
    GenRequest rq{who, h, {ids_dev, 1, nullptr, n}, {S, H, r}, {semantic_offset, semantic_vocab, infer_token, acoustic_offset, codebook_size, stop_token},
                  {max_new, temperature, top_k, uniforms_dev, u_stride}, {out_ids_dev, out_stride, out_len_dev, finish_dev, logits_out_dev}, {state_dev, state_bytes, max_len},
                  stream_, status_dev};
    if (int rc = check_long_rules(rq, &q)) return rc;
    // ---- every stream of the call, checked before any is changed: its place, its record, and what its windows need of the caller's arrays
    const int block = h->block, carry = r * (S - H);
    std::vector<char> named((size_t)streams, 0);
    std::vector<int64_t> n_before((size_t)n), p_base((size_t)n);
    std::vector<int> k0((size_t)n), k1((size_t)n);
    int64_t total_new = 0;
    for (int i = 0; i < n; ++i) {
        const std::string at = std::string(who) + ": stream " + std::to_string(i) + " of the call: ";
        if (place[i] < 0 || place[i] >= streams || named[place[i]]) { set_error(at + "its place must be 0 to streams - 1 and named once"); return -1; }
        named[place[i]] = 1;
        const int64_t* ps = pos + 2 * (size_t)place[i];
        if (final[i] != 0 && final[i] != 1) { set_error(at + "final must be 0 or 1"); return -1; }
        if (n_new[i] < 0) { set_error(at + "n_new must not be negative"); return -1; }
        if (ps[1] != 0) { set_error(at + "the stream is finished: a push after the final call"); return -1; }
        if (ps[0] < 0 || ps[0] + n_new[i] > GPT_MAX_SOURCE) { set_error(at + "a stream takes at most 65536 ids"); return -1; }
        if (final[i] && ps[0] + n_new[i] < 1) { set_error(at + "a final call with nothing pushed"); return -1; }
        if (u_pos0[i] < 0 || u_pos0[i] > INT32_MAX) { set_error(at + "u_pos0 must not be negative and must fit 31 bits"); return -1; }
        n_before[i] = ps[0];
        k0[i] = gpt_stream_windows_run(ps[0], S, H);
        k1[i] = gpt_stream_windows_run(ps[0] + n_new[i], S, H);
        p_base[i] = k0[i] > 0 ? (int64_t)r * k0[i] * H : 0;   // the stream position of out_ids_dev[i][0]
        total_new += n_new[i];
        if (k1[i] > k0[i] || final[i]) {
            const int64_t N = ps[0] + n_new[i];
            const GptWindow first = gpt_window((int)(final[i] && k0[i] == k1[i] ? N : (int64_t)k0[i] * H + S + 1), k0[i], S, H, r, max_new, block);
            const GptWindow last = gpt_window((int)(final[i] ? N : (int64_t)(k1[i] - 1) * H + S + 1), final[i] ? k1[i] : k1[i] - 1, S, H, r, max_new, block);
            const int64_t end = (int64_t)last.stream_base + last.budget;
            if (!(first.stream_base >= u_pos0[i] && end <= u_pos0[i] + u_stride)) { set_error(at + "the uniforms do not cover the stream positions this call draws"); return -1; }
            if (end - p_base[i] > out_stride) { set_error(at + "out_stride must hold the carry and the ids this call can produce"); return -1; }
        }
    }
    AT_REQUIRE(total_new == 0 || ids_dev != nullptr, "ids need a pointer");
    const GptPoolState st = carve_pool(state_dev, h, streams, slots, max_len, tick_tokens, S, H, r);
    AT_REQUIRE(state_bytes >= st.bytes, "state too small: at_gpt_pool_state_bytes(h, streams, slots, max_len, tick_tokens, S, H, r)");
    if (n_ticks) *n_ticks = 0;
    if (n_rounds) *n_rounds = 0;
    if (n == 0) return 0;
    // ---- nothing above touched the device or the host record
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    hipStream_t stream = (hipStream_t)stream_;
    const SampleArgs sa = generation_args(h, st.g, rq.samp, rq.out);
    q.src = st.src;
    q.src_stride = 0;   // a stream's ring is found by its start's origin, not by its row of the call
    // each piece begins with the carry its stream's first window of the call reads
    PoolLaunch carry_in;
    for (int i = 0; i < n; ++i)
        if ((k1[i] > k0[i] || final[i]) && k0[i] > 0) carry_in.add((int64_t)i * out_stride, (int64_t)place[i] * st.carry_stride, carry);
    if (int rc = carry_in.copy(out_ids_dev, st.carry, stream)) return rc;
    GptPoolSchedule schedule(n_before.data(), n_new, final, n, S, H, r, max_new, block, slots, tick_tokens);
    std::vector<int64_t> taken((size_t)n, 0);
    std::vector<int32_t> ran((size_t)n, 0);
    int64_t id_off = 0;
    std::vector<int64_t> id0((size_t)n);
    for (int i = 0; i < n; ++i) { id0[i] = id_off; id_off += n_new[i]; }
    while (schedule.next_round()) {
        PoolLaunch copy_in, shift;
        for (int i = 0; i < n; ++i) {
            const GptStreamRound* rd = schedule.round(i);
            if (!rd) continue;
            const int64_t ring = (int64_t)place[i] * 2 * S;
            copy_in.add(ring + rd->held, id0[i] + taken[i], rd->take);
            taken[i] += rd->take;
            ran[i] += rd->n_win + (rd->final_window ? 1 : 0);
            if (rd->n_win > 0 && !rd->final_window) shift.add(ring, ring + (int64_t)rd->n_win * H, rd->held + rd->take - rd->n_win * H);
        }
        if (int rc = copy_in.copy(st.src, ids_dev, stream)) return rc;
        GptPoolTick t;
        while (schedule.next(&t)) {
            TickPlan p{};
            p.steps.n = p.R = t.n_step;
            for (int j = 0; j < t.n_step; ++j) p.steps.slot[j] = (unsigned char)t.step_slot[j];
            for (int j = 0; j < t.n_start; ++j) {
                const GptQueueStart& s0 = t.start[j];
                p.src_org[j] = (int)((int64_t)place[s0.src] * 2 * S - t.src_pos[j]);
                p.out_org[j] = (int)p_base[s0.src];
                p.u_org[j] = (int)u_pos0[s0.src];
                p.start(s0.slot, s0.src, s0.k, s0.P, s0.final_window != 0);
            }
            if (int rc = run_tick(h, st.g, p, q, sa, stream)) return rc;
            const int at = schedule.ticks() - 1;
            if (at < trace_cap) {   // a trace too small loses its tail, the run goes on
                int32_t* row = trace + 5 * (size_t)at;
                row[0] = t.n_step; row[1] = t.n_start; row[2] = t.prefill_tokens; row[3] = t.route(); row[4] = schedule.rounds() - 1;
            }
            if (t.poll) {   // the host's only look at the device: some row is in a final window, and when that ends only the device knows
                AT_CHECK_HIP(hipMemcpyAsync(h->flags_host, st.g.done, slots * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
                AT_CHECK_HIP(hipStreamSynchronize(stream));
                schedule.seen(h->flags_host);
            }
        }
        if (int rc = shift.shift(st.src, stream)) return rc;
    }
    // the carry of each stream's next call: the last r (S - H) ids of what it has produced
    PoolLaunch carry_out;
    for (int i = 0; i < n; ++i)
        if (k1[i] > k0[i] && !final[i]) carry_out.add((int64_t)place[i] * st.carry_stride, (int64_t)i * out_stride + (int64_t)r * k1[i] * H - p_base[i], carry);
    if (int rc = carry_out.copy(st.carry, out_ids_dev, stream)) return rc;
    for (int i = 0; i < n; ++i) {
        pos[2 * (size_t)place[i]] += n_new[i];
        pos[2 * (size_t)place[i] + 1] = final[i];
        if (windows_run) windows_run[i] = ran[i];
    }
    if (n_ticks) *n_ticks = schedule.ticks();
    if (n_rounds) *n_rounds = schedule.rounds();
    if (placement) std::memcpy(placement, schedule.placement().data(), (size_t)n * 3 * sizeof(int32_t));
    return 0;
}

}  // extern "C"
