// The handle of the semantic-to-acoustic GPT (gpt.hip, gpt_model.hip) and the pure host arithmetic of its schedules, declared apart from
// the code so that the stand-alone argument checks (tools/gpt_*args.hip) can build a finalized handle with no device behind it: every entry point
// validates against the handle's dimensions alone before it touches one. The handle's plumbing (staging, upload, allocations) and the state carver are
// model_handle.h's, shared with the fine stage.
#pragma once
#include "model_handle.h"

namespace at {

constexpr int GPT_EMBD = 768, GPT_HEADS = 12, GPT_HEAD_DIM = 64, GPT_FF = 3072;
constexpr int GPT_MAX_B = 64, GPT_MAX_VOCAB = 65536, GPT_MAX_BLOCK = 1024, GPT_MAX_LAYERS = 48;
constexpr int GPT_ROW_TILE = 16;       // activation rows one pass of a linear kernel holds
constexpr int GPT_CHECK_EVERY = 16;    // steps between two looks of the host at the rows' finish flags
// finish[] of at_gpt_generate
enum { GPT_RUNNING = 0, GPT_FINISH_STOP = 1, GPT_FINISH_MAX_NEW = 2, GPT_FINISH_BLOCK = 3 };
constexpr int GPT_PASS_DONE = 4;       // done[] of a row whose non-final window is complete (at_gpt_generate_long): never written to finish[]
constexpr int GPT_MAX_SOURCE = 65536;  // source ids of one row of at_gpt_generate_long

// The long form's schedule: windows of a source of N ids at window S and hop H; window k reads source ids [k H, k H + min(S, N - k H)).
// A row with a voice prompt of pv ids (0: none) follows the same schedule on the concatenated source, prompt ids then source ids.
inline int gpt_long_windows(int N, int S, int H, int pv = 0) { return pv + N <= S ? 1 : (pv + N - S + H - 1) / H + 1; }
// what a voice prompt must satisfy: even, 2 <= pv <= S - H, so that no window's prompt exceeds S + 1 + r (S - H) tokens
inline bool gpt_voice_prompt_ok(int pv, int N, int S, int H) { return pv >= 2 && pv % 2 == 0 && pv <= S - H && N >= 1 && (int64_t)pv + N <= GPT_MAX_SOURCE; }

// Window k of a source of N ids: n_ids source ids, `carry` ids of the source's own stream behind them and INFER between make the P prompt tokens; the
// window's step 0 lies at stream_base; it runs `budget` steps (a final window: at most). The one statement of this arithmetic for the three entry points,
// the scheduler below and tools/gpt_queue_args.hip; acoustic_windows / window_steps in semantic_decoder.py are its Python twins.
// With a voice prompt of pv ids, N stays the source's own count: window k reads ids [k H, ..) of the concatenated source, window 0 carries the prompt's
// r pv coarse ids, which are given and not generated, and stream_base is the RESULT position: the stream position minus r pv.
struct GptWindow {
    int n_ids, P, budget, carry, stream_base;
    bool final_window;
};
inline GptWindow gpt_window(int N, int k, int S, int H, int r, int max_new, int block, int pv = 0) {
    GptWindow w;
    w.carry = k > 0 ? r * (S - H) : r * pv;
    w.final_window = k == gpt_long_windows(N, S, H, pv) - 1;
    w.n_ids = w.final_window ? pv + N - k * H : S;
    w.P = w.n_ids + 1 + w.carry;
    w.budget = w.final_window ? (max_new < block - w.P ? max_new : block - w.P) : r * S - w.carry;
    w.stream_base = r * k * H + w.carry - r * pv;
    return w;
}
// What a set of sources needs: positions of a cache row (the longest window with its new ids) and ids of a row of the caller's stream arrays
struct GptExtent {
    int need_len = 0;
    int64_t need_stride = 0;
};
// (need_stride counts result ids; pv NULL or the voice prompt length of each source)
inline GptExtent gpt_extent(const int32_t* src_len, int n_src, int S, int H, int r, int max_new, int block, const int32_t* pv = nullptr) {
    GptExtent e;
    for (int i = 0; i < n_src; ++i) {
        const int v = pv ? pv[i] : 0;
        const int n = gpt_long_windows(src_len[i], S, H, v);
        const GptWindow w = gpt_window(src_len[i], n - 1, S, H, r, max_new, block, v);
        const int64_t end = (int64_t)w.stream_base + w.budget;
        e.need_stride = end > e.need_stride ? end : e.need_stride;
        e.need_len = w.P + w.budget > e.need_len ? w.P + w.budget : e.need_len;
        if (n > 1 && S + 1 + r * S > e.need_len) e.need_len = S + 1 + r * S;   // a non-final window fills up to here
    }
    return e;
}

// ---- the generation queue's scheduler: pure host code, shared by at_gpt_generate_queue and tools/gpt_queue_args.hip ------------------------
// Sources run 19's windows through `slots` cache rows. A tick is one model pass over one token list: one step token of every slot that is mid-window, then
// the whole prompt of every window admitted this tick. Everything about the schedule is known from the lengths except when a final window ends; that
// comes from the rows' flags, looked at every GPT_CHECK_EVERY ticks while some slot is in a final window.
constexpr int GPT_MAX_QUEUE = 4096;                                   // sources of one at_gpt_generate_queue call
constexpr int GPT_MAX_TICK_TOKENS = GPT_MAX_B * (GPT_MAX_BLOCK + 1);  // more than every slot prefilling at once cannot be used
constexpr int GPT_GEMM_ABOVE = GPT_MAX_B;                             // a pass of more tokens takes the fp32 GEMM route (run_layers)

struct GptQueueStart {
    int slot, src, k, final_window, n_ids, P;   // window k of source src begins in slot: n_ids source ids, P prompt tokens
};
struct GptQueueTick {
    int n_step = 0, n_start = 0, prefill_tokens = 0;
    int step_slot[GPT_MAX_B];
    GptQueueStart start[GPT_MAX_B];
    bool poll = false;   // the caller must hand the rows' flags to seen() before the next tick
    int tokens() const { return n_step + prefill_tokens; }
    int route() const { return tokens() > GPT_GEMM_ABOVE ? 1 : 0; }
};

class GptQueueSchedule {
  public:
    // src_len (and pv: NULL or each source's voice prompt length) must outlive the schedule; every argument has been validated by the caller
    // (tick_tokens >= slots + the longest prompt)
    GptQueueSchedule(const int32_t* src_len, int n_src, int S, int H, int r, int max_new, int block, int slots, int tick_tokens, const int32_t* pv = nullptr)
        : len_(src_len), pv_(pv), n_src_(n_src), S_(S), H_(H), r_(r), max_new_(max_new), block_(block), slots_(slots), tick_tokens_(tick_tokens),
          placement_((size_t)n_src * 3, -1) {
        for (int j = 0; j < GPT_MAX_B; ++j) slot_[j] = Slot{};
    }
    // The next tick, or false when every source has been retired. Waiting sources take empty slots in source order; every running slot steps; windows are
    // admitted in slot order while the list stays within tick_tokens (the first always fits, so no tick is empty and no slot starves).
    bool next(GptQueueTick* t) {
        *t = GptQueueTick{};
        tick_ = n_ticks_;
        bool any = false;
        for (int j = 0; j < slots_; ++j) {
            Slot& s = slot_[j];
            if (s.src < 0 && next_src_ < n_src_) {
                s = Slot{};
                s.src = next_src_++;
                placement_[3 * (size_t)s.src] = j;
            }
            any = any || s.src >= 0;
        }
        if (!any) return false;
        for (int j = 0; j < slots_; ++j)
            if (slot_[j].src >= 0 && slot_[j].running) t->step_slot[t->n_step++] = j;
        for (int j = 0; j < slots_; ++j) {
            Slot& s = slot_[j];
            if (s.src < 0 || s.running) continue;
            const GptWindow w = gpt_window(len_[s.src], s.k, S_, H_, r_, max_new_, block_, pv_ ? pv_[s.src] : 0);
            if (t->tokens() + w.P > tick_tokens_) break;   // it waits, and so does every slot after it
            t->start[t->n_start++] = GptQueueStart{j, s.src, s.k, w.final_window ? 1 : 0, w.n_ids, w.P};
            t->prefill_tokens += w.P;
            s.running = true;
            s.final_window = w.final_window;
            s.budget = w.budget;
            s.t = 0;
            if (s.k == 0) placement_[3 * (size_t)s.src + 1] = tick_;
        }
        // the state after this tick's sampler launch, as far as the host knows it
        bool in_final = false;
        auto sampled = [&](int j) {
            Slot& s = slot_[j];
            if (++s.t < s.budget) { in_final = in_final || s.final_window; return; }
            if (s.final_window) { retire(j); return; }   // out of budget: finished whatever it drew
            ++s.k;
            s.running = false;
        };
        for (int i = 0; i < t->n_step; ++i) sampled(t->step_slot[i]);
        for (int i = 0; i < t->n_start; ++i) sampled(t->start[i].slot);
        ++n_ticks_;
        t->poll = in_final && n_ticks_ % GPT_CHECK_EVERY == 0;
        return true;
    }
    // after a tick with poll set: done[j] of every slot as the device has it now
    void seen(const int32_t* done) {
        for (int j = 0; j < slots_; ++j)
            if (slot_[j].src >= 0 && slot_[j].running && slot_[j].final_window && done[j] != GPT_RUNNING) retire(j);
    }
    // the dry run's stand-in for the device: the flag of a slot whose final window ends after final_steps[src] sampler launches
    void seen_by_steps(const int32_t* final_steps) {
        int32_t done[GPT_MAX_B];
        for (int j = 0; j < slots_; ++j) {
            const Slot& s = slot_[j];
            done[j] = s.src >= 0 && s.running && s.final_window && s.t >= final_steps[s.src] ? GPT_FINISH_STOP : GPT_RUNNING;
        }
        seen(done);
    }
    int ticks() const { return n_ticks_; }
    const std::vector<int32_t>& placement() const { return placement_; }   // [n_src][3]: slot, first tick, last tick seen

  private:
    struct Slot {
        int src = -1, k = 0, t = 0, budget = 0;
        bool running = false, final_window = false;
    };
    void retire(int j) {
        placement_[3 * (size_t)slot_[j].src + 2] = tick_;
        slot_[j] = Slot{};
    }
    const int32_t *len_, *pv_;
    int n_src_, S_, H_, r_, max_new_, block_, slots_, tick_tokens_;
    int next_src_ = 0, n_ticks_ = 0, tick_ = 0;   // tick_: the index of the tick next() made last
    Slot slot_[GPT_MAX_B];
    std::vector<int32_t> placement_;
};

// ---- the stream's scheduler: pure host code, shared by at_gpt_stream_push and tools/semantic_stream_args.hip ------------------------------
// One source whose ids arrive in pushes. With n ids there, window k has run (as a non-final window) for every k with n > k H + S: one id past the window
// must exist, since with exactly k H + S ids the window may still be the final one. The state's source buffer holds 2 S ids, from id `k H` of the next
// window to run on, so a push is absorbed in rounds: take what fits, run what became runnable, drop the (windows run) * H ids no window reads again.
inline int gpt_stream_windows_run(int64_t n, int S, int H) { return n > S ? (int)((n - S - 1) / H) + 1 : 0; }
struct GptStreamRound {
    int take;            // new ids copied behind the held ones
    int held;            // ids in the buffer before the copy; the buffer's first id is id k_first * H of the source
    int k_first, n_win;  // non-final windows k_first .. k_first + n_win - 1 run in this round
    bool final_window;   // then window k_first + n_win runs as the final one, on the ids that are left
    int final_ids;       // its source ids
};
class GptStreamSchedule {
  public:
    GptStreamSchedule(int64_t n_before, int n_new, bool final, int S, int H) : n_(n_before), left_(n_new), final_(final), S_(S), H_(H) {
        k_ = gpt_stream_windows_run(n_before, S, H);
    }
    bool next(GptStreamRound* r) {
        if (done_) return false;
        *r = GptStreamRound{};
        r->held = (int)(n_ - (int64_t)k_ * H_);
        r->take = left_ < 2 * S_ - r->held ? left_ : 2 * S_ - r->held;
        n_ += r->take;
        left_ -= r->take;
        r->k_first = k_;
        k_ = gpt_stream_windows_run(n_, S_, H_);
        r->n_win = k_ - r->k_first;
        if (left_ == 0) {
            done_ = true;
            if (final_) { r->final_window = true; r->final_ids = (int)(n_ - (int64_t)k_ * H_); }
        }
        return r->take > 0 || r->n_win > 0 || r->final_window;
    }
  private:
    int64_t n_;
    int left_, k_ = 0;
    bool final_, done_ = false;
    int S_, H_;
};

// ---- the stream pool's scheduler: pure host code, shared by at_gpt_pool_push and tools/audio_stream_pool_args.hip ---------------------------
// One call serves n streams, in ascending stream id; each has its own GptStreamSchedule. A round is global: round g of the call is round g of every stream
// that still has one (copy-in, then the round's ticks, then the shift). In a round a stream's windows form a chain (its non-final windows in order, then the
// final one when the stream is flushed and this is its last round), and the chains are 20's sources: waiting streams take free cache rows in ascending
// stream id, every running row steps, windows are admitted in slot order while the tick's list stays within tick_tokens, and a row whose stream's chain is
// complete is handed on. A round ends when every chain of it is complete: the shift must not overtake a window that still reads the ring, so no row is
// held across a round's end. The flags are polled every GPT_CHECK_EVERY ticks of the call while some row is in a final window, and never otherwise.
constexpr int GPT_MAX_POOL_STREAMS = 1024;
struct GptPoolTick : GptQueueTick {
    int src_pos[GPT_MAX_B];   // start j: the source position of its stream's ring's first id in this round (k_first * H)
};
class GptPoolSchedule {
  public:
    // the arrays must outlive the schedule; every argument has been validated by the caller (tick_tokens >= slots + the longest prompt)
    GptPoolSchedule(const int64_t* n_before, const int32_t* n_new, const int32_t* final, int n, int S, int H, int r, int max_new, int block, int slots, int tick_tokens)
        : n_(n), S_(S), H_(H), r_(r), max_new_(max_new), block_(block), slots_(slots), tick_tokens_(tick_tokens), rd_(n), live_(n, 0), placement_((size_t)n * 3, -1) {
        sched_.reserve(n);
        for (int i = 0; i < n; ++i) sched_.emplace_back(n_before[i], n_new[i], final[i] != 0, S, H);
        for (int j = 0; j < GPT_MAX_B; ++j) slot_[j] = Slot{};
    }
    // The next round, or false when no stream has one left. round(i) is stream i's part of it, NULL when it has none.
    bool next_round() {
        bool any = false;
        for (int i = 0; i < n_; ++i) {
            live_[i] = sched_[i].next(&rd_[i]) ? 1 : 0;
            any = any || live_[i];
        }
        next_src_ = 0;
        if (any) ++n_rounds_;
        return any;
    }
    const GptStreamRound* round(int i) const { return live_[i] ? &rd_[i] : nullptr; }
    // The next tick of the round, or false when every chain of the round is complete
    bool next(GptPoolTick* t) {
        *t = GptPoolTick{};
        tick_ = n_ticks_;
        bool any = false;
        for (int j = 0; j < slots_; ++j) {
            Slot& s = slot_[j];
            if (s.src < 0) {
                while (next_src_ < n_ && chain(next_src_) == 0) ++next_src_;
                if (next_src_ < n_) {
                    s = Slot{};
                    s.src = next_src_++;
                    placement_[3 * (size_t)s.src] = j;
                }
            }
            any = any || s.src >= 0;
        }
        if (!any) return false;
        for (int j = 0; j < slots_; ++j)
            if (slot_[j].src >= 0 && slot_[j].running) t->step_slot[t->n_step++] = j;
        for (int j = 0; j < slots_; ++j) {
            Slot& s = slot_[j];
            if (s.src < 0 || s.running) continue;
            const GptStreamRound& rd = rd_[s.src];
            const bool last = s.w == rd.n_win;   // past the non-final windows: the final one
            const int k = rd.k_first + s.w;
            const GptWindow w = gpt_window(last ? k * H_ + rd.final_ids : k * H_ + S_ + 1, k, S_, H_, r_, max_new_, block_);
            if (t->tokens() + w.P > tick_tokens_) break;   // it waits, and so does every slot after it
            t->src_pos[t->n_start] = rd.k_first * H_;
            t->start[t->n_start++] = GptQueueStart{j, s.src, k, last ? 1 : 0, w.n_ids, w.P};
            t->prefill_tokens += w.P;
            s.running = true;
            s.final_window = last;
            s.budget = w.budget;
            s.t = 0;
            if (placement_[3 * (size_t)s.src + 1] < 0) placement_[3 * (size_t)s.src + 1] = tick_;
        }
        bool in_final = false;
        auto sampled = [&](int j) {
            Slot& s = slot_[j];
            if (++s.t < s.budget) { in_final = in_final || s.final_window; return; }
            s.running = false;
            if (++s.w >= chain(s.src)) retire(j);   // the chain is complete: the row is handed on
        };
        for (int i = 0; i < t->n_step; ++i) sampled(t->step_slot[i]);
        for (int i = 0; i < t->n_start; ++i) sampled(t->start[i].slot);
        ++n_ticks_;
        t->poll = in_final && n_ticks_ % GPT_CHECK_EVERY == 0;
        return true;
    }
    // after a tick with poll set: done[j] of every slot as the device has it now
    void seen(const int32_t* done) {
        for (int j = 0; j < slots_; ++j)
            if (slot_[j].src >= 0 && slot_[j].running && slot_[j].final_window && done[j] != GPT_RUNNING) retire(j);
    }
    // the dry run's stand-in for the device: the flag of a slot whose final window ends after final_steps[stream] sampler launches
    void seen_by_steps(const int32_t* final_steps) {
        int32_t done[GPT_MAX_B];
        for (int j = 0; j < slots_; ++j) {
            const Slot& s = slot_[j];
            done[j] = s.src >= 0 && s.running && s.final_window && s.t >= final_steps[s.src] ? GPT_FINISH_STOP : GPT_RUNNING;
        }
        seen(done);
    }
    int ticks() const { return n_ticks_; }
    int rounds() const { return n_rounds_; }
    const std::vector<int32_t>& placement() const { return placement_; }   // [n][3]: the slot of its last chain, its first tick, its last tick seen (-1: no window)

  private:
    struct Slot {
        int src = -1, w = 0, t = 0, budget = 0;   // w: the window's index in the stream's chain of this round
        bool running = false, final_window = false;
    };
    int chain(int i) const { return live_[i] ? rd_[i].n_win + (rd_[i].final_window ? 1 : 0) : 0; }
    void retire(int j) {
        placement_[3 * (size_t)slot_[j].src + 2] = tick_;
        slot_[j] = Slot{};
    }
    int n_, S_, H_, r_, max_new_, block_, slots_, tick_tokens_;
    int next_src_ = 0, n_ticks_ = 0, n_rounds_ = 0, tick_ = 0;
    std::vector<GptStreamSchedule> sched_;
    std::vector<GptStreamRound> rd_;
    std::vector<char> live_;
    Slot slot_[GPT_MAX_B];
    std::vector<int32_t> placement_;
};

struct GptLayer {
    const float *ln1 = nullptr, *qkv = nullptr, *proj = nullptr, *ln2 = nullptr, *fc = nullptr, *fc_proj = nullptr;
};

}  // namespace at

struct at_gpt : at::ModelHandle {   // device, finalized, staged, allocs
    int n_layer = 0, vocab = 0, block = 0;
    const float *wte = nullptr, *wpe = nullptr, *ln_f = nullptr;
    std::vector<at::GptLayer> layers;
    int32_t* flags_host = nullptr;    // pinned: the rows' finish flags as the host last saw them (GPT_MAX_B words)
    // truncation of the generators' sampler (at_gpt_set_truncation): the nucleus' mass (1: off) and float32(log(min_p)) (-inf: off)
    float top_p = 1.0f, lmin = -__builtin_huge_valf();
};
