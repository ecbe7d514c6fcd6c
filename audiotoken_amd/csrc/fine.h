// The handle of the fine stage (fine.hip) and the pure host arithmetic of its schedules, declared apart from the code so that the stand-alone
// argument checks (tools/fine_*args.hip) can build a finalized handle with no device behind it: every entry point validates against the handle's dimensions
// alone before it touches one. The handle's plumbing (staging, upload, allocations) and the state carver are model_handle.h's, shared with the GPT.
#pragma once
#include "model_handle.h"

namespace at {

constexpr int FINE_CODES = 8;          // code books of a frame; the first FINE_COARSE are given
constexpr int FINE_COARSE = 2;
constexpr int FINE_PASSES = FINE_CODES - FINE_COARSE;   // forwards of one window: code books 2 to 7
constexpr int FINE_HEADS = 7;          // lm_heads[j] predicts code book j + 1
constexpr int FINE_TABLE = 1056;       // rows of an embedding table and of a head
constexpr int FINE_VOCAB = 1024;       // the ids a head may produce; 1024 itself is the "nothing yet" id of a cell
constexpr int FINE_MAX_B = 64, FINE_MAX_BLOCK = 1024, FINE_MAX_LAYERS = 48;
constexpr int FINE_MAX_T = 1 << 18;    // frames of one row (58 minutes at 75 frames a second)

struct FineLayer {
    const float *ln1_g = nullptr, *ln1_b = nullptr, *qkv = nullptr, *proj = nullptr, *ln2_g = nullptr, *ln2_b = nullptr, *fc = nullptr, *fc_proj = nullptr;
    const float *qkv_b = nullptr, *proj_b = nullptr, *fc_b = nullptr, *fc_proj_b = nullptr;   // all four or none
};

// The history rule, stated once: a row of T frames that continues a history of Th frames keeps the last h = min(H, Th) of them, H = W / 2,
// in cells [0, h) of its work array of L = max(h + T, W) cells; its own frames are cells [h, h + T). h = 0 is the rule without a history.
inline int fine_history(int Th, int W) { return Th < W / 2 ? Th : W / 2; }
inline int fine_cells(int T, int W, int h = 0) { return h + T > W ? h + T : W; }
// the windows of a row of T frames after h history cells: n = max(0, ceil((T - (W - h)) / H)) + 1
inline int fine_windows(int T, int W, int h = 0) {
    const int H = W / 2;
    return (h + T > W ? (h + T - W + H - 1) / H : 0) + 1;
}
// window k of that row reads cells [start, start + W) and predicts from cell fill on: buffer positions >= rel = fill - start, 0 <= rel <= H.
// With h > 0 every window has rel > 0, and no window writes below cell h.
inline void fine_window(int k, int T, int W, int h, int* start, int* fill) {
    const int H = W / 2, L = fine_cells(T, W, h);
    *start = k * H < L - W ? k * H : L - W;
    *fill = h + k * H < L - H ? h + k * H : L - H;
}

constexpr int FINE_MAX_QUEUE = 4096;   // rows of one at_fine_generate_queue call

// ---- the window queue's schedule: pure host code, known from the lengths alone ------------------------------------------------
// Rows take empty slots in the caller's order; a slot runs its row's windows 0 .. n - 1 in consecutive passes; a slot whose row ran its last window takes
// the next waiting row in the next pass. Pass p is the current window of every occupied slot, in slot order.
struct FineQueuePass {
    int n = 0;                                                 // windows of the pass
    int slot[FINE_MAX_B], row[FINE_MAX_B], k[FINE_MAX_B];      // of each window
    int n_admit = 0, admit[FINE_MAX_B];                        // indices into the window list: windows whose row enters its slot in this pass (k = 0)
    int n_retire = 0, retire[FINE_MAX_B];                      // indices into the window list: windows that are their row's last
};

class FineQueueSchedule {
public:
    // lens: n_rows lengths, each 1 to FINE_MAX_T; 1 <= slots <= FINE_MAX_B; the caller has checked both. hist: null, or the rows' history cells h
    FineQueueSchedule(const int32_t* lens, int n_rows, int W, int slots, const int32_t* hist = nullptr)
        : n_rows_(n_rows), slots_(slots), windows_(n_rows), placement_(3 * (size_t)n_rows, -1) {
        for (int b = 0; b < n_rows; ++b) windows_[b] = fine_windows(lens[b], W, hist ? hist[b] : 0);
        for (int j = 0; j < FINE_MAX_B; ++j) holds_[j] = -1;
    }
    // the next pass; false once every row has retired
    bool next(FineQueuePass* p) {
        *p = FineQueuePass();
        for (int j = 0; j < slots_; ++j) {
            if (holds_[j] < 0 && waiting_ < n_rows_) {
                holds_[j] = waiting_++;
                at_[j] = 0;
                placement_[3 * (size_t)holds_[j]] = j;
                placement_[3 * (size_t)holds_[j] + 1] = passes_;
                p->admit[p->n_admit++] = p->n;
            }
            if (holds_[j] < 0) continue;
            const int i = p->n++, b = holds_[j];
            p->slot[i] = j;
            p->row[i] = b;
            p->k[i] = at_[j]++;
            if (at_[j] == windows_[b]) {
                p->retire[p->n_retire++] = i;
                placement_[3 * (size_t)b + 2] = passes_;
                holds_[j] = -1;
            }
        }
        if (p->n == 0) return false;
        ++passes_;
        return true;
    }
    int passes() const { return passes_; }
    const std::vector<int32_t>& placement() const { return placement_; }   // [n_rows][3]: slot, first pass, last pass
    const std::vector<int>& windows() const { return windows_; }

private:
    int n_rows_, slots_, waiting_ = 0, passes_ = 0;
    int holds_[FINE_MAX_B], at_[FINE_MAX_B] = {};
    std::vector<int> windows_;
    std::vector<int32_t> placement_;
};

// ---- the stream's scheduler: pure host code, shared by at_fine_stream_push and tools/semantic_stream_args.hip ---------------------------
// One row whose coarse frames arrive in pushes, no history. With T frames there, window j has run at start = j H for every j with j H + W <= T; such a
// window is the same whether or not it turns out to be the row's last. The state's work array holds FINE_STREAM_CELLS(W) = 2 W cells, from the start of
// the last window run on (the row's last window, at start = T - W, reads down to there), so a push is absorbed in rounds: take what fits, run what became
// runnable, emit what turned final, shift. After non-last window j frames [j H, (j + 1) H) are final; after the last everything up to T.
inline int fine_stream_windows_run(int64_t T, int W) { return T >= W ? (int)((T - W) / (W / 2)) + 1 : 0; }
inline int fine_stream_cells(int W) { return 2 * W; }
struct FineStreamRound {
    int take;                 // new frames handed over behind the held ones
    long long first;          // the row's frame in cell 0 during this round
    int held;                 // frames in the array before the hand-over
    int j_first, n_win;       // windows j_first .. j_first + n_win - 1 run at start = j H, rel = 0
    int pad;                  // final, T < W: cells [T, W) are filled with 1024 and the single window runs (counted in n_win)
    bool last_window;         // final: one more window at start = T - W ...
    int last_rel;             // ... predicting buffer positions >= last_rel > 0
    long long emit_from, emit_to;   // the row's frames that turn final in this round
    int shift;                // cells dropped from the front after the round
};
class FineStreamSchedule {
  public:
    FineStreamSchedule(long long T_before, int n_new, bool final, int W) : T_(T_before), left_(n_new), final_(final), W_(W), H_(W / 2) {
        j_ = fine_stream_windows_run(T_before, W);
    }
    bool next(FineStreamRound* r) {
        if (done_) return false;
        *r = FineStreamRound{};
        r->first = first_of(j_);
        r->held = (int)(T_ - r->first);
        const int room = fine_stream_cells(W_) - r->held;
        r->take = left_ < room ? left_ : room;
        T_ += r->take;
        left_ -= r->take;
        r->j_first = j_;
        r->emit_from = r->emit_to = (long long)j_ * H_;
        j_ = fine_stream_windows_run(T_, W_);
        r->n_win = j_ - r->j_first;
        r->emit_to = (long long)j_ * H_;
        if (left_ == 0) {
            done_ = true;
            if (final_) {
                if (T_ < W_) { r->pad = (int)(W_ - T_); r->n_win = 1; }
                else if ((T_ - W_) % H_ != 0) { r->last_window = true; r->last_rel = (int)((long long)j_ * H_ - (T_ - W_)); }
                r->emit_to = T_;
            }
        }
        r->shift = done_ && final_ ? 0 : (int)(first_of(j_) - r->first);
        return r->take > 0 || r->n_win > 0 || r->last_window || r->emit_to > r->emit_from;
    }
  private:
    long long first_of(int j) const { return j > 0 ? (long long)(j - 1) * H_ : 0; }
    long long T_;
    int left_, j_ = 0;
    bool final_, done_ = false;
    int W_, H_;
};

// ---- the stream pool's scheduler: pure host code, shared by at_fine_pool_push and tools/audio_stream_pool_args.hip ---------------------------
// One call serves n streams, each with its own FineStreamSchedule. A round is global: round g of the call is round g of every stream that still has one
// (hand-over, the runnable windows, emit, shift). A stream's runnable windows of a round form a chain (window j + 1 reads what window j wrote), so they run
// in waves: wave i holds the i-th runnable window of every stream that has one, in the call's order, in passes of up to fine_slots windows. Two windows of
// one stream never share a pass. Everything is known from the counts: nothing is polled.
constexpr int FINE_MAX_POOL_STREAMS = 1024;
struct FinePoolPass {
    int n = 0, wave = 0;
    int stream[FINE_MAX_B], j[FINE_MAX_B], cell[FINE_MAX_B], rel[FINE_MAX_B];   // per window: its stream of the call, its index, its first cell in the stream's array, rel
};
class FinePoolSchedule {
  public:
    // the arrays must outlive the schedule; the caller has checked every argument
    FinePoolSchedule(const int64_t* T_before, const int32_t* n_new, const int32_t* final, int n, int W, int fine_slots)
        : n_(n), W_(W), slots_(fine_slots), rd_(n), live_(n, 0), T_(n) {
        sched_.reserve(n);
        for (int i = 0; i < n; ++i) {
            sched_.emplace_back(T_before[i], n_new[i], final[i] != 0, W);
            T_[i] = T_before[i] + n_new[i];
        }
    }
    bool next_round() {
        bool any = false;
        for (int i = 0; i < n_; ++i) {
            live_[i] = sched_[i].next(&rd_[i]) ? 1 : 0;
            any = any || live_[i];
        }
        wave_ = 0;
        at_ = 0;
        if (any) ++n_rounds_;
        return any;
    }
    const FineStreamRound* round(int i) const { return live_[i] ? &rd_[i] : nullptr; }
    // the next pass of the round, or false when every window of it has run
    bool next(FinePoolPass* p) {
        *p = FinePoolPass();
        for (;;) {
            for (; at_ < n_ && p->n < slots_; ++at_) {
                if (chain(at_) <= wave_) continue;
                const FineStreamRound& rd = rd_[at_];
                const int plain = rd.pad ? 1 : rd.n_win, H = W_ / 2, i = p->n++;
                const bool last = wave_ >= plain;
                p->stream[i] = at_;
                p->j[i] = rd.j_first + wave_;
                p->cell[i] = last ? (int)(T_[at_] - W_ - rd.first) : (int)((long long)(rd.j_first + wave_) * H - rd.first);
                p->rel[i] = last ? rd.last_rel : 0;
            }
            if (p->n > 0) { p->wave = wave_; ++n_passes_; return true; }
            bool more = false;
            for (int i = 0; i < n_; ++i) more = more || chain(i) > wave_ + 1;
            if (!more) return false;
            ++wave_;
            at_ = 0;
        }
    }
    int rounds() const { return n_rounds_; }
    int passes() const { return n_passes_; }

  private:
    int chain(int i) const { return live_[i] ? (rd_[i].pad ? 1 : rd_[i].n_win) + (rd_[i].last_window ? 1 : 0) : 0; }
    int n_, W_, slots_, wave_ = 0, at_ = 0, n_rounds_ = 0, n_passes_ = 0;
    std::vector<FineStreamSchedule> sched_;
    std::vector<FineStreamRound> rd_;
    std::vector<char> live_;
    std::vector<long long> T_;
};

}  // namespace at

struct at_fine : at::ModelHandle {  // device, finalized, staged, allocs
    int n_layer = 0, embd = 0, block = 0;
    bool bias = false;                // the four linears of every block carry a bias
    const float* wtes[at::FINE_CODES] = {};
    const float* heads[at::FINE_HEADS] = {};
    const float *wpe = nullptr, *lnf_g = nullptr, *lnf_b = nullptr;
    std::vector<at::FineLayer> layers;
};
