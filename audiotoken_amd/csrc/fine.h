// The handle of the fine stage (fine.hip), declared apart from its code so that the stand-alone argument check (tools/fine_args.hip) can
// build a finalized handle with no device behind it: every entry point validates against the handle's dimensions alone before it touches one.
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "at_common.h"

namespace at {

constexpr int FINE_CODES = 8;          // code books of a frame; the first FINE_COARSE are given
constexpr int FINE_COARSE = 2;
constexpr int FINE_PASSES = FINE_CODES - FINE_COARSE;   // forwards of one window: code books 2 to 7
constexpr int FINE_HEADS = 7;          // lm_heads[j] predicts code book j + 1
constexpr int FINE_TABLE = 1056;       // rows of an embedding table and of a head
constexpr int FINE_VOCAB = 1024;       // the ids a head may produce; 1024 itself is the "nothing yet" id of a cell
constexpr int FINE_MAX_B = 64, FINE_MAX_BLOCK = 1024, FINE_MAX_LAYERS = 48;
constexpr int FINE_MAX_T = 1 << 18;    // frames of one row (58 minutes at 75 frames a second)

struct FineHostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
};

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

}  // namespace at

struct at_fine {
    int device = 0;
    bool finalized = false;
    std::map<std::string, at::FineHostTensor> staged;
    int n_layer = 0, embd = 0, block = 0;
    bool bias = false;                // the four linears of every block carry a bias
    std::vector<void*> allocs;        // every device allocation of finalize()
    const float* wtes[at::FINE_CODES] = {};
    const float* heads[at::FINE_HEADS] = {};
    const float *wpe = nullptr, *lnf_g = nullptr, *lnf_b = nullptr;
    std::vector<at::FineLayer> layers;
};
