// The handle of the fine stage (fine.hip), declared apart from its code so that the stand-alone argument check (tools/fine_args.hip) can
// build a finalized handle with no device behind it: every entry point validates against the handle's dimensions alone before it touches one.
#pragma once
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

// the windows of a row of T frames: n = max(0, ceil((T - W) / H)) + 1 with H = W / 2
inline int fine_windows(int T, int W) {
    const int H = W / 2;
    return (T > W ? (T - W + H - 1) / H : 0) + 1;
}

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
