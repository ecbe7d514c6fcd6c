// The handle of the semantic-to-acoustic GPT (gpt.hip), declared apart from its code so that the stand-alone argument check
// (tools/gpt_args.hip) can build a finalized handle with no device behind it: every entry point validates against `dims` alone before it touches one.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "at_common.h"

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
inline int gpt_long_windows(int N, int S, int H) { return N <= S ? 1 : (N - S + H - 1) / H + 1; }

struct GptHostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
};

struct GptLayer {
    const float *ln1 = nullptr, *qkv = nullptr, *proj = nullptr, *ln2 = nullptr, *fc = nullptr, *fc_proj = nullptr;
};

}  // namespace at

struct at_gpt {
    int device = 0;
    bool finalized = false;
    std::map<std::string, at::GptHostTensor> staged;
    int n_layer = 0, vocab = 0, block = 0;
    std::vector<void*> allocs;        // every device allocation of finalize()
    const float *wte = nullptr, *wpe = nullptr, *ln_f = nullptr;
    std::vector<at::GptLayer> layers;
    int32_t* flags_host = nullptr;    // pinned: the rows' finish flags as the host last saw them (GPT_MAX_B words)
};
