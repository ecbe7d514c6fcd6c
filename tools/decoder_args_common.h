// What the ten stand-alone argument checks of the semantic decoder share (tools/gpt_*args.hip, fine_*args.hip, semantic_stream_args.hip): the error sink, the
// case bookkeeping, stand-ins for device pointers, exact-size copies of host arrays, finalized handles of both stages built by hand (csrc/gpt.h, csrc/fine.h)
// with dimensions and no device memory behind them, and stand-ins for the launchers the fine forward calls, which count their calls: a program that links
// fine.hip ends by showing that none was reached. A program that does not link gemm_f32.hip defines ARGS_STAND_IN_GEMM before it includes this header.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../audiotoken_amd/csrc/fine.h"
#include "../audiotoken_amd/csrc/gpt.h"
#include "../audiotoken_amd/csrc/w2vbert_kernels.h"
#include "../include/audiotoken_hip.h"

namespace at {
static std::string g_error;
static int g_launches = 0;
void set_error(const std::string& msg) { g_error = msg; }   // the library's lives in encodec.hip, which these programs do not link
#ifdef ARGS_STAND_IN_GEMM
int launch_gemm(const GemmArgs&, hipStream_t) { ++g_launches; return -1; }
#endif
int launch_relpos_attention(const AttnArgs&, hipStream_t) { ++g_launches; return -1; }
int launch_layernorm(const float*, const float*, const float*, const float*, float*, long long, int, hipStream_t) { ++g_launches; return -1; }
}  // namespace at

static int failures = 0;

static void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s (last error: %s)\n", what, at::g_error.c_str());
        ++failures;
    }
}
static bool refused(int rc, const char* text) { return rc != 0 && at::g_error.find(text) != std::string::npos; }
static int verdict(const char* name) {
    if (failures) {
        std::printf("%d case(s) failed\n", failures);
        return 1;
    }
    std::printf("%s: ok\n", name);
    return 0;
}

// stand-ins for device pointers: never dereferenced by a call that is refused
static int32_t fake_i[4];
static float fake_f[4];

// a host array in a heap block of exactly the size the call may read, so that a read past it is a sanitizer report; nullptr for an empty one
static std::unique_ptr<int32_t[]> exact_copy(const std::vector<int32_t>& v) {
    if (v.empty()) return nullptr;
    std::unique_ptr<int32_t[]> p(new int32_t[v.size()]);
    std::memcpy(p.get(), v.data(), v.size() * sizeof(int32_t));
    return p;
}

// a 2-layer GPT of 128 positions, finalized by hand
static void finalize_by_hand(at_gpt* model, int vocab) {
    model->finalized = true;
    model->n_layer = 2;
    model->vocab = vocab;
    model->block = 128;
    model->layers.resize(2);
}
// a 2-layer fine model of 768 channels and a window of 128, finalized by hand
static void finalize_by_hand(at_fine* model) {
    model->finalized = true;
    model->n_layer = 2;
    model->embd = 768;
    model->block = 128;
    model->layers.resize(2);
}

constexpr int INT_MAX_ = std::numeric_limits<int>::max(), INT_MIN_ = std::numeric_limits<int>::min();
