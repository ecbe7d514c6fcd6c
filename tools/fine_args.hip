// The argument checks of the fine stage's entry points (audiotoken_amd/csrc/fine.hip: at_fine_generate, at_fine_state_bytes, at_fine_num_windows) under
// AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program. Every case below is refused before anything is launched, so it needs no
// device: the handle is a finalized at_fine built here by hand (fine.h), with dimensions and no device memory behind it. Built and run by
// `make -C audiotoken_amd/csrc fine_asan`:
//   hipcc --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined tools/fine_args.hip audiotoken_amd/csrc/fine.hip
// The three launchers fine.hip's forward calls (GEMM, attention, LayerNorm) are stand-ins that count their calls (decoder_args_common.h): the program ends by
// showing that none was reached. The host array (the rows' lengths) lives in a heap block of exactly the size the call may read.
#define ARGS_STAND_IN_GEMM
#include "decoder_args_common.h"

struct Call {
    at_fine* h;
    const int32_t* coarse = fake_i;
    int stride = 300;
    std::vector<int32_t> lens{300, 1};
    int B = 2;
    float temperature = 0.5f;
    int greedy = 0;
    const float* uniforms = fake_f;
    int n_max = 4;
    int32_t* out = fake_i;
    void* state = fake_f;
    size_t state_bytes = 0;
    int max_T = 300;

    int run() const {
        const auto l = exact_copy(lens);
        at::g_error.clear();
        return at_fine_generate(h, coarse, stride, l.get(), B, temperature, greedy, uniforms, n_max, out, nullptr, nullptr, state,
                                state_bytes, max_T, nullptr, nullptr);
    }
};

int main() {
    at_fine model;
    finalize_by_hand(&model);
    at_fine raw;   // never finalized

    // ---- the window count: n = max(0, ceil((T - W) / H)) + 1
    const int W = 128, H = 64;
    const int Ts[8] = {1, H, W - 1, W, W + 1, W + H, W + H + 1, 2 * W + 3}, want[8] = {1, 1, 1, 1, 2, 2, 3, 4};
    for (int i = 0; i < 8; ++i) expect(at_fine_num_windows(&model, Ts[i]) == want[i], "the window count");
    expect(at_fine_num_windows(&model, 0) == 0 && at::g_error.find("T must be") != std::string::npos, "windows of T = 0");
    expect(at_fine_num_windows(&model, (1 << 18) + 1) == 0, "windows of T past the limit");
    expect(at_fine_num_windows(&model, std::numeric_limits<int>::max()) == 0, "windows of T = INT_MAX");
    expect(at_fine_num_windows(&model, std::numeric_limits<int>::min()) == 0, "windows of T = INT_MIN");
    expect(at_fine_num_windows(&raw, 5) == 0 && at_fine_num_windows(nullptr, 5) == 0, "windows before finalize");
    expect(at_fine_num_windows(&model, 1 << 18) == (1 << 18) / H - 1, "windows of the longest row");

    // ---- at_fine_state_bytes
    at::g_error.clear();
    expect(at_fine_state_bytes(&model, 1, 1) > 0, "state bytes of one row");
    expect(at_fine_state_bytes(&model, 1, 1) == at_fine_state_bytes(&model, 1, 128), "a row shorter than the window works in a whole window");
    expect(at_fine_state_bytes(&model, 64, 128) > at_fine_state_bytes(&model, 1, 128), "state bytes grow with B");
    expect(at_fine_state_bytes(&model, 2, 1000) > at_fine_state_bytes(&model, 2, 128), "state bytes grow with max_T");
    expect(at_fine_state_bytes(nullptr, 1, 64) == 0 && at::g_error.find("not finalized") != std::string::npos, "state bytes of a null handle");
    expect(at_fine_state_bytes(&raw, 1, 64) == 0, "state bytes before finalize");
    expect(at_fine_state_bytes(&model, 0, 64) == 0 && at::g_error.find("B must be") != std::string::npos, "state bytes, B = 0");
    expect(at_fine_state_bytes(&model, 65, 64) == 0, "state bytes, B = 65");
    expect(at_fine_state_bytes(&model, std::numeric_limits<int>::min(), 64) == 0, "state bytes, B = INT_MIN");
    expect(at_fine_state_bytes(&model, 1, 0) == 0 && at::g_error.find("max_T") != std::string::npos, "state bytes, max_T = 0");
    expect(at_fine_state_bytes(&model, 1, (1 << 18) + 1) == 0, "state bytes, max_T past the limit");
    expect(at_fine_state_bytes(&model, 1, std::numeric_limits<int>::max()) == 0, "state bytes, max_T = INT_MAX");
    expect(at_fine_state_bytes(&model, 64, 1 << 18) > 0, "state bytes of the largest call");
    expect(at_fine_num_layers(&model) == 2 && at_fine_hidden(&model) == 768 && at_fine_block_size(&model) == 128 && at_fine_has_bias(&model) == 0, "the getters");
    expect(at_fine_num_layers(&raw) == 0 && at_fine_hidden(nullptr) == 0 && at_fine_block_size(&raw) == 0, "the getters before finalize");

    // ---- at_fine_generate: a well-formed call with a state that is too small is refused last, which shows the rest was accepted
    Call ok{&model};
    ok.state_bytes = 16;
    expect(refused(ok.run(), "state too small"), "a state that is too small");
    const size_t need = at_fine_state_bytes(&model, 2, 300);
    { Call c = ok; c.state_bytes = need - 1; expect(refused(c.run(), "state too small"), "a state one byte short"); }
    { Call c = ok; c.h = nullptr; expect(refused(c.run(), "not finalized"), "a null handle"); }
    { Call c = ok; c.h = &raw; expect(refused(c.run(), "not finalized"), "a handle before finalize"); }
    { Call c = ok; c.B = 0; expect(refused(c.run(), "B must be"), "B = 0"); }
    { Call c = ok; c.B = 65; expect(refused(c.run(), "B must be"), "B = 65"); }
    { Call c = ok; c.B = -1; expect(refused(c.run(), "B must be"), "B = -1"); }
    { Call c = ok; c.coarse = nullptr; expect(refused(c.run(), "null pointer"), "null coarse codes"); }
    { Call c = ok; c.lens.clear(); expect(refused(c.run(), "null pointer"), "null lens"); }
    { Call c = ok; c.out = nullptr; expect(refused(c.run(), "null pointer"), "null out"); }
    { Call c = ok; c.uniforms = nullptr; expect(refused(c.run(), "null pointer"), "sampling without uniforms"); }
    { Call c = ok; c.uniforms = nullptr; c.greedy = 1; expect(refused(c.run(), "state too small"), "the argmax needs no uniforms"); }
    { Call c = ok; c.greedy = 1; c.temperature = std::nanf(""); expect(refused(c.run(), "state too small"), "the argmax reads no temperature"); }
    { Call c = ok; c.greedy = 2; expect(refused(c.run(), "greedy"), "greedy = 2"); }
    { Call c = ok; c.state = nullptr; c.state_bytes = need; expect(refused(c.run(), "null state"), "a null state"); }
    { Call c = ok; c.stride = 0; expect(refused(c.run(), "t_stride"), "t_stride = 0"); }
    { Call c = ok; c.stride = (1 << 18) + 1; expect(refused(c.run(), "t_stride"), "t_stride past the limit"); }
    { Call c = ok; c.stride = 299; expect(refused(c.run(), "row 0 must be"), "a row longer than its stride"); }
    { Call c = ok; c.max_T = 299; expect(refused(c.run(), "row 0 must be"), "a row longer than max_T"); }
    { Call c = ok; c.max_T = 0; expect(refused(c.run(), "max_T"), "max_T = 0"); }
    { Call c = ok; c.max_T = std::numeric_limits<int>::max(); expect(refused(c.run(), "max_T"), "max_T = INT_MAX"); }
    { Call c = ok; c.lens = {300, 0}; expect(refused(c.run(), "row 1 must be"), "an empty row"); }
    { Call c = ok; c.lens = {300, std::numeric_limits<int32_t>::min()}; expect(refused(c.run(), "row 1"), "a length of INT_MIN"); }
    { Call c = ok; c.lens = {std::numeric_limits<int32_t>::max(), 1}; expect(refused(c.run(), "row 0"), "a length of INT_MAX"); }
    { Call c = ok; c.temperature = 0.0f; expect(refused(c.run(), "temperature"), "temperature = 0"); }
    { Call c = ok; c.temperature = -1.0f; expect(refused(c.run(), "temperature"), "temperature < 0"); }
    { Call c = ok; c.temperature = std::nanf(""); expect(refused(c.run(), "temperature"), "temperature = NaN"); }
    { Call c = ok; c.temperature = std::numeric_limits<float>::infinity(); expect(refused(c.run(), "temperature"), "temperature = inf"); }
    { Call c = ok; c.n_max = 3; expect(refused(c.run(), "n_max"), "n_max one short: 300 frames at W = 128 are 4 windows"); }
    { Call c = ok; c.n_max = 0; expect(refused(c.run(), "n_max"), "n_max = 0"); }
    { Call c = ok; c.n_max = 9; expect(refused(c.run(), "state too small"), "an n_max larger than needed"); }
    expect(at::g_launches == 0, "no case reached a launch");
    return verdict("fine argument checks");
}
