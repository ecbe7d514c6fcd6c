// The argument checks of the GPT decoder's entry points (audiotoken_amd/csrc/gpt.hip: at_gpt_generate, at_gpt_state_bytes; gpt_model.hip: at_op_topk_sample) under
// AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program. Every case below is refused before anything is launched, so it needs no
// device: the handle is a finalized at_gpt built by hand (decoder_args_common.h). Built and run by `make -C audiotoken_amd/csrc gpt_asan`:
//   hipcc --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined tools/gpt_args.hip audiotoken_amd/csrc/{gpt,gpt_model,gemm_f32}.hip
// (gemm_f32.hip only because the model pass calls its launcher; nothing of it runs here).
#include "decoder_args_common.h"

struct Call {
    at_gpt* h;
    const int32_t* prompts = fake_i;
    int stride = 100;
    std::vector<int32_t> lens{100, 7};
    int B = 2, max_new = 16;
    float temperature = 0.8f;
    int top_k = 100, stop = -1;
    const float* uniforms = fake_f;
    std::vector<int32_t> allow;   // empty: none
    int32_t *out_ids = fake_i, *out_len = fake_i, *finish = fake_i;
    void* state = fake_f;
    size_t state_bytes = 0;
    int max_len = 116;

    int run() const {
        const auto l = exact_copy(lens), a = exact_copy(allow);
        at::g_error.clear();
        return at_gpt_generate(h, prompts, stride, l.get(), B, max_new, temperature, top_k, stop, uniforms, a.get(), out_ids, out_len, finish, nullptr, state,
                               state_bytes, max_len, nullptr, nullptr);
    }
};

int main() {
    at_gpt model;
    finalize_by_hand(&model, 128);
    at_gpt raw;   // never finalized

    // ---- at_gpt_state_bytes
    at::g_error.clear();
    expect(at_gpt_state_bytes(&model, 1, 128) > 0, "state bytes of one row");
    expect(at_gpt_state_bytes(&model, 64, 128) > at_gpt_state_bytes(&model, 1, 128), "state bytes grow with B");
    expect(at_gpt_state_bytes(&model, 2, 128) > at_gpt_state_bytes(&model, 2, 64), "state bytes grow with max_len");
    expect(at_gpt_state_bytes(nullptr, 1, 64) == 0 && at::g_error.find("not finalized") != std::string::npos, "state bytes of a null handle");
    expect(at_gpt_state_bytes(&raw, 1, 64) == 0, "state bytes before finalize");
    expect(at_gpt_state_bytes(&model, 0, 64) == 0 && at::g_error.find("B must be") != std::string::npos, "state bytes, B = 0");
    expect(at_gpt_state_bytes(&model, 65, 64) == 0, "state bytes, B = 65");
    expect(at_gpt_state_bytes(&model, INT_MIN_, 64) == 0, "state bytes, B = INT_MIN");
    expect(at_gpt_state_bytes(&model, 1, 0) == 0 && at::g_error.find("max_len") != std::string::npos, "state bytes, max_len = 0");
    expect(at_gpt_state_bytes(&model, 1, 129) == 0, "state bytes, max_len past the block");
    expect(at_gpt_state_bytes(&model, 1, INT_MAX_) == 0, "state bytes, max_len = INT_MAX");
    expect(at_gpt_num_layers(&model) == 2 && at_gpt_vocab(&model) == 128 && at_gpt_block_size(&model) == 128, "the getters");
    expect(at_gpt_num_layers(&raw) == 0 && at_gpt_vocab(nullptr) == 0, "the getters before finalize");

    // ---- at_gpt_generate: a well-formed call with a state that is too small is refused last, which shows the rest was accepted
    Call ok{&model};
    ok.state_bytes = 16;
    expect(refused(ok.run(), "state too small"), "a state that is too small");
    const size_t need = at_gpt_state_bytes(&model, 2, 116);
    { Call c = ok; c.state_bytes = need - 1; expect(refused(c.run(), "state too small"), "a state one byte short"); }
    { Call c = ok; c.h = nullptr; expect(refused(c.run(), "not finalized"), "a null handle"); }
    { Call c = ok; c.h = &raw; expect(refused(c.run(), "not finalized"), "a handle before finalize"); }
    { Call c = ok; c.B = 0; expect(refused(c.run(), "B must be"), "B = 0"); }
    { Call c = ok; c.B = 65; expect(refused(c.run(), "B must be"), "B = 65"); }
    { Call c = ok; c.B = -1; expect(refused(c.run(), "B must be"), "B = -1"); }
    { Call c = ok; c.prompts = nullptr; expect(refused(c.run(), "null pointer"), "null prompts"); }
    { Call c = ok; c.lens.clear(); expect(refused(c.run(), "null pointer"), "null prompt_len"); }
    { Call c = ok; c.uniforms = nullptr; expect(refused(c.run(), "null pointer"), "null uniforms"); }
    { Call c = ok; c.out_ids = nullptr; expect(refused(c.run(), "null pointer"), "null out_ids"); }
    { Call c = ok; c.out_len = nullptr; expect(refused(c.run(), "null pointer"), "null out_len"); }
    { Call c = ok; c.finish = nullptr; expect(refused(c.run(), "null pointer"), "null finish"); }
    { Call c = ok; c.state = nullptr; c.state_bytes = need; expect(refused(c.run(), "null state"), "a null state"); }
    { Call c = ok; c.stride = 0; expect(refused(c.run(), "prompt_stride"), "prompt_stride = 0"); }
    { Call c = ok; c.stride = 129; expect(refused(c.run(), "prompt_stride"), "prompt_stride past the block"); }
    { Call c = ok; c.lens = {100, 129}; expect(refused(c.run(), "longer than the model's block"), "a prompt longer than the block"); }
    { Call c = ok; c.lens = {100, 101}; expect(refused(c.run(), "row 1 must be 1 to prompt_stride"), "a prompt longer than its row"); }
    { Call c = ok; c.lens = {0, 7}; expect(refused(c.run(), "row 0 must be 1 to prompt_stride"), "an empty prompt"); }
    { Call c = ok; c.lens = {100, INT_MIN_}; expect(refused(c.run(), "row 1"), "prompt_len = INT_MIN"); }
    { Call c = ok; c.lens = {INT_MAX_, 7}; expect(refused(c.run(), "row 0"), "prompt_len = INT_MAX"); }
    { Call c = ok; c.max_new = 0; expect(refused(c.run(), "max_new"), "max_new = 0"); }
    { Call c = ok; c.max_new = 1025; expect(refused(c.run(), "max_new"), "max_new = 1025"); }
    { Call c = ok; c.max_new = INT_MAX_; expect(refused(c.run(), "max_new"), "max_new = INT_MAX"); }
    { Call c = ok; c.temperature = 0.0f; expect(refused(c.run(), "temperature"), "temperature = 0"); }
    { Call c = ok; c.temperature = -1.0f; expect(refused(c.run(), "temperature"), "temperature < 0"); }
    { Call c = ok; c.temperature = std::nanf(""); expect(refused(c.run(), "temperature"), "temperature = NaN"); }
    { Call c = ok; c.temperature = std::numeric_limits<float>::infinity(); expect(refused(c.run(), "temperature"), "temperature = inf"); }
    { Call c = ok; c.top_k = 0; expect(refused(c.run(), "top_k"), "top_k = 0"); }
    { Call c = ok; c.top_k = -5; expect(refused(c.run(), "top_k"), "top_k < 0"); }
    { Call c = ok; c.stop = 128; expect(refused(c.run(), "stop_token"), "a stop token outside the vocabulary"); }
    { Call c = ok; c.max_len = 115; c.state_bytes = need; expect(refused(c.run(), "max_len"), "max_len one short of prompt + max_new"); }
    { Call c = ok; c.max_len = 129; c.state_bytes = need; expect(refused(c.run(), "max_len"), "max_len past the block"); }
    { Call c = ok; c.max_new = 1000; c.max_len = 128; expect(refused(c.run(), "state too small"), "prompt + max_new past the block: max_len = block is enough"); }
    { Call c = ok; c.allow = {0, 64, 0, 0, 64, 128, 0, 0}; expect(refused(c.run(), "state too small"), "well-formed allow ranges"); }
    { Call c = ok; c.allow = {0, 129, 0, 0, 64, 128, 0, 0}; expect(refused(c.run(), "allow ranges"), "an allow range past the vocabulary"); }
    { Call c = ok; c.allow = {0, 64, 0, 0, 70, 64, 0, 0}; expect(refused(c.run(), "allow ranges"), "an allow range with lo > hi at odd steps"); }
    { Call c = ok; c.allow = {-1, 64, 0, 0, 64, 128, 0, 0}; expect(refused(c.run(), "allow ranges"), "a negative allow bound"); }
    { Call c = ok; c.allow = {5, 5, 0, 0, 64, 128, 0, 0}; expect(refused(c.run(), "both empty"), "allow ranges that allow nothing"); }

    // ---- at_op_topk_sample
    auto sample = [&](const float* z, int B, int V, float t, int k, const float* u, std::vector<int32_t> allow, int32_t* out) {
        const auto a = exact_copy(allow);
        at::g_error.clear();
        return at_op_topk_sample(z, B, V, t, k, u, a.get(), out, nullptr);
    };
    expect(refused(sample(nullptr, 1, 128, 1.f, 1, fake_f, {}, fake_i), "null pointer"), "sample: null logits");
    expect(refused(sample(fake_f, 1, 128, 1.f, 1, nullptr, {}, fake_i), "null pointer"), "sample: null uniforms");
    expect(refused(sample(fake_f, 1, 128, 1.f, 1, fake_f, {}, nullptr), "null pointer"), "sample: null out");
    expect(refused(sample(fake_f, 0, 128, 1.f, 1, fake_f, {}, fake_i), "B must be"), "sample: B = 0");
    expect(refused(sample(fake_f, 65536, 128, 1.f, 1, fake_f, {}, fake_i), "B must be"), "sample: B = 65536");
    expect(refused(sample(fake_f, 1, 0, 1.f, 1, fake_f, {}, fake_i), "V must be"), "sample: V = 0");
    expect(refused(sample(fake_f, 1, 65537, 1.f, 1, fake_f, {}, fake_i), "V must be"), "sample: V = 65537");
    expect(refused(sample(fake_f, 1, 128, 0.f, 1, fake_f, {}, fake_i), "temperature"), "sample: temperature = 0");
    expect(refused(sample(fake_f, 1, 128, 1.f, 0, fake_f, {}, fake_i), "top_k"), "sample: top_k = 0");
    expect(refused(sample(fake_f, 1, 128, 1.f, 1, fake_f, {0, 129, 0, 0}, fake_i), "allow ranges"), "sample: an allow range past V");
    expect(refused(sample(fake_f, 1, 128, 1.f, 1, fake_f, {3, 3, 9, 9}, fake_i), "both empty"), "sample: allow ranges that allow nothing");
    return verdict("gpt argument checks");
}
