// The argument checks of teacher-forced scoring (audiotoken_amd/csrc/gpt_score.hip: at_gpt_score, at_gpt_score_state_bytes, at_op_score_rows)
// under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program. Every case below is refused before anything is launched, so it needs no
// device: the handle is a finalized at_gpt built by hand (decoder_args_common.h). Built and run by `make -C audiotoken_amd/csrc gpt_score_asan`:
//   hipcc --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined tools/gpt_score_args.hip audiotoken_amd/csrc/{gpt_score,gpt,gpt_model,gemm_f32}.hip
#include "decoder_args_common.h"

struct Call {
    at_gpt* h;
    const int32_t* seq = fake_i;
    int stride = 100;
    std::vector<int32_t> lens{100, 7}, from{40, 1};
    int n_rows = 2;
    float temperature = 1.0f;
    std::vector<int32_t> allow;   // empty: none
    float* logprob = fake_f;
    int32_t* rank = fake_i;
    int out_stride = 60;
    void* state = fake_f;
    size_t state_bytes = 0;
    int rows = 2, max_len = 100, pass_tokens = 200, head_rows = 16;

    int run() const {
        const auto l = exact_copy(lens), f = exact_copy(from), a = exact_copy(allow);
        at::g_error.clear();
        return at_gpt_score(h, seq, stride, l.get(), f.get(), n_rows, temperature, a.get(), logprob, rank, out_stride, nullptr, state, state_bytes, rows, max_len,
                            pass_tokens, head_rows, nullptr, nullptr);
    }
};

int main() {
    at_gpt model;
    finalize_by_hand(&model, 128);
    at_gpt raw;   // never finalized

    // ---- at_gpt_score_state_bytes
    at::g_error.clear();
    const size_t base = at_gpt_score_state_bytes(&model, 2, 100, 200, 16);
    expect(base > 0, "state bytes of a small call");
    expect(at_gpt_score_state_bytes(&model, 3, 100, 200, 16) > base, "state bytes grow with the cache rows");
    expect(at_gpt_score_state_bytes(&model, 2, 101, 200, 16) > base, "state bytes grow with max_len");
    expect(at_gpt_score_state_bytes(&model, 2, 100, 201, 16) > base, "state bytes grow with pass_tokens");
    expect(at_gpt_score_state_bytes(&model, 2, 100, 200, 32) - base == 16 * 128 * 4, "state bytes grow with head_rows by one chunk's logits");
    expect(at_gpt_score_state_bytes(&model, 64, 128, 65600, 4096) > 0, "the largest state");
    expect(at_gpt_score_state_bytes(nullptr, 2, 100, 200, 16) == 0 && at::g_error.find("not finalized") != std::string::npos, "state bytes of a null handle");
    expect(at_gpt_score_state_bytes(&raw, 2, 100, 200, 16) == 0, "state bytes before finalize");
    expect(at_gpt_score_state_bytes(&model, 0, 100, 200, 16) == 0 && at::g_error.find("rows must be") != std::string::npos, "state bytes, rows = 0");
    expect(at_gpt_score_state_bytes(&model, 65, 100, 200, 16) == 0, "state bytes, rows = 65");
    expect(at_gpt_score_state_bytes(&model, INT_MIN_, 100, 200, 16) == 0, "state bytes, rows = INT_MIN");
    expect(at_gpt_score_state_bytes(&model, 2, 1, 200, 16) == 0 && at::g_error.find("max_len") != std::string::npos, "state bytes, max_len = 1");
    expect(at_gpt_score_state_bytes(&model, 2, 129, 200, 16) == 0, "state bytes, max_len past the block");
    expect(at_gpt_score_state_bytes(&model, 2, 100, 99, 16) == 0 && at::g_error.find("pass_tokens") != std::string::npos, "state bytes, pass_tokens below max_len");
    expect(at_gpt_score_state_bytes(&model, 2, 100, 65601, 16) == 0, "state bytes, pass_tokens past 65600");
    expect(at_gpt_score_state_bytes(&model, 2, 100, INT_MAX_, 16) == 0, "state bytes, pass_tokens = INT_MAX");
    expect(at_gpt_score_state_bytes(&model, 2, 100, 200, 0) == 0 && at::g_error.find("head_rows") != std::string::npos, "state bytes, head_rows = 0");
    expect(at_gpt_score_state_bytes(&model, 2, 100, 200, 24) == 0, "state bytes, head_rows no multiple of 16");
    expect(at_gpt_score_state_bytes(&model, 2, 100, 200, 4112) == 0, "state bytes, head_rows past 4096");
    expect(at_gpt_score_state_bytes(&model, 2, 100, 200, INT_MIN_) == 0, "state bytes, head_rows = INT_MIN");

    // ---- at_gpt_score: a well-formed call with a state that is too small is refused last, which shows the rest was accepted
    Call ok{&model};
    ok.state_bytes = 16;
    expect(refused(ok.run(), "state too small"), "a state that is too small");
    { Call c = ok; c.state_bytes = base - 1; expect(refused(c.run(), "state too small"), "a state one byte short"); }
    { Call c = ok; c.h = nullptr; expect(refused(c.run(), "not finalized"), "a null handle"); }
    { Call c = ok; c.h = &raw; expect(refused(c.run(), "not finalized"), "a handle before finalize"); }
    { Call c = ok; c.n_rows = 0; expect(refused(c.run(), "n_rows"), "n_rows = 0"); }
    { Call c = ok; c.n_rows = 65537; expect(refused(c.run(), "n_rows"), "n_rows = 65537"); }
    { Call c = ok; c.n_rows = INT_MIN_; expect(refused(c.run(), "n_rows"), "n_rows = INT_MIN"); }
    { Call c = ok; c.seq = nullptr; expect(refused(c.run(), "null pointer"), "null seq"); }
    { Call c = ok; c.lens.clear(); expect(refused(c.run(), "null pointer"), "null seq_len"); }
    { Call c = ok; c.from.clear(); expect(refused(c.run(), "null pointer"), "null score_from"); }
    { Call c = ok; c.logprob = nullptr; expect(refused(c.run(), "null pointer"), "null logprob_out"); }
    { Call c = ok; c.rank = nullptr; expect(refused(c.run(), "null pointer"), "null rank_out"); }
    { Call c = ok; c.state = nullptr; c.state_bytes = base; expect(refused(c.run(), "null state"), "a null state"); }
    { Call c = ok; c.stride = 1; expect(refused(c.run(), "seq_stride"), "seq_stride = 1"); }
    { Call c = ok; c.out_stride = 0; expect(refused(c.run(), "out_stride"), "out_stride = 0"); }
    { Call c = ok; c.out_stride = INT_MAX_; expect(refused(c.run(), "2^31"), "n_rows * out_stride past 2^31"); }
    { Call c = ok; c.out_stride = 59; expect(refused(c.run(), "row 0 scores more positions than out_stride"), "out_stride one short"); }
    { Call c = ok; c.lens = {101, 7}; expect(refused(c.run(), "seq_len of row 0"), "a row longer than max_len"); }
    { Call c = ok; c.max_len = 128; c.pass_tokens = 256; c.lens = {101, 7}; expect(refused(c.run(), "seq_len of row 0"), "a row longer than seq_stride"); }
    { Call c = ok; c.lens = {100, 1}; expect(refused(c.run(), "seq_len of row 1"), "a row of one id"); }
    { Call c = ok; c.lens = {100, INT_MIN_}; expect(refused(c.run(), "seq_len of row 1"), "seq_len = INT_MIN"); }
    { Call c = ok; c.lens = {INT_MAX_, 7}; expect(refused(c.run(), "seq_len of row 0"), "seq_len = INT_MAX"); }
    { Call c = ok; c.from = {0, 1}; expect(refused(c.run(), "score_from of row 0"), "score_from = 0"); }
    { Call c = ok; c.from = {40, 7}; expect(refused(c.run(), "score_from of row 1"), "score_from = seq_len"); }
    { Call c = ok; c.from = {INT_MIN_, 1}; expect(refused(c.run(), "score_from of row 0"), "score_from = INT_MIN"); }
    { Call c = ok; c.from = {40, INT_MAX_}; expect(refused(c.run(), "score_from of row 1"), "score_from = INT_MAX"); }
    { Call c = ok; c.temperature = 0.0f; expect(refused(c.run(), "temperature"), "temperature = 0"); }
    { Call c = ok; c.temperature = -1.0f; expect(refused(c.run(), "temperature"), "temperature < 0"); }
    { Call c = ok; c.temperature = std::nanf(""); expect(refused(c.run(), "temperature"), "temperature = NaN"); }
    { Call c = ok; c.temperature = std::numeric_limits<float>::infinity(); expect(refused(c.run(), "temperature"), "temperature = inf"); }
    { Call c = ok; c.rows = 0; expect(refused(c.run(), "rows must be"), "rows = 0"); }
    { Call c = ok; c.rows = 65; expect(refused(c.run(), "rows must be"), "rows = 65"); }
    { Call c = ok; c.max_len = 129; expect(refused(c.run(), "max_len"), "max_len past the block"); }
    { Call c = ok; c.pass_tokens = 99; expect(refused(c.run(), "pass_tokens"), "pass_tokens below max_len"); }
    { Call c = ok; c.head_rows = 8; expect(refused(c.run(), "head_rows"), "head_rows = 8"); }
    { Call c = ok; c.head_rows = 4100; expect(refused(c.run(), "head_rows"), "head_rows past 4096"); }
    { Call c = ok; c.allow = {0, 64, 0, 0, 64, 128, 0, 0}; expect(refused(c.run(), "state too small"), "well-formed allow ranges"); }
    { Call c = ok; c.allow = {0, 129, 0, 0, 64, 128, 0, 0}; expect(refused(c.run(), "allow ranges"), "an allow range past the vocabulary"); }
    { Call c = ok; c.allow = {0, 64, 0, 0, 70, 64, 0, 0}; expect(refused(c.run(), "allow ranges"), "an allow range with lo > hi at odd positions"); }
    { Call c = ok; c.allow = {5, 5, 0, 0, 64, 128, 0, 0}; expect(refused(c.run(), "both empty"), "allow ranges that allow nothing"); }
    { Call c = ok; c.n_rows = 1; c.lens = {100}; c.from = {99}; c.out_stride = 1; expect(refused(c.run(), "state too small"), "one row scored at its last id alone"); }

    // ---- at_op_score_rows
    auto score = [&](const float* z, int R, int V, const int32_t* t, float temp, std::vector<int32_t> allow, float* lp, int32_t* rank) {
        const auto a = exact_copy(allow);
        at::g_error.clear();
        return at_op_score_rows(z, R, V, t, temp, a.get(), lp, rank, nullptr);
    };
    expect(refused(score(nullptr, 1, 128, fake_i, 1.f, {}, fake_f, fake_i), "null pointer"), "score rows: null logits");
    expect(refused(score(fake_f, 1, 128, nullptr, 1.f, {}, fake_f, fake_i), "null pointer"), "score rows: null targets");
    expect(refused(score(fake_f, 1, 128, fake_i, 1.f, {}, nullptr, fake_i), "null pointer"), "score rows: null logprob_out");
    expect(refused(score(fake_f, 1, 128, fake_i, 1.f, {}, fake_f, nullptr), "null pointer"), "score rows: null rank_out");
    expect(refused(score(fake_f, 0, 128, fake_i, 1.f, {}, fake_f, fake_i), "R must be"), "score rows: R = 0");
    expect(refused(score(fake_f, 65537, 128, fake_i, 1.f, {}, fake_f, fake_i), "R must be"), "score rows: R = 65537");
    expect(refused(score(fake_f, 1, 0, fake_i, 1.f, {}, fake_f, fake_i), "V must be"), "score rows: V = 0");
    expect(refused(score(fake_f, 1, 65537, fake_i, 1.f, {}, fake_f, fake_i), "V must be"), "score rows: V = 65537");
    expect(refused(score(fake_f, 1, 128, fake_i, 0.f, {}, fake_f, fake_i), "temperature"), "score rows: temperature = 0");
    expect(refused(score(fake_f, 1, 128, fake_i, std::nanf(""), {}, fake_f, fake_i), "temperature"), "score rows: temperature = NaN");
    expect(refused(score(fake_f, 1, 128, fake_i, 1.f, {0, 129, 0, 0}, fake_f, fake_i), "allow ranges"), "score rows: an allow range past V");
    expect(refused(score(fake_f, 1, 128, fake_i, 1.f, {3, 3, 9, 9}, fake_f, fake_i), "both empty"), "score rows: allow ranges that allow nothing");
    return verdict("gpt score argument checks");
}
