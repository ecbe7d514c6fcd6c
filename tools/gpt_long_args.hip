// The argument and schedule checks of the long form's entry points (audiotoken_amd/csrc/gpt.hip: at_gpt_generate_long, at_gpt_long_state_bytes,
// at_gpt_long_num_windows) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program, the way tools/gpt_args.hip checks at_gpt_generate:
// the handle is a finalized at_gpt built by hand (decoder_args_common.h) and every case is refused before anything is launched. Built and run by
// `make -C audiotoken_amd/csrc gpt_long_asan`.
#include "decoder_args_common.h"

// A model of 128 positions and 256 ids: semantic ids [0, 64), the two code books [64, 128) and [128, 192), INFER 200, STOP 201. S = 8, H = 4, r = 3:
// a window holds 8 + 1 + 24 = 33 positions; rows of 30 ids (7 windows: the last reads 6 ids, starts at stream 84, carries 12) and 5 ids (one window).
struct Call {
    at_gpt* h;
    const int32_t* src = fake_i;
    int stride = 30;
    std::vector<int32_t> lens{30, 5};
    int B = 2, S = 8, H = 4, r = 3;
    int sem_off = 0, sem_vocab = 64, infer = 200, ac_off = 64, cb = 64, stop = 201;
    int max_new = 16;
    float temperature = 0.8f;
    int top_k = 100;
    const float* uniforms = fake_f;
    int u_stride = 100;        // 84 + min(16, 128 - 19)
    int32_t *out_ids = fake_i, *out_len = fake_i, *finish = fake_i;
    int out_stride = 100;
    void* state = fake_f;
    size_t state_bytes = 0;
    int max_len = 35;          // the final window of row 0: 6 + 1 + 12 + 16; a non-final one: 33

    int run() const {
        const auto l = exact_copy(lens);
        at::g_error.clear();
        return at_gpt_generate_long(h, src, stride, l.get(), B, S, H, r, sem_off, sem_vocab, infer, ac_off, cb, stop, max_new, temperature,
                                    top_k, uniforms, u_stride, out_ids, out_stride, out_len, finish, nullptr, state, state_bytes, max_len, nullptr, nullptr);
    }
};

int main() {
    at_gpt model;
    finalize_by_hand(&model, 256);
    at_gpt raw;   // never finalized

    // ---- the schedule's window count
    expect(at_gpt_long_num_windows(1, 8, 4) == 1 && at_gpt_long_num_windows(8, 8, 4) == 1 && at_gpt_long_num_windows(9, 8, 4) == 2, "windows up to S + 1");
    expect(at_gpt_long_num_windows(12, 8, 4) == 2 && at_gpt_long_num_windows(13, 8, 4) == 3 && at_gpt_long_num_windows(30, 8, 4) == 7, "windows past S + H");
    expect(at_gpt_long_num_windows(17, 8, 8) == 3 && at_gpt_long_num_windows(65536, 2, 2) == 32768, "windows without overlap");
    expect(at_gpt_long_num_windows(0, 8, 4) == 0 && at_gpt_long_num_windows(65537, 8, 4) == 0, "windows: N out of range");
    expect(at_gpt_long_num_windows(9, 7, 4) == 0 && at_gpt_long_num_windows(9, 8, 3) == 0 && at_gpt_long_num_windows(9, 8, 10) == 0, "windows: odd S, odd H, H > S");
    expect(at_gpt_long_num_windows(INT_MAX_, INT_MAX_, INT_MAX_) == 0 && at_gpt_long_num_windows(INT_MIN_, 8, 4) == 0, "windows: extreme values");

    // ---- at_gpt_long_state_bytes
    at::g_error.clear();
    expect(at_gpt_long_state_bytes(&model, 2, 35) >= at_gpt_state_bytes(&model, 2, 35), "the long state holds the plain one (one layout serves both calls)");
    expect(at_gpt_long_state_bytes(&model, 64, 128) > at_gpt_long_state_bytes(&model, 1, 128), "long state bytes grow with B");
    expect(at_gpt_long_state_bytes(nullptr, 1, 64) == 0 && at::g_error.find("not finalized") != std::string::npos, "long state bytes of a null handle");
    expect(at_gpt_long_state_bytes(&raw, 1, 64) == 0, "long state bytes before finalize");
    expect(at_gpt_long_state_bytes(&model, 0, 64) == 0 && at_gpt_long_state_bytes(&model, 65, 64) == 0 && at_gpt_long_state_bytes(&model, INT_MIN_, 64) == 0,
           "long state bytes, B out of range");
    expect(at_gpt_long_state_bytes(&model, 1, 0) == 0 && at_gpt_long_state_bytes(&model, 1, 129) == 0 && at_gpt_long_state_bytes(&model, 1, INT_MAX_) == 0,
           "long state bytes, max_len out of range");

    // ---- at_gpt_generate_long: a well-formed call with a state that is too small is refused last, which shows the rest was accepted
    Call ok{&model};
    ok.state_bytes = 16;
    expect(refused(ok.run(), "state too small"), "a state that is too small");
    const size_t need = at_gpt_long_state_bytes(&model, 2, 35);
    { Call c = ok; c.state_bytes = need - 1; expect(refused(c.run(), "state too small"), "a state one byte short"); }
    { Call c = ok; c.state_bytes = at_gpt_state_bytes(&model, 2, 35) - 1; expect(refused(c.run(), "state too small"), "the plain call's state, one byte short"); }
    { Call c = ok; c.h = nullptr; expect(refused(c.run(), "not finalized"), "a null handle"); }
    { Call c = ok; c.h = &raw; expect(refused(c.run(), "not finalized"), "a handle before finalize"); }
    for (int B : {0, 65, -1, INT_MIN_}) { Call c = ok; c.B = B; expect(refused(c.run(), "B must be"), "B out of range"); }
    { Call c = ok; c.src = nullptr; expect(refused(c.run(), "null pointer"), "null src"); }
    { Call c = ok; c.lens.clear(); expect(refused(c.run(), "null pointer"), "null src_len"); }
    { Call c = ok; c.uniforms = nullptr; expect(refused(c.run(), "null pointer"), "null uniforms"); }
    { Call c = ok; c.out_ids = nullptr; expect(refused(c.run(), "null pointer"), "null out_ids"); }
    { Call c = ok; c.out_len = nullptr; expect(refused(c.run(), "null pointer"), "null out_len"); }
    { Call c = ok; c.finish = nullptr; expect(refused(c.run(), "null pointer"), "null finish"); }
    { Call c = ok; c.state = nullptr; c.state_bytes = need; expect(refused(c.run(), "null state"), "a null state"); }
    // the schedule
    { Call c = ok; c.S = 7; expect(refused(c.run(), "must be even"), "an odd window"); }
    { Call c = ok; c.H = 3; expect(refused(c.run(), "must be even"), "an odd hop"); }
    { Call c = ok; c.H = 0; expect(refused(c.run(), "must be even"), "hop 0"); }
    { Call c = ok; c.S = 0; expect(refused(c.run(), "must be even"), "window 0"); }
    { Call c = ok; c.S = -8; expect(refused(c.run(), "must be even"), "a negative window"); }
    { Call c = ok; c.H = 10; expect(refused(c.run(), "must not exceed the window"), "a hop past the window"); }
    { Call c = ok; c.S = 32; c.H = 16; expect(refused(c.run(), "does not fit"), "S + 1 + r S one past the block (129)"); }
    { Call c = ok; c.S = INT_MAX_ - 1; c.H = 2; expect(refused(c.run(), "does not fit"), "S = INT_MAX - 1"); }
    { Call c = ok; c.r = 0; expect(refused(c.run(), "r (acoustic ids"), "r = 0"); }
    { Call c = ok; c.r = INT_MAX_; expect(refused(c.run(), "r (acoustic ids"), "r = INT_MAX"); }
    { Call c = ok; c.r = 15; expect(refused(c.run(), "does not fit"), "r too large for the block (8 + 1 + 120)"); }
    // the sources
    { Call c = ok; c.stride = 0; expect(refused(c.run(), "src_stride"), "src_stride = 0"); }
    { Call c = ok; c.lens = {30, 0}; expect(refused(c.run(), "row 1 must be 1 to"), "an empty source"); }
    { Call c = ok; c.lens = {31, 5}; expect(refused(c.run(), "row 0 must be 1 to"), "a source longer than its row"); }
    { Call c = ok; c.lens = {30, INT_MIN_}; expect(refused(c.run(), "row 1"), "src_len = INT_MIN"); }
    { Call c = ok; c.stride = INT_MAX_; c.lens = {65537, 5}; expect(refused(c.run(), "row 0"), "a source past 65536 ids"); }
    // the token space
    { Call c = ok; c.sem_off = -1; expect(refused(c.run(), "semantic ids"), "a negative semantic offset"); }
    { Call c = ok; c.sem_vocab = 0; expect(refused(c.run(), "semantic ids"), "an empty semantic vocabulary"); }
    { Call c = ok; c.sem_off = 200; c.sem_vocab = 57; expect(refused(c.run(), "semantic ids"), "semantic ids past the vocabulary"); }
    { Call c = ok; c.sem_off = INT_MAX_; c.sem_vocab = INT_MAX_; expect(refused(c.run(), "semantic ids"), "semantic offset + vocabulary overflow"); }
    { Call c = ok; c.infer = 256; expect(refused(c.run(), "infer_token"), "INFER outside the vocabulary"); }
    { Call c = ok; c.infer = -1; expect(refused(c.run(), "infer_token"), "a negative INFER"); }
    { Call c = ok; c.ac_off = -1; expect(refused(c.run(), "code books"), "a negative acoustic offset"); }
    { Call c = ok; c.cb = 0; expect(refused(c.run(), "code books"), "an empty code book"); }
    { Call c = ok; c.ac_off = 129; expect(refused(c.run(), "code books"), "code book 1 past the vocabulary"); }
    { Call c = ok; c.cb = INT_MAX_; expect(refused(c.run(), "code books"), "codebook_size = INT_MAX"); }
    { Call c = ok; c.stop = 256; expect(refused(c.run(), "stop_token"), "a stop token outside the vocabulary"); }
    { Call c = ok; c.stop = -1; expect(refused(c.run(), "state too small"), "no stop token is accepted"); }
    // the sampling arguments
    for (int m : {0, 1025, INT_MAX_, -1}) { Call c = ok; c.max_new = m; expect(refused(c.run(), "max_new"), "max_new out of range"); }
    for (float t : {0.0f, -1.0f, std::nanf(""), std::numeric_limits<float>::infinity()}) {
        Call c = ok; c.temperature = t; expect(refused(c.run(), "temperature"), "a bad temperature");
    }
    { Call c = ok; c.top_k = 0; expect(refused(c.run(), "top_k"), "top_k = 0"); }
    { Call c = ok; c.top_k = -5; expect(refused(c.run(), "top_k"), "top_k < 0"); }
    // the strides and the state's length
    { Call c = ok; c.out_stride = 99; expect(refused(c.run(), "out_stride and u_stride"), "out_stride one short of the longest stream"); }
    { Call c = ok; c.u_stride = 99; expect(refused(c.run(), "out_stride and u_stride"), "u_stride one short of the longest stream"); }
    { Call c = ok; c.out_stride = -1; expect(refused(c.run(), "out_stride and u_stride"), "a negative out_stride"); }
    { Call c = ok; c.max_len = 34; c.state_bytes = need; expect(refused(c.run(), "max_len"), "max_len one short of the final window"); }
    { Call c = ok; c.max_len = 129; c.state_bytes = need; expect(refused(c.run(), "max_len"), "max_len past the block"); }
    { Call c = ok; c.max_new = 2; c.max_len = 32; c.state_bytes = need; expect(refused(c.run(), "max_len"), "max_len short of a non-final window (33)"); }
    { Call c = ok; c.max_new = 2; c.max_len = 33; expect(refused(c.run(), "state too small"), "max_len = S + 1 + r S is enough for a short final window"); }
    { Call c = ok; c.lens = {5, 5}; c.stride = 5; c.max_len = 22; c.out_stride = c.u_stride = 16;
      expect(refused(c.run(), "state too small"), "single windows: strides of max_new and max_len of prompt + max_new"); }
    { Call c = ok; c.max_new = 1024; c.max_len = 128; c.out_stride = c.u_stride = 84 + 109;
      expect(refused(c.run(), "state too small"), "a budget cut by the block: 128 - 19 steps"); }
    { Call c = ok; c.max_new = 1024; c.max_len = 128; c.out_stride = 84 + 108; c.u_stride = 84 + 109;
      expect(refused(c.run(), "out_stride and u_stride"), "a budget cut by the block, out_stride one short"); }
    { Call c = ok; c.B = 64; c.lens.assign(64, 30); c.lens[63] = 1; expect(refused(c.run(), "state too small"), "64 rows"); }
    return verdict("gpt long-form argument checks");
}
