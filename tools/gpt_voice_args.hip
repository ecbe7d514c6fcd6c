// The argument and schedule checks of the GPT's voice prompts (audiotoken_amd/csrc/gpt.hip: at_gpt_generate_long_prompted, at_gpt_generate_queue_prompted,
// at_gpt_long_num_windows_prompted; csrc/gpt.h: gpt_window / gpt_extent with a prompt length) under AddressSanitizer +
// UndefinedBehaviorSanitizer, as a stand-alone program, the way tools/gpt_long_args.hip checks the prompt-free calls. Modes:
//   gpt_voice_args                                          every refusal path and the accepted edges P = 2 and P = S - H
//   gpt_voice_args extent S H r block max_new P:N [P:N ...] the prompted geometry alone: prints "extent <need_len> <need_stride>", then
//                                                           "window <source> <k> <n_ids> <prompt tokens> <budget> <final> <result base>" per window
// Built and run by `make -C audiotoken_amd/csrc gpt_voice_asan` (VOICE_ARGS="extent ..." for the other mode).
#include <cstdlib>

#include "decoder_args_common.h"

// The model and the token space of tools/gpt_long_args.hip: 128 positions, 256 ids, S = 8, H = 4, r = 3. Row 0 has 30 ids after a prompt of 4 (8 windows
// of the 34 concatenated ids: the last reads 6, carries 12 and starts at result position 84), row 1 has 5 ids and no prompt.
struct Call {
    at_gpt* h;
    const int32_t* src = fake_i;
    int stride = 30;
    std::vector<int32_t> lens{30, 5};
    int B = 2;
    const int32_t *p_sem = fake_i, *p_codes = fake_i;
    int p_stride = 4, f_stride = 6;
    std::vector<int32_t> p_len{4, 2}, p_of{0, -1};
    int n_prompts = 2;
    bool null_of = false;
    int S = 8, H = 4, r = 3;
    int sem_off = 0, sem_vocab = 64, infer = 200, ac_off = 64, cb = 64, stop = 201;
    int max_new = 16;
    float temperature = 0.8f;
    int top_k = 100;
    const float* uniforms = fake_f;
    int u_stride = 100;
    int32_t *out_ids = fake_i, *out_len = fake_i, *finish = fake_i;
    int out_stride = 100;
    void* state = fake_f;
    size_t state_bytes = 16;   // too small: a well-formed call is refused last, for this
    int max_len = 35, slots = 2, tick_tokens = 37;
    bool queue = false;

    int run() const {
        const auto l = exact_copy(lens), pl = exact_copy(p_len), po = exact_copy(p_of);
        at::g_error.clear();
        if (queue)
            return at_gpt_generate_queue_prompted(h, src, stride, l.get(), B, p_sem, p_stride, p_codes, f_stride, pl.get(), n_prompts, null_of ? nullptr : po.get(), S,
                                                  H, r, sem_off, sem_vocab, infer, ac_off, cb, stop, max_new, temperature, top_k, uniforms, u_stride, out_ids,
                                                  out_stride, out_len, finish, nullptr, state, state_bytes, max_len, slots, tick_tokens, nullptr, 0, nullptr, nullptr,
                                                  nullptr, nullptr);
        return at_gpt_generate_long_prompted(h, src, stride, l.get(), B, p_sem, p_stride, p_codes, f_stride, pl.get(), n_prompts, null_of ? nullptr : po.get(), S, H, r,
                                             sem_off, sem_vocab, infer, ac_off, cb, stop, max_new, temperature, top_k, uniforms, u_stride, out_ids, out_stride, out_len,
                                             finish, nullptr, state, state_bytes, max_len, nullptr, nullptr);
    }
};

static int refusals() {
    at_gpt model;
    finalize_by_hand(&model, 256);

    // ---- the window count after a prompt: the count of the concatenated source
    expect(at_gpt_long_num_windows_prompted(2, 5, 8, 4) == 1 && at_gpt_long_num_windows_prompted(2, 6, 8, 4) == 1 && at_gpt_long_num_windows_prompted(2, 7, 8, 4) == 2,
           "windows around P + N = S");
    expect(at_gpt_long_num_windows_prompted(4, 30, 8, 4) == 8 && at_gpt_long_num_windows_prompted(4, 30, 8, 4) == at_gpt_long_num_windows(34, 8, 4), "windows of P + N");
    expect(at_gpt_long_num_windows_prompted(4, 65532, 8, 4) == at_gpt_long_num_windows(65536, 8, 4), "P + N = 65536 is accepted");
    expect(at_gpt_long_num_windows_prompted(4, 65533, 8, 4) == 0 && at_gpt_long_num_windows_prompted(4, 0, 8, 4) == 0, "windows: N out of range");
    expect(at_gpt_long_num_windows_prompted(0, 5, 8, 4) == 0 && at_gpt_long_num_windows_prompted(3, 5, 8, 4) == 0 && at_gpt_long_num_windows_prompted(6, 5, 8, 4) == 0 &&
               at_gpt_long_num_windows_prompted(-2, 5, 8, 4) == 0, "windows: P zero, odd, past S - H, negative");
    expect(at_gpt_long_num_windows_prompted(2, 5, 7, 4) == 0 && at_gpt_long_num_windows_prompted(2, 5, 8, 3) == 0 && at_gpt_long_num_windows_prompted(2, 5, 8, 10) == 0,
           "windows: odd S, odd H, H > S");
    expect(at_gpt_long_num_windows_prompted(INT_MAX_, INT_MAX_, INT_MAX_, 2) == 0 && at_gpt_long_num_windows_prompted(INT_MIN_, INT_MIN_, 8, 4) == 0, "windows: extreme values");
    expect(at_gpt_long_num_windows_prompted(2, 5, 8, 8) == 0, "windows: no prompt fits a schedule without overlap (S - H = 0)");

    for (bool queue : {false, true}) {
        Call ok{&model};
        ok.queue = queue;
        // ---- accepted: refused only for the state, which is checked last
        expect(refused(ok.run(), "state too small"), "a well-formed prompted call");
        { Call c = ok; c.p_len = {4, 2}; c.p_of = {1, 0}; c.max_len = 37; c.tick_tokens = 39; expect(refused(c.run(), "state too small"), "P = 2 and P = S - H, both in use"); }
        { Call c = ok; c.p_of = {-1, -1}; expect(refused(c.run(), "state too small"), "a table no source uses"); }
        { Call c = ok; c.n_prompts = 0; c.p_len.clear(); c.p_sem = c.p_codes = nullptr; c.p_of = {-1, -1}; expect(refused(c.run(), "state too small"), "an empty table"); }
        { Call c = ok; c.p_of = {0, 0}; expect(refused(c.run(), "state too small"), "one entry shared by both sources"); }
        { Call c = ok; c.lens = {2, 5}; c.stride = 5; c.max_len = 35; expect(refused(c.run(), "state too small"), "P + N below S: one window with the prompt as its carry"); }
        // ---- the extent counts the prompt: the same sources without one need less
        { Call c = ok; c.out_stride = 99; expect(refused(c.run(), "out_stride and u_stride"), "out_stride one short of the prompted row's result"); }
        { Call c = ok; c.u_stride = 99; expect(refused(c.run(), "out_stride and u_stride"), "u_stride one short of the prompted row's result"); }
        { Call c = ok; c.p_of = {-1, -1}; c.out_stride = c.u_stride = 99; expect(refused(c.run(), "out_stride and u_stride"), "unprompted, 30 ids need 100 as well"); }
        { Call c = ok; c.p_of = {1, -1}; c.max_len = 37; c.tick_tokens = 39; c.out_stride = c.u_stride = 94;
          expect(refused(c.run(), "state too small"), "30 ids after 2: 7 windows, the final one of 8 ids starts at result position 72 + 12 - 6"); }
        { Call c = ok; c.p_of = {1, -1}; c.max_len = 37; c.tick_tokens = 39; c.out_stride = c.u_stride = 93;
          expect(refused(c.run(), "out_stride and u_stride"), "30 ids after 2, a stride one short"); }
        { Call c = ok; c.p_of = {1, -1}; c.max_len = 36; c.tick_tokens = 39; expect(refused(c.run(), "max_len"), "30 ids after 2, max_len one short of 8 + 1 + 12 + 16"); }
        { Call c = ok; c.max_len = 34; expect(refused(c.run(), "max_len"), "max_len one short of the final window"); }
        // ---- the table
        { Call c = ok; c.null_of = true; expect(refused(c.run(), "null prompt_of_src"), "null prompt_of_src"); }
        { Call c = ok; c.p_sem = nullptr; expect(refused(c.run(), "null prompt table"), "null prompt ids"); }
        { Call c = ok; c.p_codes = nullptr; expect(refused(c.run(), "null prompt table"), "null prompt codes"); }
        { Call c = ok; c.p_len.clear(); expect(refused(c.run(), "null prompt table"), "null prompt lengths"); }
        for (int n : {-1, 4097, INT_MAX_, INT_MIN_}) { Call c = ok; c.n_prompts = n; expect(refused(c.run(), "n_prompts"), "n_prompts out of range"); }
        { Call c = ok; c.p_stride = 0; expect(refused(c.run(), "p_stride and f_stride"), "p_stride = 0"); }
        { Call c = ok; c.f_stride = -1; expect(refused(c.run(), "p_stride and f_stride"), "a negative f_stride"); }
        for (int P : {0, 1, 3, 6, -2, INT_MAX_, INT_MIN_}) {
            Call c = ok; c.p_len = {P, 2}; c.p_stride = 8; c.f_stride = 12;
            expect(refused(c.run(), "must be even, 2 to S - H"), "a prompt length that is zero, odd, past S - H or negative");
        }
        { Call c = ok; c.p_len = {4, 6}; c.p_stride = 8; c.f_stride = 12; expect(refused(c.run(), "prompt 1 must be even"), "an unused entry is checked too"); }
        { Call c = ok; c.H = 8; expect(refused(c.run(), "must be even, 2 to S - H"), "no prompt fits S = H"); }
        { Call c = ok; c.p_stride = 3; expect(refused(c.run(), "does not fit"), "a prompt longer than p_stride"); }
        { Call c = ok; c.f_stride = 5; expect(refused(c.run(), "does not fit"), "a prompt whose r P / 2 frames exceed f_stride"); }
        for (int e : {2, -2, INT_MAX_, INT_MIN_}) { Call c = ok; c.p_of = {e, -1}; expect(refused(c.run(), "source 0 must be -1 or an entry"), "prompt_of_src out of range"); }
        { Call c = ok; c.stride = INT_MAX_; c.lens = {65533, 5}; expect(refused(c.run(), "exceeds 65536"), "P + N one past 65536"); }
        // ---- what the prompt-free call refuses stays refused
        { Call c = ok; c.lens = {30, 0}; expect(refused(c.run(), "1 must be 1 to"), "an empty source"); }
        { Call c = ok; c.S = 7; expect(refused(c.run(), "must be even"), "an odd window"); }
        { Call c = ok; c.cb = 0; expect(refused(c.run(), "code books"), "an empty code book"); }
        { Call c = ok; c.h = nullptr; expect(refused(c.run(), "not finalized"), "a null handle"); }
    }
    // the queue's schedule takes the prompted windows: 2 sources of 30 ids, one prompted, through one slot
    {
        const int32_t lens[2] = {30, 30}, pv[2] = {4, 0};
        at::GptQueueSchedule a(lens, 2, 8, 4, 3, 16, 128, 1, 34, pv), b(lens, 2, 8, 4, 3, 16, 128, 1, 34);
        at::GptQueueTick t;
        expect(a.next(&t) && t.n_start == 1 && t.start[0].P == 8 + 1 + 12 && t.start[0].n_ids == 8, "the queue's first window carries the prompt's 12 ids");
        expect(b.next(&t) && t.n_start == 1 && t.start[0].P == 8 + 1, "and none without a prompt");
    }
    return verdict("gpt voice prompt argument checks");
}

static int extent_run(int argc, char** argv) {
    if (argc < 8) {
        std::printf("usage: gpt_voice_args extent S H r block max_new P:N [P:N ...]\n");
        return 2;
    }
    const int S = std::atoi(argv[2]), H = std::atoi(argv[3]), r = std::atoi(argv[4]), block = std::atoi(argv[5]), max_new = std::atoi(argv[6]);
    std::vector<int32_t> lens, pv;
    for (int i = 7; i < argc; ++i) {
        const char* colon = std::strchr(argv[i], ':');
        pv.push_back(std::atoi(argv[i]));
        lens.push_back(colon ? std::atoi(colon + 1) : 0);
    }
    bool ok = S >= 2 && S % 2 == 0 && H >= 2 && H % 2 == 0 && H <= S && r >= 1 && (long long)S + 1 + (long long)r * S <= block && max_new >= 1 && max_new <= 1024;
    for (size_t i = 0; i < lens.size(); ++i) ok = ok && (pv[i] == 0 ? lens[i] >= 1 && lens[i] <= at::GPT_MAX_SOURCE : at::gpt_voice_prompt_ok(pv[i], lens[i], S, H));
    if (!ok) {
        std::printf("refused: the geometry, a prompt's or a source's length\n");
        return 2;
    }
    const at::GptExtent e = at::gpt_extent(lens.data(), (int)lens.size(), S, H, r, max_new, block, pv.data());
    std::printf("extent %d %lld\n", e.need_len, (long long)e.need_stride);
    for (size_t i = 0; i < lens.size(); ++i)
        for (int k = 0; k < at::gpt_long_windows(lens[i], S, H, pv[i]); ++k) {
            const at::GptWindow w = at::gpt_window(lens[i], k, S, H, r, max_new, block, pv[i]);
            std::printf("window %zu %d %d %d %d %d %d\n", i, k, w.n_ids, w.P, w.budget, w.final_window ? 1 : 0, w.stream_base);
        }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::strcmp(argv[1], "extent") == 0) return extent_run(argc, argv);
    return refusals();
}
