// The generation queue's host side (audiotoken_amd/csrc/gpt.hip: at_gpt_generate_queue, at_gpt_queue_state_bytes; csrc/gpt.h: GptQueueSchedule) under
// AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program, the way tools/gpt_long_args.hip checks the long form. Three modes:
//   gpt_queue_args                                    every refusal path on a finalized at_gpt built by hand (decoder_args_common.h)
//   gpt_queue_args dry S H r block max_new slots tick_tokens N:e [N:e ...]
//                                                     the scheduler alone: sources of N ids whose final window ends after e sampler launches; prints
//                                                     "tick <steps> <starts> <prefill> <route>" per tick, then "source <slot> <first> <last>" per source
//   gpt_queue_args extent S H r block max_new N [N ...]
//                                                     the shared geometry alone (gpt.h: gpt_extent, gpt_window): prints "extent <need_len> <need_stride>", then
//                                                     "window <source> <k> <n_ids> <P> <budget> <final> <stream_base>" per window
// Built and run by `make -C audiotoken_amd/csrc gpt_queue_asan` (QUEUE_ARGS="dry ..." or "extent ..." for the other modes).
#include <cstdlib>

#include "decoder_args_common.h"

// The model and the token space of tools/gpt_long_args.hip: 128 positions, 256 ids, S = 8, H = 4, r = 3; sources of 30 ids (7 windows, the stream reaches
// 84 + 16 = 100 positions, the final window 6 + 1 + 12 + 16 = 35 tokens) and 5 ids, through 2 slots.
struct Call {
    at_gpt* h;
    const int32_t* src = fake_i;
    int stride = 30;
    std::vector<int32_t> lens{30, 5, 30};
    int n_src = 3, S = 8, H = 4, r = 3;
    int sem_off = 0, sem_vocab = 64, infer = 200, ac_off = 64, cb = 64, stop = 201;
    int max_new = 16;
    float temperature = 0.8f;
    int top_k = 100;
    const float* uniforms = fake_f;
    int u_stride = 100;
    int32_t *out_ids = fake_i, *out_len = fake_i, *finish = fake_i;
    int out_stride = 100;
    void* state = fake_f;
    size_t state_bytes = 0;
    int max_len = 35, slots = 2, tick_tokens = 37;
    int32_t* trace = nullptr;
    int trace_cap = 0;

    int run() const {
        const auto l = exact_copy(lens);
        at::g_error.clear();
        return at_gpt_generate_queue(h, src, stride, l.get(), n_src, S, H, r, sem_off, sem_vocab, infer, ac_off, cb, stop, max_new,
                                     temperature, top_k, uniforms, u_stride, out_ids, out_stride, out_len, finish, nullptr, state, state_bytes, max_len, slots,
                                     tick_tokens, trace, trace_cap, nullptr, nullptr, nullptr, nullptr);
    }
};

static int refusals() {
    at_gpt model;
    finalize_by_hand(&model, 256);
    at_gpt raw;   // never finalized

    // ---- at_gpt_queue_state_bytes
    at::g_error.clear();
    expect(at_gpt_queue_state_bytes(&model, 2, 35, 37) > 0, "state bytes of a well-formed queue");
    expect(at_gpt_queue_state_bytes(&model, 2, 35, 4 * 35) > at_gpt_queue_state_bytes(&model, 2, 35, 37), "state bytes grow with tick_tokens");
    expect(at_gpt_queue_state_bytes(&model, 64, 128, 192) > at_gpt_queue_state_bytes(&model, 1, 128, 192), "state bytes grow with slots");
    expect(at_gpt_queue_state_bytes(nullptr, 1, 64, 65) == 0 && at::g_error.find("not finalized") != std::string::npos, "state bytes of a null handle");
    expect(at_gpt_queue_state_bytes(&raw, 1, 64, 65) == 0, "state bytes before finalize");
    expect(at_gpt_queue_state_bytes(&model, 0, 64, 65) == 0 && at_gpt_queue_state_bytes(&model, 65, 64, 200) == 0 &&
               at_gpt_queue_state_bytes(&model, INT_MIN_, 64, 65) == 0, "state bytes, slots out of range");
    expect(at_gpt_queue_state_bytes(&model, 1, 0, 65) == 0 && at_gpt_queue_state_bytes(&model, 1, 129, 200) == 0 &&
               at_gpt_queue_state_bytes(&model, 1, INT_MAX_, INT_MAX_) == 0, "state bytes, max_len out of range");
    expect(at_gpt_queue_state_bytes(&model, 2, 35, 36) == 0 && at::g_error.find("tick_tokens") != std::string::npos, "state bytes, tick_tokens one short");
    expect(at_gpt_queue_state_bytes(&model, 2, 35, 65601) == 0 && at_gpt_queue_state_bytes(&model, 2, 35, INT_MAX_) == 0 &&
               at_gpt_queue_state_bytes(&model, 2, 35, -1) == 0, "state bytes, tick_tokens out of range");
    expect(at_gpt_long_state_bytes(&model, 2, 35) > 0 && at_gpt_state_bytes(&model, 2, 35) > 0, "the older state sizes are still answered");

    // ---- at_gpt_generate_queue: a well-formed call with a state that is too small is refused last, which shows the rest was accepted
    Call ok{&model};
    ok.state_bytes = 16;
    expect(refused(ok.run(), "state too small"), "a state that is too small");
    const size_t need = at_gpt_queue_state_bytes(&model, 2, 35, 37);
    { Call c = ok; c.state_bytes = need - 1; expect(refused(c.run(), "state too small"), "a state one byte short"); }
    { Call c = ok; c.h = nullptr; expect(refused(c.run(), "not finalized"), "a null handle"); }
    { Call c = ok; c.h = &raw; expect(refused(c.run(), "not finalized"), "a handle before finalize"); }
    for (int n : {0, 4097, -1, INT_MIN_}) { Call c = ok; c.n_src = n; expect(refused(c.run(), "n_src must be"), "n_src out of range"); }
    for (int n : {0, 65, -1, INT_MIN_, INT_MAX_}) { Call c = ok; c.slots = n; expect(refused(c.run(), "slots must be"), "slots out of range"); }
    { Call c = ok; c.src = nullptr; expect(refused(c.run(), "null pointer"), "null src"); }
    { Call c = ok; c.lens.clear(); expect(refused(c.run(), "null pointer"), "null src_len"); }
    { Call c = ok; c.uniforms = nullptr; expect(refused(c.run(), "null pointer"), "null uniforms"); }
    { Call c = ok; c.out_ids = nullptr; expect(refused(c.run(), "null pointer"), "null out_ids"); }
    { Call c = ok; c.out_len = nullptr; expect(refused(c.run(), "null pointer"), "null out_len"); }
    { Call c = ok; c.finish = nullptr; expect(refused(c.run(), "null pointer"), "null finish"); }
    { Call c = ok; c.state = nullptr; c.state_bytes = need; expect(refused(c.run(), "null state"), "a null state"); }
    { Call c = ok; c.trace_cap = 4; expect(refused(c.run(), "trace_cap"), "a trace capacity without a trace"); }
    { Call c = ok; c.trace = fake_i; c.trace_cap = -1; expect(refused(c.run(), "trace_cap"), "a negative trace capacity"); }
    { Call c = ok; c.trace = fake_i; c.trace_cap = 1; expect(refused(c.run(), "state too small"), "a trace of one row is accepted"); }
    // the schedule
    { Call c = ok; c.S = 7; expect(refused(c.run(), "must be even"), "an odd window"); }
    { Call c = ok; c.H = 3; expect(refused(c.run(), "must be even"), "an odd hop"); }
    { Call c = ok; c.H = 0; expect(refused(c.run(), "must be even"), "hop 0"); }
    { Call c = ok; c.S = -8; expect(refused(c.run(), "must be even"), "a negative window"); }
    { Call c = ok; c.H = 10; expect(refused(c.run(), "must not exceed the window"), "a hop past the window"); }
    { Call c = ok; c.S = 32; c.H = 16; expect(refused(c.run(), "does not fit"), "S + 1 + r S one past the block (129)"); }
    { Call c = ok; c.S = INT_MAX_ - 1; c.H = 2; expect(refused(c.run(), "does not fit"), "S = INT_MAX - 1"); }
    { Call c = ok; c.r = 0; expect(refused(c.run(), "r (acoustic ids"), "r = 0"); }
    { Call c = ok; c.r = INT_MAX_; expect(refused(c.run(), "r (acoustic ids"), "r = INT_MAX"); }
    // the sources
    { Call c = ok; c.stride = 0; expect(refused(c.run(), "src_stride"), "src_stride = 0"); }
    { Call c = ok; c.lens = {30, 0, 30}; expect(refused(c.run(), "source 1 must be 1 to"), "an empty source"); }
    { Call c = ok; c.lens = {31, 5, 30}; expect(refused(c.run(), "source 0 must be 1 to"), "a source longer than its row"); }
    { Call c = ok; c.lens = {30, 5, INT_MIN_}; expect(refused(c.run(), "source 2"), "src_len = INT_MIN"); }
    { Call c = ok; c.stride = INT_MAX_; c.lens = {65537, 5, 30}; expect(refused(c.run(), "source 0"), "a source past 65536 ids"); }
    // the token space
    { Call c = ok; c.sem_off = -1; expect(refused(c.run(), "semantic ids"), "a negative semantic offset"); }
    { Call c = ok; c.sem_off = INT_MAX_; c.sem_vocab = INT_MAX_; expect(refused(c.run(), "semantic ids"), "semantic offset + vocabulary overflow"); }
    { Call c = ok; c.infer = 256; expect(refused(c.run(), "infer_token"), "INFER outside the vocabulary"); }
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
    // the strides, the state's length and the tick
    { Call c = ok; c.out_stride = 99; expect(refused(c.run(), "out_stride and u_stride"), "out_stride one short of the longest stream"); }
    { Call c = ok; c.u_stride = 99; expect(refused(c.run(), "out_stride and u_stride"), "u_stride one short of the longest stream"); }
    { Call c = ok; c.out_stride = -1; expect(refused(c.run(), "out_stride and u_stride"), "a negative out_stride"); }
    { Call c = ok; c.max_len = 34; c.tick_tokens = 36; expect(refused(c.run(), "max_len"), "max_len one short of the final window"); }
    { Call c = ok; c.max_len = 129; c.tick_tokens = 200; expect(refused(c.run(), "max_len"), "max_len past the block"); }
    { Call c = ok; c.tick_tokens = 36; c.state_bytes = need; expect(refused(c.run(), "tick_tokens"), "tick_tokens one short of slots + max_len"); }
    { Call c = ok; c.tick_tokens = 65601; c.state_bytes = need; expect(refused(c.run(), "tick_tokens"), "tick_tokens past its limit"); }
    { Call c = ok; c.tick_tokens = INT_MIN_; c.state_bytes = need; expect(refused(c.run(), "tick_tokens"), "tick_tokens = INT_MIN"); }
    { Call c = ok; c.slots = 64; c.tick_tokens = 64 + 35; expect(refused(c.run(), "state too small"), "more slots than sources"); }
    { Call c = ok; c.n_src = 4096; c.lens.assign(4096, 30); c.lens[4095] = 1; expect(refused(c.run(), "state too small"), "4096 sources"); }
    return verdict("gpt queue argument checks");
}

// what at_gpt_generate_queue requires of the geometry before it builds a schedule
static bool geometry_ok(int S, int H, int r, int block, int max_new) {
    return S >= 2 && S % 2 == 0 && H >= 2 && H % 2 == 0 && H <= S && r >= 1 && block <= at::GPT_MAX_BLOCK && (int64_t)S + 1 + (int64_t)r * S <= block && max_new >= 1;
}

static int dry_run(int argc, char** argv) {
    if (argc < 10) {
        std::printf("usage: gpt_queue_args dry S H r block max_new slots tick_tokens N:e [N:e ...]\n");
        return 2;
    }
    const int S = std::atoi(argv[2]), H = std::atoi(argv[3]), r = std::atoi(argv[4]), block = std::atoi(argv[5]), max_new = std::atoi(argv[6]);
    const int slots = std::atoi(argv[7]), tick_tokens = std::atoi(argv[8]);
    std::vector<int32_t> lens, ends;
    for (int i = 9; i < argc; ++i) {
        int N = 0, e = 0;
        if (std::sscanf(argv[i], "%d:%d", &N, &e) != 2 || N < 1 || N > at::GPT_MAX_SOURCE || e < 1) {
            std::printf("bad source %s\n", argv[i]);
            return 2;
        }
        lens.push_back(N);
        ends.push_back(e);
    }
    int longest = 0;
    const bool geometry = geometry_ok(S, H, r, block, max_new) && slots >= 1 && slots <= at::GPT_MAX_B && (int)lens.size() <= at::GPT_MAX_QUEUE;
    if (geometry)
        for (int32_t N : lens)
            for (int k = 0; k < at::gpt_long_windows(N, S, H); ++k) {
                const int P = at::gpt_window(N, k, S, H, r, max_new, block).P;
                longest = P > longest ? P : longest;
            }
    if (!geometry || tick_tokens < slots + longest) {
        std::printf("refused: the geometry, or tick_tokens below slots + the longest prompt\n");
        return 2;
    }
    at::GptQueueSchedule schedule(lens.data(), (int)lens.size(), S, H, r, max_new, block, slots, tick_tokens);
    at::GptQueueTick t;
    while (schedule.next(&t)) {
        std::printf("tick %d %d %d %d\n", t.n_step, t.n_start, t.prefill_tokens, t.route());
        if (t.poll) schedule.seen_by_steps(ends.data());
    }
    const std::vector<int32_t>& p = schedule.placement();
    for (size_t i = 0; i < lens.size(); ++i) std::printf("source %d %d %d\n", p[3 * i], p[3 * i + 1], p[3 * i + 2]);
    std::printf("ticks %d\n", schedule.ticks());
    return 0;
}

static int extent_run(int argc, char** argv) {
    if (argc < 8) {
        std::printf("usage: gpt_queue_args extent S H r block max_new N [N ...]\n");
        return 2;
    }
    const int S = std::atoi(argv[2]), H = std::atoi(argv[3]), r = std::atoi(argv[4]), block = std::atoi(argv[5]), max_new = std::atoi(argv[6]);
    std::vector<int32_t> lens;
    for (int i = 7; i < argc; ++i) lens.push_back(std::atoi(argv[i]));
    bool ok = geometry_ok(S, H, r, block, max_new);
    for (int32_t N : lens) ok = ok && N >= 1 && N <= at::GPT_MAX_SOURCE;
    if (!ok) {
        std::printf("refused: the geometry or a source's length\n");
        return 2;
    }
    const at::GptExtent e = at::gpt_extent(lens.data(), (int)lens.size(), S, H, r, max_new, block);
    std::printf("extent %d %lld\n", e.need_len, (long long)e.need_stride);
    for (size_t i = 0; i < lens.size(); ++i)
        for (int k = 0; k < at::gpt_long_windows(lens[i], S, H); ++k) {
            const at::GptWindow w = at::gpt_window(lens[i], k, S, H, r, max_new, block);
            std::printf("window %zu %d %d %d %d %d %d\n", i, k, w.n_ids, w.P, w.budget, w.final_window ? 1 : 0, w.stream_base);
        }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::strcmp(argv[1], "dry") == 0) return dry_run(argc, argv);
    if (argc >= 2 && std::strcmp(argv[1], "extent") == 0) return extent_run(argc, argv);
    return refusals();
}
