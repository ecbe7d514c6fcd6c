// The fine stage's window queue on the host (audiotoken_amd/csrc/fine.hip: at_fine_generate_queue, at_fine_queue_state_bytes; csrc/fine.h:
// FineQueueSchedule) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program, the way tools/gpt_queue_args.hip checks the GPT's
// queue. Two modes:
//   fine_queue_args                        every refusal path on a finalized at_fine built by hand (fine.h), with no device behind it
//   fine_queue_args dry W slots T [T ...]  the scheduler alone for rows of T frames at block W: prints "pass <slot>:<row>:<k> ..." per pass, then
//                                          "row <slot> <first pass> <last pass>" per row, then "passes <n>"
// Built and run by `make -C audiotoken_amd/csrc fine_queue_asan` (FINE_QUEUE_ARGS="dry ..." for the second mode). The three launchers fine.hip's forward
// calls are stand-ins that count their calls: the program ends by showing that none was reached. The host arrays live in heap blocks of exactly the size
// the call may touch, so an access past them is a sanitizer report.
#define ARGS_STAND_IN_GEMM
#include "decoder_args_common.h"

// W = 128: rows of 300 frames (4 windows), 1 frame and 129 frames (2 windows) through 2 slots
struct Call {
    at_fine* h;
    const int32_t* coarse = fake_i;
    std::vector<int32_t> lens{300, 1, 129};
    int n_rows = 3;
    float temperature = 0.5f;
    int greedy = 0;
    const float* uniforms = fake_f;
    int32_t* out = fake_i;
    void* state = fake_f;
    size_t state_bytes = 0;
    int max_T = 300, slots = 2;
    bool with_trace = false, with_placement = true;
    int trace_cap = 0;

    int run() const {
        const auto l = exact_copy(lens);
        std::unique_ptr<int32_t[]> trace(new int32_t[trace_cap > 0 ? 3 * (size_t)trace_cap : 1]);
        std::unique_ptr<int32_t[]> place(new int32_t[n_rows > 0 && n_rows <= at::FINE_MAX_QUEUE ? 3 * (size_t)n_rows : 1]);
        int32_t passes = -7;
        at::g_error.clear();
        const int rc = at_fine_generate_queue(h, coarse, l.get(), n_rows, temperature, greedy, uniforms, out, nullptr, nullptr, state,
                                              state_bytes, max_T, slots, with_trace ? trace.get() : nullptr, trace_cap, &passes,
                                              with_placement ? place.get() : nullptr, nullptr, nullptr);
        if (rc != 0 && passes != -7) {
            std::printf("FAILED: a refused call wrote its pass count\n");
            ++failures;
        }
        return rc;
    }
};

static int refusals() {
    at_fine model;
    finalize_by_hand(&model);
    at_fine raw;   // never finalized

    // ---- at_fine_queue_state_bytes: the layout of at_fine_state_bytes for (slots, max_T), nothing per row
    at::g_error.clear();
    expect(at_fine_queue_state_bytes(&model, 2, 300) > 0, "state bytes of a well-formed queue");
    expect(at_fine_queue_state_bytes(&model, 2, 300) == at_fine_state_bytes(&model, 2, 300), "the queue's state is the layout of (slots, max_T)");
    expect(at_fine_queue_state_bytes(&model, 64, 300) > at_fine_queue_state_bytes(&model, 1, 300), "state bytes grow with slots");
    expect(at_fine_queue_state_bytes(&model, 2, 1000) > at_fine_queue_state_bytes(&model, 2, 300), "state bytes grow with max_T");
    expect(at_fine_queue_state_bytes(&model, 1, 1) == at_fine_queue_state_bytes(&model, 1, 128), "a row shorter than the window works in a whole window");
    expect(at_fine_queue_state_bytes(nullptr, 1, 64) == 0 && at::g_error.find("not finalized") != std::string::npos, "state bytes of a null handle");
    expect(at_fine_queue_state_bytes(&raw, 1, 64) == 0, "state bytes before finalize");
    for (int s : {0, 65, -1, INT_MIN_, INT_MAX_}) expect(at_fine_queue_state_bytes(&model, s, 64) == 0 && at::g_error.find("slots") != std::string::npos, "state bytes, slots out of range");
    for (int t : {0, (1 << 18) + 1, -1, INT_MIN_, INT_MAX_}) expect(at_fine_queue_state_bytes(&model, 1, t) == 0 && at::g_error.find("max_T") != std::string::npos, "state bytes, max_T out of range");
    expect(at_fine_queue_state_bytes(&model, 64, 1 << 18) > 0, "state bytes of the largest queue");

    // ---- at_fine_generate_queue: a well-formed call with a state that is too small is refused last, which shows the rest was accepted
    Call ok{&model};
    ok.state_bytes = 16;
    expect(refused(ok.run(), "state too small"), "a state that is too small");
    const size_t need = at_fine_queue_state_bytes(&model, 2, 300);
    { Call c = ok; c.state_bytes = need - 1; expect(refused(c.run(), "state too small"), "a state one byte short"); }
    { Call c = ok; c.h = nullptr; expect(refused(c.run(), "not finalized"), "a null handle"); }
    { Call c = ok; c.h = &raw; expect(refused(c.run(), "not finalized"), "a handle before finalize"); }
    for (int n : {0, 4097, -1, INT_MIN_, INT_MAX_}) { Call c = ok; c.n_rows = n; expect(refused(c.run(), "n_rows must be"), "n_rows out of range"); }
    for (int n : {0, 65, -1, INT_MIN_, INT_MAX_}) { Call c = ok; c.slots = n; expect(refused(c.run(), "slots must be"), "slots out of range"); }
    { Call c = ok; c.coarse = nullptr; expect(refused(c.run(), "null pointer"), "null coarse codes"); }
    { Call c = ok; c.lens.clear(); expect(refused(c.run(), "null pointer"), "null lens"); }
    { Call c = ok; c.out = nullptr; expect(refused(c.run(), "null pointer"), "null out"); }
    { Call c = ok; c.uniforms = nullptr; expect(refused(c.run(), "null pointer"), "sampling without uniforms"); }
    { Call c = ok; c.uniforms = nullptr; c.greedy = 1; expect(refused(c.run(), "state too small"), "the argmax needs no uniforms"); }
    { Call c = ok; c.greedy = 1; c.temperature = std::nanf(""); expect(refused(c.run(), "state too small"), "the argmax reads no temperature"); }
    { Call c = ok; c.greedy = 2; expect(refused(c.run(), "greedy"), "greedy = 2"); }
    { Call c = ok; c.state = nullptr; c.state_bytes = need; expect(refused(c.run(), "null state"), "a null state"); }
    for (float t : {0.0f, -1.0f, std::nanf(""), std::numeric_limits<float>::infinity()}) {
        Call c = ok; c.temperature = t; expect(refused(c.run(), "temperature"), "a bad temperature");
    }
    { Call c = ok; c.max_T = 299; expect(refused(c.run(), "row 0 must be"), "a row longer than max_T"); }
    for (int t : {0, (1 << 18) + 1, INT_MAX_, INT_MIN_}) { Call c = ok; c.max_T = t; expect(refused(c.run(), "max_T"), "max_T out of range"); }
    { Call c = ok; c.lens = {300, 0, 129}; expect(refused(c.run(), "row 1 must be"), "an empty row"); }
    { Call c = ok; c.lens = {300, 1, INT_MIN_}; expect(refused(c.run(), "row 2"), "a length of INT_MIN"); }
    { Call c = ok; c.lens = {INT_MAX_, 1, 129}; expect(refused(c.run(), "row 0"), "a length of INT_MAX"); }
    { Call c = ok; c.trace_cap = 4; expect(refused(c.run(), "trace_cap"), "a trace capacity without a trace"); }
    { Call c = ok; c.with_trace = true; c.trace_cap = -1; expect(refused(c.run(), "trace_cap"), "a negative trace capacity"); }
    { Call c = ok; c.with_trace = true; c.trace_cap = 1; expect(refused(c.run(), "state too small"), "a trace of one row is accepted"); }
    { Call c = ok; c.with_placement = false; expect(refused(c.run(), "state too small"), "no placement is accepted"); }
    { Call c = ok; c.slots = 64; c.state_bytes = at_fine_queue_state_bytes(&model, 64, 300) - 1; expect(refused(c.run(), "state too small"), "more slots than rows"); }
    { Call c = ok; c.n_rows = 4096; c.lens.assign(4096, 300); c.lens[4095] = 1; expect(refused(c.run(), "state too small"), "4096 rows"); }
    { Call c = ok; c.max_T = 1 << 18; c.lens = {1 << 18, 1 << 18, 1}; expect(refused(c.run(), "state too small"), "rows of the largest length"); }
    expect(at::g_launches == 0, "no case reached a launch");
    return verdict("fine queue argument checks");
}

static int dry_run(int argc, char** argv) {
    if (argc < 5) {
        std::printf("usage: fine_queue_args dry W slots T [T ...]\n");
        return 2;
    }
    const int W = std::atoi(argv[2]), slots = std::atoi(argv[3]);
    std::vector<int32_t> lens;
    for (int i = 4; i < argc; ++i) lens.push_back(std::atoi(argv[i]));
    bool ok = W >= 128 && W % 128 == 0 && W <= at::FINE_MAX_BLOCK && slots >= 1 && slots <= at::FINE_MAX_B && (int)lens.size() <= at::FINE_MAX_QUEUE;
    for (int32_t T : lens) ok = ok && T >= 1 && T <= at::FINE_MAX_T;
    if (!ok) {
        std::printf("refused: the block, the slots or a row's length\n");
        return 2;
    }
    at::FineQueueSchedule schedule(lens.data(), (int)lens.size(), W, slots);
    at::FineQueuePass p;
    while (schedule.next(&p)) {
        std::printf("pass");
        for (int i = 0; i < p.n; ++i) std::printf(" %d:%d:%d", p.slot[i], p.row[i], p.k[i]);
        std::printf(" | %d %d\n", p.n_admit, p.n_retire);
    }
    const std::vector<int32_t>& place = schedule.placement();
    for (size_t b = 0; b < lens.size(); ++b) std::printf("row %d %d %d\n", place[3 * b], place[3 * b + 1], place[3 * b + 2]);
    std::printf("passes %d\n", schedule.passes());
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::strcmp(argv[1], "dry") == 0) return dry_run(argc, argv);
    return refusals();
}
