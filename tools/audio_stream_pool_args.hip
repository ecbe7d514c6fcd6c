// The host side of the semantic-to-audio stream pools (audiotoken_amd/csrc/gpt.hip: at_gpt_pool_push, at_gpt_pool_state_bytes; fine.hip:
// at_fine_pool_push, at_fine_pool_state_bytes; gpt.h / fine.h: GptPoolSchedule, FinePoolSchedule) under AddressSanitizer + UndefinedBehaviorSanitizer, as a
// stand-alone program in the style of tools/semantic_stream_args.hip: both handles are finalized by hand with no device behind them, and every case is refused before anything is launched. Built and run by
// `make -C audiotoken_amd/csrc audio_stream_pool_asan`.
//   no arguments                                                             every refusal path
//   gpt S H r block max_new slots tick_tokens n_before:n_new:final:end ...   one call of GptPoolSchedule for these streams (end: the sampler launches the
//                                                                            final window takes): a line per stream and round, per tick and per stream
//   fine W fine_slots T_before:n_new:final ...                               one call of FinePoolSchedule: a line per stream and round and per pass
// tests/test_semantic_pool_cpu.py compares the printed lines with the Python twins' (semantic_pool.pool_schedule / fine_pool_passes).
#include <cstdlib>

#include "decoder_args_common.h"

// A model of 128 positions and 256 ids as in semantic_stream_args.hip: semantic ids [0, 64), the two code books [64, 128) and [128, 192), INFER 200, STOP 201;
// S = 8, H = 4, r = 3. A pool of 4 streams on 2 cache rows; the call names the streams in places 2 and 0: the first has 13 ids behind it (windows 0 and 1
// have run) and is pushed 4 more (window 2 runs, stream positions 36 to 47, after a carry of 12), the second is new, is pushed 3 ids and flushed (its only
// window: a budget of 16 from position 0).
struct PoolCall {
    at_gpt* h;
    void* state = fake_f;
    size_t state_bytes = 0;
    int streams = 4, slots = 2, max_len = 41, tick_tokens = 43;   // at least max(S + 1 + r S, min(block, S + 1 + r (S - H) + max_new)) = max(33, 37) positions
    int64_t pos[8] = {0, 0, 7, 0, 13, 0, 3, 1};
    int n = 2;
    int32_t place[2] = {2, 0};
    const int32_t* ids = fake_i;
    int32_t n_new[2] = {4, 3}, final[2] = {0, 1};
    int S = 8, H = 4, r = 3;
    int sem_off = 0, sem_vocab = 64, infer = 200, ac_off = 64, cb = 64, stop = 201, max_new = 16;
    float temperature = 0.8f;
    int top_k = 100;
    const float* uniforms = fake_f;
    int u_stride = 16;
    int64_t u_pos0[2] = {36, 0};
    int32_t *out_ids = fake_i, *out_len = fake_i, *finish = fake_i;
    int out_stride = 24;   // the carry (12) and window 2's ids (12); the flushed stream needs 16
    int32_t* trace = nullptr;
    int trace_cap = 0;

    int run() {
        at::g_error.clear();
        int64_t before[8];
        std::memcpy(before, pos, sizeof(before));
        const int rc = at_gpt_pool_push(h, state, state_bytes, streams, slots, max_len, tick_tokens, pos, n, place, ids, n_new, final, S, H, r, sem_off, sem_vocab,
                                        infer, ac_off, cb, stop, max_new, temperature, top_k, uniforms, u_stride, u_pos0, out_ids, out_stride, out_len, finish, nullptr,
                                        nullptr, trace, trace_cap, nullptr, nullptr, nullptr, nullptr, nullptr);
        expect(rc == 0 || std::memcmp(before, pos, sizeof(before)) == 0, "a refused call leaves every stream's record as it was");
        return rc;
    }
    bool untouched() const {
        const int64_t want[8] = {0, 0, 7, 0, 13, 0, 3, 1};
        return std::memcmp(pos, want, sizeof(want)) == 0;
    }
};

alignas(16) static int32_t fake_ids[4];

// The fine model of fine_args.hip (W = 128). A pool of 3 streams, 2 windows a pass; the call names the streams in places 1 and 0: the first has 100 frames
// behind it and hands over 60 more (window 0 runs, frames [0, 64) turn final), the second is new, hands over 10 frames and is flushed (the padded window).
struct FinePoolCall {
    at_fine* h;
    void* state = fake_f;
    size_t state_bytes = 0;
    int streams = 3, fine_slots = 2;
    int64_t pos[6] = {0, 0, 100, 0, 50, 1};
    int n = 2;
    int32_t place[2] = {1, 0};
    const int32_t* ids = fake_ids;
    int64_t id_off[2] = {0, 200};
    int32_t n_frames[2] = {60, 10}, final[2] = {0, 1};
    int ac_off = 64, cb = 1024;
    float temperature = 0.5f;
    int greedy = 0;
    const float* uniforms = fake_f;
    int32_t u_cell0[2] = {0, 1}, u_win0[2] = {0, 0}, u_windows[2] = {1, 1};
    int64_t* emit = reinterpret_cast<int64_t*>(fake_ids);
    int emit_stride = 64;
    int32_t n_emitted[2] = {-1, -1};
    int32_t* trace = nullptr;
    int trace_cap = 0;

    int run() {
        at::g_error.clear();
        int64_t before[6];
        std::memcpy(before, pos, sizeof(before));
        const int rc = at_fine_pool_push(h, state, state_bytes, streams, fine_slots, pos, n, place, ids, id_off, n_frames, final, ac_off, cb, temperature, greedy, uniforms,
                                         u_cell0, u_win0, u_windows, emit, emit_stride, n_emitted, nullptr, trace, trace_cap, nullptr, nullptr, nullptr);
        expect(rc == 0 || (std::memcmp(before, pos, sizeof(before)) == 0 && n_emitted[0] == -1 && n_emitted[1] == -1), "fine: a refused call leaves every record as it was");
        return rc;
    }
};

static int dry_fine(int argc, char** argv) {
    const int W = std::atoi(argv[2]), fine_slots = std::atoi(argv[3]);
    std::vector<int64_t> before;
    std::vector<int32_t> n_new, final;
    for (int i = 4; i < argc; ++i) {
        long long b = 0;
        int m = 0, f = 0;
        if (std::sscanf(argv[i], "%lld:%d:%d", &b, &m, &f) != 3) { std::printf("refused: %s\n", argv[i]); return 2; }
        before.push_back(b); n_new.push_back(m); final.push_back(f);
    }
    const int n = (int)before.size();
    at::FinePoolSchedule s(before.data(), n_new.data(), final.data(), n, W, fine_slots);
    while (s.next_round()) {
        for (int i = 0; i < n; ++i)
            if (const at::FineStreamRound* r = s.round(i))
                std::printf("round %d %d %d %lld %d %d %d %d %d %d %lld %lld %d\n", s.rounds() - 1, i, r->take, r->first, r->held, r->j_first, r->n_win, r->pad,
                            r->last_window ? 1 : 0, r->last_rel, r->emit_from, r->emit_to, r->shift);
        at::FinePoolPass p;
        while (s.next(&p)) {
            std::printf("pass %d %d", s.rounds() - 1, p.wave);
            for (int w = 0; w < p.n; ++w) std::printf(" %d:%d:%d", p.stream[w], p.j[w], p.rel[w]);
            std::printf("\n");
        }
    }
    return 0;
}

static int dry(int argc, char** argv) {
    const int S = std::atoi(argv[2]), H = std::atoi(argv[3]), r = std::atoi(argv[4]), block = std::atoi(argv[5]), max_new = std::atoi(argv[6]);
    const int slots = std::atoi(argv[7]), tick_tokens = std::atoi(argv[8]);
    std::vector<int64_t> before;
    std::vector<int32_t> n_new, final, ends;
    for (int i = 9; i < argc; ++i) {
        long long b = 0;
        int m = 0, f = 0, e = 0;
        if (std::sscanf(argv[i], "%lld:%d:%d:%d", &b, &m, &f, &e) != 4) { std::printf("refused: %s\n", argv[i]); return 2; }
        before.push_back(b); n_new.push_back(m); final.push_back(f); ends.push_back(e);
    }
    const int n = (int)before.size();
    at::GptPoolSchedule s(before.data(), n_new.data(), final.data(), n, S, H, r, max_new, block, slots, tick_tokens);
    while (s.next_round()) {
        for (int i = 0; i < n; ++i)
            if (const at::GptStreamRound* rd = s.round(i))
                std::printf("round %d %d %d %d %d %d %d %d\n", s.rounds() - 1, i, rd->take, rd->held, rd->k_first, rd->n_win, rd->final_window ? 1 : 0, rd->final_ids);
        at::GptPoolTick t;
        while (s.next(&t)) {
            std::printf("tick %d %d %d %d %d\n", t.n_step, t.n_start, t.prefill_tokens, t.route(), s.rounds() - 1);
            if (t.poll) s.seen_by_steps(ends.data());
        }
    }
    for (int i = 0; i < n; ++i) std::printf("place %d %d %d\n", s.placement()[3 * i], s.placement()[3 * i + 1], s.placement()[3 * i + 2]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 10 && std::string(argv[1]) == "gpt") return dry(argc, argv);
    if (argc >= 5 && std::string(argv[1]) == "fine") return dry_fine(argc, argv);
    at_gpt model;
    finalize_by_hand(&model, 256);
    at_gpt raw;
    at_fine fine;
    finalize_by_hand(&fine);
    at_fine fraw;

    // ---- at_gpt_pool_state_bytes: the queue's state and, per stream, 2 S source ids and r (S - H) + 1 carry ids
    const int max_len = 41;
    const size_t need = at_gpt_pool_state_bytes(&model, 4, 2, max_len, 43, 8, 4, 3);
    const size_t queue = at_gpt_queue_state_bytes(&model, 2, max_len, 43);
    expect(need == queue + 256 + 256, "4 streams: 64 source ids and 52 carry ids, each array rounded to 256 bytes");
    expect(at_gpt_pool_state_bytes(&model, 64, 2, max_len, 43, 8, 4, 3) == queue + 64 * 16 * 4 + (64 * 13 * 4 + 255) / 256 * 256, "64 streams");
    expect(at_gpt_pool_state_bytes(nullptr, 4, 2, max_len, 43, 8, 4, 3) == 0 && at_gpt_pool_state_bytes(&raw, 4, 2, max_len, 43, 8, 4, 3) == 0, "state bytes without a finalized model");
    expect(at_gpt_pool_state_bytes(&model, 0, 2, max_len, 43, 8, 4, 3) == 0 && at_gpt_pool_state_bytes(&model, 1025, 2, max_len, 43, 8, 4, 3) == 0, "state bytes: streams out of range");
    expect(at_gpt_pool_state_bytes(&model, 4, 0, max_len, 43, 8, 4, 3) == 0 && at_gpt_pool_state_bytes(&model, 4, 65, max_len, 43 + 63, 8, 4, 3) == 0, "state bytes: slots out of range");
    expect(at_gpt_pool_state_bytes(&model, 4, 2, 32, 43, 8, 4, 3) == 0 && at_gpt_pool_state_bytes(&model, 4, 2, 129, 131, 8, 4, 3) == 0, "state bytes: max_len below a non-final window, past the block");
    expect(at_gpt_pool_state_bytes(&model, 4, 2, max_len, 42, 8, 4, 3) == 0, "state bytes: tick_tokens below slots + max_len");
    expect(at_gpt_pool_state_bytes(&model, 4, 2, max_len, 43, 7, 4, 3) == 0 && at_gpt_pool_state_bytes(&model, 4, 2, max_len, 43, 8, 10, 3) == 0 &&
               at_gpt_pool_state_bytes(&model, 4, 2, 128, 130, 32, 16, 3) == 0, "state bytes: odd S, H > S, a window past the block");

    // ---- at_gpt_pool_push: a well-formed call with a state that is too small is refused last
    PoolCall ok{&model};
    ok.state_bytes = 16;
    expect(refused(ok.run(), "state too small"), "a state that is too small");
    expect(ok.untouched(), "a refused call leaves every stream's record as it was");
    { PoolCall c = ok; c.state_bytes = need - 1; expect(refused(c.run(), "state too small"), "a state one byte short"); }
    { PoolCall c = ok; c.h = nullptr; expect(refused(c.run(), "not finalized"), "a null handle"); }
    { PoolCall c = ok; c.h = &raw; expect(refused(c.run(), "not finalized"), "a handle before finalize"); }
    { PoolCall c = ok; c.state = nullptr; expect(refused(c.run(), "null state"), "a null state"); }
    { PoolCall c = ok; c.uniforms = nullptr; expect(refused(c.run(), "null pointer"), "null uniforms"); }
    { PoolCall c = ok; c.out_ids = nullptr; expect(refused(c.run(), "null pointer"), "null out_ids"); }
    { PoolCall c = ok; c.out_len = nullptr; expect(refused(c.run(), "null pointer"), "null out_len"); }
    { PoolCall c = ok; c.finish = nullptr; expect(refused(c.run(), "null pointer"), "null finish"); }
    { PoolCall c = ok; c.ids = nullptr; expect(refused(c.run(), "ids need a pointer"), "ids without a pointer"); }
    { PoolCall c = ok; c.trace_cap = 4; expect(refused(c.run(), "trace_cap"), "a trace capacity without a trace"); }
    { PoolCall c = ok; c.streams = 0; expect(refused(c.run(), "streams must be"), "no streams"); }
    { PoolCall c = ok; c.streams = 1025; expect(refused(c.run(), "streams must be"), "too many streams"); }
    { PoolCall c = ok; c.streams = 1; expect(refused(c.run(), "n (the call's streams)"), "more streams in the call than the pool has"); }
    { PoolCall c = ok; c.n = -1; expect(refused(c.run(), "n (the call's streams)"), "a negative n"); }
    { PoolCall c = ok; c.slots = 0; expect(refused(c.run(), "slots must be"), "no slots"); }
    { PoolCall c = ok; c.slots = 65; expect(refused(c.run(), "slots must be"), "65 slots"); }
    { PoolCall c = ok; c.max_len = 36; expect(refused(c.run(), "max_len"), "max_len one short of the final window with max_new"); }
    { PoolCall c = ok; c.max_len = 129; c.tick_tokens = 131; expect(refused(c.run(), "max_len"), "max_len past the block"); }
    { PoolCall c = ok; c.tick_tokens = 42; expect(refused(c.run(), "tick_tokens"), "tick_tokens below slots + max_len"); }
    { PoolCall c = ok; c.place[1] = 2; expect(refused(c.run(), "named once"), "a place named twice"); }
    { PoolCall c = ok; c.place[0] = 4; expect(refused(c.run(), "named once"), "a place past the pool"); }
    { PoolCall c = ok; c.place[0] = -1; expect(refused(c.run(), "named once"), "a negative place"); }
    { PoolCall c = ok; c.place[0] = 3; expect(refused(c.run(), "after the final call"), "a flushed stream"); }
    { PoolCall c = ok; c.n_new[0] = -1; expect(refused(c.run(), "must not be negative"), "a negative n_new"); }
    { PoolCall c = ok; c.final[1] = 2; expect(refused(c.run(), "final must be"), "final = 2"); }
    { PoolCall c = ok; c.n_new[1] = 0; expect(refused(c.run(), "nothing pushed"), "a stream flushed with nothing ever pushed"); }
    { PoolCall c = ok; c.pos[4] = 65533; expect(refused(c.run(), "at most 65536"), "a stream past 65536 ids"); }
    { PoolCall c = ok; c.pos[0] = -1; expect(refused(c.run(), "at most 65536"), "a negative record"); }
    { PoolCall c = ok; c.S = 7; expect(refused(c.run(), "must be even"), "an odd window"); }
    { PoolCall c = ok; c.H = 10; expect(refused(c.run(), "must not exceed the window"), "a hop past the window"); }
    { PoolCall c = ok; c.r = 0; expect(refused(c.run(), "r (acoustic ids"), "r = 0"); }
    { PoolCall c = ok; c.sem_vocab = 0; expect(refused(c.run(), "semantic ids"), "an empty semantic vocabulary"); }
    { PoolCall c = ok; c.infer = 256; expect(refused(c.run(), "infer_token"), "INFER outside the vocabulary"); }
    { PoolCall c = ok; c.ac_off = 129; expect(refused(c.run(), "code books"), "code book 1 past the vocabulary"); }
    { PoolCall c = ok; c.stop = 256; expect(refused(c.run(), "stop_token"), "a stop token outside the vocabulary"); }
    for (int m : {0, 1025, -1}) { PoolCall c = ok; c.max_new = m; expect(refused(c.run(), "max_new"), "max_new out of range"); }
    { PoolCall c = ok; c.temperature = 0.0f; expect(refused(c.run(), "temperature"), "temperature 0"); }
    { PoolCall c = ok; c.top_k = 0; expect(refused(c.run(), "top_k"), "top_k = 0"); }
    // the caller's arrays against the windows each stream of the call will run
    { PoolCall c = ok; c.u_pos0[0] = 37; expect(refused(c.run(), "stream 0 of the call: the uniforms do not cover"), "uniforms of the first stream that begin one position late"); }
    { PoolCall c = ok; c.u_stride = 15; expect(refused(c.run(), "stream 1 of the call: the uniforms do not cover"), "uniforms one short of the flushed stream's budget"); }
    { PoolCall c = ok; c.u_pos0[1] = -1; expect(refused(c.run(), "must not be negative"), "a negative u_pos0"); }
    { PoolCall c = ok; c.u_pos0[1] = (int64_t)1 << 31; expect(refused(c.run(), "must fit 31 bits"), "a u_pos0 past int"); }
    { PoolCall c = ok; c.out_stride = INT_MAX_ / 2 + 1; expect(refused(c.run(), "n * out_stride must fit"), "pieces that an int cannot address"); }
    { PoolCall c = ok; c.out_stride = 23; expect(refused(c.run(), "stream 0 of the call: out_stride"), "out_stride one short of the carry and the new ids"); }
    { PoolCall c = ok; c.n_new[0] = 3; c.u_pos0[0] = 0; expect(refused(c.run(), "state too small"), "a push that runs no window needs no draws"); }
    { PoolCall c = ok; c.n = 0; c.state_bytes = need; expect(c.run() == 0 && c.untouched(), "a call that names no stream does nothing"); }
    expect(ok.untouched(), "no refused call changed a record");

    // ---- the fine pool
    at::g_error.clear();
    const size_t fneed = at_fine_pool_state_bytes(&fine, 3, 2);
    expect(fneed == at_fine_state_bytes(&fine, 2, 128) - 2 * 128 * 8 * 4 + 3 * 256 * 8 * 4, "the fine pool's state: 2 W cells a stream, the activations of fine_slots windows");
    expect(at_fine_pool_state_bytes(&fine, 4, 2) - fneed == 2 * 128 * 8 * 4, "a stream's share of the fine state: 2 W cells of 8 ints");
    expect(at_fine_pool_state_bytes(nullptr, 3, 2) == 0 && at_fine_pool_state_bytes(&fraw, 3, 2) == 0, "fine state bytes without a finalized model");
    expect(at_fine_pool_state_bytes(&fine, 0, 2) == 0 && at_fine_pool_state_bytes(&fine, 1025, 2) == 0 && at_fine_pool_state_bytes(&fine, 3, 0) == 0 &&
               at_fine_pool_state_bytes(&fine, 3, 65) == 0, "fine state bytes: streams and fine_slots out of range");
    FinePoolCall fok{&fine};
    fok.state_bytes = 16;
    expect(refused(fok.run(), "state too small"), "fine: a state that is too small");
    { FinePoolCall c = fok; c.state_bytes = fneed - 1; expect(refused(c.run(), "state too small"), "fine: a state one byte short"); }
    { FinePoolCall c = fok; c.h = nullptr; expect(refused(c.run(), "not finalized"), "fine: a null handle"); }
    { FinePoolCall c = fok; c.h = &fraw; expect(refused(c.run(), "not finalized"), "fine: a handle before finalize"); }
    { FinePoolCall c = fok; c.state = nullptr; expect(refused(c.run(), "null state"), "fine: a null state"); }
    { FinePoolCall c = fok; c.streams = 0; expect(refused(c.run(), "streams must be"), "fine: no streams"); }
    { FinePoolCall c = fok; c.streams = 1; expect(refused(c.run(), "n (the call's streams)"), "fine: more streams in the call than the pool has"); }
    { FinePoolCall c = fok; c.fine_slots = 65; expect(refused(c.run(), "fine_slots must be"), "fine: 65 windows a pass"); }
    { FinePoolCall c = fok; c.ids = nullptr; expect(refused(c.run(), "frames need a pointer"), "fine: frames without a pointer"); }
    { FinePoolCall c = fok; c.ids = fake_ids + 1; expect(refused(c.run(), "8-byte aligned"), "fine: ids that are not 8-byte aligned"); }
    { FinePoolCall c = fok; c.id_off[1] = 201; expect(refused(c.run(), "id_off must be even"), "fine: an odd id_off"); }
    { FinePoolCall c = fok; c.id_off[0] = -2; expect(refused(c.run(), "id_off must be even"), "fine: a negative id_off"); }
    { FinePoolCall c = fok; c.n_frames[0] = -1; expect(refused(c.run(), "must not be negative"), "fine: a negative n_frames"); }
    { FinePoolCall c = fok; c.final[0] = -1; expect(refused(c.run(), "final must be"), "fine: final = -1"); }
    { FinePoolCall c = fok; c.greedy = 2; expect(refused(c.run(), "greedy must be"), "fine: greedy = 2"); }
    { FinePoolCall c = fok; c.temperature = std::nanf(""); expect(refused(c.run(), "temperature"), "fine: a NaN temperature"); }
    { FinePoolCall c = fok; c.cb = 0; expect(refused(c.run(), "code books"), "fine: an empty code book"); }
    { FinePoolCall c = fok; c.place[1] = 1; expect(refused(c.run(), "named once"), "fine: a place named twice"); }
    { FinePoolCall c = fok; c.place[0] = 3; expect(refused(c.run(), "named once"), "fine: a place past the pool"); }
    { FinePoolCall c = fok; c.place[1] = 2; expect(refused(c.run(), "after the final call"), "fine: a finished stream"); }
    { FinePoolCall c = fok; c.n_frames[1] = 0; expect(refused(c.run(), "nothing pushed"), "fine: a final call with nothing pushed"); }
    { FinePoolCall c = fok; c.pos[2] = 262144; expect(refused(c.run(), "at most 262144"), "fine: a stream past 262144 frames"); }
    { FinePoolCall c = fok; c.uniforms = nullptr; expect(refused(c.run(), "uniforms do not cover"), "fine: sampling without uniforms"); }
    { FinePoolCall c = fok; c.u_windows[1] = 0; expect(refused(c.run(), "stream 1 of the call: the uniforms do not cover"), "fine: no draws for the second stream's window"); }
    { FinePoolCall c = fok; c.u_win0[0] = 1; expect(refused(c.run(), "stream 0 of the call: the uniforms do not cover"), "fine: draws that begin one window late"); }
    { FinePoolCall c = fok; c.u_cell0[0] = -1; expect(refused(c.run(), "must not be negative"), "fine: a negative draw cell"); }
    { FinePoolCall c = fok; c.uniforms = nullptr; c.greedy = 1; expect(refused(c.run(), "state too small"), "fine: the argmax needs no uniforms"); }
    { FinePoolCall c = fok; c.emit_stride = 63; expect(refused(c.run(), "emit_dev must hold"), "fine: emit_stride one short"); }
    { FinePoolCall c = fok; c.emit_stride = INT_MAX_ / 16 + 1; expect(refused(c.run(), "n * 8 * emit_stride must fit"), "fine: pieces that an int cannot address"); }
    { FinePoolCall c = fok; c.emit = nullptr; expect(refused(c.run(), "emit_dev must hold"), "fine: frames turn final and there is nowhere to put them"); }
    { FinePoolCall c = fok; c.trace_cap = 2; expect(refused(c.run(), "trace_cap"), "fine: a trace capacity without a trace"); }
    { FinePoolCall c = fok; c.n = 0; c.state_bytes = fneed; expect(c.run() == 0, "fine: a call that names no stream does nothing"); }
    expect(at::g_launches == 0, "no launcher was reached");
    if (!failures) std::printf("all refusals refused, %d launches\n", at::g_launches);
    return verdict("stream pool argument checks");
}
