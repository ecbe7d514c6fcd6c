// The host side of the semantic-to-audio stream (audiotoken_amd/csrc/gpt.hip: at_gpt_stream_push, at_gpt_stream_state_bytes; fine.hip:
// at_fine_stream_push, at_fine_stream_state_bytes, at_op_fine_handover; gpt.h / fine.h: GptStreamSchedule, FineStreamSchedule) under AddressSanitizer +
// UndefinedBehaviorSanitizer, as a stand-alone program in the style of tools/gpt_long_args.hip: both handles are finalized by hand with no device behind
// them, and every case is refused before anything is launched. Built and run by `make -C audiotoken_amd/csrc semantic_stream_asan`.
//   no arguments                         every refusal path
//   gpt S H n_before:n_new:final ...     the rounds GptStreamSchedule makes of each push, one line per round
//   fine W T_before:n_new:final ...      the rounds FineStreamSchedule makes of each push
// tests/test_semantic_stream_cpu.py compares the printed rounds with the Python twins' (semantic_stream.gpt_stream_rounds / fine_stream_rounds).
#include <cstdlib>

#include "decoder_args_common.h"

alignas(16) static int32_t fake_ids[4];

// A model of 128 positions and 256 ids as in gpt_long_args.hip: semantic ids [0, 64), the two code books [64, 128) and [128, 192), INFER 200, STOP 201;
// S = 8, H = 4, r = 3. A stream with 13 ids behind it (windows 0 and 1 have run) that is pushed 4 more: window 2 runs, stream positions 36 to 47.
struct GptCall {
    at_gpt* h;
    void* state = fake_f;
    size_t state_bytes = 0;
    int64_t pos[2] = {13, 0};
    const int32_t* ids = fake_i;
    int n_new = 4, final = 0, S = 8, H = 4, r = 3;
    int sem_off = 0, sem_vocab = 64, infer = 200, ac_off = 64, cb = 64, stop = 201, max_new = 16;
    float temperature = 0.8f;
    int top_k = 100;
    const float* uniforms = fake_f;
    int64_t u_pos0 = 36, u_len = 12;
    int32_t *out_ids = fake_i, *out_len = fake_i, *finish = fake_i;
    int out_cap = 24;   // the carry (12) and window 2's ids (12)

    int run() {
        at::g_error.clear();
        return at_gpt_stream_push(h, state, state_bytes, pos, ids, n_new, final, S, H, r, sem_off, sem_vocab, infer, ac_off, cb, stop, max_new, temperature, top_k,
                                  uniforms, u_pos0, u_len, out_ids, out_cap, out_len, finish, nullptr, nullptr, nullptr);
    }
};

// The fine model of fine_args.hip (W = 128). A stream with 100 frames behind it that is pushed 60 more: window 0 runs, frames [0, 64) turn final.
struct FineCall {
    at_fine* h;
    void* state = fake_f;
    size_t state_bytes = 0;
    int64_t pos[2] = {100, 0};
    const int32_t* ids = fake_ids;
    int n_frames = 60, final = 0, ac_off = 64, cb = 1024;
    float temperature = 0.5f;
    int greedy = 0;
    const float* uniforms = fake_f;
    int u_win0 = 0, u_windows = 1;
    int64_t* emit = reinterpret_cast<int64_t*>(fake_ids);
    int emit_stride = 64;
    int32_t n_emitted = -1;

    int run() {
        at::g_error.clear();
        return at_fine_stream_push(h, state, state_bytes, pos, ids, n_frames, final, ac_off, cb, temperature, greedy, uniforms, u_win0, u_windows, emit, emit_stride,
                                   &n_emitted, nullptr, nullptr, nullptr);
    }
};

static int dry(int argc, char** argv) {
    const bool gpt = std::string(argv[1]) == "gpt";
    const int a = std::atoi(argv[2]), b = gpt ? std::atoi(argv[3]) : 0;
    for (int i = gpt ? 4 : 3; i < argc; ++i) {
        long long before = 0;
        int n_new = 0, final = 0;
        if (std::sscanf(argv[i], "%lld:%d:%d", &before, &n_new, &final) != 3) { std::printf("refused: %s\n", argv[i]); return 2; }
        std::printf("push %lld %d %d\n", before, n_new, final);
        if (gpt) {
            at::GptStreamSchedule s(before, n_new, final != 0, a, b);
            at::GptStreamRound r;
            while (s.next(&r)) std::printf("round %d %d %d %d %d %d\n", r.take, r.held, r.k_first, r.n_win, r.final_window ? 1 : 0, r.final_ids);
        } else {
            at::FineStreamSchedule s(before, n_new, final != 0, a);
            at::FineStreamRound r;
            while (s.next(&r))
                std::printf("round %d %lld %d %d %d %d %d %d %lld %lld %d\n", r.take, r.first, r.held, r.j_first, r.n_win, r.pad, r.last_window ? 1 : 0, r.last_rel,
                            r.emit_from, r.emit_to, r.shift);
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 4) return dry(argc, argv);
    at_gpt model;
    finalize_by_hand(&model, 256);
    at_gpt raw;
    at_fine fine;
    finalize_by_hand(&fine);
    at_fine fraw;

    // ---- at_gpt_stream_state_bytes: fixed by the geometry
    const size_t need = at_gpt_stream_state_bytes(&model, 8, 4, 3);
    expect(need > at_gpt_long_state_bytes(&model, 1, 128), "the stream state holds the one-row state and its own buffers");
    expect(at_gpt_stream_state_bytes(nullptr, 8, 4, 3) == 0 && at_gpt_stream_state_bytes(&raw, 8, 4, 3) == 0, "state bytes without a finalized model");
    expect(at_gpt_stream_state_bytes(&model, 7, 4, 3) == 0 && at_gpt_stream_state_bytes(&model, 8, 10, 3) == 0 && at_gpt_stream_state_bytes(&model, 32, 16, 3) == 0,
           "state bytes: odd S, H > S, a window past the block");
    expect(at_gpt_stream_state_bytes(&model, INT_MAX_ - 1, 2, 3) == 0 && at_gpt_stream_state_bytes(&model, 8, 4, 0) == 0, "state bytes: extreme values");

    // ---- at_gpt_stream_push: a well-formed call with a state that is too small is refused last
    GptCall ok{&model};
    ok.state_bytes = 16;
    expect(refused(ok.run(), "state too small"), "a state that is too small");
    expect(ok.pos[0] == 13 && ok.pos[1] == 0, "a refused call leaves the stream's record as it was");
    { GptCall c = ok; c.state_bytes = need - 1; expect(refused(c.run(), "state too small"), "a state one byte short"); }
    { GptCall c = ok; c.h = nullptr; expect(refused(c.run(), "not finalized"), "a null handle"); }
    { GptCall c = ok; c.h = &raw; expect(refused(c.run(), "not finalized"), "a handle before finalize"); }
    { GptCall c = ok; c.state = nullptr; expect(refused(c.run(), "null state"), "a null state"); }
    { GptCall c = ok; c.uniforms = nullptr; expect(refused(c.run(), "null pointer"), "null uniforms"); }
    { GptCall c = ok; c.out_ids = nullptr; expect(refused(c.run(), "null pointer"), "null out_ids"); }
    { GptCall c = ok; c.out_len = nullptr; expect(refused(c.run(), "null pointer"), "null out_len"); }
    { GptCall c = ok; c.finish = nullptr; expect(refused(c.run(), "null pointer"), "null finish"); }
    { GptCall c = ok; c.ids = nullptr; expect(refused(c.run(), "ids need a pointer"), "ids without a pointer"); }
    { GptCall c = ok; c.n_new = -1; expect(refused(c.run(), "must not be negative"), "a negative n_new"); }
    { GptCall c = ok; c.final = 2; expect(refused(c.run(), "final must be"), "final = 2"); }
    { GptCall c = ok; c.pos[1] = 1; expect(refused(c.run(), "after the final call"), "a push after the final call"); }
    { GptCall c = ok; c.pos[1] = 1; c.final = 1; c.n_new = 0; expect(refused(c.run(), "after the final call"), "a second final call"); }
    { GptCall c = ok; c.pos[0] = 0; c.n_new = 0; c.final = 1; expect(refused(c.run(), "nothing pushed"), "a final call with nothing pushed"); }
    { GptCall c = ok; c.pos[0] = 65533; expect(refused(c.run(), "at most 65536"), "a stream past 65536 ids"); }
    { GptCall c = ok; c.pos[0] = -1; expect(refused(c.run(), "at most 65536"), "a negative record"); }
    { GptCall c = ok; c.S = 7; expect(refused(c.run(), "must be even"), "an odd window"); }
    { GptCall c = ok; c.H = 10; expect(refused(c.run(), "must not exceed the window"), "a hop past the window"); }
    { GptCall c = ok; c.S = 32; c.H = 16; expect(refused(c.run(), "does not fit"), "S + 1 + r S one past the block"); }
    { GptCall c = ok; c.r = 0; expect(refused(c.run(), "r (acoustic ids"), "r = 0"); }
    { GptCall c = ok; c.sem_vocab = 0; expect(refused(c.run(), "semantic ids"), "an empty semantic vocabulary"); }
    { GptCall c = ok; c.infer = 256; expect(refused(c.run(), "infer_token"), "INFER outside the vocabulary"); }
    { GptCall c = ok; c.ac_off = 129; expect(refused(c.run(), "code books"), "code book 1 past the vocabulary"); }
    { GptCall c = ok; c.stop = 256; expect(refused(c.run(), "stop_token"), "a stop token outside the vocabulary"); }
    for (int m : {0, 1025, -1}) { GptCall c = ok; c.max_new = m; expect(refused(c.run(), "max_new"), "max_new out of range"); }
    { GptCall c = ok; c.temperature = 0.0f; expect(refused(c.run(), "temperature"), "temperature 0"); }
    { GptCall c = ok; c.top_k = 0; expect(refused(c.run(), "top_k"), "top_k = 0"); }
    // the caller's arrays against the windows the call will run
    { GptCall c = ok; c.u_pos0 = 37; expect(refused(c.run(), "uniforms do not cover"), "uniforms that begin one position late"); }
    { GptCall c = ok; c.u_len = 11; expect(refused(c.run(), "uniforms do not cover"), "uniforms one short"); }
    { GptCall c = ok; c.u_pos0 = -1; expect(refused(c.run(), "must not be negative"), "a negative u_pos0"); }
    { GptCall c = ok; c.out_cap = 23; expect(refused(c.run(), "out_cap"), "out_cap one short of the carry and the new ids"); }
    { GptCall c = ok; c.n_new = 3; c.u_len = 0; c.out_cap = 0; expect(refused(c.run(), "state too small"), "a push that runs no window needs no draws and no room"); }
    { GptCall c = ok; c.n_new = 0; c.final = 1; c.u_pos0 = 36; c.u_len = 16; c.out_cap = 28;
      expect(refused(c.run(), "state too small"), "the final window after 13 ids: 5 ids, 12 carried, a budget of 16"); }
    { GptCall c = ok; c.n_new = 0; c.final = 1; c.u_pos0 = 36; c.u_len = 15; c.out_cap = 28; expect(refused(c.run(), "uniforms do not cover"), "the final window, uniforms one short"); }
    { GptCall c = ok; c.pos[0] = 0; c.n_new = 200; c.u_pos0 = 0; c.u_len = 588; c.out_cap = 588;
      expect(refused(c.run(), "state too small"), "a long first push: 48 windows, 24 + 47 * 12 ids"); }
    { GptCall c = ok; c.pos[0] = 0; c.n_new = 200; c.u_pos0 = 0; c.u_len = 587; c.out_cap = 588; expect(refused(c.run(), "uniforms do not cover"), "a long first push, one draw short"); }
    { GptCall c = ok; c.pos[0] = 0; c.n_new = 200; c.u_pos0 = 0; c.u_len = 588; c.out_cap = 587; expect(refused(c.run(), "out_cap"), "a long first push, one id short"); }

    // ---- the fine stream
    at::g_error.clear();
    const size_t fneed = at_fine_stream_state_bytes(&fine);
    expect(fneed == at_fine_state_bytes(&fine, 1, 256), "the fine stream's state is one row of 2 W cells");
    expect(at_fine_stream_state_bytes(nullptr) == 0 && at_fine_stream_state_bytes(&fraw) == 0, "fine state bytes without a finalized model");
    FineCall fok{&fine};
    fok.state_bytes = 16;
    expect(refused(fok.run(), "state too small"), "fine: a state that is too small");
    expect(fok.pos[0] == 100 && fok.pos[1] == 0 && fok.n_emitted == -1, "fine: a refused call leaves the record as it was");
    { FineCall c = fok; c.state_bytes = fneed - 1; expect(refused(c.run(), "state too small"), "fine: a state one byte short"); }
    { FineCall c = fok; c.h = nullptr; expect(refused(c.run(), "not finalized"), "fine: a null handle"); }
    { FineCall c = fok; c.h = &fraw; expect(refused(c.run(), "not finalized"), "fine: a handle before finalize"); }
    { FineCall c = fok; c.state = nullptr; expect(refused(c.run(), "null state"), "fine: a null state"); }
    { FineCall c = fok; c.ids = nullptr; expect(refused(c.run(), "frames need a pointer"), "fine: frames without a pointer"); }
    { FineCall c = fok; c.ids = fake_ids + 1; expect(refused(c.run(), "8-byte aligned"), "fine: ids that are not 8-byte aligned"); }
    { FineCall c = fok; c.n_frames = -1; expect(refused(c.run(), "must not be negative"), "fine: a negative n_frames"); }
    { FineCall c = fok; c.final = -1; expect(refused(c.run(), "final must be"), "fine: final = -1"); }
    { FineCall c = fok; c.greedy = 2; expect(refused(c.run(), "greedy must be"), "fine: greedy = 2"); }
    { FineCall c = fok; c.temperature = std::nanf(""); expect(refused(c.run(), "temperature"), "fine: a NaN temperature"); }
    { FineCall c = fok; c.cb = 0; expect(refused(c.run(), "code books"), "fine: an empty code book"); }
    { FineCall c = fok; c.ac_off = INT_MAX_; expect(refused(c.run(), "code books"), "fine: code books past int32"); }
    { FineCall c = fok; c.pos[1] = 1; expect(refused(c.run(), "after the final call"), "fine: a push after the final call"); }
    { FineCall c = fok; c.pos[0] = 0; c.n_frames = 0; c.final = 1; expect(refused(c.run(), "nothing pushed"), "fine: a final call with nothing pushed"); }
    { FineCall c = fok; c.pos[0] = 262144; expect(refused(c.run(), "at most 262144"), "fine: a stream past 262144 frames"); }
    { FineCall c = fok; c.uniforms = nullptr; expect(refused(c.run(), "uniforms do not cover"), "fine: sampling without uniforms"); }
    { FineCall c = fok; c.u_windows = 0; expect(refused(c.run(), "uniforms do not cover"), "fine: no window's draws"); }
    { FineCall c = fok; c.u_win0 = 1; expect(refused(c.run(), "uniforms do not cover"), "fine: draws that begin one window late"); }
    { FineCall c = fok; c.uniforms = nullptr; c.greedy = 1; expect(refused(c.run(), "state too small"), "fine: the argmax needs no uniforms"); }
    { FineCall c = fok; c.emit_stride = 63; expect(refused(c.run(), "emit_dev must hold"), "fine: emit_stride one short"); }
    { FineCall c = fok; c.emit = nullptr; expect(refused(c.run(), "emit_dev must hold"), "fine: frames turn final and there is nowhere to put them"); }
    { FineCall c = fok; c.n_frames = 27; c.emit = nullptr; c.emit_stride = 0; c.u_windows = 0;
      expect(refused(c.run(), "state too small"), "fine: a push that runs no window needs no draws and no room"); }
    { FineCall c = fok; c.n_frames = 0; c.final = 1; c.emit_stride = 100; expect(refused(c.run(), "state too small"), "fine: the padded single window emits T frames"); }
    { FineCall c = fok; c.n_frames = 0; c.final = 1; c.emit_stride = 99; expect(refused(c.run(), "emit_dev must hold"), "fine: the padded single window, one column short"); }
    { FineCall c = fok; c.pos[0] = 0; c.n_frames = 1000; c.u_windows = 14; c.emit_stride = 896;
      expect(refused(c.run(), "state too small"), "fine: a long first push: 14 windows, 896 frames final"); }
    { FineCall c = fok; c.pos[0] = 0; c.n_frames = 1000; c.u_windows = 13; c.emit_stride = 896; expect(refused(c.run(), "uniforms do not cover"), "fine: a long first push, one window short"); }
    { FineCall c = fok; c.pos[0] = 0; c.n_frames = 1000; c.final = 1; c.u_windows = 15; c.emit_stride = 1000;
      expect(refused(c.run(), "state too small"), "fine: a long only push: 15 windows, the last at rel > 0, every frame final"); }
    // ---- the hand-over op
    at::g_error.clear();
    expect(refused(at_op_fine_handover(nullptr, 4, 0, 64, 64, fake_ids, nullptr, nullptr), "frames need a pointer"), "hand-over: frames without a pointer");
    expect(refused(at_op_fine_handover(fake_ids, 1, 0, 64, 64, nullptr, nullptr, nullptr), "work array"), "hand-over: a null work array");
    expect(refused(at_op_fine_handover(fake_ids, 1, -1, 64, 64, fake_ids, nullptr, nullptr), "work array"), "hand-over: a negative n_pad");
    expect(refused(at_op_fine_handover(fake_ids, 1, 0, 64, 64, fake_ids + 1, nullptr, nullptr), "16-byte aligned"), "hand-over: a work array that is not 16-byte aligned");
    expect(refused(at_op_fine_handover(fake_ids + 1, 1, 0, 64, 64, fake_ids, nullptr, nullptr), "8-byte aligned"), "hand-over: ids that are not 8-byte aligned");
    expect(at::g_launches == 0, "no launcher was reached");
    return verdict("semantic stream argument checks");
}
