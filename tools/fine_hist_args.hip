// The argument checks of the fine stage's history forms (audiotoken_amd/csrc/fine.hip: at_fine_generate_hist, at_fine_generate_queue_hist,
// at_fine_num_windows_hist, at_fine_state_bytes_hist, at_fine_queue_state_bytes_hist) under AddressSanitizer + UndefinedBehaviorSanitizer,
// as a stand-alone program next to tools/fine_args.hip. Two modes:
//   fine_hist_args                          every refusal path: nothing reaches a launch, so it needs no device
//   fine_hist_args sched W T Th [T Th ...]  the schedule alone (fine.h): per pair "row <h> <L> <n>" and then "<start> <fill>" per window
// Built and run by `make -C audiotoken_amd/csrc fine_hist_asan` (FINE_HIST_ARGS="sched ..." for the second mode). The handle is a finalized at_fine built
// by hand, the three launchers fine.hip's forward calls are stand-ins that count their calls, and the host arrays live in heap blocks of exactly the size
// a call may read, so a read past one is a sanitizer report.
#define ARGS_STAND_IN_GEMM
#include "decoder_args_common.h"

// W = 128, H = 64. Row 0 continues history 0 (70 frames: h = 64), row 1 has none. 300 frames after 64 history cells are 5 windows, without them 4.
struct Call {
    at_fine* h;
    bool queue = false;
    std::vector<int32_t> lens{300, 1};
    const int32_t* hist = fake_i;
    int h_stride = 70;
    std::vector<int32_t> hist_lens{70, 1};
    int n_hist = 2;
    std::vector<int32_t> of_row{0, -1};
    int max_hist = 70;
    int n_max = 5;
    size_t state_bytes = 16;
    int max_T = 300;

    int run() const {
        const auto l = exact_copy(lens), hl = exact_copy(hist_lens), of = exact_copy(of_row);
        at::g_error.clear();
        const int B = (int)lens.size();
        if (queue)
            return at_fine_generate_queue_hist(h, fake_i, l.get(), B, hist, h_stride, hl.get(), n_hist,
                                               of.get(), max_hist, 0.5f, 0, fake_f, fake_i, nullptr, nullptr, fake_f, state_bytes,
                                               max_T, 2, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
        return at_fine_generate_hist(h, fake_i, 300, l.get(), B, hist, h_stride, hl.get(), n_hist,
                                     of.get(), max_hist, 0.5f, 0, fake_f, n_max, fake_i, nullptr, nullptr, fake_f, state_bytes, max_T,
                                     nullptr, nullptr);
    }
};

static int refusals() {
    at_fine model;
    finalize_by_hand(&model);
    at_fine raw;   // never finalized
    const int W = 128, H = 64, top = 1 << 18;

    // ---- the window count with a history: n = max(0, ceil((T - (W - h)) / H)) + 1, h = min(H, Th)
    expect(at_fine_num_windows_hist(&model, 300, 0) == at_fine_num_windows(&model, 300), "no history: the count of at_fine_num_windows");
    expect(at_fine_num_windows_hist(&model, W - 1, 1) == 1 && at_fine_num_windows_hist(&model, W, 1) == 2, "one history frame moves the first hop by one");
    expect(at_fine_num_windows_hist(&model, H, H) == 1 && at_fine_num_windows_hist(&model, H + 1, H) == 2, "a full history leaves H cells to window 0");
    expect(at_fine_num_windows_hist(&model, H + 1, H + 5) == 2 && at_fine_num_windows_hist(&model, H + 1, top) == 2, "a history longer than H counts as H");
    expect(at_fine_num_windows_hist(&model, 300, 70) == 5, "300 frames after 64 history cells");
    expect(at_fine_num_windows_hist(&model, 300, -1) == 0 && at::g_error.find("history") != std::string::npos, "windows of Th = -1");
    expect(at_fine_num_windows_hist(&model, 300, top + 1) == 0, "windows of Th past the limit");
    expect(at_fine_num_windows_hist(&model, 300, std::numeric_limits<int>::min()) == 0, "windows of Th = INT_MIN");
    expect(at_fine_num_windows_hist(&model, 0, 5) == 0 && at_fine_num_windows_hist(&model, top + 1, 5) == 0, "windows of a bad T");
    expect(at_fine_num_windows_hist(&raw, 5, 5) == 0 && at_fine_num_windows_hist(nullptr, 5, 5) == 0, "windows before finalize");
    expect(at_fine_num_windows_hist(&model, top, top) == top / H, "windows of the longest row after the longest history");

    // ---- the state sizes: work arrays of max(min(H, max_hist) + max_T, W) cells
    at::g_error.clear();
    expect(at_fine_state_bytes_hist(&model, 2, 300, 0) == at_fine_state_bytes(&model, 2, 300), "no history: the size of at_fine_state_bytes");
    expect(at_fine_state_bytes_hist(&model, 2, 300, 1) > at_fine_state_bytes(&model, 2, 300), "state bytes grow with the history");
    expect(at_fine_state_bytes_hist(&model, 2, 300, H) == at_fine_state_bytes_hist(&model, 2, 300, top), "a history longer than H takes H cells");
    expect(at_fine_state_bytes_hist(&model, 2, 300, H) == at_fine_state_bytes(&model, 2, 300 + H), "H history cells cost what H more frames cost");
    expect(at_fine_state_bytes_hist(&model, 1, 1, H) == at_fine_state_bytes(&model, 1, 1), "a short row with its history still works in one window");
    expect(at_fine_state_bytes_hist(&model, 2, 300, -1) == 0 && at::g_error.find("max_hist") != std::string::npos, "state bytes, max_hist = -1");
    expect(at_fine_state_bytes_hist(&model, 2, 300, top + 1) == 0, "state bytes, max_hist past the limit");
    expect(at_fine_state_bytes_hist(&model, 0, 300, 5) == 0 && at_fine_state_bytes_hist(&model, 2, 0, 5) == 0, "state bytes, bad B or max_T");
    expect(at_fine_state_bytes_hist(nullptr, 2, 300, 5) == 0 && at_fine_state_bytes_hist(&raw, 2, 300, 5) == 0, "state bytes before finalize");
    expect(at_fine_state_bytes_hist(&model, 64, top, top) > 0, "state bytes of the largest call");
    expect(at_fine_queue_state_bytes_hist(&model, 2, 300, 70) == at_fine_state_bytes_hist(&model, 2, 300, 70), "the queue's state is the lockstep state of its slots");
    expect(at_fine_queue_state_bytes_hist(&model, 2, 300, 0) == at_fine_queue_state_bytes(&model, 2, 300), "the queue: no history");
    expect(at_fine_queue_state_bytes_hist(&model, 2, 300, -1) == 0 && at_fine_queue_state_bytes_hist(&model, 65, 300, 5) == 0, "the queue's state: bad arguments");

    // ---- both generators: a well-formed call with a state that is too small is refused last, which shows the rest was accepted
    for (int q = 0; q < 2; ++q) {
        Call ok{&model};
        ok.queue = q == 1;
        expect(refused(ok.run(), "state too small"), "a state that is too small");
        const size_t need = q ? at_fine_queue_state_bytes_hist(&model, 2, 300, 70) : at_fine_state_bytes_hist(&model, 2, 300, 70);
        { Call c = ok; c.state_bytes = need - 1; expect(refused(c.run(), "state too small"), "a state one byte short"); }
        { Call c = ok; c.state_bytes = at_fine_state_bytes(&model, 2, 300); expect(refused(c.run(), "state too small"), "a state sized without the history"); }
        { Call c = ok; c.h = nullptr; expect(refused(c.run(), "not finalized"), "a null handle"); }
        { Call c = ok; c.h = &raw; expect(refused(c.run(), "not finalized"), "a handle before finalize"); }
        { Call c = ok; c.hist = nullptr; expect(refused(c.run(), "null pointer"), "a null history table"); }
        { Call c = ok; c.hist_lens.clear(); expect(refused(c.run(), "null pointer"), "null history lengths"); }
        { Call c = ok; c.of_row.clear(); expect(refused(c.run(), "null pointer"), "a null history-of-row"); }
        { Call c = ok; c.n_hist = -1; expect(refused(c.run(), "n_hist"), "n_hist = -1"); }
        { Call c = ok; c.n_hist = 4097; expect(refused(c.run(), "n_hist"), "n_hist past the limit"); }
        { Call c = ok; c.h_stride = 0; expect(refused(c.run(), "h_stride"), "h_stride = 0"); }
        { Call c = ok; c.h_stride = top + 1; expect(refused(c.run(), "h_stride"), "h_stride past the limit"); }
        { Call c = ok; c.h_stride = 69; expect(refused(c.run(), "history 0 must be"), "a history longer than its stride"); }
        { Call c = ok; c.max_hist = 69; expect(refused(c.run(), "history 0 must be"), "a history longer than max_hist"); }
        { Call c = ok; c.max_hist = -1; expect(refused(c.run(), "max_hist"), "max_hist = -1"); }
        { Call c = ok; c.max_hist = top + 1; expect(refused(c.run(), "max_hist"), "max_hist past the limit"); }
        { Call c = ok; c.hist_lens = {70, 0}; expect(refused(c.run(), "history 1 must be"), "an empty history"); }
        { Call c = ok; c.hist_lens = {70, std::numeric_limits<int32_t>::min()}; expect(refused(c.run(), "history 1"), "a history length of INT_MIN"); }
        { Call c = ok; c.hist_lens = {std::numeric_limits<int32_t>::max(), 1}; expect(refused(c.run(), "history 0"), "a history length of INT_MAX"); }
        { Call c = ok; c.of_row = {0, 2}; expect(refused(c.run(), "row 1 must be -1 or"), "a history index past the table"); }
        { Call c = ok; c.of_row = {-2, -1}; expect(refused(c.run(), "row 0 must be -1 or"), "a history index below -1"); }
        { Call c = ok; c.of_row = {std::numeric_limits<int32_t>::max(), -1}; expect(refused(c.run(), "row 0"), "a history index of INT_MAX"); }
        { Call c = ok; c.n_hist = 0; expect(refused(c.run(), "row 0 must be -1"), "an empty table with a row that names an entry"); }
        { Call c = ok; c.n_hist = 0; c.of_row = {-1, -1}; c.hist = nullptr; c.hist_lens.clear(); c.n_max = 4; c.max_hist = 0;
          expect(refused(c.run(), "state too small"), "an empty table: the call without a history"); }
        { Call c = ok; c.n_hist = 0; c.of_row.clear(); c.hist = nullptr; c.hist_lens.clear(); expect(refused(c.run(), "state too small"), "an empty table needs no pointers"); }
        { Call c = ok; c.lens = {300, 0}; expect(refused(c.run(), "row 1 must be"), "an empty row"); }
        { Call c = ok; c.max_T = 299; expect(refused(c.run(), "row 0 must be"), "a row longer than max_T"); }
        // the edges that are accepted: one history frame, exactly H, more than H (the last H count), every row on one entry
        { Call c = ok; c.hist_lens = {1, 1}; c.n_max = 5; expect(refused(c.run(), "state too small"), "Th = 1"); }
        { Call c = ok; c.hist_lens = {H, 1}; expect(refused(c.run(), "state too small"), "Th = H"); }
        { Call c = ok; c.hist_lens = {H + 5, 1}; expect(refused(c.run(), "state too small"), "Th > H"); }
        { Call c = ok; c.h_stride = top; c.max_hist = top; c.hist_lens = {top, 1}; expect(refused(c.run(), "state too small"), "the longest history"); }
        { Call c = ok; c.of_row = {0, 0}; expect(refused(c.run(), "state too small"), "one entry shared by both rows"); }
        if (!q) {
            { Call c = ok; c.n_max = 4; expect(refused(c.run(), "n_max"), "n_max one short: 300 frames after 64 history cells are 5 windows"); }
            { Call c = ok; c.of_row = {-1, -1}; c.n_max = 4; expect(refused(c.run(), "state too small"), "without the history 4 windows are enough"); }
        }
    }
    expect(at::g_launches == 0, "no case reached a launch");
    return verdict("fine history argument checks");
}

static int sched(int argc, char** argv) {
    if (argc < 5 || (argc - 3) % 2) {
        std::printf("usage: fine_hist_args sched W T Th [T Th ...]\n");
        return 2;
    }
    const int W = std::atoi(argv[2]);
    if (!(W >= 128 && W % 128 == 0 && W <= at::FINE_MAX_BLOCK)) {
        std::printf("refused\n");
        return 2;
    }
    for (int i = 3; i + 1 < argc; i += 2) {
        const int T = std::atoi(argv[i]), Th = std::atoi(argv[i + 1]);
        if (!(T >= 1 && T <= at::FINE_MAX_T && Th >= 0 && Th <= at::FINE_MAX_T)) {
            std::printf("refused\n");
            return 2;
        }
        const int h = at::fine_history(Th, W), n = at::fine_windows(T, W, h);
        std::printf("row %d %d %d\n", h, at::fine_cells(T, W, h), n);
        for (int k = 0; k < n; ++k) {
            int start, fill;
            at::fine_window(k, T, W, h, &start, &fill);
            std::printf("%d %d\n", start, fill);
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::strcmp(argv[1], "sched") == 0) return sched(argc, argv);
    return refusals();
}
