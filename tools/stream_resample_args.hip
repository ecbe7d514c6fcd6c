// The host-side descriptor check of the streaming resampler (audiotoken_amd/csrc/stream_resample.hip: at_resample_rows_check) and the launcher's own argument
// checks under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program: it needs no device, because the checker is pure host code and every
// launcher case below is refused before anything is launched. Built and run by `make -C audiotoken_amd/csrc resample_asan`:
//   hipcc --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined tools/stream_resample_args.hip audiotoken_amd/csrc/stream_resample.hip
// The descriptor lists live in heap blocks of exactly nrows entries, so a read past the list is a sanitizer report, not a lucky pass; the extreme rows
// (positions at the ends of int64) are there for the checker's own arithmetic: it must refuse them without overflowing.
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../audiotoken_amd/csrc/at_common.h"
#include "../include/audiotoken_hip.h"

namespace at {
static std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }   // the library's lives in encodec.hip, which this program does not link
}  // namespace at

static int failures = 0;

static void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s (last error: %s)\n", what, at::g_error.c_str());
        ++failures;
    }
}

static int check(const std::vector<at_resample_row>& rows, int nrows) {
    std::unique_ptr<at_resample_row[]> heap(new at_resample_row[rows.size() ? rows.size() : 1]);   // exactly the list: no slack behind it
    if (!rows.empty()) std::memcpy(heap.get(), rows.data(), rows.size() * sizeof(at_resample_row));
    at::g_error.clear();
    return at_resample_rows_check(heap.get(), nrows);
}

static bool refused(int rc, const char* text) { return rc != 0 && at::g_error.find(text) != std::string::npos; }

static short pcm[8];
static float table[8];

// a stream at 44.1 kHz (o = 147, n = 80, width = 12) after its first push of 4096 samples: the window opens with `width` stored zeros
static at_resample_row first_push() {
    at_resample_row d{};
    d.pcm = pcm;
    d.table = table;
    d.src_base = -12;
    d.src_len = 12 + 4096;
    d.out_start = 0;
    d.out_len = ((4096 - 12) / 147) * 80;
    d.fmt = AT_PCM_S16;
    d.scale = 1.0f / 32768.0f;
    d.o = 147;
    d.n = 80;
    d.width = 12;
    return d;
}

// the whole signal of 4096 samples in one final row
static at_resample_row whole() {
    at_resample_row d = first_push();
    d.src_base = 0;
    d.src_len = d.src_total = 4096;
    d.final = 1;
    d.out_len = (int)((80ll * 4096 + 146) / 147);
    return d;
}

int main() {
    const int64_t big = std::numeric_limits<int64_t>::max(), small = std::numeric_limits<int64_t>::min();
    at_resample_row d = first_push();
    expect(check({d}, 1) == 0, "a first push");
    expect(check({whole()}, 1) == 0, "the whole signal, final");
    expect(check({d, whole(), d}, 3) == 0, "three rows");
    expect(check({d, whole()}, 1) == 0, "only the first nrows entries are read");
    at::g_error.clear();
    expect(refused(at_resample_rows_check(nullptr, 1), "null descriptor list"), "a null list");
    expect(refused(check({d}, 0), "nrows"), "nrows = 0");
    expect(refused(check({d}, -1), "nrows"), "nrows < 0");
    { at_resample_row e = d; e.pcm = nullptr; expect(refused(check({d, e}, 2), "row 1: null pcm"), "a null pcm pointer in the second row"); }
    { at_resample_row e = d; e.table = nullptr; expect(refused(check({e}, 1), "null resampling table"), "a null table at a resampled rate"); }
    { at_resample_row e = d; e.out_len = -1; expect(refused(check({e}, 1), "negative out_len"), "out_len = -1"); }
    { at_resample_row e = d; e.out_len = std::numeric_limits<int>::min(); expect(refused(check({e}, 1), "negative out_len"), "out_len = INT_MIN"); }
    { at_resample_row e = d; e.fmt = 4; expect(refused(check({e}, 1), "unknown sample format"), "fmt = 4"); }
    { at_resample_row e = d; e.fmt = -1; expect(refused(check({e}, 1), "unknown sample format"), "fmt = -1"); }
    { at_resample_row e = d; e.width = 11; expect(refused(check({e}, 1), "do not belong together"), "a width of another ratio"); }
    { at_resample_row e = d; e.o = 294; e.n = 160; expect(refused(check({e}, 1), "do not belong together"), "o and n with a common factor"); }
    { at_resample_row e = d; e.o = e.n = 2; expect(refused(check({e}, 1), "do not belong together"), "o = n = 2"); }
    { at_resample_row e = d; e.o = e.n = 1; e.width = 0; expect(refused(check({e}, 1), "do not belong together"), "a table at the native rate"); }
    { at_resample_row e = d; e.o = 0; expect(refused(check({e}, 1), "[1, 65535]"), "o = 0"); }
    { at_resample_row e = d; e.n = 65536; expect(refused(check({e}, 1), "[1, 65535]"), "n = 65536"); }
    { at_resample_row e = d; e.o = std::numeric_limits<int>::max(); expect(refused(check({e}, 1), "[1, 65535]"), "o = INT_MAX"); }
    { at_resample_row e = d; e.out_len += 80; expect(refused(check({e}, 1), "not final with a tap outside"), "one frame more than is ready"); }
    { at_resample_row e = d; e.src_base = 0; expect(refused(check({e}, 1), "not final with a tap outside"), "a first push without the stored zeros"); }
    { at_resample_row e = d; e.src_len = 12 + 26 * 147 + 12 + 147; expect(check({e}, 1) == 0, "a window that ends with the last tap of frame 26"); }
    { at_resample_row e = d; e.src_len = 12 + 26 * 147 + 12 + 147 - 1; expect(refused(check({e}, 1), "not final with a tap outside"), "a window one sample short"); }
    { at_resample_row e = whole(); e.src_base = 1; e.src_len -= 1; expect(refused(check({e}, 1), "final row with a tap inside"), "a final window that misses sample 0"); }
    { at_resample_row e = whole(); e.src_len -= 1; expect(refused(check({e}, 1), "final row with a tap inside"), "a final window that misses the last sample"); }
    { at_resample_row e = whole(); e.out_len += 1; expect(refused(check({e}, 1), "past the end"), "one output past ceil(n L / o)"); }
    { at_resample_row e = whole(); e.src_total = -1; expect(refused(check({e}, 1), "src_total"), "src_total = -1"); }
    { at_resample_row e = whole(); e.src_total = big; expect(refused(check({e}, 1), "src_total"), "src_total = INT64_MAX"); }
    for (int64_t v : {big, small}) {
        { at_resample_row e = d; e.src_base = v; expect(check({e}, 1) != 0, "src_base at an end of int64"); }
        { at_resample_row e = d; e.src_len = v; expect(check({e}, 1) != 0, "src_len at an end of int64"); }
        { at_resample_row e = d; e.out_start = v; expect(check({e}, 1) != 0, "out_start at an end of int64"); }
        { at_resample_row e = d; e.dst_off = v; expect(check({e}, 1) != 0, "dst_off at an end of int64"); }
        { at_resample_row e = whole(); e.out_start = v; expect(check({e}, 1) != 0, "a final out_start at an end of int64"); }
    }
    {   // positions far beyond 32 bits are fine when they belong together: 2^33 frames into a stream
        at_resample_row e = whole();
        const int64_t shift = 1ll << 33;
        e.src_base = shift * 147;
        e.src_total = e.src_base + 4096;
        e.out_start = shift * 80 + 80;          // from frame 1 on: frame 0 has taps before the window
        e.out_len -= 80;
        expect(check({e}, 1) == 0, "a row 2^33 frames into its stream");
        e.out_start -= 80;
        expect(refused(check({e}, 1), "final row with a tap inside"), "its frame 0, whose taps lie before the window");
    }
    {   // the native rate: conversion only
        at_resample_row e{};
        e.pcm = pcm;
        e.src_len = 8;
        e.out_len = 8;
        e.fmt = AT_PCM_F32;
        e.o = e.n = 1;
        expect(check({e}, 1) == 0, "a native row");
        e.out_len = 9;
        expect(refused(check({e}, 1), "not final with a tap outside"), "a native row that reads past its window");
    }
    {   // many rows: the list is walked to its end and no further
        std::vector<at_resample_row> all(4096, d);
        expect(check(all, 4096) == 0, "4096 rows");
        all.back().fmt = 9;
        expect(refused(check(all, 4096), "row 4095"), "4096 rows, the last one bad");
        all.push_back(d);
        expect(refused(check(all, 4097), "nrows"), "4097 rows");
    }
    // ---- the launcher's own checks: refused before the device is touched ----
    alignas(16) static float out[8];
    alignas(8) static at_resample_row one[1];
    auto launch = [&](const at_resample_row* r, int n, float* o) {
        at::g_error.clear();
        return at_resample_rows(r, n, o, nullptr);
    };
    expect(refused(launch(nullptr, 1, out), "null pointer"), "null rows");
    expect(refused(launch(one, 1, nullptr), "null pointer"), "null out");
    expect(refused(launch(one, 0, out), "nrows"), "nrows = 0 at the launcher");
    expect(refused(launch(one, 4097, out), "nrows"), "nrows = 4097 at the launcher");
    expect(refused(launch(one, 1, reinterpret_cast<float*>(reinterpret_cast<char*>(out) + 2)), "misaligned"), "an output that is not 4-byte aligned");
    if (failures) {
        std::printf("%d case(s) failed\n", failures);
        return 1;
    }
    std::printf("stream resampler argument checks: ok\n");
    return 0;
}
