// Host-side argument checks of the stream pool copies (audiotoken_amd/csrc/stream_pool.hip) under AddressSanitizer, as a stand-alone program: it needs no
// device, because every case below is refused before anything is launched. Built and run by `make -C audiotoken_amd/csrc pool_asan`:
//   hipcc --offload-arch=gfx950 -Xarch_host -fsanitize=address tools/stream_pool_args.hip audiotoken_amd/csrc/stream_pool.hip
// The slot lists live in heap blocks of exactly B entries, so a read past the list is an AddressSanitizer report, not a lucky pass.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../audiotoken_amd/csrc/encodec_kernels.h"

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

static int check(const std::vector<int32_t>& slots, int B, int S) {
    std::unique_ptr<int32_t[]> heap(new int32_t[slots.size() ? slots.size() : 1]);   // exactly the list: no slack behind it
    if (!slots.empty()) std::memcpy(heap.get(), slots.data(), slots.size() * sizeof(int32_t));
    at::g_error.clear();
    return at::check_pool_slots(heap.get(), B, S);
}

static bool refused(int rc, const char* text) { return rc != 0 && at::g_error.find(text) != std::string::npos; }

int main() {
    // ---- the slot list ----
    expect(check({4, 0, 2}, 3, 5) == 0, "three distinct slots of five");
    expect(check({0}, 1, 1) == 0, "B = S = 1");
    expect(check({4, 3, 2, 1, 0}, 5, 5) == 0, "B = S, reversed");
    at::g_error.clear();
    expect(refused(at::check_pool_slots(nullptr, 1, 5), "null host slot list"), "a null list");
    expect(refused(check({0}, 0, 5), "1 <= B <= S"), "B = 0");
    expect(refused(check({0}, -3, 5), "1 <= B <= S"), "B < 0");
    expect(refused(check({0, 1, 2, 3, 4, 0}, 6, 5), "1 <= B <= S"), "B > S");
    expect(refused(check({0}, 1, 0), "1 <= B <= S"), "S = 0");
    expect(refused(check({0, 5, 2}, 3, 5), "outside [0, S)"), "slot S");
    expect(refused(check({0, 1, -1}, 3, 5), "outside [0, S)"), "slot -1");
    expect(refused(check({2147483647}, 1, 5), "outside [0, S)"), "slot INT_MAX");
    expect(refused(check({-2147483647 - 1}, 1, 5), "outside [0, S)"), "slot INT_MIN");
    expect(refused(check({2, 0, 2}, 3, 5), "duplicate slot"), "a duplicate slot");
    expect(refused(check({1, 1}, 2, 2), "duplicate slot"), "a duplicate with B = S");
    expect(check({7, 1}, 1, 8) == 0, "only the first B entries are read");
    {   // a large pool: the seen-set is sized by S
        std::vector<int32_t> all(100000);
        for (int i = 0; i < 100000; ++i) all[(size_t)i] = 99999 - i;
        expect(check(all, 100000, 100000) == 0, "S = B = 100000");
        all[99999] = all[0];
        expect(refused(check(all, 100000, 100000), "duplicate slot"), "S = B = 100000 with one duplicate");
    }
    // ---- the launcher's own checks: refused before the device is touched ----
    alignas(16) static float a[64], b[64];
    const int32_t slots[1] = {0};
    const int enc[6] = {640, 512, 512, 512, 512, 3072};
    auto launch = [&](const void* src, void* dst, const int32_t* s, const int* w, int n, int B, int S) {
        at::g_error.clear();
        return at::launch_stream_pool_copy(src, dst, s, w, n, B, S, true, nullptr);
    };
    expect(refused(launch(nullptr, b, slots, enc, 6, 1, 5), "null pointer"), "null source");
    expect(refused(launch(a, nullptr, slots, enc, 6, 1, 5), "null pointer"), "null destination");
    expect(refused(launch(a, b, nullptr, enc, 6, 1, 5), "null pointer"), "null device slots");
    expect(refused(launch(a, b, slots, nullptr, 6, 1, 5), "null pointer"), "null widths");
    expect(refused(launch(a, b, slots, enc, 0, 1, 5), "planes"), "no planes");
    expect(refused(launch(a, b, slots, enc, 7, 1, 5), "planes"), "seven planes");
    expect(refused(launch(a, b, slots, enc, 6, 6, 5), "planes"), "B > S");
    expect(refused(launch(a + 1, b, slots, enc, 6, 1, 5), "16-byte aligned"), "an unaligned source");
    expect(refused(launch(a, b + 2, slots, enc, 6, 1, 5), "16-byte aligned"), "an unaligned destination");
    const int odd[6] = {640, 512, 510, 512, 512, 3072}, zero[6] = {640, 0, 512, 512, 512, 3072}, neg[6] = {640, -4, 512, 512, 512, 3072};
    expect(refused(launch(a, b, slots, odd, 6, 1, 5), "multiples of 4"), "a width that is no multiple of 4");
    expect(refused(launch(a, b, slots, zero, 6, 1, 5), "multiples of 4"), "a plane of width 0");
    expect(refused(launch(a, b, slots, neg, 6, 1, 5), "multiples of 4"), "a negative width");
    expect(refused(launch(a, b, slots, enc, 6, 1, 2000000), "too large"), "a pool past 32-bit float4 indices");
    if (failures) {
        std::printf("%d case(s) failed\n", failures);
        return 1;
    }
    std::printf("stream pool argument checks: ok\n");
    return 0;
}
