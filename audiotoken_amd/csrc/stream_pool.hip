// Stream pools: rows of a stream state moved between a pool of S slots and a staging state of B rows.
//
// Both stream states (encodec_plan.h: StreamState, DecStreamState) are lists of planes [rows][w] that follow each other: a plane of an R-row state starts
// R * (sum of the widths before it) floats behind the state's base. One kernel copies row src_row(b) of every plane of the source to row dst_row(b) of
// the same plane of the destination, for b < B: gather reads row slots[b] of an S-row pool into row b of a B-row state, scatter is the inverse.
// A pure copy on 16-byte loads and stores (every width is a multiple of 4 floats, so every row start is 16-byte aligned when the bases are): no LDS,
// no atomics. The index space (b, float4 of a stream's planes in order) is walked grid-stride, so one row already spreads over several workgroups and
// 256 rows do not need more of them than the chip holds.
#include "encodec_kernels.h"

namespace at {

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

struct PoolPlanes {
    unsigned pre4[kPoolMaxPlanes + 1];  // float4 of a stream before plane p; the last entry = float4 of a whole stream (unused planes have width 0)
};

__global__ __launch_bounds__(256) void stream_pool_copy_kernel(const f4* __restrict__ src, f4* __restrict__ dst, const int* __restrict__ slots, PoolPlanes pl,
                                                               unsigned B, unsigned S, int gather) {
    const unsigned per4 = pl.pre4[kPoolMaxPlanes];
    const unsigned total = B * per4;   // the launcher keeps this below 2^31
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const unsigned b = i / per4, k = i - b * per4;
        unsigned lo = 0, hi = pl.pre4[1];   // the plane k falls into: [lo, hi) float4 of a stream (compile-time indices: the struct stays in scalar registers)
#pragma unroll
        for (int p = 1; p < kPoolMaxPlanes; ++p)
            if (k >= pl.pre4[p]) { lo = pl.pre4[p]; hi = pl.pre4[p + 1]; }
        const unsigned slot = (unsigned)slots[b];
        if (slot >= S) continue;   // validated on the host from the caller's copy of the list; a row outside the pool is never touched
        const unsigned w4 = hi - lo, j = k - lo;
        const size_t in_pool = (size_t)S * lo + (size_t)slot * w4 + j, in_state = (size_t)B * lo + (size_t)b * w4 + j;
        dst[gather ? in_state : in_pool] = src[gather ? in_pool : in_state];
    }
}

}  // namespace

int check_pool_slots(const int32_t* slots_host, int B, int S) {
    AT_REQUIRE(slots_host, "stream pool: null host slot list");
    AT_REQUIRE(B >= 1 && B <= S, "stream pool: need 1 <= B <= S");
    std::vector<bool> seen((size_t)S, false);
    for (int b = 0; b < B; ++b) {
        const int32_t s = slots_host[b];
        AT_REQUIRE(s >= 0 && s < S, "stream pool: slot outside [0, S)");
        AT_REQUIRE(!seen[(size_t)s], "stream pool: duplicate slot");
        seen[(size_t)s] = true;
    }
    return 0;
}

int launch_stream_pool_copy(const void* src, void* dst, const int* slots_dev, const int* widths, int n_planes, int B, int S, bool gather, hipStream_t stream) {
    AT_REQUIRE(src && dst && slots_dev && widths, "stream_pool_copy: null pointer");
    AT_REQUIRE(n_planes >= 1 && n_planes <= kPoolMaxPlanes && B >= 1 && B <= S, "stream_pool_copy: need 1 <= planes <= 6 and 1 <= B <= S");
    AT_REQUIRE((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) % 16 == 0, "stream_pool_copy: a state or pool that is not 16-byte aligned");
    PoolPlanes pl;
    pl.pre4[0] = 0;
    for (int p = 0; p < kPoolMaxPlanes; ++p) {
        const int w = p < n_planes ? widths[p] : 0;
        AT_REQUIRE(w >= 0 && w % 4 == 0 && (p >= n_planes || w > 0), "stream_pool_copy: plane widths must be positive multiples of 4 floats");
        pl.pre4[p + 1] = pl.pre4[p] + (unsigned)(w / 4);
    }
    const unsigned long long total = (unsigned long long)B * pl.pre4[kPoolMaxPlanes];
    AT_REQUIRE((unsigned long long)S * pl.pre4[kPoolMaxPlanes] < (1ull << 31), "stream_pool_copy: pool too large for 32-bit indices");
    const unsigned long long want = (total + 255) / 256, cap = 8ull * (unsigned)device_cus();
    hipLaunchKernelGGL(stream_pool_copy_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, stream, reinterpret_cast<const f4*>(src),
                       reinterpret_cast<f4*>(dst), slots_dev, pl, (unsigned)B, (unsigned)S, gather ? 1 : 0);
    AT_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace at
