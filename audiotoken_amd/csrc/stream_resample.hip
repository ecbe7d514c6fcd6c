// Stateful resampling of streamed audio: the resampling rule of the device feeder (audio_device.hip: chunk_sample) evaluated at
// GLOBAL sample positions of a signal that arrives in pieces. A row is a window of the signal on the device — the tail the stream carried over plus the new
// samples, or a whole resident file — and a run of consecutive output samples [out_start, out_start + out_len) whose taps lie in that window (or outside the
// signal: zeros). Output j: f = j / n, p = j % n, base = f o - width, y[j] = sum_{k in [lo_p, hi_p)} fmaf(K[p][k], x[base + k], acc) in ascending k — the very
// products and the very order chunk_sample takes when its chunk is the whole signal, so any cutting of the signal into rows gives that kernel's bits
// (tests/test_resample_stream_gpu.py: torch.equal).
//
// Positions are 64-bit (2^31 outputs are one day at 24 kHz), the per-sample arithmetic is not: a work item = 1024 consecutive outputs of one row resolves
// (f, p) of its first output once — uniform, with a 32-bit division while the position fits — and the window-relative index of that frame's tap 0 once; every
// sample then is a 32-bit offset from there. One launch serves all rows although only the device knows their lengths: the host fixes the grid (a few
// workgroups per compute unit) and every workgroup walks the rows' 1024-sample blocks in order, taking every gridDim.x-th one. The source samples are read
// through the caches as in the feeder's kernel (neighbouring outputs share all but o / n of their taps); no LDS, no atomics, 16-byte stores wherever the
// destination is aligned.
#include "at_common.h"
#include "../../include/audiotoken_hip.h"

#include <cmath>

namespace at {

namespace {

// mirrors `at_resample_row` (include/audiotoken_hip.h)
struct ResampleRow {
    const void* pcm;
    const float* table;
    long long src_base, src_len, src_total, out_start;
    int out_len, fmt;
    float scale;
    int o, n, width, final;
    int reserved;
    long long dst_off;
};

constexpr int kBlock = 1024;         // outputs per work item: 256 threads x 4
constexpr int kMaxRows = 4096;       // rows per launch: with out_len < 2^31 the block count of a launch stays below 2^33
constexpr long long kMaxPos = 1ll << 46;   // positions the checker accepts: n * position and f * o stay inside 64 bits for o, n < 2^16

// the sample conversion of audio_device.hip (pcm_load), with the format a template argument: the tap loop holds no switch
template <int FMT>
__device__ __forceinline__ float load_sample(const void* pcm, long long i, float scale) {
    if (FMT == AT_PCM_S16) return (float)static_cast<const short*>(pcm)[i] * scale;
    if (FMT == AT_PCM_S32) return (float)static_cast<const int*>(pcm)[i] * scale;
    if (FMT == AT_PCM_U8) return ((float)static_cast<const unsigned char*>(pcm)[i] - 128.0f) * scale;
    return static_cast<const float*>(pcm)[i];
}

__device__ __forceinline__ int clamp30(long long v) {
    const long long lim = 1ll << 30;
    return (int)(v < -lim ? -lim : (v > lim ? lim : v));
}

// block `blk` of row d: outputs [blk * 1024, min(out_len, blk * 1024 + 1024)) of the row, 4 consecutive ones per thread
template <int FMT>
__device__ __forceinline__ void resample_block(const ResampleRow& d, long long blk, float* __restrict__ out) {
    const long long i0 = blk * kBlock + (long long)threadIdx.x * 4;   // first of this thread's outputs inside the row
    if (i0 >= d.out_len) return;
    const int left = (int)(d.out_len - i0);                           // outputs of the row from i0 on (>= 1)
    const bool native = d.table == nullptr;
    // ---- uniform: where the block starts in the signal ----
    const long long j0 = d.out_start + blk * kBlock;
    long long f0;
    int p0;
    if (native) {
        f0 = j0;
        p0 = 0;
    } else if ((unsigned long long)j0 >> 32) {
        f0 = j0 / d.n;
        p0 = (int)(j0 - f0 * d.n);
    } else {
        const unsigned q = (unsigned)j0 / (unsigned)d.n;
        f0 = q;
        p0 = (int)((unsigned)j0 - q * (unsigned)d.n);
    }
    // window-relative index of tap 0 of frame f0, and the part of the window that holds samples of the signal, relative to it
    const long long rel0 = f0 * d.o - d.width - d.src_base;
    const long long lo_rel = d.src_base < 0 ? -d.src_base : 0;
    long long hi_rel = d.src_len;
    if (d.final && d.src_total - d.src_base < hi_rel) hi_rel = d.src_total - d.src_base;
    const int vlo = clamp30(lo_rel - rel0), vhi = clamp30(hi_rel - rel0);
    // ---- per thread: 32-bit from here ----
    const int kw = 2 * d.width + d.o;
    const int lin = p0 + (int)threadIdx.x * 4;
    int df = native ? lin : lin / d.n;     // frames past f0
    int p = native ? 0 : lin - df * d.n;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[e] = 0.f;
        if (e < left) {
            const int r0 = df * d.o;       // offset of this frame's tap 0 from rel0
            if (native) {
                if (r0 >= vlo && r0 < vhi) v[e] = load_sample<FMT>(d.pcm, rel0 + r0, d.scale);
            } else {
                const float* w = d.table + (long long)p * kw;
                const int* range = reinterpret_cast<const int*>(d.table + (long long)d.n * kw) + 2 * p;
                const int lo = range[0], hi = range[1];
                float acc = 0.f;
                for (int k = lo; k < hi; ++k) {
                    const int r = r0 + k;
                    const float x = (r >= vlo && r < vhi) ? load_sample<FMT>(d.pcm, rel0 + r, d.scale) : 0.f;
                    acc = fmaf(w[k], x, acc);
                }
                v[e] = acc;
            }
        }
        if (native || ++p == d.n) {
            p = 0;
            ++df;
        }
    }
    float* dst = out + d.dst_off + i0;
    if (left >= 4 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < left) dst[e] = v[e];
    }
}

__global__ __launch_bounds__(256) void resample_rows_kernel(const ResampleRow* __restrict__ rows, int nrows, float* __restrict__ out) {
    long long w = blockIdx.x, first = 0;   // this workgroup's next block among all rows' blocks; blocks before row r
    for (int r = 0; r < nrows; ++r) {
        const int len = rows[r].out_len;
        const long long end = first + (len > 0 ? (len >> 10) + ((len & (kBlock - 1)) != 0) : 0);
        if (w < end) {
            const ResampleRow d = rows[r];
            for (; w < end; w += gridDim.x) {
                switch (d.fmt) {
                    case AT_PCM_S16: resample_block<AT_PCM_S16>(d, w - first, out); break;
                    case AT_PCM_S32: resample_block<AT_PCM_S32>(d, w - first, out); break;
                    case AT_PCM_U8: resample_block<AT_PCM_U8>(d, w - first, out); break;
                    default: resample_block<AT_PCM_F32>(d, w - first, out); break;
                }
            }
        }
        first = end;
    }
}

int64_t gcd64(int64_t a, int64_t b) {
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

}  // namespace

}  // namespace at

extern "C" {

static_assert(sizeof(at_resample_row) == sizeof(at::ResampleRow) && sizeof(at_resample_row) == 88, "at_resample_row layout");

int at_resample_rows_check(const at_resample_row* rows, int nrows) {
    using namespace at;
    AT_REQUIRE(rows, "at_resample_rows_check: null descriptor list");
    AT_REQUIRE(nrows >= 1 && nrows <= kMaxRows, "at_resample_rows_check: need 1 <= nrows <= 4096");
    for (int r = 0; r < nrows; ++r) {
        const at_resample_row& d = rows[r];
        const std::string row = "at_resample_rows_check: row " + std::to_string(r) + ": ";
        AT_REQUIRE(d.pcm, row + "null pcm pointer");
        AT_REQUIRE(d.fmt == AT_PCM_S16 || d.fmt == AT_PCM_S32 || d.fmt == AT_PCM_F32 || d.fmt == AT_PCM_U8, row + "unknown sample format");
        AT_REQUIRE(d.out_len >= 0, row + "negative out_len");
        AT_REQUIRE(d.src_len >= 0 && d.out_start >= 0 && d.dst_off >= 0, row + "negative src_len, out_start or dst_off");
        AT_REQUIRE(d.o >= 1 && d.n >= 1 && d.o < 65536 && d.n < 65536 && d.width >= 0, row + "o and n must lie in [1, 65535], width >= 0");
        if (d.o == d.n) {
            AT_REQUIRE(d.o == 1 && d.width == 0 && !d.table, row + "o, n, width do not belong together: the native rate is o = n = 1, width = 0, no table");
        } else {
            const int m = d.o < d.n ? d.o : d.n;
            const int width = (int)std::ceil((double)(6 * (int64_t)d.o) / ((double)m * 0.99));   // audio_io.resample_table
            AT_REQUIRE(gcd64(d.o, d.n) == 1 && d.width == width, row + "o, n, width do not belong together: o and n coprime, width = ceil(6 o / (0.99 min(o, n)))");
            AT_REQUIRE(d.table, row + "null resampling table");
        }
        AT_REQUIRE(d.src_base >= -kMaxPos && d.src_base <= kMaxPos && d.src_len <= kMaxPos && d.out_start <= kMaxPos && d.dst_off <= kMaxPos,
                   row + "position beyond 2^46");
        if (d.final) {
            AT_REQUIRE(d.src_total >= 0 && d.src_total <= kMaxPos, row + "src_total outside [0, 2^46]");
            const int64_t total_out = (d.n * d.src_total + d.o - 1) / d.o;
            AT_REQUIRE(d.out_start + d.out_len <= total_out, row + "outputs past the end of the signal: ceil(n src_total / o)");
        }
        if (d.out_len == 0) continue;
        const int64_t fa = d.out_start / d.n, fb = (d.out_start + d.out_len - 1) / d.n;
        int64_t lo = fa * d.o - d.width, hi = fb * d.o + d.width + d.o;   // taps of the row's outputs: source samples [lo, hi)
        const int64_t wlo = d.src_base, whi = d.src_base + d.src_len;
        if (d.final) {
            if (lo < 0) lo = 0;
            if (hi > d.src_total) hi = d.src_total;
            AT_REQUIRE(lo >= hi || (lo >= wlo && hi <= whi), row + "a final row with a tap inside the signal but outside its window");
        } else {
            AT_REQUIRE(lo >= wlo && hi <= whi, row + "a row that is not final with a tap outside its window");
        }
    }
    return 0;
}

int at_resample_rows(const at_resample_row* rows_dev, int nrows, float* out, at_stream_t stream) {
    using namespace at;
    AT_REQUIRE(rows_dev && out, "at_resample_rows: null pointer");
    AT_REQUIRE(nrows >= 1 && nrows <= kMaxRows, "at_resample_rows: need 1 <= nrows <= 4096");
    AT_REQUIRE(reinterpret_cast<uintptr_t>(out) % 4 == 0 && reinterpret_cast<uintptr_t>(rows_dev) % 8 == 0, "at_resample_rows: misaligned pointer");
    hipLaunchKernelGGL(resample_rows_kernel, dim3(8u * (unsigned)device_cus()), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const ResampleRow*>(rows_dev),
                       nrows, out);
    AT_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
