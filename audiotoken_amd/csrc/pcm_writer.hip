// Device side of the output path of decode_batch_files: the decoder's padded float32 batch -> the 16-bit PCM of its valid samples, compacted
// into ONE int16 buffer that a single device-to-host copy carries to the WAV writer (audiotoken_amd/writer.py). The mirror image of audio_device.hip: there
// the host keeps headers and index arithmetic and the device touches the samples on the way in; here the same split on the way out. Clamp, scale, round and
// narrow on the host cost 5-10 x the decode itself and hold 4 bytes per sample across the bus; here the bus carries 2.
//
// Arithmetic per sample x of a row with scale s (the host computes s in fp32 and passes it in the descriptor, so numpy reproduces every bit:
// tests/pcm_ref.py), limit L (0.99 for the product path: the reference's save_audio clamps to +-0.99):
//   NaN          -> 0, counted as non-finite
//   +-infinity   -> +-L, counted as non-finite
//   otherwise    y = x * s (one fp32 multiply), c = min(max(y, -L), L), counted as clipped when c != y
//   q = rint(c * 32768)  round half to even (v_rndne_f32; the multiply by 2^15 is exact), stored as int16: |q| <= 32440 at L = 0.99
// There is no addition anywhere, so -ffp-contract=on has nothing to fuse (the ISA holds v_mul_f32 / v_rndne_f32 and no fma).
//
// Shape: pure streaming, 4 B in and 2 B out per sample. A tile is 2048 consecutive samples of one row: every thread loads two float4 and stores one 16-byte
// group of eight int16 when the row's source and destination are 16-byte aligned (row offsets of the product path are multiples of 320 samples: always),
// and falls back to element accesses for a misaligned row and for the ragged end of any row. Tiles are taken grid-stride by at most 8 workgroups per CU, so
// a 3-row batch and a 256-row batch both spread over the chip. Counts: one packed per-thread counter, a wave reduction, then ONE vector atomic instruction per wave
// (lane 0 adds the clipped count, lane 1 the non-finite count) and none when both are zero. Peaks: fmaxf per thread and per wave, then an integer atomic max
// on the bit pattern (non-negative floats order like unsigned integers), so the result does not depend on arrival order.
#include "at_common.h"
#include "../../include/audiotoken_hip.h"
#include "pcm_quant.h"

#include <cmath>

namespace at {

// mirrors `at_pcm_row_desc` (include/audiotoken_hip.h)
struct PcmRow {
    long long src_off;   // first sample of the row, in floats from `src`
    long long dst_off;   // first sample of the row in the packed output, in int16 elements from `dst`
    long long n;         // samples of the row
    float scale;         // multiplies every finite sample before the clamp
    int reserved;
};

constexpr int PCM_PER_THREAD = 8;
constexpr int PCM_TILE = 256 * PCM_PER_THREAD;

__device__ __forceinline__ unsigned pack2(int lo, int hi) { return ((unsigned)lo & 0xffffu) | ((unsigned)hi << 16); }

__global__ __launch_bounds__(256) void pcm_pack_kernel(const float* __restrict__ src, const PcmRow* __restrict__ rows, unsigned tiles_per_row, unsigned total_tiles,
                                                       float limit, short* __restrict__ dst, unsigned* __restrict__ counts) {
    const int i0 = (int)threadIdx.x * PCM_PER_THREAD, lane = (int)threadIdx.x & 63;
    for (unsigned tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
        const unsigned row = tile / tiles_per_row, tr = tile - row * tiles_per_row;
        const PcmRow d = rows[row];
        const long long base = (long long)tr * PCM_TILE;
        if (base >= d.n) continue;                                  // (the same for the whole workgroup)
        const long long left = d.n - base;
        const float* s = src + d.src_off + base;
        short* o = dst + d.dst_off + base;
        const bool aligned = (((uintptr_t)s | (uintptr_t)o) & 15) == 0;
        unsigned cnt = 0;
        if (aligned && i0 + PCM_PER_THREAD <= left) {
            const float4 a = *reinterpret_cast<const float4*>(s + i0), b = *reinterpret_cast<const float4*>(s + i0 + 4);
            uint4 q;
            q.x = pack2(pcm_quant(a.x, d.scale, limit, cnt), pcm_quant(a.y, d.scale, limit, cnt));
            q.y = pack2(pcm_quant(a.z, d.scale, limit, cnt), pcm_quant(a.w, d.scale, limit, cnt));
            q.z = pack2(pcm_quant(b.x, d.scale, limit, cnt), pcm_quant(b.y, d.scale, limit, cnt));
            q.w = pack2(pcm_quant(b.z, d.scale, limit, cnt), pcm_quant(b.w, d.scale, limit, cnt));
            *reinterpret_cast<uint4*>(o + i0) = q;
        } else {
            for (int e = 0; e < PCM_PER_THREAD; ++e)
                if (i0 + e < left) o[i0 + e] = (short)pcm_quant(s[i0 + e], d.scale, limit, cnt);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off);
        const unsigned mine = lane == 0 ? (cnt & 0xffffu) : (cnt >> 16);
        if (lane < 2 && mine != 0) atomicAdd(counts + 2 * (size_t)row + lane, mine);
    }
}

__global__ __launch_bounds__(256) void pcm_peaks_kernel(const float* __restrict__ src, const PcmRow* __restrict__ rows, unsigned tiles_per_row, unsigned total_tiles,
                                                        unsigned* __restrict__ peaks) {
    const int i0 = (int)threadIdx.x * PCM_PER_THREAD, lane = (int)threadIdx.x & 63;
    for (unsigned tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
        const unsigned row = tile / tiles_per_row, tr = tile - row * tiles_per_row;
        const PcmRow d = rows[row];
        const long long base = (long long)tr * PCM_TILE;
        if (base >= d.n) continue;
        const long long left = d.n - base;
        const float* s = src + d.src_off + base;
        float v[PCM_PER_THREAD];
        if ((((uintptr_t)s) & 15) == 0 && i0 + PCM_PER_THREAD <= left) {
            const float4 a = *reinterpret_cast<const float4*>(s + i0), b = *reinterpret_cast<const float4*>(s + i0 + 4);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else {
#pragma unroll
            for (int e = 0; e < PCM_PER_THREAD; ++e) v[e] = i0 + e < left ? s[i0 + e] : 0.0f;
        }
        float m = 0.0f;
#pragma unroll
        for (int e = 0; e < PCM_PER_THREAD; ++e) {
            const float ax = fabsf(v[e]);
            m = fmaxf(m, ax < INFINITY ? ax : 0.0f);                 // (a NaN compares false: neither it nor an infinity takes part)
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
        if (lane == 0 && m > 0.0f) atomicMax(peaks + row, __float_as_uint(m));
    }
}

// tiles of a launch over `nrows` rows of at most `max_n` samples; 0 = too many for the 32-bit tile index
inline unsigned pcm_tiles(int nrows, long long max_n, unsigned* per_row) {
    const unsigned long long tpr = ((unsigned long long)max_n + PCM_TILE - 1) / PCM_TILE;
    const unsigned long long total = tpr * (unsigned long long)nrows;
    if (tpr == 0 || total >= (1ull << 31)) return 0;
    *per_row = (unsigned)tpr;
    return (unsigned)total;
}
inline unsigned pcm_grid(unsigned total) {
    const unsigned cap = 8u * (unsigned)device_cus();
    return total < cap ? total : cap;
}

}  // namespace at

extern "C" {

static_assert(sizeof(at_pcm_row_desc) == sizeof(at::PcmRow), "at_pcm_row_desc layout");

int at_pcm_peaks(const float* src, const at_pcm_row_desc* rows_dev, int nrows, int64_t max_n, float* peaks, at_stream_t stream) {
    using namespace at;
    AT_REQUIRE(src && rows_dev && peaks && nrows >= 0 && max_n >= 0, "at_pcm_peaks: bad arguments");
    if (nrows == 0) return 0;
    unsigned per_row = 0;
    const unsigned total = max_n > 0 ? pcm_tiles(nrows, max_n, &per_row) : 0;
    AT_REQUIRE(max_n == 0 || total > 0, "at_pcm_peaks: nrows x max_n is beyond 2^31 tiles of 2048 samples");
    AT_CHECK_HIP(hipMemsetAsync(peaks, 0, sizeof(float) * (size_t)nrows, (hipStream_t)stream));
    if (total == 0) return 0;
    hipLaunchKernelGGL(pcm_peaks_kernel, dim3(pcm_grid(total)), dim3(256), 0, (hipStream_t)stream, src, reinterpret_cast<const PcmRow*>(rows_dev), per_row, total,
                       reinterpret_cast<unsigned*>(peaks));
    AT_CHECK_HIP(hipGetLastError());
    return 0;
}

int at_pcm_pack(const float* src, const at_pcm_row_desc* rows_dev, int nrows, int64_t max_n, float limit, int16_t* dst, uint32_t* counts, at_stream_t stream) {
    using namespace at;
    AT_REQUIRE(src && rows_dev && dst && counts && nrows >= 0 && max_n >= 0, "at_pcm_pack: bad arguments");
    AT_REQUIRE(limit > 0.0f && limit <= 32767.0f / 32768.0f, "at_pcm_pack: limit must lie in (0, 32767 / 32768]");
    if (nrows == 0) return 0;
    unsigned per_row = 0;
    const unsigned total = max_n > 0 ? pcm_tiles(nrows, max_n, &per_row) : 0;
    AT_REQUIRE(max_n == 0 || total > 0, "at_pcm_pack: nrows x max_n is beyond 2^31 tiles of 2048 samples");
    AT_CHECK_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t) * (size_t)nrows, (hipStream_t)stream));
    if (total == 0) return 0;
    hipLaunchKernelGGL(pcm_pack_kernel, dim3(pcm_grid(total)), dim3(256), 0, (hipStream_t)stream, src, reinterpret_cast<const PcmRow*>(rows_dev), per_row, total, limit,
                       reinterpret_cast<short*>(dst), counts);
    AT_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
