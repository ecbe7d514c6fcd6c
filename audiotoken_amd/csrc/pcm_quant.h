// The float -> 16-bit PCM rule of the output path (arithmetic stated at the top of pcm_writer.hip), shared by the PCM writer
// (pcm_writer.hip) and the FLAC encoder (flac_encode.hip): ONE function, so the two formats cannot disagree about a sample.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace at {

// cnt: clipped samples in the low half, non-finite samples in the high half (the callers quantise at most 16 samples per thread, 1024 per wave: the halves cannot carry into each other)
__device__ __forceinline__ int pcm_quant(float x, float scale, float limit, unsigned& cnt) {
    const float ax = fabsf(x);
    const bool nan = x != x, inf = ax == INFINITY;
    const float y = x * scale;
    const float c = fminf(fmaxf(y, -limit), limit);
    cnt += (nan || inf) ? 0x10000u : (c != y ? 1u : 0u);
    const float v = nan ? 0.0f : (inf ? copysignf(limit, x) : c);
    return (int)rintf(v * 32768.0f);
}

}  // namespace at
