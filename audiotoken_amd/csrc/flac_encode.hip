// FLAC output of decode_batch_files / save_audio (RFC 9639): the decoder's padded float32 batch -> FLAC subframes, compacted back to back, so
// that ONE device-to-host copy per batch carries the COMPRESSED samples; the host adds what needs no samples (frame headers, CRC-8 / CRC-16, STREAMINFO).
// The sample value is pcm_quant of the PCM writer (pcm_quant.h): the two formats cannot disagree about a sample.
//
// The encoding rule (every decision is integer arithmetic, so the kernel, the host twin below and tests/flac_enc_ref.py produce IDENTICAL bytes):
//   stream    mono, 16 bit, variable block size; every row is cut into blocks of 4096 samples plus one shorter last block; one subframe per frame
//   subframe  8-bit header, no wasted bits. CONSTANT when all n samples are equal; otherwise VERBATIM when n <= 32; otherwise FIXED orders o = 0..4 compete:
//             residual r in int32, folded u = (r << 1) ^ (r >> 31); partitioned Rice method 0 (4-bit parameters, no escapes), partition orders p = 0..pmax with
//             pmax the largest p <= 6 such that n % 2^p == 0 and (n >> p) >= 32; a partition of cnt residuals costs 4 + min over k = 0..14 of
//             cnt (k + 1) + sum(u >> k), ties to the smaller k (partition 0 holds (n >> p) - o residuals); bits(o, p) = 8 + 16 o + 6 + sum of its partitions;
//             the smallest wins, ties to the smaller o, then the smaller p; when that is >= 8 + 16 n the subframe is VERBATIM.
//
// Device shape: one 256-thread workgroup per block, grid-stride over the blocks, at most 8 workgroups per CU (as the PCM kernel). The samples are quantised
// once into LDS; every thread then owns 16 CONSECUTIVE samples plus the 4 before them in registers, so the five residual orders are four in-place
// differencing passes. Per order the 15 sums of (u >> k) are accumulated per FINEST partition (n >> pmax >= 32 samples, so a thread touches at most two);
// wave 0 then holds one finest partition per lane and walks the partition orders upwards by adding children with shuffles: the (o, p, k[]) choice is
// workgroup-uniform. Code lengths go through an exclusive scan to bit offsets; codes are ORed into a zeroed big-endian LDS bit buffer, which is written to the
// block's slot of the caller's workspace. A one-workgroup scan over the blocks' byte counts and a compaction copy follow.
#include "at_common.h"
#include "../../include/audiotoken_hip.h"
#include "pcm_quant.h"

#include <cstring>
#include <vector>

namespace at {

// mirrors `at_flac_row_desc` (include/audiotoken_hip.h)
struct FlacRow {
    long long src_off;   // first sample of the row, in floats from `src`
    long long n;         // samples of the row
    int first_block;     // index of the row's first block among the launch's blocks (rows in order, ceil(n / 4096) blocks each)
    float scale;         // multiplies every finite sample before the clamp
};
// mirrors `at_flac_block`
struct FlacBlock {
    long long first;     // first sample of the block inside its row
    long long byte_off;  // of the subframe in the compacted bytes: the exclusive prefix sum of nbytes in record order
    int row, n, kind, order, porder, nbytes;
};

constexpr int FLAC_BLOCK = AT_FLAC_BLOCK;
constexpr int FLAC_PER_THREAD = 16;                       // 256 threads x 16 consecutive samples = one block
constexpr int FLAC_SLOT = 8208;                           // bytes of workspace per block: the worst case 1 + 2 * 4096, rounded up to 16
constexpr int FLAC_WORDS = FLAC_SLOT / 4;
constexpr int FLAC_MAX_K = 14;
constexpr unsigned FLAC_SUM_CLAMP = 1u << 20;
static_assert(FLAC_BLOCK == 256 * FLAC_PER_THREAD && 1 + 2 * FLAC_BLOCK <= FLAC_SLOT && FLAC_SLOT % 16 == 0, "block geometry");

__host__ __device__ inline int flac_pmax(int n) {
    int p = 0;
    while (p < 6 && (n % (2 << p)) == 0 && (n >> (p + 1)) >= 32) ++p;
    return p;
}
__host__ __device__ inline unsigned flac_fold(int r) { return ((unsigned)r << 1) ^ (unsigned)(r >> 31); }

// FLAC is MSB-first: bit b of the subframe is bit 31 - (b & 31) of big-endian word b >> 5. `v` (< 2^len, 1 <= len <= 32) may straddle two words, so it is
// shifted inside 64 bits and both halves are ORed (vector LDS instructions) into the ZEROED buffer; a unary run of zeros needs no write at all, only its
// stop bit does. The word bound keeps a wrong length (there is none: the chosen encoding is below 8 + 16 n bits) inside the buffer.
__device__ __forceinline__ void flac_put(unsigned* buf, unsigned bit, unsigned v, int len) {
    const unsigned w = bit >> 5, sh = bit & 31;
    const unsigned long long x = (unsigned long long)v << (64 - (int)sh - len);
    const unsigned hi = (unsigned)(x >> 32), lo = (unsigned)x;
    if (hi != 0 && w < (unsigned)FLAC_WORDS) atomicOr(buf + w, hi);
    if (lo != 0 && w + 1 < (unsigned)FLAC_WORDS) atomicOr(buf + w + 1, lo);
}

__global__ __launch_bounds__(256) void flac_encode_kernel(const float* __restrict__ src, const FlacRow* __restrict__ rows, int nrows, int nblocks, float limit,
                                                          FlacBlock* __restrict__ blocks, unsigned char* __restrict__ slots, unsigned* __restrict__ counts) {
    __shared__ int s_smp[FLAC_BLOCK + 4];        // s_smp[4 + i] = sample i; s_smp[0..3] = 0: the four "samples before the block" of thread 0's window
    __shared__ unsigned s_bits[FLAC_WORDS];      // the subframe, big-endian words
    __shared__ unsigned s_psum[64 * 16];         // [finest partition][k]: sum(u >> k) of the order at hand
    __shared__ int s_kparam[64];                 // Rice parameters of the best (o, p) so far
    __shared__ unsigned s_wave[4];
    __shared__ int s_choice[4];                  // bits, order, partition order of the best FIXED candidate; [3] = "the samples differ"
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, i0 = tid * FLAC_PER_THREAD;

    for (int blk = (int)blockIdx.x; blk < nblocks; blk += (int)gridDim.x) {
        // the block's row: the LAST row whose first_block <= blk (a row without samples has no block and shares its first_block with the row after it)
        int lo = 0, hi = nrows - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (rows[mid].first_block <= blk) lo = mid; else hi = mid - 1;
        }
        const FlacRow d = rows[lo];
        const long long first = (long long)(blk - d.first_block) * FLAC_BLOCK;
        const long long left = d.n - first;
        const int n = (first < 0 || left <= 0) ? 0 : (left < FLAC_BLOCK ? (int)left : FLAC_BLOCK);   // (0: descriptors that do not add up; nothing is read)
        if (n == 0) {                                                    // (the same for the whole workgroup)
            if (tid == 0) blocks[blk] = FlacBlock{first, 0, lo, 0, AT_FLAC_VERBATIM, 0, 0, 0};
            continue;
        }
        // ---- quantise once into LDS (coalesced: sample tid + 256 e), count as at_pcm_pack does ----
        const float* sp = src + d.src_off + first;
        unsigned cnt = 0;
#pragma unroll
        for (int e = 0; e < FLAC_PER_THREAD; ++e) {
            const int i = tid + 256 * e;
            if (i < n) s_smp[4 + i] = pcm_quant(sp[i], d.scale, limit, cnt);
        }
        if (tid < 4) s_smp[tid] = 0;
        for (int w = tid; w < FLAC_WORDS; w += 256) s_bits[w] = 0;
        if (tid == 0) s_choice[3] = 0;
        // (16 samples per thread: the packed halves hold at most 1024 per wave)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off);
        const unsigned mine = lane == 0 ? (cnt & 0xffffu) : (cnt >> 16);
        if (lane < 2 && mine != 0) atomicAdd(counts + 2 * (size_t)lo + lane, mine);
        __syncthreads();

        // ---- the thread's window: win[w] = sample i0 - 4 + w (0 before the block and past its end) ----
        int win[FLAC_PER_THREAD + 4];
#pragma unroll
        for (int w = 0; w < FLAC_PER_THREAD + 4; ++w) win[w] = (i0 + w < n + 4) ? s_smp[i0 + w] : 0;
        const int s0 = s_smp[4];
        bool differs = false;
#pragma unroll
        for (int e = 0; e < FLAC_PER_THREAD; ++e) differs |= (i0 + e < n) && win[4 + e] != s0;
        if (differs) s_choice[3] = 1;
        __syncthreads();
        const bool constant = s_choice[3] == 0;

        int kind = constant ? AT_FLAC_CONSTANT : AT_FLAC_VERBATIM, order = 0, porder = 0, bits = constant ? 24 : 8 + 16 * n;
        if (!constant && n > 32) {
            // ---- the FIXED candidates ----
            // The last block's n changes pmax (n = 64: 1; n = 1408 = 64 * 22: 5; n odd: 0), and the finest partition's length L = n >> pmax is no multiple of
            // the 16 samples of a thread: a thread's samples lie in partition pa and, from sample `boundary` on, in pa + 1 (L >= 32 > 16: never a third).
            const int pmax = flac_pmax(n), J = 1 << pmax, L = n >> pmax;
            const int pa = i0 / L, boundary = (pa + 1) * L;
            const int wfirst = 1024 * wave, wlast = wfirst + 1023 < n ? wfirst + 1023 : n - 1;
            const bool wave_uniform = wfirst < n && wfirst / L == wlast / L;     // the whole wave lies in one finest partition: reduce in registers
            int best_bits = 0x7fffffff, best_o = 0, best_p = 0;                  // (wave 0)
            int dw[FLAC_PER_THREAD + 4];
#pragma unroll
            for (int w = 0; w < FLAC_PER_THREAD + 4; ++w) dw[w] = win[w];
#pragma unroll 1
            for (int o = 0; o <= 4; ++o) {
                for (int j = tid; j < 64 * 16; j += 256) s_psum[j] = 0;
                __syncthreads();
                unsigned u[FLAC_PER_THREAD];
#pragma unroll
                for (int e = 0; e < FLAC_PER_THREAD; ++e) u[e] = (i0 + e >= o && i0 + e < n) ? flac_fold(dw[4 + e]) : 0u;   // the o warm-up samples have no residual
                const bool straddles = boundary < i0 + FLAC_PER_THREAD && boundary < n;
                // sum(u >> 0) over 4096 samples reaches 2^33. A thread's partial sum (16 samples, u < 2^21: below 2^25) is clamped to 2^20 instead of widening
                // every sum to 64 bits: a partition's k = 14 never costs more than 143 bits per sample (<= 585 728 < 2^20 for 4096 samples), so a sum that holds
                // a clamped part is >= 2^20 in every partition that contains it and cannot be a minimum, while every sum that can be one is exact; 512
                // clamped parts stay below 2^30. The choice is the one of exact arithmetic.
#pragma unroll
                for (int k = 0; k <= FLAC_MAX_K; ++k) {
                    unsigned tot = 0, sb = 0;
#pragma unroll
                    for (int e = 0; e < FLAC_PER_THREAD; ++e) tot += u[e] >> k;
                    if (straddles) {
#pragma unroll
                        for (int e = 0; e < FLAC_PER_THREAD; ++e) sb += (i0 + e >= boundary) ? (u[e] >> k) : 0u;
                    }
                    unsigned a = tot - sb;
                    a = a < FLAC_SUM_CLAMP ? a : FLAC_SUM_CLAMP;
                    sb = sb < FLAC_SUM_CLAMP ? sb : FLAC_SUM_CLAMP;
                    if (wave_uniform) {
#pragma unroll
                        for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off);
                        if (lane == 0 && a != 0) atomicAdd(&s_psum[(wfirst / L) * 16 + k], a);
                    } else if (i0 < n) {
                        if (a != 0) atomicAdd(&s_psum[pa * 16 + k], a);
                        if (sb != 0) atomicAdd(&s_psum[(pa + 1) * 16 + k], sb);     // (sb != 0 only when boundary < n: pa + 1 < J)
                    }
                }
                __syncthreads();
                unsigned sums[FLAC_MAX_K + 1];
                if (wave == 0) {
#pragma unroll
                    for (int k = 0; k <= FLAC_MAX_K; ++k) sums[k] = lane < J ? s_psum[lane * 16 + k] : 0u;
                }
                __syncthreads();                                          // s_psum is free for the next order
                if (wave == 0) {
                    // lane j = finest partition j; at partition order p the lanes j % step == 0 (step = 2^(pmax - p)) hold partition j / step, the sum of its children
                    for (int p = pmax; p >= 0; --p) {
                        const int step = 1 << (pmax - p);
                        const bool active = lane < J && (lane & (step - 1)) == 0;
                        const unsigned pcnt = (unsigned)((n >> p) - (lane == 0 ? o : 0));   // partition 0 excludes the warm-up samples
                        unsigned best = 0xffffffffu;
                        int bk = 0;
#pragma unroll
                        for (int k = 0; k <= FLAC_MAX_K; ++k) {
                            const unsigned c = pcnt * (unsigned)(k + 1) + sums[k];
                            if (c < best) { best = c; bk = k; }           // ties to the smaller k
                        }
                        unsigned total = active ? 4u + best : 0u;
#pragma unroll
                        for (int off = 32; off >= 1; off >>= 1) total += __shfl_xor(total, off);
                        const int cand = 8 + 16 * o + 6 + (int)total;
                        if (cand < best_bits || (cand == best_bits && o == best_o)) {   // ties: the smaller o (visited first), then the smaller p (visited last)
                            best_bits = cand; best_o = o; best_p = p;
                            if (active) s_kparam[lane >> (pmax - p)] = bk;
                        }
                        if (p > 0) {
#pragma unroll
                            for (int k = 0; k <= FLAC_MAX_K; ++k) sums[k] += __shfl_down(sums[k], step);
                        }
                    }
                }
#pragma unroll
                for (int w = FLAC_PER_THREAD + 3; w >= 1; --w) dw[w] -= dw[w - 1];   // order o -> o + 1 (|r| <= 2^19 at order 4)
            }
            if (tid == 0) { s_choice[0] = best_bits; s_choice[1] = best_o; s_choice[2] = best_p; }
            __syncthreads();
            if (s_choice[0] < 8 + 16 * n) { kind = AT_FLAC_FIXED; bits = s_choice[0]; order = s_choice[1]; porder = s_choice[2]; }
        }

        // ---- write the subframe into the zeroed bit buffer ----
        if (kind == AT_FLAC_CONSTANT) {
            if (tid == 0) flac_put(s_bits, 8, (unsigned)s0 & 0xffffu, 16);       // (the header byte of CONSTANT is 0)
        } else if (kind == AT_FLAC_VERBATIM) {
            if (tid == 0) flac_put(s_bits, 0, 0x02u, 8);
#pragma unroll
            for (int e = 0; e < FLAC_PER_THREAD; ++e)
                if (i0 + e < n) flac_put(s_bits, 8u + 16u * (unsigned)(i0 + e), (unsigned)win[4 + e] & 0xffffu, 16);
        } else {
            int dw[FLAC_PER_THREAD + 4];
#pragma unroll
            for (int w = 0; w < FLAC_PER_THREAD + 4; ++w) dw[w] = win[w];
            for (int o = 0; o < order; ++o) {
#pragma unroll
                for (int w = FLAC_PER_THREAD + 3; w >= 1; --w) dw[w] -= dw[w - 1];
            }
            const int Lp = n >> porder, ja = i0 / Lp, bnd = (ja + 1) * Lp;
            const int ka = i0 < n ? s_kparam[ja] : 0, kb = (bnd < n && bnd < i0 + FLAC_PER_THREAD) ? s_kparam[ja + 1] : 0;
            // code length per sample: (u >> k) zeros, the stop bit, k low bits; the partition's 4-bit parameter goes in front of its first residual
            unsigned mylen = 0;
#pragma unroll
            for (int e = 0; e < FLAC_PER_THREAD; ++e) {
                const int i = i0 + e;
                if (i >= order && i < n) {
                    const bool inb = i >= bnd;
                    const int k = inb ? kb : ka;
                    const bool head = inb ? i == bnd : (ja == 0 ? i == order : i == ja * Lp);
                    mylen += (flac_fold(dw[4 + e]) >> k) + 1u + (unsigned)k + (head ? 4u : 0u);
                }
            }
            unsigned incl = mylen;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned t = __shfl_up(incl, off);
                if (lane >= off) incl += t;
            }
            if (lane == 63) s_wave[wave] = incl;
            __syncthreads();
            unsigned pos = 8u + 16u * (unsigned)order + 6u + (incl - mylen);
            for (int w = 0; w < wave; ++w) pos += s_wave[w];
#pragma unroll
            for (int e = 0; e < FLAC_PER_THREAD; ++e) {
                const int i = i0 + e;
                if (i >= order && i < n) {
                    const bool inb = i >= bnd;
                    const int k = inb ? kb : ka;
                    const bool head = inb ? i == bnd : (ja == 0 ? i == order : i == ja * Lp);
                    if (head) { flac_put(s_bits, pos, (unsigned)k, 4); pos += 4; }
                    const unsigned uu = flac_fold(dw[4 + e]), q = uu >> k;
                    flac_put(s_bits, pos + q, (1u << k) | (uu & ((1u << k) - 1u)), k + 1);
                    pos += q + 1u + (unsigned)k;
                }
            }
            if (tid == 0) {
                flac_put(s_bits, 0, (unsigned)(8 | order) << 1, 8);
                for (int i = 0; i < order; ++i) flac_put(s_bits, 8u + 16u * (unsigned)i, (unsigned)s_smp[4 + i] & 0xffffu, 16);
                if (porder != 0) flac_put(s_bits, 8u + 16u * (unsigned)order, (unsigned)porder, 6);   // 2 bits of method 0, 4 bits of partition order
            }
        }
        __syncthreads();
        const int nbytes = (bits + 7) >> 3;                               // (the padding to a byte is the buffer's zeros)
        unsigned* slot = reinterpret_cast<unsigned*>(slots + (size_t)blk * FLAC_SLOT);
        for (int w = tid; w < (nbytes + 3) >> 2; w += 256) slot[w] = __builtin_bswap32(s_bits[w]);
        if (tid == 0) blocks[blk] = FlacBlock{first, 0, lo, n, kind, order, porder, nbytes};
        __syncthreads();                                                  // the next block overwrites the LDS
    }
}

// byte_off = the exclusive prefix sum of nbytes: one workgroup, a contiguous run of records per thread
__global__ __launch_bounds__(256) void flac_scan_kernel(FlacBlock* __restrict__ blocks, int nblocks) {
    __shared__ long long part[256];
    const int tid = (int)threadIdx.x, per = (nblocks + 255) / 256;
    const int b0 = tid * per < nblocks ? tid * per : nblocks, b1 = b0 + per < nblocks ? b0 + per : nblocks;
    long long s = 0;
    for (int b = b0; b < b1; ++b) s += blocks[b].nbytes;
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        long long run = 0;
        for (int i = 0; i < 256; ++i) { const long long t = part[i]; part[i] = run; run += t; }
    }
    __syncthreads();
    long long run = part[tid];
    for (int b = b0; b < b1; ++b) { blocks[b].byte_off = run; run += blocks[b].nbytes; }
}

// the slots' subframes back to back; a subframe that would pass `cap` is not copied (the caller sizes `bytes` by the worst case, so there is none)
__global__ __launch_bounds__(256) void flac_compact_kernel(const FlacBlock* __restrict__ blocks, int nblocks, const unsigned char* __restrict__ slots,
                                                           unsigned char* __restrict__ out, long long cap) {
    for (int blk = (int)blockIdx.x; blk < nblocks; blk += (int)gridDim.x) {
        const long long off = blocks[blk].byte_off;
        const int nb = blocks[blk].nbytes;
        if (nb <= 0 || nb > FLAC_SLOT || off < 0 || off + nb > cap) continue;
        const unsigned char* s = slots + (size_t)blk * FLAC_SLOT;
        for (int i = (int)threadIdx.x; i < nb; i += 256) out[off + i] = s[i];
    }
}

// ---- host: MSB-first bit writer, the twin of the rule, framing ---------------------------------------------------------------------------------------------------
struct BitWriter {
    uint8_t* p;
    int64_t bits = 0;
    explicit BitWriter(uint8_t* out) : p(out) {}
    void put(uint32_t v, int len) {                                       // the caller zeroed the output
        for (int b = len - 1; b >= 0; --b, ++bits)
            if ((v >> b) & 1u) p[bits >> 3] |= (uint8_t)(0x80u >> (bits & 7));
    }
};

// one block from int16 samples by the rule, in exact 64-bit arithmetic; `out` holds 1 + 2 n zeroed bytes; returns the subframe's bytes
static int flac_encode_block_host(const int16_t* s, int n, uint8_t* out, int* kind_out, int* order_out, int* porder_out) {
    std::memset(out, 0, (size_t)(1 + 2 * n));
    BitWriter bw(out);
    *order_out = *porder_out = 0;
    bool constant = true;
    for (int i = 1; i < n; ++i) constant = constant && s[i] == s[0];
    if (constant) {
        *kind_out = AT_FLAC_CONSTANT;
        bw.put(0, 8);
        bw.put((uint16_t)s[0], 16);
        return 3;
    }
    auto verbatim = [&]() {
        *kind_out = AT_FLAC_VERBATIM;
        bw.put(0x02, 8);
        for (int i = 0; i < n; ++i) bw.put((uint16_t)s[i], 16);
        return 1 + 2 * n;
    };
    if (n <= 32) return verbatim();
    const int pmax = flac_pmax(n), J = 1 << pmax;
    std::vector<int32_t> r(s, s + n), best_r;
    std::vector<int64_t> fin((size_t)J * 15), cur;
    std::vector<int> ks, best_k;
    int64_t best_bits = INT64_MAX;
    int best_o = 0, best_p = 0;
    for (int o = 0; o <= 4; ++o) {
        if (o > 0) for (int i = n - 1; i >= o; --i) r[i] -= r[i - 1];   // r[i], i >= o: the order-o residual
        const int L = n >> pmax;
        std::fill(fin.begin(), fin.end(), 0);
        for (int i = o; i < n; ++i) {
            const uint32_t u = flac_fold(r[i]);
            int64_t* f = &fin[(size_t)(i / L) * 15];
            for (int k = 0; k <= FLAC_MAX_K; ++k) f[k] += u >> k;
        }
        cur = fin;
        for (int p = pmax; p >= 0; --p) {
            const int parts = 1 << p;
            int64_t total = 8 + 16 * o + 6;
            ks.assign(parts, 0);
            for (int j = 0; j < parts; ++j) {
                const int64_t cnt = (n >> p) - (j == 0 ? o : 0);
                int64_t bestc = INT64_MAX;
                for (int k = 0; k <= FLAC_MAX_K; ++k) {
                    const int64_t c = cnt * (k + 1) + cur[(size_t)j * 15 + k];
                    if (c < bestc) { bestc = c; ks[j] = k; }
                }
                total += 4 + bestc;
            }
            if (total < best_bits || (total == best_bits && o == best_o)) { best_bits = total; best_o = o; best_p = p; best_k = ks; best_r = r; }
            for (int j = 0; j < parts / 2; ++j)
                for (int k = 0; k <= FLAC_MAX_K; ++k) cur[(size_t)j * 15 + k] = cur[(size_t)(2 * j) * 15 + k] + cur[(size_t)(2 * j + 1) * 15 + k];
        }
    }
    if (best_bits >= 8 + 16 * (int64_t)n) return verbatim();
    *kind_out = AT_FLAC_FIXED; *order_out = best_o; *porder_out = best_p;
    bw.put((uint32_t)(8 | best_o) << 1, 8);
    for (int i = 0; i < best_o; ++i) bw.put((uint16_t)s[i], 16);
    bw.put((uint32_t)best_p, 6);
    const int Lp = n >> best_p;
    for (int j = 0; j < (1 << best_p); ++j) {
        const int k = best_k[j];
        bw.put((uint32_t)k, 4);
        for (int i = j == 0 ? best_o : j * Lp; i < (j + 1) * Lp; ++i) {
            const uint32_t u = flac_fold(best_r[i]);
            bw.bits += u >> k;                                            // the unary run: zeros are already there
            bw.put((1u << k) | (u & ((1u << k) - 1u)), k + 1);
        }
    }
    return (int)((bw.bits + 7) >> 3);
}

static uint8_t flac_crc8(const uint8_t* d, size_t n) {
    uint8_t c = 0;
    for (size_t i = 0; i < n; ++i) {
        c ^= d[i];
        for (int b = 0; b < 8; ++b) c = (uint8_t)((c & 0x80) ? ((c << 1) ^ 0x07) : (c << 1));
    }
    return c;
}
struct FlacCrc16Table {
    uint16_t t[256];
    FlacCrc16Table() {
        for (int i = 0; i < 256; ++i) {
            uint16_t c = (uint16_t)(i << 8);
            for (int b = 0; b < 8; ++b) c = (uint16_t)((c & 0x8000) ? ((c << 1) ^ 0x8005) : (c << 1));
            t[i] = c;
        }
    }
};
static uint16_t flac_crc16(const uint8_t* d, size_t n, uint16_t c) {
    static const FlacCrc16Table tab;
    for (size_t i = 0; i < n; ++i) c = (uint16_t)((c << 8) ^ tab.t[((c >> 8) ^ d[i]) & 0xff]);
    return c;
}
static int flac_rate_code(int sr) {
    static const int table[12] = {0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
    for (int c = 1; c < 12; ++c) if (table[c] == sr) return c;
    return 0;                                                             // "take it from STREAMINFO"
}

inline unsigned flac_grid(unsigned total) {
    const unsigned cap = 8u * (unsigned)device_cus();
    return total < cap ? total : cap;
}

}  // namespace at

extern "C" {

static_assert(sizeof(at_flac_row_desc) == sizeof(at::FlacRow) && sizeof(at_flac_row_desc) == 24, "at_flac_row_desc layout");
static_assert(sizeof(at_flac_block) == sizeof(at::FlacBlock) && sizeof(at_flac_block) == 40, "at_flac_block layout");

size_t at_flac_encode_workspace_bytes(int nblocks) { return nblocks > 0 ? (size_t)nblocks * at::FLAC_SLOT : 0; }

int at_flac_encode_rows(const float* src, const at_flac_row_desc* rows_dev, int nrows, int nblocks, float limit, at_flac_block* blocks, uint8_t* bytes,
                        int64_t bytes_cap, uint32_t* counts, void* workspace, size_t workspace_bytes, at_stream_t stream) {
    using namespace at;
    AT_REQUIRE(src && rows_dev && blocks && bytes && counts && nrows >= 0 && nblocks >= 0 && bytes_cap >= 0, "at_flac_encode_rows: bad arguments");
    AT_REQUIRE(limit > 0.0f && limit <= 32767.0f / 32768.0f, "at_flac_encode_rows: limit must lie in (0, 32767 / 32768]");
    AT_REQUIRE(nrows > 0 || nblocks == 0, "at_flac_encode_rows: blocks without rows");
    AT_REQUIRE(nblocks == 0 || (workspace && workspace_bytes >= at_flac_encode_workspace_bytes(nblocks)),
               "at_flac_encode_rows: workspace smaller than at_flac_encode_workspace_bytes(nblocks)");
    AT_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)blocks & 7) == 0, "at_flac_encode_rows: workspace must be 16-byte aligned, blocks 8-byte aligned");
    if (nrows == 0) return 0;
    AT_CHECK_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t) * (size_t)nrows, (hipStream_t)stream));
    if (nblocks == 0) return 0;
    FlacBlock* recs = reinterpret_cast<FlacBlock*>(blocks);
    hipLaunchKernelGGL(flac_encode_kernel, dim3(flac_grid((unsigned)nblocks)), dim3(256), 0, (hipStream_t)stream, src, reinterpret_cast<const FlacRow*>(rows_dev), nrows,
                       nblocks, limit, recs, reinterpret_cast<unsigned char*>(workspace), counts);
    AT_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(flac_scan_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, recs, nblocks);
    AT_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(flac_compact_kernel, dim3(flac_grid((unsigned)nblocks)), dim3(256), 0, (hipStream_t)stream, recs, nblocks,
                       reinterpret_cast<const unsigned char*>(workspace), reinterpret_cast<unsigned char*>(bytes), (long long)bytes_cap);
    AT_CHECK_HIP(hipGetLastError());
    return 0;
}

int64_t at_flac_encode_pcm16(const int16_t* samples, int64_t n, int row, at_flac_block* blocks, int64_t blocks_cap, uint8_t* bytes, int64_t bytes_cap,
                             int64_t byte_off) {
    using namespace at;
    AT_REQUIRE(n >= 0 && (samples || n == 0) && blocks && bytes && row >= 0 && blocks_cap >= 0 && byte_off >= 0, "at_flac_encode_pcm16: bad arguments");
    const int64_t nb = (n + FLAC_BLOCK - 1) / FLAC_BLOCK;
    AT_REQUIRE(nb <= blocks_cap, "at_flac_encode_pcm16: more blocks than blocks_cap");
    AT_REQUIRE(byte_off + nb + 2 * n <= bytes_cap, "at_flac_encode_pcm16: bytes_cap below the worst case byte_off + blocks + 2 n");
    for (int64_t b = 0; b < nb; ++b) {
        const int64_t first = b * FLAC_BLOCK;
        const int bn = (int)(n - first < FLAC_BLOCK ? n - first : FLAC_BLOCK);
        int kind = 0, order = 0, porder = 0;
        const int nbytes = flac_encode_block_host(samples + first, bn, bytes + byte_off, &kind, &order, &porder);
        blocks[b] = at_flac_block{first, byte_off, row, bn, kind, order, porder, nbytes};
        byte_off += nbytes;
    }
    return nb;
}

int64_t at_flac_write_frames(const at_flac_block* blocks, int nblocks, const uint8_t* bytes, int64_t bytes_len, int sample_rate, const int64_t* first_sample_of_row,
                             int nrows, uint8_t* out, int64_t cap, int64_t* stats) {
    using namespace at;
    AT_REQUIRE(blocks && bytes && first_sample_of_row && out && stats && nblocks >= 0 && nrows >= 0 && bytes_len >= 0 && cap >= 0 && sample_rate > 0,
               "at_flac_write_frames: bad arguments");
    int64_t pos = 0, min_frame = 0, max_frame = 0, min_block = 0, max_block = 0, last_block = 0, samples = 0;
    const int rate_code = flac_rate_code(sample_rate);
    for (int b = 0; b < nblocks; ++b) {
        const at_flac_block& r = blocks[b];
        AT_REQUIRE(r.row >= 0 && r.row < nrows && r.n >= 1 && r.n <= 65536 && r.first >= 0, "at_flac_write_frames: damaged block record");
        AT_REQUIRE(r.nbytes >= 1 && r.byte_off >= 0 && r.byte_off + r.nbytes <= bytes_len, "at_flac_write_frames: a record points outside the subframe bytes");
        const int64_t number = first_sample_of_row[r.row] + r.first;
        AT_REQUIRE(first_sample_of_row[r.row] >= 0 && number + r.n <= (1ll << 36) - 1, "at_flac_write_frames: past FLAC's 2^36 - 1 samples");
        AT_REQUIRE(pos + 16 + r.nbytes + 2 <= cap, "at_flac_write_frames: output buffer too small (16 + nbytes + 2 bytes per frame)");
        uint8_t* f = out + pos;
        int h = 0;
        f[h++] = 0xff;
        f[h++] = 0xf9;                                                    // sync, reserved 0, blocking strategy 1: variable block size
        const int bs_code = r.n == 4096 ? 12 : (r.n <= 256 ? 6 : 7);
        f[h++] = (uint8_t)((bs_code << 4) | rate_code);
        f[h++] = 0x08;                                                    // channel code 0 (mono), sample-size code 4 (16 bit), reserved 0
        // the first sample's index as the UTF-8-like number (up to 36 bits: 7 bytes)
        const uint64_t v = (uint64_t)number;
        if (v < 0x80) f[h++] = (uint8_t)v;
        else {
            int extra = v < 0x800 ? 1 : v < 0x10000 ? 2 : v < 0x200000 ? 3 : v < 0x4000000 ? 4 : v < 0x80000000ull ? 5 : 6;
            f[h++] = (uint8_t)((0xff << (7 - extra)) | (extra == 6 ? 0 : (v >> (6 * extra))));
            for (int i = extra - 1; i >= 0; --i) f[h++] = (uint8_t)(0x80 | ((v >> (6 * i)) & 0x3f));
        }
        if (bs_code == 6) f[h++] = (uint8_t)(r.n - 1);
        else if (bs_code == 7) { f[h++] = (uint8_t)((r.n - 1) >> 8); f[h++] = (uint8_t)(r.n - 1); }
        f[h] = flac_crc8(f, (size_t)h);
        ++h;
        std::memcpy(f + h, bytes + r.byte_off, (size_t)r.nbytes);
        const int64_t body = h + r.nbytes;
        const uint16_t c = flac_crc16(f, (size_t)body, 0);
        f[body] = (uint8_t)(c >> 8);
        f[body + 1] = (uint8_t)c;
        const int64_t flen = body + 2;
        pos += flen;
        min_frame = b == 0 || flen < min_frame ? flen : min_frame;
        max_frame = flen > max_frame ? flen : max_frame;
        if (b + 1 < nblocks) min_block = min_block == 0 || r.n < min_block ? r.n : min_block;
        max_block = r.n > max_block ? r.n : max_block;
        last_block = r.n;
        samples += r.n;
    }
    stats[0] = min_frame; stats[1] = max_frame; stats[2] = min_block; stats[3] = max_block; stats[4] = last_block; stats[5] = nblocks; stats[6] = samples;
    return pos;
}

int at_flac_streaminfo(int sample_rate, int min_block, int max_block, int min_frame, int max_frame, int64_t total_samples, uint8_t* out42) {
    AT_REQUIRE(out42 != nullptr, "at_flac_streaminfo: null output");
    AT_REQUIRE(sample_rate > 0 && sample_rate < (1 << 20), "at_flac_streaminfo: the sample rate field has 20 bits");
    AT_REQUIRE(min_block >= 0 && max_block >= min_block && max_block <= 65535, "at_flac_streaminfo: block sizes must lie in [0, 65535]");
    AT_REQUIRE(min_frame >= 0 && max_frame >= min_frame && max_frame < (1 << 24), "at_flac_streaminfo: frame sizes have 24 bits");
    AT_REQUIRE(total_samples >= 0 && total_samples <= (1ll << 36) - 1, "at_flac_streaminfo: FLAC's limit is 2^36 - 1 samples");
    uint8_t* o = out42;
    std::memset(o, 0, 42);                                                // (the MD5 stays zero: not computed)
    std::memcpy(o, "fLaC", 4);
    o[4] = 0x80;                                                          // last metadata block, type 0 = STREAMINFO
    o[7] = 34;
    uint8_t* s = o + 8;
    s[0] = (uint8_t)(min_block >> 8); s[1] = (uint8_t)min_block;
    s[2] = (uint8_t)(max_block >> 8); s[3] = (uint8_t)max_block;
    s[4] = (uint8_t)(min_frame >> 16); s[5] = (uint8_t)(min_frame >> 8); s[6] = (uint8_t)min_frame;
    s[7] = (uint8_t)(max_frame >> 16); s[8] = (uint8_t)(max_frame >> 8); s[9] = (uint8_t)max_frame;
    s[10] = (uint8_t)(sample_rate >> 12); s[11] = (uint8_t)(sample_rate >> 4);
    s[12] = (uint8_t)(((sample_rate & 15) << 4) | (0 << 1) | 0);          // channels - 1 = 0; bits - 1 = 15 = 0b01111: its top bit here
    s[13] = (uint8_t)((15 << 4) | ((total_samples >> 32) & 15));
    s[14] = (uint8_t)(total_samples >> 24); s[15] = (uint8_t)(total_samples >> 16); s[16] = (uint8_t)(total_samples >> 8); s[17] = (uint8_t)total_samples;
    return 0;
}

}  // extern "C"
