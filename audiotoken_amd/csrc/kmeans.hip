// Device k-means (Lloyd's algorithm + greedy k-means++) for fitting the semantic tokenizers' code books.
//
// E-step: the tokenizers' own nearest-code path (the split-operand score GEMM, then vq_argmax_kernel with the code rows given, which re-evaluates near-ties
// exactly in float64), over fixed row chunks so that the score buffer is O(chunk x K).
// M-step: bitwise reproducible, no float atomics (cdna_hip_programming Guideline 12 / Appendix B "Scatter / gather"): an integer histogram of the labels per
// 4096-row tile, a stable counting-sort scatter of the row indices by label (the inverted index), then per cluster the member rows in that fixed order,
// summed in float64 by 512-row parts (one wave each) whose partials are added in part order. The same pass writes each row's exact squared distance to its
// OLD centre (float64): the inertia and the relocation of empty clusters (sklearn's _relocate_empty_clusters rule) come from it.
// k-means++: sklearn's greedy variant, n_local_trials = 2 + int(ln K), the caller's uniforms; one pass over X per centre.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/audiotoken_hip.h"
#include "at_common.h"
#include "gemm_bf16x3.h"
#include "w2vbert_kernels.h"

namespace at {
namespace {

typedef float kf4 __attribute__((ext_vector_type(4)));

constexpr int KM_TILE = 4096;        // rows per tile of the counting sort
constexpr int KM_PART = 512;         // member rows per partial sum (Appendix B: lists split into fixed chunks summed by separate waves)
constexpr int KM_PP_ROWS = 1024;     // rows per workgroup of the k-means++ distance pass
constexpr int KM_PP_SEG = 4096;      // rows per workgroup of the k-means++ scan
constexpr int KM_MAX_TRIALS = 16;
constexpr long long KM_DOTS_FLOATS = 1LL << 27;   // score buffer cap: 512 MB

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

// |c|^2 per code row (fp32, the approximate scan of vq_argmax only: its refinement is exact)
__global__ __launch_bounds__(256) void km_e2_kernel(const float* __restrict__ C, float* __restrict__ e2, int K, int D) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= K) return;
    float acc = 0.f;
    for (int c = lane; c < (D >> 2); c += 64) {
        const kf4 v = reinterpret_cast<const kf4*>(C + (long long)k * D)[c];
        acc += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) e2[k] = acc;
}

// ---- M-step --------------------------------------------------------------------------------------------------------------------------------------
// scal (int): [0] n_changed, [1] n_invalid (labels outside [0, K)), [2] n_empty, [3] parts
__global__ __launch_bounds__(256) void km_hist_kernel(const int16_t* __restrict__ labels, const int16_t* __restrict__ prev, long long N, int K,
                                                      int* __restrict__ tile_counts, int* __restrict__ scal) {
    const long long t = blockIdx.x;
    const long long r0 = t * KM_TILE, r1 = min(N, r0 + KM_TILE);
    int changed = 0, invalid = 0;
    for (long long i = r0 + threadIdx.x; i < r1; i += 256) {
        const int l = labels[i];
        if (l < 0 || l >= K) { ++invalid; continue; }
        atomicAdd(&tile_counts[t * K + l], 1);
        if (prev && prev[i] != l) ++changed;
    }
    __shared__ int red[2][4];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { changed += __shfl_xor(changed, off); invalid += __shfl_xor(invalid, off); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = changed; red[1][threadIdx.x >> 6] = invalid; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int c = red[0][0] + red[0][1] + red[0][2] + red[0][3], v = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        if (c) atomicAdd(&scal[0], c);
        if (v) atomicAdd(&scal[1], v);
    }
}

// per label: the tile counts become the exclusive prefix over tiles (in place), counts[l] the total
__global__ __launch_bounds__(256) void km_colscan_kernel(int* __restrict__ tile_counts, int ntiles, int K, int* __restrict__ counts) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= K) return;
    int run = 0;
    for (int t = 0; t < ntiles; ++t) {
        const int c = tile_counts[(long long)t * K + l];
        tile_counts[(long long)t * K + l] = run;
        run += c;
    }
    counts[l] = run;
}

// one workgroup: offsets = exclusive scan of counts, part_base = exclusive scan of ceil(count / KM_PART), the empty clusters in increasing index order
__global__ __launch_bounds__(1024) void km_scan_kernel(const int* __restrict__ counts, int K, int* __restrict__ offsets, int* __restrict__ part_base,
                                                      int* __restrict__ empty_list, int* __restrict__ scal) {
    __shared__ int s_cnt[1024], s_par[1024], s_emp[1024];
    const int per = (K + 1023) / 1024;
    const int l0 = min(K, (int)threadIdx.x * per), l1 = min(K, l0 + per);
    int c = 0, p = 0, e = 0;
    for (int l = l0; l < l1; ++l) { const int n = counts[l]; c += n; p += (n + KM_PART - 1) / KM_PART; e += n == 0; }
    s_cnt[threadIdx.x] = c; s_par[threadIdx.x] = p; s_emp[threadIdx.x] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = 0, b = 0, d = 0;
        for (int j = 0; j < 1024; ++j) {
            const int x = s_cnt[j], y = s_par[j], z = s_emp[j];
            s_cnt[j] = a; s_par[j] = b; s_emp[j] = d;
            a += x; b += y; d += z;
        }
        offsets[K] = a; part_base[K] = b; scal[2] = d; scal[3] = b;
    }
    __syncthreads();
    c = s_cnt[threadIdx.x]; p = s_par[threadIdx.x]; e = s_emp[threadIdx.x];
    for (int l = l0; l < l1; ++l) {
        const int n = counts[l];
        offsets[l] = c; part_base[l] = p;
        if (n == 0) empty_list[e++] = l;
        c += n; p += (n + KM_PART - 1) / KM_PART;
    }
}

// stable counting-sort scatter: one wave per tile walks its rows in order, 64 at a time; the running position of every label within the tile is kept in LDS
__global__ __launch_bounds__(64) void km_scatter_kernel(const int16_t* __restrict__ labels, long long N, int K, const int* __restrict__ tile_base,
                                                        const int* __restrict__ offsets, int* __restrict__ order) {
    extern __shared__ int pos[];   // [K]
    const long long t = blockIdx.x;
    const int lane = threadIdx.x;
    for (int l = lane; l < K; l += 64) pos[l] = offsets[l] + tile_base[t * K + l];
    __syncthreads();
    const long long r0 = t * KM_TILE, r1 = min(N, r0 + KM_TILE);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (long long base = r0; base < r1; base += 64) {
        const long long i = base + lane;
        int l = i < r1 ? (int)labels[i] : -1;
        if (l >= K) l = -1;
        unsigned long long pending = __ballot(l >= 0);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            const int ll = __shfl(l, leader);
            const unsigned long long mask = __ballot(l == ll);
            const int p0 = pos[ll];
            if (l == ll) order[p0 + __popcll(mask & below)] = (int)i;
            __builtin_amdgcn_wave_barrier();
            if (lane == leader) pos[ll] = p0 + __popcll(mask);
            __builtin_amdgcn_wave_barrier();
            pending &= ~mask;
        }
    }
}

// cluster of part p: the largest k with part_base[k] <= p
__device__ __forceinline__ int km_part_cluster(const int* __restrict__ part_base, int K, int p) {
    int lo = 0, hi = K - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (part_base[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// one wave per part: float64 sums of its member rows in inverted-index order, and each member's exact squared distance to the old centre
template <int MAXQ>
__global__ __launch_bounds__(256) void km_partsum_kernel(const float* __restrict__ X, const float* __restrict__ C_old, const int* __restrict__ order,
                                                         const int* __restrict__ offsets, const int* __restrict__ counts, const int* __restrict__ part_base,
                                                         const int* __restrict__ scal, int K, int D, double* __restrict__ part_sum,
                                                         double* __restrict__ part_d2, double* __restrict__ rowd2) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= scal[3]) return;
    const int k = km_part_cluster(part_base, K, p);
    const int j0 = offsets[k] + (p - part_base[k]) * KM_PART;
    const int j1 = min(offsets[k] + counts[k], j0 + KM_PART);
    const int nq = D >> 2;
    kf4 c[MAXQ];
    double acc[MAXQ][4];
#pragma unroll
    for (int q = 0; q < MAXQ; ++q) {
        const int cc = lane + 64 * q;
        c[q] = cc < nq ? reinterpret_cast<const kf4*>(C_old + (long long)k * D)[cc] : kf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[q][e] = 0.0;
    }
    double pd2 = 0.0;
    for (int j = j0; j < j1; ++j) {
        const long long i = order[j];
        double d2 = 0.0;
#pragma unroll
        for (int q = 0; q < MAXQ; ++q) {
            const int cc = lane + 64 * q;
            if (cc < nq) {
                const kf4 x = reinterpret_cast<const kf4*>(X + i * D)[cc];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc[q][e] += (double)x[e];
                    const double df = (double)x[e] - (double)c[q][e];
                    d2 = fma(df, df, d2);
                }
            }
        }
        d2 = wave_sum_d(d2);
        pd2 += d2;
        if (lane == 0) rowd2[i] = d2;
    }
#pragma unroll
    for (int q = 0; q < MAXQ; ++q) {
        const int cc = lane + 64 * q;
        if (cc < nq)
#pragma unroll
            for (int e = 0; e < 4; ++e) part_sum[(long long)p * D + 4 * cc + e] = acc[q][e];
    }
    if (lane == 0) part_d2[p] = pd2;
}

// relocation of the empty clusters: the n_empty rows farthest from their centre (ties to the lower row index), in decreasing distance, go to the empty
// clusters in increasing index order. One workgroup, one arg-max pass over the rows per empty cluster; nothing to do (one tiny launch) when none is empty.
__global__ __launch_bounds__(1024) void km_relocate_kernel(const double* __restrict__ rowd2, long long N, const int16_t* __restrict__ labels,
                                                          const int* __restrict__ empty_list, const int* __restrict__ scal, int* __restrict__ reloc) {
    const int n = scal[2];
    if (n == 0) return;
    __shared__ double s_d[16];
    __shared__ long long s_i[16];
    double prev_d = INFINITY;
    long long prev_i = -1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int j = 0; j < n; ++j) {
        double bd = -1.0;
        long long bi = -1;
        for (long long i = threadIdx.x; i < N; i += 1024) {
            const double d = rowd2[i];
            // strictly after (prev_d, prev_i) in the order (distance descending, row ascending)
            const bool after = d < prev_d || (d == prev_d && i > prev_i);
            if (after && (d > bd || (d == bd && (bi < 0 || i < bi)))) { bd = d; bi = i; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double od = __shfl_xor(bd, off);
            const long long oi = __shfl_xor(bi, off);
            if (oi >= 0 && (bi < 0 || od > bd || (od == bd && oi < bi))) { bd = od; bi = oi; }
        }
        if (lane == 0) { s_d[w] = bd; s_i[w] = bi; }
        __syncthreads();
        bd = s_d[0]; bi = s_i[0];
        for (int v = 1; v < 16; ++v)
            if (s_i[v] >= 0 && (bi < 0 || s_d[v] > bd || (s_d[v] == bd && s_i[v] < bi))) { bd = s_d[v]; bi = s_i[v]; }
        __syncthreads();
        if (threadIdx.x == 0) {
            reloc[3 * j] = (int)bi;
            reloc[3 * j + 1] = bi >= 0 ? (int)labels[bi] : -1;
            reloc[3 * j + 2] = empty_list[j];
        }
        prev_d = bd; prev_i = bi;
    }
}

// one wave per cluster: the parts' partials in part order, the relocations applied in order, new centre = sum / count rounded to fp32 once
template <int MAXQ>
__global__ __launch_bounds__(256) void km_finalize_kernel(const double* __restrict__ part_sum, const int* __restrict__ part_base,
                                                          const int* __restrict__ counts_in, const float* __restrict__ X, const int* __restrict__ reloc,
                                                          const int* __restrict__ scal, const float* __restrict__ C_old, float* __restrict__ C_new,
                                                          int* __restrict__ counts_out, double* __restrict__ shift_k, float* __restrict__ cmax_k, int K, int D) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= K) return;
    const int nq = D >> 2;
    double s[MAXQ][4];
#pragma unroll
    for (int q = 0; q < MAXQ; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) s[q][e] = 0.0;
    for (int p = part_base[k]; p < part_base[k + 1]; ++p) {
#pragma unroll
        for (int q = 0; q < MAXQ; ++q) {
            const int cc = lane + 64 * q;
            if (cc < nq)
#pragma unroll
                for (int e = 0; e < 4; ++e) s[q][e] += part_sum[(long long)p * D + 4 * cc + e];
        }
    }
    int cnt = counts_in[k];
    const int n = scal[2];
    for (int j = 0; j < n; ++j) {
        const int row = reloc[3 * j], old = reloc[3 * j + 1], nw = reloc[3 * j + 2];
        if (row < 0 || (old != k && nw != k)) continue;
        const double sign = old == k ? -1.0 : 1.0;
        if (nw == k) {
#pragma unroll
            for (int q = 0; q < MAXQ; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) s[q][e] = 0.0;
            cnt = 0;
        }
#pragma unroll
        for (int q = 0; q < MAXQ; ++q) {
            const int cc = lane + 64 * q;
            if (cc < nq) {
                const kf4 x = reinterpret_cast<const kf4*>(X + (long long)row * D)[cc];
#pragma unroll
                for (int e = 0; e < 4; ++e) s[q][e] += sign * (double)x[e];
            }
        }
        cnt += old == k ? -1 : 1;
    }
    double sh = 0.0;
    float mx = 0.f;
#pragma unroll
    for (int q = 0; q < MAXQ; ++q) {
        const int cc = lane + 64 * q;
        if (cc < nq) {
            const kf4 co = reinterpret_cast<const kf4*>(C_old + (long long)k * D)[cc];
            kf4 cn;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                cn[e] = (float)(cnt > 0 ? s[q][e] / (double)cnt : s[q][e]);
                const double df = (double)cn[e] - (double)co[e];
                sh = fma(df, df, sh);
                mx = fmaxf(mx, fabsf(cn[e]));
            }
            reinterpret_cast<kf4*>(C_new + (long long)k * D)[cc] = cn;
        }
    }
    sh = wave_sum_d(sh);
    mx = wave_max_f(mx);
    if (lane == 0) { counts_out[k] = cnt; shift_k[k] = sh; cmax_k[k] = mx; }
}

// stats: [0] inertia (ordered sum of the parts), [1] shift2, [2] n_changed, [3] n_empty, [4] max |C_new|, [5] n_invalid
__global__ __launch_bounds__(256) void km_stats_kernel(const double* __restrict__ part_d2, const int* __restrict__ scal, const double* __restrict__ shift_k,
                                                       const float* __restrict__ cmax_k, int K, double* __restrict__ stats) {
    __shared__ double s_a[256], s_b[256];
    __shared__ float s_m[256];
    const int P = scal[3];
    const int pp = (P + 255) / 256, pk = (K + 255) / 256;
    double a = 0.0, b = 0.0;
    float m = 0.f;
    for (int p = threadIdx.x * pp; p < min(P, (int)(threadIdx.x + 1) * pp); ++p) a += part_d2[p];
    for (int k = threadIdx.x * pk; k < min(K, (int)(threadIdx.x + 1) * pk); ++k) { b += shift_k[k]; m = fmaxf(m, cmax_k[k]); }
    s_a[threadIdx.x] = a; s_b[threadIdx.x] = b; s_m[threadIdx.x] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        a = 0.0; b = 0.0; m = 0.f;
        for (int j = 0; j < 256; ++j) { a += s_a[j]; b += s_b[j]; m = fmaxf(m, s_m[j]); }
        stats[0] = a; stats[1] = b; stats[2] = (double)scal[0]; stats[3] = (double)scal[2]; stats[4] = (double)m; stats[5] = (double)scal[1];
    }
}

// ---- k-means++ -----------------------------------------------------------------------------------------------------------------------------------
// pp (int): [0] best trial of the last step, [1 .. trials] candidate rows
__global__ void km_pp_first_kernel(const double* __restrict__ u, long long N, int* __restrict__ pp) {
    if (threadIdx.x == 0) {
        long long r = (long long)floor(u[0] * (double)N);
        r = r < 0 ? 0 : (r > N - 1 ? N - 1 : r);
        pp[0] = 0;
        pp[1] = (int)r;
    }
}

// closest = cand_min[best]; inclusive scan of closest within each KM_PP_SEG segment (fixed order; the global value is the segments' prefix plus it),
// segment totals
__global__ __launch_bounds__(256) void km_pp_scan_kernel(const double* __restrict__ cand_min, const int* __restrict__ pp, long long N,
                                                         double* __restrict__ closest, double* __restrict__ scan, double* __restrict__ seg_tot) {
    __shared__ double s[256];
    const long long cb = (long long)pp[0] * N;
    const long long s0 = (long long)blockIdx.x * KM_PP_SEG;
    constexpr int per = KM_PP_SEG / 256;
    const long long r0 = s0 + threadIdx.x * per;
    double v[per];
    double run = 0.0;
#pragma unroll
    for (int j = 0; j < per; ++j) {
        const long long i = r0 + j;
        v[j] = i < N ? cand_min[cb + i] : 0.0;
        if (i < N) closest[i] = v[j];
        run += v[j];
        v[j] = run;
    }
    s[threadIdx.x] = run;
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0;
        for (int j = 0; j < 256; ++j) { const double x = s[j]; s[j] = a; a += x; }
        seg_tot[blockIdx.x] = a;
    }
    __syncthreads();
    const double off = s[threadIdx.x];
#pragma unroll
    for (int j = 0; j < per; ++j) {
        const long long i = r0 + j;
        if (i < N) scan[i] = off + v[j];
    }
}

// one workgroup: inclusive prefix of the segment totals (fixed order), then per trial the first row whose inclusive scan is >= u * total
__global__ __launch_bounds__(1024) void km_pp_search_kernel(const double* __restrict__ seg_tot, int nseg, const double* __restrict__ scan, long long N,
                                                            const double* __restrict__ u, int trials, double* __restrict__ seg_pre, int* __restrict__ pp) {
    __shared__ double s[1024];
    const int per = (nseg + 1023) / 1024;
    const int a0 = min(nseg, (int)threadIdx.x * per), a1 = min(nseg, a0 + per);
    double run = 0.0;
    for (int j = a0; j < a1; ++j) run += seg_tot[j];
    s[threadIdx.x] = run;
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0;
        for (int j = 0; j < 1024; ++j) { const double x = s[j]; s[j] = a; a += x; }
    }
    __syncthreads();
    run = s[threadIdx.x];
    for (int j = a0; j < a1; ++j) { run += seg_tot[j]; seg_pre[j] = run; }
    __threadfence_block();
    __syncthreads();   // seg_pre is read back by other threads of this workgroup below
    if ((int)threadIdx.x < trials) {
        const double total = seg_pre[nseg - 1];
        const double v = u[threadIdx.x] * total;
        int lo = 0, hi = nseg - 1;   // first segment whose inclusive prefix >= v (the last one if none)
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (seg_pre[mid] >= v) hi = mid; else lo = mid + 1; }
        const double base = lo > 0 ? seg_pre[lo - 1] : 0.0;   // scan[] is inclusive within its segment
        long long a = (long long)lo * KM_PP_SEG, b = min(N, a + KM_PP_SEG) - 1;
        while (a < b) { const long long mid = (a + b) >> 1; if (base + scan[mid] >= v) b = mid; else a = mid + 1; }
        pp[1 + threadIdx.x] = (int)a;
    }
}

// one pass over X: for every trial t, cand_min[t][i] = min(closest_i, |x_i - x_cand_t|^2) (float64; first: no closest yet) and the workgroup's
// potential per trial (its waves' row-ordered sums added in wave order)
template <int MAXQ>
__global__ __launch_bounds__(256) void km_pp_dist_kernel(const float* __restrict__ X, long long N, int D, const int* __restrict__ pp, int trials, int first,
                                                         const double* __restrict__ closest, double* __restrict__ cand_min, double* __restrict__ blk_pot) {
    extern __shared__ float cand[];   // [trials][D]
    __shared__ double s_pot[4][KM_MAX_TRIALS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nq = D >> 2;
    for (int t = 0; t < trials; ++t)
        for (int c = threadIdx.x; c < nq; c += 256)
            reinterpret_cast<kf4*>(cand + t * D)[c] = reinterpret_cast<const kf4*>(X + (long long)pp[1 + t] * D)[c];
    __syncthreads();
    double pot[KM_MAX_TRIALS];
#pragma unroll
    for (int t = 0; t < KM_MAX_TRIALS; ++t) pot[t] = 0.0;
    const long long r0 = (long long)blockIdx.x * KM_PP_ROWS + w * (KM_PP_ROWS / 4);
    const long long r1 = min(N, r0 + KM_PP_ROWS / 4);
    for (long long i = r0; i < r1; ++i) {
        kf4 x[MAXQ];
#pragma unroll
        for (int q = 0; q < MAXQ; ++q) {
            const int cc = lane + 64 * q;
            x[q] = cc < nq ? reinterpret_cast<const kf4*>(X + i * D)[cc] : kf4{0.f, 0.f, 0.f, 0.f};
        }
        const double cl = first ? INFINITY : closest[i];
#pragma unroll
        for (int t = 0; t < KM_MAX_TRIALS; ++t) {
            if (t >= trials) continue;   // uniform: keeps the loop unrolled and pot[] in registers
            double d2 = 0.0;
#pragma unroll
            for (int q = 0; q < MAXQ; ++q) {
                const int cc = lane + 64 * q;
                if (cc < nq) {
                    const kf4 c = reinterpret_cast<const kf4*>(cand + t * D)[cc];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const double df = (double)x[q][e] - (double)c[e];
                        d2 = fma(df, df, d2);
                    }
                }
            }
            d2 = wave_sum_d(d2);
            const double m = fmin(cl, d2);
            pot[t] += m;
            if (lane == 0) cand_min[(long long)t * N + i] = m;
        }
    }
    if (lane == 0)
        for (int t = 0; t < trials; ++t) s_pot[w][t] = pot[t];
    __syncthreads();
    if ((int)threadIdx.x < trials) {
        const int t = threadIdx.x;
        blk_pot[(long long)blockIdx.x * trials + t] = ((s_pot[0][t] + s_pot[1][t]) + s_pot[2][t]) + s_pot[3][t];
    }
}

// one workgroup: the trials' potentials (block partials, one wave per trial, fixed order), the best candidate becomes centre c. Ties go to the first
// trial, as sklearn's np.argmin over the candidates: duplicate rows give equal potentials, and the row sklearn keeps is the first drawn, not the lowest.
__global__ __launch_bounds__(1024) void km_pp_choose_kernel(const double* __restrict__ blk_pot, int nblk, int trials, const float* __restrict__ X, int D,
                                                            int c, int* __restrict__ pp, float* __restrict__ C_out, int64_t* __restrict__ picked) {
    __shared__ double s_pot[KM_MAX_TRIALS];
    __shared__ int s_best;
    const int lane = threadIdx.x & 63, t = threadIdx.x >> 6;
    if (t < trials) {
        const int per = (nblk + 63) / 64;
        double a = 0.0;
        for (int b = lane * per; b < min(nblk, (lane + 1) * per); ++b) a += blk_pot[(long long)b * trials + t];
        a = wave_sum_d(a);
        if (lane == 0) s_pot[t] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int best = 0;
        for (int j = 1; j < trials; ++j)
            if (s_pot[j] < s_pot[best]) best = j;
        s_best = best;
    }
    __syncthreads();
    const int best = s_best;
    const long long row = pp[1 + best];
    for (int k = threadIdx.x; k < (D >> 2); k += 1024)
        reinterpret_cast<kf4*>(C_out + (long long)c * D)[k] = reinterpret_cast<const kf4*>(X + row * D)[k];
    __syncthreads();
    if (threadIdx.x == 0) { pp[0] = best; picked[c] = row; }
}

}  // namespace
}  // namespace at

using namespace at;

struct at_kmeans {
    int device = 0;
    long long N = 0;
    int D = 0, K = 0, Kpad = 0;
    int chunk = 0, chunk_pad = 0, nchunks = 0, ntiles = 0, max_parts = 0, trials = 0, nseg = 0, npp_blk = 0;
    int scheme = XB_SCHEME_F16X2;
    const float* X = nullptr;
    float x_max_abs = 0.f, x_scale = 1.f;
    bool have_data = false;
    char* base = nullptr;
    // carved from one allocation (km_layout)
    piece_t* xs = nullptr;      // f16x2: X as operand pieces, per chunk [2][D/16][chunk_pad][16]
    piece_t* xchunk = nullptr;  // bf16x3: one chunk's pieces, split per call
    piece_t* cs = nullptr;      // the centres as pieces [np][D/16][Kpad][16]
    float* e2 = nullptr;        // [Kpad]
    float* dots = nullptr;      // [chunk_pad][Kpad]
    int* pair = nullptr;        // range pairs: [0..1] the rows, [2..3] the centres
    int* tile = nullptr;        // [ntiles][K]
    int* cnt = nullptr;         // [K]
    int* offsets = nullptr;     // [K + 1]
    int* part_base = nullptr;   // [K + 1]
    int* empty_list = nullptr;  // [K]
    int* reloc = nullptr;       // [K][3]
    int* scal = nullptr;        // [4]
    int* order = nullptr;       // [N]
    double* part_sum = nullptr; // [max_parts][D]
    double* part_d2 = nullptr;  // [max_parts]
    double* rowd2 = nullptr;    // [N]
    double* shift_k = nullptr;  // [K]
    float* cmax_k = nullptr;    // [K]
    int* pp = nullptr;          // [1 + trials]
    double* closest = nullptr;  // [N]
    double* scan = nullptr;     // [N]
    double* seg_tot = nullptr;  // [nseg]
    double* seg_pre = nullptr;  // [nseg]
    double* cand_min = nullptr; // [trials][N]
    double* blk_pot = nullptr;  // [npp_blk][trials]
};

namespace {

int km_trials(int K) { return 2 + (int)std::log((double)K); }

// Every buffer of a handle, carved from one allocation at 256-byte alignment. base == nullptr: sizes only.
size_t km_layout(at_kmeans* h) {
    size_t off = 0;
    auto take = [&](auto*& p, size_t bytes) {
        off = (off + 255) / 256 * 256;
        p = h->base ? reinterpret_cast<std::remove_reference_t<decltype(p)>>(h->base + off) : nullptr;
        off += bytes;
    };
    const long long N = h->N;
    const int D = h->D, K = h->K;
    take(h->xs, (size_t)h->nchunks * 2 * D * h->chunk_pad * sizeof(piece_t));
    take(h->xchunk, (size_t)3 * D * h->chunk_pad * sizeof(piece_t));
    take(h->cs, (size_t)3 * D * h->Kpad * sizeof(piece_t));
    take(h->e2, (size_t)h->Kpad * sizeof(float));
    take(h->dots, (size_t)h->chunk_pad * h->Kpad * sizeof(float));
    take(h->pair, 4 * sizeof(int));
    take(h->tile, (size_t)h->ntiles * K * sizeof(int));
    take(h->cnt, (size_t)K * sizeof(int));
    take(h->offsets, (size_t)(K + 1) * sizeof(int));
    take(h->part_base, (size_t)(K + 1) * sizeof(int));
    take(h->empty_list, (size_t)K * sizeof(int));
    take(h->reloc, (size_t)3 * K * sizeof(int));
    take(h->scal, 4 * sizeof(int));
    take(h->order, (size_t)N * sizeof(int));
    take(h->part_sum, (size_t)h->max_parts * D * sizeof(double));
    take(h->part_d2, (size_t)h->max_parts * sizeof(double));
    take(h->rowd2, (size_t)N * sizeof(double));
    take(h->shift_k, (size_t)K * sizeof(double));
    take(h->cmax_k, (size_t)K * sizeof(float));
    take(h->pp, (size_t)(1 + KM_MAX_TRIALS) * sizeof(int));
    take(h->closest, (size_t)N * sizeof(double));
    take(h->scan, (size_t)N * sizeof(double));
    take(h->seg_tot, (size_t)h->nseg * sizeof(double));
    take(h->seg_pre, (size_t)h->nseg * sizeof(double));
    take(h->cand_min, (size_t)h->trials * N * sizeof(double));
    take(h->blk_pot, (size_t)h->npp_blk * h->trials * sizeof(double));
    return (off + 255) / 256 * 256;
}

int km_check_shape(long long N, int D, int K) {
    AT_REQUIRE(D >= 64 && D % 64 == 0 && D <= 1024, "k-means: D % 64 == 0 and 64 <= D <= 1024 (split-GEMM K blocking, vq_argmax row limit)");
    AT_REQUIRE(K >= 4 && K <= 32767 && K % 4 == 0, "k-means: 4 <= K <= 32767 and K % 4 == 0 (int16 labels, vq_argmax reads code rows four at a time)");
    AT_REQUIRE(N >= K && N < (1LL << 31) - KM_TILE, "k-means: K <= N < 2^31 rows");
    return 0;
}

void km_dims(at_kmeans* h) {
    const long long N = h->N;
    const int K = h->K;
    h->Kpad = (K + 127) / 128 * 128;
    long long ch = std::min<long long>(65536, KM_DOTS_FLOATS / h->Kpad / 256 * 256);
    ch = std::max<long long>(256, ch);
    ch = std::min<long long>(ch, (N + 255) / 256 * 256);
    h->chunk = (int)ch;
    h->chunk_pad = (int)ch;
    h->nchunks = (int)((N + ch - 1) / ch);
    h->ntiles = (int)((N + KM_TILE - 1) / KM_TILE);
    h->max_parts = (int)(N / KM_PART + K + 1);
    h->trials = km_trials(K);
    h->nseg = (int)((N + KM_PP_SEG - 1) / KM_PP_SEG);
    h->npp_blk = (int)((N + KM_PP_ROWS - 1) / KM_PP_ROWS);
}

template <int Q>
int km_launch_partsum(at_kmeans* h, const float* C_old, hipStream_t s) {
    hipLaunchKernelGGL(km_partsum_kernel<Q>, dim3((unsigned)((h->max_parts + 3) / 4)), dim3(256), 0, s, h->X, C_old, h->order, h->offsets, h->cnt,
                       h->part_base, h->scal, h->K, h->D, h->part_sum, h->part_d2, h->rowd2);
    AT_CHECK_HIP(hipGetLastError());
    return 0;
}
template <int Q>
int km_launch_finalize(at_kmeans* h, const float* C_old, float* C_new, int32_t* counts, hipStream_t s) {
    hipLaunchKernelGGL(km_finalize_kernel<Q>, dim3((unsigned)((h->K + 3) / 4)), dim3(256), 0, s, h->part_sum, h->part_base, h->cnt, h->X, h->reloc,
                       h->scal, C_old, C_new, reinterpret_cast<int*>(counts), h->shift_k, h->cmax_k, h->K, h->D);
    AT_CHECK_HIP(hipGetLastError());
    return 0;
}
template <int Q>
int km_launch_pp_dist(at_kmeans* h, int trials, int first, hipStream_t s) {
    static LdsAttrFlags flags;
    const size_t lds = (size_t)trials * h->D * sizeof(float);
    if (lds > 65536)
        if (int rc = set_max_dynamic_lds(flags, km_pp_dist_kernel<Q>, (size_t)KM_MAX_TRIALS * 1024 * sizeof(float))) return rc;
    hipLaunchKernelGGL(km_pp_dist_kernel<Q>, dim3((unsigned)h->npp_blk), dim3(256), lds, s, h->X, h->N, h->D, h->pp, trials, first, h->closest,
                       h->cand_min, h->blk_pot);
    AT_CHECK_HIP(hipGetLastError());
    return 0;
}
#define KM_BY_Q(fn, ...) ((h->D <= 256) ? fn<1>(__VA_ARGS__) : (h->D <= 512) ? fn<2>(__VA_ARGS__) : (h->D <= 768) ? fn<3>(__VA_ARGS__) : fn<4>(__VA_ARGS__))

float km_act_scale(float x_max_abs) {
    // LayerNorm-ed rows (1 <~ max |x| <= sqrt(D) <= 32): the tokenizers' scale; anything else (large, or so small that the fp16 pieces would be
    // subnormal under x 16): the weight rule on max |X|
    return (x_max_abs <= 32.0f && x_max_abs >= 0.5f) ? XB_F16_ACT_SCALE : xb_weight_scale(x_max_abs);
}

int km_split_rows(at_kmeans* h, hipStream_t s) {
    AT_CHECK_HIP(hipMemsetAsync(h->pair, 0, 2 * sizeof(int), s));
    if (h->scheme != XB_SCHEME_F16X2) return 0;
    for (int c = 0; c < h->nchunks; ++c) {
        const long long r0 = (long long)c * h->chunk, rows = std::min<long long>(h->chunk, h->N - r0);
        piece_t* dst = h->xs + (size_t)c * 2 * h->D * h->chunk_pad;
        if (int rc = launch_split_blocked(h->X + r0 * h->D, h->D, rows, h->chunk_pad, h->D, dst, s, XB_SCHEME_F16X2, h->x_scale, h->pair)) return rc;
    }
    return 0;
}

}  // namespace

extern "C" {

size_t at_kmeans_device_bytes(int64_t N, int D, int K) {
    if (km_check_shape(N, D, K)) return 0;
    at_kmeans h;
    h.N = N; h.D = D; h.K = K;
    km_dims(&h);
    return km_layout(&h);
}

at_kmeans_t* at_kmeans_create(int device, int64_t N, int D, int K) {
    if (km_check_shape(N, D, K)) return nullptr;
    DeviceGuard guard(device);
    if (!guard.ok) { set_error("at_kmeans_create: cannot select the device"); return nullptr; }
    at_kmeans* h = new at_kmeans();
    h->device = device; h->N = N; h->D = D; h->K = K;
    km_dims(h);
    const size_t bytes = km_layout(h);
    if (hipMalloc((void**)&h->base, bytes) != hipSuccess) {
        set_error("at_kmeans_create: device allocation of " + std::to_string(bytes) + " bytes failed");
        (void)hipGetLastError();
        delete h;
        return nullptr;
    }
    km_layout(h);
    return h;
}

void at_kmeans_destroy(at_kmeans_t* h) {
    if (!h) return;
    {
        DeviceGuard guard(h->device);
        if (h->base) (void)hipFree(h->base);
    }
    delete h;
}

int at_kmeans_set_option(at_kmeans_t* h, const char* name, int value) {
    AT_REQUIRE(h && name, "at_kmeans_set_option: bad arguments");
    if (std::string(name) == "scheme") {
        AT_REQUIRE(value == XB_SCHEME_BF16X3 || value == XB_SCHEME_F16X2, "at_kmeans_set_option: scheme 0 (bf16x3) or 1 (f16x2)");
        h->scheme = value;
        h->have_data = false;   // the rows are split again (f16x2) or per chunk (bf16x3) after the next at_kmeans_set_data
        return 0;
    }
    set_error(std::string("at_kmeans_set_option: unknown option ") + name);
    return -1;
}

int at_kmeans_get_option(const at_kmeans_t* h, const char* name) {
    AT_REQUIRE(h && name, "at_kmeans_get_option: bad arguments");
    if (std::string(name) == "scheme") return h->scheme;
    if (std::string(name) == "chunk_rows") return h->chunk;
    if (std::string(name) == "trials") return h->trials;
    set_error(std::string("at_kmeans_get_option: unknown option ") + name);
    return -1;
}

int at_kmeans_set_data(at_kmeans_t* h, const float* X, float x_max_abs, at_stream_t stream) {
    AT_REQUIRE(h && X && x_max_abs >= 0.f, "at_kmeans_set_data: bad arguments");
    AT_REQUIRE(reinterpret_cast<uintptr_t>(X) % 16 == 0, "at_kmeans_set_data: X must be 16-byte aligned");
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    h->X = X;
    h->x_max_abs = x_max_abs;
    h->x_scale = km_act_scale(x_max_abs);
    if (int rc = km_split_rows(h, (hipStream_t)stream)) return rc;
    h->have_data = true;
    return 0;
}

int at_kmeans_assign(at_kmeans_t* h, const float* C, float c_max_abs, int16_t* labels, int32_t* status_dev, at_stream_t stream_) {
    AT_REQUIRE(h && C && labels, "at_kmeans_assign: bad arguments");
    AT_REQUIRE(h->have_data, "at_kmeans_assign: at_kmeans_set_data first");
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    hipStream_t s = (hipStream_t)stream_;
    const int D = h->D, K = h->K;
    // centres are means / rows of X: max |X| bounds them when the caller has no better number
    const float cmax = c_max_abs > 0.f ? c_max_abs : h->x_max_abs;
    const float sw = h->scheme == XB_SCHEME_F16X2 ? xb_weight_scale(cmax) : 1.0f;
    const float sa = h->scheme == XB_SCHEME_F16X2 ? h->x_scale : 1.0f;
    if (status_dev) AT_CHECK_HIP(hipMemsetAsync(status_dev, 0, sizeof(int32_t), s));
    AT_CHECK_HIP(hipMemsetAsync(h->pair + 2, 0, 2 * sizeof(int), s));
    hipLaunchKernelGGL(km_e2_kernel, dim3((unsigned)((K + 3) / 4)), dim3(256), 0, s, C, h->e2, K, D);
    AT_CHECK_HIP(hipGetLastError());
    if (int rc = launch_split_blocked(C, D, K, h->Kpad, D, h->cs, s, h->scheme, sw, h->pair + 2)) return rc;
    for (int c = 0; c < h->nchunks; ++c) {
        const long long r0 = (long long)c * h->chunk, rows = std::min<long long>(h->chunk, h->N - r0);
        const piece_t* A;
        if (h->scheme == XB_SCHEME_F16X2) {
            A = h->xs + (size_t)c * 2 * D * h->chunk_pad;
        } else {
            if (int rc = launch_split_blocked(h->X + r0 * D, D, rows, h->chunk_pad, D, h->xchunk, s, XB_SCHEME_BF16X3, 1.0f, nullptr)) return rc;
            A = h->xchunk;
        }
        Bf16x3Args va;
        va.A = A; va.W = h->cs; va.bias = nullptr; va.M = (int)rows; va.N = h->Kpad; va.K = D; va.Mpad = h->chunk_pad;
        va.epi = XB_EPI_LINEAR; va.C = h->dots; va.ldc = h->Kpad; va.R = nullptr; va.ldr = h->Kpad; va.alpha = 1.f;
        va.scheme = h->scheme; va.status = nullptr;
        if (h->scheme == XB_SCHEME_F16X2) { va.acc_scale = 1.0f / (sa * sw); va.split_scale = sa; }
        if (int rc = launch_gemm_bf16x3(va, s)) return rc;
        if (int rc = launch_vq_argmax(h->X + r0 * D, h->dots, h->e2, labels + r0, rows, D, K, s, reinterpret_cast<int*>(status_dev), h->Kpad, C)) return rc;
    }
    if (status_dev) return launch_range_combine(h->pair, 2, reinterpret_cast<int*>(status_dev), s);
    return 0;
}

int at_kmeans_update(at_kmeans_t* h, const int16_t* labels, const int16_t* prev_labels, const float* C_old, float* C_new, int32_t* counts,
                     double* stats_dev, at_stream_t stream_) {
    AT_REQUIRE(h && labels && C_old && C_new && counts && stats_dev, "at_kmeans_update: bad arguments");
    AT_REQUIRE(h->have_data, "at_kmeans_update: at_kmeans_set_data first");
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    hipStream_t s = (hipStream_t)stream_;
    const int K = h->K;
    AT_CHECK_HIP(hipMemsetAsync(h->tile, 0, (size_t)h->ntiles * K * sizeof(int), s));
    AT_CHECK_HIP(hipMemsetAsync(h->scal, 0, 4 * sizeof(int), s));
    hipLaunchKernelGGL(km_hist_kernel, dim3((unsigned)h->ntiles), dim3(256), 0, s, labels, prev_labels, h->N, K, h->tile, h->scal);
    AT_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(km_colscan_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, s, h->tile, h->ntiles, K, h->cnt);
    AT_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(km_scan_kernel, dim3(1), dim3(1024), 0, s, h->cnt, K, h->offsets, h->part_base, h->empty_list, h->scal);
    AT_CHECK_HIP(hipGetLastError());
    {
        static LdsAttrFlags flags;
        const size_t lds = (size_t)K * sizeof(int);
        if (lds > 65536)
            if (int rc = set_max_dynamic_lds(flags, km_scatter_kernel, (size_t)32768 * sizeof(int))) return rc;
        hipLaunchKernelGGL(km_scatter_kernel, dim3((unsigned)h->ntiles), dim3(64), lds, s, labels, h->N, K, h->tile, h->offsets, h->order);
        AT_CHECK_HIP(hipGetLastError());
    }
    if (int rc = KM_BY_Q(km_launch_partsum, h, C_old, s)) return rc;
    hipLaunchKernelGGL(km_relocate_kernel, dim3(1), dim3(1024), 0, s, h->rowd2, h->N, labels, h->empty_list, h->scal, h->reloc);
    AT_CHECK_HIP(hipGetLastError());
    if (int rc = KM_BY_Q(km_launch_finalize, h, C_old, C_new, counts, s)) return rc;
    hipLaunchKernelGGL(km_stats_kernel, dim3(1), dim3(256), 0, s, h->part_d2, h->scal, h->shift_k, h->cmax_k, K, stats_dev);
    AT_CHECK_HIP(hipGetLastError());
    return 0;
}

int at_kmeans_layernorm(const float* x, float* y, int64_t rows, int D, int split_kernel, void* workspace, size_t workspace_bytes, at_stream_t stream) {
    AT_REQUIRE(x && y && rows >= 1 && D >= 64 && D % 64 == 0 && D <= 1024, "at_kmeans_layernorm: bad arguments");
    if (!split_kernel) return launch_layernorm(x, nullptr, nullptr, nullptr, y, rows, D, (hipStream_t)stream);
    // the semantic_m quantiser step's kernel: fp32 rows and fp16 operand pieces in one pass (the pieces go to the workspace and are not used)
    const long long rows_pad = (rows + 7) / 8 * 8;
    AT_REQUIRE(workspace && workspace_bytes >= (size_t)rows_pad * D * 2 * sizeof(piece_t), "at_kmeans_layernorm: workspace >= round_up(rows, 8) * D * 4 bytes");
    return launch_layernorm_split(x, nullptr, nullptr, nullptr, y, rows, D, SplitOut{static_cast<piece_t*>(workspace), rows_pad, XB_SCHEME_F16X2, XB_F16_ACT_SCALE, nullptr},
                                  (hipStream_t)stream);
}

int at_kmeans_row_d2(const at_kmeans_t* h, double* out, at_stream_t stream) {
    AT_REQUIRE(h && out, "at_kmeans_row_d2: bad arguments");
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    AT_CHECK_HIP(hipMemcpyAsync(out, h->rowd2, (size_t)h->N * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int at_kmeans_relocations(const at_kmeans_t* h, int32_t* out, at_stream_t stream) {
    AT_REQUIRE(h && out, "at_kmeans_relocations: bad arguments");
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    AT_CHECK_HIP(hipMemcpyAsync(out, h->reloc, (size_t)3 * h->K * sizeof(int), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int at_kmeans_plusplus(at_kmeans_t* h, const double* uniforms, int trials, float* C_out, int64_t* picked_rows, at_stream_t stream_) {
    AT_REQUIRE(h && uniforms && C_out && picked_rows, "at_kmeans_plusplus: bad arguments");
    AT_REQUIRE(h->X, "at_kmeans_plusplus: at_kmeans_set_data first");
    AT_REQUIRE(trials == h->trials, "at_kmeans_plusplus: trials must be 2 + int(ln K) (at_kmeans_get_option(h, \"trials\"))");
    DeviceGuard guard(h->device);
    AT_REQUIRE(guard.ok, "cannot select the handle's device");
    hipStream_t s = (hipStream_t)stream_;
    const int K = h->K;
    hipLaunchKernelGGL(km_pp_first_kernel, dim3(1), dim3(64), 0, s, uniforms, h->N, h->pp);
    AT_CHECK_HIP(hipGetLastError());
    if (int rc = KM_BY_Q(km_launch_pp_dist, h, 1, 1, s)) return rc;
    hipLaunchKernelGGL(km_pp_choose_kernel, dim3(1), dim3(1024), 0, s, h->blk_pot, h->npp_blk, 1, h->X, h->D, 0, h->pp, C_out, picked_rows);
    AT_CHECK_HIP(hipGetLastError());
    for (int c = 1; c < K; ++c) {
        hipLaunchKernelGGL(km_pp_scan_kernel, dim3((unsigned)h->nseg), dim3(256), 0, s, h->cand_min, h->pp, h->N, h->closest, h->scan, h->seg_tot);
        AT_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(km_pp_search_kernel, dim3(1), dim3(1024), 0, s, h->seg_tot, h->nseg, h->scan, h->N, uniforms + (size_t)c * trials, trials,
                           h->seg_pre, h->pp);
        AT_CHECK_HIP(hipGetLastError());
        if (int rc = KM_BY_Q(km_launch_pp_dist, h, trials, 0, s)) return rc;
        hipLaunchKernelGGL(km_pp_choose_kernel, dim3(1), dim3(1024), 0, s, h->blk_pot, h->npp_blk, trials, h->X, h->D, c, h->pp, C_out, picked_rows);
        AT_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
