// bfgx_mapstats.hpp -- reductions over whole HEALPix maps for gfx950: the higher-order statistics of shells (moments and
// cross-moments of up to three maps, counts of local maxima and minima).
//
//   mapstats_sum_kernel<K>      pass 1: per-block fp64 sums of the K maps over the good pixels, and their number
//   mapstats_central_kernel<K>  pass 2: per-block fp64 sums of prod_a (x_a - mean_a)^{e_a} for every exponent tuple of degree 2..4
//   mapstats_combine_kernel     one workgroup: the block partials of a pass added in a fixed order, divided by n
//   mapstats_peaks_kernel       one lane per pixel: the 8 neighbours (hpx::pix_neighbours), strict maximum / minimum, a histogram of
//                               the extrema's values per workgroup in LDS, integer atomics to the result
//
// A pixel is good if every map is finite and not UNSEEN there (hpx::good_value) and the mask, if there is one, is nonzero.
//
// Determinism of the moments.  The grid (moment_blocks) depends on npix alone; a lane adds its pixels in ascending order, a wave adds
// its lanes by a shuffle tree, lane 0 of wave 0 adds the four waves in order, and mapstats_combine_kernel adds the block partials the
// same way.  No float atomics: a repeated call gives the same bits.  The peak counts are integers, so their atomics are exact.
//
// Per pixel: pass 1 and pass 2 each read K doubles (+ 1 mask byte) and write nothing; the peaks kernel reads 1 double (+ 1 byte),
// gathers 8 neighbour values (+ 8 bytes) that mostly hit L2 (neighbours lie on the same and the two adjacent rings), and writes 1
// flag byte when asked to.
#pragma once
#include "bfgx_hpx.hpp"

namespace bfgx {
namespace mapstats {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 1024;
constexpr int kMaxMaps = 3;
constexpr int kMaxOrder = 4;
constexpr int kSlots = 32;                 // doubles per block partial: up to 31 sums, the pixel count in the last one
constexpr int kMaxBins = 4096;

__host__ __device__ inline int moment_blocks(int64_t npix) { return (int)(npix < (int64_t)kThreads * kMaxBlocks ? (npix + kThreads - 1) / kThreads : kMaxBlocks); }

// exponent tuples of degree 2..order in the order of include/bfgx.h: C(K + d - 1, d) of degree d
__host__ __device__ inline int moment_terms(int K, int order)
{
    int n = 0;
    for (int d = 2; d <= order; ++d) n += K == 1 ? 1 : K == 2 ? d + 1 : (d + 1) * (d + 2) / 2;
    return n;
}

// sum over the workgroup in a fixed order; the result is valid in thread 0.  s_w: kWaves doubles of LDS per call site
__device__ inline double block_sum(double v, double *s_w)
{
#pragma unroll
    for (int st = 32; st > 0; st >>= 1) v += __shfl_down(v, st, 64);
    __syncthreads();                                                    // (s_w may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = s_w[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) t += s_w[w];
    return t;
}

template <int K>
__device__ inline bool good_pixel(const double *__restrict__ maps, const uint8_t *__restrict__ mask, int64_t npix, int64_t i, double x[K])
{
    bool ok = !mask || mask[i] != 0;
#pragma unroll
    for (int a = 0; a < K; ++a) {
        x[a] = maps[a * npix + i];
        ok = ok && hpx::good_value(x[a]);
    }
    return ok;
}

// part[blockIdx.x][a] = sum of map a, a < K; part[blockIdx.x][kSlots - 1] = good pixels (exact: < 2^53)
template <int K>
__global__ void __launch_bounds__(kThreads)
mapstats_sum_kernel(int64_t npix, const double *__restrict__ maps, const uint8_t *__restrict__ mask, double *__restrict__ part)
{
    __shared__ double s_w[kWaves];
    double sum[K];
    double cnt = 0.0;
#pragma unroll
    for (int a = 0; a < K; ++a) sum[a] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < npix; i += (int64_t)gridDim.x * kThreads) {
        double x[K];
        if (good_pixel<K>(maps, mask, npix, i, x)) {
            cnt += 1.0;
#pragma unroll
            for (int a = 0; a < K; ++a) sum[a] += x[a];
        }
    }
    double *dst = part + (int64_t)blockIdx.x * kSlots;
#pragma unroll
    for (int a = 0; a < K; ++a) {
        const double t = block_sum(sum[a], s_w);
        if (threadIdx.x == 0) dst[a] = t;
    }
    const double t = block_sum(cnt, s_w);
    if (threadIdx.x == 0) dst[kSlots - 1] = t;
}

// part[blockIdx.x][t] = sum over the block's good pixels of prod_a (x_a - mean_a)^{e_a}, t over the tuples of degree 2..4
template <int K>
__global__ void __launch_bounds__(kThreads)
mapstats_central_kernel(int64_t npix, const double *__restrict__ maps, const uint8_t *__restrict__ mask, const double *__restrict__ mean,
                        double *__restrict__ part)
{
    constexpr int NT = K == 1 ? 3 : K == 2 ? 12 : 31;
    __shared__ double s_w[kWaves];
    double mu[kMaxMaps] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < K; ++a) mu[a] = mean[a];
    double acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < npix; i += (int64_t)gridDim.x * kThreads) {
        double x[K];
        if (!good_pixel<K>(maps, mask, npix, i, x)) continue;
        double pw[kMaxMaps][kMaxOrder + 1];                               // pw[a][e] = (x_a - mean_a)^e; 1 for the maps beyond K
#pragma unroll
        for (int a = 0; a < kMaxMaps; ++a) {
            const double d = a < K ? x[a < K ? a : 0] - mu[a] : 1.0;
            pw[a][0] = 1.0;
#pragma unroll
            for (int e = 1; e <= kMaxOrder; ++e) pw[a][e] = pw[a][e - 1] * d;
        }
        int t = 0;
#pragma unroll
        for (int d = 2; d <= kMaxOrder; ++d) {
#pragma unroll
            for (int e0 = d; e0 >= 0; --e0) {
#pragma unroll
                for (int e1 = d - e0; e1 >= 0; --e1) {
                    const int e2 = d - e0 - e1;
                    if ((K == 1 && e0 != d) || (K == 2 && e2 != 0)) continue;
                    acc[t++] += pw[0][e0] * pw[1][e1] * pw[2][e2];
                }
            }
        }
    }
    double *dst = part + (int64_t)blockIdx.x * kSlots;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const double v = block_sum(acc[t], s_w);
        if (threadIdx.x == 0) dst[t] = v;
    }
}

// One workgroup.  count = sum_b part[b][kSlots - 1]; out[v] = (sum_b part[b][v]) / count for v < nvals (NaN when count = 0);
// n_out (pass 1 only) receives the count.  Lane j adds partials j, j + 256, ... in order, then block_sum.
__global__ void __launch_bounds__(kThreads)
mapstats_combine_kernel(int nblocks, int nvals, const double *__restrict__ part, double *__restrict__ out, int64_t *__restrict__ n_out)
{
    __shared__ double s_w[kWaves];
    __shared__ double s_cnt;
    double c = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += kThreads) c += part[(int64_t)b * kSlots + kSlots - 1];
    c = block_sum(c, s_w);
    if (threadIdx.x == 0) { s_cnt = c; if (n_out) *n_out = (int64_t)c; }
    __syncthreads();
    const double cnt = s_cnt;
    for (int v = 0; v < nvals; ++v) {
        double s = 0.0;
        for (int b = threadIdx.x; b < nblocks; b += kThreads) s += part[(int64_t)b * kSlots + v];
        s = block_sum(s, s_w);
        if (threadIdx.x == 0) out[v] = s / cnt;
    }
}

struct Peaks {
    int64_t nside, npix;
    int order, nest, nb;
};

// counts[0][b] maxima, counts[1][b] minima with edges[b] <= value < edges[b + 1]; flags (optional) +1 / -1 / 0 per pixel.
// Dynamic LDS: 2 nb ints.
__global__ void __launch_bounds__(kThreads)
mapstats_peaks_kernel(Peaks a, const double *__restrict__ map, const uint8_t *__restrict__ mask, const double *__restrict__ edges,
                      unsigned long long *__restrict__ counts, int8_t *__restrict__ flags)
{
    extern __shared__ int s_hist[];
    for (int b = threadIdx.x; b < 2 * a.nb; b += kThreads) s_hist[b] = 0;
    __syncthreads();
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < a.npix; p += (int64_t)gridDim.x * kThreads) {
        const double v = map[p];
        int kind = 0;
        if (hpx::good_value(v) && (!mask || mask[p] != 0)) {
            int64_t nbr[8];
            hpx::pix_neighbours(a.nside, a.order, a.nest, p, nbr);
            bool ok = true, above = true, below = true;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (nbr[k] < 0) continue;
                const double w = map[nbr[k]];
                ok = ok && hpx::good_value(w) && (!mask || mask[nbr[k]] != 0);
                above = above && v > w;
                below = below && v < w;
            }
            kind = !ok ? 0 : above ? 1 : below ? -1 : 0;
        }
        if (flags) flags[p] = (int8_t)kind;
        if (kind != 0 && v >= edges[0] && v < edges[a.nb]) {
            int lo = 0, hi = a.nb;                                         // edges[lo] <= v < edges[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (v >= edges[mid]) lo = mid; else hi = mid;
            }
            atomicAdd(&s_hist[(kind > 0 ? 0 : a.nb) + lo], 1);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < 2 * a.nb; b += kThreads)
        if (s_hist[b]) atomicAdd(&counts[b], (unsigned long long)s_hist[b]);
}

}  // namespace mapstats
}  // namespace bfgx
