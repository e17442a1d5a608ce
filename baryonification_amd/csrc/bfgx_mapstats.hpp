// bfgx_mapstats.hpp -- reductions over whole HEALPix maps for gfx950: the higher-order statistics of shells (moments and
// cross-moments of up to three maps, counts of local maxima and minima, Minkowski functionals of the excursion sets), and the
// counts of maxima and minima of a square grid.  The moment and Minkowski kernels take npix values in any pixelisation.
//
//   mapstats_sum_kernel<K>      pass 1: per-block fp64 sums of the K maps over the good pixels, and their number
//   mapstats_central_kernel<K>  pass 2: per-block fp64 sums of prod_a (x_a - mean_a)^{e_a} for every exponent tuple of degree 2..4
//   mapstats_combine_kernel     one workgroup: the block partials of a pass added in a fixed order, divided by n
//   mapstats_peaks_kernel       one lane per pixel: the 8 neighbours (hpx::pix_neighbours), strict maximum / minimum, a histogram of
//                               the extrema's values per workgroup in LDS, integer atomics to the result
//   mapstats_peaks_grid_kernel  the same outputs for a square grid [n][n]: tiles of 32 x 64 pixels staged in LDS with their halo
//   mapstats_minkowski_kernel   one lane per pixel: the bin of u, sqrt(g2) and c / g2 from the six derivative maps, per-block fp64
//                               sums per bin in a fixed order (below), integer counts per bin
//   mapstats_minkowski_combine_kernel   one lane per (sum, bin): the block partials added in block order
//
// A pixel is good if every map is finite and not UNSEEN there (hpx::good_value) and the mask, if there is one, is nonzero.
//
// Determinism of the moments.  The grid (moment_blocks) depends on npix alone; a lane adds its pixels in ascending order, a wave adds
// its lanes by a shuffle tree, lane 0 of wave 0 adds the four waves in order, and mapstats_combine_kernel adds the block partials the
// same way.  No float atomics: a repeated call gives the same bits.  The peak counts are integers, so their atomics are exact.
//
// Determinism of the Minkowski sums.  The same grid; every step of a workgroup takes 256 consecutive pixels, so what a wave holds
// depends on npix alone.  A wave serves the bin of its lowest unserved lane: the lanes holding that bin contribute their two terms to a
// fixed tree of lane-to-lane moves (half_sum; the others 0), lanes 31 and 63 add the results to the wave's own LDS slots
// [wave][2][nb]; then the next unserved lane's bin.  At the end the four waves' slots are added in order into work[block][2][nb], and
// the combine kernel adds the blocks in order.  The order of every addition is a function of the input alone: no float atomics, a
// repeated call gives the same bits.
//
// Per pixel: pass 1 and pass 2 each read K doubles (+ 1 mask byte) and write nothing; the peaks kernel reads 1 double (+ 1 byte),
// gathers 8 neighbour values (+ 8 bytes) that mostly hit L2 (neighbours lie on the same and the two adjacent rings), and writes 1
// flag byte when asked to; the grid peaks kernel reads 1.10 doubles (+ 1.10 bytes), its 8 neighbours from LDS, and writes the same
// flag byte; the Minkowski kernel reads 6 doubles (+ 1 byte) = 49 B and writes nothing.
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

// ---- extrema of a square grid [n][n] (C order), 3 <= n <= 16384: the 8 neighbours are (i + di, j + dj), wrapped on both axes when
// `periodic`, else a pixel on the border is never an extremum
constexpr int kGridTileW = 64;             // pixels of a tile row: four whole 128-byte lines, one pixel per lane of a wave
constexpr int kGridTileH = 32;             // rows of a tile: each of the four waves takes every fourth
constexpr int kGridLdsW = kGridTileW + 2, kGridLdsH = kGridTileH + 2;      // with the one-pixel halo: 34 x 66 doubles = 17 952 B
constexpr int kGridMaxBlocks = 2048;       // 8 workgroups per CU (LDS: 8 x 17.5 KiB + the histograms), each taking tiles in turn
constexpr int64_t kGridMinN = 3, kGridMaxN = 16384;

// the value of pixel (i, j) if it is good, NaN if it is bad or outside the map.  periodic: i = -1 is row n - 1 and i = n is row 0 (the
// only rows outside [0, n) a neighbour can lie in), the same for j.  A NaN makes every comparison false, so a pixel with a bad or
// missing neighbour, or bad itself, is neither above nor below its neighbours: no separate flags
__device__ inline double grid_good_value(const double *__restrict__ map, const uint8_t *__restrict__ mask, int n, int periodic, int i, int j)
{
    if (periodic) {
        i = i == -1 ? n - 1 : i == n ? 0 : i;
        j = j == -1 ? n - 1 : j == n ? 0 : j;
    }
    if (i < 0 || i >= n || j < 0 || j >= n) return __longlong_as_double(0x7ff8000000000000ll);
    const int64_t p = (int64_t)i * n + j;
    const double v = map[p];
    return hpx::good_value(v) && (!mask || mask[p] != 0) ? v : __longlong_as_double(0x7ff8000000000000ll);
}

// The outputs of mapstats_peaks_kernel for a square grid.  A workgroup takes tiles of kGridTileH x kGridTileW pixels in turn: the tile
// and its halo (wrapped at the seams, NaN outside a map that is not periodic, NaN where the pixel is bad) are staged in LDS once, so a
// value is fetched once per tile that needs it (1.10 fetches per pixel) and not nine times; then lane = column, so a wave reads a row
// of LDS at consecutive addresses.  Tiles beyond the map's edge are partial.  Dynamic LDS: 2 nb ints.
__global__ void __launch_bounds__(kThreads)
mapstats_peaks_grid_kernel(int n, int periodic, int nb, const double *__restrict__ map, const uint8_t *__restrict__ mask,
                           const double *__restrict__ edges, unsigned long long *__restrict__ counts, int8_t *__restrict__ flags)
{
    extern __shared__ int s_hist[];
    __shared__ double s_v[kGridLdsH * kGridLdsW];
    for (int b = threadIdx.x; b < 2 * nb; b += kThreads) s_hist[b] = 0;
    const int tcols = (n + kGridTileW - 1) / kGridTileW, trows = (n + kGridTileH - 1) / kGridTileH;
    const int col = threadIdx.x & (kGridTileW - 1);
    for (int tile = blockIdx.x; tile < tcols * trows; tile += gridDim.x) {
        const int i0 = (tile / tcols) * kGridTileH, j0 = (tile % tcols) * kGridTileW;
        __syncthreads();                                                   // (the histogram is zeroed; the last tile has been read)
        for (int t = threadIdx.x; t < kGridLdsH * kGridLdsW; t += kThreads)
            s_v[t] = grid_good_value(map, mask, n, periodic, i0 - 1 + t / kGridLdsW, j0 - 1 + t % kGridLdsW);
        __syncthreads();
        const int j = j0 + col;
        for (int r = threadIdx.x / kGridTileW; r < kGridTileH; r += kThreads / kGridTileW) {
            const int i = i0 + r;
            if (i >= n || j >= n) continue;
            const double *c = s_v + (r + 1) * kGridLdsW + col + 1;
            const double v = c[0];
            bool above = true, below = true;
#pragma unroll
            for (int di = -1; di <= 1; ++di) {
#pragma unroll
                for (int dj = -1; dj <= 1; ++dj) {
                    if (di == 0 && dj == 0) continue;
                    const double w = c[di * kGridLdsW + dj];
                    above = above && v > w;
                    below = below && v < w;
                }
            }
            const int kind = above ? 1 : below ? -1 : 0;
            if (flags) flags[(int64_t)i * n + j] = (int8_t)kind;
            if (kind != 0 && v >= edges[0] && v < edges[nb]) {
                int lo = 0, hi = nb;                                       // edges[lo] <= v < edges[hi]
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (v >= edges[mid]) lo = mid; else hi = mid;
                }
                atomicAdd(&s_hist[(kind > 0 ? 0 : nb) + lo], 1);
            }
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < 2 * nb; b += kThreads)
        if (s_hist[b]) atomicAdd(&counts[b], (unsigned long long)s_hist[b]);
}

constexpr int kMaxMfBins = 512;

// LDS of mapstats_minkowski_kernel: edges[nb + 1] and sums[kWaves][2][nb] doubles, counts[nb + 3] ints: 38 932 B at nb = 512, so four
// workgroups still share a CU's 160 KiB (the grid has at most kMaxBlocks = 4 x 256 of them)
__host__ __device__ constexpr size_t minkowski_lds_bytes(int nb)
{
    return sizeof(double) * (size_t)(nb + 1 + kWaves * 2 * nb) + sizeof(int) * (size_t)(nb + 3);
}
static_assert(minkowski_lds_bytes(kMaxMfBins) <= 160 * 1024 / 4, "four workgroups per CU");

// v of the lane that kCtrl names (a DPP control: row_shr:n = 0x110 + n, row_bcast15 = 0x142), 0.0 where there is no such lane or the
// row (16 lanes) is not in kRowMask
template <int kCtrl, int kRowMask>
__device__ inline double dpp_fetch(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), kCtrl, kRowMask, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), kCtrl, kRowMask, 0xf, false);
    return __hiloint2double(hi, lo);
}

// lane 31 returns the sum of v over lanes 0..31 and lane 63 that over lanes 32..63, in one fixed order: within every row of 16 lanes
// lane i adds the lanes 1, 2, 4 and 8 below it in turn (lane 15 then holds the row), then rows 1 and 3 add lane 15 of the row below.
// DPP moves run on the vector unit; the same tree through __shfl_down would be 10 LDS-crossbar operations
__device__ inline double half_sum(double v)
{
    v += dpp_fetch<0x111, 0xf>(v);
    v += dpp_fetch<0x112, 0xf>(v);
    v += dpp_fetch<0x114, 0xf>(v);
    v += dpp_fetch<0x118, 0xf>(v);
    v += dpp_fetch<0x142, 0xa>(v);
    return v;
}

// the two summed terms of a pixel from x = [u, u_t, u_p, lap, q_plus, q_cross]: t1 = sqrt(g2), t2 = c / g2 (0 where g2 = 0).  Every product
// is rounded (no fused multiply-add), so the terms are those of the same expressions in IEEE arithmetic anywhere else
__device__ inline void minkowski_terms(const double x[6], double &t1, double &t2)
{
#pragma clang fp contract(off)
    const double a2 = x[1] * x[1], b2 = x[2] * x[2], g2 = a2 + b2;
    const double c = x[1] * x[2] * x[5] - 0.5 * x[3] * g2 + 0.5 * x[4] * (a2 - b2);
    t1 = sqrt(g2);
    t2 = g2 > 0.0 ? c / g2 : 0.0;
}

// ders = [u, u_t, u_p, lap, q_plus, q_cross][npix]; a pixel is good if all six are finite, u is not UNSEEN and the mask, if there is one, is
// nonzero.  Over the good pixels with edges[b] <= u < edges[b + 1]:
// part[blockIdx.x][0][b] = sum sqrt(g2), part[blockIdx.x][1][b] = sum c / g2 (0 where g2 = 0), g2 = u_t^2 + u_p^2,
// c = u_t u_p q_cross - lap g2 / 2 + q_plus (u_t^2 - u_p^2) / 2; counts[b] pixels in bin b, counts[nb] below edges[0],
// counts[nb + 1] at or above edges[nb], counts[nb + 2] good pixels.  Dynamic LDS: minkowski_lds_bytes(nb).
__global__ void __launch_bounds__(kThreads)
mapstats_minkowski_kernel(int64_t npix, int nb, const double *__restrict__ ders, const uint8_t *__restrict__ mask,
                          const double *__restrict__ edges, unsigned long long *__restrict__ counts, double *__restrict__ part)
{
    extern __shared__ double s_mf[];
    double *s_edges = s_mf;                                                // [nb + 1]
    double *s_sum = s_mf + nb + 1;                                         // [kWaves][2][nb]
    int *s_cnt = reinterpret_cast<int *>(s_sum + kWaves * 2 * nb);         // [nb + 3]
    for (int b = threadIdx.x; b <= nb; b += kThreads) s_edges[b] = edges[b];
    for (int b = threadIdx.x; b < kWaves * 2 * nb; b += kThreads) s_sum[b] = 0.0;
    for (int b = threadIdx.x; b < nb + 3; b += kThreads) s_cnt[b] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const bool upper = lane >= 32;
    double *w_sum = s_sum + (threadIdx.x >> 6) * 2 * nb;
    const double e_lo = s_edges[0], e_hi = s_edges[nb];
    // base is the same for every lane of the workgroup: no lane leaves the loop before the shuffles of its wave
    for (int64_t base = (int64_t)blockIdx.x * kThreads; base < npix; base += (int64_t)gridDim.x * kThreads) {
        const int64_t i = base + threadIdx.x;
        int bin = -1;
        double t1 = 0.0, t2 = 0.0;
        if (i < npix) {
            double x[6];
            bool ok = !mask || mask[i] != 0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                x[a] = ders[a * npix + i];
                ok = ok && isfinite(x[a]);
            }
            if (ok && hpx::good_value(x[0])) {
                const double u = x[0];
                if (u < e_lo) bin = nb;
                else if (!(u < e_hi)) bin = nb + 1;
                else {
                    int lo = 0, hi = nb;                                   // edges[lo] <= u < edges[hi]
                    while (hi - lo > 1) {
                        const int mid = (lo + hi) >> 1;
                        if (u >= s_edges[mid]) lo = mid; else hi = mid;
                    }
                    bin = lo;
                    minkowski_terms(x, t1, t2);
                }
                atomicAdd(&s_cnt[bin], 1);
                atomicAdd(&s_cnt[nb + 2], 1);
                if (bin >= nb) bin = -1;
            }
        }
        // lanes 0..31 reduce the first term and lanes 32..63 the second: each half first takes its term from the other half, then one
        // tree of 5 steps (half_sum) serves both sums, which end in lanes 31 and 63
        const double keep = upper ? t2 : t1, give = upper ? t1 : t2;
        unsigned long long pending = __ballot(bin >= 0);
        while (pending) {
            const int b = __builtin_amdgcn_readlane(bin, __ffsll((long long)pending) - 1);   // the bin of the lowest unserved lane
            const bool mine = bin == b;
            const double v = half_sum((mine ? keep : 0.0) + __shfl_xor(mine ? give : 0.0, 32, 64));
            if ((lane & 31) == 31) w_sum[(upper ? nb : 0) + b] += v;
            pending &= ~__ballot(mine);
        }
    }
    __syncthreads();
    double *dst = part + (int64_t)blockIdx.x * 2 * nb;
    for (int v = threadIdx.x; v < 2 * nb; v += kThreads) {
        double t = s_sum[v];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) t += s_sum[w * 2 * nb + v];
        dst[v] = t;
    }
    for (int b = threadIdx.x; b < nb + 3; b += kThreads)
        if (s_cnt[b]) atomicAdd(&counts[b], (unsigned long long)s_cnt[b]);
}

// sums[v] = part[0][v] + part[1][v] + ... in block order, v < nvals (= 2 nb): one lane per value
__global__ void __launch_bounds__(kThreads)
mapstats_minkowski_combine_kernel(int nblocks, int nvals, const double *__restrict__ part, double *__restrict__ sums)
{
    const int v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= nvals) return;
    double t = part[v];
#pragma unroll 8
    for (int b = 1; b < nblocks; ++b) t += part[(int64_t)b * nvals + v];
    sums[v] = t;
}

}  // namespace mapstats
}  // namespace bfgx
