// HEALPix pixel functions for gfx950 (MI355X): healpy.ud_grade, get_interp_weights / get_interp_val and the reference's
// regrid_pixels_hpix (HealpixRunner.py:14-67) as kernels over whole maps.
//
//   hpx_degrade_kernel        ud_grade, nside_out < nside_in: one output pixel per group of G = min(rat2, 256) lanes
//   hpx_upgrade_kernel        ud_grade, nside_out >= nside_in (and pure reorders): one lane per output pixel
//   hpx_interp_weights_kernel get_interp_weights: one lane per point (healpix_cxx get_interpol, bfgx_kernels.hpp)
//   hpx_interp_val_kernel     get_interp_val: one lane per point, every map of the point in the same lane
//   hpx_scatter_add_kernel    regrid_pixels_hpix: one lane per (i, j), fp64 global atomic add
//   hpx_neighbours_kernel     get_all_neighbours: one lane per pixel index (pix_neighbours, also the stencil of bfgx_mapstats.hpp)
//
// NEST <-> RING follows Gorski et al. 2005 (healpix_cxx xyf2ring / ring2xyf / xyf2nest / nest2xyf): a pixel is its base face f
// plus (ix, iy) in [0, nside)^2 within the face, and the NEST index is f nside^2 + the bit interleave of ix (even bits) and iy
// (odd bits).  Indices are 64-bit throughout.
//
// Degrade reads.  The rat2 = r^2 children of output pixel (f, x, y) are (f, x r + u, y r + v), u, v < r.  A RING row is a line of
// constant ix + iy, along which the ring index grows with ix - iy, so the children lie on 2 r - 1 rows u + v = t, each a contiguous
// run of min(t, 2 r - 2 - t) + 1 ring pixels (the run of face 4 can wrap at phi = 0).  A group enumerates its children row by row
// and along each run (diag_uv), so lanes next to each other read ring pixels next to each other; groups of one workgroup take output
// pixels in output order, and for a RING output those are neighbours along an output ring, whose runs interleave on the same input
// rows.  The same child order is used for every input ordering, so the result does not depend on it.
#pragma once
#include "bfgx_kernels.hpp"

namespace bfgx {
namespace hpx {

constexpr int kThreads = 256;
constexpr double kUnseen = -1.6375e30;

__host__ __device__ inline int ilog2(int64_t v) { int o = 0; while ((int64_t)1 << (o + 1) <= v) ++o; return o; }

__host__ __device__ inline int64_t spread_bits(int64_t v)          // bit k of v -> bit 2k
{
    uint64_t x = (uint64_t)v & 0xffffffffull;
    x = (x | (x << 16)) & 0x0000ffff0000ffffull;
    x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
    x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return (int64_t)x;
}

__host__ __device__ inline int64_t compress_bits(int64_t v)        // bit 2k of v -> bit k
{
    uint64_t x = (uint64_t)v & 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x >> 4)) & 0x00ff00ff00ff00ffull;
    x = (x | (x >> 8)) & 0x0000ffff0000ffffull;
    x = (x | (x >> 16)) & 0x00000000ffffffffull;
    return (int64_t)x;
}

__host__ __device__ inline int jrll(int f) { return (f >> 2) + 2; }                        // {2 x4, 3 x4, 4 x4}
__host__ __device__ inline int jpll(int f) { return ((f & 3) << 1) + ((f >> 2) == 1 ? 0 : 1); }   // {1,3,5,7, 0,2,4,6, 1,3,5,7}

__host__ __device__ inline int64_t xyf2nest(int order, int64_t ix, int64_t iy, int f)
{
    return ((int64_t)f << (2 * order)) + spread_bits(ix) + (spread_bits(iy) << 1);
}

__host__ __device__ inline void nest2xyf(int order, int64_t pix, int64_t &ix, int64_t &iy, int &f)
{
    f = (int)(pix >> (2 * order));
    pix &= ((int64_t)1 << (2 * order)) - 1;
    ix = compress_bits(pix);
    iy = compress_bits(pix >> 1);
}

__host__ __device__ inline int64_t xyf2ring(int64_t nside, int64_t ix, int64_t iy, int f)
{
    const int64_t nl4 = 4 * nside;
    const int64_t jr = (int64_t)jrll(f) * nside - ix - iy - 1;
    int64_t nr, start, kshift;
    if (jr < nside) {
        nr = jr; start = 2 * jr * (jr - 1); kshift = 0;
    } else if (jr > 3 * nside) {
        nr = nl4 - jr; start = 12 * nside * nside - 2 * nr * (nr + 1); kshift = 0;
    } else {
        nr = nside; start = 2 * nside * (nside - 1) + (jr - nside) * nl4; kshift = (jr - nside) & 1;
    }
    int64_t jp = ((int64_t)jpll(f) * nr + ix - iy + 1 + kshift) / 2;
    if (jp > nl4) jp -= nl4;
    if (jp < 1) jp += nl4;
    return start + jp - 1;
}

__host__ __device__ inline int64_t isqrt_pix(int64_t v)
{
    int64_t r = (int64_t)sqrt((double)v + 0.5);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

// kPow2: nside = 2^order and the belt divides by shifts; otherwise order is unused and any nside >= 1 is taken
template <bool kPow2>
__host__ __device__ inline void ring2xyf_t(int64_t nside, int order, int64_t pix, int64_t &ix, int64_t &iy, int &f)
{
    const int64_t nl2 = 2 * nside, ncap = 2 * nside * (nside - 1), npix = 12 * nside * nside;
    int64_t iring, iphi, kshift, nr;
    if (pix < ncap) {
        iring = (1 + isqrt_pix(1 + 2 * pix)) >> 1;
        iphi = (pix + 1) - 2 * iring * (iring - 1);
        kshift = 0; nr = iring;
        f = (int)((iphi - 1) / nr);
    } else if (pix < npix - ncap) {
        const int64_t ip = pix - ncap;
        const int64_t tmp = kPow2 ? ip >> (order + 2) : ip / (4 * nside);
        iring = tmp + nside;
        iphi = ip - tmp * 4 * nside + 1;
        kshift = (iring + nside) & 1;
        nr = nside;
        const int64_t ire = tmp + 1, irm = nl2 + 1 - tmp;
        const int64_t jm = iphi - (ire >> 1) + nside - 1, jp = iphi - (irm >> 1) + nside - 1;      // both >= 0
        const int64_t ifm = kPow2 ? jm >> order : jm / nside;
        const int64_t ifp = kPow2 ? jp >> order : jp / nside;
        f = (int)((ifp == ifm) ? (ifp | 4) : ((ifp < ifm) ? ifp : (ifm + 8)));
    } else {
        const int64_t ip = npix - pix;
        iring = (1 + isqrt_pix(2 * ip - 1)) >> 1;
        iphi = 4 * iring + 1 - (ip - 2 * iring * (iring - 1));
        kshift = 0; nr = iring;
        iring = 2 * nl2 - iring;
        f = (int)((iphi - 1) / nr + 8);
    }
    const int64_t irt = iring - ((2 + (f >> 2)) * nside) + 1;
    int64_t ipt = 2 * iphi - (int64_t)jpll(f) * nr - kshift - 1;
    if (ipt >= nl2) ipt -= 8 * nside;
    ix = (ipt - irt) >> 1;
    iy = (-ipt - irt) >> 1;
}

__host__ __device__ inline void ring2xyf(int64_t nside, int order, int64_t pix, int64_t &ix, int64_t &iy, int &f)
{
    ring2xyf_t<true>(nside, order, pix, ix, iy, f);
}

// nside must be 2^order
__host__ __device__ inline int64_t ring2nest(int64_t nside, int order, int64_t pix)
{
    int64_t ix, iy; int f;
    ring2xyf(nside, order, pix, ix, iy, f);
    return xyf2nest(order, ix, iy, f);
}

__host__ __device__ inline int64_t nest2ring(int64_t nside, int order, int64_t pix)
{
    int64_t ix, iy; int f;
    nest2xyf(order, pix, ix, iy, f);
    return xyf2ring(nside, ix, iy, f);
}

// The 8 neighbours of a pixel in healpy.get_all_neighbours' order SW, W, NW, N, NE, E, SE, S; -1 where there is none (the E and W
// corners of the 8 polar faces lack their E / W neighbour, the N and S corners of the 4 equatorial faces their N / S one: 24 in every
// map).  A step (dx, dy) that leaves the face [0, nside)^2 lands in the face across that edge or corner (healpix_cxx neighbors(): the
// face table, then the mirror / swap of (x, y) that a polar face's rotated neighbour asks for).  kNest: NEST indices, nside = 2^order.
// RING with kPow2 = false takes any nside.
template <bool kNest, bool kPow2>
__host__ __device__ inline void pix_neighbours(int64_t nside, int order, int64_t pix, int64_t out[8])
{
    const int xoff[8] = {-1, -1, 0, 1, 1, 1, 0, -1}, yoff[8] = {0, 1, 1, 1, 0, -1, -1, -1};
    // face across the edge / corner nbnum = 4 + (x over ? 1 : x under ? -1 : 0) + 3 (the same for y), for base face 0..11
    const signed char face[9][12] = {{8, 9, 10, 11, -1, -1, -1, -1, 10, 11, 8, 9},      // S
                                     {5, 6, 7, 4, 8, 9, 10, 11, 9, 10, 11, 8},          // SE
                                     {-1, -1, -1, -1, 5, 6, 7, 4, -1, -1, -1, -1},      // E
                                     {4, 5, 6, 7, 11, 8, 9, 10, 11, 8, 9, 10},          // SW
                                     {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11},            // the face itself
                                     {1, 2, 3, 0, 0, 1, 2, 3, 5, 6, 7, 4},              // NE
                                     {-1, -1, -1, -1, 7, 4, 5, 6, -1, -1, -1, -1},      // W
                                     {3, 0, 1, 2, 3, 0, 1, 2, 4, 5, 6, 7},              // NW
                                     {2, 3, 0, 1, -1, -1, -1, -1, 0, 1, 2, 3}};         // N
    // bit 0: x -> nside - 1 - x, bit 1: the same for y, bit 2: swap x and y; by face row (north, equatorial, south)
    const unsigned char swap[9][3] = {{0, 0, 3}, {0, 0, 6}, {0, 0, 0}, {0, 0, 5}, {0, 0, 0}, {5, 0, 0}, {0, 0, 0}, {6, 0, 0}, {3, 0, 0}};
    int64_t ix, iy; int f;
    if (kNest) nest2xyf(order, pix, ix, iy, f);
    else ring2xyf_t<kPow2>(nside, order, pix, ix, iy, f);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int64_t x = ix + xoff[k], y = iy + yoff[k];
        int nbnum = 4;
        if (x < 0) { x += nside; nbnum -= 1; } else if (x >= nside) { x -= nside; nbnum += 1; }
        if (y < 0) { y += nside; nbnum -= 3; } else if (y >= nside) { y -= nside; nbnum += 3; }
        const int nf = face[nbnum][f];
        if (nf < 0) { out[k] = -1; continue; }
        const int bits = swap[nbnum][f >> 2];
        if (bits & 1) x = nside - 1 - x;
        if (bits & 2) y = nside - 1 - y;
        if (bits & 4) { const int64_t t = x; x = y; y = t; }
        out[k] = kNest ? xyf2nest(order, x, y, nf) : xyf2ring(nside, x, y, nf);
    }
}

// order = log2 nside, or -1 when nside is no power of two (RING only)
__host__ __device__ inline int nbr_order(int64_t nside) { return (nside & (nside - 1)) == 0 ? ilog2(nside) : -1; }

__host__ __device__ inline void pix_neighbours(int64_t nside, int order, int nest, int64_t pix, int64_t out[8])
{
    if (nest) pix_neighbours<true, true>(nside, order, pix, out);
    else if (order >= 0) pix_neighbours<false, true>(nside, order, pix, out);
    else pix_neighbours<false, false>(nside, order, pix, out);
}

// child c (0 <= c < r^2) in run order: rows t = u + v ascending, u ascending along a row (the ring index ascending)
__device__ inline void diag_uv(int64_t c, int64_t r, int64_t &u, int64_t &v)
{
    const int64_t upper = r * (r + 1) / 2;                            // rows t < r hold t + 1 children each
    const bool lower = c >= upper;
    const int64_t cc = lower ? r * r - 1 - c : c;
    int64_t t = (int64_t)((sqrt(8.0 * (double)cc + 1.0) - 1.0) * 0.5);
    while (t * (t + 1) / 2 > cc) --t;
    while ((t + 1) * (t + 2) / 2 <= cc) ++t;
    const int64_t pos = cc - t * (t + 1) / 2;
    if (!lower) { u = pos; v = t - pos; }
    else { u = r - 1 - pos; v = (2 * r - 2 - t) - u; }                 // row 2r-2-t, walked from its far end
}

__device__ inline bool good_value(double v)
{
    return isfinite(v) && !(fabs(v - kUnseen) <= 1e-8 + 1e-5 * fabs(kUnseen));     // healpy.mask_bad tolerance, or not finite
}

struct Degrade {
    int64_t nside_in, nside_out, npix_in, npix_out;
    int order_in, order_out, lr;            // log2 nside_in, log2 nside_out, log2 (nside_in / nside_out)
    int nest_in, nest_out, pess;
    int lg;                                 // log2 G: lanes per output pixel
    double ratio;
};

// map blockIdx.y; output pixel q = blockIdx.x * (256 / G) + threadIdx.x / G; child c = lane + k G of that pixel, k < rat2 / G, summed
// in that order by the lane, then by a tree over the G lanes (stride G/2 .. 1): a fixed order, so results are bit-reproducible
template <typename TI, typename TO>
__global__ void __launch_bounds__(kThreads)
hpx_degrade_kernel(Degrade d, const TI *__restrict__ in, TO *__restrict__ out)
{
    __shared__ double s_sum[kThreads];
    __shared__ int s_hit[kThreads];
    const int G = 1 << d.lg;
    const int lane = threadIdx.x & (G - 1);
    const int64_t q = (int64_t)blockIdx.x * (kThreads >> d.lg) + (threadIdx.x >> d.lg);
    const TI *src = in + (int64_t)blockIdx.y * d.npix_in;
    const int64_t r = (int64_t)1 << d.lr, rat2 = r * r;
    double sum = 0.0;
    int hit = 0;
    if (q < d.npix_out) {
        const int64_t P = d.nest_out ? q : ring2nest(d.nside_out, d.order_out, q);
        int64_t x, y; int f;
        nest2xyf(d.order_out, P, x, y, f);
        for (int64_t c = lane; c < rat2; c += G) {
            int64_t u, v;
            diag_uv(c, r, u, v);
            const int64_t ix = (x << d.lr) + u, iy = (y << d.lr) + v;
            const int64_t p = d.nest_in ? xyf2nest(d.order_in, ix, iy, f) : xyf2ring(d.nside_in, ix, iy, f);
            const double val = (double)src[p];
            const bool ok = good_value(val);
            sum += ok ? val : 0.0;
            hit += ok ? 1 : 0;
        }
    }
    s_sum[threadIdx.x] = sum;
    s_hit[threadIdx.x] = hit;
    for (int st = G >> 1; st > 0; st >>= 1) {
        __syncthreads();
        if (lane < st) { s_sum[threadIdx.x] += s_sum[threadIdx.x + st]; s_hit[threadIdx.x] += s_hit[threadIdx.x + st]; }
    }
    __syncthreads();
    if (lane == 0 && q < d.npix_out) {
        const int nh = s_hit[threadIdx.x];
        const bool bad = d.pess ? (nh != rat2) : (nh == 0);
        out[(int64_t)blockIdx.y * d.npix_out + q] = bad ? (TO)kUnseen : (TO)((s_sum[threadIdx.x] * d.ratio) / (double)nh);
    }
}

// every output pixel takes its parent's value times ratio (lr = log2 (nside_out / nside_in); lr = 0: a reorder)
template <typename TI, typename TO>
__global__ void __launch_bounds__(kThreads)
hpx_upgrade_kernel(Degrade d, const TI *__restrict__ in, TO *__restrict__ out)
{
    const TI *src = in + (int64_t)blockIdx.y * d.npix_in;
    TO *dst = out + (int64_t)blockIdx.y * d.npix_out;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < d.npix_out; q += (int64_t)gridDim.x * kThreads) {
        const int64_t P = d.nest_out ? q : ring2nest(d.nside_out, d.order_out, q);
        const int64_t Pp = P >> (2 * d.lr);
        const int64_t p = d.nest_in ? Pp : nest2ring(d.nside_in, d.order_in, Pp);
        dst[q] = (TO)((double)src[p] * d.ratio);
    }
}

struct Interp {
    Hpx h;
    int order;                              // log2 nside (nest only)
    int nest;
    int64_t n;
};

// the 4 neighbours and weights of point i; false (pixels -1, weights NaN) for theta outside [0, pi], a non-finite phi or a pixel
// index outside [0, npix).  phi is reduced to [0, 2 pi) first.  Pixel centres (ipix) take the pixel's own ring as the ring above,
// which is what the rule gives in exact arithmetic (a recomputed cos(theta) can land a rounding step above the ring).
__device__ inline bool interp_point(const Interp &a, const double *theta, const double *phi, const int64_t *ipix, int64_t i,
                                    int64_t pix[4], double w[4])
{
    bool ok;
    if (ipix) {
        int64_t p = ipix[i];
        ok = p >= 0 && p < a.h.npix;
        if (ok) {
            if (a.nest) p = nest2ring(a.h.nside, a.order, p);
            const int64_t ir = p < a.h.ncap ? (1 + isqrt_pix(1 + 2 * p)) >> 1
                             : p < a.h.npix - a.h.ncap ? (p - a.h.ncap) / (4 * a.h.nside) + a.h.nside
                             : 4 * a.h.nside - ((1 + isqrt_pix(2 * (a.h.npix - p) - 1)) >> 1);
            int64_t sp, nr; double th; bool sh;
            ring_info2(a.h, ir, sp, nr, th, sh);
            const double ph = ((double)(p - sp) + (sh ? 0.5 : 0.0)) * (kTwoPi / (double)nr);
            get_interpol_ring<true>(a.h, ir, th, ph, pix, w);
        }
    } else {
        const double th = theta[i];
        double ph = phi[i];
        ok = th >= 0.0 && th <= kPi && isfinite(ph);
        if (ok) {
            if (ph < 0.0 || ph >= kTwoPi) {
                ph = fmod(ph, kTwoPi);
                if (ph < 0.0) ph += kTwoPi;
                if (ph >= kTwoPi) ph -= kTwoPi;
            }
            get_interpol<true>(a.h, th, ph, pix, w);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (ok && (pix[k] < 0 || pix[k] >= a.h.npix)) ok = false;
    }
    if (!ok) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { pix[k] = -1; w[k] = __builtin_nan(""); }
        return false;
    }
    if (a.nest) {
#pragma unroll
        for (int k = 0; k < 4; ++k) pix[k] = ring2nest(a.h.nside, a.order, pix[k]);
    }
    return true;
}

// pix_out / w_out [4][n]
__global__ void __launch_bounds__(kThreads)
hpx_interp_weights_kernel(Interp a, const double *__restrict__ theta, const double *__restrict__ phi, const int64_t *__restrict__ ipix,
                          int64_t *__restrict__ pix_out, double *__restrict__ w_out)
{
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kThreads) {
        int64_t pix[4]; double w[4];
        interp_point(a, theta, phi, ipix, i, pix, w);
#pragma unroll
        for (int k = 0; k < 4; ++k) { pix_out[k * a.n + i] = pix[k]; w_out[k * a.n + i] = w[k]; }
    }
}

// out[m][i] = sum_k maps[m][pix_k] w_k, k = 0..3 in order; NaN where the point is invalid
template <typename TM>
__global__ void __launch_bounds__(kThreads)
hpx_interp_val_kernel(Interp a, int64_t nmaps, const TM *__restrict__ maps, const double *__restrict__ theta, const double *__restrict__ phi,
                      double *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kThreads) {
        int64_t pix[4]; double w[4];
        const bool ok = interp_point(a, theta, phi, nullptr, i, pix, w);
        for (int64_t m = 0; m < nmaps; ++m) {
            const TM *src = maps + m * a.h.npix;
            double v = __builtin_nan("");
            if (ok) v = (double)src[pix[0]] * w[0] + (double)src[pix[1]] * w[1] + (double)src[pix[2]] * w[2] + (double)src[pix[3]] * w[3];
            out[m * a.n + i] = v;
        }
    }
}

// hmap[pix[i][j]] += w[i][j] * vals[i] (pix, w: [n][4]); indices in [-npix, 0) wrap, anything else outside [0, npix) is skipped
__global__ void __launch_bounds__(kThreads)
hpx_scatter_add_kernel(int64_t npix, double *__restrict__ hmap, int64_t n, const double *__restrict__ vals, const int64_t *__restrict__ pix,
                       const double *__restrict__ w)
{
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < 4 * n; e += (int64_t)gridDim.x * kThreads) {
        int64_t p = pix[e];
        if (p < 0) p += npix;
        if (p >= 0 && p < npix) atomicAdd(hmap + p, w[e] * vals[e >> 2]);
    }
}

// out[8][n]: the neighbours of ipix[i] (pix_neighbours); -1 throughout for an index outside [0, npix)
__global__ void __launch_bounds__(kThreads)
hpx_neighbours_kernel(int64_t nside, int order, int nest, int64_t n, const int64_t *__restrict__ ipix, int64_t *__restrict__ out)
{
    const int64_t npix = 12 * nside * nside;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        const int64_t p = ipix[i];
        int64_t nb[8];
        if (p >= 0 && p < npix) {
            pix_neighbours(nside, order, nest, p, nb);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) nb[k] = -1;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) out[k * n + i] = nb[k];
    }
}

}  // namespace hpx
}  // namespace bfgx
