// bfgx_grid_stack.hpp -- halo-centred radial profiles of gridded maps (MeasureProfilesGrid): the regular-grid counterpart of bfgx_stack.hpp
// and bfgx_snapshot_stack.hpp.
//
// Geometry.  map[i0, i1(, i2)] is the pixel whose centre is (x, y(, z)) = (bins[i0], bins[i1](, bins[i2])): where the grid runners put a
// halo and what ParticleSnapshot.make_map produces.  res = bins[1] - bins[0], period L = npix res, a = 1 / (1 + redshift).  A halo is valid
// iff M > 0 and M and its coordinates in use are finite (grid_pairs_prep_kernel's rule); R_com = dev_radius(M, a) / a and
// R_q = clip(epsilon_max R_com, 0, max(bins) / 2) (BaryonifyGrid's clip, GridGeom::half_box).  Per axis Delta_k = bins[i_k] - x_k, minus L
// where Delta_k > L / 2, plus L where Delta_k < -L / 2; d = sqrt(sum Delta_k^2) is the TRUE minimum-image distance -- not the reference's
// cutout linspace(-N/2, N/2, N) res, which stretches radii by N / (N - 1) and swaps the sub-pixel dx and dy: a measurement inherits neither.
// A pixel belongs to halo j iff d^2 <= R_q^2 (R_q < L / 2: at most once); x = d or, scaled, d / R_com; bin b holds
// edges[b] <= x < edges[b + 1].  A finite map value adds 1 to npix[j, b] and its value to sum[j, b].  With a shear pair (2-D) a pixel with
// finite g1 and g2 and d > 0 adds 1 to npix_shear and
//     gamma_t = -(g1 c2 + g2 s2),  gamma_x = g1 s2 - g2 c2,  c2 = (Dx^2 - Dy^2) / d^2,  s2 = 2 Dx Dy / d^2
// (gamma_t + i gamma_x = -(g1 + i g2) e^{-2 i phi}, phi from +x towards +y; a mass peak has gamma_t > 0) to sum_t / sum_x.
//
//   grid_stack_prep_kernel   per halo: valid, R_com, R_q^2, the nearest centre pixel per axis (nearest_bin) and the visited offsets around
//                            it, [-w, w] with w = floor(R_q / res) + 1 -- or, where 2 w + 1 >= npix (or the halo lies off the grid), the
//                            WHOLE axis exactly once: a wrapped pixel visited twice would be counted twice.
//   grid_stack_kernel        one 256-thread workgroup per halo (grid-stride over halos).  A row is the run of visited pixels along the
//                            LAST axis (contiguous in memory; two runs where it wraps) at one (i0[, i1]).  256 rows at a time: thread t
//                            clips row t to the chord of the ball, |Delta_last| <= sqrt(R_q^2 - sum of the other Delta^2) widened by one
//                            pixel (no lanes for the cube's corners, 48 % of a 3-D cube); a workgroup scan turns the chord lengths
//                            into the prefix of their concatenation and thread t takes pixels t, t + 256, ... of it: lanes run along
//                            the last axis and no lane waits behind the longest row.  The exact d^2 <= R_q^2 test decides membership.
//                            The bins of the halo live in LDS (one StackBins per workgroup; the scan, the edges, the bin rule, the bins
//                            and their store are bfgx_stack_core.hpp's; a grid holds fewer than 2^32 pixels, so a 32-bit count cannot
//                            overflow); when the halo is done thread b stores bin b of each output once.  No global atomics and no zero-fill: every (halo, bin) cell of every output is
//                            written exactly once, also for invalid halos and halos without pixels.  int64 pixel indices, fp64 throughout.
#pragma once
#include "bfgx_grid.hpp"
#include "bfgx_stack_core.hpp"

namespace bfgx {

constexpr int kGridStackThreads = 256;

struct GridStackRec {
    double pos[3];                    // halo position by ARRAY axis: (x, y, z)
    double dcen[3];                   // bins[cen] - pos
    double R, Rq2;                    // R_com; R_q^2
    int32_t cen[3];                   // nearest centre pixel
    int32_t mlo[3], n[3];             // visited offsets from cen: mlo .. mlo + n - 1 (n <= npix; an axis not in use: 0, 1)
    int32_t valid;
    int32_t clip;                     // the last axis is a window around an on-grid halo: offset m lies at m res + dcen, unwrapped
};

struct GridStackArgs {
    const double *map, *g1, *g2;      // [npix]^ndim, C order (g1 == nullptr: no shear pair)
    const double *edges;              // nb + 1 ascending bin edges
    int32_t nb, scaled;
    StackOut out;                     // [nhalo][nb]
};

__device__ inline double grid_min_image(double d, double L, double Lh)
{
    d -= (d > Lh) ? L : 0.0;
    d += (d < -Lh) ? L : 0.0;
    return d;
}

__global__ void __launch_bounds__(kGridBlock)
grid_stack_prep_kernel(Background bg, bfgx_massdef md, double eps, GridGeom g, int64_t nh, const double *__restrict__ M,
                       const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z, GridStackRec *__restrict__ recs)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nh) return;
    GridStackRec r;
    for (int k = 0; k < 3; ++k) { r.pos[k] = 0.0; r.dcen[k] = 0.0; r.cen[k] = 0; r.mlo[k] = 0; r.n[k] = 1; }
    r.R = 0.0; r.Rq2 = 0.0; r.valid = 0; r.clip = 0;
    const double M_j = M[j];
    const double pos[3] = {x[j], y[j], (g.ndim == 3) ? z[j] : 0.0};
    if ((M_j > 0.0) && isfinite(M_j) && isfinite(pos[0]) && isfinite(pos[1]) && isfinite(pos[2])) {
        const int N = g.npix;
        const double R_com = dev_radius(bg, md, M_j, g.a) / g.a;
        const double R_q = fmin(fmax(eps * R_com, 0.0), g.half_box);
        const double wq = floor(R_q / g.res) + 1.0;
        const int w = (wq < (double)N) ? (int)wq : N;
        r.valid = 1; r.clip = 1; r.R = R_com; r.Rq2 = R_q * R_q;
        for (int k = 0; k < g.ndim; ++k) {
            const int c = nearest_bin(g.bins, N, pos[k]);
            const double dc = g.bins[c] - pos[k];
            // on the grid |dc| <= res / 2 (a float32 coordinate at the box's end: a little more) and offset m lies at m res + dc, so the
            // pixels of the ball have |m| <= R_q / res + 3 / 4 < w + 1
            const bool off = !(fabs(dc) <= 0.75 * g.res);
            const bool whole = off || 2 * w + 1 >= N;
            r.pos[k] = pos[k]; r.dcen[k] = dc; r.cen[k] = c;
            r.mlo[k] = whole ? -(N / 2) : -w;
            r.n[k] = whole ? N : 2 * w + 1;
            if (k == g.ndim - 1 && whole) r.clip = 0;       // (a whole axis wraps: the chord is not one run of offsets)
        }
    }
    recs[j] = r;
}

template <bool SHEAR>
struct GridStackLds {
    uint32_t prefix[kGridStackThreads];       // exclusive prefix of the chord lengths of this round
    int32_t m0[kGridStackThreads];            // first offset of each chord on the last axis
    int64_t base[kGridStackThreads];          // pixel index of the row's pixel 0 on the last axis
    double s01[kGridStackThreads];            // sum of the other axes' Delta^2
    double d0[kGridStackThreads];             // Delta of axis 0 (the shear's Dx)
    StackBins<SHEAR> bins;
    uint32_t wtot[kGridStackThreads / kWave];
    double edges[kStackEdgeLds];
};

template <int DIM, bool SHEAR>
__global__ void __launch_bounds__(kGridStackThreads)
grid_stack_kernel(GridGeom g, int64_t nh, const GridStackRec *__restrict__ recs, GridStackArgs a)
{
    static_assert(DIM == 3 || DIM == 2, "2-D or 3-D grids");
    static_assert(!SHEAR || DIM == 2, "the shear pair is flat-sky: 2-D grids only");
    __shared__ GridStackLds<SHEAR> S;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    stack_load_edges(S.edges, a.edges, a.nb, tid, kGridStackThreads);
    const int nb = a.nb, N = g.npix;
    const double L = (double)N * g.res, Lh = 0.5 * L;
    constexpr int LA = DIM - 1;                                                 // the last axis
    for (int64_t j = blockIdx.x; j < nh; j += gridDim.x) {                      // (every branch on r or j below is uniform over the workgroup)
        const GridStackRec &r = recs[j];
        if (tid < kStackMaxBins) S.bins.clear(tid);
        __syncthreads();
        const double e0 = S.edges[0];
        const double den = (a.scaled && r.valid) ? r.R : 1.0;
        const double Rq2 = r.Rq2, xl = r.pos[LA], dl = r.dcen[LA];
        const int cl = r.cen[LA], ml = r.mlo[LA], nl = r.n[LA];
        const int nrow = r.valid ? ((DIM == 3) ? r.n[0] * r.n[1] : r.n[0]) : 0;
        for (int rbase = 0; rbase < nrow; rbase += kGridStackThreads) {
            const int row = rbase + tid;
            uint32_t cnt = 0;
            if (row < nrow) {
                const int i0 = (DIM == 3) ? row / r.n[1] : row;
                int p0 = r.cen[0] + r.mlo[0] + i0; p0 += (p0 < 0) ? N : 0; p0 -= (p0 >= N) ? N : 0;
                const double D0 = grid_min_image(g.bins[p0] - r.pos[0], L, Lh);
                double s01 = D0 * D0;
                int64_t base = (int64_t)p0 * N;
                if (DIM == 3) {
                    int p1 = r.cen[1] + r.mlo[1] + (row - i0 * r.n[1]); p1 += (p1 < 0) ? N : 0; p1 -= (p1 >= N) ? N : 0;
                    const double D1 = grid_min_image(g.bins[p1] - r.pos[1], L, Lh);
                    s01 += D1 * D1;
                    base = (base + p1) * N;
                }
                if (s01 <= Rq2) {                                               // (else no pixel of the row is in the ball: d^2 >= s01)
                    int kA = 0, kB = nl - 1;
                    if (r.clip) {                                               // offsets m with |m res + dl| <= chord / 2 + res
                        const double half = __dsqrt_rn(Rq2 - s01) + g.res;
                        kA = max(kA, (int)ceil((-half - dl) / g.res) - ml);
                        kB = min(kB, (int)floor((half - dl) / g.res) - ml);
                    }
                    cnt = (uint32_t)max(0, kB - kA + 1);
                    S.m0[tid] = ml + kA; S.base[tid] = base; S.s01[tid] = s01; S.d0[tid] = D0;
                }
            }
            uint32_t excl, total;
            block_ragged_prefix<kGridStackThreads>(cnt, lane, wid, S.wtot, excl, total);
            S.prefix[tid] = excl;
            __syncthreads();
            for (uint32_t t = tid; t < total; t += kGridStackThreads) {
                const int slot = ragged_find<kGridStackThreads>(S.prefix, t);
                int p = cl + S.m0[slot] + (int)(t - S.prefix[slot]); p += (p < 0) ? N : 0; p -= (p >= N) ? N : 0;
                const int64_t pix = S.base[slot] + p;
                const double v = a.map[pix];
                double ga = 0.0, gb = 0.0;
                if (SHEAR) { ga = a.g1[pix]; gb = a.g2[pix]; }
                const double Dl = grid_min_image(g.bins[p] - xl, L, Lh);
                const double d2 = S.s01[slot] + Dl * Dl;
                if (!(d2 <= Rq2)) continue;
                const double dd = __dsqrt_rn(d2);
                const double xv = a.scaled ? dd / den : dd;
                const int b = stack_find_bin(S.edges, e0, xv, nb);
                if (b < 0) continue;
                if (isfinite(v)) S.bins.add(b, v);
                if constexpr (SHEAR) if (isfinite(ga) && isfinite(gb) && d2 > 0.0) {   // (the halo on the pixel centre has no position angle)
                    const double Dx = S.d0[slot], inv = 1.0 / d2;
                    const double c2 = (Dx - Dl) * (Dx + Dl) * inv, s2 = 2.0 * Dx * Dl * inv;
                    S.bins.add_shear(b, -(ga * c2 + gb * s2), ga * s2 - gb * c2);
                }
            }
            __syncthreads();                                                    // the round's chords and the bins are settled
        }
        if (tid < nb) S.bins.store(tid, j * nb + tid, a.out);
    }
}

}  // namespace bfgx
