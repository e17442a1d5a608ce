// bfgx_snapshot_stack.hpp -- halo-centred radial profiles of particle snapshots (MeasureProfilesSnapshot): the box counterpart of
// bfgx_stack.hpp.
//
// Per halo j the particles of BaryonifySnapshot's query ball -- minimum-image separation d with the roundings of the reference's numpy
// (snap_sep), d^2 <= R_q^2, R_q = clip(epsilon_max R_j / a, 0, L / 2) (snap_pairs_prep_kernel) -- are binned in x = d (comoving Mpc) or,
// scaled, x = d / (R_j / a): a particle falls into bin b iff edges[b] <= x < edges[b + 1], adds 1 to npart[j, b] and, when its weight is
// finite, its weight to sum[j, b].
//
// The particles are binned into the periodic cell grid of the per-pair route (snap_bin_particles: count, scan, stable sort by cell) and
// gathered into cell order once (snap_stack_gather_kernel).  The cells of a halo's cube along the LAST axis are consecutive in the cell
// index, so one (cx[, cy]) column of the cube is one contiguous run of sorted particles -- two where the column wraps around the box.
//
//   snap_stack_kernel   one workgroup per halo (grid-stride over halos).  256 columns at a time: thread t looks up the one or two runs of
//                       column t, a workgroup scan turns the run lengths into the prefix of their concatenation, and thread t takes
//                       particles t, t + 256, ... of it: lanes map to particles, consecutive lanes read consecutive records, and no
//                       lane waits behind the fullest cell.  The bins of the halo live in LDS while the particles stream by (one
//                       StackBins per workgroup; the scan, the edges, the bin rule, the bins and their store are
//                       bfgx_stack_core.hpp's; a particle is in a halo's ball at most once, R_q <= L / 2, so a 32-bit count stays
//                       below the 2^32 particles of a call); when the halo is done thread b stores bin b of each output once.  No global atomics and no zero-fill: every
//                       (halo, bin) cell is written exactly once, also for invalid halos and halos without particles.  Counts are
//                       exact and reproducible; fp64 throughout.
#pragma once
#include "bfgx_snapshot_pairs.hpp"
#include "bfgx_stack_core.hpp"

namespace bfgx {

constexpr int kSnapStackThreads = 256;
constexpr int kSnapStackSlots = 2 * kSnapStackThreads;       // two runs per column: a column that wraps around the box

struct SnapStackArgs {
    const double *x, *y, *z, *w;              // particle records in cell order (w == nullptr: counts only)
    const uint32_t *cell_start;               // ncell + 1 exclusive prefix of the per-cell counts (32-bit sums, read unsigned)
    const double *M;                          // halo masses (the scaled abscissa needs R_j)
    const double *edges;                      // nb + 1 ascending bin edges
    int32_t nb, scaled;
    StackOut out;                             // [nhalo][nb]: npix = npart; sum is nullptr without weights; no shear members
};

__global__ void __launch_bounds__(256)
snap_stack_gather_kernel(int64_t np, const uint32_t *__restrict__ idx, const double *__restrict__ x, const double *__restrict__ y,
                         const double *__restrict__ z, const double *__restrict__ w, double *__restrict__ xs, double *__restrict__ ys,
                         double *__restrict__ zs, double *__restrict__ ws)
{
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= np) return;
    const uint32_t i = idx[s];
    xs[s] = x[i];
    ys[s] = y[i];
    if (z) zs[s] = z[i];
    if (w) ws[s] = w[i];
}

struct SnapStackLds {
    uint32_t prefix[kSnapStackSlots];         // exclusive prefix of the run lengths of this round
    uint32_t start[kSnapStackSlots];          // first sorted particle of each run
    StackBins<false> bins;
    uint32_t wtot[kSnapStackThreads / kWave];
    double edges[kStackEdgeLds];
};

template <int DIM, bool WEIGHTS>
__global__ void __launch_bounds__(kSnapStackThreads)
snap_stack_kernel(SnapGeom g, Background bg, bfgx_massdef md, int64_t nh, const SnapHaloRec *__restrict__ recs, SnapStackArgs a)
{
    __shared__ SnapStackLds S;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    stack_load_edges(S.edges, a.edges, a.nb, tid, kSnapStackThreads);
    const int nb = a.nb, nc = g.nc;
    for (int64_t j = blockIdx.x; j < nh; j += gridDim.x) {                  // (every branch on r or j below is uniform over the workgroup)
        const SnapHaloRec &r = recs[j];
        if (tid < kStackMaxBins) S.bins.clear(tid);
        __syncthreads();
        const double e0 = S.edges[0];
        // x = d / (R_j / a) or d: R_j / a as the prep kernel's R_q has it, before epsilon_max and the clipping
        const double den = (a.scaled && r.valid) ? dev_radius(bg, md, a.M[j], g.a) / g.a : 1.0;
        const int nlast = r.cn[DIM - 1], clast = r.clo[DIM - 1];
        const int ncol = r.valid ? ((DIM == 3) ? r.cn[0] * r.cn[1] : r.cn[0]) : 0;
        for (int base = 0; base < ncol; base += kSnapStackThreads) {
            const int col = base + tid;
            uint32_t sA = 0, cA = 0, sB = 0, cB = 0;
            if (col < ncol) {
                int64_t row;                                                    // cell index of the column's cell 0 on the last axis
                if (DIM == 3) {
                    const int iy = col % r.cn[1], ix = col / r.cn[1];
                    int cx = r.clo[0] + ix; cx -= (cx >= nc) ? nc : 0;
                    int cy = r.clo[1] + iy; cy -= (cy >= nc) ? nc : 0;
                    row = ((int64_t)cx * nc + cy) * nc;
                } else {
                    int cx = r.clo[0] + col; cx -= (cx >= nc) ? nc : 0;
                    row = (int64_t)cx * nc;
                }
                const int end = clast + nlast;                                  // (the whole axis: clast = 0, nlast = nc)
                sA = a.cell_start[row + clast];
                cA = a.cell_start[row + min(end, nc)] - sA;
                if (end > nc) {                                                 // the column wraps: cells [0, end - nc) too
                    sB = a.cell_start[row];
                    cB = a.cell_start[row + (end - nc)] - sB;
                }
            }
            uint32_t excl, total;
            block_ragged_prefix<kSnapStackThreads>(cA + cB, lane, wid, S.wtot, excl, total);
            S.prefix[2 * tid] = excl; S.prefix[2 * tid + 1] = excl + cA;
            S.start[2 * tid] = sA; S.start[2 * tid + 1] = sB;
            __syncthreads();
            for (uint64_t tt = tid; tt < total; tt += kSnapStackThreads) {
                const uint32_t t = (uint32_t)tt;
                const int slot = ragged_find<kSnapStackSlots>(S.prefix, t);
                const int64_t p = (int64_t)S.start[slot] + (t - S.prefix[slot]);
                double d[3];
                const double d2 = snap_sep<DIM>(g, r, a.x, a.y, a.z, p, d);
                if (!(d2 <= r.Rq2)) continue;
                const double dd = __dsqrt_rn(d2);
                const double xv = a.scaled ? dd / den : dd;
                const int b = stack_find_bin(S.edges, e0, xv, nb);
                if (b < 0) continue;
                S.bins.count(b);
                if (WEIGHTS) {
                    const double wv = a.w[p];
                    if (isfinite(wv)) S.bins.add_sum(b, wv);
                }
            }
            __syncthreads();                                                    // the round's runs and the bins are settled
        }
        if (tid < nb) S.bins.store(tid, j * nb + tid, a.out, WEIGHTS);
    }
}

}  // namespace bfgx
