// bfgx_grid_pairs.hpp -- per-(halo, pixel) kernels of the regular-grid runners for models that are Python callables.
//
// The reference's BaryonifyGrid / PaintProfilesGrid call the model once per halo on r_grid.flatten() of the halo's WHOLE
// Nsize^d cutout (Map2DRunner.py:534, :577, :801).  These kernels make that cutout's radii for a range of halos, in the
// reference's flatten order, and turn the values the caller's model returned into pixel offsets / painted values:
//
//   grid_pairs_prep_kernel    per-halo cutout geometry of grid_prep_kernel (Nsize, centre pixels, {dy, dx, dz}, linspace
//                             step / start / top, shear matrix) with no table and no clipping to a ball: a callable declares
//                             no cut, so every pixel of the cube is a pair; counts[j] = Nsize^d (0: halo skipped, :498)
//   grid_pairs_items_kernel   the work-item table: halo j owns items [item0[j], item0[j + 1]) of kGridChunk pairs each
//   grid_pairs_kernel         MODE 0: r (sheared with use_ellipticity, :525-530) of the pairs of items [it_lo, it_hi);
//                             MODE 1: offset = value / res along the unsheared unit vector (:534-536, :577-579);
//                             MODE 2: value where isfinite(value) & (r < eps * R_j) (:800-812).  fp64 global atomics
//
// Pair p of halo j is element p - off[j] of the halo's r_grid.flatten(): cutout index (i, jj[, k]) in C order, first axis
// indexed around x_cen and paired with the y coordinate (meshgrid indexing='xy').  The radii are computed with numpy's
// roundings (cutout_coord, add_nc / mul_nc), so without ellipticity they equal the reference's bit for bit.  A non-finite
// offset is accumulated as it is: the post-loop isfinite() of the reference zeroes that pixel's whole total (:580, :591),
// which the grid regrid kernel does.
#pragma once
#include "bfgx_grid.hpp"

namespace bfgx {

// the head of GridHaloRec these kernels read (the table corners behind it are not used)
constexpr int kGridRecHeadWords = (int)(offsetof(GridHaloRec, w) / 4);

// flags: bit 0 = the reference's "Halo offsets ... larger than res" assert (2D maps, :516, :747)
__global__ void __launch_bounds__(kGridBlock)
grid_pairs_prep_kernel(DevModel m, GridGeom g, GridCatalog c, int mode, GridHaloRec *__restrict__ recs, int64_t *__restrict__ counts,
                       int32_t *__restrict__ flags)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= c.n) return;
    GridHaloRec r;
    r.nsize = 0; r.nchunks = 0; r.chunk0 = 0; r.oob = 0; r.ell = 0;
    for (int q = 0; q < 3; ++q) { r.dax[q] = 0.0; r.cen[q] = 0; r.lo[q] = 0; r.n[q] = 0; }
    for (int q = 0; q < 4; ++q) r.rmat[q] = 0.0;
    for (int q = 0; q < kNCmax; ++q) { r.w[q] = 0.0; r.rowoff[q] = 0; }      // (not read here; kept defined)
    r.step = r.start = r.top = r.rcut = r.lnoff = 0.0;

    const double M_j = c.M[j], x_j = c.x[j], y_j = c.y[j], z_j = (g.ndim == 3) ? c.z[j] : 0.0;
    const double a = g.a;
    const bool valid = (M_j > 0.0) && isfinite(M_j) && isfinite(x_j) && isfinite(y_j) && isfinite(z_j);
    double Ns = 0.0, R_com = 0.0;
    if (valid) {
        const double R_phys = dev_radius(m.bg_runner, m.md_runner, M_j, a);       // physical Mpc (:486, :718)
        R_com = R_phys / a;
        if (mode == 0) {
            double R_q = m.eps_runner * R_phys / a;                               // :487
            R_q = fmin(fmax(R_q, 0.0), g.half_box);                               // :488
            Ns = 2.0 * R_q / g.res;                                               // :496
        } else {
            Ns = 2.0 * m.eps_runner * R_com / g.res;                              // :726
        }
    }
    int nsize = 0;
    if (valid && isfinite(Ns)) {
        const double half = floor(Ns * 0.5);                                      // int(Nsize // 2) * 2
        nsize = (half > 1.0e6) ? 2000000 : 2 * (int)half;
        if (mode == 0) { if (nsize < 2) nsize = 0; }                              // :498 skip
        else nsize = max(2, min(nsize, g.npix / 2));                              // :728
        if (nsize > g.npix) nsize = g.npix - (g.npix & 1);
    }
    int64_t count = 0;
    if (nsize >= 2) {
        r.nsize = nsize;
        r.start = -(double)nsize / 2.0;
        r.top = (double)nsize / 2.0;
        r.step = (r.top - r.start) / (double)(nsize - 1);
        r.cen[0] = nearest_bin(g.bins, g.npix, x_j);
        r.cen[1] = nearest_bin(g.bins, g.npix, y_j);
        r.cen[2] = (g.ndim == 3) ? nearest_bin(g.bins, g.npix, z_j) : 0;
        const double dx = g.bins[r.cen[0]] - x_j, dy = g.bins[r.cen[1]] - y_j;
        const double dz = (g.ndim == 3) ? g.bins[r.cen[2]] - z_j : 0.0;
        r.dax[0] = dy; r.dax[1] = dx; r.dax[2] = dz;
        if (g.ndim == 2 && !(dx <= g.res && dy <= g.res)) atomicOr(flags, 1);
        r.rcut = R_com * m.eps_runner;                                            // MODE 1's mask radius (:800)
        if (c.rmat) { r.ell = 1; for (int q = 0; q < 4; ++q) r.rmat[q] = c.rmat[4 * j + q]; }
        count = (int64_t)nsize * nsize * (g.ndim == 3 ? nsize : 1);
    }
    recs[j] = r;
    counts[j] = count;
}

__global__ void __launch_bounds__(kGridBlock)
grid_pairs_items_kernel(int64_t n, const int64_t *__restrict__ item0, int32_t *__restrict__ item_halo)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    for (int64_t q = item0[j]; q < item0[j + 1]; ++q) item_halo[q] = (int32_t)j;
}

// MODE 0: pairs' radii -> out[pair - base];  MODE 1: offsets from vals[pair - base] into out[3 * pixel];  MODE 2: painted vals into out[pixel]
template <int DIM, int MODE>
__global__ void __launch_bounds__(kGridBlock)
grid_pairs_kernel(GridGeom g, const GridHaloRec *__restrict__ recs, const int32_t *__restrict__ item_halo, const int64_t *__restrict__ item0,
                  const int64_t *__restrict__ off, int64_t it_lo, int64_t it_hi, int64_t base, const double *__restrict__ vals,
                  double *__restrict__ out)
{
    __shared__ GridHaloRec R;
    __shared__ int64_t s_first, s_end;
    for (int64_t item = it_lo + blockIdx.x; item < it_hi; item += gridDim.x) {
        __syncthreads();
        const int32_t h = item_halo[item];
        {
            const int32_t *src = reinterpret_cast<const int32_t *>(recs + h);
            int32_t *dst = reinterpret_cast<int32_t *>(&R);
            for (int t = threadIdx.x; t < kGridRecHeadWords; t += kGridBlock) dst[t] = src[t];
            if (threadIdx.x == 0) {                                               // the item's pairs, as indices into the batch
                const int64_t first = (item - item0[h]) * kGridChunk, hb = off[h] - base;
                s_first = hb + first;
                s_end = hb + min(off[h + 1] - off[h], first + kGridChunk);
            }
        }
        __syncthreads();
        const int64_t p0 = s_first, p1 = s_end, hb = off[h] - base;
        const int n = R.nsize, wdt = n >> 1, N = g.npix;
        for (int64_t p = p0 + (int64_t)threadIdx.x; p < p1; p += kGridBlock) {
            const int64_t t = p - hb;                                             // index into the halo's r_grid.flatten()
            const int k = (DIM == 3) ? (int)(t % n) : 0;
            const int64_t q = (DIM == 3) ? t / n : t;
            const int i = (int)(q / n), jj = (int)(q % n);
            // meshgrid(x, x[, x], indexing='xy'): x_grid[i, j, k] = x[j], y_grid = x[i], z_grid = x[k]
            const double Y = cutout_coord(i, n, R.step, R.start, R.top, g.res) + R.dax[0];
            const double X = cutout_coord(jj, n, R.step, R.start, R.top, g.res) + R.dax[1];
            const double Z = (DIM == 3) ? cutout_coord(k, n, R.step, R.start, R.top, g.res) + R.dax[2] : 0.0;
            double r2 = add_nc(mul_nc(X, X), mul_nc(Y, Y));
            if (DIM == 3) r2 = add_nc(r2, mul_nc(Z, Z));
            const double rr = __dsqrt_rn(r2);                                     // :519, :556
            double r_eval = rr;
            if (DIM == 2 && R.ell) {                                              // (N, 2) @ Rmat, :525-530
                const double Xe = X * R.rmat[0] + Y * R.rmat[2], Ye = X * R.rmat[1] + Y * R.rmat[3];
                r_eval = __dsqrt_rn(add_nc(mul_nc(Xe, Xe), mul_nc(Ye, Ye)));
            }
            if (MODE == 0) { out[p] = r_eval; continue; }
            int pi = R.cen[0] - wdt + i, pj = R.cen[1] - wdt + jj, pk = (DIM == 3) ? R.cen[2] - wdt + k : 0;   // pick_indices
            pi += (pi < 0) ? N : 0; pi -= (pi >= N) ? N : 0;
            pj += (pj < 0) ? N : 0; pj -= (pj >= N) ? N : 0;
            if (DIM == 3) { pk += (pk < 0) ? N : 0; pk -= (pk >= N) ? N : 0; }
            const int64_t flat = (DIM == 3) ? ((int64_t)pi * N + pj) * N + pk : (int64_t)pi * N + pj;
            const double v = vals[p];
            if (MODE == 1) {
                const double o = v / g.res;                                       // :534, :569
                // an exact zero changes nothing; a NaN (0 / 0 unit vector at r = 0, or the model's own) is added as it is
                const double cx = o * (X / rr), cy = o * (Y / rr);
                if (cx != 0.0) atomicAdd(out + DIM * flat + 0, cx);
                if (cy != 0.0) atomicAdd(out + DIM * flat + 1, cy);
                if (DIM == 3) { const double cz = o * (Z / rr); if (cz != 0.0) atomicAdd(out + DIM * flat + 2, cz); }
            } else {
                if (isfinite(v) && r_eval < R.rcut && v != 0.0) atomicAdd(out + flat, v);      // :800-812
            }
        }
    }
}

}  // namespace bfgx
