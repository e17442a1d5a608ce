// bfgx_snapshot_pairs.hpp -- per-(halo, particle) kernels of BaryonifySnapshot for models that are Python callables.
//
// The reference calls model.displacement(d, M_j, a_j) once per halo on the distances of the particles its periodic KD-tree finds
// within R_q (SnapshotRunner.py:217-245).  Here the particles are binned into a periodic cell grid (a stable radix sort by cell, so a
// cell lists its particles in ascending index), every halo walks the cells of its query ball's bounding cube with the exact fp64 test
// of the existing snapshot kernels (min-image separations, d^2 <= R_q^2), and the (halo, particle) pairs are sorted by halo, then by
// particle index: within a halo the model gets its particles in ascending index.
//
//   snap_pairs_prep_kernel   per-halo position, R_q^2 and cell cube (snap_halo_prep_kernel's geometry, no table)
//   snap_pairs_bin_kernel    per particle: cell key, the [0, L] check (flags bit 1), per-cell counts
//   snap_pairs_walk_kernel   one workgroup per halo: FILL = 0 counts its pairs, FILL = 1 writes halo << 32 | particle keys
//   snap_pairs_kernel        MODE 0: d of pairs [p0, p1); MODE 1: offset = value * a (non-finite -> 0) along the min-image unit
//                            vector, fp64 global atomics into the particle's accumulator (:228-245)
//   snap_pairs_finish_kernel position + accumulated offset, re-wrapped once (:254-262)
#pragma once
#include "bfgx_snapshot.hpp"

namespace bfgx {

__global__ void __launch_bounds__(256)
snap_pairs_prep_kernel(DevModel m, SnapGeom g, int64_t nh, const double *__restrict__ M, const double *__restrict__ hx,
                       const double *__restrict__ hy, const double *__restrict__ hz, SnapHaloRec *__restrict__ recs)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nh) return;
    SnapHaloRec r;
    const double M_j = M[j];
    r.pos[0] = hx[j]; r.pos[1] = hy[j]; r.pos[2] = (g.ndim == 3) ? hz[j] : 0.0;
    r.valid = (M_j > 0.0) && isfinite(M_j) && isfinite(r.pos[0]) && isfinite(r.pos[1]) && isfinite(r.pos[2]);
    r.Rq2 = 0.0; r.rcut = 0.0; r.lnoff = 0.0; r.oob = 0;
    for (int q = 0; q < kNC; ++q) { r.w[q] = 0.0; r.rowoff[q] = 0; }
    for (int q = 0; q < 3; ++q) { r.clo[q] = 0; r.cn[q] = 0; }
    if (r.valid) {
        const double a = g.a;
        double R_q = m.eps_runner * dev_radius(m.bg_runner, m.md_runner, M_j, a) / a;    // :220-221
        R_q = fmin(fmax(R_q, 0.0), g.L / 2);                                            // :222
        r.Rq2 = R_q * R_q;
        if (!(R_q >= 0.0) || !isfinite(R_q)) r.valid = 0;
        for (int ax = 0; ax < g.ndim && r.valid; ++ax) {                                 // as snap_halo_prep_kernel
            double p = r.pos[ax];
            p -= floor(p / g.L) * g.L;
            const double lo_v = p - R_q, hi_v = p + R_q;
            int cl = (int)floor(lo_v * g.inv_cell), ch = (int)floor(hi_v * g.inv_cell);
            if (lo_v <= 0.0) cl -= 1;
            if (hi_v >= g.L) ch += 1;
            int n = ch - cl + 1;
            if (n >= g.nc) { cl = 0; n = g.nc; }
            cl %= g.nc; if (cl < 0) cl += g.nc;
            r.clo[ax] = cl; r.cn[ax] = n;
        }
        if (g.ndim == 2) { r.clo[2] = 0; r.cn[2] = 1; }
    }
    recs[j] = r;
}

// flags: bit 1 = a particle lies outside [0, L] (scipy's periodic KDTree refuses such data)
__global__ void __launch_bounds__(256)
snap_pairs_bin_kernel(SnapGeom g, int64_t np, const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                      uint32_t *__restrict__ cell, uint32_t *__restrict__ idx, int32_t *__restrict__ cell_count, int32_t *__restrict__ flags)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= np) return;
    const double xi = x[i], yi = y[i], zi = (g.ndim == 3) ? z[i] : 0.0;
    if (!((xi >= 0.0 && xi <= g.L) && (yi >= 0.0 && yi <= g.L) && (g.ndim == 2 || (zi >= 0.0 && zi <= g.L)))) atomicOr(flags, 2);
    const int64_t c = snap_cell_index(g, snap_cell(xi, g), snap_cell(yi, g), (g.ndim == 3) ? snap_cell(zi, g) : 0);
    cell[i] = (uint32_t)c;
    idx[i] = (uint32_t)i;
    atomicAdd(cell_count + c, 1);
}

// min-image separation of particle i from halo r and its square, with the roundings of the reference's numpy (:224-228, :67-92)
template <int DIM>
__device__ inline double snap_sep(const SnapGeom &g, const SnapHaloRec &r, const double *x, const double *y, const double *z, int64_t i,
                                  double d[3])
{
    d[0] = min_image(x[i] - r.pos[0], g.L);
    d[1] = min_image(y[i] - r.pos[1], g.L);
    d[2] = (DIM == 3) ? min_image(z[i] - r.pos[2], g.L) : 0.0;
    double d2 = add_nc(mul_nc(d[0], d[0]), mul_nc(d[1], d[1]));
    if (DIM == 3) d2 = add_nc(d2, mul_nc(d[2], d[2]));
    return d2;
}

template <int DIM, int FILL>
__global__ void __launch_bounds__(256)
snap_pairs_walk_kernel(SnapGeom g, int64_t nh, const SnapHaloRec *__restrict__ recs, const double *__restrict__ x, const double *__restrict__ y,
                       const double *__restrict__ z, const int32_t *__restrict__ cell_start, const uint32_t *__restrict__ cell_idx,
                       int64_t *__restrict__ counts, const int64_t *__restrict__ off, int64_t *__restrict__ cursor, uint64_t *__restrict__ keys)
{
    __shared__ long long wsum[256 / kWave];
    for (int64_t j = blockIdx.x; j < nh; j += gridDim.x) {
        const SnapHaloRec &r = recs[j];
        long long cnt = 0;
        if (r.valid) {
            const int ncube = r.cn[0] * r.cn[1] * r.cn[2];
            for (int c = threadIdx.x; c < ncube; c += 256) {                     // a thread per cell of the cube, its particles in turn
                const int64_t cc = snap_cube_cell(g, r, c);
                const int s0 = cell_start[cc], s1 = cell_start[cc + 1];
                for (int s = s0; s < s1; ++s) {
                    const uint32_t i = cell_idx[s];
                    double d[3];
                    if (!(snap_sep<DIM>(g, r, x, y, z, i, d) <= r.Rq2)) continue;
                    if (FILL) keys[off[j] + atomicAdd((unsigned long long *)(cursor + j), 1ull)] = ((uint64_t)j << 32) | i;
                    else ++cnt;
                }
            }
        }
        if (!FILL) {
#pragma unroll
            for (int s = kWave >> 1; s > 0; s >>= 1) cnt += __shfl_down(cnt, s, kWave);
            if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x / kWave] = cnt;
            __syncthreads();
            if (threadIdx.x == 0) {
                int64_t t = 0;
                for (int w = 0; w < 256 / kWave; ++w) t += wsum[w];
                counts[j] = t;
            }
            __syncthreads();
        }
    }
}

// MODE 0: d of pairs [p0, p1) -> out[p - p0];  MODE 1: vals[p - p0] -> offsets into acc[3 * particle]
template <int DIM, int MODE>
__global__ void __launch_bounds__(256)
snap_pairs_kernel(SnapGeom g, const SnapHaloRec *__restrict__ recs, const double *__restrict__ x, const double *__restrict__ y,
                  const double *__restrict__ z, const uint64_t *__restrict__ keys, int64_t p0, int64_t p1, const double *__restrict__ vals,
                  double *__restrict__ out)
{
    for (int64_t p = p0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < p1; p += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t key = keys[p];
        const int64_t j = (int64_t)(key >> 32), i = (int64_t)(key & 0xffffffffull);
        double d[3];
        const double dd = __dsqrt_rn(snap_sep<DIM>(g, recs[j], x, y, z, i, d));      // :228 compute_distance
        if (MODE == 0) { out[p - p0] = dd; continue; }
        double o = mul_nc(vals[p - p0], g.a);                                       // :240 displacement * a_j
        if (!isfinite(o)) o = 0.0;                                                  // :241
        // offset * (dx / d): a NaN at d = 0 is added as it is, an exact zero changes nothing
        for (int ax = 0; ax < DIM; ++ax) {
            const double c = o * (d[ax] / dd);
            if (c != 0.0) atomicAdd(out + 3 * i + ax, c);
        }
    }
}

__global__ void __launch_bounds__(256)
snap_pairs_finish_kernel(SnapGeom g, int64_t np, const double *__restrict__ acc, const double *__restrict__ x, const double *__restrict__ y,
                         const double *__restrict__ z, double *__restrict__ ox, double *__restrict__ oy, double *__restrict__ oz)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= np) return;
    const double *in[3] = {x, y, z};
    double *o[3] = {ox, oy, oz};
    for (int ax = 0; ax < g.ndim; ++ax) {
        double v = in[ax][i] + acc[3 * i + ax];                                     // :254-256
        if (v > g.L) v -= g.L;                                                      // :258-262
        if (v < 0.0) v += g.L;
        o[ax][i] = v;
    }
}

}  // namespace bfgx
