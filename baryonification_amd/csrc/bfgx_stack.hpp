// bfgx_stack.hpp -- halo-centred radial profiles of shell maps (MeasureProfilesShell): the adjoint of PaintProfilesShell.
//
// Per halo j the pixels of query_disc(NSIDE, vec_j, R_j epsilon_max / D_j) -- the discs, the ring rows and the separations of
// halo_pairs_kernel (bfgx_kernels.hpp) -- are GATHERED instead of painted: a pixel at x = r_sep / a_j (comoving Mpc) or r_sep / R_j
// (scaled) falls into bin b iff edges[b] <= x < edges[b + 1] and adds its value to sum[j, b] and 1 to npix[j, b]; a spin-2 pair (g1, g2)
// in the HEALPix convention (components on e_theta, e_phi) adds its tangential and cross components about the halo,
//     gamma_t + i gamma_x = -(g1 + i g2) e^{-2 i phi},
// phi the position angle of the great circle towards the halo at the pixel, measured from e_theta towards e_phi.
//
// One wave per halo.  One enumeration, one r_sep and one bin search per pair serve every map of the call.  The bins of the halo live in
// the wave's LDS while its pixels stream by (one StackBins per wave: the edges, the bin rule, the bins and their store are
// bfgx_stack_core.hpp's); when the disc is done lane b stores bin b of every output once.  No global atomics and no zero-fill: every
// (halo, bin) cell is written exactly once, also for a halo without pixels.  fp64 throughout.
#pragma once
#include "bfgx_stack_core.hpp"

namespace bfgx {

struct StackArgs {
    const double *map, *g1, *g2;              // RING maps (g1 == nullptr: no shear pair)
    const double *M, *z;                      // catalog columns: M <= 0 / non-finite or z <= -1 is an invalid halo (all-zero row)
    const double *edges;                      // nb + 1 ascending bin edges
    int32_t nb, scaled;                       // scaled: x = r_sep / R_j instead of r_sep / a_j
    StackOut out;                             // [nhalo][nb]
};

template <bool SHEAR>
struct StackWaveLds {
    RowLds rows;
    StackBins<SHEAR> bins;                    // (a disc holds fewer than 2^31 pixels: 12 * 8192^2 = 8.1e8)
};

// healpy.mask_bad's rule (what sht::unseen_to_zero applies), or not finite
__device__ inline bool stack_counts(double v)
{
    return isfinite(v) && !(fabs(v + 1.6375e30) <= 1e-8 + 1e-5 * 1.6375e30);
}

template <bool SHEAR>
__global__ void __launch_bounds__(kWave * kWavesPerBlock)
stack_profiles_kernel(Hpx h, Background bg, bfgx_massdef md, int64_t nhalo, const HaloRec *__restrict__ recs, StackArgs a)
{
    __shared__ StackWaveLds<SHEAR> lds[kWavesPerBlock];
    __shared__ double s_edges[kStackEdgeLds];
    stack_load_edges(s_edges, a.edges, a.nb, threadIdx.x, blockDim.x);
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1);
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int64_t j = (int64_t)blockIdx.x * kWavesPerBlock + wid;
    if (j >= nhalo) return;                      // whole wave exits together (no workgroup barrier below)
    RowLds &L = lds[wid].rows;
    StackBins<SHEAR> &B = lds[wid].bins;
    B.clear(lane);
    const HaloRec &r = recs[j];
    const double M_j = a.M[j], z_j = a.z[j];
    const bool bad = !(M_j > 0.0) || !isfinite(M_j) || !(z_j > -1.0);
    const double den = a.scaled ? dev_radius(bg, md, M_j, r.a) : r.a;     // x = r_sep / R_j or r_sep / a_j (HealpixRunner.py:441)
    const double e0 = s_edges[0];
    const int nb = a.nb;
    __builtin_amdgcn_wave_barrier();

    auto pair = [&](int64_t pix, double z, double sth, double phi_pix) {
        const double m = a.map[pix];
        double ga = 0.0, gb = 0.0;
        if (SHEAR) { ga = a.g1[pix]; gb = a.g2[pix]; }
        double sd, cd;
        sincos_dphi(phi_pix - r.phi0, sd, cd);
        const double vx = sth * cd, vy = sth * sd;
        const double dx = r.D * (vx - r.s0), dy = r.D * vy, dz = r.D * (z - r.z0);      // :435-437
        const double r_sep = sqrt(dx * dx + dy * dy + dz * dz);                         // :438
        const double x = r_sep / den;
        const int b = stack_find_bin(s_edges, e0, x, nb);
        if (b < 0) return;
        if (stack_counts(m)) B.add(b, m);
        if constexpr (SHEAR) if (stack_counts(ga) && stack_counts(gb)) {
            // tangent at the pixel towards the halo, on (e_theta, e_phi) = ((z cd, z sd, -sth), (-sd, cd, 0)):
            //   t_th = s0 z cd - z0 sth,  t_ph = -s0 sd.   t_th is a difference of nearly equal products for a nearby pixel: the two
            //   products carry their rounding errors along (two-product by fma), so that what is left is the rounding of the inputs
            const double p = r.s0 * z, pe = __builtin_fma(r.s0, z, -p);
            const double q = r.z0 * sth, qe = __builtin_fma(r.z0, sth, -q);
            const double t_th = __builtin_fma(p, cd, -q) + __builtin_fma(pe, cd, -qe);
            const double t_ph = -r.s0 * sd;
            const double n2 = t_th * t_th + t_ph * t_ph;
            if (n2 > 0.0) {                         // (the halo on the pixel centre has no position angle)
                const double inv = 1.0 / n2;
                const double c2 = (t_th - t_ph) * (t_th + t_ph) * inv, s2 = 2.0 * t_th * t_ph * inv;
                B.add_shear(b, -(ga * c2 + gb * s2), ga * s2 - gb * c2);
            }
        }
    };

    if (!bad) {
        for (int rbase = r.rfirst; rbase <= r.rlast; rbase += kWave) {
            const int ring = rbase + lane;
            RowSpan s;
            s.cnt = 0; s.lo = 0; s.start = 0; s.nr = 1; s.shifted = false; s.z = 0.0; s.sth = 0.0;
            if (ring <= r.rlast) disc_row(h, ring, r.z0, r.xa, r.cosr, r.phi0, r.irmin, r.irmax, s);
            const int incl = wave_scan_incl(s.cnt, lane);
            const int total = __shfl(incl, kWave - 1, kWave);
            L.prefix[lane] = incl - s.cnt;
            L.nr[lane] = (int)s.nr; L.lo[lane] = s.lo; L.start[lane] = s.start;
            L.z[lane] = s.z; L.sth[lane] = s.sth; L.shift[lane] = s.shifted ? 0.5 : 0.0;
            __builtin_amdgcn_wave_barrier();
            for (int t = lane; t < total; t += kWave) {
                int row = 0;                      // largest row with prefix[row] <= t
#pragma unroll
                for (int st = kWave >> 1; st > 0; st >>= 1)
                    if (L.prefix[row + st] <= t) row += st;
                const int nrr = L.nr[row];
                int k = L.lo[row] + (t - L.prefix[row]);
                if (k >= nrr) k -= nrr;
                pair(L.start[row] + k, L.z[row], L.sth[row], ((double)k + L.shift[row]) * (kTwoPi / (double)nrr));
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < nb) B.store(lane, j * nb + lane, a.out);
}

}  // namespace bfgx
