// bfgx_sht.hpp -- spherical-harmonic transforms of RING-ordered HEALPix maps in fp64 for gfx950: scalar (spin 0: healpy.map2alm /
// alm2map / alm2cl / anafast, the last step of reference notebooks 04, 05 and 09) and spin-weighted (healpy.map2alm_spin /
// alm2map_spin, weak lensing of shells; the spin Legendre stage is described above sht_spin_legendre_analysis_kernel).
//
// Two stages per transform:
//  * ring stage, one workgroup per ring: a ring of n = 4k pixels (k = ring number in the caps, nside in the belt) is split into
//    its four interleaved sub-sequences of length k; each pair of them is packed into one complex sequence, transformed by
//    Bluestein's algorithm over the radix-2 butterflies of bfgx_fft.hpp (lds_fft_stages, power-of-two size M >= 2k - 1, in
//    LDS), and the four are combined into X[0..n).  F_m = (4 pi / Npix) e^{-i m phi0} X[m mod n] (aliasing of m >= n exact).
//    Synthesis runs the same steps backwards (fold m -> m mod n, combine, two Bluestein transforms, real parts).
//  * Legendre stage, one workgroup per m: every lane owns kRings north/south ring pairs and runs the normalised recurrence
//      lambda_{l+1,m} = c1_{l+1} x lambda_{lm} - c2_{l+1} lambda_{l-1,m}
//    in l, shared by the pair through lambda_lm(-x) = (-1)^{l+m} lambda_lm(x).  lambda_mm ~ sin^m(theta) underflows fp64 long
//    before lambda_lm is O(1) again, so a lane keeps lambda as (value, scale index k): true value = value * 2^(512 k).  The start
//    value is built from an exact power-of-two exponent (binary powering of sin(theta) with frexp), and the recurrence rescales
//    by 2^-512 whenever |value| > 2^256 (checked every kLB steps: the recurrence cannot grow a value by 2^256 within them).
//    While k < 0 the true |lambda| < 2^-200 and it contributes nothing (it is multiplied by 0).
//    Analysis reduces over rings for every l without a cross-lane reduction per l: a lane holds kLB products per ring block in
//    registers and one reduce-scatter of DPP row moves per kLB l (lane j of a 16-lane row ends with the row's sum for l0 + j).
//    Synthesis needs no reduction: each lane sums over l for its own rings.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bfgx_fft.hpp"

namespace bfgx {
namespace sht {

constexpr int kRingThreads = 256;
constexpr int kLegThreads = 256;
constexpr int kRings = 4;                 // ring pairs per lane in the Legendre stage
constexpr int kLB = 16;                   // l per register block (= lanes per DPP row)
constexpr int kSynL = 256;                // l per LDS chunk of the synthesis
constexpr int kMaxNside = 2048;           // ring stage LDS: (M + 2k) complex with M = 2^ceil(log2(2k - 1)) <= 4096 -> 128 KiB
constexpr double kUnseen = -1.6375e30;

// one ring (0-based r = ring number - 1): z = cos(theta), s = sin(theta), first pixel, pixels, half-pixel phase shift, offset of
// the Bluestein kernel of k = nphi / 4 in the B table
struct Ring {
    double z, s;
    int64_t pix0;
    int32_t nphi, shifted;
    int64_t boff;
};

__host__ __device__ inline int pow2_ge(int n) { int m = 1; while (m < n) m <<= 1; return m; }
__host__ __device__ inline int log2_pow2(int m) { int l = 0; while ((1 << l) < m) ++l; return l; }
__host__ __device__ inline int64_t alm_index(int lmax, int l, int m) { return (int64_t)m * (2 * lmax + 1 - m) / 2 + l; }
__device__ inline int brev(int i, int lg) { return lg ? (int)(__brev((unsigned)i) >> (32 - lg)) : 0; }
__device__ inline double2 conj2(double2 a) { return make_double2(a.x, -a.y); }
__device__ inline double2 add2(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ inline double2 sub2(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ inline double2 scl2(double2 a, double s) { return make_double2(a.x * s, a.y * s); }
// e^{i pi a / b} for integers a, b > 0 (the argument reduced exactly first)
__device__ inline double2 expi_pi(int64_t a, int64_t b)
{
    const int64_t r = ((a % (2 * b)) + 2 * b) % (2 * b);
    double sn, cs;
    sincospi((double)r / (double)b, &sn, &cs);
    return make_double2(cs, sn);
}
// healpy.mask_bad: |v - UNSEEN| <= atol + rtol |UNSEEN| (rtol 1e-5, atol 1e-8) counts as 0
__device__ inline double unseen_to_zero(double v) { return fabs(v - kUnseen) <= 1e-8 + 1e-5 * 1.6375e30 ? 0.0 : v; }

// twiddles of size M (the tables of all powers of two are stored back to back: size M starts at M/2 - 1)
__host__ __device__ inline int64_t tw_offset(int M) { return M >= 2 ? M / 2 - 1 : 0; }

// DFT_k of in(j), j < k, by Bluestein: c_j = e^{-i pi j^2 / k}; X_q = c_q conj(FFT_M(conj(FFT_M(a) B))) with a_j = in(j) c_j and
// B = FFT_M(conj chirp, wrapped) / M from the table; out(q, X_q) for q < k.  The whole workgroup calls it; buf = M complex of LDS.
template <class In, class Out>
__device__ void bluestein(In in, Out out, double2 *buf, int k, int M, const double2 *__restrict__ twall, const double2 *__restrict__ B,
                          int tid, int nthr)
{
    const int lg = log2_pow2(M);
    const double2 *tw = twall + tw_offset(M);
    __syncthreads();
    for (int j = tid; j < M; j += nthr) {
        double2 v = make_double2(0.0, 0.0);
        if (j < k) v = cmul(in(j), expi_pi(-(int64_t)j * j, k));
        buf[brev(j, lg)] = v;
    }
    lds_fft_stages(buf, M, 1, tw, tid, nthr);
    for (int i = tid; i < M; i += nthr) {
        const int r = brev(i, lg);
        if (i <= r) {
            const double2 a = cmul(buf[i], B[i]), b = cmul(buf[r], B[r]);
            buf[i] = conj2(b);
            buf[r] = conj2(a);
        }
    }
    lds_fft_stages(buf, M, 1, tw, tid, nthr);
    for (int q = tid; q < k; q += nthr) out(q, cmul(expi_pi(-(int64_t)q * q, k), conj2(buf[q])));
}

// B table: one workgroup per k = 1..kmax: B_k = FFT_M(b) / M, b_j = e^{+i pi j^2 / k} for |j| < k (wrapped mod M)
__global__ void __launch_bounds__(kRingThreads)
sht_bluestein_table_kernel(const double2 *__restrict__ twall, const int64_t *__restrict__ boff, double2 *__restrict__ btab)
{
    extern __shared__ double2 sbuf[];
    const int k = blockIdx.x + 1, M = pow2_ge(2 * k - 1), lg = log2_pow2(M);
    for (int j = threadIdx.x; j < M; j += kRingThreads) {
        const int jj = (j < k) ? j : ((M - j < k) ? M - j : -1);
        sbuf[brev(j, lg)] = (jj >= 0) ? expi_pi((int64_t)jj * jj, k) : make_double2(0.0, 0.0);
    }
    lds_fft_stages(sbuf, M, 1, twall + tw_offset(M), threadIdx.x, kRingThreads);
    double2 *dst = btab + boff[k];
    for (int i = threadIdx.x; i < M; i += kRingThreads) dst[i] = scl2(sbuf[i], 1.0 / M);
}

// analysis ring stage: F[m][ring] = norm e^{-i m phi0} X[m mod n], m <= mmax
__global__ void __launch_bounds__(kRingThreads)
sht_ring_analysis_kernel(const double *__restrict__ map, const Ring *__restrict__ rings, int nrings, int mmax, double norm,
                         const double2 *__restrict__ twall, const double2 *__restrict__ btab, double2 *__restrict__ F)
{
    extern __shared__ double2 sbuf[];
    const Ring R = rings[blockIdx.x];
    const int n = R.nphi, k = n >> 2, M = pow2_ge(2 * k - 1);
    double2 *buf = sbuf, *z01 = sbuf + M, *z23 = z01 + k;
    const double *mp = map + R.pix0;
    const double2 *B = btab + R.boff;
    const int tid = threadIdx.x;
    // sub-sequence t of the ring is x[4j + t]; z01 = x0 + i x1, z23 = x2 + i x3
    bluestein([&](int j) { return make_double2(unseen_to_zero(mp[4 * j]), unseen_to_zero(mp[4 * j + 1])); },
              [&](int q, double2 v) { z01[q] = v; }, buf, k, M, twall, B, tid, kRingThreads);
    bluestein([&](int j) { return make_double2(unseen_to_zero(mp[4 * j + 2]), unseen_to_zero(mp[4 * j + 3])); },
              [&](int q, double2 v) { z23[q] = v; }, buf, k, M, twall, B, tid, kRingThreads);
    __syncthreads();
    for (int m = tid; m <= mmax; m += kRingThreads) {
        const int idx = m % n, q = idx % k, qc = (k - q) % k;
        // Y_{2u}[q] = (Z[q] + conj Z[k-q]) / 2, Y_{2u+1}[q] = (Z[q] - conj Z[k-q]) / (2i) for Z = z01 (u = 0), z23 (u = 1)
        const double2 a = z01[q], ac = conj2(z01[qc]), b = z23[q], bc = conj2(z23[qc]);
        const double2 y0 = scl2(add2(a, ac), 0.5), d1 = sub2(a, ac), y1 = make_double2(0.5 * d1.y, -0.5 * d1.x);
        const double2 y2 = scl2(add2(b, bc), 0.5), d3 = sub2(b, bc), y3 = make_double2(0.5 * d3.y, -0.5 * d3.x);
        // X[idx] = sum_t e^{-2 pi i t idx / n} Y_t[q]
        const double2 w1 = expi_pi(-2 * (int64_t)idx, n), w2 = expi_pi(-4 * (int64_t)idx, n), w3 = expi_pi(-6 * (int64_t)idx, n);
        double2 x = add2(add2(y0, cmul(w1, y1)), add2(cmul(w2, y2), cmul(w3, y3)));
        if (R.shifted) x = cmul(x, expi_pi(-(int64_t)m, n));            // phi0 = pi / n
        F[(int64_t)m * nrings + blockIdx.x] = scl2(x, norm);
    }
}

// synthesis ring stage: map_j = Re sum_{k'} H[k'] e^{2 pi i k' j / n}, H[k'] = sum_{m = k' mod n} w_m G_m e^{i m phi0} (w_0 = 1,
// w_m = 2).  With U_t[q] = e^{2 pi i q t / n} sum_s i^{st} H[q + k s]: map[4p + t] = Re DFT_k(conj U_t)[p] = DFT_k(V_t)[p], V_t the
// Hermitian part of conj U_t, so the pairs V_0 + i V_1, V_2 + i V_3 give the four sub-sequences as real and imaginary parts.
__global__ void __launch_bounds__(kRingThreads)
sht_ring_synthesis_kernel(const double2 *__restrict__ G, const Ring *__restrict__ rings, int nrings, int mmax,
                          const double2 *__restrict__ twall, const double2 *__restrict__ btab, double *__restrict__ map)
{
    extern __shared__ double2 sbuf[];
    const Ring R = rings[blockIdx.x];
    const int n = R.nphi, k = n >> 2, M = pow2_ge(2 * k - 1);
    double2 *buf = sbuf, *z01 = sbuf + M, *z23 = z01 + k;
    const int tid = threadIdx.x;
    auto H = [&](int kk) {
        double2 h = make_double2(0.0, 0.0);
        for (int m = kk; m <= mmax; m += n) {
            double2 g = G[(int64_t)m * nrings + blockIdx.x];
            if (R.shifted) g = cmul(g, expi_pi((int64_t)m, n));
            h = add2(h, scl2(g, m ? 2.0 : 1.0));
        }
        return h;
    };
    auto Ubar = [&](int q, double2 *u) {         // conj U_t[q], t = 0..3
        const double2 h0 = H(q), h1 = H(q + k), h2 = H(q + 2 * k), h3 = H(q + 3 * k);
        // sum_s i^{st} h_s: t = 0: h0 + h1 + h2 + h3; t = 1: h0 + i h1 - h2 - i h3; t = 2: h0 - h1 + h2 - h3; t = 3: h0 - i h1 - h2 + i h3
        const double2 a = add2(h0, h2), b = add2(h1, h3), c = sub2(h0, h2), d = sub2(h1, h3);
        const double2 id = make_double2(-d.y, d.x);
        const double2 s0 = add2(a, b), s1 = add2(c, id), s2 = sub2(a, b), s3 = sub2(c, id);
        u[0] = conj2(s0);
        u[1] = conj2(cmul(expi_pi(2 * (int64_t)q, n), s1));
        u[2] = conj2(cmul(expi_pi(4 * (int64_t)q, n), s2));
        u[3] = conj2(cmul(expi_pi(6 * (int64_t)q, n), s3));
    };
    for (int q = tid; q <= k / 2; q += kRingThreads) {
        const int qc = (k - q) % k;
        double2 u[4], uc[4], v[4], vc[4];
        Ubar(q, u);
        if (qc != q) Ubar(qc, uc);
        else for (int t = 0; t < 4; ++t) uc[t] = u[t];
        for (int t = 0; t < 4; ++t) { v[t] = scl2(add2(u[t], conj2(uc[t])), 0.5); vc[t] = scl2(add2(uc[t], conj2(u[t])), 0.5); }
        z01[q] = make_double2(v[0].x - v[1].y, v[0].y + v[1].x);
        z23[q] = make_double2(v[2].x - v[3].y, v[2].y + v[3].x);
        z01[qc] = make_double2(vc[0].x - vc[1].y, vc[0].y + vc[1].x);
        z23[qc] = make_double2(vc[2].x - vc[3].y, vc[2].y + vc[3].x);
    }
    double *mp = map + R.pix0;
    const double2 *B = btab + R.boff;
    bluestein([&](int j) { return z01[j]; }, [&](int p, double2 v) { mp[4 * p] = v.x; mp[4 * p + 1] = v.y; }, buf, k, M, twall, B, tid, kRingThreads);
    bluestein([&](int j) { return z23[j]; }, [&](int p, double2 v) { mp[4 * p + 2] = v.x; mp[4 * p + 3] = v.y; }, buf, k, M, twall, B, tid, kRingThreads);
}

// c1_l, c2_l of the recurrence producing lambda_lm (l > m; 0 beyond lmax, so that the last block runs on harmlessly)
__device__ inline void rec_coef(int l, int m, int lmax, double &c1, double &c2)
{
    if (l > lmax || l <= m) { c1 = 0.0; c2 = 0.0; return; }
    const double dl = l, dm = m;
    c1 = sqrt((4.0 * dl * dl - 1.0) / ((dl - dm) * (dl + dm)));
    const double lp = dl - 1.0;
    c2 = (l == m + 1) ? 0.0 : c1 * sqrt(((lp - dm) * (lp + dm)) / (4.0 * lp * lp - 1.0));
}

// scaled start value: lambda_mm = pref[m] s^m as (value, scale index), true = value * 2^(512 k), |value| in [2^-256, 2^256)
__device__ inline void lambda_mm(double pref, double s, int m, double &v, int &k)
{
    int e = 0, t;
    double mant = frexp(pref, &t);
    e += t;
    int be;
    double b = frexp(s, &be);
    for (int mm = m; mm; mm >>= 1) {
        if (mm & 1) { mant = frexp(mant * b, &t); e += t + be; }
        b = frexp(b * b, &t);
        be = 2 * be + t;
    }
    k = (e + 256) >= 0 ? (e + 256) / 512 : -((-(e + 256) + 511) / 512);
    v = ldexp(mant, e - 512 * k);
}

__device__ inline void rescale(double &v0, double &v1, int &k)
{
    if (fabs(v1) > 0x1p+256 || fabs(v0) > 0x1p+256) { v0 *= 0x1p-512; v1 *= 0x1p-512; ++k; }
}

template <int CTRL>
__device__ inline double dpp_d(double v)
{
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

// one reduce-scatter level over a 16-lane row: partner = lane ^ (2 H - 1) (DPP CTRL); lanes with bit H of their row position keep the
// upper half of a[0 .. 2H) and receive the partner's copy of it
template <int H, int CTRL>
__device__ inline void rs_level(double2 *a, bool up)
{
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const double2 keep = up ? a[i + H] : a[i], send = up ? a[i] : a[i + H];
        a[i] = make_double2(keep.x + dpp_d<CTRL>(send.x), keep.y + dpp_d<CTRL>(send.y));
    }
}

// analysis Legendre stage: alm[l, m] (+)= sum_pairs lambda_lm(x) (l + m even ? F_n + F_s : F_n - F_s), one workgroup per m
__global__ void __launch_bounds__(kLegThreads)
sht_legendre_analysis_kernel(const double2 *__restrict__ F, const Ring *__restrict__ rings, int nside, int lmax,
                             const double *__restrict__ pref, int accumulate, double2 *__restrict__ alm)
{
    __shared__ double2 coef[2][kLB];                               // (c1, c2) of l0 + 1 + j
    __shared__ double2 red[2][kLegThreads / kLB][kLB];             // per-row partial sums
    const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int nrings = 4 * nside - 1, npairs = 2 * nside;
    const int64_t a0 = alm_index(lmax, 0, m);
    const double pm = pref[m];
    const int nchunks = (npairs + kLegThreads * kRings - 1) / (kLegThreads * kRings);
    int cb = 0;
    for (int ch = 0; ch < nchunks; ++ch) {
        double x[kRings], v0[kRings], v1[kRings];
        int ks[kRings];
        double2 E[kRings], O[kRings];
#pragma unroll
        for (int r = 0; r < kRings; ++r) {
            const int p = (ch * kRings + r) * kLegThreads + tid;
            double s = 1.0;
            x[r] = 0.0;
            E[r] = O[r] = make_double2(0.0, 0.0);
            if (p < npairs) {
                const Ring R = rings[p];
                const int rs = nrings - 1 - p;
                x[r] = R.z; s = R.s;
                const double2 fn = F[(int64_t)m * nrings + p];
                const double2 fs = (rs != p) ? F[(int64_t)m * nrings + rs] : make_double2(0.0, 0.0);
                E[r] = add2(fn, fs); O[r] = sub2(fn, fs);
            }
            lambda_mm(pm, s, m, v1[r], ks[r]);
            v0[r] = 0.0;
        }
        for (int l0 = m; l0 <= lmax; l0 += kLB) {
            if (tid < kLB) { double c1, c2; rec_coef(l0 + 1 + tid, m, lmax, c1, c2); coef[cb][tid] = make_double2(c1, c2); }
            __syncthreads();
            double2 acc[kLB];
#pragma unroll
            for (int j = 0; j < kLB; ++j) acc[j] = make_double2(0.0, 0.0);
            const bool odd0 = (l0 + m) & 1;
#pragma unroll
            for (int r = 0; r < kRings; ++r) {
                const double on = ks[r] == 0 ? 1.0 : 0.0;
                const double2 P0 = scl2(odd0 ? O[r] : E[r], on), P1 = scl2(odd0 ? E[r] : O[r], on);
                double a = v0[r], b = v1[r];
                const double xr = x[r];
#pragma unroll
                for (int j = 0; j < kLB; ++j) {
                    const double2 P = (j & 1) ? P1 : P0;
                    acc[j].x = fma(b, P.x, acc[j].x);
                    acc[j].y = fma(b, P.y, acc[j].y);
                    const double2 c = coef[cb][j];
                    const double nb = fma(c.x * xr, b, -c.y * a);
                    a = b; b = nb;
                }
                v0[r] = a; v1[r] = b;
                rescale(v0[r], v1[r], ks[r]);
            }
            // reduce-scatter over each 16-lane row: lane position j ends with the row's sum for l0 + j
            rs_level<8, 0x140>(acc, lane & 8);                     // row_mirror: lane ^ 15
            rs_level<4, 0x141>(acc, lane & 4);                     // row_half_mirror: lane ^ 7
            rs_level<2, 0x1B>(acc, lane & 2);                      // quad_perm [3,2,1,0]: lane ^ 3
            rs_level<1, 0xB1>(acc, lane & 1);                      // quad_perm [1,0,3,2]: lane ^ 1
            red[cb][tid >> 4][tid & 15] = acc[0];
            __syncthreads();
            if (tid < 2 * kLB) {
                const int j = tid >> 1, c = tid & 1;
                double sum = 0.0;
                for (int w = 0; w < kLegThreads / kLB; ++w) sum += c ? red[cb][w][j].y : red[cb][w][j].x;
                const int l = l0 + j;
                if (l <= lmax) {
                    double *dst = reinterpret_cast<double *>(alm + a0 + l) + c;
                    *dst = (ch == 0 && !accumulate) ? sum : *dst + sum;
                }
            }
            cb ^= 1;
        }
    }
}

// synthesis Legendre stage: G[m][ring] = sum_l a_lm lambda_lm(+-x) (Im a_l0 ignored), one workgroup per m, no reduction
__global__ void __launch_bounds__(kLegThreads)
sht_legendre_synthesis_kernel(const double2 *__restrict__ alm, const Ring *__restrict__ rings, int nside, int lmax,
                              const double *__restrict__ pref, double2 *__restrict__ G)
{
    __shared__ double2 sa[kSynL], sc[kSynL];                       // a_lm and (c1, c2) of l0 + 1 + j
    const int m = blockIdx.x, tid = threadIdx.x;
    const int nrings = 4 * nside - 1, npairs = 2 * nside;
    const int64_t a0 = alm_index(lmax, 0, m);
    const double pm = pref[m];
    const int nchunks = (npairs + kLegThreads * kRings - 1) / (kLegThreads * kRings);
    for (int ch = 0; ch < nchunks; ++ch) {
        double x[kRings], v0[kRings], v1[kRings];
        int ks[kRings];
        double2 ge[kRings], go[kRings];
#pragma unroll
        for (int r = 0; r < kRings; ++r) {
            const int p = (ch * kRings + r) * kLegThreads + tid;
            double s = 1.0;
            x[r] = 0.0;
            if (p < npairs) { x[r] = rings[p].z; s = rings[p].s; }
            lambda_mm(pm, s, m, v1[r], ks[r]);
            v0[r] = 0.0;
            ge[r] = go[r] = make_double2(0.0, 0.0);
        }
        for (int L0 = m; L0 <= lmax; L0 += kSynL) {
            __syncthreads();
            for (int j = tid; j < kSynL; j += kLegThreads) {
                const int l = L0 + j;
                double2 a = make_double2(0.0, 0.0);
                if (l <= lmax) { a = alm[a0 + l]; if (m == 0) a.y = 0.0; }
                double c1, c2;
                rec_coef(l + 1, m, lmax, c1, c2);
                sa[j] = a; sc[j] = make_double2(c1, c2);
            }
            __syncthreads();
            const int nb = min(kSynL, lmax - L0 + 1);
            for (int j0 = 0; j0 < nb; j0 += kLB) {
                const bool odd0 = (L0 + j0 + m) & 1;
#pragma unroll
                for (int r = 0; r < kRings; ++r) {
                    const double on = ks[r] == 0 ? 1.0 : 0.0;
                    double a = v0[r], b = v1[r];
                    const double xr = x[r];
                    double2 e = make_double2(0.0, 0.0), o = make_double2(0.0, 0.0);
#pragma unroll
                    for (int j = 0; j < kLB; ++j) {
                        const double2 al = sa[j0 + j];       // (zero beyond lmax)
                        if (j & 1) { o.x = fma(b, al.x, o.x); o.y = fma(b, al.y, o.y); }
                        else { e.x = fma(b, al.x, e.x); e.y = fma(b, al.y, e.y); }
                        const double2 c = sc[j0 + j];
                        const double nbv = fma(c.x * xr, b, -c.y * a);
                        a = b; b = nbv;
                    }
                    v0[r] = a; v1[r] = b;
                    if (odd0) { double2 t = e; e = o; o = t; }
                    ge[r].x = fma(on, e.x, ge[r].x); ge[r].y = fma(on, e.y, ge[r].y);
                    go[r].x = fma(on, o.x, go[r].x); go[r].y = fma(on, o.y, go[r].y);
                    rescale(v0[r], v1[r], ks[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kRings; ++r) {
            const int p = (ch * kRings + r) * kLegThreads + tid;
            if (p < npairs) {
                const int rs = nrings - 1 - p;
                G[(int64_t)m * nrings + p] = add2(ge[r], go[r]);
                if (rs != p) G[(int64_t)m * nrings + rs] = sub2(ge[r], go[r]);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- spin-weighted Legendre stage
// Spin-s transforms (healpy map2alm_spin / alm2map_spin, HEALPix/libsharp convention) of a pair of real maps:
//   map0 + i map1 = -sum_{l >= s} sum_{m = -l..l} (G_lm + i C_lm) sY_lm,   sY_lm(theta, phi) = slambda_lm(theta) e^{i m phi},
// G and C the coefficients of real fields (only m >= 0 stored).  Per m >= 0 a lane runs two columns in l:
//   lam+ = slambda_lm,  lam- = (-1)^m slambda_{l,-m},
// both by the normalised Wigner-d recurrence lam_L = a_L (x +- b_L) lam_{L-1} - c_L lam_{L-2} (b_L = m s / (L (L - 1)); + for lam+,
// - for lam-), from l0 = max(m, s) with
//   lam+_{l0} = (-1)^m P cos^|m-s|(theta/2) sin^(m+s)(theta/2),  lam-_{l0} = (m >= s ? (-1)^(m+s) : 1) P cos^(m+s)(theta/2) sin^|m-s|(theta/2),
//   P = sqrt((2 l0 + 1) / (4 pi) binom(2 l0, m + s)).
// The south ring of a pair follows from lam+(pi - theta) = (-1)^(l+m+s) lam-(theta) and lam-(pi - theta) = (-1)^(l+m+s) lam+(theta).
// With P = F0 + i F1 and M = F0 - i F1 (F0, F1: ring stage of map0, map1) the analysis is G + i C = -sum lam+ P, G - i C = -sum lam- M;
// the synthesis is F0 + i F1 = -sum_l (G + i C) lam+, F0 - i F1 = -sum_l (G - i C) lam-.  Both columns keep their own
// (value, scale index) as lambda_mm does: P and the powers of cos and sin(theta/2) are built with exact exponents.
constexpr int kSpinRings = 2;             // ring pairs per lane (two columns, four inputs or outputs per ring)

// mant 2^e *= x^n for x > 0, the exponent kept exactly (binary powering with frexp)
__device__ inline void mul_pow(double &mant, int &e, double x, int n)
{
    int be, t;
    double b = frexp(x, &be);
    for (int nn = n; nn; nn >>= 1) {
        if (nn & 1) { mant = frexp(mant * b, &t); e += t + be; }
        b = frexp(b * b, &t);
        be = 2 * be + t;
    }
}

// mant 2^e as (value, scale index): true = value 2^(512 k), |value| in [2^-256, 2^256)
__device__ inline void to_scaled(double mant, int e, double &v, int &k)
{
    k = (e + 256) >= 0 ? (e + 256) / 512 : -((-(e + 256) + 511) / 512);
    v = ldexp(mant, e - 512 * k);
}

// P = sqrt((2 l0 + 1) / (4 pi) binom(2 l0, l0 + t)), l0 = max(m, s), t = min(m, s), as mant 2^e.  binom(2 l0, l0 + t) =
// 4^l0 prod_{k <= l0} (2k - 1) / (2k) prod_{i <= t} (l0 - t + i) / (l0 + i); for m >= s the first two factors are the spin-0
// prefactor pref[m]^2 (4 pi / (2m + 1)) of the plan
__device__ inline void spin_pref(const double *__restrict__ pref, int m, int s, double &mant, int &e)
{
    const int l0 = max(m, s), t = min(m, s);
    int tt;
    mant = 1.0; e = 0;
    for (int i = 1; i <= t; ++i) { mant = frexp(mant * ((double)(l0 - t + i) / (double)(l0 + i)), &tt); e += tt; }
    double base;
    if (m >= s) base = fabs(pref[m]);
    else {
        double q = (2.0 * s + 1.0) / (4.0 * M_PI);
        for (int k = 1; k <= s; ++k) q *= (2.0 * k - 1.0) / (2.0 * k);
        base = sqrt(q);
    }
    if (e & 1) { mant *= 2.0; --e; }
    mant = frexp(base * sqrt(mant), &tt);
    e = e / 2 + l0 + tt;
}

// start values of both columns at l0 on a north ring (z >= 0): cos(theta/2) from z, sin(theta/2) = sin(theta) / (2 cos(theta/2))
__device__ inline void spin_start(double pmant, int pe, int m, int s, double z, double sn, double &vp, int &kp, double &vm, int &km)
{
    const double c = sqrt(0.5 * (1.0 + z)), h = sn / (2.0 * c);
    const int d = abs(m - s);
    double mp = pmant, mm = pmant;
    int ep = pe, em = pe;
    mul_pow(mp, ep, c, d);
    mul_pow(mp, ep, h, m + s);
    mul_pow(mm, em, c, m + s);
    mul_pow(mm, em, h, d);
    to_scaled((m & 1) ? -mp : mp, ep, vp, kp);
    to_scaled((m >= s && ((m + s) & 1)) ? -mm : mm, em, vm, km);
}

// a_L, a_L b_L and c_L of the spin recurrence (0 beyond lmax and for L <= l0, so that a last block runs on harmlessly)
__device__ inline void spin_rec_coef(int L, int m, int s, int lmax, double &a, double &ab, double &c)
{
    if (L > lmax || L <= max(m, s)) { a = 0.0; ab = 0.0; c = 0.0; return; }
    const double dl = L, dm = m, ds = s, d1 = dl - 1.0;
    const double den = (dl * dl - dm * dm) * (dl * dl - ds * ds);
    a = dl * sqrt((2.0 * dl + 1.0) * (2.0 * dl - 1.0) / den);
    ab = a * (dm * ds) / (dl * d1);
    c = (dl / d1) * sqrt((2.0 * dl + 1.0) / (2.0 * dl - 3.0) * ((d1 * d1 - dm * dm) * (d1 * d1 - ds * ds)) / den);
}

__device__ inline double2 neg2(double2 a) { return make_double2(-a.x, -a.y); }

// spin analysis Legendre stage: G, C [l, m] for l = max(m, s) .. lmax (0 for m <= l < s), one workgroup per m.  A lane accumulates
// Ap = sum lam+ P and Am = sum lam- M for 16 l in registers; the reduce-scatter and the fixed-order row sum are those of
// sht_legendre_analysis_kernel, once for Ap and once for Am; then G = -(Ap + Am) / 2, C = i (Ap - Am) / 2.
__global__ void __launch_bounds__(kLegThreads)
sht_spin_legendre_analysis_kernel(const double2 *__restrict__ F0, const double2 *__restrict__ F1, const Ring *__restrict__ rings, int nside,
                                  int lmax, int spin, const double *__restrict__ pref, double2 *__restrict__ almG, double2 *__restrict__ almC)
{
    __shared__ double cA[2][kLB], cAB[2][kLB], cC[2][kLB];        // a, a b, c of l0 + 1 + j
    __shared__ double2 red[2][2][kLegThreads / kLB][kLB];          // per-row partial sums of Ap, Am
    const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int nrings = 4 * nside - 1, npairs = 2 * nside, ls = max(m, spin);
    const int64_t a0 = alm_index(lmax, 0, m);
    for (int l = m + tid; l < ls; l += kLegThreads) { almG[a0 + l] = make_double2(0.0, 0.0); almC[a0 + l] = make_double2(0.0, 0.0); }
    double pmant;
    int pe;
    spin_pref(pref, m, spin, pmant, pe);
    const int nchunks = (npairs + kLegThreads * kSpinRings - 1) / (kLegThreads * kSpinRings);
    int cb = 0;
    for (int ch = 0; ch < nchunks; ++ch) {
        double x[kSpinRings], p0[kSpinRings], p1[kSpinRings], q0[kSpinRings], q1[kSpinRings];
        int kp[kSpinRings], km[kSpinRings];
        double2 PN[kSpinRings], MN[kSpinRings], PS[kSpinRings], MS[kSpinRings];
#pragma unroll
        for (int r = 0; r < kSpinRings; ++r) {
            const int p = (ch * kSpinRings + r) * kLegThreads + tid;
            double sn = 1.0;
            x[r] = 0.0;
            PN[r] = MN[r] = PS[r] = MS[r] = make_double2(0.0, 0.0);
            if (p < npairs) {
                const Ring R = rings[p];
                const int rs = nrings - 1 - p;
                x[r] = R.z; sn = R.s;
                const double2 a = F0[(int64_t)m * nrings + p], b = F1[(int64_t)m * nrings + p];
                PN[r] = make_double2(a.x - b.y, a.y + b.x); MN[r] = make_double2(a.x + b.y, a.y - b.x);
                if (rs != p) {
                    const double2 c = F0[(int64_t)m * nrings + rs], d = F1[(int64_t)m * nrings + rs];
                    PS[r] = make_double2(c.x - d.y, c.y + d.x); MS[r] = make_double2(c.x + d.y, c.y - d.x);
                }
            }
            spin_start(pmant, pe, m, spin, x[r], sn, p1[r], kp[r], q1[r], km[r]);
            p0[r] = q0[r] = 0.0;
        }
        for (int l0 = ls; l0 <= lmax; l0 += kLB) {
            if (tid < kLB) spin_rec_coef(l0 + 1 + tid, m, spin, lmax, cA[cb][tid], cAB[cb][tid], cC[cb][tid]);
            __syncthreads();
            double2 ap[kLB], am[kLB];
#pragma unroll
            for (int j = 0; j < kLB; ++j) ap[j] = am[j] = make_double2(0.0, 0.0);
            const double sg0 = ((l0 + m + spin) & 1) ? -1.0 : 1.0;      // (-1)^(l+m+s) at l = l0
#pragma unroll
            for (int r = 0; r < kSpinRings; ++r) {
                const double onp = kp[r] == 0 ? 1.0 : 0.0, onm = km[r] == 0 ? 1.0 : 0.0;
                const double2 pn = scl2(PN[r], onp), ms = scl2(MS[r], onp * sg0), mn = scl2(MN[r], onm), ps = scl2(PS[r], onm * sg0);
                double a = p0[r], b = p1[r], c = q0[r], d = q1[r];
                const double xr = x[r];
#pragma unroll
                for (int j = 0; j < kLB; ++j) {
                    const double2 psj = (j & 1) ? neg2(ps) : ps, msj = (j & 1) ? neg2(ms) : ms;
                    ap[j].x = fma(b, pn.x, ap[j].x); ap[j].y = fma(b, pn.y, ap[j].y);
                    ap[j].x = fma(d, psj.x, ap[j].x); ap[j].y = fma(d, psj.y, ap[j].y);
                    am[j].x = fma(d, mn.x, am[j].x); am[j].y = fma(d, mn.y, am[j].y);
                    am[j].x = fma(b, msj.x, am[j].x); am[j].y = fma(b, msj.y, am[j].y);
                    const double A = cA[cb][j], AB = cAB[cb][j], C = cC[cb][j];
                    const double nb = fma(fma(A, xr, AB), b, -C * a), nd = fma(fma(A, xr, -AB), d, -C * c);
                    a = b; b = nb; c = d; d = nd;
                }
                p0[r] = a; p1[r] = b; q0[r] = c; q1[r] = d;
                rescale(p0[r], p1[r], kp[r]);
                rescale(q0[r], q1[r], km[r]);
            }
            rs_level<8, 0x140>(ap, lane & 8); rs_level<8, 0x140>(am, lane & 8);
            rs_level<4, 0x141>(ap, lane & 4); rs_level<4, 0x141>(am, lane & 4);
            rs_level<2, 0x1B>(ap, lane & 2);  rs_level<2, 0x1B>(am, lane & 2);
            rs_level<1, 0xB1>(ap, lane & 1);  rs_level<1, 0xB1>(am, lane & 1);
            red[cb][0][tid >> 4][tid & 15] = ap[0];
            red[cb][1][tid >> 4][tid & 15] = am[0];
            __syncthreads();
            if (tid < 4 * kLB) {
                // c = 0: Re G = -(Ap + Am).x / 2, 1: Im G = -(Ap + Am).y / 2, 2: Re C = -(Ap - Am).y / 2, 3: Im C = (Ap - Am).x / 2
                const int j = tid >> 2, c = tid & 3;
                const bool useY = c == 1 || c == 2;
                double sp = 0.0, sm = 0.0;
                for (int w = 0; w < kLegThreads / kLB; ++w) {
                    sp += useY ? red[cb][0][w][j].y : red[cb][0][w][j].x;
                    sm += useY ? red[cb][1][w][j].y : red[cb][1][w][j].x;
                }
                const double v = (c < 2) ? -0.5 * (sp + sm) : (c == 2 ? -0.5 * (sp - sm) : 0.5 * (sp - sm));
                const int l = l0 + j;
                if (l <= lmax) {
                    double *dst = reinterpret_cast<double *>((c < 2 ? almG : almC) + a0 + l) + (c & 1);
                    *dst = ch == 0 ? v : *dst + v;
                }
            }
            cb ^= 1;
        }
    }
}

// spin synthesis Legendre stage: F0, F1 [m][ring] from G, C (l >= max(m, s); Im G_l0, Im C_l0 drop out in the ring stage), one
// workgroup per m, no reduction
__global__ void __launch_bounds__(kLegThreads)
sht_spin_legendre_synthesis_kernel(const double2 *__restrict__ almG, const double2 *__restrict__ almC, const Ring *__restrict__ rings,
                                   int nside, int lmax, int spin, const double *__restrict__ pref, double2 *__restrict__ F0,
                                   double2 *__restrict__ F1)
{
    __shared__ double2 sP[kSynL], sM[kSynL];                       // G + i C and G - i C of l = L0 + j
    __shared__ double sA[kSynL], sAB[kSynL], sC[kSynL];            // a, a b, c of L0 + 1 + j
    const int m = blockIdx.x, tid = threadIdx.x;
    const int nrings = 4 * nside - 1, npairs = 2 * nside, ls = max(m, spin);
    const int64_t a0 = alm_index(lmax, 0, m);
    double pmant;
    int pe;
    spin_pref(pref, m, spin, pmant, pe);
    const int nchunks = (npairs + kLegThreads * kSpinRings - 1) / (kLegThreads * kSpinRings);
    for (int ch = 0; ch < nchunks; ++ch) {
        double x[kSpinRings], p0[kSpinRings], p1[kSpinRings], q0[kSpinRings], q1[kSpinRings];
        int kp[kSpinRings], km[kSpinRings];
        double2 QPN[kSpinRings], QMN[kSpinRings], QPS[kSpinRings], QMS[kSpinRings];
#pragma unroll
        for (int r = 0; r < kSpinRings; ++r) {
            const int p = (ch * kSpinRings + r) * kLegThreads + tid;
            double sn = 1.0;
            x[r] = 0.0;
            if (p < npairs) { x[r] = rings[p].z; sn = rings[p].s; }
            spin_start(pmant, pe, m, spin, x[r], sn, p1[r], kp[r], q1[r], km[r]);
            p0[r] = q0[r] = 0.0;
            QPN[r] = QMN[r] = QPS[r] = QMS[r] = make_double2(0.0, 0.0);
        }
        for (int L0 = ls; L0 <= lmax; L0 += kSynL) {
            __syncthreads();
            for (int j = tid; j < kSynL; j += kLegThreads) {
                const int l = L0 + j;
                double2 g = make_double2(0.0, 0.0), c = g;
                if (l <= lmax) { g = almG[a0 + l]; c = almC[a0 + l]; }
                sP[j] = make_double2(g.x - c.y, g.y + c.x);
                sM[j] = make_double2(g.x + c.y, g.y - c.x);
                spin_rec_coef(l + 1, m, spin, lmax, sA[j], sAB[j], sC[j]);
            }
            __syncthreads();
            const int nb = min(kSynL, lmax - L0 + 1);
            for (int j0 = 0; j0 < nb; j0 += kLB) {
                const double sg0 = ((L0 + j0 + m + spin) & 1) ? -1.0 : 1.0;
#pragma unroll
                for (int r = 0; r < kSpinRings; ++r) {
                    const double onp = kp[r] == 0 ? 1.0 : 0.0, onm = km[r] == 0 ? 1.0 : 0.0;
                    double a = p0[r], b = p1[r], c = q0[r], d = q1[r];
                    const double xr = x[r];
                    double2 pn = make_double2(0.0, 0.0), mn = pn, ps = pn, ms = pn;
#pragma unroll
                    for (int j = 0; j < kLB; ++j) {
                        const double2 P = sP[j0 + j], M = sM[j0 + j];     // (zero beyond lmax)
                        const double2 Pj = (j & 1) ? neg2(P) : P, Mj = (j & 1) ? neg2(M) : M;
                        pn.x = fma(b, P.x, pn.x); pn.y = fma(b, P.y, pn.y);
                        mn.x = fma(d, M.x, mn.x); mn.y = fma(d, M.y, mn.y);
                        ps.x = fma(d, Pj.x, ps.x); ps.y = fma(d, Pj.y, ps.y);
                        ms.x = fma(b, Mj.x, ms.x); ms.y = fma(b, Mj.y, ms.y);
                        const double A = sA[j0 + j], AB = sAB[j0 + j], C = sC[j0 + j];
                        const double nbv = fma(fma(A, xr, AB), b, -C * a), ndv = fma(fma(A, xr, -AB), d, -C * c);
                        a = b; b = nbv; c = d; d = ndv;
                    }
                    p0[r] = a; p1[r] = b; q0[r] = c; q1[r] = d;
                    const double fps = onm * sg0, fms = onp * sg0;
                    QPN[r].x = fma(onp, pn.x, QPN[r].x); QPN[r].y = fma(onp, pn.y, QPN[r].y);
                    QMN[r].x = fma(onm, mn.x, QMN[r].x); QMN[r].y = fma(onm, mn.y, QMN[r].y);
                    QPS[r].x = fma(fps, ps.x, QPS[r].x); QPS[r].y = fma(fps, ps.y, QPS[r].y);
                    QMS[r].x = fma(fms, ms.x, QMS[r].x); QMS[r].y = fma(fms, ms.y, QMS[r].y);
                    rescale(p0[r], p1[r], kp[r]);
                    rescale(q0[r], q1[r], km[r]);
                }
            }
        }
        // F0 = -(Qp + Qm) / 2, F1 = i (Qp - Qm) / 2
#pragma unroll
        for (int r = 0; r < kSpinRings; ++r) {
            const int p = (ch * kSpinRings + r) * kLegThreads + tid;
            if (p < npairs) {
                const int rs = nrings - 1 - p;
                const int64_t on = (int64_t)m * nrings + p, os = (int64_t)m * nrings + rs;
                F0[on] = scl2(add2(QPN[r], QMN[r]), -0.5);
                F1[on] = make_double2(-0.5 * (QPN[r].y - QMN[r].y), 0.5 * (QPN[r].x - QMN[r].x));
                if (rs != p) {
                    F0[os] = scl2(add2(QPS[r], QMS[r]), -0.5);
                    F1[os] = make_double2(-0.5 * (QPS[r].y - QMS[r].y), 0.5 * (QPS[r].x - QMS[r].x));
                }
            }
        }
    }
}

// residual of an iteration: out = clean(map) - out
__global__ void __launch_bounds__(256)
sht_residual_kernel(const double *__restrict__ map, double *__restrict__ out, int64_t npix)
{
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) out[i] = unseen_to_zero(map[i]) - out[i];
}

// cl[l] = (Re a_l0 conj b_l0 + 2 sum_{m=1}^{min(l, mmax)} Re a_lm conj b_lm) / (2l + 1) for l <= min(lmax, lmax_out), 0 beyond
__global__ void __launch_bounds__(256)
sht_alm2cl_kernel(const double2 *__restrict__ a, const double2 *__restrict__ b, int lmax, int mmax, int lmax_out, double *__restrict__ cl)
{
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l > lmax_out) return;
    if (l > lmax) { cl[l] = 0.0; return; }
    const double2 a0 = a[l], b0 = b[l];
    double s = 0.0;
    for (int m = 1; m <= min(l, mmax); ++m) {
        const int64_t i = alm_index(lmax, l, m);
        const double2 x = a[i], y = b[i];
        s += x.x * y.x + x.y * y.y;
    }
    cl[l] = (a0.x * b0.x + a0.y * b0.y + 2.0 * s) / (2.0 * l + 1.0);
}

// healpy.almxfl: out_lm = in_lm * fl[l] (fl[l] = 0 for l >= nfl); column m = blockIdx.y, one lane per l.  in == out is allowed (each
// lane reads and writes its own coefficient only)
__global__ void __launch_bounds__(256)
sht_almxfl_kernel(const double2 *in, double2 *out, int lmax, int nfl, const double *__restrict__ fl)
{
    const int m = blockIdx.y, l = blockIdx.x * 256 + threadIdx.x;
    if (l < m || l > lmax) return;
    const int64_t i = alm_index(lmax, l, m);
    const double f = l < nfl ? fl[l] : 0.0;
    const double2 a = in[i];
    out[i] = make_double2(a.x * f, a.y * f);
}

}  // namespace sht
}  // namespace bfgx
