// bfgx_sht.hpp -- scalar (spin-0) spherical-harmonic transforms of RING-ordered HEALPix maps in fp64 (healpy.map2alm /
// alm2map / alm2cl / anafast, the last step of reference notebooks 04, 05 and 09) for gfx950.
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

}  // namespace sht
}  // namespace bfgx
