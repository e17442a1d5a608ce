// bfgx_pcl.hpp -- mode-coupling matrices of a mask (pseudo-C_l), fp64, gfx950.  C ABI: bfgx_pcl_api.inc; contract: include/bfgx.h.
//
// With j = l'' from |l - l'| to l + l', L = l + l' + j, and W_j = 0 beyond lw, the kernel computes the symmetric sums
//   kind 0:  X   = sum (2j+1) W_j (l l' j; 0 0 0)^2
//   kind 1:  X   = sum (2j+1) W_j (l l' j; 0 0 0) (l l' j; 2 -2 0)
//   kind 2:  X+- = sum (2j+1) W_j (l l' j; 2 -2 0)^2 over even / odd L
// for l >= l' and writes M[l, l'] = (2l'+1) / (4 pi) X and M[l', l] = (2l+1) / (4 pi) X.  The entry zeroes the matrices first and the
// kernel visits the band |l - l'| <= lw alone (and l, l' >= 2 for kinds 1 and 2): everything else stays exactly 0.
//
// One workgroup holds one l' and W in LDS; each wave takes 64 consecutive l at a time.  For l >= l' the trip counts depend on l' alone
// (kinds 1, 2: 2 l' + 1 values of j; kind 0: every second j up to min(l + l', lw)), so a wave runs uniform loops and reads W at
// consecutive addresses.  Every entry is computed by one lane in a fixed order: no atomics, the same bits on every run.
//
// (0 0 0)^2 at even L is w(j) = g(J - l) g(J - l') g(J - j) / ((L + 1) g(J)), J = L / 2, g(n) = (2n)! / n!^2, so with a = J - l, b = J - l',
// c = J - j:   w(j + 2) / w(j) = (2a+1)(2b+1)(J+1) c / ((2c-1)(2J+3)(a+1)(b+1)),
// started at j = l - l' from w = u(l - l') u(l') / ((2l + 1) u(l)), u(n) = g(n) / 4^n = prod_{k <= n} (2k - 1) / (2k) (central()): no factorial
// is ever formed.  The signed symbol is (-1)^J sqrt(w).
//
// f(j) = (l l' j; 2 -2 0) obeys, with a(j) = sqrt((j^2 - (l - l')^2) ((l + l' + 1)^2 - j^2)),
//   a(j + 1) f(j + 1) = 4 (2j + 1) f(j) - a(j) f(j - 1)        (Schulten & Gordon 1975, the recursion in the j whose m is 0)
// and a vanishes at both ends of the range, which starts the recursion from f = 1 there.  It runs upwards over j = l - l' .. l and
// downwards over j = l + l' .. l + 1 (each towards the classical middle, the stable direction); the two pieces are matched at j = l, l + 1
// by least squares, normalised by sum (2j+1) f^2 = 1, and signed by f(l + l') ~ (-1)^(l - l').
#pragma once
namespace pcl {

constexpr int kWave = 64;
constexpr int kMaxWaves = 16;                  // waves of a workgroup: one copy of W in LDS serves up to 1024 values of l
constexpr int kMaxLmax = 8191;
constexpr int kMaxLw = 16383;                  // W_0 .. W_16383 = 128 KiB of LDS
constexpr int kUSmall = 48;                    // u(n) below this comes from a table in LDS, above it from the series

inline int w_entries(int lmax, int lw) { return std::min(lw, 2 * lmax) + 1; }            // j <= l + l' <= 2 lmax
inline size_t lds_bytes(int lmax, int lw) { return sizeof(double) * (size_t)(kUSmall + w_entries(lmax, lw)); }
inline int block_waves(int lmax, int lw) { return std::min(std::min(lw, lmax) / kWave + 1, kMaxWaves); }

// u(n) = Gamma(n + 1/2) / (sqrt(pi) Gamma(n + 1)); for n >= kUSmall its asymptotic series in 1 / n (the first omitted term is below 1e-19)
__device__ __forceinline__ double central(int n, const double *usmall)
{
    if (n < kUSmall) return usmall[n];
    const double x = 1.0 / (double)n;
    double s = 59697183.0 / 274877906944.0;
    s = fma(s, x, -28717403.0 / 17179869184.0);
    s = fma(s, x, -334477.0 / 2147483648.0);
    s = fma(s, x, 39325.0 / 33554432.0);
    s = fma(s, x, 869.0 / 4194304.0);
    s = fma(s, x, -399.0 / 262144.0);
    s = fma(s, x, -21.0 / 32768.0);
    s = fma(s, x, 5.0 / 1024.0);
    s = fma(s, x, 1.0 / 128.0);
    s = fma(s, x, -1.0 / 8.0);
    s = fma(s, x, 1.0);
    return s / sqrt(M_PI * (double)n);
}

// w(j + 2) / w(j) of the (0 0 0)^2 symbols as numerator and denominator; J = (l + l' + j) / 2, a = J - l, b = J - l', c = J - j
__device__ __forceinline__ void w_ratio(double J, double a, double b, double c, double &num, double &den)
{
    num = ((2.0 * a + 1.0) * (2.0 * b + 1.0) * (J + 1.0) * c);
    den = ((2.0 * c - 1.0) * (2.0 * J + 3.0) * (a + 1.0) * (b + 1.0));
}

// kind 0 of one (l1 >= l2) pair
__device__ __forceinline__ double x00(int l1, int l2, int lw, const double *W, const double *usmall)
{
    const int d = l1 - l2, jhi = min(l1 + l2, lw);
    double w = central(d, usmall) * central(l2, usmall) / ((2.0 * l1 + 1.0) * central(l1, usmall));
    double J = l1, a = 0.0, b = d, c = l2, acc = 0.0;
    for (int j = d;;) {
        acc += (2.0 * j + 1.0) * W[j] * w;
        j += 2;
        if (j > jhi) break;
        double num, den;
        w_ratio(J, a, b, c, num, den);
        w *= num / den;
        J += 1.0; a += 1.0; b += 1.0; c -= 1.0;
    }
    return acc;
}

// kinds 1 and 2 of one (l1 >= l2 >= 2) pair: KIND 1 returns the sum in x0, KIND 2 the even-L sum in x0 and the odd-L sum in x1
template <int KIND>
__device__ __forceinline__ void x22(int l1, int l2, int lw, const double *W, const double *usmall, double &x0, double &x1)
{
    const int d = l1 - l2, top = l1 + l2, s = top + 1;
    auto a_of = [&](int j) { return sqrt((double)(j - d) * (double)(j + d) * (double)(s - j) * (double)(s + j)); };
    const double u1 = KIND == 1 ? central(l1, usmall) : 0.0, u2 = KIND == 1 ? central(l2, usmall) : 0.0;

    // upwards, j = d + k
    double se = 0.0, so = 0.0, n_lo = 0.0, p_lo = 0.0;
    double fprev = 0.0, fcur = 1.0, acur = 0.0, w = 0.0, t = 0.0;
    if (KIND == 1) {
        w = central(d, usmall) * u2 / ((2.0 * l1 + 1.0) * u1);
        t = (l1 & 1) ? -sqrt(w) : sqrt(w);
    }
    for (int k = 0; k <= l2; ++k) {
        const int j = d + k;
        const double wj = j <= lw ? W[j] : 0.0;
        const double g = (2.0 * j + 1.0) * fcur;
        n_lo += g * fcur;
        if (KIND == 2) {
            if (k & 1) so += g * fcur * wj;
            else se += g * fcur * wj;
        } else if (!(k & 1)) {
            p_lo += g * t * wj;
            if (k + 2 <= l2) {
                double num, den;
                w_ratio((double)(l1 + k / 2), (double)(k / 2), (double)(d + k / 2), (double)(l2 - k / 2), num, den);
                w = w * num / den;
                t = -copysign(sqrt(w), t);
            }
        }
        const double anext = a_of(j + 1);
        const double fnext = (4.0 * (2.0 * j + 1.0) * fcur - acur * fprev) / anext;
        fprev = fcur; fcur = fnext; acur = anext;
    }
    const double flo_m = fprev, flo_m1 = fcur;                     // f(l1), f(l1 + 1) in the lower piece's units

    // downwards, j = top - k
    double te = 0.0, to = 0.0, n_hi = 0.0, p_hi = 0.0;
    double fnext = 0.0, anext = 0.0;
    fcur = 1.0;
    if (KIND == 1) {
        w = u1 * u2 / ((2.0 * top + 1.0) * central(top, usmall));
        t = (top & 1) ? -sqrt(w) : sqrt(w);
    }
    for (int k = 0; k < l2; ++k) {
        const int j = top - k;
        const double wj = j <= lw ? W[j] : 0.0;
        const double g = (2.0 * j + 1.0) * fcur;
        n_hi += g * fcur;
        if (KIND == 2) {
            if (k & 1) to += g * fcur * wj;
            else te += g * fcur * wj;
        } else if (!(k & 1)) {
            p_hi += g * t * wj;
            if (k + 3 <= l2) {
                double num, den;                                    // w(j) / w(j - 2)
                w_ratio((double)(top - k / 2 - 1), (double)(l2 - k / 2 - 1), (double)(l1 - k / 2 - 1), (double)(k / 2 + 1), num, den);
                w = w / (num / den);
                t = -copysign(sqrt(w), t);
            }
        }
        const double aj = a_of(j);
        const double fdown = (4.0 * (2.0 * j + 1.0) * fcur - anext * fnext) / aj;
        fnext = fcur; fcur = fdown; anext = aj;
    }
    const double fhi_m1 = fnext, fhi_m = fcur;                     // f(l1 + 1), f(l1) in the upper piece's units
    const double lam = (flo_m * fhi_m + flo_m1 * fhi_m1) / (fhi_m * fhi_m + fhi_m1 * fhi_m1);
    const double norm = n_lo + lam * lam * n_hi;
    if (KIND == 2) {
        x0 = (se + lam * lam * te) / norm;
        x1 = (so + lam * lam * to) / norm;
    } else {
        const double sign = ((d & 1) != (lam < 0.0)) ? -1.0 : 1.0;   // f(top) has the sign (-1)^(l1 - l2)
        x0 = sign * (p_lo + lam * p_hi) / sqrt(norm);
        x1 = 0.0;
    }
}

// grid: lmax + 1 workgroups, the longest columns first; block: 64 * block_waves(lmax, lw); LDS: lds_bytes(lmax, lw)
template <int KIND>
__global__ void __launch_bounds__(kWave * kMaxWaves) pcl_coupling_kernel(int lmax, int lw, const double *__restrict__ wl,
                                                                         double *__restrict__ m0, double *__restrict__ m1)
{
    extern __shared__ double pcl_lds[];
    double *usmall = pcl_lds, *W = pcl_lds + kUSmall;
    const int lp = lmax - (int)blockIdx.x;
    if (KIND != 0 && lp < 2) return;                                // (the whole workgroup)
    const int nw = min(lw, 2 * lmax) + 1;
    for (int i = threadIdx.x; i < nw; i += blockDim.x) W[i] = wl[i];
    if (threadIdx.x < kUSmall) {
        double p = 1.0;
        for (int k = 1; k <= (int)threadIdx.x; ++k) p *= (2.0 * k - 1.0) / (2.0 * k);
        usmall[threadIdx.x] = p;
    }
    __syncthreads();
    const int lend = min(lmax, lp + lw);                            // the band's last row of this column
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, nwaves = blockDim.x / kWave;
    const size_t n = (size_t)lmax + 1;
    const double four_pi = 4.0 * M_PI;
    for (int l0 = lp + wave * kWave; l0 <= lend; l0 += nwaves * kWave) {
        const int l = l0 + lane;
        const int l1 = min(l, lend);                                // (a lane past the end repeats the last row and writes nothing)
        double x0, x1 = 0.0;
        if (KIND == 0) x0 = x00(l1, lp, lw, W, usmall);
        else x22<KIND>(l1, lp, lw, W, usmall, x0, x1);
        if (l <= lend) {
            const double pre_c = (2.0 * lp + 1.0) / four_pi, pre_r = (2.0 * l + 1.0) / four_pi;
            m0[(size_t)l * n + lp] = pre_c * x0;
            m0[(size_t)lp * n + l] = pre_r * x0;
            if (KIND == 2) {
                m1[(size_t)l * n + lp] = pre_c * x1;
                m1[(size_t)lp * n + l] = pre_r * x1;
            }
        }
    }
}

}  // namespace pcl
