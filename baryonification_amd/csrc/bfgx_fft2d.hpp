// bfgx_fft2d.hpp -- 2-D FFTs of gridded flat-sky maps and what is computed per Fourier mode on top of them (power spectra in linear
// k-bins, isotropic filters, the Kaiser-Squires pair, the derivatives of a filtered map) for gfx950.
//
// Layout: a real map [N][N] (C order, axis 0 = x, axis 1 = y) <-> its half spectrum [N][pitch] of double2, pitch = fft_pitch(N), the
// coefficients c <= N/2 of axis 1 -- one plane of the 3-D code's layout (bfgx_fft.hpp).  Unnormalised, exponent -i forward.
// Rows (axis 1) are transformed by fft_r2c_lines_kernel / fft_c2r_lines_kernel, one pair of lines per workgroup.
// Columns (axis 0):
//   N <= 1024   fft_c2c_strided_kernel<0> as the 3-D plane passes use it, in place (a tile of 8 or 4 whole columns in LDS);
//   N  > 1024   a column no longer fits that pass, so it is split in four steps, N = N1 N2 with N1, N2 <= 64 (2048 = 64 x 32,
//               4096 = 64 x 64).  With the row index r = r1 N2 + r2 and the coefficient k = k1 + N1 k2,
//                   X[k1 + N1 k2] = sum_r2 w_N2^(r2 k2) { w_N^(r2 k1) sum_r1 w_N1^(r1 k1) x[r1 N2 + r2] }:
//               pass A does the N1-point transforms over rows at stride N2, times w_N^(r2 k1), in place (row r1 N2 + r2 becomes row
//               k1 N2 + r2, the same set of rows); pass B does the N2-point transforms over N2 contiguous rows and stores row k1 + N1 k2
//               of another buffer.  Both are fft2_col_step_kernel: tiles of 8 adjacent columns (whole 128-byte lines) x 4 adjacent
//               transforms, 32 lines of at most 64 points in 33 KB of LDS, butterflies by lds_fft_stages.
// The inverse is the forward transform of the conjugate (bfgx_bispec.hpp): the per-mode kernels below write conj(product) * scale, the
// column passes run as they are and fft_c2r_lines_kernel reads its input conjugated.  No transform uses atomics: bitwise repeatable.
// The per-mode kernels read the coefficients c <= N/2 only; pad columns are never read (they store zeros there).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bfgx_fft.hpp"
#include "bfgx_bispec.hpp"

namespace bfgx {

constexpr int kFft2Threads = 256;
constexpr int kFft2Cols = 8;               // adjacent columns of a tile of the split column passes: one 128-byte line per row
constexpr int kFft2Group = 4;              // adjacent transforms (rows r2 of pass A, k1 of pass B) of a tile
constexpr int kFft2Lines = kFft2Cols * kFft2Group;
constexpr int kFft2MaxPoints = 64;         // N1, N2 <= 64
constexpr int kFft2MaxNk = 2048;

__host__ __device__ inline size_t fft2_col_step_lds_bytes(int ne) { return sizeof(double2) * ((size_t)ne * kFft2Lines + (size_t)(ne >> 1)); }

// One pass of the split column transform.  Tile (jg, ct) holds the lines (j, col), j = 4 jg .. 4 jg + 3, col = 8 ct .. 8 ct + 7; point e
// of line (j, col) is read from row e * src_e + j * src_j of `src` and coefficient k is stored to row k * dst_e + j * dst_j of `dst`
// (rows of `pitch` values; pitch % 8 == 0, nj % 4 == 0).  tw_e[i] = exp(-2 pi i i / ne), i < ne / 2.  TWIDDLE: coefficient k of line j is
// multiplied by tw_n[j * k], tw_n[i] = exp(-2 pi i i / N), i < N = ne * nj.  src may be dst where a tile reads and writes the same rows
// (pass A): every load of a tile is in LDS before its first store.
template <bool TWIDDLE>
__global__ void __launch_bounds__(kFft2Threads)
fft2_col_step_kernel(const double2 *src, double2 *dst, int ne, int log2ne, int pitch, int64_t src_e, int64_t src_j, int64_t dst_e, int64_t dst_j,
                     const double2 *__restrict__ tw_e, const double2 *__restrict__ tw_n)
{
    extern __shared__ double2 fbuf[];
    constexpr int NL = kFft2Lines;
    double2 *twl = fbuf + (size_t)ne * NL;
    const int tid = threadIdx.x;
    for (int i = tid; i < (ne >> 1); i += kFft2Threads) twl[i] = tw_e[i];
    const int ctiles = pitch / kFft2Cols;
    const int c0 = (int)(blockIdx.x % ctiles) * kFft2Cols, j0 = (int)(blockIdx.x / ctiles) * kFft2Group;
    for (int t = tid; t < ne * NL; t += kFft2Threads) {
        const int l = t & (NL - 1), e = t / NL;
        const int j = j0 + l / kFft2Cols, col = c0 + (l & (kFft2Cols - 1));
        fbuf[bit_reverse(e, log2ne) * NL + l] = src[((int64_t)e * src_e + (int64_t)j * src_j) * pitch + col];
    }
    lds_fft_stages(fbuf, ne, NL, twl, tid, kFft2Threads);
    for (int t = tid; t < ne * NL; t += kFft2Threads) {
        const int l = t & (NL - 1), k = t / NL;
        const int j = j0 + l / kFft2Cols, col = c0 + (l & (kFft2Cols - 1));
        double2 f = fbuf[k * NL + l];
        if (TWIDDLE) f = cmul(f, tw_n[j * k]);
        dst[((int64_t)k * dst_e + (int64_t)j * dst_j) * pitch + col] = f;
    }
}

// fftfreq's integer wave number of index i
__device__ inline int fft2_wave_number(int i, int N) { return 2 * i < N ? i : i - N; }

// what the per-mode kernels share: the k axis of the 3-D code, klin[i] = n_i * kval (FftSetup::init's product, one rounding)
struct Fft2Bins {
    double kval, kb0, dk, inv_dk;
    int nk;
    double *paa_sum, *pbb_sum, *pab_sum, *k_sum;
    unsigned long long *counts;
};

__host__ __device__ inline size_t fft2_bin_lds_bytes(int N, int nk) { return sizeof(double) * ((size_t)N + 5 * (size_t)nk); }

// Per linear k-bin the sums of w m |F_A|^2, w m |F_B|^2, w m Re(F_A conj F_B), m k and m over the modes (a, c), c <= N/2, of two finished
// half spectra (which may be the same): m = 2 for 0 < c < N/2 (the mirrored half), w = win[a] win[c].  The bin is pk_bin_of's with the
// third index at 0 (klin[0] = 0 adds nothing to the sum of squares): the k axis is built in LDS for it.  Persistent workgroups over the
// rows, LDS histograms, one flush per workgroup.
__global__ void __launch_bounds__(kFft2Threads)
fft2_bin_kernel(const double2 *__restrict__ spec_a, const double2 *__restrict__ spec_b, int N, int pitch, Fft2Bins fb, const double *__restrict__ win)
{
    extern __shared__ double2 fbuf[];
    double *klin = reinterpret_cast<double *>(fbuf);
    double *haa = klin + N, *hbb = haa + fb.nk, *hab = hbb + fb.nk, *hk = hab + fb.nk;
    unsigned long long *hc = reinterpret_cast<unsigned long long *>(hk + fb.nk);
    const int tid = threadIdx.x, h = N >> 1;
    for (int i = tid; i < N; i += kFft2Threads) klin[i] = (double)(i < (N + 1) / 2 ? i : i - N) * fb.kval;
    for (int i = tid; i < fb.nk; i += kFft2Threads) { haa[i] = 0.0; hbb[i] = 0.0; hab[i] = 0.0; hk[i] = 0.0; hc[i] = 0ull; }
    __syncthreads();
    PkBins pb{};
    pb.klin = klin; pb.kb0 = fb.kb0; pb.dk = fb.dk; pb.inv_dk = fb.inv_dk; pb.nk = fb.nk;
    const bool same = spec_a == spec_b;
    for (int a = blockIdx.x; a < N; a += gridDim.x) {
        const double wa = win[a];
        for (int c = tid; c <= h; c += kFft2Threads) {
            double k;
            const int bin = pk_bin_of(pb, a, 0, c, k);
            if (bin < 0) continue;
            const double2 fa = spec_a[(int64_t)a * pitch + c];
            const double2 fbv = same ? fa : spec_b[(int64_t)a * pitch + c];
            const int mult = (c > 0 && c < h) ? 2 : 1;
            const double w = (double)mult * (wa * win[c]);
            atomicAdd(haa + bin, w * (fa.x * fa.x + fa.y * fa.y));
            atomicAdd(hbb + bin, w * (fbv.x * fbv.x + fbv.y * fbv.y));
            atomicAdd(hab + bin, w * (fa.x * fbv.x + fa.y * fbv.y));
            atomicAdd(hk + bin, mult * k);
            atomicAdd(hc + bin, (unsigned long long)mult);
        }
    }
    __syncthreads();
    for (int i = tid; i < fb.nk; i += kFft2Threads) {
        if (!hc[i]) continue;
        atomicAdd(fb.paa_sum + i, haa[i]); atomicAdd(fb.pbb_sum + i, hbb[i]); atomicAdd(fb.pab_sum + i, hab[i]);
        atomicAdd(fb.k_sum + i, hk[i]); atomicAdd(fb.counts + i, hc[i]);
    }
}

// the isotropic filters b(k)
enum { kFft2Gauss = 0, kFft2TopHat = 1, kFft2Table = 2, kFft2Unit = 3 };

// np.interp(k, tk, tb): linear between the nodes, held at the end values
__device__ inline double fft2_table_beam(double k, const double *__restrict__ tk, const double *__restrict__ tb, int nt)
{
    if (!(k > tk[0])) return tb[0];
    if (k >= tk[nt - 1]) return tb[nt - 1];
    int lo = 0, hi = nt - 1;                                         // tk[lo] <= k < tk[hi]
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (tk[mid] <= k) lo = mid; else hi = mid; }
    const double slope = (tb[hi] - tb[lo]) / (tk[hi] - tk[lo]);
    return slope * (k - tk[lo]) + tb[lo];
}

// b(k) of mode (a, c), k = kval sqrt(n0^2 + n1^2) with fftfreq's n0 and n1 = c.  kind: Gaussian b = exp(-k^2 param^2 / 2); top hat
// b = 2 J1(k param) / (k param), 1 at k param = 0; table (tk, tb)[nt]; unit b = 1.  One statement of the arithmetic for the per-mode kernels
__device__ inline double fft2_beam(int a, int c, int N, int kind, double kval, double param, const double *__restrict__ tk,
                                   const double *__restrict__ tb, int nt)
{
    double b = 1.0;
    if (kind != kFft2Unit) {
        const double n0 = (double)fft2_wave_number(a, N), n1 = (double)c;
        const double k = kval * sqrt(n0 * n0 + n1 * n1);
        if (kind == kFft2Gauss) b = exp(-0.5 * (k * param) * (k * param));
        else if (kind == kFft2TopHat) { const double x = k * param; b = x > 0.0 ? 2.0 * j1(x) / x : 1.0; }
        else b = fft2_table_beam(k, tk, tb, nt);
    }
    return b;
}

// out = conj(F) * b(k) * scale, ready for the inverse passes (unit: the conjugation alone, bfgx_irfft2_device).  out may be `spec`.
// Pad columns are stored as zeros and not read.
__global__ void __launch_bounds__(kFft2Threads)
fft2_filter_kernel(const double2 *spec, double2 *out, int N, int pitch, int kind, double kval, double param, const double *__restrict__ tk,
                   const double *__restrict__ tb, int nt, double scale)
{
    const int h = N >> 1;
    const unsigned total = (unsigned)N * pitch;                      // (at most 4096 * 2056 < 2^24)
    for (unsigned t = blockIdx.x * kFft2Threads + threadIdx.x; t < total; t += gridDim.x * kFft2Threads) {
        const int a = (int)(t / (unsigned)pitch), c = (int)(t - (unsigned)a * pitch);
        double2 v = make_double2(0.0, 0.0);
        if (c <= h) {
            const double b = fft2_beam(a, c, N, kind, kval, param, tk, tb, nt);
            const double2 f = spec[t];
            const double s = b * scale;
            v = make_double2(f.x * s, -f.y * s);
        }
        out[t] = v;
    }
}

// The derivatives of a filtered map from its half spectrum, one pass over the modes: `spec` [N][pitch] (as bfgx_rfft2_device leaves it) is
// read once and kept, b(k) is evaluated once per mode, and out[d][N][pitch], d < nder, receives conj(F m_d b) * scale, ready for the
// inverse passes.  With n0 = fft2_wave_number(a, N) (axis 0, x), n1 = c (axis 1, y), g0 = kval n0, g1 = kval n1, h = N / 2:
//   u 1;  u_x i g0 (0 where a == h);  u_y i g1 (0 where c == h);  u_xx -g0^2;  u_xy -g0 g1 (0 where a == h or c == h);  u_yy -g1^2
// (a factor that is odd in an index is set to 0 at that index's Nyquist value, the rule of fft2_ks_angles' s2: it would break the Hermitian
// symmetry of a real map's spectrum there).  spin_form == 0: [u, u_x, u_y, u_xx, u_xy, u_yy]; spin_form != 0: [u, u_x, u_y, lap, q_plus,
// q_cross] with the multipliers -(g0^2 + g1^2), -(g0^2 - g1^2), -2 g0 g1 (q_cross with u_xy's zero rule).  nder = 1 writes u alone, with
// the arithmetic of fft2_filter_kernel.  out must not overlap spec.  Pad columns are stored as zeros and not read.
__global__ void __launch_bounds__(kFft2Threads)
fft2_der_kernel(const double2 *__restrict__ spec, double2 *__restrict__ out, int N, int pitch, int kind, double kval, double param,
                const double *__restrict__ tk, const double *__restrict__ tb, int nt, double scale, int nder, int spin_form)
{
    const int h = N >> 1;
    const unsigned total = (unsigned)N * pitch;                      // (at most 4096 * 2056 < 2^24)
    for (unsigned t = blockIdx.x * kFft2Threads + threadIdx.x; t < total; t += gridDim.x * kFft2Threads) {
        const int a = (int)(t / (unsigned)pitch), c = (int)(t - (unsigned)a * pitch);
        const double2 zero = make_double2(0.0, 0.0);
        double2 v[6] = {zero, zero, zero, zero, zero, zero};
        if (c <= h) {
            const double b = fft2_beam(a, c, N, kind, kval, param, tk, tb, nt);
            const double2 f = spec[t];
            const double s = b * scale;
            const double fx = f.x * s, fy = f.y * s;                 // F b scale
            v[0] = make_double2(fx, -fy);
            if (nder > 1) {
                const double g0 = kval * (double)fft2_wave_number(a, N), g1 = kval * (double)c;
                const double o0 = a != h ? g0 : 0.0, o1 = c != h ? g1 : 0.0;      // the odd factors
                v[1] = make_double2(-(o0 * fy), -(o0 * fx));         // conj(i g (fx + i fy)) = -g fy - i g fx
                v[2] = make_double2(-(o1 * fy), -(o1 * fx));
                const double m00 = g0 * g0, m11 = g1 * g1, m01 = o0 * o1;
                const double m3 = spin_form ? m00 + m11 : m00, m4 = spin_form ? m00 - m11 : m01, m5 = spin_form ? 2.0 * m01 : m11;
                v[3] = make_double2(-(m3 * fx), m3 * fy);            // conj(-m (fx + i fy))
                v[4] = make_double2(-(m4 * fx), m4 * fy);
                v[5] = make_double2(-(m5 * fx), m5 * fy);
            }
        }
#pragma unroll
        for (int d = 0; d < 6; ++d)
            if (d < nder) out[(size_t)d * total + t] = v[d];
    }
}

// The Kaiser-Squires rotation of mode (a, c): c2 = (n0^2 - n1^2) / (n0^2 + n1^2), s2 = 2 n0 n1 / (n0^2 + n1^2) with fftfreq's n0 and
// n1 = c; both 0 at the zero mode; s2 = 0 where either index is the Nyquist index (the product is odd there and would break the
// Hermitian symmetry of a real map's spectrum); only n0^2 enters c2, so the sign of the Nyquist wave number does not matter.
__device__ inline void fft2_ks_angles(int a, int c, int N, double &c2, double &s2)
{
    const int h = N >> 1;
    const double n0 = (double)fft2_wave_number(a, N), n1 = (double)c;
    const double d = n0 * n0 + n1 * n1;
    c2 = 0.0; s2 = 0.0;
    if (d > 0.0) {
        c2 = (n0 * n0 - n1 * n1) / d;
        if (a != h && c != h) s2 = 2.0 * n0 * n1 / d;
    }
}

// In place on two half spectra, both results conjugated and times `scale`, ready for the inverse passes.
//   eb = 0, convergence to shear: s1 holds kappa^;            s1 <- c2 kappa^,            s2 <- s2 kappa^
//   eb = 1, shear to E / B:       s1, s2 hold g1^, g2^;       s1 <- c2 g1^ + s2 g2^,      s2 <- -s2 g1^ + c2 g2^
// Pad columns are stored as zeros and not read.
__global__ void __launch_bounds__(kFft2Threads)
fft2_ks_kernel(double2 *__restrict__ s1, double2 *__restrict__ s2, int N, int pitch, int eb, double scale)
{
    const int h = N >> 1;
    const unsigned total = (unsigned)N * pitch;
    for (unsigned t = blockIdx.x * kFft2Threads + threadIdx.x; t < total; t += gridDim.x * kFft2Threads) {
        const int a = (int)(t / (unsigned)pitch), c = (int)(t - (unsigned)a * pitch);
        double2 u = make_double2(0.0, 0.0), v = u;
        if (c <= h) {
            double c2, sn2;
            fft2_ks_angles(a, c, N, c2, sn2);
            const double2 f1 = s1[t];
            if (eb) {
                const double2 f2 = s2[t];
                u = make_double2(c2 * f1.x + sn2 * f2.x, c2 * f1.y + sn2 * f2.y);
                v = make_double2(c2 * f2.x - sn2 * f1.x, c2 * f2.y - sn2 * f1.y);
            } else {
                u = make_double2(c2 * f1.x, c2 * f1.y);
                v = make_double2(sn2 * f1.x, sn2 * f1.y);
            }
            u = make_double2(u.x * scale, -u.y * scale);
            v = make_double2(v.x * scale, -v.y * scale);
        }
        s1[t] = u;
        s2[t] = v;
    }
}

}  // namespace bfgx
