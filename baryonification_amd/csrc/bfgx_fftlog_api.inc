// C ABI of the FFTLog path (include/bfgx.h, "pixel-window convolution"); included by bfgx_api.hip.
#include <complex>

namespace {

// The coefficients are worked out in long double (64 bits of mantissa on x86-64) and rounded to double once: in double the
// recurrence and Stirling's series, terms of size 30 that cancel to ln Gamma = O(1), cost 18 x 2^-52 in ln u_m (tests/test_fftlog_host.py).
using real = long double;
using creal = std::complex<real>;
constexpr real kPiL = 3.141592653589793238462643383279502884L, kLn2L = 0.693147180559945309417232121458176568L;

// log sin(pi z), up to a multiple of 2 pi i.  Re z is reduced by its nearest integer k before it meets pi (sin(pi z) =
// (-1)^k sin(pi (z - k)), and z - k is exact), so the zeros at the integers are exact zeros (log -> -inf) and the phase beside
// them is right.  For pi |Im z| > 20 -- sinh and cosh overflow further out, in double from Im z = 226, which a grid of 332 points
// per decade reaches -- the dominant exponential is taken out:
//   sin(pi w) = (i / 2) e^(pi y) e^(-i pi x) (1 - e^(2 i pi w)),   w = x + i y, y > 0;   the conjugate for y < 0
creal clogsinpi(creal z)
{
    const real k = std::round(z.real()), x = z.real() - k, y = z.imag(), ay = std::fabs(y);
    const real turn = (std::fmod(k, (real)2) != 0) ? kPiL : 0;                // log (-1)^k
    if (kPiL * ay <= 20)
        return std::log(creal(std::sin(kPiL * x) * std::cosh(kPiL * y), std::cos(kPiL * x) * std::sinh(kPiL * y))) + creal(0, turn);
    const real t = std::exp(-2 * kPiL * ay);
    const creal up = creal(kPiL * ay - kLn2L, kPiL / 2 - kPiL * x) + std::log(creal(1 - t * std::cos(2 * kPiL * x), -t * std::sin(2 * kPiL * x)));
    return (y > 0 ? up : std::conj(up)) + creal(0, turn);
}

// ln Gamma(z) for complex z, up to a multiple of 2 pi i (real part +inf on the poles): recurrence up to Re z >= 12, then Stirling's series
creal clngamma(creal z)
{
    if (z.real() < 0.5)                                       // reflection: Gamma(z) Gamma(1 - z) = pi / sin(pi z)
        return std::log(creal(kPiL, 0)) - clogsinpi(z) - clngamma(creal(1, 0) - z);
    creal shift(0, 0);
    while (z.real() < 12) { shift += std::log(z); z += (real)1; }
    const creal zi = (real)1 / z, zi2 = zi * zi;
    // B_2k / (2k (2k - 1)): 1/12, -1/360, 1/1260, -1/1680, 1/1188, -691/360360, 1/156
    const creal ser = zi * (1 / (real)12 + zi2 * (-1 / (real)360 + zi2 * (1 / (real)1260 + zi2 * (-1 / (real)1680 + zi2 * (1 / (real)1188 +
                      zi2 * (-691 / (real)360360 + zi2 * (1 / (real)156)))))));
    return (z - (real)0.5) * std::log(z) - z + std::log(2 * kPiL) / 2 + ser - shift;
}

// FFTLog's low-ringing ln(k_c r_c) nearest to lnkr (Hamilton 2000 eq. B22)
double fftlog_good_lnkr(double dln, double mu, double q, double lnkr)
{
    const real xp = ((real)mu + 1 + q) / 2, xm = ((real)mu + 1 - q) / 2, y = kPiL / (2 * (real)dln);
    const real argp = clngamma({xp, y}).imag(), argm = clngamma({xm, y}).imag();
    const real arg = (kLn2L - lnkr) / dln + (argp + argm) / kPiL;
    return (double)(lnkr + (arg - std::round(arg)) * dln);
}

// u_m, m = 0 .. n/2 (Hamilton 2000 eq. B18)
void fftlog_u(int n, double dln, double mu, double q, double lnkr, std::vector<double> &u /* (re, im) pairs */)
{
    const int nh = n / 2;
    u.resize(2 * (size_t)(nh + 1));
    const real xp = ((real)mu + 1 + q) / 2, xm = ((real)mu + 1 - q) / 2;
    for (int m = 0; m <= nh; ++m) {
        const real y = kPiL * m / ((real)n * dln);
        if (m == 0 && xm <= 0 && xm == std::round(xm)) { u[0] = u[1] = 0.0; continue; }   // a pole of the denominator Gamma: u_0 = 0
        const creal gp = clngamma({xp, y}), gm = clngamma({xm, y});
        const real amp = std::exp(q * kLn2L + gp.real() - gm.real());
        const real ph = 2 * y * (kLn2L - lnkr) + gp.imag() + gm.imag();
        u[2 * m] = (double)(amp * std::cos(ph));
        u[2 * m + 1] = (double)(amp * std::sin(ph));
    }
    if (n % 2 == 0) u[2 * nh + 1] = 0.0;                      // the Nyquist coefficient is made real
}

// one _fftlog_transform(rs, ., dim, mu, plaw) laid out for fht_rows_kernel: pre / post factors, u, output grid
struct FftlogStage {
    std::vector<double> pre, post, u, k;
    double lnkr;                                              // ln(k_c r_c)
};

int fftlog_stage(int n, const double *r, int dim, double mu, double plaw, FftlogStage &s)
{
    if (dim != 2 && dim != 3) return fail(BFGX_ERR_INVALID, "fftlog: dim must be 2 or 3");
    if (n < 4 || n > kFhtMaxN) return fail(BFGX_ERR_INVALID, "fftlog: grid length must be in [4, %d]", kFhtMaxN);
    for (int i = 0; i < n; ++i) if (!(r[i] > 0) || (i && !(r[i] > r[i - 1]))) return fail(BFGX_ERR_INVALID, "fftlog: grid must be positive and ascending");
    const double dln = std::log(r[n - 1] / r[0]) / (n - 1.0);
    const double q = dim / 2.0 + plaw;                        // bias exponent: CCL's default power-law indices give q = 0
    const double mub = (dim == 3) ? mu + 0.5 : mu;
    const double xp = (mub + 1 + q) / 2;
    if (xp <= 0 && xp == std::round(xp))                      // Gamma((mu + 1 + q) / 2) in u_0
        return fail(BFGX_ERR_INVALID, "fftlog: dim %d, mu %g, power-law index %g put a pole of Gamma in the m = 0 coefficient", dim, mu, plaw);
    const double lnkr = s.lnkr = fftlog_good_lnkr(dln, mub, q, 0.0);
    fftlog_u(n, dln, mub, q, lnkr, s.u);
    s.pre.resize(n); s.post.resize(n); s.k.resize(n);
    const double ekr = std::exp(lnkr);
    for (int j = 0; j < n; ++j) {
        s.pre[j] = std::pow(r[j], (dim == 3 ? 1.5 : 1.0) - q);
        const double k = ekr / r[n - 1 - j];
        s.k[j] = k;
        s.post[j] = (dim == 3) ? std::pow(2 * M_PI * k, -1.5) * std::pow(k, -q) : std::pow(k, -(1.0 + q)) / (2 * M_PI);
    }
    return BFGX_OK;
}

int launch_fht(int nrows, int n, const double *in, const double *pre, const double *u, const double *post, double *out)
{
    const size_t lds = fht_lds_bytes(n);
    HIP_TRY(hipFuncSetAttribute((const void *)fht_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(fht_rows_kernel, dim3((unsigned)nrows), dim3(kFhtThreads), lds, 0, n, in, pre, (const double2 *)u, post, out);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

}  // namespace

extern "C" {

int bfgx_fftlog_kgrid(int32_t n, const double *r, int32_t dim, double mu, double plaw, double *k_out)
{
    if (!r || !k_out) return fail(BFGX_ERR_INVALID, "NULL argument");
    FftlogStage s;
    if (int rc = fftlog_stage(n, r, dim, mu, plaw, s)) return rc;
    std::memcpy(k_out, s.k.data(), sizeof(double) * n);
    return BFGX_OK;
}

int bfgx_fftlog_u(int32_t n, const double *r, int32_t dim, double mu, double plaw, double *u_out, double *lnkr_out)
{
    if (!r || !u_out || !lnkr_out) return fail(BFGX_ERR_INVALID, "NULL argument");
    FftlogStage s;
    if (int rc = fftlog_stage(n, r, dim, mu, plaw, s)) return rc;
    std::memcpy(u_out, s.u.data(), sizeof(double) * s.u.size());
    *lnkr_out = s.lnkr;
    return BFGX_OK;
}

int bfgx_pchip_rows(int device, int64_t nrows, int32_t n, const double *x, const double *y, int32_t nq, const double *q, double *out)
{
    if (!x || !y || !q || !out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (nrows < 1 || nrows > 65535 || n < 2 || nq < 1) return fail(BFGX_ERR_INVALID, "pchip: 1 <= nrows <= 65535, n >= 2, nq >= 1");
    for (int i = 1; i < n; ++i) if (!(x[i] > x[i - 1])) return fail(BFGX_ERR_INVALID, "pchip: x must be strictly ascending");
    HostCall c(device);
    const double *dx = c.in(x, n), *dy = c.in(y, nrows * n), *dq = c.in(q, nq);
    double *dout = c.out(out, nrows * nq);
    if (int rc = c.ready()) return rc;
    hipLaunchKernelGGL(pchip_rows_kernel, dim3((unsigned)((nq + 255) / 256), (unsigned)nrows), dim3(256), 0, 0, n, dx, dy, nq, dq, 1.0, dout);
    return c.finish();
}

int bfgx_fftlog_transform(int device, int64_t nrows, int32_t n, const double *r, const double *f, int32_t dim, double mu, double plaw,
                          double *k_out, double *F_out)
{
    if (!r || !f || !k_out || !F_out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (nrows < 1 || nrows > 65535) return fail(BFGX_ERR_INVALID, "fftlog: 1 <= nrows <= 65535");
    FftlogStage s;
    if (int rc = fftlog_stage(n, r, dim, mu, plaw, s)) return rc;
    HostCall c(device);
    const double *din = c.in(f, nrows * n), *dpre = c.in(s.pre.data(), n), *du = c.in(s.u.data(), s.u.size()), *dpost = c.in(s.post.data(), n);
    double *dout = c.out(F_out, nrows * n);
    if (int rc = c.ready()) return rc;
    if (int rc = launch_fht((int)nrows, n, din, dpre, du, dpost, dout)) return rc;
    if (int rc = c.finish()) return rc;
    std::memcpy(k_out, s.k.data(), sizeof(double) * n);
    return BFGX_OK;
}

int bfgx_fftlog_convolve(int device, int64_t nrows, int32_t n, const double *r_fft, const double *prof, int32_t dim, double mu,
                         double plaw_fwd, double plaw_back, const double *window, int32_t nq, const double *r_eval, double r_scale,
                         double *out)
{
    if (!r_fft || !prof || !window || !r_eval || !out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (nrows < 1 || nrows > 65535 || nq < 1) return fail(BFGX_ERR_INVALID, "fftlog: bad sizes");
    if (!(r_scale > 0)) return fail(BFGX_ERR_INVALID, "fftlog: r_scale must be > 0");
    FftlogStage s1, s2;
    if (int rc = fftlog_stage(n, r_fft, dim, mu, plaw_fwd, s1)) return rc;          // Pixel.py:146 / :208
    if (int rc = fftlog_stage(n, s1.k.data(), dim, mu, plaw_back, s2)) return rc;   // :147 / :209
    std::vector<double> mid(n), lnr(n), lnq(nq);
    for (int j = 0; j < n; ++j) {
        mid[j] = s1.post[j] * window[j] * s2.pre[j];                                 // Pk * Pixel.real(k_out), ready for the back transform
        lnr[j] = std::log(s2.k[j] * r_scale);                                        // np.log(r_out) (r_out * D_A when harmonic, :216)
    }
    for (int i = 0; i < nq; ++i) lnq[i] = std::log(r_eval[i]);
    HostCall c(device);
    const double *din = c.in(prof, nrows * n), *dpre = c.in(s1.pre.data(), n), *du1 = c.in(s1.u.data(), s1.u.size()), *dmid = c.in(mid.data(), n);
    double *dtmp = c.scratch<double>(nrows * n);
    const double *du2 = c.in(s2.u.data(), s2.u.size()), *dpost = c.in(s2.post.data(), n);
    double *dg = c.scratch<double>(nrows * n);
    const double *dx = c.in(lnr.data(), n), *dq = c.in(lnq.data(), nq);
    double *dout = c.out(out, nrows * nq);
    if (int rc = c.ready()) return rc;
    if (int rc = launch_fht((int)nrows, n, din, dpre, du1, dmid, dtmp)) return rc;
    if (int rc = launch_fht((int)nrows, n, dtmp, nullptr, du2, dpost, dg)) return rc;
    const double scale = (dim == 3) ? 8 * M_PI * M_PI * M_PI : 4 * M_PI * M_PI;      // (2 pi)^dim, :155 / :222
    hipLaunchKernelGGL(pchip_rows_kernel, dim3((unsigned)((nq + 255) / 256), (unsigned)nrows), dim3(256), 0, 0, n, dx, dg, nq, dq, scale, dout);
    return c.finish();
}

}  // extern "C"
