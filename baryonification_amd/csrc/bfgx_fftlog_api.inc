// C ABI of the FFTLog path (include/bfgx.h, "pixel-window convolution"); included by bfgx_api.hip.
#include <complex>

namespace {

// ln Gamma(z) for complex z (any Re z except the poles): recurrence up to Re z >= 12, then Stirling's series
std::complex<double> clngamma(std::complex<double> z)
{
    using cd = std::complex<double>;
    if (z.real() < 0.5) {                                     // reflection: Gamma(z) Gamma(1 - z) = pi / sin(pi z)
        const cd s = std::sin(M_PI * z);
        return std::log(cd(M_PI, 0.0)) - std::log(s) - clngamma(cd(1.0, 0.0) - z);
    }
    cd shift(0.0, 0.0);
    while (z.real() < 12.0) { shift += std::log(z); z += 1.0; }
    const cd zi = 1.0 / z, zi2 = zi * zi;
    // B_2k / (2k (2k - 1)): 1/12, -1/360, 1/1260, -1/1680, 1/1188, -691/360360, 1/156
    cd ser = zi * (1.0 / 12.0 + zi2 * (-1.0 / 360.0 + zi2 * (1.0 / 1260.0 + zi2 * (-1.0 / 1680.0 + zi2 * (1.0 / 1188.0 +
             zi2 * (-691.0 / 360360.0 + zi2 * (1.0 / 156.0)))))));
    return (z - 0.5) * std::log(z) - z + 0.5 * std::log(2.0 * M_PI) + ser - shift;
}

// FFTLog's low-ringing ln(k_c r_c) nearest to lnkr (Hamilton 2000 eq. B22)
double fftlog_good_lnkr(double dln, double mu, double q, double lnkr)
{
    const double xp = (mu + 1 + q) / 2, xm = (mu + 1 - q) / 2, y = M_PI / (2 * dln);
    const double argp = clngamma({xp, y}).imag(), argm = clngamma({xm, y}).imag();
    const double arg = (M_LN2 - lnkr) / dln + (argp + argm) / M_PI;
    return lnkr + (arg - std::round(arg)) * dln;
}

// u_m, m = 0 .. n/2 (Hamilton 2000 eq. B18)
void fftlog_u(int n, double dln, double mu, double q, double lnkr, std::vector<double> &u /* (re, im) pairs */)
{
    const int nh = n / 2;
    u.resize(2 * (size_t)(nh + 1));
    const double xp = (mu + 1 + q) / 2, xm = (mu + 1 - q) / 2;
    for (int m = 0; m <= nh; ++m) {
        const double y = M_PI * m / (n * dln);
        const std::complex<double> gp = clngamma({xp, y}), gm = clngamma({xm, y});
        const double amp = std::exp(q * M_LN2 + gp.real() - gm.real());
        const double ph = 2 * y * (M_LN2 - lnkr) + gp.imag() + gm.imag();
        u[2 * m] = amp * std::cos(ph);
        u[2 * m + 1] = amp * std::sin(ph);
    }
    if (n % 2 == 0) u[2 * nh + 1] = 0.0;                      // the Nyquist coefficient is made real
}

// one _fftlog_transform(rs, ., dim, mu, plaw) laid out for fht_rows_kernel: pre / post factors, u, output grid
struct FftlogStage {
    std::vector<double> pre, post, u, k;
};

int fftlog_stage(int n, const double *r, int dim, double mu, double plaw, FftlogStage &s)
{
    if (dim != 2 && dim != 3) return fail(BFGX_ERR_INVALID, "fftlog: dim must be 2 or 3");
    if (n < 4 || n > kFhtMaxN) return fail(BFGX_ERR_INVALID, "fftlog: grid length must be in [4, %d]", kFhtMaxN);
    for (int i = 0; i < n; ++i) if (!(r[i] > 0) || (i && !(r[i] > r[i - 1]))) return fail(BFGX_ERR_INVALID, "fftlog: grid must be positive and ascending");
    const double dln = std::log(r[n - 1] / r[0]) / (n - 1.0);
    const double q = dim / 2.0 + plaw;                        // bias exponent: CCL's default power-law indices give q = 0
    const double mub = (dim == 3) ? mu + 0.5 : mu;
    const double lnkr = fftlog_good_lnkr(dln, mub, q, 0.0);
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
