// bfgx_fft2d_api.inc -- host side and C ABI of the 2-D FFTs of gridded maps (include/bfgx.h, "flat-sky maps"): the transform pair, power
// spectra, filters, the Kaiser-Squires pair and the derivatives of a filtered map; included by bfgx_api.hip after bfgx_fourier_host.inc
// (the checks, the table cache, the strided and line launchers, k_axis_bins, upload_owned) and bfgx_xpk_api.inc (xpk_window).
// Kernels: bfgx_fft2d.hpp, and the line and strided kernels of bfgx_fft.hpp / bfgx_bispec.hpp through a setup of their own.

namespace {

// twiddles of one (device, N), built in long double on the host
struct Fft2Setup {
    DevBuf dtw;                        // exp(-2 pi i k / N), k < N: the row passes and the strided pass read k < N/2, pass A all of it
    DevBuf dtw1, dtw2;                 // N > 1024: exp(-2 pi i k / N1), k < N1/2, and the same for N2
    int lg = 0, n1 = 0, n2 = 0, lg1 = 0, lg2 = 0;
    StridedShape sh;                   // N <= 1024
    int n_cu = 256;

    static int table(DevBuf &b, int n, int count)
    {
        std::vector<double> tw;
        unit_circle(tw, n, 0, count, -1);
        return b.up(tw.data(), sizeof(double) * tw.size()) ? 1 : 0;
    }
    int init(int device, int N)        // (device: the current one)
    {
        if (int rc = fourier_kernel_attrs(device)) return rc;
        lg = ilog2_exact(N);
        if (table(dtw, N, N)) return alloc_fail("2-D fft twiddles");
        if (N > kFft2StridedMaxN) {
            lg1 = (lg + 1) / 2; lg2 = lg - lg1;                       // 2048 = 64 x 32, 4096 = 64 x 64
            n1 = 1 << lg1; n2 = 1 << lg2;
            if (table(dtw1, n1, n1 / 2) || table(dtw2, n2, n2 / 2)) return alloc_fail("2-D fft twiddles");
        } else {
            sh = strided_shape(N);
        }
        n_cu = device_cu_count(device);
        return BFGX_OK;
    }
};

FourierCache<Fft2Setup, int> g_fft2;

int fft2_setup(int device, int N, Fft2Setup **out)
{
    return g_fft2.get(std::make_tuple(device, N), out, [&](Fft2Setup &f) { return f.init(device, N); });
}

// ---- argument checks, stated once (no device call); the host and the _device entries give the same messages
int fft2_check_n(int n) { return fourier_check_grid(n, kFft2MaxN, "2-D transforms need n = 2^m with 8 <= n <= 4096"); }

int fft2_check_bins(double L, int nk, int window_order)
{
    if (nk < 1 || nk > kFft2MaxNk) return fail(BFGX_ERR_INVALID, "2-D power spectrum needs 1 <= nk <= 2048");
    if (!(L > 0)) return fail(BFGX_ERR_INVALID, "2-D power spectrum needs L > 0");
    if (window_order < 0 || window_order > 3) return fail(BFGX_ERR_INVALID, "window_order %d: 0 (none), 1 (NGP), 2 (CIC) or 3 (TSC)", window_order);
    return BFGX_OK;
}

int fft2_check_filter(int n, double L, int kind, double param, const double *tk, const double *tb, int nt)
{
    if (!(L > 0)) return fail(BFGX_ERR_INVALID, "2-D filter needs L > 0");
    if (kind == kFft2Gauss || kind == kFft2TopHat) {
        if (!(param >= 0) || !std::isfinite(param)) return fail(BFGX_ERR_INVALID, "2-D filter needs a finite width >= 0 (sigma or R)");
        return BFGX_OK;
    }
    if (kind != kFft2Table) return fail(BFGX_ERR_INVALID, "2-D filter kind %d: 0 (Gaussian), 1 (top hat) or 2 (table)", kind);
    if (!tk || !tb) return fail(BFGX_ERR_INVALID, "NULL argument");
    // (the table rides in one half spectrum of the work array)
    const int most = (int)std::min<int64_t>(kFft2MaxTable, (int64_t)n * fft_pitch(n));
    if (nt < 1 || nt > most) return fail(BFGX_ERR_INVALID, "2-D filter table needs 1 <= nodes <= %d", most);
    for (int i = 0; i < nt; ++i) {
        if (!std::isfinite(tk[i]) || !std::isfinite(tb[i])) return fail(BFGX_ERR_INVALID, "2-D filter table must be finite");
        if (i && !(tk[i] > tk[i - 1])) return fail(BFGX_ERR_INVALID, "2-D filter table: k must be strictly ascending");
    }
    return BFGX_OK;
}

// ---- the transforms.  A work array holds three half spectra: s1, s2 (results and operands of the per-mode kernels) and u (the other
// side of the out-of-place column pass at N > 1024)
struct Fft2Work {
    double2 *s1, *s2, *u;
    Fft2Work(double *work, int N) : s1((double2 *)work), s2(s1 + (int64_t)N * fft_pitch(N)), u(s2 + (int64_t)N * fft_pitch(N)) {}
};

// forward complex transforms along axis 0 of the half spectrum `from` [N][pitch] -> `to`; N <= 1024: in place, from == to; N > 1024:
// `from` is scratch afterwards and must not be `to`
int fft2_columns(Fft2Setup &f, hipStream_t s, int N, double2 *from, double2 *to)
{
    const int pitch = fft_pitch(N);
    if (N <= kFft2StridedMaxN)
        return strided_launch<0>(f.sh, s, f.sh.ztiles, f.sh.lds, to, N, f.lg, f.dtw.as<double2>(), (int64_t)pitch, (int64_t)N * pitch, 1, PkBins{});
    const unsigned ctiles = (unsigned)(pitch / kFft2Cols);
    // pass A: lines r2, points r1 at rows r1 N2 + r2 -> rows k1 N2 + r2, times w_N^(r2 k1), in place
    hipLaunchKernelGGL((fft2_col_step_kernel<true>), dim3(ctiles * (unsigned)(f.n2 / kFft2Group)), dim3(kFft2Threads), fft2_col_step_lds_bytes(f.n1), s,
                       (const double2 *)from, from, f.n1, f.lg1, pitch, (int64_t)f.n2, (int64_t)1, (int64_t)f.n2, (int64_t)1, f.dtw1.as<double2>(),
                       f.dtw.as<double2>());
    HIP_TRY(hipGetLastError());
    // pass B: lines k1, points r2 at rows k1 N2 + r2 -> rows k1 + N1 k2 of the other buffer
    hipLaunchKernelGGL((fft2_col_step_kernel<false>), dim3(ctiles * (unsigned)(f.n1 / kFft2Group)), dim3(kFft2Threads), fft2_col_step_lds_bytes(f.n2), s,
                       (const double2 *)from, to, f.n2, f.lg2, pitch, (int64_t)1, (int64_t)f.n2, (int64_t)f.n1, (int64_t)1, f.dtw2.as<double2>(),
                       f.dtw.as<double2>());
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

// map [N][N] -> its half spectrum in `out`; `u`: scratch half spectrum (N > 1024 only)
int fft2_forward(Fft2Setup &f, hipStream_t s, int N, const double *map, double2 *out, double2 *u)
{
    const int pitch = fft_pitch(N);
    double2 *rows = N <= kFft2StridedMaxN ? out : u;
    if (int rc = lines_launch(false, s, N, f.lg, f.dtw.as<double2>(), (size_t)N / 2, map, rows, pitch)) return rc;
    HIP_TRY(hipGetLastError());
    return fft2_columns(f, s, N, rows, out);
}

// `spec` holds the CONJUGATE of the spectrum to invert, times the normalisation (what the per-mode kernels leave) -> map [N][N]; spec is
// scratch afterwards, `u` as above
int fft2_inverse_conj(Fft2Setup &f, hipStream_t s, int N, double2 *spec, double2 *u, double *map)
{
    const int pitch = fft_pitch(N);
    double2 *cols = N <= kFft2StridedMaxN ? spec : u;
    if (int rc = fft2_columns(f, s, N, spec, cols)) return rc;
    if (int rc = lines_launch(true, s, N, f.lg, f.dtw.as<double2>(), (size_t)N / 2, cols, map, pitch)) return rc;
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

int fft2_filter(Fft2Setup &f, hipStream_t s, int N, const double2 *spec, double2 *out, int kind, double L, double param, const double *tk,
                const double *tb, int nt, double scale)
{
    const int pitch = fft_pitch(N);
    hipLaunchKernelGGL(fft2_filter_kernel, dim3(stream_grid(f.n_cu, (int64_t)N * pitch)), dim3(kFft2Threads), 0, s, spec, out, N, pitch, kind,
                       2 * 3.141592653589793 / L, param, tk, tb, nt, scale);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

// the table of a filter rides in `dst`, a part of the work array that the stream first writes after the table's reader
int fft2_upload_beam(hipStream_t s, double *dst, const double *table_k_host, const double *table_b_host, int ntable)
{
    std::vector<double> beam(table_k_host, table_k_host + ntable);
    beam.insert(beam.end(), table_b_host, table_b_host + ntable);
    return upload_owned(s, dst, std::move(beam));
}

int fft2_ks(Fft2Setup &f, hipStream_t s, int N, double2 *s1, double2 *s2, int eb)
{
    const int pitch = fft_pitch(N);
    hipLaunchKernelGGL(fft2_ks_kernel, dim3(stream_grid(f.n_cu, (int64_t)N * pitch)), dim3(kFft2Threads), 0, s, s1, s2, N, pitch, eb,
                       1.0 / ((double)N * (double)N));
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

}  // namespace

extern "C" {

int64_t bfgx_fft2_work_doubles(int32_t n)
{
    if (!fourier_grid_ok(n, kFft2MaxN)) return 0;
    return 6 * (int64_t)n * fft_pitch(n);
}

int bfgx_rfft2_device(int device, void *hip_stream, int32_t n, const double *map_dev, double *work_dev, double *spec_out_dev)
{
    if (!map_dev || !work_dev || !spec_out_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = fft2_check_n(n)) return rc;
    if (int rc = fourier_check_aligned(work_dev, "work_dev")) return rc;
    if (int rc = fourier_check_aligned(spec_out_dev, "spec_out_dev")) return rc;
    if (int rc = select_device(device)) return rc;
    Fft2Setup *f = nullptr;
    if (int rc = fft2_setup(device, n, &f)) return rc;
    return fft2_forward(*f, (hipStream_t)hip_stream, n, map_dev, (double2 *)spec_out_dev, Fft2Work(work_dev, n).u);
}

int bfgx_irfft2_device(int device, void *hip_stream, int32_t n, const double *spec_dev, double scale, double *work_dev, double *map_out_dev)
{
    if (!spec_dev || !work_dev || !map_out_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = fft2_check_n(n)) return rc;
    if (int rc = fourier_check_aligned(work_dev, "work_dev")) return rc;
    if (int rc = fourier_check_aligned(spec_dev, "spec_dev")) return rc;
    if (!std::isfinite(scale)) return fail(BFGX_ERR_INVALID, "irfft2 needs a finite scale");
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    Fft2Setup *f = nullptr;
    if (int rc = fft2_setup(device, n, &f)) return rc;
    const Fft2Work w(work_dev, n);
    if (int rc = fft2_filter(*f, s, n, (const double2 *)spec_dev, w.s1, kFft2Unit, 1.0, 0.0, nullptr, nullptr, 0, scale)) return rc;
    return fft2_inverse_conj(*f, s, n, w.s1, w.u, map_out_dev);
}

int bfgx_power_spectrum_2d_device(int device, void *hip_stream, int32_t n, const double *map_a_dev, const double *map_b_dev, double L, int32_t nk,
                                  int32_t window_order, double *work_dev, double *paa_sum_dev, double *pbb_sum_dev, double *pab_sum_dev,
                                  double *k_sum_dev, unsigned long long *counts_dev)
{
    if (!map_a_dev || !map_b_dev || !work_dev || !paa_sum_dev || !pbb_sum_dev || !pab_sum_dev || !k_sum_dev || !counts_dev)
        return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = fft2_check_n(n)) return rc;
    if (int rc = fft2_check_bins(L, nk, window_order)) return rc;
    if (int rc = fourier_check_aligned(work_dev, "work_dev")) return rc;
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    Fft2Setup *f = nullptr;
    const double *win = nullptr;
    if (int rc = fft2_setup(device, n, &f)) return rc;
    if (int rc = xpk_window(device, n, window_order, &win)) return rc;
    const int N = n, pitch = fft_pitch(N);
    const Fft2Work w(work_dev, N);
    const bool same = map_a_dev == map_b_dev;
    if (int rc = fft2_forward(*f, s, N, map_a_dev, w.s1, w.u)) return rc;
    if (!same) if (int rc = fft2_forward(*f, s, N, map_b_dev, w.s2, w.u)) return rc;
    if (int rc = zero_bin_sums(s, nk, counts_dev, {paa_sum_dev, pbb_sum_dev, pab_sum_dev, k_sum_dev})) return rc;
    const KAxis ka = k_axis_bins(N, L, nk);                  // (FftSetup's k axis and bins: klin[i] = n_i val is built in LDS)
    const Fft2Bins fb{ka.val, ka.k_lo, ka.dk, 1.0 / ka.dk, nk, paa_sum_dev, pbb_sum_dev, pab_sum_dev, k_sum_dev, counts_dev};
    // persistent workgroups over the rows, each flushing its histograms once
    const unsigned wgs = (unsigned)std::min<int64_t>(N, (int64_t)f->n_cu * (nk <= 256 ? 4 : 1));
    hipLaunchKernelGGL(fft2_bin_kernel, dim3(wgs), dim3(kFft2Threads), fft2_bin_lds_bytes(N, nk), s, (const double2 *)w.s1,
                       (const double2 *)(same ? w.s1 : w.s2), N, pitch, fb, win);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

int bfgx_filter_map_2d_device(int device, void *hip_stream, int32_t n, const double *map_dev, double L, int32_t kind, double param,
                              const double *table_k_host, const double *table_b_host, int32_t ntable, double *work_dev, double *map_out_dev)
{
    if (!map_dev || !work_dev || !map_out_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = fft2_check_n(n)) return rc;
    if (int rc = fft2_check_filter(n, L, kind, param, table_k_host, table_b_host, ntable)) return rc;
    if (int rc = fourier_check_aligned(work_dev, "work_dev")) return rc;
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    Fft2Setup *f = nullptr;
    if (int rc = fft2_setup(device, n, &f)) return rc;
    const int N = n;
    const Fft2Work w(work_dev, N);
    const double *tk = nullptr, *tb = nullptr;
    if (kind == kFft2Table) {
        if (int rc = fft2_upload_beam(s, (double *)w.s2, table_k_host, table_b_host, ntable)) return rc;      // (in the second spectrum)
        tk = (const double *)w.s2; tb = tk + ntable;
    }
    if (int rc = fft2_forward(*f, s, N, map_dev, w.s1, w.u)) return rc;
    if (int rc = fft2_filter(*f, s, N, w.s1, w.s1, kind, L, param, tk, tb, ntable, 1.0 / ((double)N * (double)N))) return rc;
    return fft2_inverse_conj(*f, s, N, w.s1, w.u, map_out_dev);
}

// The work array of the derivatives: nder products [n][pitch], then u, the other side of the out-of-place column pass.  The beam table
// rides in u: it is copied there before fft2_der_kernel, read by that kernel alone, and u is first written by the column passes after it.
int64_t bfgx_derivatives_2d_work_doubles(int32_t n, int32_t nder)
{
    if (!fourier_grid_ok(n, kFft2MaxN) || (nder != 1 && nder != 6)) return 0;
    return 2 * (int64_t)n * fft_pitch(n) * (nder + 1);
}

int bfgx_derivatives_2d_device(int device, void *hip_stream, int32_t n, const double *spec_dev, double L, int32_t kind, double param,
                               const double *table_k_host, const double *table_b_host, int32_t ntable, int32_t nder, int32_t spin_form,
                               double *work_dev, double *ders_out_dev)
{
    if (!spec_dev || !work_dev || !ders_out_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = fft2_check_n(n)) return rc;
    if (kind < kFft2Gauss || kind > kFft2Unit) return fail(BFGX_ERR_INVALID, "2-D derivatives kind %d: 0 (Gaussian), 1 (top hat), 2 (table) or 3 (no filter)", kind);
    if (kind == kFft2Unit) { if (!(L > 0)) return fail(BFGX_ERR_INVALID, "2-D filter needs L > 0"); }
    else if (int rc = fft2_check_filter(n, L, kind, param, table_k_host, table_b_host, ntable)) return rc;
    if (nder != 1 && nder != 6) return fail(BFGX_ERR_INVALID, "2-D derivatives: nder must be 1 or 6 (got %d)", nder);
    if (int rc = fourier_check_aligned(work_dev, "work_dev")) return rc;
    if (int rc = fourier_check_aligned(spec_dev, "spec_dev")) return rc;
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    Fft2Setup *f = nullptr;
    if (int rc = fft2_setup(device, n, &f)) return rc;
    const int N = n, pitch = fft_pitch(N);
    const int64_t half = (int64_t)N * pitch;
    double2 *prod = (double2 *)work_dev, *u = prod + (int64_t)nder * half;
    const double *tk = nullptr, *tb = nullptr;
    if (kind == kFft2Table) {
        if (int rc = fft2_upload_beam(s, (double *)u, table_k_host, table_b_host, ntable)) return rc;
        tk = (const double *)u; tb = tk + ntable;
    }
    hipLaunchKernelGGL(fft2_der_kernel, dim3(stream_grid(f->n_cu, half)), dim3(kFft2Threads), 0, s, (const double2 *)spec_dev, prod, N, pitch,
                       (int)kind, 2 * 3.141592653589793 / L, param, tk, tb, (int)ntable, 1.0 / ((double)N * (double)N), (int)nder, (int)spin_form);
    HIP_TRY(hipGetLastError());
    for (int d = 0; d < nder; ++d)
        if (int rc = fft2_inverse_conj(*f, s, N, prod + d * half, u, ders_out_dev + (int64_t)d * N * N)) return rc;
    return BFGX_OK;
}

int bfgx_kappa_to_shear_2d_device(int device, void *hip_stream, int32_t n, const double *kappa_dev, double *work_dev, double *g1_out_dev,
                                  double *g2_out_dev)
{
    if (!kappa_dev || !work_dev || !g1_out_dev || !g2_out_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = fft2_check_n(n)) return rc;
    if (int rc = fourier_check_aligned(work_dev, "work_dev")) return rc;
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    Fft2Setup *f = nullptr;
    if (int rc = fft2_setup(device, n, &f)) return rc;
    const Fft2Work w(work_dev, n);
    if (int rc = fft2_forward(*f, s, n, kappa_dev, w.s1, w.u)) return rc;
    if (int rc = fft2_ks(*f, s, n, w.s1, w.s2, 0)) return rc;
    if (int rc = fft2_inverse_conj(*f, s, n, w.s1, w.u, g1_out_dev)) return rc;
    return fft2_inverse_conj(*f, s, n, w.s2, w.u, g2_out_dev);
}

int bfgx_shear_to_kappa_2d_device(int device, void *hip_stream, int32_t n, const double *g1_dev, const double *g2_dev, double *work_dev,
                                  double *kappa_e_out_dev, double *kappa_b_out_dev)
{
    if (!g1_dev || !g2_dev || !work_dev || !kappa_e_out_dev || !kappa_b_out_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = fft2_check_n(n)) return rc;
    if (int rc = fourier_check_aligned(work_dev, "work_dev")) return rc;
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    Fft2Setup *f = nullptr;
    if (int rc = fft2_setup(device, n, &f)) return rc;
    const Fft2Work w(work_dev, n);
    if (int rc = fft2_forward(*f, s, n, g1_dev, w.s1, w.u)) return rc;
    if (int rc = fft2_forward(*f, s, n, g2_dev, w.s2, w.u)) return rc;
    if (int rc = fft2_ks(*f, s, n, w.s1, w.s2, 1)) return rc;
    if (int rc = fft2_inverse_conj(*f, s, n, w.s1, w.u, kappa_e_out_dev)) return rc;
    return fft2_inverse_conj(*f, s, n, w.s2, w.u, kappa_b_out_dev);
}

int bfgx_power_spectrum_2d(int device, int32_t n, const double *map_a, const double *map_b, double L, int32_t nk, int32_t window_order, double *paa,
                           double *pbb, double *pab, double *kcen, int64_t *counts)
{
    if (!map_a || !map_b || !paa || !pbb || !pab || !kcen || !counts) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = fft2_check_n(n)) return rc;
    if (int rc = fft2_check_bins(L, nk, window_order)) return rc;
    HostCall c(device);
    const size_t N = n;
    std::vector<double> h(4 * (size_t)nk);                   // the bins' sums (aa, bb, ab, |k|)
    std::vector<unsigned long long> hc(nk);
    const double *da = c.in(map_a, N * N), *db = (map_b == map_a) ? da : c.in(map_b, N * N);
    double *dw = c.scratch<double>((size_t)bfgx_fft2_work_doubles(n));
    double *ds = c.out(h.data(), 4 * (size_t)nk);
    unsigned long long *dc = c.out(hc.data(), nk);
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_power_spectrum_2d_device(device, nullptr, n, da, db, L, nk, window_order, dw, ds, ds + nk, ds + 2 * nk, ds + 3 * nk, dc)) return rc;
    if (int rc = c.finish()) return rc;
    bin_means(nk, h, hc, counts, {paa, pbb, pab, kcen});
    return BFGX_OK;
}

int bfgx_filter_map_2d(int device, int32_t n, const double *map, double L, int32_t kind, double param, const double *table_k, const double *table_b,
                       int32_t ntable, double *map_out)
{
    if (!map || !map_out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = fft2_check_n(n)) return rc;
    if (int rc = fft2_check_filter(n, L, kind, param, table_k, table_b, ntable)) return rc;
    HostCall c(device);
    const size_t N = n;
    const double *dm = c.in(map, N * N);
    double *dw = c.scratch<double>((size_t)bfgx_fft2_work_doubles(n)), *dout = c.out(map_out, N * N);
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_filter_map_2d_device(device, nullptr, n, dm, L, kind, param, table_k, table_b, ntable, dw, dout)) return rc;
    return c.finish();
}

int bfgx_kappa_to_shear_2d(int device, int32_t n, const double *kappa, double *g1, double *g2)
{
    if (!kappa || !g1 || !g2) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = fft2_check_n(n)) return rc;
    HostCall c(device);
    const size_t N = n;
    const double *dk = c.in(kappa, N * N);
    double *dw = c.scratch<double>((size_t)bfgx_fft2_work_doubles(n)), *d1 = c.out(g1, N * N), *d2 = c.out(g2, N * N);
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_kappa_to_shear_2d_device(device, nullptr, n, dk, dw, d1, d2)) return rc;
    return c.finish();
}

int bfgx_shear_to_kappa_2d(int device, int32_t n, const double *g1, const double *g2, double *kappa_e, double *kappa_b)
{
    if (!g1 || !g2 || !kappa_e || !kappa_b) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = fft2_check_n(n)) return rc;
    HostCall c(device);
    const size_t N = n;
    const double *d1 = c.in(g1, N * N), *d2 = c.in(g2, N * N);
    double *dw = c.scratch<double>((size_t)bfgx_fft2_work_doubles(n)), *de = c.out(kappa_e, N * N), *db = c.out(kappa_b, N * N);
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_shear_to_kappa_2d_device(device, nullptr, n, d1, d2, dw, de, db)) return rc;
    return c.finish();
}

}  // extern "C"
