// C ABI of the cross power spectrum of two gridded 3-D maps (include/bfgx.h, "cross power spectrum"); included by bfgx_api.hip after
// bfgx_fourier_host.inc, on which alone it builds (FftSetup, the transform passes, fft_bin_table, the table cache); bfgx_interlace_api.inc
// and bfgx_fft2d_api.inc take the window table and the cross pass from here.  Kernel: the cross modes of the last strided pass, BIN 3 and
// 4 of fft_c2c_strided_kernel in bfgx_fft.hpp.

namespace {

// window weights t[i] = s(n_i)^(-2p), s(n) = sin(pi n / N) / (pi n / N), n = fftfreq(N) N, per (device, n_grid, p): built in long double
// like the twiddles.  p = 0 is a table of ones.
FourierCache<DevBuf, int, int> g_xpk_win;

int xpk_window(int device, int N, int p, const double **out)
{
    DevBuf *b = nullptr;
    const int rc = g_xpk_win.get(std::make_tuple(device, N, p), &b, [&](DevBuf &buf) {
        std::vector<double> t(N);
        const long double pi = 3.141592653589793238462643383279502884L;
        for (int i = 0; i < N; ++i) {
            const int n = i < (N + 1) / 2 ? i : i - N;
            const long double x = pi * (long double)n / (long double)N;
            const long double sn = n ? sinl(x) / x : 1.0L;
            long double sp = 1.0L;
            for (int j = 0; j < 2 * p; ++j) sp *= sn;
            t[i] = (double)(1.0L / sp);
        }
        return buf.up(t.data(), sizeof(double) * N) ? alloc_fail("window table") : BFGX_OK;
    });
    if (rc == BFGX_OK) *out = b->as<double>();
    return rc;
}

// ---- argument checks, stated once (no device call); the host and the _device entries give the same messages
int xpk_check_shape(int n_grid, double L, int nk, int window_order)
{
    if (int rc = fourier_check_grid(n_grid, kFft3MaxN, "cross power spectrum needs n_grid = 2^m with 8 <= n_grid <= 1024")) return rc;
    if (nk < 1 || nk > kPkMaxNk) return fail(BFGX_ERR_INVALID, "cross power spectrum needs 1 <= nk <= 2048");
    if (!(L > 0)) return fail(BFGX_ERR_INVALID, "cross power spectrum needs L > 0");
    if (window_order < 0 || window_order > 3) return fail(BFGX_ERR_INVALID, "window_order %d: 0 (none), 1 (NGP), 2 (CIC) or 3 (TSC)", window_order);
    return BFGX_OK;
}

// complex transforms along the FIRST axis of work_b [N][nb][pitch] (the columns b0 .. b0 + nb of the middle axis) fused with the three
// sums of a cross spectrum against spec_a, map A's finished spectrum of the same columns: nothing is written back, work_b is kept as it
// was.  Bins, counts and |k| sums as in fft_axis0_pk.
int fft_axis0_xpk(FftSetup &f, hipStream_t s, int N, int nb, int b0, const double2 *spec_a, double2 *work_b, int pitch, const double *win,
                  double *paa_sum_dev, double *pbb_sum_dev, double *pab_sum_dev, double *k_sum_dev, unsigned long long *counts_dev)
{
    if (int rc = zero_bin_sums(s, f.nk, counts_dev, {paa_sum_dev, pbb_sum_dev, pab_sum_dev, k_sum_dev})) return rc;
    PkBins pb = f.bins(b0, pitch, paa_sum_dev, k_sum_dev, counts_dev);
    const XpkArgs xa{spec_a, win, pbb_sum_dev, pab_sum_dev};
    const bool use_tab = f.nk <= kPkMaxTableNk;
    const size_t lds = f.bin_lds(use_tab ? 3 : 4);
    // persistent workgroups, as many as LDS lets the CUs hold, each flushing its histograms once
    const unsigned wgs = persistent_wgs(f.n_cu, (int64_t)f.sh.ztiles * nb, lds);
    if (use_tab) {
        if (int rc = fft_bin_table(f, s, pb)) return rc;
        pb.tab = f.dtab.as<uint8_t>();
    }
    if (int rc = use_tab ? strided_launch<3>(f.sh, s, wgs, lds, work_b, N, f.lg, f.tw(), (int64_t)nb * pitch, (int64_t)pitch, nb, pb, xa)
                         : strided_launch<4>(f.sh, s, wgs, lds, work_b, N, f.lg, f.tw(), (int64_t)nb * pitch, (int64_t)pitch, nb, pb, xa))
        return rc;
    if (use_tab) return fft_table_sums(f, s, b0, nb, k_sum_dev, counts_dev);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

}  // namespace

extern "C" {

int64_t bfgx_cross_power_spectrum_work_doubles(int32_t n_grid) { return 2 * bfgx_power_spectrum_work_doubles(n_grid); }

int bfgx_fft_slab_axis0_xpk_device(int device, void *hip_stream, int32_t n_grid, int32_t ncols, int32_t col0, const double *spec_a_dev, double *work_b_dev,
                                   double L, int32_t nk, int32_t window_order, double *paa_sum_dev, double *pbb_sum_dev, double *pab_sum_dev,
                                   double *k_sum_dev, unsigned long long *counts_dev)
{
    if (!spec_a_dev || !work_b_dev || !paa_sum_dev || !pbb_sum_dev || !pab_sum_dev || !k_sum_dev || !counts_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = xpk_check_shape(n_grid, L, nk, window_order)) return rc;
    if (int rc = fourier_check_aligned(spec_a_dev, "spec_a_dev")) return rc;
    if (int rc = fourier_check_aligned(work_b_dev, "work_b_dev")) return rc;
    if (ncols < 1 || col0 < 0 || col0 > n_grid - ncols) return fail(BFGX_ERR_INVALID, "columns [%d, %lld) outside the grid", col0, (long long)col0 + ncols);
    const int pitch = fft_pitch(n_grid);
    {
        const uintptr_t bytes = sizeof(double2) * (uintptr_t)n_grid * ncols * pitch, a = (uintptr_t)spec_a_dev, b = (uintptr_t)work_b_dev;
        if (a < b + bytes && b < a + bytes) return fail(BFGX_ERR_INVALID, "spec_a_dev and work_b_dev overlap");
    }
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    FftSetup *f = nullptr;
    const double *win = nullptr;
    if (int rc = fft_setup(device, n_grid, L, nk, &f)) return rc;
    if (int rc = xpk_window(device, n_grid, window_order, &win)) return rc;
    return fft_axis0_xpk(*f, s, n_grid, ncols, col0, (const double2 *)spec_a_dev, (double2 *)work_b_dev, pitch, win, paa_sum_dev, pbb_sum_dev,
                         pab_sum_dev, k_sum_dev, counts_dev);
}

int bfgx_cross_power_spectrum_device(int device, void *hip_stream, int32_t n_grid, const double *map_a_dev, const double *map_b_dev, double L, int32_t nk,
                                     int32_t window_order, double *work_dev, double *paa_sum_dev, double *pbb_sum_dev, double *pab_sum_dev,
                                     double *k_sum_dev, unsigned long long *counts_dev)
{
    if (!map_a_dev || !map_b_dev || !work_dev || !paa_sum_dev || !pbb_sum_dev || !pab_sum_dev || !k_sum_dev || !counts_dev)
        return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = xpk_check_shape(n_grid, L, nk, window_order)) return rc;
    if (int rc = fourier_check_aligned(work_dev, "work_dev")) return rc;
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    FftSetup *f = nullptr;
    const double *win = nullptr;
    if (int rc = fft_setup(device, n_grid, L, nk, &f)) return rc;
    if (int rc = xpk_window(device, n_grid, window_order, &win)) return rc;
    const int N = n_grid, pitch = fft_pitch(N);
    double2 *spec_a = (double2 *)work_dev, *work_b = spec_a + (int64_t)N * N * pitch;
    // A: all three axes, the spectrum kept; B: the plane passes, then the last pass against A's spectrum
    if (int rc = fft_planes(*f, s, N, N, map_a_dev, spec_a, pitch)) return rc;
    if (int rc = fft_axis0_store(*f, s, N, N, spec_a, pitch)) return rc;
    if (int rc = fft_planes(*f, s, N, N, map_b_dev, work_b, pitch)) return rc;
    return fft_axis0_xpk(*f, s, N, N, 0, spec_a, work_b, pitch, win, paa_sum_dev, pbb_sum_dev, pab_sum_dev, k_sum_dev, counts_dev);
}

int bfgx_cross_power_spectrum(int device, int32_t n_grid, const double *map_a, const double *map_b, double L, int32_t nk, int32_t window_order,
                              double *paa, double *pbb, double *pab, double *kcen, int64_t *counts)
{
    if (!map_a || !map_b || !paa || !pbb || !pab || !kcen || !counts) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = xpk_check_shape(n_grid, L, nk, window_order)) return rc;
    HostCall c(device);
    const size_t N = n_grid;
    std::vector<double> h(4 * (size_t)nk);                   // the bins' sums (aa, bb, ab, |k|)
    std::vector<unsigned long long> hc(nk);
    const double *da = c.in(map_a, N * N * N), *db = (map_b == map_a) ? da : c.in(map_b, N * N * N);
    double *dw = c.scratch<double>((size_t)bfgx_cross_power_spectrum_work_doubles(n_grid));
    double *ds = c.out(h.data(), 4 * (size_t)nk);
    unsigned long long *dc = c.out(hc.data(), nk);
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_cross_power_spectrum_device(device, nullptr, n_grid, da, db, L, nk, window_order, dw, ds, ds + nk, ds + 2 * nk, ds + 3 * nk, dc)) return rc;
    if (int rc = c.finish()) return rc;
    bin_means(nk, h, hc, counts, {paa, pbb, pab, kcen});
    return BFGX_OK;
}

}  // extern "C"
