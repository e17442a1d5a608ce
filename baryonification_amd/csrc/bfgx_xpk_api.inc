// C ABI of the cross power spectrum of two gridded 3-D maps (include/bfgx.h, "cross power spectrum"); included by bfgx_api.hip after
// bfgx_bispec_api.inc (FftSetup, fft_setup, fft_planes, fft_bin_table, fft_pitch; fft_axis0_store).  Kernel: the cross modes of the last
// strided pass, BIN 3 and 4 of fft_c2c_strided_kernel in bfgx_fft.hpp.

namespace {

// window weights t[i] = s(n_i)^(-2p), s(n) = sin(pi n / N) / (pi n / N), n = fftfreq(N) N, per (device, n_grid, p): built in long double
// like the twiddles, uploaded by the first call that wants them, kept until bfgx_cache_clear.  p = 0 is a table of ones.
std::mutex g_xpk_mu;
std::map<std::tuple<int, int, int>, DevBuf *> g_xpk_win;

int xpk_window(int device, int N, int p, const double **out)
{
    std::lock_guard<std::mutex> lk(g_xpk_mu);
    const auto key = std::make_tuple(device, N, p);
    auto it = g_xpk_win.find(key);
    if (it == g_xpk_win.end()) {
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
        DevBuf *b = new DevBuf();
        if (b->up(t.data(), sizeof(double) * N)) { delete b; return alloc_fail("window table"); }
        it = g_xpk_win.emplace(key, b).first;
    }
    *out = it->second->as<double>();
    return BFGX_OK;
}

void xpk_release_all()
{
    std::lock_guard<std::mutex> lk(g_xpk_mu);
    for (auto &kv : g_xpk_win) { (void)hipSetDevice(std::get<0>(kv.first)); delete kv.second; }
    g_xpk_win.clear();
}

// ---- argument checks, stated once (no device call); the host and the _device entries give the same messages
int xpk_check_shape(int n_grid, double L, int nk, int window_order)
{
    if (n_grid > 1024 || ilog2_exact(n_grid) < 3) return fail(BFGX_ERR_UNSUPPORTED, "cross power spectrum needs n_grid = 2^m with 8 <= n_grid <= 1024");
    if (nk < 1 || nk > 2048) return fail(BFGX_ERR_INVALID, "cross power spectrum needs 1 <= nk <= 2048");
    if (!(L > 0)) return fail(BFGX_ERR_INVALID, "cross power spectrum needs L > 0");
    if (window_order < 0 || window_order > 3) return fail(BFGX_ERR_INVALID, "window_order %d: 0 (none), 1 (NGP), 2 (CIC) or 3 (TSC)", window_order);
    return BFGX_OK;
}

int xpk_check_aligned(const void *p, const char *what)
{
    if (reinterpret_cast<uintptr_t>(p) & 15) return fail(BFGX_ERR_INVALID, "%s must be 16-byte aligned (complex values)", what);
    return BFGX_OK;
}

// complex transforms along the FIRST axis of work_b [N][nb][pitch] (the columns b0 .. b0 + nb of the middle axis) fused with the three
// sums of a cross spectrum against spec_a, map A's finished spectrum of the same columns: nothing is written back, work_b is kept as it
// was.  Bins, counts and |k| sums as in fft_axis0_pk.
int fft_axis0_xpk(FftSetup &f, hipStream_t s, int N, int nb, int b0, const double2 *spec_a, double2 *work_b, int pitch, int nk, const double *win,
                  double *paa_sum_dev, double *pbb_sum_dev, double *pab_sum_dev, double *k_sum_dev, unsigned long long *counts_dev)
{
    HIP_TRY(hipMemsetAsync(paa_sum_dev, 0, sizeof(double) * nk, s));
    HIP_TRY(hipMemsetAsync(pbb_sum_dev, 0, sizeof(double) * nk, s));
    HIP_TRY(hipMemsetAsync(pab_sum_dev, 0, sizeof(double) * nk, s));
    HIP_TRY(hipMemsetAsync(k_sum_dev, 0, sizeof(double) * nk, s));
    HIP_TRY(hipMemsetAsync(counts_dev, 0, sizeof(unsigned long long) * nk, s));
    const int64_t ntiles = (int64_t)f.ztiles * nb;
    PkBins pb{f.dkl.as<double>(), f.k_lo, f.dk, 1.0 / f.dk, nk, b0, paa_sum_dev, k_sum_dev, counts_dev, nullptr, pitch};
    const XpkArgs xa{spec_a, win, pbb_sum_dev, pab_sum_dev};
    const bool use_tab = nk <= 254;
    const size_t lds = use_tab ? f.lds_bin3 : f.lds_bin4;
    // persistent workgroups, as many as LDS lets the CUs hold, each flushing its histograms once
    const unsigned wgs = (unsigned)std::min<int64_t>(ntiles, (int64_t)f.n_cu * std::max<size_t>(1, (size_t)(160 * 1024) / lds));
    if (use_tab) {
        if (int rc = fft_bin_table(f, s, N, nk, pb)) return rc;
        pb.tab = f.dtab.as<uint8_t>();
        if (int rc = f.xpk_launch<3>(s, wgs, lds, work_b, N, (int64_t)nb * pitch, (int64_t)pitch, nb, pb, xa)) return rc;
        hipLaunchKernelGGL(pk_table_sums_kernel, dim3((unsigned)nk), dim3(256), 0, s, nk, b0, nb, f.dksb.as<double>(),
                           f.dcnb.as<unsigned long long>(), k_sum_dev, counts_dev);
        HIP_TRY(hipGetLastError());
        return BFGX_OK;
    }
    if (int rc = f.xpk_launch<4>(s, wgs, lds, work_b, N, (int64_t)nb * pitch, (int64_t)pitch, nb, pb, xa)) return rc;
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
    if (int rc = xpk_check_aligned(spec_a_dev, "spec_a_dev")) return rc;
    if (int rc = xpk_check_aligned(work_b_dev, "work_b_dev")) return rc;
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
    return fft_axis0_xpk(*f, s, n_grid, ncols, col0, (const double2 *)spec_a_dev, (double2 *)work_b_dev, pitch, nk, win, paa_sum_dev, pbb_sum_dev,
                         pab_sum_dev, k_sum_dev, counts_dev);
}

int bfgx_cross_power_spectrum_device(int device, void *hip_stream, int32_t n_grid, const double *map_a_dev, const double *map_b_dev, double L, int32_t nk,
                                     int32_t window_order, double *work_dev, double *paa_sum_dev, double *pbb_sum_dev, double *pab_sum_dev,
                                     double *k_sum_dev, unsigned long long *counts_dev)
{
    if (!map_a_dev || !map_b_dev || !work_dev || !paa_sum_dev || !pbb_sum_dev || !pab_sum_dev || !k_sum_dev || !counts_dev)
        return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = xpk_check_shape(n_grid, L, nk, window_order)) return rc;
    if (int rc = xpk_check_aligned(work_dev, "work_dev")) return rc;
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
    return fft_axis0_xpk(*f, s, N, N, 0, spec_a, work_b, pitch, nk, win, paa_sum_dev, pbb_sum_dev, pab_sum_dev, k_sum_dev, counts_dev);
}

int bfgx_cross_power_spectrum(int device, int32_t n_grid, const double *map_a, const double *map_b, double L, int32_t nk, int32_t window_order,
                              double *paa, double *pbb, double *pab, double *kcen, int64_t *counts)
{
    if (!map_a || !map_b || !paa || !pbb || !pab || !kcen || !counts) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = xpk_check_shape(n_grid, L, nk, window_order)) return rc;
    HostCall c(device);
    const size_t N = n_grid;
    std::vector<double> h(4 * (size_t)nk);                   // the bins' sums (aa, bb, ab, |k|), divided by their counts below
    std::vector<unsigned long long> hc(nk);
    const double *da = c.in(map_a, N * N * N), *db = (map_b == map_a) ? da : c.in(map_b, N * N * N);
    double *dw = c.scratch<double>((size_t)bfgx_cross_power_spectrum_work_doubles(n_grid));
    double *ds = c.out(h.data(), 4 * (size_t)nk);
    unsigned long long *dc = c.out(hc.data(), nk);
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_cross_power_spectrum_device(device, nullptr, n_grid, da, db, L, nk, window_order, dw, ds, ds + nk, ds + 2 * nk, ds + 3 * nk, dc)) return rc;
    if (int rc = c.finish()) return rc;
    for (int i = 0; i < nk; ++i) {
        const double n = (double)hc[i];                      // 0 / 0 -> NaN for empty bins, as in bfgx_power_spectrum
        counts[i] = (int64_t)hc[i];
        paa[i] = h[i] / n;
        pbb[i] = h[nk + i] / n;
        pab[i] = h[2 * (size_t)nk + i] / n;
        kcen[i] = h[3 * (size_t)nk + i] / n;
    }
    return BFGX_OK;
}

}  // extern "C"
