// bfgx_fft_api.inc -- C ABI of the power spectrum of gridded 3-D maps and of the forward slab transforms (include/bfgx.h, "power
// spectrum"); included by bfgx_api.hip after bfgx_fourier_host.inc, on which alone it builds (FftSetup, fft_planes, fft_bin_table).
// Kernels: bfgx_fft.hpp.

namespace {

// complex transforms along the FIRST axis of F [N][nb][pitch] (the columns b0 .. b0 + nb of the middle axis) fused with the P(k)
// sums: the transformed tiles are binned from LDS and never written back (F is scratch afterwards)
int fft_axis0_pk(FftSetup &f, hipStream_t s, int N, int nb, int b0, double2 *F, int pitch, double *pk_sum_dev, double *k_sum_dev,
                 unsigned long long *counts_dev)
{
    if (int rc = zero_bin_sums(s, f.nk, counts_dev, {pk_sum_dev, k_sum_dev})) return rc;
    // axis 0: element (i, b, c) at (i * nb + b) * pitch + c.  A fixed number of workgroups strides over the tiles, each flushing
    // its histogram once (3 nk global atomics per workgroup, not per tile)
    const unsigned wgs = persistent_wgs(f.n_cu, (int64_t)f.sh.ztiles * nb, f.bin_lds(2));
    PkBins pb = f.bins(b0, pitch, pk_sum_dev, k_sum_dev, counts_dev);
    const bool use_tab = f.nk <= kPkMaxTableNk;
    if (use_tab) {
        if (int rc = fft_bin_table(f, s, pb)) return rc;
        pb.tab = f.dtab.as<uint8_t>();
    }
    if (int rc = use_tab ? strided_launch<2>(f.sh, s, wgs, f.bin_lds(2), F, N, f.lg, f.tw(), (int64_t)nb * pitch, (int64_t)pitch, nb, pb)
                         : strided_launch<1>(f.sh, s, wgs, f.bin_lds(1), F, N, f.lg, f.tw(), (int64_t)nb * pitch, (int64_t)pitch, nb, pb))
        return rc;
    if (use_tab) return fft_table_sums(f, s, b0, nb, k_sum_dev, counts_dev);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

}  // namespace

extern "C" {

int32_t bfgx_fft_pitch(int32_t n_grid) { return fft_pitch(n_grid); }

int64_t bfgx_power_spectrum_work_doubles(int32_t n_grid)
{
    return 2 * (int64_t)n_grid * n_grid * fft_pitch(n_grid);
}

int bfgx_power_spectrum_device(int device, void *hip_stream, int32_t n_grid, const double *map_dev, double L, int32_t nk,
                               double *work_dev, double *pk_sum_dev, double *k_sum_dev, unsigned long long *counts_dev)
{
    if (!map_dev || !work_dev || !pk_sum_dev || !k_sum_dev || !counts_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = fourier_check_grid(n_grid, kFft3MaxN, kPkGridMsg)) return rc;
    if (nk < 1 || nk > kPkMaxNk || !(L > 0)) return fail(BFGX_ERR_INVALID, "power spectrum needs 1 <= nk <= 2048, L > 0");
    if (int rc = fourier_check_aligned(work_dev, "work_dev")) return rc;
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    FftSetup *f = nullptr;
    if (int rc = fft_setup(device, n_grid, L, nk, &f)) return rc;
    const int pitch = fft_pitch(n_grid);
    if (int rc = fft_planes(*f, s, n_grid, n_grid, map_dev, (double2 *)work_dev, pitch)) return rc;
    return fft_axis0_pk(*f, s, n_grid, n_grid, 0, (double2 *)work_dev, pitch, pk_sum_dev, k_sum_dev, counts_dev);
}

int bfgx_fft_slab_planes_device(int device, void *hip_stream, int32_t n_grid, int32_t planes, const double *map_dev, double *work_dev)
{
    if (!map_dev || !work_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = fourier_check_grid(n_grid, kFft3MaxN, kPkGridMsg)) return rc;
    if (planes < 1 || planes > n_grid || ((int64_t)planes * n_grid) % 2) return fail(BFGX_ERR_INVALID, "slab of %d planes", planes);
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    FftSetup *f = nullptr;
    if (int rc = fft_setup(device, n_grid, 1.0, 1, &f)) return rc;
    return fft_planes(*f, s, n_grid, planes, map_dev, (double2 *)work_dev, fft_pitch(n_grid));
}

int bfgx_fft_slab_axis0_pk_device(int device, void *hip_stream, int32_t n_grid, int32_t ncols, int32_t col0, double *work_dev, double L,
                                  int32_t nk, double *pk_sum_dev, double *k_sum_dev, unsigned long long *counts_dev)
{
    if (!work_dev || !pk_sum_dev || !k_sum_dev || !counts_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = fourier_check_grid(n_grid, kFft3MaxN, kPkGridMsg)) return rc;
    if (nk < 1 || nk > kPkMaxNk || !(L > 0)) return fail(BFGX_ERR_INVALID, "power spectrum needs 1 <= nk <= 2048, L > 0");
    if (ncols < 1 || col0 < 0 || col0 + ncols > n_grid) return fail(BFGX_ERR_INVALID, "columns [%d, %d) outside the grid", col0, col0 + ncols);
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    FftSetup *f = nullptr;
    if (int rc = fft_setup(device, n_grid, L, nk, &f)) return rc;
    return fft_axis0_pk(*f, s, n_grid, ncols, col0, (double2 *)work_dev, fft_pitch(n_grid), pk_sum_dev, k_sum_dev, counts_dev);
}

int bfgx_power_spectrum(int device, int32_t n_grid, const double *map, double L, int32_t nk, double *pk, double *kcen, int64_t *counts)
{
    if (!map || !pk || !kcen || !counts) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = fourier_check_grid(n_grid, kFft3MaxN, kPkGridMsg)) return rc;
    if (nk < 1 || nk > kPkMaxNk) return fail(BFGX_ERR_INVALID, "power spectrum needs 1 <= nk <= 2048");
    HostCall c(device);
    const size_t N = n_grid;
    std::vector<double> h(2 * (size_t)nk);                   // the bins' sums (|F|^2, |k|)
    std::vector<unsigned long long> hc(nk);
    const double *dm = c.in(map, N * N * N);
    double *dw = c.scratch<double>(bfgx_power_spectrum_work_doubles(n_grid)), *ds = c.out(h.data(), 2 * (size_t)nk);
    unsigned long long *dc = c.out(hc.data(), nk);
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_power_spectrum_device(device, nullptr, n_grid, dm, L, nk, dw, ds, ds + nk, dc)) return rc;
    if (int rc = c.finish()) return rc;
    bin_means(nk, h, hc, counts, {pk, kcen});
    return BFGX_OK;
}

}  // extern "C"
