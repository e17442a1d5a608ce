// C ABI of the interlaced power spectrum of two grids displaced by half a cell, and of P(k) straight from particle columns
// (include/bfgx.h, "interlaced power spectrum"); included by bfgx_api.hip after bfgx_fourier_host.inc (FftSetup, the transform passes,
// the table cache), bfgx_xpk_api.inc (xpk_check_shape, xpk_window, fft_axis0_xpk) and bfgx_deposit_cloud_api.inc (deposit_cloud_impl).  Kernels: BIN 5 of fft_c2c_strided_kernel (the twisted store of grid
// 1) and interlace_combine_kernel in bfgx_fft.hpp; the shifted deposit in bfgx_deposit_cloud.hpp.
//
// With F1, F2 the transforms of the two grids, the combined coefficient is C = (F1 + Phi F2) / 2, Phi = phi[a] phi[b] phi[c], and
// |C|^2 = (|F1|^2 + |F2|^2 + 2 Re(F1 conj(Phi F2))) / 4.  Grid 1's last pass stores A' = 2 F1 conj(Phi); the cross pass of grid 2 against
// A' then sums |A'|^2 = 4 |F1|^2 into p1_sum, and |F2|^2 and Re(A' conj F2) = 2 Re(F1 conj(Phi F2)) both into p_sum; the combine kernel
// leaves p1_sum / 4 and (p1_sum / 4 + p_sum) / 4.  No scratch beyond the two half spectra, no bin kernel of its own.

namespace {

// The per-axis phase is phi[i] = exp(+i pi n_i / N), n = fftfreq(N) N, with phi[N/2] = 1 (either sign of i is as valid there; a real
// value keeps the combined field real, which the half spectrum's double count of the modes 0 < c < N/2 needs).  The kernel looks the
// product phi[a] phi[b] phi[c] up by the sum of the three wave numbers, the Nyquist index counted as 0 (twist_wave_number): the table is
// phase[j] = exp(+i pi j / N), j < 2N.  Per (device, n_grid), built in long double like the twiddles, kept until bfgx_cache_clear.
FourierCache<DevBuf, int> g_interlace_phi;

int interlace_phi(int device, int N, const double2 **out)
{
    DevBuf *b = nullptr;
    const int rc = g_interlace_phi.get(std::make_tuple(device, N), &b, [&](DevBuf &buf) {
        std::vector<double> t;
        unit_circle(t, 2 * N, 0, N, +1);                                                          // (|angle| <= pi)
        unit_circle(t, 2 * N, -N, N, +1);
        t[0] = 1.0; t[1] = 0.0; t[2 * N] = -1.0; t[2 * N + 1] = 0.0;                              // 1, -1, i and -i exactly
        t[N] = 0.0; t[N + 1] = 1.0; t[3 * N] = 0.0; t[3 * N + 1] = -1.0;
        return buf.up(t.data(), sizeof(double) * t.size()) ? alloc_fail("interlacing phase table") : BFGX_OK;
    });
    if (rc == BFGX_OK) *out = b->as<double2>();
    return rc;
}

// the two grids -> p_sum, p1_sum, k_sum, counts (arguments checked by the callers; the device is selected)
int interlaced_enqueue(int device, hipStream_t s, int N, const double *map1, const double *map2, double L, int nk, int window_order, double *work,
                       double *p_sum, double *p1_sum, double *k_sum, unsigned long long *counts)
{
    FftSetup *f = nullptr;
    const double *win = nullptr;
    const double2 *phi = nullptr;
    if (int rc = fft_setup(device, N, L, nk, &f)) return rc;
    if (int rc = xpk_window(device, N, window_order, &win)) return rc;
    if (int rc = interlace_phi(device, N, &phi)) return rc;
    const int pitch = fft_pitch(N);
    double2 *spec_a = (double2 *)work, *work_b = spec_a + (int64_t)N * N * pitch;
    if (int rc = fft_planes(*f, s, N, N, map1, spec_a, pitch)) return rc;
    if (int rc = fft_axis0_store<5>(*f, s, N, N, spec_a, pitch, TwistArgs{phi})) return rc;
    if (int rc = fft_planes(*f, s, N, N, map2, work_b, pitch)) return rc;
    if (int rc = fft_axis0_xpk(*f, s, N, N, 0, spec_a, work_b, pitch, win, p1_sum, p_sum, p_sum, k_sum, counts)) return rc;
    hipLaunchKernelGGL(interlace_combine_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, s, nk, p_sum, p1_sum);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

// one grid: the windowed auto spectrum through the cross pass of the map against itself.  p_sum is first where the two sums nobody
// wants land, then a copy of p1_sum.
int windowed_auto_enqueue(int device, hipStream_t s, int N, const double *map, double L, int nk, int window_order, double *work, double *p_sum,
                          double *p1_sum, double *k_sum, unsigned long long *counts)
{
    if (int rc = bfgx_cross_power_spectrum_device(device, (void *)s, N, map, map, L, nk, window_order, work, p1_sum, p_sum, p_sum, k_sum, counts)) return rc;
    HIP_TRY(hipMemcpyAsync(p_sum, p1_sum, sizeof(double) * nk, hipMemcpyDeviceToDevice, s));
    return BFGX_OK;
}

int particle_pk_check(int n_grid, double L, int order, int interlace, int nk)
{
    if (order != 2 && order != 3)
        return fail(BFGX_ERR_INVALID, "the particle power spectrum takes order 2 (CIC) or 3 (TSC), not %d: nearest grid point has no interlaced form", order);
    if (interlace != 0 && interlace != 1) return fail(BFGX_ERR_INVALID, "interlace %d: 0 (one grid) or 1 (two grids half a cell apart)", interlace);
    if (int rc = xpk_check_shape(n_grid, L, nk, order)) return rc;
    if (!std::isfinite(L)) return fail(BFGX_ERR_INVALID, "the particle power spectrum needs a finite L");
    return BFGX_OK;
}

}  // namespace

extern "C" {

int bfgx_interlaced_power_spectrum_device(int device, void *hip_stream, int32_t n_grid, const double *map1_dev, const double *map2_dev, double L,
                                          int32_t nk, int32_t window_order, double *work_dev, double *p_sum_dev, double *p1_sum_dev,
                                          double *k_sum_dev, unsigned long long *counts_dev)
{
    if (!map1_dev || !map2_dev || !work_dev || !p_sum_dev || !p1_sum_dev || !k_sum_dev || !counts_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = xpk_check_shape(n_grid, L, nk, window_order)) return rc;
    if (int rc = fourier_check_aligned(work_dev, "work_dev")) return rc;
    if (int rc = select_device(device)) return rc;
    return interlaced_enqueue(device, (hipStream_t)hip_stream, n_grid, map1_dev, map2_dev, L, nk, window_order, work_dev, p_sum_dev, p1_sum_dev,
                              k_sum_dev, counts_dev);
}

int64_t bfgx_particle_power_spectrum_work_doubles(int32_t n_grid)
{
    return 2 * (int64_t)n_grid * n_grid * n_grid + bfgx_cross_power_spectrum_work_doubles(n_grid);
}

int bfgx_particle_power_spectrum_device(int device, void *hip_stream, int64_t n, const double *x, const double *y, const double *z, const double *mass,
                                        int32_t n_grid, double L, int32_t order, int32_t interlace, int32_t nk, double *work_dev, double *p_sum_dev,
                                        double *p1_sum_dev, double *k_sum_dev, unsigned long long *counts_dev)
{
    if ((n > 0 && (!x || !y || !z)) || !work_dev || !p_sum_dev || !p1_sum_dev || !k_sum_dev || !counts_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (n < 0) return fail(BFGX_ERR_INVALID, "n = %lld particles", (long long)n);
    if (int rc = particle_pk_check(n_grid, L, order, interlace, nk)) return rc;
    if (int rc = fourier_check_aligned(work_dev, "work_dev")) return rc;
    // work: map 1, map 2, the two half spectra (n_grid^3 is a multiple of 2 doubles, so the spectra stay 16-byte aligned)
    const int64_t npts = (int64_t)n_grid * n_grid * n_grid;
    double *map1 = work_dev, *map2 = map1 + npts, *spectra = map2 + npts;
    if (int rc = deposit_cloud_impl(device, hip_stream, 3, n, x, y, z, mass, n_grid, L, order, map1)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    if (!interlace) return windowed_auto_enqueue(device, s, n_grid, map1, L, nk, order, spectra, p_sum_dev, p1_sum_dev, k_sum_dev, counts_dev);
    if (int rc = deposit_cloud_impl(device, hip_stream, 3, n, x, y, z, mass, n_grid, L, order, map2, 1, 1)) return rc;
    return interlaced_enqueue(device, s, n_grid, map1, map2, L, nk, order, spectra, p_sum_dev, p1_sum_dev, k_sum_dev, counts_dev);
}

int bfgx_particle_power_spectrum(int device, int64_t n, const double *x, const double *y, const double *z, const double *mass, int32_t n_grid,
                                 double L, int32_t order, int32_t interlace, int32_t nk, double *pk, double *pk_grid1, double *kcen, int64_t *counts)
{
    if ((n > 0 && (!x || !y || !z)) || !pk || !pk_grid1 || !kcen || !counts) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (n < 0) return fail(BFGX_ERR_INVALID, "n = %lld particles", (long long)n);
    if (int rc = particle_pk_check(n_grid, L, order, interlace, nk)) return rc;
    HostCall c(device);
    std::vector<double> h(3 * (size_t)nk);                   // the bins' sums (combined, grid 1, |k|)
    std::vector<unsigned long long> hc(nk);
    const double *dx = c.in(x, n), *dy = c.in(y, n), *dz = c.in(z, n), *dm = mass ? c.in(mass, n) : nullptr;
    double *dw = c.scratch<double>((size_t)bfgx_particle_power_spectrum_work_doubles(n_grid));
    double *ds = c.out(h.data(), 3 * (size_t)nk);
    unsigned long long *dc = c.out(hc.data(), nk);
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_particle_power_spectrum_device(device, nullptr, n, dx, dy, dz, dm, n_grid, L, order, interlace, nk, dw, ds, ds + nk, ds + 2 * nk, dc))
        return rc;
    if (int rc = c.finish()) return rc;
    bin_means(nk, h, hc, counts, {pk, pk_grid1, kcen});
    return BFGX_OK;
}

}  // extern "C"
