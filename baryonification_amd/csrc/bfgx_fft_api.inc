// bfgx_fft_api.inc -- host side of the 3-D FFT and C ABI of the power spectrum of gridded maps (include/bfgx.h, "power spectrum");
// included by bfgx_api.hip after bfgx_deposit_api.inc.  bfgx_bispec_api.inc, bfgx_xpk_api.inc and bfgx_interlace_api.inc build on FftSetup, fft_setup, fft_planes
// and fft_pitch.
// Kernels: bfgx_fft.hpp.

namespace {

int ilog2_exact(int n) { int l = 0; while ((1 << l) < n) ++l; return ((1 << l) == n) ? l : -1; }

// twiddles exp(-2 pi i k / N) and the notebook's k axis / bins (cells 12: fftfreq, linspace), built on the host
struct FftSetup {
    DevBuf dtw, dkl;
    DevBuf dtab, dksb, dcnb;          // the tabulated bins (pk_table_build_kernel), built by the first binned pass when nk <= 254
    bool tab_ready = false;
    int lg = 0, nz = 0, tile = 1, lt = 2, threads = 256;
    unsigned ztiles = 1;
    size_t lds = 0, lds_bin1 = 0, lds_bin2 = 0, lds_bin3 = 0, lds_bin4 = 0;
    // the instantiation of the strided kernel for this setup's (lines per tile, threads)
    template <int BIN> const void *strided_fn()
    {
        if (lt == 3) return threads == 1024 ? (const void *)fft_c2c_strided_kernel<BIN, 3, 1024> : threads == 512 ? (const void *)fft_c2c_strided_kernel<BIN, 3, 512> : (const void *)fft_c2c_strided_kernel<BIN, 3, 256>;
        return threads == 1024 ? (const void *)fft_c2c_strided_kernel<BIN, 2, 1024> : threads == 512 ? (const void *)fft_c2c_strided_kernel<BIN, 2, 512> : (const void *)fft_c2c_strided_kernel<BIN, 2, 256>;
    }
    template <int BIN> int strided_attr(size_t bytes)
    {
        HIP_TRY(hipFuncSetAttribute(strided_fn<BIN>(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        return BFGX_OK;
    }
    template <int BIN> int strided_launch(hipStream_t s, unsigned wgs, size_t bytes, double2 *F, int N, int64_t stride, int64_t outer_stride, int nouter,
                                          const PkBins &pb)
    {
        const double2 *twp = dtw.as<double2>();
        int lg_ = lg, nz_ = nz, nzt_ = (int)ztiles;
        PkBins pbv = pb;
        void *args[] = {&F, &N, &lg_, &nz_, &stride, &outer_stride, &twp, &nzt_, &nouter, &pbv};
        HIP_TRY(hipLaunchKernel(strided_fn<BIN>(), dim3(wgs), dim3((unsigned)threads), args, bytes, s));
        return BFGX_OK;
    }
    // the cross modes (BIN 3, 4; bfgx_xpk_api.inc): instantiated for the thread counts init() selects
    template <int BIN> const void *xpk_fn()
    {
        if (lt == 3) return threads == 512 ? (const void *)fft_c2c_strided_kernel<BIN, 3, 512, XpkArgs> : (const void *)fft_c2c_strided_kernel<BIN, 3, 256, XpkArgs>;
        return threads == 512 ? (const void *)fft_c2c_strided_kernel<BIN, 2, 512, XpkArgs> : (const void *)fft_c2c_strided_kernel<BIN, 2, 256, XpkArgs>;
    }
    template <int BIN> int xpk_attr(size_t bytes)
    {
        HIP_TRY(hipFuncSetAttribute(xpk_fn<BIN>(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        return BFGX_OK;
    }
    template <int BIN> int xpk_launch(hipStream_t s, unsigned wgs, size_t bytes, double2 *F, int N, int64_t stride, int64_t outer_stride, int nouter,
                                      const PkBins &pb, const XpkArgs &xa)
    {
        const double2 *twp = dtw.as<double2>();
        int lg_ = lg, nz_ = nz, nzt_ = (int)ztiles;
        PkBins pbv = pb;
        XpkArgs xav = xa;
        void *args[] = {&F, &N, &lg_, &nz_, &stride, &outer_stride, &twp, &nzt_, &nouter, &pbv, &xav};
        HIP_TRY(hipLaunchKernel(xpk_fn<BIN>(), dim3(wgs), dim3((unsigned)threads), args, bytes, s));
        return BFGX_OK;
    }
    // the twisted store pass of an interlaced pair (BIN 5; bfgx_interlace_api.inc): the LDS of BIN 0, the thread counts init() selects
    const void *twist_fn()
    {
        if (lt == 3) return threads == 512 ? (const void *)fft_c2c_strided_kernel<5, 3, 512, TwistArgs> : (const void *)fft_c2c_strided_kernel<5, 3, 256, TwistArgs>;
        return threads == 512 ? (const void *)fft_c2c_strided_kernel<5, 2, 512, TwistArgs> : (const void *)fft_c2c_strided_kernel<5, 2, 256, TwistArgs>;
    }
    int twist_launch(hipStream_t s, unsigned wgs, double2 *F, int N, int64_t stride, int64_t outer_stride, int nouter, int b0, const double2 *phase)
    {
        const double2 *twp = dtw.as<double2>();
        int lg_ = lg, nz_ = nz, nzt_ = (int)ztiles;
        PkBins pbv{};
        pbv.b0 = b0;
        TwistArgs tav{phase};
        void *args[] = {&F, &N, &lg_, &nz_, &stride, &outer_stride, &twp, &nzt_, &nouter, &pbv, &tav};
        HIP_TRY(hipLaunchKernel(twist_fn(), dim3(wgs), dim3((unsigned)threads), args, lds, s));
        return BFGX_OK;
    }
    int n_cu = 256;
    double k_lo = 0, dk = 0;
    int init(int device, int N, double L, int nk)            // (device: the current one)
    {
        lg = ilog2_exact(N);
        if (lg < 3 || N > 1024) return fail(BFGX_ERR_UNSUPPORTED, "power spectrum needs n_grid = 2^m with 8 <= n_grid <= 1024");
        nz = N / 2 + 1;
        std::vector<double> tw(N), klin(N);
        for (int k = 0; k < N / 2; ++k) {
            const long double ang = -2.0L * 3.141592653589793238462643383279502884L * (long double)k / (long double)N;
            tw[2 * k] = (double)cosl(ang); tw[2 * k + 1] = (double)sinl(ang);
        }
        const double two_pi = 2 * 3.141592653589793;
        const double d = 1 / (two_pi / (L)) / N;                       // np.fft.fftfreq(Ngrd, 1 / (2 pi / Lbox) / Ngrd)
        const double val = 1.0 / (N * d);
        for (int i = 0; i < N; ++i) klin[i] = (double)(i < (N + 1) / 2 ? i : i - N) * val;
        k_lo = two_pi / L;
        const double k_hi = two_pi / L * N / 2;                        // np.linspace(k_lo, k_hi, nk + 1)
        const double step = (k_hi - k_lo) / nk;
        const double kb1 = (nk == 1) ? k_hi : (1.0 * step + k_lo);
        dk = kb1 - k_lo;
        if (dtw.up(tw.data(), sizeof(double) * N) || dkl.up(klin.data(), sizeof(double) * N)) return alloc_fail("fft tables");
        lt = kFftTileLog2;
        while (((size_t)N << lt) > 4096 && lt > 2) --lt;                                              // at most 64 KB of tile per workgroup
        tile = 1 << lt;
        // two radix-4 quads per thread and pass where the tile has that many (N = 512, 8 lines)
        const int nq = (N >> 2) << lt;
        threads = nq >= 512 ? 512 : 256;       // (1024 threads: one workgroup per CU, measured 15 % slower at N = 512)
        ztiles = (unsigned)((nz + tile - 1) / tile);
        lds = fft_c2c_lds_bytes(N, lt, 0, 0);
        lds_bin1 = fft_c2c_lds_bytes(N, lt, nk, 1);
        lds_bin2 = fft_c2c_lds_bytes(N, lt, nk, 2);
        if (int rc = strided_attr<0>(lds)) return rc;
        if (int rc = strided_attr<1>(lds_bin1)) return rc;
        if (int rc = strided_attr<2>(lds_bin2)) return rc;
        lds_bin3 = fft_c2c_lds_bytes(N, lt, nk, 3);
        lds_bin4 = fft_c2c_lds_bytes(N, lt, nk, 4);
        if (int rc = xpk_attr<3>(lds_bin3)) return rc;
        if (int rc = xpk_attr<4>(lds_bin4)) return rc;
        HIP_TRY(hipFuncSetAttribute(twist_fn(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        n_cu = device_cu_count(device);
        return BFGX_OK;
    }
};

// twiddle / wavenumber tables per (device, n_grid, L, nk): built by the first call, kept until bfgx_cache_clear, so that the
// power-spectrum entry points only enqueue
std::mutex g_fft_mu;
std::map<std::tuple<int, int, double, int>, FftSetup *> g_fft;

int fft_setup(int device, int N, double L, int nk, FftSetup **out)
{
    std::lock_guard<std::mutex> lk(g_fft_mu);
    const auto key = std::make_tuple(device, N, L, nk);
    auto it = g_fft.find(key);
    if (it == g_fft.end()) {
        FftSetup *f = new FftSetup();
        if (int rc = f->init(device, N, L, nk)) { delete f; return rc; }
        it = g_fft.emplace(key, f).first;
    }
    *out = it->second;
    return BFGX_OK;
}

void fft_release_all()
{
    std::lock_guard<std::mutex> lk(g_fft_mu);
    for (auto &kv : g_fft) { (void)hipSetDevice(std::get<0>(kv.first)); delete kv.second; }
    g_fft.clear();
}

// rows of the half spectrum padded to whole 128-byte lines (8 complex values): a tile of 8 adjacent lines of a strided pass then
// moves exactly one line per row.  nz = 257 unpadded rows start at every multiple of 16 bytes and a 64-byte tile drags in 2.7x
// the bytes it uses (FETCH_SIZE, profiles/r02i_grid3d_summary.txt).
inline int fft_pitch(int N) { return (N / 2 + 1 + 7) & ~7; }

// real lines along the last axis + complex transforms along the middle axis of `planes` planes: map [planes][N][N] -> F [planes][N][pitch]
int fft_planes(FftSetup &f, hipStream_t s, int N, int planes, const double *map_dev, double2 *F, int pitch)
{
    {
        // two line pairs per workgroup of 2 x 128 threads up to N = 512 (a workgroup per pair is launch-bound there: 0.51 -> 0.47 ms at
        // 512^3; 4 pairs, or 64 / 256 threads per pair: 0.52 - 0.60), one pair x 256 threads above (N = 1024: 3.5 ms; 2 x 128: 4.7)
        const size_t npairs = (size_t)planes * N / 2;
        const bool two = N <= 512 && npairs % 2 == 0;
        const unsigned wg = (unsigned)(two ? npairs / 2 : npairs);
        const size_t ldsb = (two ? 2 : 1) * sizeof(double2) * N;
#define BFGX_R2C(P, T) hipLaunchKernelGGL((fft_r2c_lines_kernel<P, T>), dim3(wg), dim3(P * T), ldsb, s, map_dev, F, N, f.lg, f.dtw.as<double2>(), pitch)
        if (two) BFGX_R2C(2, 128);
        else BFGX_R2C(1, 256);
#undef BFGX_R2C
    }
    HIP_TRY(hipGetLastError());
    // axis 1: element (a, i, c) at (a * N + i) * pitch + c
    const unsigned wgs = f.ztiles * (unsigned)planes;
    if (int rc = f.strided_launch<0>(s, wgs, f.lds, F, N, (int64_t)pitch, (int64_t)N * pitch, planes, PkBins{})) return rc;
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

// bins, counts and |k| sums are functions of (N, L, nk) alone: tabulated by the first binned pass that wants them (one byte per mode),
// looked up afterwards.  pb: the setup's k axis and bins.
int fft_bin_table(FftSetup &f, hipStream_t s, int N, int nk, const PkBins &pb)
{
    if (f.tab_ready) return BFGX_OK;
    if (f.dtab.up(nullptr, ((size_t)N * f.ztiles * N) << f.lt) || f.dksb.up(nullptr, sizeof(double) * (size_t)N * nk) ||
        f.dcnb.up(nullptr, sizeof(unsigned long long) * (size_t)N * nk))
        return alloc_fail("P(k) bin table");
    PkBins all = pb;
    all.b0 = 0;
    hipLaunchKernelGGL(pk_table_build_kernel, dim3((unsigned)N), dim3(kFftBlock), 16 * (size_t)nk, s, all, N, f.nz, f.lt, (int)f.ztiles, f.dtab.as<uint8_t>(),
                       f.dksb.as<double>(), f.dcnb.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));                    // (built once; later calls on any stream find it complete)
    f.tab_ready = true;
    return BFGX_OK;
}

// complex transforms along the FIRST axis of F [N][nb][pitch] (the columns b0 .. b0 + nb of the middle axis) fused with the P(k)
// sums: the transformed tiles are binned from LDS and never written back (F is scratch afterwards)
int fft_axis0_pk(FftSetup &f, hipStream_t s, int N, int nb, int b0, double2 *F, int pitch, int nk, double *pk_sum_dev, double *k_sum_dev,
                 unsigned long long *counts_dev)
{
    HIP_TRY(hipMemsetAsync(pk_sum_dev, 0, sizeof(double) * nk, s));
    HIP_TRY(hipMemsetAsync(k_sum_dev, 0, sizeof(double) * nk, s));
    HIP_TRY(hipMemsetAsync(counts_dev, 0, sizeof(unsigned long long) * nk, s));
    // axis 0: element (i, b, c) at (i * nb + b) * pitch + c.  A fixed number of workgroups strides over the tiles, each flushing
    // its histogram once (3 nk global atomics per workgroup, not per tile)
    const int64_t ntiles = (int64_t)f.ztiles * nb;
    const unsigned wgs = (unsigned)std::min<int64_t>(ntiles, (int64_t)f.n_cu * std::max<size_t>(1, (size_t)(160 * 1024) / f.lds_bin2));
    PkBins pb{f.dkl.as<double>(), f.k_lo, f.dk, 1.0 / f.dk, nk, b0, pk_sum_dev, k_sum_dev, counts_dev, nullptr, pitch};
    const bool use_tab = nk <= 254;
    if (use_tab) {
        if (int rc = fft_bin_table(f, s, N, nk, pb)) return rc;
        pb.tab = f.dtab.as<uint8_t>();
        if (int rc = f.strided_launch<2>(s, wgs, f.lds_bin2, F, N, (int64_t)nb * pitch, (int64_t)pitch, nb, pb)) return rc;
        hipLaunchKernelGGL(pk_table_sums_kernel, dim3((unsigned)nk), dim3(256), 0, s, nk, b0, nb, f.dksb.as<double>(),
                           f.dcnb.as<unsigned long long>(), k_sum_dev, counts_dev);
        HIP_TRY(hipGetLastError());
        return BFGX_OK;
    }
    if (int rc = f.strided_launch<1>(s, wgs, f.lds_bin1, F, N, (int64_t)nb * pitch, (int64_t)pitch, nb, pb)) return rc;
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
    if (nk < 1 || nk > 2048 || !(L > 0)) return fail(BFGX_ERR_INVALID, "power spectrum needs 1 <= nk <= 2048, L > 0");
    if (reinterpret_cast<uintptr_t>(work_dev) & 15) return fail(BFGX_ERR_INVALID, "work_dev must be 16-byte aligned (complex values)");
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    FftSetup *f = nullptr;
    if (int rc = fft_setup(device, n_grid, L, nk, &f)) return rc;
    const int pitch = fft_pitch(n_grid);
    if (int rc = fft_planes(*f, s, n_grid, n_grid, map_dev, (double2 *)work_dev, pitch)) return rc;
    return fft_axis0_pk(*f, s, n_grid, n_grid, 0, (double2 *)work_dev, pitch, nk, pk_sum_dev, k_sum_dev, counts_dev);
}

int bfgx_fft_slab_planes_device(int device, void *hip_stream, int32_t n_grid, int32_t planes, const double *map_dev, double *work_dev)
{
    if (!map_dev || !work_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
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
    if (nk < 1 || nk > 2048 || !(L > 0)) return fail(BFGX_ERR_INVALID, "power spectrum needs 1 <= nk <= 2048, L > 0");
    if (ncols < 1 || col0 < 0 || col0 + ncols > n_grid) return fail(BFGX_ERR_INVALID, "columns [%d, %d) outside the grid", col0, col0 + ncols);
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    FftSetup *f = nullptr;
    if (int rc = fft_setup(device, n_grid, L, nk, &f)) return rc;
    return fft_axis0_pk(*f, s, n_grid, ncols, col0, (double2 *)work_dev, fft_pitch(n_grid), nk, pk_sum_dev, k_sum_dev, counts_dev);
}

int bfgx_power_spectrum(int device, int32_t n_grid, const double *map, double L, int32_t nk, double *pk, double *kcen, int64_t *counts)
{
    if (!map || !pk || !kcen || !counts) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (ilog2_exact(n_grid) < 3 || n_grid > 1024) return fail(BFGX_ERR_UNSUPPORTED, "power spectrum needs n_grid = 2^m with 8 <= n_grid <= 1024");
    if (nk < 1 || nk > 2048) return fail(BFGX_ERR_INVALID, "power spectrum needs 1 <= nk <= 2048");
    HostCall c(device);
    const size_t N = n_grid;
    std::vector<double> hp(nk), hk(nk);                      // the bins' sums, divided by their counts below
    std::vector<unsigned long long> hc(nk);
    const double *dm = c.in(map, N * N * N);
    double *dw = c.scratch<double>(bfgx_power_spectrum_work_doubles(n_grid)), *dp = c.out(hp.data(), nk), *dk = c.out(hk.data(), nk);
    unsigned long long *dc = c.out(hc.data(), nk);
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_power_spectrum_device(device, nullptr, n_grid, dm, L, nk, dw, dp, dk, dc)) return rc;
    if (int rc = c.finish()) return rc;
    for (int i = 0; i < nk; ++i) {
        counts[i] = (int64_t)hc[i];
        pk[i] = hp[i] / (double)hc[i];           // 0 / 0 -> NaN for empty bins, as np.bincount(...) / k_c gives
        kcen[i] = hk[i] / (double)hc[i];
    }
    return BFGX_OK;
}

}  // extern "C"
