// bfgx_fft2d_api.inc -- host side and C ABI of the 2-D FFTs of gridded maps (include/bfgx.h, "flat-sky maps"): the transform pair, power
// spectra, filters, the Kaiser-Squires pair and the derivatives of a filtered map; included by bfgx_api.hip after bfgx_interlace_api.inc (fft_pitch, ilog2_exact, xpk_window).
// Kernels: bfgx_fft2d.hpp, and the line and strided kernels of bfgx_fft.hpp / bfgx_bispec.hpp through a setup of their own.

namespace {

constexpr int kFft2MinN = 8, kFft2MaxN = 4096, kFft2StridedMaxN = 1024, kFft2MaxTable = 65536;

// twiddles of one (device, N), built in long double on the host, kept until bfgx_cache_clear
struct Fft2Setup {
    DevBuf dtw;                        // exp(-2 pi i k / N), k < N: the row passes and the strided pass read k < N/2, pass A all of it
    DevBuf dtw1, dtw2;                 // N > 1024: exp(-2 pi i k / N1), k < N1/2, and the same for N2
    int lg = 0, n1 = 0, n2 = 0, lg1 = 0, lg2 = 0;
    int lt = 3, threads = 256;         // N <= 1024: FftSetup's choice of the strided instantiation
    unsigned ztiles = 1;
    size_t lds = 0;
    int n_cu = 256;
    std::vector<double> beam;          // the table of the last filter call (host side of its upload)

    static int table(DevBuf &b, int n, int count)
    {
        std::vector<double> tw(2 * (size_t)count);
        for (int k = 0; k < count; ++k) {
            const long double ang = -2.0L * 3.141592653589793238462643383279502884L * (long double)k / (long double)n;
            tw[2 * k] = (double)cosl(ang); tw[2 * k + 1] = (double)sinl(ang);
        }
        return b.up(tw.data(), sizeof(double) * tw.size()) ? 1 : 0;
    }
    int init(int device, int N)
    {
        lg = ilog2_exact(N);
        if (table(dtw, N, N)) return alloc_fail("2-D fft twiddles");
        if (N > kFft2StridedMaxN) {
            lg1 = (lg + 1) / 2; lg2 = lg - lg1;                       // 2048 = 64 x 32, 4096 = 64 x 64
            n1 = 1 << lg1; n2 = 1 << lg2;
            if (table(dtw1, n1, n1 / 2) || table(dtw2, n2, n2 / 2)) return alloc_fail("2-D fft twiddles");
        } else {
            lt = kFftTileLog2;
            while (((size_t)N << lt) > 4096 && lt > 2) --lt;
            threads = ((N >> 2) << lt) >= 512 ? 512 : 256;
            ztiles = (unsigned)((N / 2 + 1 + (1 << lt) - 1) >> lt);
            lds = fft_c2c_lds_bytes(N, lt, 0, 0);
        }
        n_cu = device_cu_count(device);
        return BFGX_OK;
    }
    const void *strided_fn() const
    {
        if (lt == 3) return threads == 512 ? (const void *)fft_c2c_strided_kernel<0, 3, 512> : (const void *)fft_c2c_strided_kernel<0, 3, 256>;
        return threads == 512 ? (const void *)fft_c2c_strided_kernel<0, 2, 512> : (const void *)fft_c2c_strided_kernel<0, 2, 256>;
    }
};

std::mutex g_fft2_mu;
std::map<std::pair<int, int>, Fft2Setup *> g_fft2;
std::vector<int> g_fft2_attr_devices;          // (under g_fft2_mu) the devices whose kernels have their dynamic-LDS attribute

// The dynamic-LDS attribute belongs to a kernel instantiation: each gets the most any N asks of it, once per device, so the order in
// which setups of different sizes are built and used does not matter.
int fft2_kernel_attrs(int device)
{
    if (std::find(g_fft2_attr_devices.begin(), g_fft2_attr_devices.end(), device) != g_fft2_attr_devices.end()) return BFGX_OK;
#define BFGX_FFT2_ATTR(FN, BYTES) HIP_TRY(hipFuncSetAttribute((const void *)(FN), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(BYTES)))
    BFGX_FFT2_ATTR((fft_c2c_strided_kernel<0, 3, 256>), fft_c2c_lds_bytes(128, 3, 0, 0));
    BFGX_FFT2_ATTR((fft_c2c_strided_kernel<0, 3, 512>), fft_c2c_lds_bytes(512, 3, 0, 0));
    BFGX_FFT2_ATTR((fft_c2c_strided_kernel<0, 2, 512>), fft_c2c_lds_bytes(1024, 2, 0, 0));
    BFGX_FFT2_ATTR((fft_r2c_lines_kernel<1, 512>), sizeof(double2) * kFft2MaxN);
    BFGX_FFT2_ATTR((fft_c2r_lines_kernel<1, 512>), sizeof(double2) * kFft2MaxN);
    BFGX_FFT2_ATTR((fft2_col_step_kernel<true>), fft2_col_step_lds_bytes(kFft2MaxPoints));
    BFGX_FFT2_ATTR((fft2_col_step_kernel<false>), fft2_col_step_lds_bytes(kFft2MaxPoints));
    BFGX_FFT2_ATTR(fft2_bin_kernel, fft2_bin_lds_bytes(kFft2MaxN, kFft2MaxNk));
#undef BFGX_FFT2_ATTR
    g_fft2_attr_devices.push_back(device);
    return BFGX_OK;
}

int fft2_setup(int device, int N, Fft2Setup **out)
{
    std::lock_guard<std::mutex> lk(g_fft2_mu);
    if (int rc = fft2_kernel_attrs(device)) return rc;
    const auto key = std::make_pair(device, N);
    auto it = g_fft2.find(key);
    if (it == g_fft2.end()) {
        Fft2Setup *f = new Fft2Setup();
        if (int rc = f->init(device, N)) { delete f; return rc; }
        it = g_fft2.emplace(key, f).first;
    }
    *out = it->second;
    return BFGX_OK;
}

void fft2_release_all()
{
    std::lock_guard<std::mutex> lk(g_fft2_mu);
    for (auto &kv : g_fft2) { (void)hipSetDevice(kv.first.first); delete kv.second; }
    g_fft2.clear();
}

// ---- argument checks, stated once (no device call); the host and the _device entries give the same messages
int fft2_check_n(int n)
{
    if (n < kFft2MinN || n > kFft2MaxN || ilog2_exact(n) < 3) return fail(BFGX_ERR_UNSUPPORTED, "2-D transforms need n = 2^m with 8 <= n <= 4096");
    return BFGX_OK;
}

int fft2_check_aligned(const void *p, const char *what)
{
    if (reinterpret_cast<uintptr_t>(p) & 15) return fail(BFGX_ERR_INVALID, "%s must be 16-byte aligned (complex values)", what);
    return BFGX_OK;
}

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

unsigned fft2_stream_grid(const Fft2Setup &f, int64_t items) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, (int64_t)f.n_cu * 8)); }

// forward complex transforms along axis 0 of the half spectrum `from` [N][pitch] -> `to`; N <= 1024: in place, from == to; N > 1024:
// `from` is scratch afterwards and must not be `to`
int fft2_columns(Fft2Setup &f, hipStream_t s, int N, double2 *from, double2 *to)
{
    const int pitch = fft_pitch(N);
    if (N <= kFft2StridedMaxN) {
        const double2 *twp = f.dtw.as<double2>();
        int lg = f.lg, nz = N / 2 + 1, nzt = (int)f.ztiles, nouter = 1, n = N;
        int64_t stride = pitch, outer = (int64_t)N * pitch;
        PkBins pb{};
        void *args[] = {&to, &n, &lg, &nz, &stride, &outer, &twp, &nzt, &nouter, &pb};
        HIP_TRY(hipLaunchKernel(f.strided_fn(), dim3(f.ztiles), dim3((unsigned)f.threads), args, f.lds, s));
        return BFGX_OK;
    }
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

// the workgroup shapes of the line passes: fft_planes' up to N = 1024, one pair x 512 threads above
#define BFGX_FFT2_LINES(KERNEL, N, ...)                                                                                                   \
    do {                                                                                                                                  \
        const size_t npairs = (size_t)(N) / 2;                                                                                            \
        if ((N) > kFft2StridedMaxN) hipLaunchKernelGGL((KERNEL<1, 512>), dim3((unsigned)npairs), dim3(512), sizeof(double2) * (N), s, __VA_ARGS__); \
        else if ((N) <= 512 && npairs % 2 == 0) hipLaunchKernelGGL((KERNEL<2, 128>), dim3((unsigned)(npairs / 2)), dim3(256), 2 * sizeof(double2) * (N), s, __VA_ARGS__); \
        else hipLaunchKernelGGL((KERNEL<1, 256>), dim3((unsigned)npairs), dim3(256), sizeof(double2) * (N), s, __VA_ARGS__);            \
    } while (0)

// map [N][N] -> its half spectrum in `out`; `u`: scratch half spectrum (N > 1024 only)
int fft2_forward(Fft2Setup &f, hipStream_t s, int N, const double *map, double2 *out, double2 *u)
{
    const int pitch = fft_pitch(N);
    double2 *rows = N <= kFft2StridedMaxN ? out : u;
    BFGX_FFT2_LINES(fft_r2c_lines_kernel, N, map, rows, N, f.lg, f.dtw.as<double2>(), pitch);
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
    const double2 *in = cols;
    BFGX_FFT2_LINES(fft_c2r_lines_kernel, N, in, map, N, f.lg, f.dtw.as<double2>(), pitch);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}
#undef BFGX_FFT2_LINES

int fft2_filter(Fft2Setup &f, hipStream_t s, int N, const double2 *spec, double2 *out, int kind, double L, double param, const double *tk,
                const double *tb, int nt, double scale)
{
    const int pitch = fft_pitch(N);
    hipLaunchKernelGGL(fft2_filter_kernel, dim3(fft2_stream_grid(f, (int64_t)N * pitch)), dim3(kFft2Threads), 0, s, spec, out, N, pitch, kind,
                       2 * 3.141592653589793 / L, param, tk, tb, nt, scale);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

void fft2_free_beam(void *p) { delete static_cast<std::vector<double> *>(p); }

int fft2_ks(Fft2Setup &f, hipStream_t s, int N, double2 *s1, double2 *s2, int eb)
{
    const int pitch = fft_pitch(N);
    hipLaunchKernelGGL(fft2_ks_kernel, dim3(fft2_stream_grid(f, (int64_t)N * pitch)), dim3(kFft2Threads), 0, s, s1, s2, N, pitch, eb,
                       1.0 / ((double)N * (double)N));
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

}  // namespace

extern "C" {

int64_t bfgx_fft2_work_doubles(int32_t n)
{
    if (n < kFft2MinN || n > kFft2MaxN || ilog2_exact(n) < 3) return 0;
    return 6 * (int64_t)n * fft_pitch(n);
}

int bfgx_rfft2_device(int device, void *hip_stream, int32_t n, const double *map_dev, double *work_dev, double *spec_out_dev)
{
    if (!map_dev || !work_dev || !spec_out_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = fft2_check_n(n)) return rc;
    if (int rc = fft2_check_aligned(work_dev, "work_dev")) return rc;
    if (int rc = fft2_check_aligned(spec_out_dev, "spec_out_dev")) return rc;
    if (int rc = select_device(device)) return rc;
    Fft2Setup *f = nullptr;
    if (int rc = fft2_setup(device, n, &f)) return rc;
    return fft2_forward(*f, (hipStream_t)hip_stream, n, map_dev, (double2 *)spec_out_dev, Fft2Work(work_dev, n).u);
}

int bfgx_irfft2_device(int device, void *hip_stream, int32_t n, const double *spec_dev, double scale, double *work_dev, double *map_out_dev)
{
    if (!spec_dev || !work_dev || !map_out_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = fft2_check_n(n)) return rc;
    if (int rc = fft2_check_aligned(work_dev, "work_dev")) return rc;
    if (int rc = fft2_check_aligned(spec_dev, "spec_dev")) return rc;
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
    if (int rc = fft2_check_aligned(work_dev, "work_dev")) return rc;
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
    HIP_TRY(hipMemsetAsync(paa_sum_dev, 0, sizeof(double) * nk, s));
    HIP_TRY(hipMemsetAsync(pbb_sum_dev, 0, sizeof(double) * nk, s));
    HIP_TRY(hipMemsetAsync(pab_sum_dev, 0, sizeof(double) * nk, s));
    HIP_TRY(hipMemsetAsync(k_sum_dev, 0, sizeof(double) * nk, s));
    HIP_TRY(hipMemsetAsync(counts_dev, 0, sizeof(unsigned long long) * nk, s));
    // the k axis and the bins of FftSetup::init (np.fft.fftfreq, np.linspace), the same roundings
    const double two_pi = 2 * 3.141592653589793;
    const double d = 1 / (two_pi / (L)) / N;
    const double val = 1.0 / (N * d);
    const double k_lo = two_pi / L, k_hi = two_pi / L * N / 2;
    const double step = (k_hi - k_lo) / nk;
    const double kb1 = (nk == 1) ? k_hi : (1.0 * step + k_lo);
    const double dk = kb1 - k_lo;
    const Fft2Bins fb{val, k_lo, dk, 1.0 / dk, nk, paa_sum_dev, pbb_sum_dev, pab_sum_dev, k_sum_dev, counts_dev};
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
    if (int rc = fft2_check_aligned(work_dev, "work_dev")) return rc;
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    Fft2Setup *f = nullptr;
    if (int rc = fft2_setup(device, n, &f)) return rc;
    const int N = n;
    const Fft2Work w(work_dev, N);
    const double *tk = nullptr, *tb = nullptr;
    if (kind == kFft2Table) {
        // the table rides in the second spectrum of the work array; the copy is ordered on the stream before its reader
        std::lock_guard<std::mutex> lk(g_fft2_mu);
        f->beam.assign(table_k_host, table_k_host + ntable);
        f->beam.insert(f->beam.end(), table_b_host, table_b_host + ntable);
        HIP_TRY(hipMemcpyAsync(w.s2, f->beam.data(), sizeof(double) * f->beam.size(), hipMemcpyHostToDevice, s));
        tk = (const double *)w.s2; tb = tk + ntable;
    }
    if (int rc = fft2_forward(*f, s, N, map_dev, w.s1, w.u)) return rc;
    if (int rc = fft2_filter(*f, s, N, w.s1, w.s1, kind, L, param, tk, tb, ntable, 1.0 / ((double)N * (double)N))) return rc;
    return fft2_inverse_conj(*f, s, N, w.s1, w.u, map_out_dev);
}

// The work array of the derivatives: nder products [n][pitch], then u, the other side of the out-of-place column pass.  The beam table
// rides in u: it is copied there before fft2_der_kernel, read by that kernel alone, and u is first written by the column passes after it.
// Its host copy is a vector of the call's own (not Fft2Setup::beam, which calls on one setup share), deleted by a host function that the
// stream runs after the copy: two threads on one setup cannot reach each other's table.
int64_t bfgx_derivatives_2d_work_doubles(int32_t n, int32_t nder)
{
    if (n < kFft2MinN || n > kFft2MaxN || ilog2_exact(n) < 3 || (nder != 1 && nder != 6)) return 0;
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
    if (int rc = fft2_check_aligned(work_dev, "work_dev")) return rc;
    if (int rc = fft2_check_aligned(spec_dev, "spec_dev")) return rc;
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    Fft2Setup *f = nullptr;
    if (int rc = fft2_setup(device, n, &f)) return rc;
    const int N = n, pitch = fft_pitch(N);
    const int64_t half = (int64_t)N * pitch;
    double2 *prod = (double2 *)work_dev, *u = prod + (int64_t)nder * half;
    const double *tk = nullptr, *tb = nullptr;
    if (kind == kFft2Table) {
        // the host side of the upload belongs to this call alone: it is freed by the stream itself, after the copy that reads it
        std::vector<double> *beam = new std::vector<double>(table_k_host, table_k_host + ntable);
        beam->insert(beam->end(), table_b_host, table_b_host + ntable);
        hipError_t e = hipMemcpyAsync(u, beam->data(), sizeof(double) * beam->size(), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipLaunchHostFunc(s, fft2_free_beam, beam);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(s);                             // (the copy may be pending: nothing reads the vector after this)
            delete beam;
            HIP_TRY(e);
        }
        tk = (const double *)u; tb = tk + ntable;
    }
    hipLaunchKernelGGL(fft2_der_kernel, dim3(fft2_stream_grid(*f, half)), dim3(kFft2Threads), 0, s, (const double2 *)spec_dev, prod, N, pitch,
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
    if (int rc = fft2_check_aligned(work_dev, "work_dev")) return rc;
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
    if (int rc = fft2_check_aligned(work_dev, "work_dev")) return rc;
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
    std::vector<double> h(4 * (size_t)nk);                   // the bins' sums (aa, bb, ab, |k|), divided by their counts below
    std::vector<unsigned long long> hc(nk);
    const double *da = c.in(map_a, N * N), *db = (map_b == map_a) ? da : c.in(map_b, N * N);
    double *dw = c.scratch<double>((size_t)bfgx_fft2_work_doubles(n));
    double *ds = c.out(h.data(), 4 * (size_t)nk);
    unsigned long long *dc = c.out(hc.data(), nk);
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_power_spectrum_2d_device(device, nullptr, n, da, db, L, nk, window_order, dw, ds, ds + nk, ds + 2 * nk, ds + 3 * nk, dc)) return rc;
    if (int rc = c.finish()) return rc;
    for (int i = 0; i < nk; ++i) {
        const double m = (double)hc[i];                      // 0 / 0 -> NaN for empty bins, as in bfgx_power_spectrum
        counts[i] = (int64_t)hc[i];
        paa[i] = h[i] / m;
        pbb[i] = h[nk + i] / m;
        pab[i] = h[2 * (size_t)nk + i] / m;
        kcen[i] = h[3 * (size_t)nk + i] / m;
    }
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
