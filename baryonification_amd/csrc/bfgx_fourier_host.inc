// bfgx_fourier_host.inc -- what the Fourier families share on the host, each part stated once: the argument checks, the table cache, the
// dynamic-LDS attributes, the launchers of the strided and the line kernels, the 3-D setup with the transform passes built on it, and
// the small helpers (unit-circle tables, the k axis and bins, the bin sums).  Included by bfgx_api.hip before bfgx_fft_api.inc,
// bfgx_bispec_api.inc, bfgx_xpk_api.inc, bfgx_interlace_api.inc and bfgx_fft2d_api.inc, which all build on it.
// Kernels: bfgx_fft.hpp, bfgx_bispec.hpp, bfgx_fft2d.hpp.

namespace {

// ---- argument checks (no device call)
int ilog2_exact(int n) { int l = 0; while ((1 << l) < n) ++l; return ((1 << l) == n) ? l : -1; }

constexpr int kFft3MaxN = 1024, kFft2MaxN = 4096, kFft2StridedMaxN = 1024, kFft2MaxTable = 65536;
constexpr int kPkMaxNk = 2048, kPkMaxTableNk = 254;               // bins of a 3-D P(k); bins a byte of the bin table can name
static_assert(kFft2MaxNk == kPkMaxNk, "the 2-D and 3-D spectra take the same number of bins");
constexpr const char *kPkGridMsg = "power spectrum needs n_grid = 2^m with 8 <= n_grid <= 1024";

bool fourier_grid_ok(int n, int max_n) { return n <= max_n && ilog2_exact(n) >= 3; }

// n = 2^m, 8 <= n <= max_n, in the wording of the family
int fourier_check_grid(int n, int max_n, const char *msg)
{
    if (!fourier_grid_ok(n, max_n)) return fail(BFGX_ERR_UNSUPPORTED, "%s", msg);
    return BFGX_OK;
}

int fourier_check_aligned(const void *p, const char *what)
{
    if (reinterpret_cast<uintptr_t>(p) & 15) return fail(BFGX_ERR_INVALID, "%s must be 16-byte aligned (complex values)", what);
    return BFGX_OK;
}

// ---- the table cache: values per (device, ...), built by the first call that wants them, kept until bfgx_cache_clear, so that the entry
// points only enqueue.  Every cache registers itself: fourier_release_all() empties them all.
std::vector<std::function<void()>> g_fourier_release;

template <typename V, typename... K>
struct FourierCache {
    using Key = std::tuple<int, K...>;                            // (device, ...)
    std::mutex mu;
    std::map<Key, std::unique_ptr<V>> map;
    FourierCache() { g_fourier_release.push_back([this] { release(); }); }
    // the value of `key`, made by build(V &) -> error code when the key is new; under the cache's lock
    template <typename Build> int get(const Key &key, V **out, Build build)
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = map.find(key);
        if (it == map.end()) {
            auto v = std::make_unique<V>();
            if (int rc = build(*v)) return rc;
            it = map.emplace(key, std::move(v)).first;
        }
        *out = it->second.get();
        return BFGX_OK;
    }
    void release()
    {
        std::lock_guard<std::mutex> lk(mu);
        for (auto &kv : map) { (void)hipSetDevice(std::get<0>(kv.first)); kv.second.reset(); }
        map.clear();
    }
};

void fourier_release_all() { for (auto &release : g_fourier_release) release(); }

// ---- small helpers
// appends exp(sign 2 pi i k / n), k = first .. first + count - 1, as (re, im) pairs; the angle in long double, not reduced
void unit_circle(std::vector<double> &t, int n, int first, int count, int sign)
{
    for (int k = first; k < first + count; ++k) {
        const long double ang = (long double)sign * 2.0L * 3.141592653589793238462643383279502884L * (long double)k / (long double)n;
        t.push_back((double)cosl(ang));
        t.push_back((double)sinl(ang));
    }
}

// the notebook's k axis and bins (cells 12): klin[i] = n_i val, n = fftfreq(N) N, and nk bins of width dk from k_lo.  The binned results
// depend on these roundings: the operations stay in this order.
struct KAxis { double val, k_lo, dk; };
KAxis k_axis_bins(int N, double L, int nk)
{
    const double two_pi = 2 * 3.141592653589793;
    const double d = 1 / (two_pi / (L)) / N;                       // np.fft.fftfreq(Ngrd, 1 / (2 pi / Lbox) / Ngrd)
    const double val = 1.0 / (N * d);
    const double k_lo = two_pi / L;
    const double k_hi = two_pi / L * N / 2;                        // np.linspace(k_lo, k_hi, nk + 1)
    const double step = (k_hi - k_lo) / nk;
    const double kb1 = (nk == 1) ? k_hi : (1.0 * step + k_lo);
    return KAxis{val, k_lo, kb1 - k_lo};
}

int zero_bin_sums(hipStream_t s, int nk, unsigned long long *counts_dev, std::initializer_list<double *> sums_dev)
{
    for (double *p : sums_dev) HIP_TRY(hipMemsetAsync(p, 0, sizeof(double) * nk, s));
    HIP_TRY(hipMemsetAsync(counts_dev, 0, sizeof(unsigned long long) * nk, s));
    return BFGX_OK;
}

// rows of bin sums [rows][nk] and the bins' counts -> the means, row by row; 0 / 0 -> NaN for empty bins, as np.bincount(...) / k_c gives
void bin_means(int nk, const std::vector<double> &sums, const std::vector<unsigned long long> &hc, int64_t *counts, std::initializer_list<double *> means)
{
    for (int i = 0; i < nk; ++i) counts[i] = (int64_t)hc[i];
    size_t row = 0;
    for (double *m : means) {
        for (int i = 0; i < nk; ++i) m[i] = sums[row * (size_t)nk + i] / (double)hc[i];
        ++row;
    }
}

template <typename T> void free_host_vector(void *p) { delete static_cast<std::vector<T> *>(p); }

// the stream on which the frees of upload_owned run: one per device, non-blocking, made at first use and kept
std::mutex g_upload_mu;
std::map<int, hipStream_t> g_upload_free_streams;

hipError_t upload_free_stream(hipStream_t *out)                   // (of the current device)
{
    int device = 0;
    if (hipError_t e = hipGetDevice(&device)) return e;
    std::lock_guard<std::mutex> lk(g_upload_mu);
    auto it = g_upload_free_streams.find(device);
    if (it == g_upload_free_streams.end()) {
        hipStream_t st = nullptr;
        if (hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking)) return e;
        it = g_upload_free_streams.emplace(device, st).first;
    }
    *out = it->second;
    return hipSuccess;
}

// An upload whose host side belongs to the call alone: `host` moves onto the heap, the copy to `dst` is enqueued on `s`, and a host
// function frees the vector after the copy that reads it.  Calls that share a cached setup cannot reach each other's data.  The host
// function waits for the copy through an event, on a stream of its own: on `s` itself every later kernel of the call would wait for
// the runtime's callback thread (0.2 ms per bispectrum call at N = 256, measured).
template <typename T>
int upload_owned(hipStream_t s, void *dst, std::vector<T> &&host)
{
    std::vector<T> *h = new std::vector<T>(std::move(host));
    hipStream_t frees = nullptr;
    hipEvent_t copied = nullptr;
    hipError_t e = hipMemcpyAsync(dst, h->data(), sizeof(T) * h->size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = upload_free_stream(&frees);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&copied, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(copied, s);
    if (e == hipSuccess) e = hipStreamWaitEvent(frees, copied, 0);
    if (e == hipSuccess) e = hipLaunchHostFunc(frees, free_host_vector<T>, h);
    if (copied) (void)hipEventDestroy(copied);                     // (released by the runtime once it has completed)
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s);                             // (the copy may be pending: nothing reads the vector after this)
        delete h;
        HIP_TRY(e);
    }
    return BFGX_OK;
}

// rows of the half spectrum padded to whole 128-byte lines (8 complex values): a tile of 8 adjacent lines of a strided pass then
// moves exactly one line per row.  nz = 257 unpadded rows start at every multiple of 16 bytes and a 64-byte tile drags in 2.7x
// the bytes it uses (FETCH_SIZE, profiles/r02i_grid3d_summary.txt).
inline int fft_pitch(int N) { return (N / 2 + 1 + 7) & ~7; }

constexpr size_t kCuLdsBytes = 160 * 1024;

unsigned stream_grid(int n_cu, int64_t items) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, (int64_t)n_cu * 8)); }

// persistent workgroups striding over `ntiles` tiles: as many as LDS lets the CUs hold at once
unsigned persistent_wgs(int n_cu, int64_t ntiles, size_t lds)
{
    return (unsigned)std::min<int64_t>(ntiles, (int64_t)n_cu * std::max<size_t>(1, kCuLdsBytes / lds));
}

// ---- the strided kernel: the instantiation for N <= 1024 and its launch
struct StridedShape {
    int kind = 0;                      // 0: <LT 3, 256 threads> (N <= 128), 1: <3, 512> (N = 256, 512), 2: <2, 512> (N = 1024)
    int lt = 3, threads = 256;
    unsigned ztiles = 1;
    size_t lds = 0;                    // of BIN 0 and 5
};

StridedShape strided_shape(int N)
{
    StridedShape sh;
    sh.lt = kFftTileLog2;
    while (((size_t)N << sh.lt) > 4096 && sh.lt > 2) --sh.lt;                                         // at most 64 KB of tile per workgroup
    // two radix-4 quads per thread and pass where the tile has that many (N = 512, 8 lines)
    sh.threads = ((N >> 2) << sh.lt) >= 512 ? 512 : 256;     // (1024 threads: one workgroup per CU, measured 15 % slower at N = 512)
    sh.kind = sh.lt == 2 ? 2 : sh.threads == 512 ? 1 : 0;
    sh.ztiles = (unsigned)((N / 2 + 1 + (1 << sh.lt) - 1) >> sh.lt);
    sh.lds = fft_c2c_lds_bytes(N, sh.lt, 0, 0);
    return sh;
}

// XA: nothing (BIN 0, 1, 2), XpkArgs (the cross modes, BIN 3, 4) or TwistArgs (the twisted store, BIN 5)
template <int BIN, typename... XA> const void *strided_fn(int kind)
{
    return kind == 0 ? (const void *)fft_c2c_strided_kernel<BIN, 3, 256, XA...>
         : kind == 1 ? (const void *)fft_c2c_strided_kernel<BIN, 3, 512, XA...> : (const void *)fft_c2c_strided_kernel<BIN, 2, 512, XA...>;
}

// element i of line l of tile (o, kz0) at F[o * outer_stride + i * stride + kz0 + l], o < nouter; tw: exp(-2 pi i k / N), k < N / 2
template <int BIN, typename... XA>
int strided_launch(const StridedShape &sh, hipStream_t s, unsigned wgs, size_t lds, double2 *F, int N, int lg, const double2 *tw, int64_t stride,
                   int64_t outer_stride, int nouter, PkBins pb, XA... xa)
{
    int nz = N / 2 + 1, nzt = (int)sh.ztiles;
    void *args[] = {&F, &N, &lg, &nz, &stride, &outer_stride, &tw, &nzt, &nouter, &pb, (void *)&xa...};
    HIP_TRY(hipLaunchKernel(strided_fn<BIN, XA...>(sh.kind), dim3(wgs), dim3((unsigned)sh.threads), args, lds, s));
    return BFGX_OK;
}

// ---- the line kernels: real lines of `in` -> half spectra in `out` (r2c), or back (c2r), `npairs` pairs of lines of length N.
// Two line pairs per workgroup of 2 x 128 threads up to N = 512 (a workgroup per pair is launch-bound there: 0.51 -> 0.47 ms at 512^3;
// 4 pairs, or 64 / 256 threads per pair: 0.52 - 0.60), one pair x 256 threads at N = 1024 (3.5 ms; 2 x 128: 4.7), one pair x 512 above
template <int P, int T> const void *lines_fn(bool c2r) { return c2r ? (const void *)fft_c2r_lines_kernel<P, T> : (const void *)fft_r2c_lines_kernel<P, T>; }

int lines_launch(bool c2r, hipStream_t s, int N, int lg, const double2 *tw, size_t npairs, const void *in, void *out, int pitch)
{
    const bool wide = N > 1024, two = N <= 512 && npairs % 2 == 0;
    const void *fn = wide ? lines_fn<1, 512>(c2r) : two ? lines_fn<2, 128>(c2r) : lines_fn<1, 256>(c2r);
    const unsigned wg = (unsigned)(two ? npairs / 2 : npairs);
    const size_t lds = (two ? 2 : 1) * sizeof(double2) * N;
    void *args[] = {&in, &out, &N, &lg, &tw, &pitch};
    HIP_TRY(hipLaunchKernel(fn, dim3(wg), dim3(wide ? 512u : 256u), args, lds, s));
    return BFGX_OK;
}

// the instantiations of bispec_triangle_kernel: terms per thread (the last one holds kBispecMaxTri + kBispecMaxBins terms)
#define BFGX_BISPEC_TPT_LIST(X) X(1) X(2) X(3) X(4) X(5) X(6) X(8) X(10) X(12) X(16) X(20) X(24) X(28) X(33)
static_assert(kBispecMaxPerThread == 33, "the list ends at kBispecMaxPerThread");

// ---- the dynamic-LDS attribute belongs to a kernel instantiation, not to a setup: every instantiation the Fourier code launches gets the
// most any admissible shape can ask of it, once per device, so the order in which sizes are used does not matter.  The sizes come from
// the kernels' own *_lds_bytes functions and the limits of the argument checks; the setups call this when they are built.
std::mutex g_fourier_attr_mu;
std::vector<int> g_fourier_attr_devices;        // (under the mutex) the devices whose kernels have the attribute: recorded after every call succeeded

// The largest of them: the per-mode cross pass (BIN 4) at N = 1024 with 2048 bins, fft_c2c_lds_bytes(1024, 2, 2048, 4).  The kernels' size
// functions are not constexpr, so the figure is restated here for the static check, and every size they return is held to it below.
constexpr size_t kFourierMostLds = sizeof(double2) * ((kFft3MaxN << 2) + kFft3MaxN / 2) + sizeof(double) * 5 * kPkMaxNk;
static_assert(kFourierMostLds <= kCuLdsBytes, "the largest Fourier workgroup fits the LDS of a CU");

int fourier_set_lds(const void *fn, size_t bytes)
{
    if (bytes > kFourierMostLds) return fail(BFGX_ERR_HIP, "a Fourier kernel asks for %zu bytes of LDS: more than the %zu foreseen", bytes, kFourierMostLds);
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return BFGX_OK;
}

template <int BIN, typename... XA> int strided_attrs(int max_nk)
{
    size_t most[3] = {0, 0, 0};
    for (int N = 8; N <= kFft3MaxN; N *= 2) {
        const StridedShape sh = strided_shape(N);
        most[sh.kind] = std::max(most[sh.kind], fft_c2c_lds_bytes(N, sh.lt, max_nk, BIN));
    }
    for (int kind = 0; kind < 3; ++kind)
        if (int rc = fourier_set_lds(strided_fn<BIN, XA...>(kind), most[kind])) return rc;
    return BFGX_OK;
}

int fourier_kernel_attrs(int device)            // (device: the current one)
{
    std::lock_guard<std::mutex> lk(g_fourier_attr_mu);
    if (std::find(g_fourier_attr_devices.begin(), g_fourier_attr_devices.end(), device) != g_fourier_attr_devices.end()) return BFGX_OK;
    if (int rc = strided_attrs<0>(0)) return rc;
    if (int rc = strided_attrs<1>(kPkMaxNk)) return rc;
    if (int rc = strided_attrs<2>(kPkMaxTableNk)) return rc;
    if (int rc = strided_attrs<3, XpkArgs>(kPkMaxTableNk)) return rc;
    if (int rc = strided_attrs<4, XpkArgs>(kPkMaxNk)) return rc;
    if (int rc = strided_attrs<5, TwistArgs>(0)) return rc;
    for (int c2r = 0; c2r < 2; ++c2r) {
        if (int rc = fourier_set_lds(lines_fn<2, 128>(c2r), 2 * sizeof(double2) * 512)) return rc;
        if (int rc = fourier_set_lds(lines_fn<1, 256>(c2r), sizeof(double2) * 1024)) return rc;
        if (int rc = fourier_set_lds(lines_fn<1, 512>(c2r), sizeof(double2) * kFft2MaxN)) return rc;
    }
    if (int rc = fourier_set_lds((const void *)fft2_col_step_kernel<true>, fft2_col_step_lds_bytes(kFft2MaxPoints))) return rc;
    if (int rc = fourier_set_lds((const void *)fft2_col_step_kernel<false>, fft2_col_step_lds_bytes(kFft2MaxPoints))) return rc;
    if (int rc = fourier_set_lds((const void *)fft2_bin_kernel, fft2_bin_lds_bytes(kFft2MaxN, kFft2MaxNk))) return rc;
#define BFGX_TRI_ATTR(T) if (int rc = fourier_set_lds((const void *)bispec_triangle_kernel<T>, bispec_lds_bytes(kBispecMaxBins))) return rc;
    BFGX_BISPEC_TPT_LIST(BFGX_TRI_ATTR)
#undef BFGX_TRI_ATTR
    g_fourier_attr_devices.push_back(device);
    return BFGX_OK;
}

// ---- the 3-D setup: twiddles exp(-2 pi i k / N), the k axis and the bins of one (device, n_grid, L, nk), built on the host
struct FftSetup {
    DevBuf dtw, dkl;
    DevBuf dtab, dksb, dcnb;          // the tabulated bins (pk_table_build_kernel), built by the first binned pass when nk <= 254
    std::mutex tab_mu;                // held while they are built, up to the end of the build kernel
    std::atomic<bool> tab_ready{false};
    int N = 0, nk = 0, lg = 0, nz = 0, n_cu = 256;
    StridedShape sh;
    double k_lo = 0, dk = 0;
    size_t bin_lds(int bin) const { return fft_c2c_lds_bytes(N, sh.lt, nk, bin); }
    const double2 *tw() const { return dtw.as<double2>(); }
    int init(int device, int N_, double L, int nk_)            // (device: the current one; the entries have checked N, L, nk)
    {
        if (int rc = fourier_kernel_attrs(device)) return rc;
        N = N_; nk = nk_;
        lg = ilog2_exact(N);
        nz = N / 2 + 1;
        std::vector<double> twid, klin(N);
        unit_circle(twid, N, 0, N / 2, -1);
        const KAxis ka = k_axis_bins(N, L, nk);
        for (int i = 0; i < N; ++i) klin[i] = (double)(i < (N + 1) / 2 ? i : i - N) * ka.val;
        k_lo = ka.k_lo; dk = ka.dk;
        if (dtw.up(twid.data(), sizeof(double) * N) || dkl.up(klin.data(), sizeof(double) * N)) return alloc_fail("fft tables");
        sh = strided_shape(N);
        n_cu = device_cu_count(device);
        return BFGX_OK;
    }
    // the k axis and the bins as the binned passes take them
    PkBins bins(int b0, int pitch, double *pk_sum_dev, double *k_sum_dev, unsigned long long *counts_dev) const
    {
        return PkBins{dkl.as<double>(), k_lo, dk, 1.0 / dk, nk, b0, pk_sum_dev, k_sum_dev, counts_dev, nullptr, pitch};
    }
};

FourierCache<FftSetup, int, double, int> g_fft;

int fft_setup(int device, int N, double L, int nk, FftSetup **out)
{
    return g_fft.get(std::make_tuple(device, N, L, nk), out, [&](FftSetup &f) { return f.init(device, N, L, nk); });
}

// ---- the transform passes
// real lines along the last axis + complex transforms along the middle axis of `planes` planes: map [planes][N][N] -> F [planes][N][pitch]
int fft_planes(FftSetup &f, hipStream_t s, int N, int planes, const double *map_dev, double2 *F, int pitch)
{
    if (int rc = lines_launch(false, s, N, f.lg, f.tw(), (size_t)planes * N / 2, map_dev, F, pitch)) return rc;
    HIP_TRY(hipGetLastError());
    // axis 1: element (a, i, c) at (a * N + i) * pitch + c
    if (int rc = strided_launch<0>(f.sh, s, f.sh.ztiles * (unsigned)planes, f.sh.lds, F, N, f.lg, f.tw(), (int64_t)pitch, (int64_t)N * pitch, planes, PkBins{}))
        return rc;
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

// forward complex transforms, in place, along the FIRST axis of F [N][ncols][pitch], element (i, b, c) at (i * ncols + b) * pitch + c:
// persistent workgroups over the tiles.  BIN 5 with xa = TwistArgs: the twisted store of an interlaced pair
template <int BIN = 0, typename... XA>
int fft_axis0_store(FftSetup &f, hipStream_t s, int N, int ncols, double2 *F, int pitch, XA... xa)
{
    const unsigned wgs = persistent_wgs(f.n_cu, (int64_t)f.sh.ztiles * ncols, f.sh.lds);
    if (int rc = strided_launch<BIN>(f.sh, s, wgs, f.sh.lds, F, N, f.lg, f.tw(), (int64_t)ncols * pitch, (int64_t)pitch, ncols, PkBins{}, xa...)) return rc;
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

int fft_conj(const FftSetup &f, hipStream_t s, double2 *F, int64_t n)
{
    hipLaunchKernelGGL(fft_conj_kernel, dim3(stream_grid(f.n_cu, n)), dim3(256), 0, s, F, n);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

// forward transforms along the middle axis of F [planes][N][pitch], then complex to real along the last one -> map [planes][N][N].
// F holds the CONJUGATE of the spectrum to invert (conj(FFT(conj X)) = IFFT(X)): the last pass reads it back conjugated.
int ifft_planes_conj(FftSetup &f, hipStream_t s, int N, int planes, double2 *F, double *map, int pitch)
{
    if (int rc = strided_launch<0>(f.sh, s, f.sh.ztiles * (unsigned)planes, f.sh.lds, F, N, f.lg, f.tw(), (int64_t)pitch, (int64_t)N * pitch, planes, PkBins{}))
        return rc;
    HIP_TRY(hipGetLastError());
    if (int rc = lines_launch(true, s, N, f.lg, f.tw(), (size_t)planes * N / 2, F, map, pitch)) return rc;
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

// Bins, counts and |k| sums are functions of (N, L, nk) alone: tabulated by the first binned pass that wants them (one byte per mode),
// looked up afterwards.  Built exactly once: a thread that finds another one building waits for it.  pb: the setup's k axis and bins.
int fft_bin_table(FftSetup &f, hipStream_t s, const PkBins &pb)
{
    if (f.tab_ready.load(std::memory_order_acquire)) return BFGX_OK;
    std::lock_guard<std::mutex> lk(f.tab_mu);
    if (f.tab_ready.load(std::memory_order_relaxed)) return BFGX_OK;
    const int N = f.N, nk = f.nk;
    if (f.dtab.up(nullptr, ((size_t)N * f.sh.ztiles * N) << f.sh.lt) || f.dksb.up(nullptr, sizeof(double) * (size_t)N * nk) ||
        f.dcnb.up(nullptr, sizeof(unsigned long long) * (size_t)N * nk))
        return alloc_fail("P(k) bin table");
    PkBins all = pb;
    all.b0 = 0;
    hipLaunchKernelGGL(pk_table_build_kernel, dim3((unsigned)N), dim3(kFftBlock), 16 * (size_t)nk, s, all, N, f.nz, f.sh.lt, (int)f.sh.ztiles,
                       f.dtab.as<uint8_t>(), f.dksb.as<double>(), f.dcnb.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));                    // (built once; later calls on any stream find it complete)
    f.tab_ready.store(true, std::memory_order_release);
    return BFGX_OK;
}

// the tabulated part of a binned pass's sums: k_sum and counts of the columns [b0, b0 + nb)
int fft_table_sums(FftSetup &f, hipStream_t s, int b0, int nb, double *k_sum_dev, unsigned long long *counts_dev)
{
    hipLaunchKernelGGL(pk_table_sums_kernel, dim3((unsigned)f.nk), dim3(256), 0, s, f.nk, b0, nb, f.dksb.as<double>(), f.dcnb.as<unsigned long long>(),
                       k_sum_dev, counts_dev);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

}  // namespace
