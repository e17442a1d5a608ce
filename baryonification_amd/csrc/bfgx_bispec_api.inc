// C ABI of the bispectrum of gridded 3-D maps and of the inverse slab transforms it is built on (include/bfgx.h, "bispectrum");
// included by bfgx_api.hip after bfgx_fourier_host.inc, on which alone it builds (FftSetup, the transform passes, the table cache,
// upload_owned).  Kernels: bfgx_bispec.hpp.

namespace {

// the n^2 -> bin table of one (device, n, L, edges): what the triangle kernels need besides the FFT setup
struct BispecSetup {
    DevBuf dtab;                         // uint8 [3 (n/2)^2 + 1], 255 = outside the bins
    int init(int N, double L, int nb, const double *edges)
    {
        const int h = N / 2;
        std::vector<uint8_t> tab(3 * (size_t)h * h + 1);
        for (size_t n2 = 0; n2 < tab.size(); ++n2) {
            const double k = 2 * 3.141592653589793 / L * sqrt((double)n2);
            const int i = (int)(std::upper_bound(edges, edges + nb + 1, k) - edges) - 1;       // np.searchsorted(edges, k, side='right') - 1
            tab[n2] = (i >= 0 && i < nb) ? (uint8_t)i : (uint8_t)255;
        }
        if (dtab.up(tab.data(), tab.size())) return alloc_fail("bispectrum bin table");
        return BFGX_OK;
    }
};

FourierCache<BispecSetup, int, double, std::vector<double>> g_bispec;

int bispec_setup(int device, int N, double L, int nb, const double *edges, BispecSetup **out)
{
    return g_bispec.get(std::make_tuple(device, N, L, std::vector<double>(edges, edges + nb + 1)), out,
                        [&](BispecSetup &b) { return b.init(N, L, nb, edges); });
}

// ---- argument checks, stated once (no device call)
int bispec_check_grid(int n_grid) { return fourier_check_grid(n_grid, kFft3MaxN, "n_grid must be a power of two with 8 <= n_grid <= 1024"); }

int bispec_check_bins(double L, int nbins, const double *edges)
{
    if (nbins < 1 || nbins > kBispecMaxBins) return fail(BFGX_ERR_INVALID, "bispectrum needs 1 <= nbins <= %d", kBispecMaxBins);
    if (!(L > 0)) return fail(BFGX_ERR_INVALID, "bispectrum needs L > 0");
    for (int i = 0; i <= nbins; ++i) {
        if (!std::isfinite(edges[i]) || edges[i] < 0) return fail(BFGX_ERR_INVALID, "k_edges must be finite and non-negative");
        if (i && !(edges[i] > edges[i - 1])) return fail(BFGX_ERR_INVALID, "k_edges must be strictly ascending");
    }
    return BFGX_OK;
}

int bispec_check_triangles(int nbins, int ntri, const int32_t *tri)
{
    if (ntri < 1 || ntri > kBispecMaxTri) return fail(BFGX_ERR_INVALID, "bispectrum needs 1 <= ntri <= %d", kBispecMaxTri);
    for (int64_t i = 0; i < 3 * (int64_t)ntri; ++i)
        if (tri[i] < 0 || tri[i] >= nbins) return fail(BFGX_ERR_INVALID, "triangle %d: bin index %d outside [0, %d)", (int)(i / 3), (int)tri[i], nbins);
    return BFGX_OK;
}

// fields[i] = the inverse transform of spec [N][N][pitch] restricted to bin i (unit: of ones there), i < nb; scratch: one half spectrum
int bispec_fields(FftSetup &f, BispecSetup &bs, hipStream_t s, int N, int nb, const double2 *spec, int unit, double2 *scratch, double *fields)
{
    const int pitch = fft_pitch(N);
    const int64_t nspec = (int64_t)N * N * pitch, npts = (int64_t)N * N * N;
    for (int i = 0; i < nb; ++i) {
        hipLaunchKernelGGL(bispec_select_kernel, dim3(stream_grid(f.n_cu, nspec)), dim3(256), 0, s, spec, scratch, bs.dtab.as<uint8_t>(), N, pitch, i, unit);
        HIP_TRY(hipGetLastError());
        if (int rc = fft_axis0_store(f, s, N, N, scratch, pitch)) return rc;
        if (int rc = ifft_planes_conj(f, s, N, N, scratch, fields + (int64_t)i * npts, pitch)) return rc;
    }
    return BFGX_OK;
}

// layout of the work array of bfgx_bispectrum_device, in doubles: the spectrum, a scratch half spectrum, the nb fields, the partial sums
// of the triangle kernel, the packed terms
struct BispecWork {
    int64_t spec, scratch, fields, partials, ent, total;
    BispecWork(int N, int nb)
    {
        const int64_t half = 2 * (int64_t)N * N * fft_pitch(N), npts = (int64_t)N * N * N;
        spec = 0; scratch = half; fields = 2 * half;
        partials = fields + (int64_t)nb * npts;
        ent = partials + std::min<int64_t>(npts / kBispecChunk, kBispecMaxWgs) * kBispecThreads * kBispecMaxPerThread;
        total = ent + (kBispecMaxTri + kBispecMaxBins) / 2;
    }
};

// all terms of one sweep: tri_out[ntri] and diag_out[nb] = sums over the points of the fields' products / N^3
int bispec_sums(const FftSetup &f, hipStream_t s, int N, int nb, const double *fields, const uint32_t *ent_dev, int ntri, double *partials,
                double *tri_out, double *diag_out)
{
    const int64_t npts = (int64_t)N * N * N;
    const int ntot = ntri + nb;
    int tpt = kBispecMaxPerThread;                                   // the smallest instantiation that holds all terms
#define BFGX_TRI_PICK(T) if (tpt == kBispecMaxPerThread && (int64_t)T * kBispecThreads >= ntot) tpt = T;
    BFGX_BISPEC_TPT_LIST(BFGX_TRI_PICK)
#undef BFGX_TRI_PICK
    int G = 4;                                                       // (256 / G subsets of the chunk's 64 pairs of points)
    while (G < ntot && G < kBispecThreads) G <<= 1;
    const size_t lds = bispec_lds_bytes(nb);
    // persistent workgroups, each striding over the chunks: as many as the CUs hold at once -- by LDS, and by registers (the compiler's
    // report: 4 waves per SIMD up to 3 terms per thread, 3 up to 10, 2 up to 20, 1 above; at 3 terms per thread a fourth workgroup per
    // CU measured 5 % slower, 37.8 against 35.9 ms for two sweeps of 580 terms at N = 512) -- and as the partials of the work array
    // have room for
    const int by_regs = tpt <= 2 ? 4 : tpt <= 10 ? 3 : tpt <= 20 ? 2 : 1;
    const int per_cu = (int)std::min<size_t>((size_t)by_regs, std::max<size_t>(1, kCuLdsBytes / lds));
    const int64_t room = (int64_t)kBispecMaxWgs * kBispecMaxPerThread / tpt;
    const int nwg = (int)std::min<int64_t>(std::min<int64_t>(npts / kBispecChunk, room), (int64_t)f.n_cu * per_cu);
#define BFGX_TRI(T) case T: hipLaunchKernelGGL((bispec_triangle_kernel<T>), dim3((unsigned)nwg), dim3(kBispecThreads), lds, s, fields, npts, nb, ent_dev, ntot, G, partials); break;
    switch (tpt) { BFGX_BISPEC_TPT_LIST(BFGX_TRI) }
#undef BFGX_TRI
    HIP_TRY(hipGetLastError());
    const double *pc = partials;
    hipLaunchKernelGGL(bispec_finish_kernel, dim3((unsigned)ntot), dim3(256), 0, s, pc, nwg, tpt, ntot, G, ntri, 1.0 / (double)npts, tri_out, diag_out);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

}  // namespace

extern "C" {

int bfgx_fft_slab_axis0_device(int device, void *hip_stream, int32_t n_grid, int32_t ncols, double *work_dev, int32_t inverse)
{
    if (!work_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = bispec_check_grid(n_grid)) return rc;
    if (ncols < 1 || ncols > n_grid) return fail(BFGX_ERR_INVALID, "slab of %d columns: 1 <= ncols <= n_grid", ncols);
    if (int rc = fourier_check_aligned(work_dev, "work_dev")) return rc;
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    FftSetup *f = nullptr;
    if (int rc = fft_setup(device, n_grid, 1.0, 1, &f)) return rc;
    const int pitch = fft_pitch(n_grid);
    const int64_t n = (int64_t)n_grid * ncols * pitch;
    if (inverse) if (int rc = fft_conj(*f, s, (double2 *)work_dev, n)) return rc;
    if (int rc = fft_axis0_store(*f, s, n_grid, ncols, (double2 *)work_dev, pitch)) return rc;
    if (inverse) if (int rc = fft_conj(*f, s, (double2 *)work_dev, n)) return rc;
    return BFGX_OK;
}

int bfgx_ifft_slab_planes_device(int device, void *hip_stream, int32_t n_grid, int32_t planes, double *work_dev, double *map_out_dev)
{
    if (!work_dev || !map_out_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = bispec_check_grid(n_grid)) return rc;
    if (planes < 1 || planes > n_grid || ((int64_t)planes * n_grid) % 2) return fail(BFGX_ERR_INVALID, "slab of %d planes: 1 <= planes <= n_grid", planes);
    if (int rc = fourier_check_aligned(work_dev, "work_dev")) return rc;
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    FftSetup *f = nullptr;
    if (int rc = fft_setup(device, n_grid, 1.0, 1, &f)) return rc;
    const int pitch = fft_pitch(n_grid);
    if (int rc = fft_conj(*f, s, (double2 *)work_dev, (int64_t)planes * n_grid * pitch)) return rc;
    return ifft_planes_conj(*f, s, n_grid, planes, (double2 *)work_dev, map_out_dev, pitch);
}

int64_t bfgx_bispectrum_work_doubles(int32_t n_grid, int32_t nbins)
{
    if (!fourier_grid_ok(n_grid, kFft3MaxN) || nbins < 1 || nbins > kBispecMaxBins) return 0;
    return BispecWork(n_grid, nbins).total;
}

int bfgx_bispectrum_shell_fields_device(int device, void *hip_stream, int32_t n_grid, double L, int32_t nbins, const double *k_edges_host,
                                        const double *spec_dev, int32_t unit, double *scratch_spec_dev, double *fields_dev)
{
    if (!k_edges_host || !spec_dev || !scratch_spec_dev || !fields_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = bispec_check_grid(n_grid)) return rc;
    if (int rc = bispec_check_bins(L, nbins, k_edges_host)) return rc;
    if (int rc = fourier_check_aligned(spec_dev, "spec_dev")) return rc;
    if (int rc = fourier_check_aligned(scratch_spec_dev, "scratch_spec_dev")) return rc;
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    FftSetup *f = nullptr;
    BispecSetup *bs = nullptr;
    if (int rc = fft_setup(device, n_grid, 1.0, 1, &f)) return rc;
    if (int rc = bispec_setup(device, n_grid, L, nbins, k_edges_host, &bs)) return rc;
    return bispec_fields(*f, *bs, s, n_grid, nbins, (const double2 *)spec_dev, unit, (double2 *)scratch_spec_dev, fields_dev);
}

int bfgx_bispectrum_device(int device, void *hip_stream, int32_t n_grid, const double *map_dev, double L, int32_t nbins, const double *k_edges_host,
                           int32_t ntri, const int32_t *tri_host, double *work_dev, double *b_sum_dev, double *n_tri_dev, double *pk_sum_dev,
                           double *n_modes_dev)
{
    if (!map_dev || !k_edges_host || !tri_host || !work_dev || !b_sum_dev || !n_tri_dev || !pk_sum_dev || !n_modes_dev)
        return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = bispec_check_grid(n_grid)) return rc;
    if (int rc = bispec_check_bins(L, nbins, k_edges_host)) return rc;
    if (int rc = bispec_check_triangles(nbins, ntri, tri_host)) return rc;
    if (int rc = fourier_check_aligned(work_dev, "work_dev")) return rc;
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    FftSetup *f = nullptr;
    BispecSetup *bs = nullptr;
    if (int rc = fft_setup(device, n_grid, 1.0, 1, &f)) return rc;
    if (int rc = bispec_setup(device, n_grid, L, nbins, k_edges_host, &bs)) return rc;
    const int N = n_grid, pitch = fft_pitch(N);
    const BispecWork w(N, nbins);
    double2 *spec = (double2 *)(work_dev + w.spec), *scratch = (double2 *)(work_dev + w.scratch);
    double *fields = work_dev + w.fields, *partials = work_dev + w.partials;
    uint32_t *ent_dev = (uint32_t *)(work_dev + w.ent);
    // the full half spectrum, kept
    if (int rc = fft_planes(*f, s, N, N, map_dev, spec, pitch)) return rc;
    if (int rc = fft_axis0_store(*f, s, N, N, spec, pitch)) return rc;
    // sweep 1: the data fields I_i; sweep 2: the unit fields U_i in the same buffers
    if (int rc = bispec_fields(*f, *bs, s, N, nbins, spec, 0, scratch, fields)) return rc;
    // the terms: the triangles, then (i, i, ones) for the diagonal sums.  Uploaded here, behind work that keeps the device busy meanwhile
    // and before its first reader
    std::vector<uint32_t> ent((size_t)ntri + nbins);
    for (int t = 0; t < ntri; ++t) ent[t] = (uint32_t)tri_host[3 * t] | (uint32_t)tri_host[3 * t + 1] << 8 | (uint32_t)tri_host[3 * t + 2] << 16;
    for (int i = 0; i < nbins; ++i) ent[ntri + i] = (uint32_t)i | (uint32_t)i << 8 | (uint32_t)nbins << 16;
    if (int rc = upload_owned(s, ent_dev, std::move(ent))) return rc;
    if (int rc = bispec_sums(*f, s, N, nbins, fields, ent_dev, ntri, partials, b_sum_dev, pk_sum_dev)) return rc;
    if (int rc = bispec_fields(*f, *bs, s, N, nbins, spec, 1, scratch, fields)) return rc;
    return bispec_sums(*f, s, N, nbins, fields, ent_dev, ntri, partials, n_tri_dev, n_modes_dev);
}

int bfgx_bispectrum(int device, int32_t n_grid, const double *map, double L, int32_t nbins, const double *k_edges, int32_t ntri, const int32_t *tri,
                    double *b_sum, double *n_tri, double *pk_sum, double *n_modes)
{
    if (!map || !k_edges || !tri || !b_sum || !n_tri || !pk_sum || !n_modes) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = bispec_check_grid(n_grid)) return rc;
    if (int rc = bispec_check_bins(L, nbins, k_edges)) return rc;
    if (int rc = bispec_check_triangles(nbins, ntri, tri)) return rc;
    HostCall c(device);
    const size_t N = n_grid;
    const double *dm = c.in(map, N * N * N);
    double *dw = c.scratch<double>((size_t)bfgx_bispectrum_work_doubles(n_grid, nbins));       // (a box that does not fit fails here)
    double *db = c.out(b_sum, ntri), *dn = c.out(n_tri, ntri), *dp = c.out(pk_sum, nbins), *dc = c.out(n_modes, nbins);
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_bispectrum_device(device, nullptr, n_grid, dm, L, nbins, k_edges, ntri, tri, dw, db, dn, dp, dc)) return rc;
    return c.finish();
}

}  // extern "C"
