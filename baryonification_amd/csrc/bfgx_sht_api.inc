// bfgx_sht_api.inc -- C ABI of the spherical-harmonic transforms (bfgx_sht.hpp); included from bfgx_api.hip.
//
// Work array of bfgx_sht_work_doubles(nside, lmax, mmax) doubles, filled once by bfgx_sht_prepare_device and then reused by every
// transform of that shape (all offsets in doubles, 16-byte aligned):
//   twiddles of every power of two up to Mmax | Bluestein kernels B_k, k = 1..nside | their offsets (int64) | Ring[4 nside - 1] |
//   lambda_mm prefactors [mmax + 1] | F / G [mmax + 1][4 nside - 1] complex | one map of scratch (iterations of map2alm)
// The spin entries take a second array of bfgx_sht_spin_work_doubles(nside, lmax, mmax) doubles: the F / G of the second map.
namespace {

struct ShtLayout {
    int nside, lmax, mmax, nrings, kmax, Mmax;
    int64_t npix, o_tw, o_btab, o_boff, o_rings, o_pref, o_F, o_map, total;
};

int64_t even_up(int64_t n) { return (n + 1) & ~(int64_t)1; }

int sht_check(int32_t nside, int32_t lmax, int32_t mmax)
{
    if (nside < 1 || nside > sht::kMaxNside) return fail(BFGX_ERR_INVALID, "spherical-harmonic transforms support 1 <= nside <= %d (got %d)", sht::kMaxNside, nside);
    if (lmax < 0 || lmax > 32767) return fail(BFGX_ERR_INVALID, "lmax must be in [0, 32767] (got %d)", lmax);
    if (mmax < 0 || mmax > lmax) return fail(BFGX_ERR_INVALID, "mmax must be in [0, lmax] (got mmax %d, lmax %d)", mmax, lmax);
    return BFGX_OK;
}

ShtLayout sht_layout(int nside, int lmax, int mmax)
{
    ShtLayout L;
    L.nside = nside; L.lmax = lmax; L.mmax = mmax;
    L.nrings = 4 * nside - 1; L.kmax = nside; L.Mmax = sht::pow2_ge(2 * nside - 1);
    L.npix = 12 * (int64_t)nside * nside;
    int64_t bt = 0;
    for (int k = 1; k <= nside; ++k) bt += sht::pow2_ge(2 * k - 1);
    int64_t o = 0;
    L.o_tw = o;    o += even_up(2 * (int64_t)std::max(L.Mmax, 2));
    L.o_btab = o;  o += 2 * bt;
    L.o_boff = o;  o += even_up(nside + 1);
    L.o_rings = o; o += even_up((int64_t)L.nrings * (sizeof(sht::Ring) / sizeof(double)));
    L.o_pref = o;  o += even_up(mmax + 1);
    L.o_F = o;     o += 2 * (int64_t)(mmax + 1) * L.nrings;
    L.o_map = o;   o += even_up(L.npix);
    L.total = o;
    return L;
}

size_t sht_ring_lds(const ShtLayout &L) { return sizeof(double2) * ((size_t)L.Mmax + 2 * (size_t)L.kmax); }

int sht_set_lds(const ShtLayout &L)
{
    const int lds = (int)sht_ring_lds(L);
    HIP_TRY(hipFuncSetAttribute((const void *)sht::sht_ring_analysis_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    HIP_TRY(hipFuncSetAttribute((const void *)sht::sht_ring_synthesis_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    HIP_TRY(hipFuncSetAttribute((const void *)sht::sht_bluestein_table_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(sizeof(double2) * L.Mmax)));
    return BFGX_OK;
}

struct ShtPtrs {
    const double2 *tw, *btab;
    const sht::Ring *rings;
    const double *pref;
    double2 *F;
    double *map;
};

ShtPtrs sht_ptrs(const ShtLayout &L, double *work)
{
    ShtPtrs p;
    p.tw = reinterpret_cast<const double2 *>(work + L.o_tw);
    p.btab = reinterpret_cast<const double2 *>(work + L.o_btab);
    p.rings = reinterpret_cast<const sht::Ring *>(work + L.o_rings);
    p.pref = work + L.o_pref;
    p.F = reinterpret_cast<double2 *>(work + L.o_F);
    p.map = work + L.o_map;
    return p;
}

// a work array of the caller's, on the device
int sht_work_check(const void *work, const char *name)
{
    if (!work) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (reinterpret_cast<uintptr_t>(work) & 15) return fail(BFGX_ERR_INVALID, "%s must be 16-byte aligned (complex values)", name);
    return BFGX_OK;
}

// The prologue of the _device entries, after their argument checks.  First half (all that bfgx_sht_prepare_device needs): the work array,
// the device, the layout ...
int sht_begin(int device, int32_t nside, int32_t lmax, int32_t mmax, const void *work, ShtLayout &L)
{
    if (int rc = sht_work_check(work, "work_dev")) return rc;
    if (int rc = select_device(device)) return rc;
    L = sht_layout(nside, lmax, mmax);
    return BFGX_OK;
}

// ... and for a transform also the LDS limit of the ring kernels and the pointers into the work array
int sht_begin(int device, int32_t nside, int32_t lmax, int32_t mmax, double *work, ShtLayout &L, ShtPtrs &p)
{
    if (int rc = sht_begin(device, nside, lmax, mmax, work, L)) return rc;
    if (int rc = sht_set_lds(L)) return rc;
    p = sht_ptrs(L, work);
    return BFGX_OK;
}

// the argument checks of each operation, shared by its host entry and its _device entry
// (map2alm, anafast and, with iter = 0, alm2map: `in` and `out` are the map and the alm, either way round)
int sht_transform_check(int32_t nside, int32_t lmax, int32_t mmax, int32_t iter, const void *in, const void *out)
{
    if (!in || !out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (iter < 0) return fail(BFGX_ERR_INVALID, "iter must be >= 0 (got %d)", iter);
    return sht_check(nside, lmax, mmax);
}

int sht_alm2cl_check(int32_t lmax, int32_t mmax, int32_t lmax_out, const void *alm1, const void *cl)
{
    if (!alm1 || !cl) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (lmax < 0 || mmax < 0 || mmax > lmax || lmax_out < 0) return fail(BFGX_ERR_INVALID, "alm2cl needs 0 <= mmax <= lmax, lmax_out >= 0");
    return BFGX_OK;
}

int sht_almxfl_check(int32_t lmax, int32_t mmax, int64_t nfl, const void *fl, const void *in, const void *out)
{
    if (!fl || !in || !out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (lmax < 0 || lmax > 32767 || mmax < 0 || mmax > lmax) return fail(BFGX_ERR_INVALID, "almxfl needs 0 <= mmax <= lmax <= 32767 (got mmax %d, lmax %d)", mmax, lmax);
    if (nfl < 0) return fail(BFGX_ERR_INVALID, "nfl must be >= 0 (got %lld)", (long long)nfl);
    return BFGX_OK;
}

// alm = A(map) (accumulate: alm += A(map))
int sht_analysis(const ShtLayout &L, const ShtPtrs &p, hipStream_t s, const double *map, double2 *alm, int accumulate)
{
    const double norm = 4.0 * M_PI / (double)L.npix;
    hipLaunchKernelGGL(sht::sht_ring_analysis_kernel, dim3(L.nrings), dim3(sht::kRingThreads), sht_ring_lds(L), s,
                       map, p.rings, L.nrings, L.mmax, norm, p.tw, p.btab, p.F);
    hipLaunchKernelGGL(sht::sht_legendre_analysis_kernel, dim3(L.mmax + 1), dim3(sht::kLegThreads), 0, s,
                       (const double2 *)p.F, p.rings, L.nside, L.lmax, p.pref, accumulate, alm);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

int sht_synthesis(const ShtLayout &L, const ShtPtrs &p, hipStream_t s, const double2 *alm, double *map)
{
    hipLaunchKernelGGL(sht::sht_legendre_synthesis_kernel, dim3(L.mmax + 1), dim3(sht::kLegThreads), 0, s,
                       alm, p.rings, L.nside, L.lmax, p.pref, p.F);
    hipLaunchKernelGGL(sht::sht_ring_synthesis_kernel, dim3(L.nrings), dim3(sht::kRingThreads), sht_ring_lds(L), s,
                       (const double2 *)p.F, p.rings, L.nrings, L.mmax, p.tw, p.btab, map);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

int sht_map2alm(const ShtLayout &L, const ShtPtrs &p, hipStream_t s, const double *map, double2 *alm, int iter)
{
    if (int rc = sht_analysis(L, p, s, map, alm, 0)) return rc;
    for (int it = 0; it < iter; ++it) {
        if (int rc = sht_synthesis(L, p, s, alm, p.map)) return rc;
        const unsigned nb = (unsigned)std::min<int64_t>((L.npix + 255) / 256, 4096);
        hipLaunchKernelGGL(sht::sht_residual_kernel, dim3(nb), dim3(256), 0, s, map, p.map, L.npix);
        if (int rc = sht_analysis(L, p, s, p.map, alm, 1)) return rc;
    }
    return BFGX_OK;
}

int sht_alm2cl(hipStream_t s, int lmax, int mmax, int lmax_out, const double2 *a, const double2 *b, double *cl)
{
    hipLaunchKernelGGL(sht::sht_alm2cl_kernel, dim3((unsigned)((lmax_out + 256) / 256)), dim3(256), 0, s, a, b, lmax, mmax, lmax_out, cl);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

int64_t sht_alm_size(int lmax, int mmax) { return (int64_t)(mmax + 1) * (2 * (int64_t)lmax + 2 - mmax) / 2; }

// spin transforms: a second F buffer (F of map1), [mmax + 1][4 nside - 1] complex, outside the spin-0 work array
int64_t sht_spin_work(const ShtLayout &L) { return 2 * (int64_t)(L.mmax + 1) * L.nrings; }

// (both spin transforms: `in` and `out` are the maps and the alms, either way round)
int sht_spin_check(int32_t nside, int32_t lmax, int32_t mmax, int32_t spin, const void *in, const void *out)
{
    if (!in || !out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = sht_check(nside, lmax, mmax)) return rc;
    if (spin < 1) return fail(BFGX_ERR_INVALID, "spin must be >= 1 (got %d; spin 0 is bfgx_sht_map2alm / bfgx_sht_alm2map)", spin);
    if (spin > lmax) return fail(BFGX_ERR_INVALID, "spin must be <= lmax (got spin %d, lmax %d)", spin, lmax);
    return BFGX_OK;
}

// [G | C] = A_s(map0, map1): maps = map0 | map1 (npix each), alms = G | C (alm size each)
int sht_spin_analysis(const ShtLayout &L, const ShtPtrs &p, double2 *F1, hipStream_t s, int spin, const double *maps, double2 *alms)
{
    const double norm = 4.0 * M_PI / (double)L.npix;
    hipLaunchKernelGGL(sht::sht_ring_analysis_kernel, dim3(L.nrings), dim3(sht::kRingThreads), sht_ring_lds(L), s,
                       maps, p.rings, L.nrings, L.mmax, norm, p.tw, p.btab, p.F);
    hipLaunchKernelGGL(sht::sht_ring_analysis_kernel, dim3(L.nrings), dim3(sht::kRingThreads), sht_ring_lds(L), s,
                       maps + L.npix, p.rings, L.nrings, L.mmax, norm, p.tw, p.btab, F1);
    hipLaunchKernelGGL(sht::sht_spin_legendre_analysis_kernel, dim3(L.mmax + 1), dim3(sht::kLegThreads), 0, s,
                       (const double2 *)p.F, (const double2 *)F1, p.rings, L.nside, L.lmax, spin, p.pref, alms,
                       alms + sht_alm_size(L.lmax, L.mmax));
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

int sht_spin_synthesis(const ShtLayout &L, const ShtPtrs &p, double2 *F1, hipStream_t s, int spin, const double2 *alms, double *maps)
{
    hipLaunchKernelGGL(sht::sht_spin_legendre_synthesis_kernel, dim3(L.mmax + 1), dim3(sht::kLegThreads), 0, s,
                       alms, alms + sht_alm_size(L.lmax, L.mmax), p.rings, L.nside, L.lmax, spin, p.pref, p.F, F1);
    hipLaunchKernelGGL(sht::sht_ring_synthesis_kernel, dim3(L.nrings), dim3(sht::kRingThreads), sht_ring_lds(L), s,
                       (const double2 *)p.F, p.rings, L.nrings, L.mmax, p.tw, p.btab, maps);
    hipLaunchKernelGGL(sht::sht_ring_synthesis_kernel, dim3(L.nrings), dim3(sht::kRingThreads), sht_ring_lds(L), s,
                       (const double2 *)F1, p.rings, L.nrings, L.mmax, p.tw, p.btab, maps + L.npix);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

}  // namespace

extern "C" {

int64_t bfgx_sht_work_doubles(int32_t nside, int32_t lmax, int32_t mmax)
{
    if (sht_check(nside, lmax, mmax)) return -1;
    return sht_layout(nside, lmax, mmax).total;
}

int bfgx_sht_prepare_device(int device, void *hip_stream, int32_t nside, int32_t lmax, int32_t mmax, double *work_dev)
{
    if (int rc = sht_check(nside, lmax, mmax)) return rc;
    ShtLayout L;
    if (int rc = sht_begin(device, nside, lmax, mmax, work_dev, L)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    // twiddles e^{-2 pi i j / M}, j < M/2, of every power of two M <= Mmax
    std::vector<double> tw(L.o_btab - L.o_tw, 0.0);
    for (int M = 2; M <= L.Mmax; M <<= 1)
        for (int j = 0; j < M / 2; ++j) {
            const long double a = -2.0L * 3.14159265358979323846264338327950288L * j / M;
            tw[2 * (sht::tw_offset(M) + j)] = (double)cosl(a);
            tw[2 * (sht::tw_offset(M) + j) + 1] = (double)sinl(a);
        }
    std::vector<int64_t> boff(nside + 1, 0);
    for (int k = 1, o = 0; k <= nside; ++k) { boff[k] = o; o += sht::pow2_ge(2 * k - 1); }
    std::vector<sht::Ring> rings(L.nrings);
    for (int i = 1; i <= L.nrings; ++i) {
        sht::Ring &R = rings[i - 1];
        const int is = 4 * nside - i;                              // ring number from the south pole
        long double z, omz;                                         // z and 1 - |z| (exact in the caps)
        if (i < nside || is < nside) {
            const int j = i < nside ? i : is;
            omz = (long double)j * j * 4.0L / (long double)L.npix;
            z = i < nside ? 1.0L - omz : omz - 1.0L;
            R.nphi = 4 * j;
            R.pix0 = i < nside ? 2 * (int64_t)i * (i - 1) : L.npix - 2 * (int64_t)is * (is + 1);
            R.shifted = 1;
        } else {
            z = (long double)(2 * nside - i) * 2.0L / (3.0L * nside);
            omz = 1.0L - fabsl(z);
            R.nphi = 4 * nside;
            R.pix0 = 2 * (int64_t)nside * (nside - 1) + (int64_t)(i - nside) * 4 * nside;
            R.shifted = ((i - nside) % 2) == 0;
        }
        R.z = (double)z;
        R.s = (double)sqrtl(omz * (2.0L - omz));
        R.boff = boff[R.nphi / 4];
    }
    // lambda_mm = (-1)^m sqrt((2m + 1) / (4 pi) prod_{k <= m} (2k - 1) / (2k)) sin^m(theta): the prefactor never underflows
    std::vector<double> pref(mmax + 1);
    long double prod = 1.0L;
    for (int m = 0; m <= mmax; ++m) {
        if (m) prod *= (long double)(2 * m - 1) / (long double)(2 * m);
        const long double v = sqrtl((2.0L * m + 1.0L) / (4.0L * 3.14159265358979323846264338327950288L) * prod);
        pref[m] = (double)((m & 1) ? -v : v);
    }
    HIP_TRY(hipMemcpyAsync(work_dev + L.o_tw, tw.data(), sizeof(double) * tw.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(work_dev + L.o_boff, boff.data(), sizeof(int64_t) * boff.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(work_dev + L.o_rings, rings.data(), sizeof(sht::Ring) * rings.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(work_dev + L.o_pref, pref.data(), sizeof(double) * pref.size(), hipMemcpyHostToDevice, s));
    if (int rc = sht_set_lds(L)) return rc;
    hipLaunchKernelGGL(sht::sht_bluestein_table_kernel, dim3(nside), dim3(sht::kRingThreads), sizeof(double2) * L.Mmax, s,
                       reinterpret_cast<const double2 *>(work_dev + L.o_tw), reinterpret_cast<const int64_t *>(work_dev + L.o_boff),
                       reinterpret_cast<double2 *>(work_dev + L.o_btab));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));                               // (the host tables go out of scope)
    return BFGX_OK;
}

int bfgx_sht_map2alm_device(int device, void *hip_stream, int32_t nside, int32_t lmax, int32_t mmax, int32_t iter, const double *map_dev,
                            double *alm_dev, double *work_dev)
{
    if (int rc = sht_transform_check(nside, lmax, mmax, iter, map_dev, alm_dev)) return rc;
    ShtLayout L; ShtPtrs p;
    if (int rc = sht_begin(device, nside, lmax, mmax, work_dev, L, p)) return rc;
    return sht_map2alm(L, p, (hipStream_t)hip_stream, map_dev, reinterpret_cast<double2 *>(alm_dev), iter);
}

int bfgx_sht_alm2map_device(int device, void *hip_stream, int32_t nside, int32_t lmax, int32_t mmax, const double *alm_dev, double *map_dev,
                            double *work_dev)
{
    if (int rc = sht_transform_check(nside, lmax, mmax, 0, alm_dev, map_dev)) return rc;
    ShtLayout L; ShtPtrs p;
    if (int rc = sht_begin(device, nside, lmax, mmax, work_dev, L, p)) return rc;
    return sht_synthesis(L, p, (hipStream_t)hip_stream, reinterpret_cast<const double2 *>(alm_dev), map_dev);
}

int bfgx_sht_alm2cl_device(int device, void *hip_stream, int32_t lmax, int32_t mmax, int32_t lmax_out, const double *alm1_dev,
                           const double *alm2_dev, double *cl_dev)
{
    if (int rc = sht_alm2cl_check(lmax, mmax, lmax_out, alm1_dev, cl_dev)) return rc;
    if (int rc = select_device(device)) return rc;
    const double2 *a = reinterpret_cast<const double2 *>(alm1_dev), *b = alm2_dev ? reinterpret_cast<const double2 *>(alm2_dev) : a;
    return sht_alm2cl((hipStream_t)hip_stream, lmax, mmax, lmax_out, a, b, cl_dev);
}

int bfgx_sht_almxfl_device(int device, void *hip_stream, int32_t lmax, int32_t mmax, int64_t nfl, const double *fl_dev, const double *alm_in_dev,
                           double *alm_out_dev)
{
    if (int rc = sht_almxfl_check(lmax, mmax, nfl, fl_dev, alm_in_dev, alm_out_dev)) return rc;
    if (int rc = select_device(device)) return rc;
    hipLaunchKernelGGL(sht::sht_almxfl_kernel, dim3((unsigned)(lmax / 256 + 1), (unsigned)(mmax + 1)), dim3(256), 0, (hipStream_t)hip_stream,
                       reinterpret_cast<const double2 *>(alm_in_dev), reinterpret_cast<double2 *>(alm_out_dev), lmax,
                       (int)std::min<int64_t>(nfl, (int64_t)lmax + 1), fl_dev);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

// host entries: numpy in, numpy out (PCIe included); alm are complex128 in healpy order, counted here in doubles
int bfgx_sht_almxfl(int device, int32_t lmax, int32_t mmax, int64_t nfl, const double *fl, const double *alm_in, double *alm_out)
{
    if (int rc = sht_almxfl_check(lmax, mmax, nfl, fl, alm_in, alm_out)) return rc;
    HostCall c(device);
    const int64_t na = sht_alm_size(lmax, mmax), nf = std::min<int64_t>(nfl, (int64_t)lmax + 1);
    const double *df = c.in(fl, nf);
    double *da = c.inout(alm_in, alm_out, 2 * na);                                   // multiplied in place on the device
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_sht_almxfl_device(device, nullptr, lmax, mmax, nf, df, da, da)) return rc;
    return c.finish();
}

int bfgx_sht_map2alm(int device, int32_t nside, int32_t lmax, int32_t mmax, int32_t iter, const double *map, double *alm)
{
    if (int rc = sht_transform_check(nside, lmax, mmax, iter, map, alm)) return rc;
    HostCall c(device);
    const ShtLayout L = sht_layout(nside, lmax, mmax);
    double *dw = c.scratch<double>(L.total);
    const double *dm = c.in(map, L.npix);
    double *da = c.out(alm, 2 * sht_alm_size(lmax, mmax));
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_sht_prepare_device(device, nullptr, nside, lmax, mmax, dw)) return rc;
    if (int rc = bfgx_sht_map2alm_device(device, nullptr, nside, lmax, mmax, iter, dm, da, dw)) return rc;
    return c.finish();
}

int bfgx_sht_alm2map(int device, int32_t nside, int32_t lmax, int32_t mmax, const double *alm, double *map)
{
    if (int rc = sht_transform_check(nside, lmax, mmax, 0, alm, map)) return rc;
    HostCall c(device);
    const ShtLayout L = sht_layout(nside, lmax, mmax);
    double *dw = c.scratch<double>(L.total), *dm = c.out(map, L.npix);
    const double *da = c.in(alm, 2 * sht_alm_size(lmax, mmax));
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_sht_prepare_device(device, nullptr, nside, lmax, mmax, dw)) return rc;
    if (int rc = bfgx_sht_alm2map_device(device, nullptr, nside, lmax, mmax, da, dm, dw)) return rc;
    return c.finish();
}

int bfgx_sht_alm2cl(int device, int32_t lmax, int32_t mmax, int32_t lmax_out, const double *alm1, const double *alm2, double *cl)
{
    if (int rc = sht_alm2cl_check(lmax, mmax, lmax_out, alm1, cl)) return rc;
    HostCall c(device);
    const int64_t na = sht_alm_size(lmax, mmax);
    const double *d1 = c.in(alm1, 2 * na), *d2 = alm2 ? c.in(alm2, 2 * na) : nullptr;
    double *dc = c.out(cl, lmax_out + 1);
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_sht_alm2cl_device(device, nullptr, lmax, mmax, lmax_out, d1, d2, dc)) return rc;
    return c.finish();
}

// anafast: map2alm of one or two maps, alm2cl on the device; only cl (and the alm when alm1_out / alm2_out are given) come back
int bfgx_sht_anafast(int device, int32_t nside, int32_t lmax, int32_t mmax, int32_t iter, const double *map1, const double *map2,
                     double *cl, double *alm1_out, double *alm2_out)
{
    if (int rc = sht_transform_check(nside, lmax, mmax, iter, map1, cl)) return rc;
    HostCall c(device);
    const ShtLayout L = sht_layout(nside, lmax, mmax);
    const int64_t na = sht_alm_size(lmax, mmax);
    double *dw = c.scratch<double>(L.total);
    double *dm = const_cast<double *>(c.in(map1, L.npix));                           // (filled a second time below)
    double *da1 = c.out(alm1_out, 2 * na), *da2 = map2 ? c.out(alm2_out, 2 * na) : nullptr, *dc = c.out(cl, lmax + 1);
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_sht_prepare_device(device, nullptr, nside, lmax, mmax, dw)) return rc;
    if (int rc = bfgx_sht_map2alm_device(device, nullptr, nside, lmax, mmax, iter, dm, da1, dw)) return rc;
    if (map2) {
        // the one copy the scaffold does not make: map2 takes the place of map1 in the same buffer once the first transform has been queued
        // (the blocking copy waits for it)
        HIP_TRY(hipMemcpy(dm, map2, sizeof(double) * L.npix, hipMemcpyHostToDevice));
        if (int rc = bfgx_sht_map2alm_device(device, nullptr, nside, lmax, mmax, iter, dm, da2, dw)) return rc;
    }
    if (int rc = bfgx_sht_alm2cl_device(device, nullptr, lmax, mmax, lmax, da1, da2, dc)) return rc;
    return c.finish();
}


// spin-s transforms of a pair of maps (healpy map2alm_spin / alm2map_spin); maps = map0 | map1, alms = G | C
int64_t bfgx_sht_spin_work_doubles(int32_t nside, int32_t lmax, int32_t mmax)
{
    if (sht_check(nside, lmax, mmax)) return -1;
    return sht_spin_work(sht_layout(nside, lmax, mmax));
}

int bfgx_sht_map2alm_spin_device(int device, void *hip_stream, int32_t nside, int32_t lmax, int32_t mmax, int32_t spin, const double *maps_dev,
                                 double *alms_dev, double *work_dev, double *spin_work_dev)
{
    if (int rc = sht_work_check(spin_work_dev, "spin_work_dev")) return rc;
    if (int rc = sht_spin_check(nside, lmax, mmax, spin, maps_dev, alms_dev)) return rc;
    ShtLayout L; ShtPtrs p;
    if (int rc = sht_begin(device, nside, lmax, mmax, work_dev, L, p)) return rc;
    return sht_spin_analysis(L, p, reinterpret_cast<double2 *>(spin_work_dev), (hipStream_t)hip_stream, spin, maps_dev,
                             reinterpret_cast<double2 *>(alms_dev));
}

int bfgx_sht_alm2map_spin_device(int device, void *hip_stream, int32_t nside, int32_t lmax, int32_t mmax, int32_t spin, const double *alms_dev,
                                 double *maps_dev, double *work_dev, double *spin_work_dev)
{
    if (int rc = sht_work_check(spin_work_dev, "spin_work_dev")) return rc;
    if (int rc = sht_spin_check(nside, lmax, mmax, spin, alms_dev, maps_dev)) return rc;
    ShtLayout L; ShtPtrs p;
    if (int rc = sht_begin(device, nside, lmax, mmax, work_dev, L, p)) return rc;
    return sht_spin_synthesis(L, p, reinterpret_cast<double2 *>(spin_work_dev), (hipStream_t)hip_stream, spin,
                              reinterpret_cast<const double2 *>(alms_dev), maps_dev);
}

int bfgx_sht_map2alm_spin(int device, int32_t nside, int32_t lmax, int32_t mmax, int32_t spin, const double *maps, double *alms)
{
    if (int rc = sht_spin_check(nside, lmax, mmax, spin, maps, alms)) return rc;
    HostCall c(device);
    const ShtLayout L = sht_layout(nside, lmax, mmax);
    double *dw = c.scratch<double>(L.total), *ds = c.scratch<double>(sht_spin_work(L));
    const double *dm = c.in(maps, 2 * L.npix);
    double *da = c.out(alms, 4 * sht_alm_size(lmax, mmax));
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_sht_prepare_device(device, nullptr, nside, lmax, mmax, dw)) return rc;
    if (int rc = bfgx_sht_map2alm_spin_device(device, nullptr, nside, lmax, mmax, spin, dm, da, dw, ds)) return rc;
    return c.finish();
}

int bfgx_sht_alm2map_spin(int device, int32_t nside, int32_t lmax, int32_t mmax, int32_t spin, const double *alms, double *maps)
{
    if (int rc = sht_spin_check(nside, lmax, mmax, spin, alms, maps)) return rc;
    HostCall c(device);
    const ShtLayout L = sht_layout(nside, lmax, mmax);
    double *dw = c.scratch<double>(L.total), *ds = c.scratch<double>(sht_spin_work(L)), *dm = c.out(maps, 2 * L.npix);
    const double *da = c.in(alms, 4 * sht_alm_size(lmax, mmax));
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_sht_prepare_device(device, nullptr, nside, lmax, mmax, dw)) return rc;
    if (int rc = bfgx_sht_alm2map_spin_device(device, nullptr, nside, lmax, mmax, spin, da, dm, dw, ds)) return rc;
    return c.finish();
}

}  // extern "C"
