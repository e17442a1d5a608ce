// bfgx_hpx_api.inc -- C ABI of the HEALPix pixel functions (bfgx_hpx.hpp); included from bfgx_api.hip.
// Every argument is checked before any device call; the host entries also check index and angle ranges on the host arrays.
namespace {

constexpr int64_t kHpxMaxNside = 8192;

bool hpx_pow2(int64_t v) { return v >= 1 && (v & (v - 1)) == 0; }

int hpx_check_nside(int64_t nside, bool need_pow2, const char *what)
{
    if (nside < 1 || nside > kHpxMaxNside || (need_pow2 && !hpx_pow2(nside)))
        return fail(BFGX_ERR_INVALID, "%s must be %sin [1, %lld] (got %lld)", what, need_pow2 ? "a power of two " : "", (long long)kHpxMaxNside,
                    (long long)nside);
    return BFGX_OK;
}

// dtype codes: 0 = float32, 1 = float64
int hpx_check_dtype(int32_t dt, const char *what)
{
    if (dt != 0 && dt != 1) return fail(BFGX_ERR_INVALID, "%s must be 0 (float32) or 1 (float64) (got %d)", what, dt);
    return BFGX_OK;
}

size_t hpx_dsize(int32_t dt) { return dt ? sizeof(double) : sizeof(float); }

int hpx_ud_grade_check(int64_t nside_in, int64_t nside_out, int64_t nmaps, int32_t dtype_in, int32_t dtype_out, double ratio, const void *in,
                       const void *out)
{
    if (!in || !out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = hpx_check_nside(nside_in, true, "nside_in")) return rc;
    if (int rc = hpx_check_nside(nside_out, true, "nside_out")) return rc;
    if (nmaps < 1 || nmaps > 65535) return fail(BFGX_ERR_INVALID, "nmaps must be in [1, 65535] (got %lld)", (long long)nmaps);
    if (int rc = hpx_check_dtype(dtype_in, "dtype_in")) return rc;
    if (int rc = hpx_check_dtype(dtype_out, "dtype_out")) return rc;
    if (!std::isfinite(ratio)) return fail(BFGX_ERR_INVALID, "ratio must be finite");
    return BFGX_OK;
}

template <typename TI, typename TO>
void hpx_ud_grade_launch(const hpx::Degrade &d, int64_t nmaps, hipStream_t s, const void *in, void *out)
{
    if (d.nside_out < d.nside_in) {
        const unsigned nb = (unsigned)((d.npix_out + (hpx::kThreads >> d.lg) - 1) / (hpx::kThreads >> d.lg));
        hipLaunchKernelGGL((hpx::hpx_degrade_kernel<TI, TO>), dim3(nb, (unsigned)nmaps), dim3(hpx::kThreads), 0, s, d, (const TI *)in, (TO *)out);
    } else {
        const unsigned nb = (unsigned)std::min<int64_t>((d.npix_out + hpx::kThreads - 1) / hpx::kThreads, 1 << 20);
        hipLaunchKernelGGL((hpx::hpx_upgrade_kernel<TI, TO>), dim3(nb, (unsigned)nmaps), dim3(hpx::kThreads), 0, s, d, (const TI *)in, (TO *)out);
    }
}

int hpx_ud_grade_enqueue(hipStream_t s, int64_t nside_in, int64_t nside_out, int64_t nmaps, int32_t nest_in, int32_t nest_out, int32_t pess,
                         double ratio, int32_t dtype_in, int32_t dtype_out, const void *in, void *out)
{
    hpx::Degrade d;
    d.nside_in = nside_in; d.nside_out = nside_out;
    d.npix_in = 12 * nside_in * nside_in; d.npix_out = 12 * nside_out * nside_out;
    d.order_in = hpx::ilog2(nside_in); d.order_out = hpx::ilog2(nside_out);
    d.lr = d.order_in >= d.order_out ? d.order_in - d.order_out : d.order_out - d.order_in;
    d.nest_in = nest_in ? 1 : 0; d.nest_out = nest_out ? 1 : 0; d.pess = pess ? 1 : 0;
    d.lg = std::min(2 * d.lr, 8);                                      // G = min(rat2, 256) lanes per output pixel
    d.ratio = ratio;
    if (dtype_in && dtype_out) hpx_ud_grade_launch<double, double>(d, nmaps, s, in, out);
    else if (dtype_in) hpx_ud_grade_launch<double, float>(d, nmaps, s, in, out);
    else if (dtype_out) hpx_ud_grade_launch<float, double>(d, nmaps, s, in, out);
    else hpx_ud_grade_launch<float, float>(d, nmaps, s, in, out);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

int hpx_interp_check(int64_t nside, int32_t nest, int64_t n)
{
    if (int rc = hpx_check_nside(nside, nest != 0, "nside")) return rc;
    if (n < 0) return fail(BFGX_ERR_INVALID, "n must be >= 0 (got %lld)", (long long)n);
    return BFGX_OK;
}

// the argument checks of each operation, shared by its host entry and its _device entry (with hpx_ud_grade_check above)
int hpx_interp_weights_check(int64_t nside, int32_t nest, int64_t n, const void *theta, const void *phi, const void *ipix, const void *pix,
                             const void *w)
{
    if (!pix || !w || (ipix ? (theta || phi) : (!theta || !phi)))
        return fail(BFGX_ERR_INVALID, "NULL argument (give theta and phi, or ipix alone)");
    return hpx_interp_check(nside, nest, n);
}

int hpx_interp_val_check(int64_t nside, int32_t nest, int64_t nmaps, int32_t dtype, const void *maps, int64_t n, const void *theta,
                         const void *phi, const void *out)
{
    if (!maps || !theta || !phi || !out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = hpx_interp_check(nside, nest, n)) return rc;
    if (nmaps < 1) return fail(BFGX_ERR_INVALID, "nmaps must be >= 1 (got %lld)", (long long)nmaps);
    return hpx_check_dtype(dtype, "dtype");
}

int hpx_neighbours_check(int64_t nside, int32_t nest, int64_t n, const void *ipix, const void *out)
{
    if (!ipix || !out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = hpx_interp_check(nside, nest, n)) return rc;
    if (n > (INT64_MAX >> 4)) return fail(BFGX_ERR_INVALID, "n is too large (%lld)", (long long)n);
    return BFGX_OK;
}

int hpx_scatter_add_check(int64_t npix, int64_t n, const void *hmap, const void *vals, const void *pix, const void *w)
{
    if (!hmap || !vals || !pix || !w) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (npix < 1 || n < 0) return fail(BFGX_ERR_INVALID, "npix must be >= 1 and n >= 0 (got npix %lld, n %lld)", (long long)npix, (long long)n);
    if (n > (INT64_MAX >> 3)) return fail(BFGX_ERR_INVALID, "n is too large (%lld)", (long long)n);
    return BFGX_OK;
}

// checks that read host arrays: the host entries only.  Pixel numbers in [0, npix)
int hpx_check_pixels(int64_t n, const int64_t *ipix, int64_t npix)
{
    for (int64_t i = 0; i < n; ++i)
        if (ipix[i] < 0 || ipix[i] >= npix) return fail(BFGX_ERR_INVALID, "ipix[%lld] = %lld is outside [0, %lld)", (long long)i, (long long)ipix[i], (long long)npix);
    return BFGX_OK;
}

// scatter_add's indices (4 per entry) in [-npix, npix)
int hpx_check_scatter_indices(int64_t n, const int64_t *pix, int64_t npix)
{
    for (int64_t e = 0; e < 4 * n; ++e)
        if (pix[e] < -npix || pix[e] >= npix)
            return fail(BFGX_ERR_INVALID, "index %lld (entry %lld) is outside [-%lld, %lld)", (long long)pix[e], (long long)e, (long long)npix,
                        (long long)npix);
    return BFGX_OK;
}

// theta in [0, pi], phi finite
int hpx_check_angles(int64_t n, const double *theta, const double *phi)
{
    for (int64_t i = 0; i < n; ++i) {
        if (!(theta[i] >= 0.0 && theta[i] <= M_PI)) return fail(BFGX_ERR_INVALID, "theta[%lld] = %g is outside [0, pi]", (long long)i, theta[i]);
        if (!std::isfinite(phi[i])) return fail(BFGX_ERR_INVALID, "phi[%lld] is not finite", (long long)i);
    }
    return BFGX_OK;
}

hpx::Interp hpx_interp_args(int64_t nside, int32_t nest, int64_t n)
{
    hpx::Interp a;
    a.h = make_hpx(nside);
    a.order = hpx::ilog2(nside);
    a.nest = nest ? 1 : 0;
    a.n = n;
    return a;
}

unsigned hpx_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + hpx::kThreads - 1) / hpx::kThreads, 1 << 20)); }

}  // namespace

extern "C" {

int bfgx_hpx_ud_grade_device(int device, void *hip_stream, int64_t nside_in, int64_t nside_out, int64_t nmaps, int32_t nest_in,
                             int32_t nest_out, int32_t pess, double ratio, int32_t dtype_in, int32_t dtype_out, const void *map_in_dev,
                             void *map_out_dev)
{
    if (int rc = hpx_ud_grade_check(nside_in, nside_out, nmaps, dtype_in, dtype_out, ratio, map_in_dev, map_out_dev)) return rc;
    if (int rc = select_device(device)) return rc;
    return hpx_ud_grade_enqueue((hipStream_t)hip_stream, nside_in, nside_out, nmaps, nest_in, nest_out, pess, ratio, dtype_in, dtype_out,
                                map_in_dev, map_out_dev);
}

int bfgx_hpx_ud_grade(int device, int64_t nside_in, int64_t nside_out, int64_t nmaps, int32_t nest_in, int32_t nest_out, int32_t pess,
                      double ratio, int32_t dtype_in, int32_t dtype_out, const void *map_in, void *map_out)
{
    if (int rc = hpx_ud_grade_check(nside_in, nside_out, nmaps, dtype_in, dtype_out, ratio, map_in, map_out)) return rc;
    HostCall c(device);
    // (maps of either dtype: counted in bytes)
    const char *di = c.in((const char *)map_in, hpx_dsize(dtype_in) * (size_t)nmaps * 12 * nside_in * nside_in);
    char *dout = c.out((char *)map_out, hpx_dsize(dtype_out) * (size_t)nmaps * 12 * nside_out * nside_out);
    if (int rc = c.ready()) return rc;
    if (int rc = hpx_ud_grade_enqueue(nullptr, nside_in, nside_out, nmaps, nest_in, nest_out, pess, ratio, dtype_in, dtype_out, di, dout)) return rc;
    return c.finish();
}

int bfgx_hpx_interp_weights_device(int device, void *hip_stream, int64_t nside, int32_t nest, int64_t n, const double *theta_dev,
                                   const double *phi_dev, const int64_t *ipix_dev, int64_t *pix_dev, double *w_dev)
{
    if (int rc = hpx_interp_weights_check(nside, nest, n, theta_dev, phi_dev, ipix_dev, pix_dev, w_dev)) return rc;
    if (int rc = select_device(device)) return rc;
    if (n == 0) return BFGX_OK;
    hipLaunchKernelGGL(hpx::hpx_interp_weights_kernel, dim3(hpx_blocks(n)), dim3(hpx::kThreads), 0, (hipStream_t)hip_stream,
                       hpx_interp_args(nside, nest, n), theta_dev, phi_dev, ipix_dev, pix_dev, w_dev);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

int bfgx_hpx_interp_weights(int device, int64_t nside, int32_t nest, int64_t n, const double *theta, const double *phi, const int64_t *ipix,
                            int64_t *pix_out, double *w_out)
{
    if (int rc = hpx_interp_weights_check(nside, nest, n, theta, phi, ipix, pix_out, w_out)) return rc;
    if (int rc = ipix ? hpx_check_pixels(n, ipix, 12 * nside * nside) : hpx_check_angles(n, theta, phi)) return rc;
    HostCall c(device);
    if (c.rc || n == 0) return c.rc;
    const double *dt = ipix ? nullptr : c.in(theta, n), *dp = ipix ? nullptr : c.in(phi, n);
    const int64_t *di = ipix ? c.in(ipix, n) : nullptr;
    int64_t *dpix = c.out(pix_out, 4 * n);
    double *dw = c.out(w_out, 4 * n);
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_hpx_interp_weights_device(device, nullptr, nside, nest, n, dt, dp, di, dpix, dw)) return rc;
    return c.finish();
}

int bfgx_hpx_interp_val_device(int device, void *hip_stream, int64_t nside, int32_t nest, int64_t nmaps, int32_t dtype, const void *maps_dev,
                               int64_t n, const double *theta_dev, const double *phi_dev, double *out_dev)
{
    if (int rc = hpx_interp_val_check(nside, nest, nmaps, dtype, maps_dev, n, theta_dev, phi_dev, out_dev)) return rc;
    if (int rc = select_device(device)) return rc;
    if (n == 0) return BFGX_OK;
    const hpx::Interp a = hpx_interp_args(nside, nest, n);
    hipStream_t s = (hipStream_t)hip_stream;
    if (dtype)
        hipLaunchKernelGGL(hpx::hpx_interp_val_kernel<double>, dim3(hpx_blocks(n)), dim3(hpx::kThreads), 0, s, a, nmaps, (const double *)maps_dev,
                           theta_dev, phi_dev, out_dev);
    else
        hipLaunchKernelGGL(hpx::hpx_interp_val_kernel<float>, dim3(hpx_blocks(n)), dim3(hpx::kThreads), 0, s, a, nmaps, (const float *)maps_dev,
                           theta_dev, phi_dev, out_dev);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

int bfgx_hpx_interp_val(int device, int64_t nside, int32_t nest, int64_t nmaps, int32_t dtype, const void *maps, int64_t n, const double *theta,
                        const double *phi, double *out)
{
    if (int rc = hpx_interp_val_check(nside, nest, nmaps, dtype, maps, n, theta, phi, out)) return rc;
    if (int rc = hpx_check_angles(n, theta, phi)) return rc;
    HostCall c(device);
    if (c.rc || n == 0) return c.rc;
    const char *dm = c.in((const char *)maps, hpx_dsize(dtype) * (size_t)nmaps * 12 * nside * nside);      // (either dtype: in bytes)
    const double *dt = c.in(theta, n), *dp = c.in(phi, n);
    double *dout = c.out(out, nmaps * n);
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_hpx_interp_val_device(device, nullptr, nside, nest, nmaps, dtype, dm, n, dt, dp, dout)) return rc;
    return c.finish();
}

int bfgx_hpx_neighbours_device(int device, void *hip_stream, int64_t nside, int32_t nest, int64_t n, const int64_t *ipix_dev, int64_t *out_dev)
{
    if (int rc = hpx_neighbours_check(nside, nest, n, ipix_dev, out_dev)) return rc;
    if (int rc = select_device(device)) return rc;
    if (n == 0) return BFGX_OK;
    hipLaunchKernelGGL(hpx::hpx_neighbours_kernel, dim3(hpx_blocks(n)), dim3(hpx::kThreads), 0, (hipStream_t)hip_stream, nside,
                       hpx::nbr_order(nside), nest ? 1 : 0, n, ipix_dev, out_dev);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

int bfgx_hpx_neighbours(int device, int64_t nside, int32_t nest, int64_t n, const int64_t *ipix, int64_t *out)
{
    if (int rc = hpx_neighbours_check(nside, nest, n, ipix, out)) return rc;
    if (int rc = hpx_check_pixels(n, ipix, 12 * nside * nside)) return rc;
    HostCall c(device);
    if (c.rc || n == 0) return c.rc;
    const int64_t *di = c.in(ipix, n);
    int64_t *dout = c.out(out, 8 * n);
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_hpx_neighbours_device(device, nullptr, nside, nest, n, di, dout)) return rc;
    return c.finish();
}

int bfgx_hpx_scatter_add_device(int device, void *hip_stream, int64_t npix, double *hmap_dev, int64_t n, const double *vals_dev,
                                const int64_t *pix_dev, const double *w_dev)
{
    if (int rc = hpx_scatter_add_check(npix, n, hmap_dev, vals_dev, pix_dev, w_dev)) return rc;
    if (int rc = select_device(device)) return rc;
    if (n == 0) return BFGX_OK;
    hipLaunchKernelGGL(hpx::hpx_scatter_add_kernel, dim3(hpx_blocks(4 * n)), dim3(hpx::kThreads), 0, (hipStream_t)hip_stream, npix, hmap_dev, n,
                       vals_dev, pix_dev, w_dev);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

int bfgx_hpx_scatter_add(int device, int64_t npix, double *hmap, int64_t n, const double *vals, const int64_t *pix, const double *w)
{
    if (int rc = hpx_scatter_add_check(npix, n, hmap, vals, pix, w)) return rc;
    if (int rc = hpx_check_scatter_indices(n, pix, npix)) return rc;
    HostCall c(device);
    if (c.rc || n == 0) return c.rc;
    double *dh = c.inout(hmap, npix);
    const double *dv = c.in(vals, n);
    const int64_t *dp = c.in(pix, 4 * n);
    const double *dw = c.in(w, 4 * n);
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_hpx_scatter_add_device(device, nullptr, npix, dh, n, dv, dp, dw)) return rc;
    return c.finish();
}

}  // extern "C"
