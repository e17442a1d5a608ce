// bfgx_pcl_api.inc -- C ABI of the mode-coupling matrices (bfgx_pcl.hpp); included from bfgx_api.hip.
// Every argument is checked before any device call, by the one check both entries share.  The device entry is enqueue-only on hip_stream.
namespace {

int pcl_check(int32_t lmax, int32_t lw, int32_t kind, const double *wl, const double *m0, const double *m1)
{
    if (!wl || !m0) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (kind < 0 || kind > 2) return fail(BFGX_ERR_INVALID, "kind must be 0 (M00), 1 (M0+) or 2 (M++ and M--) (got %d)", kind);
    if (kind == 2 && !m1) return fail(BFGX_ERR_INVALID, "NULL argument: kind 2 writes M-- to m1");
    if (lmax < 0 || lmax > pcl::kMaxLmax) return fail(BFGX_ERR_INVALID, "lmax must be in [0, %d] (got %d)", pcl::kMaxLmax, lmax);
    if (lw < 0 || lw > pcl::kMaxLw) return fail(BFGX_ERR_INVALID, "lw must be in [0, %d] (got %d)", pcl::kMaxLw, lw);
    return BFGX_OK;
}

template <int KIND>
int pcl_launch(hipStream_t s, int lmax, int lw, const double *wl, double *m0, double *m1)
{
    const size_t lds = pcl::lds_bytes(lmax, lw);
    HIP_TRY(hipFuncSetAttribute((const void *)pcl::pcl_coupling_kernel<KIND>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(pcl::pcl_coupling_kernel<KIND>, dim3((unsigned)(lmax + 1)), dim3(pcl::kWave * pcl::block_waves(lmax, lw)), lds, s, lmax, lw,
                       wl, m0, m1);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

}  // namespace

extern "C" {

int bfgx_pcl_coupling_device(int device, void *hip_stream, int32_t lmax, int32_t lw, int32_t kind, const double *wl_dev, double *m0_dev,
                             double *m1_dev)
{
    if (int rc = pcl_check(lmax, lw, kind, wl_dev, m0_dev, m1_dev)) return rc;
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t bytes = sizeof(double) * ((size_t)lmax + 1) * ((size_t)lmax + 1);
    HIP_TRY(hipMemsetAsync(m0_dev, 0, bytes, s));                   // the kernel writes the band alone
    if (kind == 2) HIP_TRY(hipMemsetAsync(m1_dev, 0, bytes, s));
    if (kind == 0) return pcl_launch<0>(s, lmax, lw, wl_dev, m0_dev, nullptr);
    if (kind == 1) return pcl_launch<1>(s, lmax, lw, wl_dev, m0_dev, nullptr);
    return pcl_launch<2>(s, lmax, lw, wl_dev, m0_dev, m1_dev);
}

int bfgx_pcl_coupling(int device, int32_t lmax, int32_t lw, int32_t kind, const double *wl, double *m0, double *m1)
{
    if (int rc = pcl_check(lmax, lw, kind, wl, m0, m1)) return rc;
    HostCall c(device);
    const size_t n2 = ((size_t)lmax + 1) * ((size_t)lmax + 1);
    const double *dw = c.in(wl, (size_t)lw + 1);
    double *d0 = c.out(m0, n2), *d1 = kind == 2 ? c.out(m1, n2) : nullptr;
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_pcl_coupling_device(device, nullptr, lmax, lw, kind, dw, d0, d1)) return rc;
    return c.finish();
}

}  // extern "C"
