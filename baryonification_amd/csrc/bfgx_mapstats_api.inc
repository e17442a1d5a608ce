// bfgx_mapstats_api.inc -- C ABI of the map reductions (bfgx_mapstats.hpp); included from bfgx_api.hip.
// Every argument is checked before any device call.  The device entries are enqueue-only on hip_stream.
namespace {

static_assert(BFGX_MAPSTATS_WORK_DOUBLES == mapstats::kMaxBlocks * mapstats::kSlots, "work array of bfgx_mapstats_moments_device");

template <int K>
void mapstats_moments_launch(hipStream_t s, int64_t npix, int nterms, const double *maps, const uint8_t *mask, int64_t *n_out, double *out,
                             double *work)
{
    const int nb = mapstats::moment_blocks(npix);
    hipLaunchKernelGGL(mapstats::mapstats_sum_kernel<K>, dim3(nb), dim3(mapstats::kThreads), 0, s, npix, maps, mask, work);
    hipLaunchKernelGGL(mapstats::mapstats_combine_kernel, dim3(1), dim3(mapstats::kThreads), 0, s, nb, K, (const double *)work, out, n_out);
    hipLaunchKernelGGL(mapstats::mapstats_central_kernel<K>, dim3(nb), dim3(mapstats::kThreads), 0, s, npix, maps, mask, (const double *)out, work);
    hipLaunchKernelGGL(mapstats::mapstats_combine_kernel, dim3(1), dim3(mapstats::kThreads), 0, s, nb, nterms, (const double *)work, out + K,
                       (int64_t *)nullptr);
}

}  // namespace

extern "C" {

int32_t bfgx_mapstats_moment_terms(int32_t nmaps, int32_t order)
{
    if (nmaps < 1 || nmaps > mapstats::kMaxMaps || order < 2 || order > mapstats::kMaxOrder) return -1;
    return mapstats::moment_terms(nmaps, order);
}

int bfgx_mapstats_moments_device(int device, void *hip_stream, int64_t npix, int32_t nmaps, int32_t order, const double *maps_dev,
                                 const uint8_t *mask_dev, int64_t *n_dev, double *out_dev, double *work_dev)
{
    if (!maps_dev || !n_dev || !out_dev || !work_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (npix < 1 || npix > 12 * kHpxMaxNside * kHpxMaxNside) return fail(BFGX_ERR_INVALID, "npix must be in [1, %lld] (got %lld)", (long long)(12 * kHpxMaxNside * kHpxMaxNside), (long long)npix);
    if (nmaps < 1 || nmaps > mapstats::kMaxMaps) return fail(BFGX_ERR_INVALID, "nmaps must be in [1, %d] (got %d)", mapstats::kMaxMaps, nmaps);
    if (order < 2 || order > mapstats::kMaxOrder) return fail(BFGX_ERR_INVALID, "order must be in [2, %d] (got %d)", mapstats::kMaxOrder, order);
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const int nt = mapstats::moment_terms(nmaps, order);
    if (nmaps == 1) mapstats_moments_launch<1>(s, npix, nt, maps_dev, mask_dev, n_dev, out_dev, work_dev);
    else if (nmaps == 2) mapstats_moments_launch<2>(s, npix, nt, maps_dev, mask_dev, n_dev, out_dev, work_dev);
    else mapstats_moments_launch<3>(s, npix, nt, maps_dev, mask_dev, n_dev, out_dev, work_dev);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

int bfgx_mapstats_peaks_device(int device, void *hip_stream, int64_t nside, int32_t nest, const double *map_dev, const uint8_t *mask_dev,
                               int32_t nb, const double *edges_dev, int64_t *counts_dev, int8_t *flags_dev)
{
    if (!map_dev || !edges_dev || !counts_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = hpx_check_nside(nside, nest != 0, "nside")) return rc;
    if (nb < 1 || nb > mapstats::kMaxBins) return fail(BFGX_ERR_INVALID, "nb must be in [1, %d] (got %d)", mapstats::kMaxBins, nb);
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    mapstats::Peaks a;
    a.nside = nside; a.npix = 12 * nside * nside;
    a.order = hpx::nbr_order(nside); a.nest = nest ? 1 : 0; a.nb = nb;
    HIP_TRY(hipMemsetAsync(counts_dev, 0, sizeof(int64_t) * 2 * nb, s));
    hipLaunchKernelGGL(mapstats::mapstats_peaks_kernel, dim3((unsigned)std::min<int64_t>((a.npix + mapstats::kThreads - 1) / mapstats::kThreads, 8192)), dim3(mapstats::kThreads), sizeof(int) * 2 * nb, s, a, map_dev,
                       mask_dev, edges_dev, reinterpret_cast<unsigned long long *>(counts_dev), flags_dev);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

int bfgx_mapstats_peaks_2d_device(int device, void *hip_stream, int64_t n, int32_t periodic, const double *map_dev, const uint8_t *mask_dev,
                                  int32_t nb, const double *edges_dev, int64_t *counts_dev, int8_t *flags_dev)
{
    if (!map_dev || !edges_dev || !counts_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (n < mapstats::kGridMinN || n > mapstats::kGridMaxN) return fail(BFGX_ERR_INVALID, "n must be in [%lld, %lld] (got %lld)", (long long)mapstats::kGridMinN, (long long)mapstats::kGridMaxN, (long long)n);
    if (nb < 1 || nb > mapstats::kMaxBins) return fail(BFGX_ERR_INVALID, "nb must be in [1, %d] (got %d)", mapstats::kMaxBins, nb);
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(hipMemsetAsync(counts_dev, 0, sizeof(int64_t) * 2 * nb, s));
    const int64_t tiles = ((n + mapstats::kGridTileW - 1) / mapstats::kGridTileW) * ((n + mapstats::kGridTileH - 1) / mapstats::kGridTileH);
    hipLaunchKernelGGL(mapstats::mapstats_peaks_grid_kernel, dim3((unsigned)std::min<int64_t>(tiles, mapstats::kGridMaxBlocks)), dim3(mapstats::kThreads),
                       sizeof(int) * 2 * nb, s, (int)n, periodic ? 1 : 0, (int)nb, map_dev, mask_dev, edges_dev,
                       reinterpret_cast<unsigned long long *>(counts_dev), flags_dev);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

int64_t bfgx_mapstats_minkowski_work_doubles(int64_t npix, int32_t nb)
{
    if (npix < 1 || npix > 12 * kHpxMaxNside * kHpxMaxNside || nb < 1 || nb > mapstats::kMaxMfBins) return -1;
    return (int64_t)mapstats::moment_blocks(npix) * 2 * nb;
}

int bfgx_mapstats_minkowski_device(int device, void *hip_stream, int64_t npix, const double *ders_dev, const uint8_t *mask_dev, int32_t nb,
                                   const double *edges_dev, int64_t *counts_dev, double *sums_dev, double *work_dev)
{
    if (!ders_dev || !edges_dev || !counts_dev || !sums_dev || !work_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (npix < 1 || npix > 12 * kHpxMaxNside * kHpxMaxNside) return fail(BFGX_ERR_INVALID, "npix must be in [1, %lld] (got %lld)", (long long)(12 * kHpxMaxNside * kHpxMaxNside), (long long)npix);
    if (nb < 1 || nb > mapstats::kMaxMfBins) return fail(BFGX_ERR_INVALID, "nb must be in [1, %d] (got %d)", mapstats::kMaxMfBins, nb);
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const int nblocks = mapstats::moment_blocks(npix);
    HIP_TRY(hipMemsetAsync(counts_dev, 0, sizeof(int64_t) * (nb + 3), s));
    hipLaunchKernelGGL(mapstats::mapstats_minkowski_kernel, dim3(nblocks), dim3(mapstats::kThreads), mapstats::minkowski_lds_bytes(nb), s, npix,
                       (int)nb, ders_dev, mask_dev, edges_dev, reinterpret_cast<unsigned long long *>(counts_dev), work_dev);
    hipLaunchKernelGGL(mapstats::mapstats_minkowski_combine_kernel, dim3((2 * nb + mapstats::kThreads - 1) / mapstats::kThreads),
                       dim3(mapstats::kThreads), 0, s, nblocks, 2 * (int)nb, (const double *)work_dev, sums_dev);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

}  // extern "C"
