// bfgx_route_api.inc -- C ABI of the halo routing of a multi-GPU step: which rank's rings a halo's disc touches, and the packing of
// catalog rows by destination.  Kernels: bfgx_kernels.hpp.  Needs the shell plan (bfgx_api.hip).

extern "C" {

// launch size of a pass over n halos
static unsigned route_grid(int64_t n, int64_t cap = kRouteGrid) { return (unsigned)std::min<int64_t>((n + 255) / 256, cap); }

// shared argument checks / set-up of the routing passes; n: the halos whose columns are read (0: none are)
static int route_args(bfgx_plan *p, int64_t n, int32_t world, const int32_t *ring_bounds, int32_t ncols, const double *const *cols,
                      RouteArgs &a)
{
    if (!p || !ring_bounds || !cols) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (world < 1 || world > kRouteMaxRanks) return fail(BFGX_ERR_INVALID, "routing supports 1 .. %d ranks", kRouteMaxRanks);
    if (ncols < 1 || ncols > kRouteMaxCols) return fail(BFGX_ERR_INVALID, "routing packs 1 .. %d columns", kRouteMaxCols);
    if (n < 0) return fail(BFGX_ERR_INVALID, "catalog size < 0");
    std::memset(&a, 0, sizeof(a));
    a.world = world; a.ncols = ncols;
    for (int j = 0; j <= world; ++j) {
        if (j > 0 && ring_bounds[j] < ring_bounds[j - 1]) return fail(BFGX_ERR_INVALID, "ring bounds must ascend");
        a.bounds[j] = ring_bounds[j];
    }
    for (int c = 0; c < ncols; ++c) { if (n > 0 && !cols[c]) return fail(BFGX_ERR_INVALID, "column pointer is NULL"); a.col[c] = cols[c]; }
    return BFGX_OK;
}

int bfgx_route_count_device(bfgx_plan *p, int64_t n, const int32_t *rings_dev, int32_t world, const int32_t *ring_bounds, int32_t *counts_dev)
{
    RouteArgs a;
    const double *none[1] = {nullptr};
    if (n < 0 || !counts_dev || (n > 0 && !rings_dev)) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = route_args(p, 0, world, ring_bounds, 1, none, a)) return rc;      // (no columns are read in the counting pass)
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemsetAsync(counts_dev, 0, sizeof(int32_t) * world, p->stream));
    if (n > 0) {
        hipLaunchKernelGGL(route_halos_kernel<false>, dim3(route_grid(n)), dim3(256), 0, p->stream, a, n, rings_dev, counts_dev,
                           (int32_t *)nullptr, (double *)nullptr);
        HIP_TRY(hipGetLastError());
    }
    return BFGX_OK;
}

int bfgx_route_fill_device(bfgx_plan *p, int64_t n, const int32_t *rings_dev, int32_t world, const int32_t *ring_bounds, const int64_t *start,
                           int32_t ncols, const double *const *cols_dev, int32_t *cursor_dev, double *rows_dev)
{
    RouteArgs a;
    if (n < 0 || !start || !cursor_dev || (n > 0 && (!rings_dev || !rows_dev))) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = route_args(p, n, world, ring_bounds, ncols, cols_dev, a)) return rc;
    for (int j = 0; j < world; ++j) a.start[j] = start[j];
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemsetAsync(cursor_dev, 0, sizeof(int32_t) * world, p->stream));
    if (n > 0) {
        hipLaunchKernelGGL(route_halos_kernel<true>, dim3(route_grid(n)), dim3(256), 0, p->stream, a, n, rings_dev, (int32_t *)nullptr,
                           cursor_dev, rows_dev);
        HIP_TRY(hipGetLastError());
    }
    return BFGX_OK;
}

int bfgx_route_pack_device(bfgx_plan *p, int64_t n, const int32_t *rings_dev, int32_t world, const int32_t *ring_bounds, int64_t blockcap,
                           int32_t ncols, const double *const *cols_dev, int32_t *cursor_dev, double *blocks_dev, int32_t *overflow_dev)
{
    RouteArgs a;
    if (n < 0 || !cursor_dev || !blocks_dev || !overflow_dev || (n > 0 && !rings_dev)) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (blockcap < 1) return fail(BFGX_ERR_INVALID, "block capacity must be >= 1");
    if (int rc = route_args(p, n, world, ring_bounds, ncols, cols_dev, a)) return rc;
    a.blockcap = blockcap; a.overflow = overflow_dev;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemsetAsync(cursor_dev, 0, sizeof(int32_t) * world, p->stream));
    hipLaunchKernelGGL(route_blank_kernel, dim3(route_grid((int64_t)world * blockcap, 1024)), dim3(256), 0, p->stream,
                       world, ncols, blockcap, blocks_dev);
    HIP_TRY(hipGetLastError());
    if (n > 0) {
        hipLaunchKernelGGL(route_halos_kernel<true>, dim3(route_grid(n)), dim3(256), 0, p->stream, a, n, rings_dev, (int32_t *)nullptr,
                           cursor_dev, blocks_dev);
        HIP_TRY(hipGetLastError());
    }
    return BFGX_OK;
}

// The routing of one resident multi-GPU step as ONE call and two launches (bfgx_disc_rings_device + bfgx_route_pack_device were four, with a
// fill): route_prepare_kernel (NaN into column 0 of every block, the cursors zeroed) and route_step_kernel (ring range per halo, rows
// packed by destination).  send_blocks_dev holds (world - 1) blocks [ncols][blockcap] in rank order WITHOUT this rank, recv_blocks_dev
// world blocks: the other ranks' in rank order (what all_to_all_single delivers when the split towards oneself is empty), this rank's
// own rows LAST -- they never enter the collective.  K0 reads the received blocks as they are (bfgx_plan_set_catalog_blocks).
int bfgx_route_step_device(bfgx_plan *p, const bfgx_catalog *cat, int32_t world, int32_t rank, const int32_t *ring_bounds, int64_t blockcap,
                           int32_t ncols, const double *const *cols_dev, int32_t *cursor_dev, double *send_blocks_dev, double *recv_blocks_dev,
                           int32_t *overflow_dev)
{
    if (!p || !cat || !cursor_dev || !recv_blocks_dev || !overflow_dev || (world > 1 && !send_blocks_dev)) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (rank < 0 || rank >= world) return fail(BFGX_ERR_INVALID, "rank out of range");
    if (blockcap < 1) return fail(BFGX_ERR_INVALID, "block capacity must be >= 1");
    if (cat->n > 0 && (!cat->M || !cat->z || !cat->dec)) return fail(BFGX_ERR_INVALID, "catalog column pointer is NULL");
    RouteStepArgs s;
    std::memset(&s, 0, sizeof(s));
    if (int rc = route_args(p, cat->n, world, ring_bounds, ncols, cols_dev, s.r)) return rc;
    s.r.blockcap = blockcap; s.r.overflow = overflow_dev;
    s.rank = rank; s.margin = p->route_margin;
    s.M = cat->M; s.z = cat->z; s.dec = cat->dec;
    s.send = send_blocks_dev; s.recv = recv_blocks_dev;
    HIP_TRY(hipSetDevice(p->device));
    const int64_t nblank = (int64_t)(2 * world - 1) * blockcap;
    hipLaunchKernelGGL(route_prepare_kernel, dim3(route_grid(nblank, 1024)), dim3(256), 0, p->stream, world, ncols, blockcap,
                       send_blocks_dev, recv_blocks_dev, cursor_dev);
    if (cat->n > 0)
        // (2048 workgroups: eight waves per SIMD hide the latency of the strided column stores; each adds to the per-destination cursors once)
        hipLaunchKernelGGL(route_step_kernel, dim3(route_grid(cat->n, 4 * kRouteGrid)), dim3(256), 0, p->stream, s, p->model, p->hpx,
                           cat->n, cursor_dev);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

int bfgx_disc_rings_device(bfgx_plan *p, const bfgx_catalog *cat, int32_t *rings_dev)
{
    // (uses none of the plan's per-halo workspace: the catalog may be larger than the plan's max_halos)
    if (!p || !cat) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (cat->n < 0) return fail(BFGX_ERR_INVALID, "catalog size < 0");
    if (cat->n > 0 && (!cat->M || !cat->z || !cat->dec)) return fail(BFGX_ERR_INVALID, "catalog column pointer is NULL");
    if (cat->n > 0 && !rings_dev) return fail(BFGX_ERR_INVALID, "rings pointer is NULL");
    HIP_TRY(hipSetDevice(p->device));
    if (cat->n > 0) {
        hipLaunchKernelGGL(disc_rings_kernel, dim3((unsigned)((cat->n + 255) / 256)), dim3(256), 0, p->stream, p->model, p->hpx, cat->n, cat->M, cat->z,
                           cat->dec, rings_dev, p->route_margin);
        HIP_TRY(hipGetLastError());
    }
    return BFGX_OK;
}

int bfgx_plan_set_route_margin(bfgx_plan *p, int32_t rings)
{
    if (!p) return fail(BFGX_ERR_INVALID, "NULL plan");
    if (rings < 0 || rings > 4 * p->hpx.nside) return fail(BFGX_ERR_INVALID, "route margin must be 0 .. 4 nside rings");
    p->route_margin = rings;
    return BFGX_OK;
}

}  // extern "C"
