// bfgx_deposit_cloud_api.inc -- C ABI of the CIC / TSC particle deposit (ParticleSnapshot.make_map(N, assignment='cic' | 'tsc')) and of
// the same on the grid displaced by half a cell (bfgx_deposit_cloud_shifted_device, grid 2 of bfgx_interlace_api.inc); included
// by bfgx_api.hip after bfgx_deposit_api.inc, whose workspace (DepWork, with the halo scratch), dep_tileable and record buffers (DepRecBuf)
// it shares.  Kernels: bfgx_deposit_cloud.hpp; declarations: include/bfgx.h.

namespace {

// f(dim, order, shift) with all three as integral constants; shift: the grid displaced by half a cell (the second grid of an interlaced pair)
template <typename F> void cloud_dispatch(int ndim, int order, int shift, F &&f)
{
    grid_dim(ndim, [&](auto dim) {
        auto with_order = [&](auto sh) {
            if (order == 2) f(dim, std::integral_constant<int, 2>{}, sh);
            else f(dim, std::integral_constant<int, 3>{}, sh);
        };
        if (shift) with_order(std::true_type{});
        else with_order(std::false_type{});
    });
}

// the tile-owned form: the NGP sort (deposit_tiled) with the particle's index as payload, then the tile and fold launches
int deposit_cloud_tiled(DepWork &w, const DepGeom &g, int order, int shift, hipStream_t s, int64_t n, const double *x, const double *y, const double *z,
                        const double *mass, double L, double *map_out_dev, int64_t stride)
{
    // counters as in deposit_tiled: count2[T + 1] start2[T + 1] cursor2[T], kDepPad words apart | level-1 histograms [B1][chunks] + 1
    const unsigned chunks = (unsigned)((n + kDepChunk - 1) / kDepChunk);
    const size_t o_c2 = 0, o_s2 = o_c2 + g.T + 1, o_k2 = o_s2 + g.T + 1, o_wg = o_k2 + (size_t)g.T * kDepPad;
    const int64_t nwg = (int64_t)g.B1 * chunks + 1;
    uint32_t *const keys[2] = {w.keys[0].as<uint32_t>(), w.keys[1].as<uint32_t>()};
    double *const index[2] = {w.mass[0].as<double>(), w.mass[1].as<double>()};
    int32_t *const ctr = w.ctr.as<int32_t>(), *const bsum = w.bsum.as<int32_t>();
    int64_t *const total = w.total.as<int64_t>();
    double *const halo = w.halo.as<double>();
    HIP_TRY(hipMemsetAsync(ctr, 0, sizeof(int32_t) * (o_wg + (size_t)nwg), s));
    int32_t *c2 = ctr + o_c2, *s2 = ctr + o_s2, *k2 = ctr + o_k2, *wg = ctr + o_wg;
    const size_t lds = sizeof(double) * (size_t)cloud_box_cells(g, order);
    const double scale = (double)g.nb / L;             // s = N / L, computed once, on the host: the kernels multiply by the same number
    int rc = BFGX_OK;
    cloud_dispatch(g.dim, order, shift, [&](auto dim, auto ord, auto sh) {
        constexpr int DIM = decltype(dim)::value, ORDER = decltype(ord)::value;
        constexpr bool SHIFT = decltype(sh)::value;
        hipLaunchKernelGGL((deposit_cloud_keys_kernel<DIM, ORDER, SHIFT>), dim3(chunks), dim3(256), 0, s, g, n, x, y, z, L, scale, keys[0], index[1], wg, stride);
        exclusive_scan(s, nwg, wg, wg, bsum, total);          // (in place)
        hipLaunchKernelGGL((deposit_split_kernel<1, true>), dim3(chunks), dim3(256), 0, s, g, n, (const int32_t *)nullptr, (const uint32_t *)keys[0],
                           (const double *)index[1], (const int32_t *)wg, (int32_t *)nullptr, keys[1], index[0], (int64_t)1);
        const int32_t *nvalid = wg + (nwg - 1);             // particles inside the box
        hipLaunchKernelGGL(deposit_count_kernel, dim3(chunks), dim3(256), 0, s, g, nvalid, (const uint32_t *)keys[1], c2);
        exclusive_scan(s, (int64_t)g.T + 1, c2, s2, bsum, total);
        hipLaunchKernelGGL((deposit_split_kernel<2, true>), dim3(chunks), dim3(256), 0, s, g, n, nvalid, (const uint32_t *)keys[1],
                           (const double *)index[0], (const int32_t *)s2, k2, keys[0], index[1], (int64_t)1);
        if (hipFuncSetAttribute((const void *)deposit_cloud_tiles_kernel<DIM, ORDER, SHIFT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            rc = fail(BFGX_ERR_HIP, "the cloud deposit's tile kernel needs %zu bytes of LDS", lds);
            return;
        }
        hipLaunchKernelGGL((deposit_cloud_tiles_kernel<DIM, ORDER, SHIFT>), dim3(g.T), dim3(kCloudTileThreads), lds, s, g, L, scale, (const int32_t *)s2,
                           (const double *)index[1], x, y, z, mass, stride, map_out_dev, halo);
        hipLaunchKernelGGL((deposit_cloud_fold_kernel<DIM, ORDER>), dim3(g.T), dim3(kCloudFoldThreads), 0, s, g, (const int32_t *)s2, (const double *)halo,
                           map_out_dev);
    });
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

// device columns (or fields of a record buffer at `stride` doubles) -> map_out_dev, enqueue-only
int deposit_cloud_impl(int device, void *hip_stream, int32_t ndim, int64_t n, const double *x, const double *y, const double *z, const double *mass,
                       int32_t n_grid, double L, int32_t order, double *map_out_dev, int64_t stride = 1, int32_t shift = 0)
{
    if ((n > 0 && (!x || !y || (ndim == 3 && !z))) || !map_out_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (shift != 0 && shift != 1) return fail(BFGX_ERR_INVALID, "shift %d: 0 (the grid) or 1 (the grid displaced by half a cell)", shift);
    if (order != 2 && order != 3)
        return fail(BFGX_ERR_INVALID, "the cloud deposit takes order 2 (CIC) or 3 (TSC), not %d; nearest grid point is bfgx_deposit_particles", order);
    if ((ndim != 2 && ndim != 3) || n_grid < 1 || n < 0 || !(L > 0.0) || !std::isfinite(L)) return fail(BFGX_ERR_INVALID, "deposit needs ndim in {2, 3}, n_grid >= 1, 0 < L < inf");
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    size_t ntot = 1;
    for (int d = 0; d < ndim; ++d) ntot *= (size_t)n_grid;
    // the switch between the forms is NGP's (deposit_impl), BFGX_DEPOSIT=atomic / tiled forces one of the two
    const DepGeom g = dep_geom(ndim, n_grid, 0, n_grid);
    bool tiled = n >= (int64_t)1 << 20 && dep_tileable(n, g);
    if (const char *e = std::getenv("BFGX_DEPOSIT")) {
        if (!std::strcmp(e, "atomic")) tiled = false;
        else if (!std::strcmp(e, "tiled")) tiled = n > 0 && dep_tileable(n, g);
    }
    if (tiled) {
        std::lock_guard<std::mutex> lk(g_dep_mu);
        DepWork &w = g_dep[device];
        const size_t nctr = (2 + (size_t)kDepPad) * ((size_t)g.T + 1) + (size_t)g.B1 * (size_t)((n + kDepChunk - 1) / kDepChunk) + 8;
        if (w.keys[0].need(sizeof(uint32_t) * (size_t)n, 8, 0) || w.keys[1].need(sizeof(uint32_t) * (size_t)n, 8, 0)) return alloc_fail("deposit keys");
        if (w.mass[0].need(sizeof(double) * (size_t)n, 8, 0) || w.mass[1].need(sizeof(double) * (size_t)n, 8, 0)) return alloc_fail("deposit indices");
        if (w.ctr.need(sizeof(int32_t) * nctr, 8, 0) || w.bsum.need(sizeof(int32_t) * (size_t)scan_block_count((int64_t)nctr), 8, 0) || w.total.need(sizeof(int64_t), 8, 0))
            return alloc_fail("deposit counters");
        if (w.halo.need(sizeof(double) * (size_t)g.T * (size_t)cloud_halo_cells(g, order), 8, 0)) return alloc_fail("deposit halo scratch");
        return deposit_cloud_tiled(w, g, order, shift, s, n, x, y, z, mass, L, map_out_dev, stride);
    }
    HIP_TRY(hipMemsetAsync(map_out_dev, 0, sizeof(double) * ntot, s));
    if (n > 0) {
        const double scale = (double)n_grid / L;       // (as in deposit_cloud_tiled)
        const unsigned blocks = (unsigned)((n + 255) / 256);
        cloud_dispatch(ndim, order, shift, [&](auto dim, auto ord, auto sh) {
            hipLaunchKernelGGL((deposit_cloud_atomic_kernel<decltype(dim)::value, decltype(ord)::value, decltype(sh)::value>), dim3(blocks), dim3(256), 0, s, n, x, y, z, mass,
                               n_grid, L, scale, map_out_dev, stride);
        });
        HIP_TRY(hipGetLastError());
    }
    return BFGX_OK;
}

}  // namespace

extern "C" {

int bfgx_deposit_cloud_device(int device, void *hip_stream, int32_t ndim, int64_t n, const double *x, const double *y, const double *z,
                              const double *mass, int32_t n_grid, double L, int32_t order, double *map_out_dev)
{
    return deposit_cloud_impl(device, hip_stream, ndim, n, x, y, z, mass, n_grid, L, order, map_out_dev);
}

int bfgx_deposit_cloud_shifted_device(int device, void *hip_stream, int32_t ndim, int64_t n, const double *x, const double *y, const double *z,
                                      const double *mass, int32_t n_grid, double L, int32_t order, int32_t shift, double *map_out_dev)
{
    return deposit_cloud_impl(device, hip_stream, ndim, n, x, y, z, mass, n_grid, L, order, map_out_dev, 1, shift);
}

int bfgx_deposit_cloud(int device, int32_t ndim, int64_t n, const double *x, const double *y, const double *z, const double *mass,
                       int32_t n_grid, double L, int32_t order, double *map_out)
{
    if (!x || !y || (ndim == 3 && !z) || !map_out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (order != 2 && order != 3)
        return fail(BFGX_ERR_INVALID, "the cloud deposit takes order 2 (CIC) or 3 (TSC), not %d; nearest grid point is bfgx_deposit_particles", order);
    if ((ndim != 2 && ndim != 3) || n_grid < 1 || n < 0) return fail(BFGX_ERR_INVALID, "deposit needs ndim in {2, 3}, n_grid >= 1");
    HostCall c(device);
    size_t ntot = 1;
    for (int d = 0; d < ndim; ++d) ntot *= (size_t)n_grid;
    const double *dx = c.in(x, n), *dy = c.in(y, n), *dz = ndim == 3 ? c.in(z, n) : nullptr, *dm = mass ? c.in(mass, n) : nullptr;
    double *dout = c.out(map_out, ntot);
    if (int rc = c.ready()) return rc;
    if (int rc = deposit_cloud_impl(device, nullptr, ndim, n, dx, dy, dz, dm, n_grid, L, order, dout)) return rc;
    return c.finish();
}

int bfgx_deposit_cloud_records(int device, int32_t ndim, int64_t n, const void *records, int32_t itemsize, int32_t off_x, int32_t off_y,
                               int32_t off_z, int32_t off_mass, int32_t n_grid, double L, int32_t order, double *map_out)
{
    if ((n > 0 && !records) || !map_out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (order != 2 && order != 3)
        return fail(BFGX_ERR_INVALID, "the cloud deposit takes order 2 (CIC) or 3 (TSC), not %d; nearest grid point is bfgx_deposit_particles_records", order);
    if ((ndim != 2 && ndim != 3) || n_grid < 1 || n < 0) return fail(BFGX_ERR_INVALID, "deposit needs ndim in {2, 3}, n_grid >= 1");
    auto bad = [&](int off) { return off < 0 || off % 8 || off + 8 > itemsize; };
    if (itemsize < 16 || itemsize % 8 || bad(off_x) || bad(off_y) || (ndim == 3 && bad(off_z)) || (off_mass >= 0 && bad(off_mass)))
        return fail(BFGX_ERR_INVALID, "records must be a multiple of 8 bytes with 8-byte aligned float64 fields");
    if (int rc = select_device(device)) return rc;
    // the buffers, the upload stream and the NaN test of the masses are those of bfgx_deposit_particles_records
    std::lock_guard<std::mutex> lk(g_deprec_mu);
    DepRecBuf &b = g_deprec[device];
    size_t ntot = 1;
    for (int d = 0; d < ndim; ++d) ntot *= (size_t)n_grid;
    const size_t rbytes = (size_t)n * (size_t)itemsize, mbytes = ntot * sizeof(double);
    if (b.rec.need(rbytes, 8, 8) || b.map.need(mbytes, 8, 8) || b.edges.need(16, 8, 8)) return alloc_fail("deposit records");
    if (!b.up) HIP_TRY(hipStreamCreateWithFlags(&b.up, hipStreamNonBlocking));
    OneShotCall call(&b.up);
    (void)call.open_in(records, rbytes, false);
    (void)call.open_out(map_out, mbytes, false);
    hipStream_t s = b.up;
    if (rbytes) HIP_TRY(hipMemcpyAsync(b.rec.p, records, rbytes, hipMemcpyHostToDevice, s));
    const double *base = (const double *)b.rec.p;
    const int64_t stride = itemsize / 8;
    int32_t nanflag = 0;
    if (off_mass >= 0 && n > 0) {
        int32_t *dflag = (int32_t *)b.edges.p;
        HIP_TRY(hipMemsetAsync(dflag, 0, sizeof(int32_t), s));
        hipLaunchKernelGGL(nan_scan_strided_kernel, dim3(2048), dim3(256), 0, s, n, base + off_mass / 8, stride, dflag);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&nanflag, dflag, sizeof(nanflag), hipMemcpyDeviceToHost, s));
    }
    if (int rc = deposit_cloud_impl(device, (void *)s, ndim, n, base + off_x / 8, base + off_y / 8, ndim == 3 ? base + off_z / 8 : nullptr,
                                    off_mass >= 0 ? base + off_mass / 8 : nullptr, n_grid, L, order, (double *)b.map.p, stride)) return rc;
    HIP_TRY(hipMemcpyAsync(map_out, b.map.p, mbytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (nanflag) return fail(BFGX_ERR_ASSERT, "If you want to make a map, provide a value for the particle mass");
    return BFGX_OK;
}

}  // extern "C"
