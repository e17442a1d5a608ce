// bfgx_deposit_api.inc -- C ABI of the particle deposit (ParticleSnapshot.make_map, io.py:622-670) and of the particle routing between
// ranks; included by bfgx_api.hip after bfgx_grid_api.inc: the fused deposit + regrid entry needs the grid plan (and grid_dim).
// bfgx_snapshot_api.inc builds on deposit_impl, DepKeysBy and DepRecBuf.  Kernels: bfgx_deposit.hpp; declarations: include/bfgx.h.

namespace {

// grow-only workspace of the tiled deposit, one per device (released by bfgx_cache_clear); one deposit in flight per device
struct DepWork {
    PoolBuf keys[2], mass[2], ctr, bsum, total;     // uint32_t keys, double masses, int32_t counters and block sums, one int64_t (slack: an eighth)
    PoolBuf halo;                                   // per-tile halo slabs of the CIC / TSC deposit (bfgx_deposit_cloud_api.inc)
};
std::mutex g_dep_mu;
std::map<int, DepWork> g_dep;

void dep_release_all()
{
    std::lock_guard<std::mutex> lk(g_dep_mu);
    while (!g_dep.empty()) {
        (void)hipSetDevice(g_dep.begin()->first);
        g_dep.erase(g_dep.begin());
    }
}

// keys_by (optional): who writes the keys [n] and the per-chunk level-1 histograms [B1][chunks] instead of deposit_keys_kernel (the snapshot
// path's displacement kernel does, for the particles it has just moved)
using DepKeysBy = std::function<int(const DepGeom &, uint32_t *, int32_t *, unsigned)>;

// can the tile-owned deposit take n particles on this grid?  (32-bit ranks and keys; buckets that fit a workgroup's scan and LDS histogram)
bool dep_tileable(int64_t n, const DepGeom &g)
{
    return n < ((int64_t)1 << 31) - kDepChunk && g.T < (1 << (32 - kDepLocalBits)) && g.B1 <= 1024 && g.B2 <= kDepHist;
}

template <bool MASS>
int deposit_tiled(DepWork &w, const DepGeom &g, hipStream_t s, int64_t n, const double *x, const double *y, const double *z,
                  const double *mass, const double *edges_dev, double *map_out_dev, double *map_out2_dev = nullptr, double *tile_sums_dev = nullptr,
                  int64_t stride = 1, const DepKeysBy *keys_by = nullptr)
{
    // counters: count2[T + 1] start2[T + 1] cursor2[T], kDepPad words apart | per-workgroup level-1 histograms [B1][chunks] + 1, scanned in place
    const unsigned chunks = (unsigned)((n + kDepChunk - 1) / kDepChunk);
    const size_t o_c2 = 0, o_s2 = o_c2 + g.T + 1, o_k2 = o_s2 + g.T + 1, o_wg = o_k2 + (size_t)g.T * kDepPad;
    const int64_t nwg = (int64_t)g.B1 * chunks + 1;
    uint32_t *const keys[2] = {w.keys[0].as<uint32_t>(), w.keys[1].as<uint32_t>()};
    double *const wmass[2] = {w.mass[0].as<double>(), w.mass[1].as<double>()};
    int32_t *const ctr = w.ctr.as<int32_t>(), *const bsum = w.bsum.as<int32_t>();
    int64_t *const total = w.total.as<int64_t>();
    HIP_TRY(hipMemsetAsync(ctr, 0, sizeof(int32_t) * (o_wg + (size_t)nwg), s));
    int32_t *c2 = ctr + o_c2, *s2 = ctr + o_s2, *k2 = ctr + o_k2, *wg = ctr + o_wg;
    if (keys_by) { if (int rc = (*keys_by)(g, keys[0], wg, chunks)) return rc; }
    else grid_dim(g.dim, [&](auto dim) {
        hipLaunchKernelGGL((deposit_keys_kernel<decltype(dim)::value>), dim3(chunks), dim3(256), 0, s, g, n, x, y, z, edges_dev, keys[0], wg, stride);
    });
    exclusive_scan(s, nwg, wg, wg, bsum, total);          // (in place)
    hipLaunchKernelGGL((deposit_split_kernel<1, MASS>), dim3(chunks), dim3(256), 0, s, g, n, (const int32_t *)nullptr, (const uint32_t *)keys[0],
                       mass, (const int32_t *)wg, (int32_t *)nullptr, keys[1], wmass[0], stride);
    const int32_t *nvalid = wg + (nwg - 1);             // particles inside the edges
    hipLaunchKernelGGL(deposit_count_kernel, dim3(chunks), dim3(256), 0, s, g, nvalid, (const uint32_t *)keys[1], c2);
    exclusive_scan(s, (int64_t)g.T + 1, c2, s2, bsum, total);
    hipLaunchKernelGGL((deposit_split_kernel<2, MASS>), dim3(chunks), dim3(256), 0, s, g, n, nvalid, (const uint32_t *)keys[1],
                       (const double *)wmass[0], (const int32_t *)s2, k2, keys[0], wmass[1], (int64_t)1);
    hipLaunchKernelGGL(deposit_tiles_kernel<MASS>, dim3(g.T), dim3(DepTileThreads<MASS>::n), 0, s, g, (const int32_t *)s2, (const uint32_t *)keys[0],
                       (const double *)wmass[1], map_out_dev, map_out2_dev, tile_sums_dev);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

}  // namespace

extern "C" {

int bfgx_route_particles_count_device(int device, void *hip_stream, int64_t n, const double *x, int32_t n_grid, const double *edges_dev,
                                      int32_t world, uint8_t *owner_dev, int32_t *counts_dev)
{
    if ((n > 0 && (!x || !owner_dev)) || !edges_dev || !counts_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (n < 0 || n_grid < 1 || world < 1 || world > kPartRouteMaxRanks || n_grid % world) return fail(BFGX_ERR_INVALID, "particle routing needs 1 <= world <= %d ranks that divide n_grid", kPartRouteMaxRanks);
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(hipMemsetAsync(counts_dev, 0, sizeof(int32_t) * world, s));
    if (n > 0) {
        hipLaunchKernelGGL(route_particles_count_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, kPartRouteGrid)), dim3(256), 0, s, n, x, edges_dev,
                           n_grid, n_grid / world, world, owner_dev, counts_dev);
        HIP_TRY(hipGetLastError());
    }
    return BFGX_OK;
}

int bfgx_route_particles_fill_device(int device, void *hip_stream, int64_t n, int32_t ncols, const double *const *cols, const uint8_t *owner_dev,
                                     int32_t world, const int64_t *start_host, int64_t total, int32_t *cursor_dev, double *cols_out_dev)
{
    if (!cols || !start_host || !cursor_dev || (n > 0 && !owner_dev) || (total > 0 && !cols_out_dev)) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (n < 0 || total < 0 || total > n || ncols < 1 || ncols > 4 || world < 1 || world > kPartRouteMaxRanks) return fail(BFGX_ERR_INVALID, "bad particle routing arguments");
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    PartRouteArgs a;
    std::memset(&a, 0, sizeof(a));
    a.world = world; a.ncols = ncols;
    for (int d = 0; d < world; ++d) a.start[d] = start_host[d];
    for (int c = 0; c < ncols; ++c) { if (n > 0 && !cols[c]) return fail(BFGX_ERR_INVALID, "column pointer is NULL"); a.col[c] = cols[c]; }
    HIP_TRY(hipMemsetAsync(cursor_dev, 0, sizeof(int32_t) * world, s));
    if (n > 0 && total > 0) {
        hipLaunchKernelGGL(route_particles_fill_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, kPartRouteGrid)), dim3(256), 0, s, a, n, total, owner_dev,
                           cursor_dev, cols_out_dev);
        HIP_TRY(hipGetLastError());
    }
    return BFGX_OK;
}

int bfgx_deposit_particles_device(int device, void *hip_stream, int32_t ndim, int64_t n, const double *x, const double *y, const double *z,
                                  const double *mass, int32_t n_grid, const double *edges_dev, double *map_out_dev)
{
    return bfgx_deposit_particles_slab_device(device, hip_stream, ndim, n, x, y, z, mass, n_grid, edges_dev, 0, n_grid, map_out_dev);
}

// map_out2_dev / tile_sums_dev / *ntiles (optional): the tile-owned form also stores a second copy of the map and the tiles' totals
// (*ntiles of them); *ntiles = 0 when the atomic form ran (small inputs), which stores neither
static int deposit_impl(int device, void *hip_stream, int32_t ndim, int64_t n, const double *x, const double *y, const double *z,
                        const double *mass, int32_t n_grid, const double *edges_dev, int32_t plane_lo, int32_t plane_n,
                        double *map_out_dev, double *map_out2_dev, double *tile_sums_dev, int32_t *ntiles, int64_t stride = 1,
                        const DepKeysBy *keys_by = nullptr)
{
    if (ntiles) *ntiles = 0;
    if ((n > 0 && (!x || !y || (ndim == 3 && !z))) || !edges_dev || !map_out_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if ((ndim != 2 && ndim != 3) || n_grid < 1 || n < 0) return fail(BFGX_ERR_INVALID, "deposit needs ndim in {2, 3}, n_grid >= 1");
    if (plane_lo < 0 || plane_n < 1 || plane_lo + plane_n > n_grid) return fail(BFGX_ERR_INVALID, "slab [%d, %d) outside the grid", plane_lo, plane_lo + plane_n);
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    size_t ntot = (size_t)plane_n;
    for (int d = 1; d < ndim; ++d) ntot *= (size_t)n_grid;
    // tile-owned form (bfgx_deposit.hpp) when there is enough work to sort; BFGX_DEPOSIT=atomic / tiled forces one of the two
    const DepGeom g = dep_geom(ndim, n_grid, plane_lo, plane_n);
    bool tiled = n >= (int64_t)1 << 20 && dep_tileable(n, g);
    if (const char *e = std::getenv("BFGX_DEPOSIT")) {
        if (!std::strcmp(e, "atomic")) tiled = false;
        else if (!std::strcmp(e, "tiled")) tiled = n > 0 && dep_tileable(n, g);
    }
    if (keys_by) {             // the keys come from another kernel: the sort is the only form there is
        tiled = n > 0 && dep_tileable(n, g);
        if (n > 0 && !tiled) return fail(BFGX_ERR_UNSUPPORTED, "the fused displace + deposit needs a grid the tile-owned deposit takes (%d tiles): call the displacement and the deposit one after the other", g.T);
    }
    if (tiled) {
        std::lock_guard<std::mutex> lk(g_dep_mu);
        DepWork &w = g_dep[device];
        const size_t nctr = (2 + (size_t)kDepPad) * ((size_t)g.T + 1) + (size_t)g.B1 * (size_t)((n + kDepChunk - 1) / kDepChunk) + 8;
        if (w.keys[0].need(sizeof(uint32_t) * (size_t)n, 8, 0) || w.keys[1].need(sizeof(uint32_t) * (size_t)n, 8, 0)) return alloc_fail("deposit keys");
        if (mass && (w.mass[0].need(sizeof(double) * (size_t)n, 8, 0) || w.mass[1].need(sizeof(double) * (size_t)n, 8, 0))) return alloc_fail("deposit masses");
        // (block sums: both scans of deposit_tiled are over fewer than nctr counts)
        if (w.ctr.need(sizeof(int32_t) * nctr, 8, 0) || w.bsum.need(sizeof(int32_t) * (size_t)scan_block_count((int64_t)nctr), 8, 0) || w.total.need(sizeof(int64_t), 8, 0))
            return alloc_fail("deposit counters");
        if (ntiles) *ntiles = g.T;
        return mass ? deposit_tiled<true>(w, g, s, n, x, y, z, mass, edges_dev, map_out_dev, map_out2_dev, tile_sums_dev, stride, keys_by)
                    : deposit_tiled<false>(w, g, s, n, x, y, z, mass, edges_dev, map_out_dev, map_out2_dev, tile_sums_dev, stride, keys_by);
    }
    HIP_TRY(hipMemsetAsync(map_out_dev, 0, sizeof(double) * ntot, s));
    if (n > 0) {
        const unsigned blocks = (unsigned)((n + 255) / 256);
        grid_dim(ndim, [&](auto dim) {
            hipLaunchKernelGGL((particle_deposit_kernel<decltype(dim)::value>), dim3(blocks), dim3(256), 0, s, n, x, y, z, mass, n_grid, edges_dev, map_out_dev, plane_lo, plane_n, stride);
        });
        HIP_TRY(hipGetLastError());
    }
    return BFGX_OK;
}

int bfgx_deposit_particles_slab_device(int device, void *hip_stream, int32_t ndim, int64_t n, const double *x, const double *y, const double *z,
                                       const double *mass, int32_t n_grid, const double *edges_dev, int32_t plane_lo, int32_t plane_n,
                                       double *map_out_dev)
{
    return deposit_impl(device, hip_stream, ndim, n, x, y, z, mass, n_grid, edges_dev, plane_lo, plane_n, map_out_dev, nullptr, nullptr, nullptr);
}

int bfgx_grid_deposit_baryonify_device(bfgx_grid_plan *p, const bfgx_grid_catalog *c, int64_t n_particles, const double *x, const double *y,
                                       const double *z, const double *mass, const double *edges_dev, double *map_in_dev, double *map_out_dev,
                                       double *sums_dev, int64_t *n_pairs_host)
{
    if (!p || !map_in_dev || !map_out_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (p->geom.slab_n != p->geom.npix) return fail(BFGX_ERR_INVALID, "the plan owns a slab: use the slab entry points");
    // ParticleSnapshot.make_map (io.py:622-670) straight into BaryonifyGrid.process (Map2DRunner.py:431-607): the deposit's last kernel
    // stores every cell of the histogram twice -- map_in and the start value of map_out -- and leaves the tiles' totals, so the pass
    // that copies map_in into map_out and sums it (1.07 GB read + 1.07 GB written at 512^3) does not run
    int32_t ntiles = 0;
    if (int rc = deposit_impl(p->device, (void *)p->stream, p->geom.ndim, n_particles, x, y, z, mass, p->geom.npix, edges_dev, 0, p->geom.npix,
                              map_in_dev, map_out_dev, p->block_sums, &ntiles)) return rc;
    return grid_baryonify_impl(p, c, map_in_dev, map_out_dev, sums_dev, n_pairs_host, ntiles);
}

int bfgx_deposit_particles(int device, int32_t ndim, int64_t n, const double *x, const double *y, const double *z, const double *mass,
                           int32_t n_grid, const double *edges, double *map_out)
{
    if (!x || !y || (ndim == 3 && !z) || !edges || !map_out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if ((ndim != 2 && ndim != 3) || n_grid < 1 || n < 0) return fail(BFGX_ERR_INVALID, "deposit needs ndim in {2, 3}, n_grid >= 1");
    for (int i = 1; i <= n_grid; ++i) if (!(edges[i] > edges[i - 1])) return fail(BFGX_ERR_INVALID, "edges must be strictly ascending");
    HostCall c(device);
    size_t ntot = 1;
    for (int d = 0; d < ndim; ++d) ntot *= (size_t)n_grid;
    const double *dx = c.in(x, n), *dy = c.in(y, n), *dz = ndim == 3 ? c.in(z, n) : nullptr, *dm = mass ? c.in(mass, n) : nullptr;
    const double *de = c.in(edges, n_grid + 1);
    double *dout = c.out(map_out, ntot);
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_deposit_particles_device(device, nullptr, ndim, n, dx, dy, dz, dm, n_grid, de, dout)) return rc;
    return c.finish();
}

}  // extern "C"

namespace {
// device buffers of the records entry below, kept between calls per device (bfgx_cache_clear frees them)
struct DepRecBuf {
    PoolBuf rec, map, edges;                   // (slack: an eighth + 8 bytes)
    hipStream_t up = nullptr;
    ~DepRecBuf() { if (up) (void)hipStreamDestroy(up); }
};
std::mutex g_deprec_mu;
std::map<int, DepRecBuf> g_deprec;
void deprec_release_all()
{
    std::lock_guard<std::mutex> lk(g_deprec_mu);
    while (!g_deprec.empty()) {
        (void)hipSetDevice(g_deprec.begin()->first);
        g_deprec.erase(g_deprec.begin());
    }
}
}  // namespace

extern "C" {

int bfgx_deposit_particles_records(int device, int32_t ndim, int64_t n, const void *records, int32_t itemsize, int32_t off_x, int32_t off_y,
                                   int32_t off_z, int32_t off_mass, int32_t n_grid, const double *edges, double *map_out)
{
    if ((n > 0 && !records) || !edges || !map_out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if ((ndim != 2 && ndim != 3) || n_grid < 1 || n < 0) return fail(BFGX_ERR_INVALID, "deposit needs ndim in {2, 3}, n_grid >= 1");
    auto bad = [&](int off) { return off < 0 || off % 8 || off + 8 > itemsize; };
    if (itemsize < 16 || itemsize % 8 || bad(off_x) || bad(off_y) || (ndim == 3 && bad(off_z)) || (off_mass >= 0 && bad(off_mass)))
        return fail(BFGX_ERR_INVALID, "records must be a multiple of 8 bytes with 8-byte aligned float64 fields");
    for (int i = 1; i <= n_grid; ++i) if (!(edges[i] > edges[i - 1])) return fail(BFGX_ERR_INVALID, "edges must be strictly ascending");
    if (int rc = select_device(device)) return rc;
    std::lock_guard<std::mutex> lk(g_deprec_mu);
    DepRecBuf &b = g_deprec[device];
    size_t ntot = 1;
    for (int d = 0; d < ndim; ++d) ntot *= (size_t)n_grid;
    const size_t rbytes = (size_t)n * (size_t)itemsize, mbytes = ntot * sizeof(double), ebytes = sizeof(double) * (size_t)(n_grid + 1);
    if (b.rec.need(rbytes, 8, 8) || b.map.need(mbytes, 8, 8) || b.edges.need(ebytes + 16, 8, 8)) return alloc_fail("deposit records");
    if (!b.up) HIP_TRY(hipStreamCreateWithFlags(&b.up, hipStreamNonBlocking));
    // the records go up as they are (page-locked for the call when the host allows it: the copy then runs at the PCIe rate); the kernels
    // read the coordinate / mass fields at their stride -- no strided gather of four columns on the host
    OneShotCall call(&b.up);
    (void)call.open_in(records, rbytes, false);              // (large arrays are page-locked for the call; small ones are copied from pageable memory)
    (void)call.open_out(map_out, mbytes, false);
    hipStream_t s = b.up;
    HIP_TRY(hipMemcpyAsync(b.edges.p, edges, ebytes, hipMemcpyHostToDevice, s));
    if (rbytes) HIP_TRY(hipMemcpyAsync(b.rec.p, records, rbytes, hipMemcpyHostToDevice, s));
    const double *base = (const double *)b.rec.p;
    const int64_t stride = itemsize / 8;
    int32_t nanflag = 0;
    if (off_mass >= 0 && n > 0) {
        // "If you want to make a map, provide a value for the particle mass" (io.py:636): the NaN test of the masses, on the device
        int32_t *dflag = (int32_t *)((char *)b.edges.p + ebytes);
        HIP_TRY(hipMemsetAsync(dflag, 0, sizeof(int32_t), s));
        hipLaunchKernelGGL(nan_scan_strided_kernel, dim3(2048), dim3(256), 0, s, n, base + off_mass / 8, stride, dflag);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&nanflag, dflag, sizeof(nanflag), hipMemcpyDeviceToHost, s));
    }
    if (int rc = deposit_impl(device, (void *)s, ndim, n, base + off_x / 8, base + off_y / 8, ndim == 3 ? base + off_z / 8 : nullptr,
                              off_mass >= 0 ? base + off_mass / 8 : nullptr, n_grid, (const double *)b.edges.p, 0, n_grid, (double *)b.map.p, nullptr, nullptr, nullptr,
                              stride)) return rc;
    HIP_TRY(hipMemcpyAsync(map_out, b.map.p, mbytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (nanflag) return fail(BFGX_ERR_ASSERT, "If you want to make a map, provide a value for the particle mass");
    return BFGX_OK;
}

}  // extern "C"
