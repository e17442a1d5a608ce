// bfgx_snapshot_api.inc -- C ABI of the particle-snapshot path (included at the end of bfgx_api.hip).
// Replaces BaryonifySnapshot.process, BaryonForge/Runners/SnapshotRunner.py:173-262 (declared in include/bfgx.h).

namespace {

int snapshot_cells(int ndim)
{
    int nc = ndim == 3 ? 128 : 1024;
    if (const char *e = std::getenv("BFGX_SNAP_CELLS")) nc = std::max(1, std::min(ndim == 3 ? 512 : 8192, std::atoi(e)));   // tests / tuning
    return nc;
}

}  // namespace

extern "C" void bfgx_snapshot_plan_destroy(struct bfgx_snapshot_plan *p);

struct bfgx_snapshot_plan {
    int device = 0;
    hipStream_t stream = nullptr;
    DevList mem;
    DevModel model;
    SnapGeom geom;
    int64_t max_halos = 0, nscan = 0, entry_capacity = 0;
    int nblocks = 0, n_cu = 256;
    SnapHaloRec *recs = nullptr;
    int32_t *count = nullptr, *start = nullptr, *cursor = nullptr, *bsum = nullptr, *flags = nullptr;
    int64_t *total = nullptr;
    unsigned long long *pairs = nullptr;
    uint32_t *bitmap = nullptr;
    SnapEntry *entries = nullptr;
};

extern "C" {

int bfgx_snapshot_plan_create(int device, void *hip_stream, const bfgx_model *model, int32_t ndim, double L, double redshift,
                              int64_t max_halos, bfgx_snapshot_plan **out)
{
    if (!model || !out) return fail(BFGX_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (ndim != 2 && ndim != 3) return fail(BFGX_ERR_INVALID, "snapshot ndim must be 2 or 3");
    if (!(L > 0) || !(redshift > -1.0) || max_halos < 0) return fail(BFGX_ERR_INVALID, "bad box size / redshift / max_halos");
    if (int rc = validate_model(model)) return rc;
    if (model->table.ndim != 3) return fail(BFGX_ERR_UNSUPPORTED, "BaryonifySnapshot passes no halo properties to the model (SnapshotRunner.py:240): 3-axis tables only");
    if (model->table.log_values) return fail(BFGX_ERR_INVALID, "BaryonifySnapshot needs a displacement table");
    if (int rc = select_device(device)) return rc;
    bfgx_snapshot_plan *p = new bfgx_snapshot_plan();
    p->device = device; p->stream = (hipStream_t)hip_stream; p->max_halos = max_halos;
    auto bail = [&](int rc) { bfgx_snapshot_plan_destroy(p); return rc; };
    int NC = 4;
    if (int rc = upload_model(p->mem, p->stream, model, false, p->model, NC)) return bail(rc);
    SnapGeom &g = p->geom;
    g.ndim = ndim; g.nc = snapshot_cells(ndim); g.L = L; g.inv_cell = (double)g.nc / L;
    g.a = 1.0 / (1.0 + redshift);
    g.ncell = 1;
    for (int d = 0; d < ndim; ++d) g.ncell *= g.nc;
    p->nscan = g.ncell + 1;
    p->nblocks = scan_block_count(p->nscan);
    DevList &mem = p->mem;
    p->entry_capacity = 16 * max_halos + 65536;
    if (mem.alloc(p->recs, (size_t)std::max<int64_t>(max_halos, 1)) || mem.alloc(p->count, (size_t)p->nscan) || mem.alloc(p->start, (size_t)p->nscan) ||
        mem.alloc(p->cursor, (size_t)p->nscan) || mem.alloc(p->bsum, (size_t)p->nblocks) || mem.alloc(p->total, 1) || mem.alloc(p->flags, 1) ||
        mem.alloc(p->pairs, 1) || mem.alloc(p->bitmap, (size_t)((g.ncell + 31) / 32)) || mem.alloc(p->entries, (size_t)p->entry_capacity))
        return bail(alloc_fail("snapshot workspace"));
    p->n_cu = device_cu_count(device);
    *out = p;
    return BFGX_OK;
}

void bfgx_snapshot_plan_destroy(bfgx_snapshot_plan *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    (void)hipStreamSynchronize(p->stream);
    p->mem.release();
    delete p;
}

// the displacement in stages (the streamed records entry interleaves the middle one with the particles' arrival):
//   snap_lists_stage     halo records, per-cell halo lists (needs the catalog only)
//   snap_displace_stage  n particles: columns px / py / pz -> ox / oy / oz with element strides sin / sout
//   snap_finish_stage    flags, pair count
static int snap_lists_stage(bfgx_snapshot_plan *p, const bfgx_grid_catalog *halos)
{
    const SnapGeom &g = p->geom;
    if (halos->n < 0 || halos->n > p->max_halos) return fail(BFGX_ERR_INVALID, "bad particle count / catalog larger than the plan's max_halos");
    if (halos->n > 0 && (!halos->M || !halos->x || !halos->y || (g.ndim == 3 && !halos->z))) return fail(BFGX_ERR_INVALID, "catalog column pointer is NULL");
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t s = p->stream;
    HIP_TRY(hipMemsetAsync(p->count, 0, sizeof(int32_t) * (size_t)p->nscan, s));
    HIP_TRY(hipMemsetAsync(p->cursor, 0, sizeof(int32_t) * (size_t)p->nscan, s));
    HIP_TRY(hipMemsetAsync(p->flags, 0, sizeof(int32_t), s));
    HIP_TRY(hipMemsetAsync(p->pairs, 0, sizeof(unsigned long long), s));
    const unsigned hblocks = (unsigned)((halos->n + 255) / 256);
    if (halos->n > 0) {
        hipLaunchKernelGGL(snap_halo_prep_kernel, dim3(hblocks), dim3(256), 0, s, p->model, g, halos->n, halos->M, halos->x, halos->y, halos->z, halos->lnM,
                           p->recs, p->flags);
        hipLaunchKernelGGL(snap_halo_count_kernel, dim3((unsigned)((halos->n + 256 / kWave - 1) / (256 / kWave))), dim3(256), 0, s, g, halos->n,
                           (const SnapHaloRec *)p->recs, p->count);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(cell_bitmap_kernel, dim3((unsigned)(((g.ncell + 31) / 32 + 255) / 256)), dim3(256), 0, s, g.ncell, (const int32_t *)p->count, p->bitmap);
    exclusive_scan(s, p->nscan, p->count, p->start, p->bsum, p->total);
    HIP_TRY(hipGetLastError());
    int64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, p->total, sizeof(total), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (total > (int64_t)INT32_MAX) return fail(BFGX_ERR_INVALID, "halo-cell lists exceed 2^31 entries: use fewer cells (BFGX_SNAP_CELLS) or split the catalog");
    if (total > p->entry_capacity) if (int rc = grow_list(p->mem, p->entries, p->entry_capacity, total)) return rc;   // (rare: very large query balls)
    if (halos->n > 0 && total > 0) {
        hipLaunchKernelGGL(snap_halo_fill_kernel, dim3((unsigned)((halos->n + 256 / kWave - 1) / (256 / kWave))), dim3(256), 0, s, g, halos->n, (const SnapHaloRec *)p->recs, (const int32_t *)p->start,
                           p->cursor, p->entries);
        HIP_TRY(hipGetLastError());
    }
    return BFGX_OK;
}

static int snap_displace_stage(bfgx_snapshot_plan *p, int64_t n_part, const double *px, const double *py, const double *pz, int64_t sin,
                               double *x_out, double *y_out, double *z_out, int64_t sout, const SnapDepArgs *keys_to = nullptr)
{
    // keys_to: the displaced particles' deposit keys instead of their coordinates (bfgx_snapshot_displace_deposit_device)
    if (n_part <= 0) return BFGX_OK;
    const SnapGeom &g = p->geom;
    hipStream_t s = p->stream;
    const int64_t units = keys_to ? (int64_t)keys_to->nchunks : (n_part + kSnapBlock - 1) / kSnapBlock;
    const unsigned pblocks = (unsigned)std::min<int64_t>(units, (int64_t)p->n_cu * 32);
    const PairTable pt = make_pair_table(p->model.tab);
    SnapDepArgs da;
    std::memset(&da, 0, sizeof(da));
    if (keys_to) da = *keys_to;
#define BFGX_SNAP_LAUNCH(DIM, KEYS)                                                                                                               \
    hipLaunchKernelGGL((snap_displace_kernel<DIM, KEYS>), dim3(pblocks), dim3(256), 0, s, pt, g, n_part, px, py, pz, (const SnapHaloRec *)p->recs, \
                       (const uint32_t *)p->bitmap, (const int32_t *)p->start, (const SnapEntry *)p->entries, x_out, y_out, z_out, p->flags,      \
                       p->pairs, sin, sout, da)
    if (g.ndim == 3) { if (keys_to) BFGX_SNAP_LAUNCH(3, true); else BFGX_SNAP_LAUNCH(3, false); }
    else { if (keys_to) BFGX_SNAP_LAUNCH(2, true); else BFGX_SNAP_LAUNCH(2, false); }
#undef BFGX_SNAP_LAUNCH
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

static int snap_finish_stage(bfgx_snapshot_plan *p, int64_t *n_pairs_host)
{
    hipStream_t s = p->stream;
    int32_t flags = 0;
    unsigned long long np = 0;
    HIP_TRY(hipMemcpyAsync(&flags, p->flags, sizeof(flags), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&np, p->pairs, sizeof(np), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (flags & 2) return fail(BFGX_ERR_INVALID, "particle coordinates must lie in [0, L] (scipy's periodic KDTree refuses such data too)");
    if (n_pairs_host) *n_pairs_host = (int64_t)np;
    return BFGX_OK;
}

int bfgx_snapshot_displace_device(bfgx_snapshot_plan *p, const bfgx_grid_catalog *halos, int64_t n_part, const double *px, const double *py,
                                  const double *pz, double *x_out, double *y_out, double *z_out, int64_t *n_pairs_host)
{
    if (!p || !halos || !x_out || !y_out) return fail(BFGX_ERR_INVALID, "NULL argument");
    const SnapGeom &g = p->geom;
    if (n_part < 0) return fail(BFGX_ERR_INVALID, "bad particle count / catalog larger than the plan's max_halos");
    if (n_part > 0 && (!px || !py || (g.ndim == 3 && (!pz || !z_out)))) return fail(BFGX_ERR_INVALID, "snapshot column pointer is NULL");
    if (int rc = snap_lists_stage(p, halos)) return rc;
    if (int rc = snap_displace_stage(p, n_part, px, py, pz, 1, x_out, y_out, z_out, 1)) return rc;
    return snap_finish_stage(p, n_pairs_host);
}

// BaryonifySnapshot.process() (SnapshotRunner.py:173-262) followed by ParticleSnapshot.make_map(n_grid) (io.py:622-670) for a caller who
// wants the MAP of the displaced particles, not the particles: the displacement kernel writes the deposit's 4-byte sort keys and the
// per-chunk bucket histograms itself, and the two-level counting sort + tile pass of bfgx_deposit.hpp carry on from there.  The halo
// lists of the plan are in place (snap_lists_stage); stride = doubles between consecutive particles of the columns (fields of records).
static int snap_displace_deposit_stage(bfgx_snapshot_plan *p, int64_t n_part, const double *px, const double *py, const double *pz, const double *mass,
                                       int64_t stride, int32_t n_grid, const double *edges_dev, double *map_out_dev)
{
    DepKeysBy keys_by = [&](const DepGeom &dg, uint32_t *keys, int32_t *wg, unsigned chunks) {
        SnapDepArgs da;
        std::memset(&da, 0, sizeof(da));
        da.dg = dg; da.edges = edges_dev; da.keys = keys; da.wg_hist = wg; da.nchunks = (int32_t)chunks;
        return snap_displace_stage(p, n_part, px, py, pz, stride, nullptr, nullptr, nullptr, 1, &da);
    };
    return deposit_impl(p->device, (void *)p->stream, p->geom.ndim, n_part, px, py, pz, mass, n_grid, edges_dev, 0, n_grid, map_out_dev, nullptr, nullptr,
                        nullptr, stride, &keys_by);
}

int bfgx_snapshot_displace_deposit_device(bfgx_snapshot_plan *p, const bfgx_grid_catalog *halos, int64_t n_part, const double *px, const double *py,
                                          const double *pz, const double *mass, int32_t n_grid, const double *edges_dev, double *map_out_dev,
                                          int64_t *n_pairs_host)
{
    if (!p || !halos || !edges_dev || !map_out_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    const SnapGeom &g = p->geom;
    if (n_part < 0 || n_grid < 1) return fail(BFGX_ERR_INVALID, "bad particle count / grid size");
    if (n_part > 0 && (!px || !py || (g.ndim == 3 && !pz))) return fail(BFGX_ERR_INVALID, "snapshot column pointer is NULL");
    if (int rc = snap_lists_stage(p, halos)) return rc;
    if (int rc = snap_displace_deposit_stage(p, n_part, px, py, pz, mass, 1, n_grid, edges_dev, map_out_dev)) return rc;
    return snap_finish_stage(p, n_pairs_host);
}

int bfgx_baryonify_snapshot_device(int device, void *hip_stream, const bfgx_grid_catalog *halos, const bfgx_model *model,
                                   const bfgx_snapshot *snap, double *x_out, double *y_out, double *z_out, int64_t *n_pairs_host)
{
    if (!halos || !model || !snap || !x_out || !y_out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (snap->n < 0 || halos->n < 0) return fail(BFGX_ERR_INVALID, "bad snapshot / catalog sizes");
    bfgx_snapshot_plan *p = nullptr;
    if (int rc = bfgx_snapshot_plan_create(device, hip_stream, model, snap->ndim, snap->L, snap->redshift, halos->n, &p)) return rc;
    struct Guard { bfgx_snapshot_plan *p; ~Guard() { bfgx_snapshot_plan_destroy(p); } } guard{p};
    return bfgx_snapshot_displace_device(p, halos, snap->n, snap->x, snap->y, snap->z, x_out, y_out, z_out, n_pairs_host);
}

int bfgx_baryonify_snapshot(const bfgx_grid_catalog *halos, const bfgx_model *model, const bfgx_snapshot *snap, double *x_out, double *y_out,
                            double *z_out, const bfgx_opts *opts, bfgx_stats *stats)
{
    if (!halos || !model || !snap || !x_out || !y_out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (snap->ndim != 2 && snap->ndim != 3) return fail(BFGX_ERR_INVALID, "snapshot ndim must be 2 or 3");
    if (snap->n < 0) return fail(BFGX_ERR_INVALID, "negative particle count");
    const int device = opts ? opts->device : 0;
    if (int rc = select_device(device)) return rc;
    GridHostCatalog hc;
    Timer t;
    t.start(nullptr);
    if (int rc = hc.upload(halos, snap->ndim, 0, nullptr)) return rc;
    DevBuf dx, dy, dz, ox, oy, oz;
    const size_t nb = sizeof(double) * (size_t)snap->n;
    if (dx.up(snap->x, nb) || dy.up(snap->y, nb) || (snap->ndim == 3 && dz.up(snap->z, nb)) || ox.up(nullptr, nb) || oy.up(nullptr, nb) ||
        (snap->ndim == 3 && oz.up(nullptr, nb)))
        return fail(BFGX_ERR_HIP, "hipMalloc / copy(particles) failed");
    const double ms_h2d = t.lap(nullptr);
    bfgx_snapshot ds = *snap;
    ds.x = dx.as<double>(); ds.y = dy.as<double>(); ds.z = snap->ndim == 3 ? dz.as<double>() : nullptr;
    int64_t npairs = 0;
    if (int rc = bfgx_baryonify_snapshot_device(device, nullptr, &hc.d, model, &ds, ox.as<double>(), oy.as<double>(),
                                                snap->ndim == 3 ? oz.as<double>() : nullptr, &npairs)) return rc;
    const double ms_k = t.lap(nullptr);
    HIP_TRY(hipMemcpy(x_out, ox.p, nb, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(y_out, oy.p, nb, hipMemcpyDeviceToHost));
    if (snap->ndim == 3) HIP_TRY(hipMemcpy(z_out, oz.p, nb, hipMemcpyDeviceToHost));
    const double ms_d2h = t.stop(nullptr);
    fill_stats(stats, nullptr, npairs, ms_h2d, ms_k, ms_d2h);
    return BFGX_OK;
}

}  // extern "C"

namespace {

// cache of the records entries: plan + one device buffer for the particle records per (device, box, model)
struct RecordsEntry : CacheEntry<bfgx_snapshot_plan> {
    PoolBuf rec;
    GridHostCatalog hc;
};
PlanCache<RecordsEntry, 2> g_snaps;
constexpr int kSnapChunksMax = 64;

// the cached plan + device record buffer (of at least `bytes`) of the records entries for (device, box, redshift, model); the caller holds
// g_snaps.mu and has validated the model
int snap_acquire(int device, const bfgx_model *model, int32_t ndim, double L, double redshift, int64_t nhalo, size_t bytes, RecordsEntry **out)
{
    CacheKey key = model_key(device, model);
    const int ncells = snapshot_cells(ndim);                 // (BFGX_SNAP_CELLS: a plan is built for one cell grid)
    key.add(ndim); key.add(L); key.add(redshift); key.add(ncells);
    auto make = [&](int64_t cap, bfgx_snapshot_plan **p) { return bfgx_snapshot_plan_create(device, nullptr, model, ndim, L, redshift, cap, p); };
    auto setup = [&](RecordsEntry *e) -> int { return e->rec.need(bytes, 8, 0) ? alloc_fail("particle records") : BFGX_OK; };
    return g_snaps.acquire(key, device, nhalo, make, setup, out);
}

// how many chunks n records of `bytes` in all travel in: pieces of at least 16 MB, at most kSnapChunksMax (BFGX_PIPE_CHUNKS sets the count)
int snap_chunk_count(int64_t n, size_t bytes, const PipeKnobs &knobs)
{
    int C = (int)std::min<size_t>(kSnapChunksMax, std::max<size_t>(1, bytes / ((size_t)16 << 20)));
    if (knobs.stage) C = std::max(1, std::min(kSnapChunksMax, knobs.chunks));
    return (knobs.off || n < C) ? 1 : C;
}
int64_t snap_chunk_first(int64_t n, int C, int c) { return (int64_t)(((__int128)n * c) / C); }       // the first record of chunk c of C

}  // namespace

extern "C" {

int bfgx_baryonify_snapshot_records(const bfgx_grid_catalog *halos, const bfgx_model *model, int32_t ndim, double L, double redshift, int64_t n,
                                    const void *records_in, void *records_out, int32_t itemsize, int32_t off_x, int32_t off_y, int32_t off_z,
                                    const bfgx_opts *opts, bfgx_stats *stats)
{
    if (!halos || !model || (n > 0 && (!records_in || !records_out))) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (ndim != 2 && ndim != 3) return fail(BFGX_ERR_INVALID, "snapshot ndim must be 2 or 3");
    if (n < 0 || halos->n < 0) return fail(BFGX_ERR_INVALID, "bad snapshot / catalog sizes");
    if (itemsize < 16 || itemsize % 8 || off_x < 0 || off_y < 0 || off_x % 8 || off_y % 8 || off_x + 8 > itemsize || off_y + 8 > itemsize ||
        (ndim == 3 && (off_z < 0 || off_z % 8 || off_z + 8 > itemsize)))
        return fail(BFGX_ERR_INVALID, "records must be a multiple of 8 bytes with 8-byte aligned float64 coordinate fields");
    if (int rc = validate_model(model)) return rc;
    const int device = entry_opts(opts).device;
    std::lock_guard<std::mutex> lk(g_snaps.mu);
    RecordsEntry *e = nullptr;
    if (int rc = snap_acquire(device, model, ndim, L, redshift, halos->n, (size_t)n * (size_t)itemsize, &e)) return rc;
    bfgx_snapshot_plan *p = e->plan;
    const size_t bytes = (size_t)n * (size_t)itemsize;
    hipStream_t s = p->stream;
    OneShotCall call(&p->stream, e);
    if (int rc = call.mark(0, s)) return rc;
    if (int rc = e->hc.upload(halos, ndim, 0, s)) return rc;
    // ---- the records travel in chunks of at least 16 MB: a chunk is displaced IN PLACE on the device as soon as it has arrived (the halo
    // lists are built underneath the first uploads) and travels back while the next ones arrive.  Page-locked on both sides for the call.
    const PipeKnobs knobs = pipe_knobs();
    int C = snap_chunk_count(n, bytes, knobs);
    if (C > 1 && !call.open(records_in, bytes, records_out, bytes, knobs.stage)) C = 1;      // pageable memory: one piece
    const char *src = (C > 1) ? call.src<char>() : (const char *)records_in;
    char *dst = (C > 1) ? call.dst<char>() : (char *)records_out;
    if (int rc = e->pools(C, C)) return rc;
    char *d_rec = (char *)e->rec.p;
    for (int c = 0; c < C; ++c) {
        const int64_t lo = snap_chunk_first(n, C, c), cnt = snap_chunk_first(n, C, c + 1) - lo;
        if (cnt > 0) HIP_TRY(hipMemcpyAsync(d_rec + (size_t)lo * itemsize, src + (size_t)lo * itemsize, (size_t)cnt * itemsize, hipMemcpyHostToDevice, e->up));
        HIP_TRY(hipEventRecord(e->ev_up[c], e->up));
    }
    if (int rc = call.mark(1, e->up)) return rc;
    if (int rc = snap_lists_stage(p, &e->hc.d)) return rc;
    const int64_t stride = itemsize / 8;
    for (int c = 0; c < C; ++c) {
        const int64_t lo = snap_chunk_first(n, C, c), cnt = snap_chunk_first(n, C, c + 1) - lo;
        HIP_TRY(hipStreamWaitEvent(s, e->ev_up[c], 0));
        double *base = (double *)(d_rec + (size_t)lo * itemsize);
        double *cx = base + off_x / 8, *cy = base + off_y / 8, *cz = ndim == 3 ? base + off_z / 8 : nullptr;
        if (int rc = snap_displace_stage(p, cnt, cx, cy, cz, stride, cx, cy, cz, stride)) return rc;
        HIP_TRY(hipEventRecord(e->ev_k[c], s));
        HIP_TRY(hipStreamWaitEvent(e->down, e->ev_k[c], 0));
        if (cnt > 0) HIP_TRY(hipMemcpyAsync(dst + (size_t)lo * itemsize, d_rec + (size_t)lo * itemsize, (size_t)cnt * itemsize, hipMemcpyDeviceToHost, e->down));
    }
    if (int rc = call.mark(2, s)) return rc;
    int64_t npairs = 0;
    const int rc_fin = snap_finish_stage(p, &npairs);
    HIP_TRY(hipStreamSynchronize(e->down));
    HIP_TRY(hipStreamSynchronize(e->up));
    if (rc_fin) return rc_fin;
    if (C > 1) call.commit();
    if (int rc = call.mark(3, e->down)) return rc;
    return call.finish(stats, nullptr, npairs);
}

int bfgx_baryonify_snapshot_records_map(const bfgx_grid_catalog *halos, const bfgx_model *model, int32_t ndim, double L, double redshift, int64_t n,
                                        const void *records_in, int32_t itemsize, int32_t off_x, int32_t off_y, int32_t off_z, int32_t off_mass,
                                        int32_t n_grid, const double *edges, double *map_out, const bfgx_opts *opts, bfgx_stats *stats)
{
    // ParticleSnapshot(cat = BaryonifySnapshot(...).process()).make_map(n_grid) in ONE call (SnapshotRunner.py:173-262, io.py:622-670): the
    // records go up once, the displaced coordinates exist only as sort keys of the deposit, the map comes back -- the two-call route
    // downloads the displaced records and uploads them again
    if (!halos || !model || (n > 0 && !records_in) || !edges || !map_out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (ndim != 2 && ndim != 3) return fail(BFGX_ERR_INVALID, "snapshot ndim must be 2 or 3");
    if (n < 0 || halos->n < 0 || n_grid < 1) return fail(BFGX_ERR_INVALID, "bad snapshot / catalog / grid sizes");
    auto bad = [&](int off) { return off < 0 || off % 8 || off + 8 > itemsize; };
    if (itemsize < 16 || itemsize % 8 || bad(off_x) || bad(off_y) || (ndim == 3 && bad(off_z)) || (off_mass >= 0 && bad(off_mass)))
        return fail(BFGX_ERR_INVALID, "records must be a multiple of 8 bytes with 8-byte aligned float64 fields");
    for (int i = 1; i <= n_grid; ++i) if (!(edges[i] > edges[i - 1])) return fail(BFGX_ERR_INVALID, "edges must be strictly ascending");
    if (int rc = validate_model(model)) return rc;
    const int device = entry_opts(opts).device;
    std::lock_guard<std::mutex> lk(g_snaps.mu);
    RecordsEntry *e = nullptr;
    if (int rc = snap_acquire(device, model, ndim, L, redshift, halos->n, (size_t)n * (size_t)itemsize, &e)) return rc;
    bfgx_snapshot_plan *p = e->plan;
    std::lock_guard<std::mutex> lk2(g_deprec_mu);
    DepRecBuf &b = g_deprec[device];
    size_t ntot = 1;
    for (int d = 0; d < ndim; ++d) ntot *= (size_t)n_grid;
    const size_t rbytes = (size_t)n * (size_t)itemsize, mbytes = ntot * sizeof(double), ebytes = sizeof(double) * (size_t)(n_grid + 1);
    if (b.map.need(mbytes, 8, 8) || b.edges.need(ebytes + 16, 8, 8)) return alloc_fail("map");
    hipStream_t s = p->stream;
    OneShotCall call(&p->stream, e);
    if (int rc = call.mark(0, s)) return rc;
    if (int rc = e->hc.upload(halos, ndim, 0, s)) return rc;
    (void)call.open_in(records_in, rbytes, false);           // (large arrays are page-locked for the call; small ones go up from pageable memory)
    (void)call.open_out(map_out, mbytes, false);
    // the records go up on their own stream while the halo lists are built
    HIP_TRY(hipMemcpyAsync(b.edges.p, edges, ebytes, hipMemcpyHostToDevice, e->up));
    if (rbytes) HIP_TRY(hipMemcpyAsync(e->rec.p, records_in, rbytes, hipMemcpyHostToDevice, e->up));
    if (int rc = e->pools(1, 0)) return rc;
    HIP_TRY(hipEventRecord(e->ev_up[0], e->up));
    if (int rc = call.mark(1, e->up)) return rc;
    if (int rc = snap_lists_stage(p, &e->hc.d)) return rc;
    HIP_TRY(hipStreamWaitEvent(s, e->ev_up[0], 0));
    const double *base = (const double *)e->rec.p;
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
    if (int rc = snap_displace_deposit_stage(p, n, base + off_x / 8, base + off_y / 8, ndim == 3 ? base + off_z / 8 : nullptr,
                                             off_mass >= 0 ? base + off_mass / 8 : nullptr, stride, n_grid, (const double *)b.edges.p, (double *)b.map.p)) return rc;
    if (int rc = call.mark(2, s)) return rc;
    HIP_TRY(hipMemcpyAsync(map_out, b.map.p, mbytes, hipMemcpyDeviceToHost, s));
    int64_t npairs = 0;
    if (int rc = snap_finish_stage(p, &npairs)) return rc;                      // (synchronises the stream: the map has arrived)
    HIP_TRY(hipStreamSynchronize(e->up));
    if (nanflag) return fail(BFGX_ERR_ASSERT, "If you want to make a map, provide a value for the particle mass");
    return call.finish(stats, nullptr, npairs);              // (no third phase: the map comes back underneath snap_finish_stage)
}

}  // extern "C"
