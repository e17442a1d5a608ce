// bfgx_grid_api.inc -- C ABI of the regular-grid path (included at the end of bfgx_api.hip: one translation unit): the grid plan, its
// halo-owned and cell-owned device entries, the one-shot grid entries and bfgx_regrid_pixels.  The particle deposit follows in
// bfgx_deposit_api.inc, the 3-D FFT / P(k) in bfgx_fft_api.inc.
// Declarations and the reference lines each entry point replaces: include/bfgx.h, "regular-grid path".

struct bfgx_grid_plan {
    int device = 0;
    hipStream_t stream = nullptr;
    GridGeom geom;
    DevModel model;
    int NC = 4;
    int64_t max_halos = 0;
    DevList mem;
    GridHaloRec *recs = nullptr;
    int32_t *chunk_halo = nullptr;        // work-item table (regrown on demand)
    int64_t capacity = 0;
    int32_t *counters = nullptr;          // [0] items, [1] flags
    unsigned long long *pair_total = nullptr;
    double *block_sums = nullptr;         // [ceil(ntot / 256)][2] per-workgroup sums of the regrid
    int n_cu = 256;
    // cell-owned path (bfgx_grid_baryonify_device), allocated by its first call: per-block halo lists
    int64_t nblk = 0, list_capacity = 0;
    int nscan_blocks = 0;
    int32_t *blk_count = nullptr, *blk_start = nullptr, *blk_bsum = nullptr, *blk_list = nullptr;   // count / start: [nblk + 1]
    int64_t *blk_total = nullptr;
    int32_t *blk_nz = nullptr, *blk_nzn = nullptr;   // the blocks that list a halo (compacted) and their number
    int32_t *axis0_flag = nullptr;        // device word the gather kernel sets when a cell moves further than axis0_limit cells along the first array axis
    float axis0_limit = 3.0e38f;          // (set by the streamed host entry for the duration of its gathers; 3e38: no check)
    double *blk_sums = nullptr;           // [nblk][3]: sum of sources, sum of deposits, contributing pairs
    KernelEvents events;                  // optional per-kernel HIP-event timing (bfgx_grid_plan_timing_*)
};

namespace {

using GridTimer = KernelTimerT<bfgx_grid_plan>;

// The grid family's kernels are templates over the corner count of the table read-out (4, 8 or 16) and over the grid's dimensions (2 or 3):
// f receives the run-time value as a tag, [&](auto nc) { ... kernel<decltype(nc)::value> ... }
template <int V> using GridTag = std::integral_constant<int, V>;
template <class F> auto grid_nc(int NC, F &&f) { return NC == 4 ? f(GridTag<4>{}) : NC == 8 ? f(GridTag<8>{}) : f(GridTag<16>{}); }
template <class F> auto grid_dim(int ndim, F &&f) { return ndim == 3 ? f(GridTag<3>{}) : f(GridTag<2>{}); }

int validate_grid(const bfgx_grid *g)
{
    if (!g || !g->bins) return fail(BFGX_ERR_INVALID, "NULL grid");
    if (g->ndim != 2 && g->ndim != 3) return fail(BFGX_ERR_INVALID, "grid ndim must be 2 or 3");
    if (g->npix < 5 || g->npix > 4096) return fail(BFGX_ERR_INVALID, "grid npix must be in [5, 4096]");
    if (g->ndim == 3 && g->npix > 1290) return fail(BFGX_ERR_INVALID, "3D grids above 1290^3 exceed 32-bit pixel offsets * 3");
    for (int i = 1; i < g->npix; ++i)
        if (!(g->bins[i] > g->bins[i - 1])) return fail(BFGX_ERR_INVALID, "grid bins must be strictly ascending");
    if (!(g->redshift > -1.0)) return fail(BFGX_ERR_INVALID, "grid redshift must be > -1");
    return BFGX_OK;
}

int launch_grid_prep(bfgx_grid_plan *p, const bfgx_grid_catalog *c, int mode)
{
    HIP_TRY(hipMemsetAsync(p->counters, 0, 2 * sizeof(int32_t), p->stream));
    if (c->n == 0) return BFGX_OK;
    GridCatalog gc;
    gc.n = c->n; gc.M = c->M; gc.x = c->x; gc.y = c->y; gc.z = c->z; gc.lnM = c->lnM; gc.rmat = c->rmat;
    for (int k = 0; k < BFGX_MAX_EXTRA; ++k) gc.extra[k] = c->extra[k];
    const int blocks = (int)((c->n + kGridBlock - 1) / kGridBlock);
    GridTimer kt(p, BFGX_K_PREP);
    grid_nc(p->NC, [&](auto nc) {
        hipLaunchKernelGGL((grid_prep_kernel<decltype(nc)::value>), dim3(blocks), dim3(kGridBlock), 0, p->stream, p->model, p->geom, gc, mode,
                           p->recs, p->chunk_halo, p->capacity, p->counters);
    });
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

template <int MODE>
int launch_grid_scatter(bfgx_grid_plan *p, int blocks, double *out)
{
    GridTimer kt(p, MODE == 0 ? BFGX_K_OFFSETS : BFGX_K_PAINT);
    grid_dim(p->geom.ndim, [&](auto dim) { grid_nc(p->NC, [&](auto nc) {
        hipLaunchKernelGGL((grid_scatter_kernel<decltype(dim)::value, MODE, decltype(nc)::value>), dim3(blocks), dim3(kGridBlock), 0, p->stream,
                           make_pair_table(p->model.tab), p->geom, p->recs, p->chunk_halo, p->counters, out, p->pair_total);
    }); });
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

// what every entry that takes a catalog asks of it: it fits the plan, the columns the grid and the table need are there
int grid_check_columns(const bfgx_grid_plan *p, const bfgx_grid_catalog *c)
{
    if (c->n < 0 || c->n > p->max_halos) return fail(BFGX_ERR_INVALID, "catalog size %lld exceeds plan max_halos %lld",
                                                     (long long)c->n, (long long)p->max_halos);
    const int nex = p->model.tab.ndim - 3;
    if (c->n > 0 && (!c->M || !c->x || !c->y || (p->geom.ndim == 3 && !c->z))) return fail(BFGX_ERR_INVALID, "catalog column pointer is NULL");
    for (int k = 0; k < nex; ++k) if (c->n > 0 && !c->extra[k]) return fail(BFGX_ERR_INVALID, "catalog misses a property column of the table");
    if (c->rmat && p->geom.ndim == 3) return fail(BFGX_ERR_UNSUPPORTED, "use_ellipticity is not implemented for 3D maps");
    return BFGX_OK;
}

// the pair count of the call so far, on the host (synchronises the stream)
int read_pair_total(hipStream_t stream, const unsigned long long *dev, int64_t *out)
{
    unsigned long long np = 0;
    HIP_TRY(hipMemcpyAsync(&np, dev, sizeof(np), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *out = (int64_t)np;
    return BFGX_OK;
}

// prep (+ regrowth of the work-item table) + scatter; mode 0 = offsets, 1 = paint
int grid_halo_loop(bfgx_grid_plan *p, const bfgx_grid_catalog *c, int mode, double *out, int64_t *n_pairs_host)
{
    if (!p || !c || !out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = grid_check_columns(p, c)) return rc;
    HIP_TRY(hipSetDevice(p->device));
    const size_t out_bytes = sizeof(double) * (size_t)(p->geom.ntot / p->geom.npix * p->geom.slab_n) * (mode == 0 ? p->geom.ndim : 1);
    HIP_TRY(hipMemsetAsync(out, 0, out_bytes, p->stream));
    HIP_TRY(hipMemsetAsync(p->pair_total, 0, sizeof(unsigned long long), p->stream));
    int32_t cnt[2] = {0, 0};
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (int rc = launch_grid_prep(p, c, mode)) return rc;
        HIP_TRY(hipMemcpyAsync(cnt, p->counters, sizeof(cnt), hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        if (cnt[0] < 0) return fail(BFGX_ERR_INVALID, "more than 2^31 work items (%d-pixel chunks): catalog too large for one call", kGridChunk);
        if ((int64_t)cnt[0] <= p->capacity) break;
        // the work-item table was too small: grow it and redo the (deterministic) preparation
        if (int rc = grow_list(p->mem, p->chunk_halo, p->capacity, (int64_t)cnt[0])) return rc;
    }
    if (cnt[1] & 1) return fail(BFGX_ERR_ASSERT, "Halo offsets are larger than res (Map2DRunner.py:516)");
    if (cnt[0] > 0) {
        const int blocks = (int)std::min<int64_t>(cnt[0], (int64_t)p->n_cu * 8);
        if (int rc = mode == 0 ? launch_grid_scatter<0>(p, blocks, out) : launch_grid_scatter<1>(p, blocks, out)) return rc;
    }
    return n_pairs_host ? read_pair_total(p->stream, p->pair_total, n_pairs_host) : BFGX_OK;
}

struct GridHostCatalog {
    PoolBuf cols[4 + 2 + BFGX_MAX_EXTRA];          // (kept by the cached one-shot entries: a warm call re-uses them)
    bfgx_grid_catalog d;
    int upload(const bfgx_grid_catalog *h, int ndim, int nex, hipStream_t s)
    {
        std::memset(&d, 0, sizeof(d));
        d.n = h->n;
        const double *src[4 + 2 + BFGX_MAX_EXTRA] = {h->M, h->x, h->y, ndim == 3 ? h->z : nullptr, h->lnM, h->rmat};
        size_t width[4 + 2 + BFGX_MAX_EXTRA] = {1, 1, 1, 1, 1, 4};
        const double **dst[4 + 2 + BFGX_MAX_EXTRA] = {&d.M, &d.x, &d.y, &d.z, &d.lnM, &d.rmat};
        for (int k = 0; k < BFGX_MAX_EXTRA; ++k) { src[6 + k] = h->extra[k]; width[6 + k] = 1; dst[6 + k] = &d.extra[k]; }
        for (int i = 0; i < 6 + nex; ++i) {
            if (!src[i]) continue;
            const size_t bytes = sizeof(double) * (size_t)h->n * width[i];
            if (cols[i].need(std::max<size_t>(bytes, 8))) return alloc_fail("catalog");
            if (h->n > 0) HIP_TRY(hipMemcpyAsync(cols[i].p, src[i], bytes, hipMemcpyHostToDevice, s));
            *dst[i] = (const double *)cols[i].p;
        }
        return BFGX_OK;
    }
};

}  // namespace

extern "C" {

int bfgx_grid_plan_create(int device, void *hip_stream, const bfgx_grid *grid, int64_t max_halos, const bfgx_model *model,
                          bfgx_grid_plan **out)
{
    if (!grid || !model || !out) return fail(BFGX_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (int rc = validate_grid(grid)) return rc;
    if (max_halos < 0) return fail(BFGX_ERR_INVALID, "max_halos < 0");
    if (int rc = validate_model(model)) return rc;
    if (model->table.ndim > 5) return fail(BFGX_ERR_UNSUPPORTED, "the regular-grid runners read out tables with at most 2 property axes (the HEALPix shell runners take %d)", BFGX_MAX_EXTRA);
    if (bfgx_device_count() <= 0) return fail(BFGX_ERR_NO_DEVICE, "no HIP device visible: libbfgx has no CPU fallback");
    HIP_TRY(hipSetDevice(device));
    bfgx_grid_plan *p = new bfgx_grid_plan();
    p->device = device;
    p->stream = (hipStream_t)hip_stream;
    p->max_halos = max_halos;
    auto bail = [&](int rc) { bfgx_grid_plan_destroy(p); return rc; };
    if (int rc = upload_model(p->mem, p->stream, model, false, p->model, p->NC)) return bail(rc);
    {
        GridGeom &g = p->geom;
        if (int rc = owned_upload(p->mem, p->stream, grid->bins, (size_t)grid->npix, g.bins)) return bail(rc);
        if (hipStreamSynchronize(p->stream) != hipSuccess) return bail(fail(BFGX_ERR_HIP, "stream sync failed"));
        g.ndim = grid->ndim; g.npix = grid->npix;
        g.res = grid->bins[1] - grid->bins[0];                          // io.py:469
        double bmax = grid->bins[0];
        for (int i = 1; i < grid->npix; ++i) bmax = std::max(bmax, grid->bins[i]);
        g.half_box = bmax / 2;                                          // Map2DRunner.py:488
        g.a = 1.0 / (1.0 + grid->redshift);                             // :485
        g.ntot = 1;
        for (int d = 0; d < grid->ndim; ++d) g.ntot *= grid->npix;
        g.slab_lo = 0; g.slab_n = grid->npix;
    }
    p->capacity = 4 * max_halos + 65536;
    if (const char *e = std::getenv("BFGX_GRID_ITEM_CAP")) p->capacity = std::max<int64_t>(1, std::atoll(e));   // tests: force regrowth
    // (at least 2048 entries: the cell-owned pass keeps the per-workgroup sums of its copy kernel here)
    if (p->mem.alloc(p->block_sums, std::max<size_t>(2 * (size_t)((p->geom.ntot + 255) / 256), 2048))) return bail(alloc_fail("block sums"));
    if (p->mem.alloc(p->recs, (size_t)std::max<int64_t>(max_halos, 1)) || p->mem.alloc(p->chunk_halo, (size_t)p->capacity) ||
        p->mem.alloc(p->counters, 2) || p->mem.alloc(p->pair_total, 1))
        return bail(alloc_fail("grid workspace"));
    p->n_cu = device_cu_count(device);
    *out = p;
    return BFGX_OK;
}

void bfgx_grid_plan_destroy(bfgx_grid_plan *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    (void)hipStreamSynchronize(p->stream);
    p->mem.release();
    p->events.destroy();
    delete p;
}

int bfgx_grid_offsets_device(bfgx_grid_plan *p, const bfgx_grid_catalog *cat, double *offsets_dev, int64_t *n_pairs_host)
{
    if (p && p->model.tab.logv) return fail(BFGX_ERR_INVALID, "the plan holds a log (profile) table: use bfgx_grid_paint_device");
    return grid_halo_loop(p, cat, 0, offsets_dev, n_pairs_host);
}

int bfgx_grid_paint_device(bfgx_grid_plan *p, const bfgx_grid_catalog *cat, double *map_out_dev, int64_t *n_pairs_host)
{
    if (p && !p->model.tab.logv) return fail(BFGX_ERR_INVALID, "the plan holds a displacement table: use bfgx_grid_offsets_device");
    return grid_halo_loop(p, cat, 1, map_out_dev, n_pairs_host);
}

int bfgx_grid_plan_set_slab(bfgx_grid_plan *p, int32_t plane_lo, int32_t plane_n)
{
    if (!p) return fail(BFGX_ERR_INVALID, "NULL plan");
    if (plane_lo < 0 || plane_n < 1 || plane_lo + plane_n > p->geom.npix) return fail(BFGX_ERR_INVALID, "slab [%d, %d) outside the grid", plane_lo, plane_lo + plane_n);
    p->geom.slab_lo = plane_lo; p->geom.slab_n = plane_n;
    return BFGX_OK;
}

int bfgx_grid_regrid_slab_device(bfgx_grid_plan *p, const double *map_in, const double *offsets, int32_t apron, double *map_out,
                                 double *sums_dev, int32_t *missed_dev)
{
    if (!p || !map_in || !offsets || !map_out) return fail(BFGX_ERR_INVALID, "NULL argument");
    const GridGeom &g = p->geom;
    if (apron < 0 || g.slab_n + 2 * (int64_t)apron > g.npix) return fail(BFGX_ERR_INVALID, "apron of %d planes does not fit the grid", apron);
    if (g.slab_n == g.npix && apron != 0) return fail(BFGX_ERR_INVALID, "a plan that owns the whole grid has no apron");
    HIP_TRY(hipSetDevice(p->device));
    const int64_t plane_cells = g.ntot / g.npix, ntot = plane_cells * g.slab_n;
    HIP_TRY(hipMemsetAsync(map_out, 0, sizeof(double) * (size_t)(plane_cells * (g.slab_n + 2 * apron)), p->stream));
    const unsigned blocks = (unsigned)((ntot + 255) / 256);
    const SlabWin sw{g.slab_lo, g.slab_n, apron};
    {
        GridTimer kt(p, BFGX_K_REGRID);
        double *bs = sums_dev ? p->block_sums : nullptr;
        grid_dim(g.ndim, [&](auto dim) {
            hipLaunchKernelGGL((grid_regrid_kernel<decltype(dim)::value>), dim3(blocks), dim3(256), 0, p->stream, g.npix, ntot, offsets, map_in, map_out, bs, sw, missed_dev);
        });
        HIP_TRY(hipGetLastError());
    }
    if (sums_dev) {         // the regrid left per-workgroup {sum of source values, sum of deposits}: no second pass over the maps
        GridTimer kt(p, BFGX_K_SUM);
        hipLaunchKernelGGL(sum_blocks_kernel, dim3(256), dim3(256), 0, p->stream, (int64_t)blocks, (const double *)p->block_sums, sums_dev);
        HIP_TRY(hipGetLastError());
    }
    return BFGX_OK;
}

int bfgx_grid_regrid_device(bfgx_grid_plan *p, const double *map_in, const double *offsets, double *map_out, double *sums_dev)
{
    if (p && p->geom.slab_n != p->geom.npix) return fail(BFGX_ERR_INVALID, "the plan owns a slab: use bfgx_grid_regrid_slab_device");
    return bfgx_grid_regrid_slab_device(p, map_in, offsets, 0, map_out, sums_dev, nullptr);
}

}  // extern "C"

namespace {

// block-id ranges whose non-empty blocks are compacted (and gathered) separately: blk_nz[lo ..) holds those of range [lo, hi).  One range
// = the whole grid; the streamed host entry gathers the grid in ranges of block rows while the map is still arriving
constexpr int kGatherRangesMax = 64;
struct GatherRanges { int n = 0; int64_t lo[kGatherRangesMax], hi[kGatherRangesMax]; int32_t nnz[kGatherRangesMax]; };

int gather_workspace(bfgx_grid_plan *p)
{
    if (p->blk_count) return BFGX_OK;
    const GridGeom &g = p->geom;
    const int nbk = gather_blocks_per_axis(g.npix, g.ndim == 3 ? GatherBlk<3>::S : GatherBlk<2>::S);
    p->nblk = (g.ndim == 3) ? (int64_t)nbk * nbk * nbk : (int64_t)nbk * nbk;
    p->nscan_blocks = scan_block_count(p->nblk + 1);
    p->list_capacity = 16 * p->max_halos + 65536;
    if (const char *e = std::getenv("BFGX_GRID_ITEM_CAP")) p->list_capacity = std::max<int64_t>(1, std::atoll(e));   // tests: force regrowth
    // (blk_count, which marks the workspace as present, last: a failure part-way leaves the next call to try again)
    int32_t *count = nullptr;
    DevList &mem = p->mem;
    if (mem.alloc(count, (size_t)(p->nblk + 1)) || mem.alloc(p->blk_start, (size_t)(p->nblk + 1)) || mem.alloc(p->blk_bsum, (size_t)p->nscan_blocks) ||
        mem.alloc(p->blk_total, 1) || mem.alloc(p->blk_sums, 3 * (size_t)p->nblk) || mem.alloc(p->blk_list, (size_t)p->list_capacity) ||
        mem.alloc(p->blk_nz, (size_t)p->nblk) || mem.alloc(p->blk_nzn, (size_t)(kGatherRangesMax + 4)))
        return alloc_fail("block lists");
    p->blk_count = count;
    p->axis0_flag = p->blk_nzn + kGatherRangesMax;           // (the streamed host entry: a cell moved beyond what its plane ranges allow)
    return BFGX_OK;
}

template <int FILL>
void launch_block_lists(bfgx_grid_plan *p, int64_t nh)
{
    grid_dim(p->geom.ndim, [&](auto dim) {
        hipLaunchKernelGGL((grid_block_lists_kernel<decltype(dim)::value, FILL>), dim3((unsigned)((nh + 256 / kWave - 1) / (256 / kWave))), dim3(256), 0, p->stream,
                           p->geom, nh, (const GridHaloRec *)p->recs, p->blk_count, (const int32_t *)p->blk_start, p->blk_list);
    });
}

void launch_gather(bfgx_grid_plan *p, const double *map_in, double *map_out, int64_t nnz, int64_t nz_off)
{
    const PairTable pt = make_pair_table(p->model.tab);
    grid_dim(p->geom.ndim, [&](auto dim) { grid_nc(p->NC, [&](auto nc) {
        hipLaunchKernelGGL((grid_gather_regrid_kernel<decltype(dim)::value, decltype(nc)::value>), dim3((unsigned)nnz), dim3(256), 0, p->stream, pt, p->geom,
                           (const GridHaloRec *)p->recs, (const int32_t *)p->blk_start, (const int32_t *)p->blk_list, (const int32_t *)p->blk_nz + nz_off,
                           map_in, map_out, p->blk_sums, p->axis0_limit, p->axis0_limit < 1.0e30f ? p->axis0_flag : (int32_t *)nullptr);
    }); });
}

}  // namespace

extern "C" {

// The cell-owned pass in stages, so that the streamed host entry can interleave them with the map's arrival:
//   grid_lists_stage   halo records, per-block halo lists, the non-empty blocks of every range compacted (needs the catalog only)
//   grid_copy_stage    map_out = map_in for a range of cells + partial sums (a cell that is not moved deposits into itself)
//   grid_gather_stage  halo loop + regrid of the moved cells for one range of blocks
//   grid_sums_stage    the two sums of the mass check, the pair count
static int grid_check_catalog(bfgx_grid_plan *p, const bfgx_grid_catalog *c)
{
    if (p->model.tab.logv) return fail(BFGX_ERR_INVALID, "the plan holds a log (profile) table: use bfgx_grid_paint_device");
    if (p->geom.slab_n != p->geom.npix) return fail(BFGX_ERR_INVALID, "the plan owns a slab: use the slab entry points");
    return grid_check_columns(p, c);
}

static int grid_lists_stage(bfgx_grid_plan *p, const bfgx_grid_catalog *c, GatherRanges &gr)
{
    hipStream_t s = p->stream;
    HIP_TRY(hipMemsetAsync(p->pair_total, 0, sizeof(unsigned long long), s));
    HIP_TRY(hipMemsetAsync(p->blk_count, 0, sizeof(int32_t) * (size_t)(p->nblk + 1), s));
    if (int rc = launch_grid_prep(p, c, 0)) return rc;                  // (its work-item table is not used here)
    int64_t total = 0;
    int32_t cnt[2] = {0, 0};
    {
        GridTimer kt(p, BFGX_K_BIN);
        if (c->n > 0) launch_block_lists<0>(p, c->n);
        exclusive_scan(s, p->nblk + 1, p->blk_count, p->blk_start, p->blk_bsum, p->blk_total);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemsetAsync(p->blk_count, 0, sizeof(int32_t) * (size_t)(p->nblk + 1), s));      // reused as the fill cursors
    // the gather kernel is launched over the blocks that list a halo only (a ball fills a few per cent of the grid: at 512^3 / 1e5 halos
    // three blocks in four list nothing and would pay the price of a workgroup to find that out); the others keep the copy of map_in
    HIP_TRY(hipMemsetAsync(p->blk_nzn, 0, sizeof(int32_t) * (kGatherRangesMax + 4), s));       // (+ axis0_flag)
    HIP_TRY(hipMemsetAsync(p->blk_sums, 0, sizeof(double) * 3 * (size_t)p->nblk, s));
    for (int r = 0; r < gr.n; ++r) {
        const int64_t nb = gr.hi[r] - gr.lo[r];
        if (nb <= 0) continue;
        hipLaunchKernelGGL(grid_nonempty_blocks_kernel, dim3((unsigned)std::min<int64_t>((nb + 255) / 256, 1024)), dim3(256), 0, s, gr.lo[r], gr.hi[r],
                           (const int32_t *)p->blk_start, p->blk_nz + gr.lo[r], p->blk_nzn + r);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(gr.nnz, p->blk_nzn, sizeof(int32_t) * (size_t)gr.n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&total, p->blk_total, sizeof(total), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(cnt, p->counters, sizeof(cnt), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (cnt[1] & 1) return fail(BFGX_ERR_ASSERT, "Halo offsets are larger than res (Map2DRunner.py:516)");
    if (total > (int64_t)INT32_MAX) return fail(BFGX_ERR_INVALID, "block lists exceed 2^31 entries: split the catalog");
    if (total > p->list_capacity) if (int rc = grow_list(p->mem, p->blk_list, p->list_capacity, total)) return rc;
    if (c->n > 0 && total > 0) {
        GridTimer kt(p, BFGX_K_BIN);
        launch_block_lists<1>(p, c->n);
        HIP_TRY(hipGetLastError());
    }
    return BFGX_OK;
}

// cells [c0, c0 + n): map_out = map_in, partial sums to block_sums[slot0 .. slot0 + nwg)
static int grid_copy_stage(bfgx_grid_plan *p, const double *map_in, double *map_out, int64_t c0, int64_t n, int slot0, int nwg)
{
    GridTimer kt(p, BFGX_K_REGRID);
    hipLaunchKernelGGL(grid_copy_sum_kernel, dim3(nwg), dim3(256), 0, p->stream, n, map_in + c0, map_out + c0, p->block_sums + slot0);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

static int grid_gather_stage(bfgx_grid_plan *p, const double *map_in, double *map_out, const GatherRanges &gr, int r)
{
    GridTimer kt(p, BFGX_K_OFFSETS);
    if (gr.nnz[r] > 0) launch_gather(p, map_in, map_out, gr.nnz[r], gr.lo[r]);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

static int grid_sums_stage(bfgx_grid_plan *p, int ncopy, double *sums_dev, int64_t *n_pairs_host)
{
    hipStream_t s = p->stream;
    {
        GridTimer kt(p, BFGX_K_SUM);
        hipLaunchKernelGGL(gather_sums_kernel, dim3(64), dim3(256), 0, s, p->nblk, (const double *)p->blk_sums, ncopy, (const double *)p->block_sums, sums_dev, p->pair_total);
        HIP_TRY(hipGetLastError());
    }
    return n_pairs_host ? read_pair_total(s, p->pair_total, n_pairs_host) : BFGX_OK;
}

// ncopy_done > 0: map_out already holds a copy of map_in and p->block_sums[0 .. ncopy_done) its partial sums (the fused deposit)
static int grid_baryonify_impl(bfgx_grid_plan *p, const bfgx_grid_catalog *c, const double *map_in, double *map_out, double *sums_dev,
                               int64_t *n_pairs_host, int ncopy_done)
{
    if (!p || !c || !map_in || !map_out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = grid_check_catalog(p, c)) return rc;
    HIP_TRY(hipSetDevice(p->device));
    if (int rc = gather_workspace(p)) return rc;
    // map_out = map_in: a cell the halo loop does not move deposits into itself (the gather kernel touches the moved cells only)
    constexpr int kCopyWgs = 2048;
    if (ncopy_done <= 0) if (int rc = grid_copy_stage(p, map_in, map_out, 0, p->geom.ntot, 0, kCopyWgs)) return rc;
    GatherRanges gr;
    gr.n = 1; gr.lo[0] = 0; gr.hi[0] = p->nblk;
    if (int rc = grid_lists_stage(p, c, gr)) return rc;
    if (int rc = grid_gather_stage(p, map_in, map_out, gr, 0)) return rc;
    return grid_sums_stage(p, ncopy_done > 0 ? ncopy_done : kCopyWgs, sums_dev, n_pairs_host);
}

int bfgx_grid_baryonify_device(bfgx_grid_plan *p, const bfgx_grid_catalog *c, const double *map_in, double *map_out, double *sums_dev,
                               int64_t *n_pairs_host)
{
    return grid_baryonify_impl(p, c, map_in, map_out, sums_dev, n_pairs_host, 0);
}

int bfgx_grid_plan_timing_enable(bfgx_grid_plan *p, int on)
{
    return p ? p->events.enable(on) : fail(BFGX_ERR_INVALID, "NULL plan");
}

int bfgx_grid_plan_timing_read(bfgx_grid_plan *p, double *ms_sum, int64_t *launches)
{
    return p ? p->events.read(p->device, p->stream, ms_sum, launches) : fail(BFGX_ERR_INVALID, "NULL argument");
}

// ---------------------------------------------------------------- one-shot host API

}  // extern "C"

namespace {

// ---- cache of the one-shot grid entries: plan + device maps per (device, grid, model), as the shell entries keep theirs --------------
struct GridEntry : CacheEntry<bfgx_grid_plan> {
    DevBuf in, out, sums;
    GridHostCatalog hc;
};
PlanCache<GridEntry, 2> g_grids;                    // (an entry holds two maps: 2.1 GB at 512^3)
std::atomic<long long> g_grid_pipe_fallbacks{0};     // streamed bfgx_baryonify_grid calls that repeated the regrid in one pass (a cell moved too far along axis 0)

// the cached entry for (device, grid, model) with a plan for at least n halos and the two device maps; g_grids.mu is held by the caller
int grid_acquire(int device, const bfgx_grid *grid, const bfgx_model *model, int64_t n, GridEntry **out)
{
    if (int rc = validate_grid(grid)) return rc;
    if (int rc = validate_model(model)) return rc;
    CacheKey key = model_key(device, model);
    key.add(grid->npix); key.add(grid->ndim); key.add(grid->redshift);
    key.add(grid->bins, sizeof(double) * (size_t)grid->npix);
    auto make = [&](int64_t cap, bfgx_grid_plan **p) { return bfgx_grid_plan_create(device, nullptr, grid, cap, model, p); };
    auto setup = [](GridEntry *e) -> int {
        const size_t bytes = (size_t)e->plan->geom.ntot * sizeof(double);
        if (!e->in.p && (e->in.alloc(bytes) || e->out.alloc(bytes) || e->sums.alloc(2 * sizeof(double)))) return alloc_fail("map buffers");
        return BFGX_OK;
    };
    return g_grids.acquire(key, device, n, make, setup, out);
}

constexpr int kGridChunksMax = 32;

// How bfgx_baryonify_grid cuts a map: ranges of whole rows of gather blocks (2^S planes of the first axis: 8 planes in 3-D, 16 rows in 2-D)
// of at least 16 MB, at most kGridChunksMax of them (BFGX_PIPE_CHUNKS sets the count: tests, small maps).  Chunk c = block rows
// [c rows_per, (c + 1) rows_per); gather range 0 = block row 0 alone, 1 = the rest of chunk 0, c + 1 = chunk c.
struct GridRangePlan {
    int C = 0, rows_per = 0, nbk = 0, S = 0, N = 0;
    bool piped = false;                  // the map travels in ranges (needs 3 of them); gr is filled
    size_t plane = 1;                    // cells per plane of the first axis
    GatherRanges gr;
    int row0(int c) const { return std::min(c * rows_per, nbk); }
    size_t cell0(int c) const { return (size_t)std::min<int64_t>((int64_t)row0(c) << S, N) * plane; }
};

GridRangePlan grid_range_plan(int ndim, int N, int S, const PipeKnobs &knobs)
{
    GridRangePlan r;
    r.S = S; r.N = N; r.nbk = gather_blocks_per_axis(N, S);
    const int nbk = r.nbk;
    for (int d = 1; d < ndim; ++d) r.plane *= (size_t)N;
    const size_t row_bytes = ((size_t)1 << S) * r.plane * sizeof(double);
    r.rows_per = (int)std::max<size_t>(2, (((size_t)16 << 20) + row_bytes - 1) / row_bytes);
    r.C = (nbk + r.rows_per - 1) / r.rows_per;
    if (r.C > kGridChunksMax) { r.rows_per = (nbk + kGridChunksMax - 1) / kGridChunksMax; r.C = (nbk + r.rows_per - 1) / r.rows_per; }
    if (knobs.stage) {
        const int want = std::max(3, std::min(kGridChunksMax, knobs.chunks));
        r.rows_per = std::max(2, nbk / want); r.C = (nbk + r.rows_per - 1) / r.rows_per;
        if (r.C > kGridChunksMax) r.C = 0;
    }
    r.piped = r.C >= 3 && r.C <= kGridChunksMax && !knobs.off;
    if (!r.piped) return r;
    const int64_t blocks_per_row = (ndim == 3) ? (int64_t)nbk * nbk : nbk;
    r.gr.n = r.C + 1; r.gr.lo[0] = 0; r.gr.hi[0] = blocks_per_row;
    r.gr.lo[1] = blocks_per_row; r.gr.hi[1] = (int64_t)r.row0(1) * blocks_per_row;
    for (int c = 1; c < r.C; ++c) { r.gr.lo[c + 1] = (int64_t)r.row0(c) * blocks_per_row; r.gr.hi[c + 1] = (int64_t)r.row0(c + 1) * blocks_per_row; }
    return r;
}

// The streamed route of bfgx_baryonify_grid (both host arrays are open in `call`): a range is copied into map_out and gathered as soon as
// it and its neighbours have arrived, and travels back while the next ones are still coming.  The first block row is gathered last (the
// grid is periodic: it deposits into the last plane), so the first range also leaves last.
int grid_streamed(OneShotCall &call, GridEntry *e, GridRangePlan &rp, double sums[2], int64_t *npairs)
{
    bfgx_grid_plan *p = e->plan;
    const double *map_in = call.src<double>();
    double *map_out = call.dst<double>(), *d_in = (double *)e->in.p, *d_out = (double *)e->out.p, *d_sums = (double *)e->sums.p;
    hipStream_t s = p->stream;
    const int C = rp.C, nwg = std::max(1, 2048 / C);
    if (int rc = grid_check_catalog(p, &e->hc.d)) return rc;
    if (int rc = gather_workspace(p)) return rc;
    if (int rc = e->pools(C, C + 1)) return rc;
    // uploads first (they need nothing), in order, on their own stream; the halo lists are built underneath them
    for (int c = 0; c < C; ++c) {
        const size_t lo = rp.cell0(c), n = rp.cell0(c + 1) - lo;
        HIP_TRY(hipMemcpyAsync(d_in + lo, map_in + lo, n * sizeof(double), hipMemcpyHostToDevice, e->up));
        HIP_TRY(hipEventRecord(e->ev_up[c], e->up));
    }
    if (int rc = call.mark(1, e->up)) return rc;                           // the last byte of the map has arrived
    if (int rc = grid_lists_stage(p, &e->hc.d, rp.gr)) return rc;
    // How far may a cell move along the first array axis in this route?  Range 1 (the rest of chunk 0) is gathered when only chunks 0 and 1
    // hold their start values: a deposit that travels back through block row 0 and across the periodic face lands in the LAST chunk before
    // that chunk has been copied, and the copy then overwrites it; block row 0, gathered last, must not reach chunk 1, which has left the
    // device by then; a middle chunk's deposits stay within its two neighbours.  One block row (2^S planes) is the tightest of these: a move
    // of up to 2^S - 1 cells (+ 1 for the second overlap cell) is safe.  The gather kernel flags anything beyond; the call then repeats
    // the regrid in one pass on the map it has already uploaded (the mass check alone would not notice: the sums are arithmetic).
    Restore<float> limit{p->axis0_limit, 3.0e38f};
    p->axis0_limit = (float)((1 << rp.S) - 1);
    auto download = [&](int c, hipEvent_t after) -> int {
        const size_t lo = rp.cell0(c), n = rp.cell0(c + 1) - lo;
        HIP_TRY(hipStreamWaitEvent(e->down, after, 0));
        HIP_TRY(hipMemcpyAsync(map_out + lo, d_out + lo, n * sizeof(double), hipMemcpyDeviceToHost, e->down));
        return BFGX_OK;
    };
    for (int c = 0; c < C; ++c) {
        HIP_TRY(hipStreamWaitEvent(s, e->ev_up[c], 0));
        if (int rc = grid_copy_stage(p, d_in, d_out, (int64_t)rp.cell0(c), (int64_t)(rp.cell0(c + 1) - rp.cell0(c)), c * nwg, nwg)) return rc;
        if (c >= 1) {
            // chunk c - 1 has its own cells and both neighbours' start values (chunk 0: all but its first block row, which needs the LAST chunk)
            if (int rc = grid_gather_stage(p, d_in, d_out, rp.gr, c - 1 == 0 ? 1 : c)) return rc;
            HIP_TRY(hipEventRecord(e->ev_k[c - 1], s));
            if (c - 2 >= 1) if (int rc = download(c - 2, e->ev_k[c - 1])) return rc;      // nothing deposits into chunk c - 2 any more
        }
    }
    if (int rc = grid_gather_stage(p, d_in, d_out, rp.gr, C)) return rc;                     // the last chunk (deposits into plane 0: chunk 0 is all there)
    if (int rc = grid_gather_stage(p, d_in, d_out, rp.gr, 0)) return rc;                     // block row 0 (deposits into the last plane)
    HIP_TRY(hipEventRecord(e->ev_k[C - 1], s));
    if (int rc = grid_sums_stage(p, C * nwg, d_sums, npairs)) return rc;                     // (synchronises the plan's stream)
    if (int rc = call.mark(2, s)) return rc;
    if (C - 2 >= 1) if (int rc = download(C - 2, e->ev_k[C - 1])) return rc;
    if (int rc = download(C - 1, e->ev_k[C - 1])) return rc;
    if (int rc = download(0, e->ev_k[C - 1])) return rc;
    int32_t moved_too_far = 0;
    HIP_TRY(hipMemcpyAsync(sums, d_sums, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&moved_too_far, p->axis0_flag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipStreamSynchronize(e->down));
    HIP_TRY(hipStreamSynchronize(e->up));
    if (moved_too_far) {
        // a cell moved further along the first axis than the plane ranges allow: the whole map is on the device -- regrid it in one pass
        p->axis0_limit = 3.0e38f;
        ++g_grid_pipe_fallbacks;
        HIP_TRY(hipMemsetAsync(d_sums, 0, 2 * sizeof(double), s));
        if (int rc = bfgx_grid_baryonify_device(p, &e->hc.d, d_in, d_out, d_sums, npairs)) return rc;
        if (int rc = call.mark(2, s)) return rc;
        HIP_TRY(hipMemcpyAsync(map_out, d_out, (size_t)p->geom.ntot * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(sums, d_sums, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return call.mark(3, e->down);
}

// The one-pass route of bfgx_baryonify_grid: the whole map up, the cell-owned pass (or, BFGX_GRID_PATH=scatter, the halo-owned kernels),
// the whole map down
int grid_one_pass(OneShotCall &call, GridEntry *e, bool scatter, const double *map_in, double *map_out, double sums[2], int64_t *npairs)
{
    bfgx_grid_plan *p = e->plan;
    const size_t ntot = (size_t)p->geom.ntot;
    double *d_in = (double *)e->in.p, *d_out = (double *)e->out.p, *d_sums = (double *)e->sums.p;
    hipStream_t s = p->stream;
    HIP_TRY(hipMemcpyAsync(d_in, map_in, ntot * sizeof(double), hipMemcpyHostToDevice, s));
    if (int rc = call.mark(1, s)) return rc;
    if (scatter) {
        DevBuf d_off;
        if (d_off.alloc(ntot * p->geom.ndim * sizeof(double))) return alloc_fail("pix_offsets");
        if (int rc = bfgx_grid_offsets_device(p, &e->hc.d, (double *)d_off.p, npairs)) return rc;
        if (int rc = bfgx_grid_regrid_device(p, d_in, (const double *)d_off.p, d_out, d_sums)) return rc;
        HIP_TRY(hipStreamSynchronize(s));
    } else if (int rc = bfgx_grid_baryonify_device(p, &e->hc.d, d_in, d_out, d_sums, npairs)) return rc;
    if (int rc = call.mark(2, s)) return rc;
    HIP_TRY(hipMemcpyAsync(map_out, d_out, ntot * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(sums, d_sums, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return call.mark(3, s);
}

}  // namespace

extern "C" {

int bfgx_baryonify_grid(const bfgx_grid_catalog *cat, const bfgx_model *model, const bfgx_grid *grid, const double *map_in,
                        double *map_out, const bfgx_opts *opts, bfgx_stats *stats)
{
    if (!cat || !model || !grid || !map_in || !map_out) return fail(BFGX_ERR_INVALID, "NULL argument");
    const bfgx_opts o = entry_opts(opts);
    std::lock_guard<std::mutex> lk(g_grids.mu);
    GridEntry *e = nullptr;
    if (int rc = grid_acquire(o.device, grid, model, cat->n, &e)) return rc;
    bfgx_grid_plan *p = e->plan;
    OneShotCall call(&p->stream, e);
    const size_t ntot = (size_t)p->geom.ntot;
    const int ndim = p->geom.ndim;
    // BFGX_GRID_PATH=scatter keeps the halo-owned kernels (what the multi-GPU entry points use) reachable from the one-shot API for tests
    const char *path = std::getenv("BFGX_GRID_PATH");
    const bool scatter = path && std::strcmp(path, "scatter") == 0;
    if (int rc = call.mark(0, p->stream)) return rc;
    if (int rc = e->hc.upload(cat, ndim, p->model.tab.ndim - 3, p->stream)) return rc;
    HIP_TRY(hipMemsetAsync(e->sums.p, 0, 2 * sizeof(double), p->stream));
    int64_t npairs = 0;
    double sums[2] = {0, 0};
    const PipeKnobs knobs = pipe_knobs();
    GridRangePlan rp = grid_range_plan(ndim, p->geom.npix, (ndim == 3) ? GatherBlk<3>::S : GatherBlk<2>::S, knobs);
    const bool piped = !scatter && rp.piped && call.open(map_in, ntot * sizeof(double), map_out, ntot * sizeof(double), knobs.stage);
    if (int rc = piped ? grid_streamed(call, e, rp, sums, &npairs) : grid_one_pass(call, e, scatter, map_in, map_out, sums, &npairs)) return rc;
    call.commit();                                           // (a staged result reaches the caller's array)
    if (int rc = call.finish(stats, sums, npairs)) return rc;
    return o.check_mass ? check_mass(sums[0], sums[1]) : BFGX_OK;      // (Map2DRunner.py:601-605)
}

long long bfgx_debug_grid_pipe_fallbacks(void) { return g_grid_pipe_fallbacks.load(); }

int bfgx_paint_grid(const bfgx_grid_catalog *cat, const bfgx_model *model, const bfgx_grid *grid, double *map_out,
                    const bfgx_opts *opts, bfgx_stats *stats)
{
    if (!cat || !model || !grid || !map_out) return fail(BFGX_ERR_INVALID, "NULL argument");
    const bfgx_opts o = entry_opts(opts);
    bfgx_grid_plan *p = nullptr;
    if (int rc = bfgx_grid_plan_create(o.device, nullptr, grid, cat->n, model, &p)) return rc;
    struct Guard { bfgx_grid_plan *p; ~Guard() { bfgx_grid_plan_destroy(p); } } guard{p};       // (its destructor drains the plan's stream first)
    const size_t ntot = (size_t)p->geom.ntot;
    GridHostCatalog hc;
    DevBuf d_out;
    Timer t;
    t.start(p->stream);
    if (int rc = hc.upload(cat, grid->ndim, p->model.tab.ndim - 3, p->stream)) return rc;
    if (d_out.alloc(ntot * sizeof(double))) return alloc_fail("map");
    const double ms_h2d = t.lap(p->stream);
    int64_t npairs = 0;
    if (int rc = bfgx_grid_paint_device(p, &hc.d, (double *)d_out.p, &npairs)) return rc;
    const double ms_k = t.lap(p->stream);
    HIP_TRY(hipMemcpyAsync(map_out, d_out.p, ntot * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    const double ms_d2h = t.stop(p->stream);
    fill_stats(stats, nullptr, npairs, ms_h2d, ms_k, ms_d2h);
    return BFGX_OK;
}

int bfgx_regrid_pixels(int device, int32_t ndim, int32_t npix, int64_t n, const double *positions, const double *values, double *grid)
{
    if (!positions || !values || !grid) return fail(BFGX_ERR_INVALID, "NULL argument");
    if ((ndim != 2 && ndim != 3) || npix < 5 || n < 0) return fail(BFGX_ERR_INVALID, "regrid_pixels needs ndim in {2, 3}, npix >= 5");
    HostCall c(device);
    size_t ntot = 1;
    for (int d = 0; d < ndim; ++d) ntot *= (size_t)npix;
    const double *dp = c.in(positions, (size_t)n * ndim), *dv = c.in(values, n);
    double *dg = c.inout(grid, ntot);
    if (int rc = c.ready()) return rc;
    if (n > 0) {
        const unsigned blocks = (unsigned)((n + 255) / 256);
        grid_dim(ndim, [&](auto dim) { hipLaunchKernelGGL((pixel_deposit_kernel<decltype(dim)::value>), dim3(blocks), dim3(256), 0, 0, npix, n, dp, dv, dg); });
    }
    return c.finish();
}

}  // extern "C"
