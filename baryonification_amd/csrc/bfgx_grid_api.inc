// bfgx_grid_api.inc -- C ABI of the regular-grid path (included at the end of bfgx_api.hip: one translation unit).
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
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[BFGX_NUM_KERNELS];
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_free;
};

namespace {

using GridTimer = KernelTimerT<bfgx_grid_plan>;

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

template <int NC>
int launch_grid_prep_nc(bfgx_grid_plan *p, const bfgx_grid_catalog *c, int mode)
{
    GridCatalog gc;
    gc.n = c->n; gc.M = c->M; gc.x = c->x; gc.y = c->y; gc.z = c->z; gc.lnM = c->lnM; gc.rmat = c->rmat;
    for (int k = 0; k < BFGX_MAX_EXTRA; ++k) gc.extra[k] = c->extra[k];
    const int blocks = (int)((c->n + kGridBlock - 1) / kGridBlock);
    hipLaunchKernelGGL(grid_prep_kernel<NC>, dim3(blocks), dim3(kGridBlock), 0, p->stream, p->model, p->geom, gc, mode,
                       p->recs, p->chunk_halo, p->capacity, p->counters);
    return BFGX_OK;
}

int launch_grid_prep(bfgx_grid_plan *p, const bfgx_grid_catalog *c, int mode)
{
    HIP_TRY(hipMemsetAsync(p->counters, 0, 2 * sizeof(int32_t), p->stream));
    if (c->n == 0) return BFGX_OK;
    GridTimer kt(p, BFGX_K_PREP);
    if (p->NC == 4) launch_grid_prep_nc<4>(p, c, mode);
    else if (p->NC == 8) launch_grid_prep_nc<8>(p, c, mode);
    else launch_grid_prep_nc<16>(p, c, mode);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

template <int DIM, int MODE, int NC>
void launch_grid_scatter_t(bfgx_grid_plan *p, int blocks, double *out)
{
    hipLaunchKernelGGL((grid_scatter_kernel<DIM, MODE, NC>), dim3(blocks), dim3(kGridBlock), 0, p->stream,
                       make_pair_table(p->model.tab), p->geom, p->recs, p->chunk_halo, p->counters, out, p->pair_total);
}

template <int DIM, int MODE>
int launch_grid_scatter(bfgx_grid_plan *p, int blocks, double *out)
{
    GridTimer kt(p, MODE == 0 ? BFGX_K_OFFSETS : BFGX_K_PAINT);
    if (p->NC == 4) launch_grid_scatter_t<DIM, MODE, 4>(p, blocks, out);
    else if (p->NC == 8) launch_grid_scatter_t<DIM, MODE, 8>(p, blocks, out);
    else launch_grid_scatter_t<DIM, MODE, 16>(p, blocks, out);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

// prep (+ regrowth of the work-item table) + scatter; mode 0 = offsets, 1 = paint
int grid_halo_loop(bfgx_grid_plan *p, const bfgx_grid_catalog *c, int mode, double *out, int64_t *n_pairs_host)
{
    if (!p || !c || !out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (c->n < 0 || c->n > p->max_halos) return fail(BFGX_ERR_INVALID, "catalog size %lld exceeds plan max_halos %lld",
                                                     (long long)c->n, (long long)p->max_halos);
    const int nex = p->model.tab.ndim - 3;
    if (c->n > 0 && (!c->M || !c->x || !c->y || (p->geom.ndim == 3 && !c->z))) return fail(BFGX_ERR_INVALID, "catalog column pointer is NULL");
    for (int k = 0; k < nex; ++k) if (c->n > 0 && !c->extra[k]) return fail(BFGX_ERR_INVALID, "catalog misses a property column of the table");
    if (c->rmat && p->geom.ndim == 3) return fail(BFGX_ERR_UNSUPPORTED, "use_ellipticity is not implemented for 3D maps");
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
        const int64_t cap = (int64_t)cnt[0] + cnt[0] / 4 + 1024;
        HIP_TRY(p->mem.regrow(p->chunk_halo, (size_t)cap));
        p->capacity = cap;
    }
    if (cnt[1] & 1) return fail(BFGX_ERR_ASSERT, "Halo offsets are larger than res (Map2DRunner.py:516)");
    if (cnt[0] > 0) {
        const int blocks = (int)std::min<int64_t>(cnt[0], (int64_t)p->n_cu * 8);
        int rc;
        if (p->geom.ndim == 3) rc = mode == 0 ? launch_grid_scatter<3, 0>(p, blocks, out) : launch_grid_scatter<3, 1>(p, blocks, out);
        else rc = mode == 0 ? launch_grid_scatter<2, 0>(p, blocks, out) : launch_grid_scatter<2, 1>(p, blocks, out);
        if (rc) return rc;
    }
    if (n_pairs_host) {
        unsigned long long np = 0;
        HIP_TRY(hipMemcpyAsync(&np, p->pair_total, sizeof(np), hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        *n_pairs_host = (int64_t)np;
    }
    return BFGX_OK;
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

int ilog2_exact(int n) { int l = 0; while ((1 << l) < n) ++l; return ((1 << l) == n) ? l : -1; }

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
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) p->n_cu = prop.multiProcessorCount;
    *out = p;
    return BFGX_OK;
}

void bfgx_grid_plan_destroy(bfgx_grid_plan *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    (void)hipStreamSynchronize(p->stream);
    p->mem.release();
    for (int k = 0; k < BFGX_NUM_KERNELS; ++k)
        for (auto &e : p->ev[k]) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    for (auto &e : p->ev_free) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
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
        if (g.ndim == 3)
            hipLaunchKernelGGL(grid_regrid_kernel<3>, dim3(blocks), dim3(256), 0, p->stream, g.npix, ntot, offsets, map_in, map_out, bs, sw, missed_dev);
        else
            hipLaunchKernelGGL(grid_regrid_kernel<2>, dim3(blocks), dim3(256), 0, p->stream, g.npix, ntot, offsets, map_in, map_out, bs, sw, missed_dev);
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
    p->nscan_blocks = (int)((p->nblk + 1 + kScanPerBlock - 1) / kScanPerBlock);
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

template <int DIM, int FILL>
void launch_block_lists(bfgx_grid_plan *p, int64_t nh)
{
    hipLaunchKernelGGL((grid_block_lists_kernel<DIM, FILL>), dim3((unsigned)((nh + 256 / kWave - 1) / (256 / kWave))), dim3(256), 0, p->stream, p->geom, nh,
                       (const GridHaloRec *)p->recs, p->blk_count, (const int32_t *)p->blk_start, p->blk_list);
}

template <int DIM>
void launch_gather(bfgx_grid_plan *p, const double *map_in, double *map_out, int64_t nnz, int64_t nz_off = 0)
{
    const PairTable pt = make_pair_table(p->model.tab);
    const dim3 grid((unsigned)nnz), block(256);
    if (p->NC == 4)
        hipLaunchKernelGGL((grid_gather_regrid_kernel<DIM, 4>), grid, block, 0, p->stream, pt, p->geom, (const GridHaloRec *)p->recs, (const int32_t *)p->blk_start,
                           (const int32_t *)p->blk_list, (const int32_t *)p->blk_nz + nz_off, map_in, map_out, p->blk_sums, p->axis0_limit,
                           p->axis0_limit < 1.0e30f ? p->axis0_flag : (int32_t *)nullptr);
    else if (p->NC == 8)
        hipLaunchKernelGGL((grid_gather_regrid_kernel<DIM, 8>), grid, block, 0, p->stream, pt, p->geom, (const GridHaloRec *)p->recs, (const int32_t *)p->blk_start,
                           (const int32_t *)p->blk_list, (const int32_t *)p->blk_nz + nz_off, map_in, map_out, p->blk_sums, p->axis0_limit,
                           p->axis0_limit < 1.0e30f ? p->axis0_flag : (int32_t *)nullptr);
    else
        hipLaunchKernelGGL((grid_gather_regrid_kernel<DIM, 16>), grid, block, 0, p->stream, pt, p->geom, (const GridHaloRec *)p->recs, (const int32_t *)p->blk_start,
                           (const int32_t *)p->blk_list, (const int32_t *)p->blk_nz + nz_off, map_in, map_out, p->blk_sums, p->axis0_limit,
                           p->axis0_limit < 1.0e30f ? p->axis0_flag : (int32_t *)nullptr);
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
    if (c->n < 0 || c->n > p->max_halos) return fail(BFGX_ERR_INVALID, "catalog size %lld exceeds plan max_halos %lld", (long long)c->n, (long long)p->max_halos);
    const int nex = p->model.tab.ndim - 3;
    if (c->n > 0 && (!c->M || !c->x || !c->y || (p->geom.ndim == 3 && !c->z))) return fail(BFGX_ERR_INVALID, "catalog column pointer is NULL");
    for (int k = 0; k < nex; ++k) if (c->n > 0 && !c->extra[k]) return fail(BFGX_ERR_INVALID, "catalog misses a property column of the table");
    if (c->rmat && p->geom.ndim == 3) return fail(BFGX_ERR_UNSUPPORTED, "use_ellipticity is not implemented for 3D maps");
    return BFGX_OK;
}

static int grid_lists_stage(bfgx_grid_plan *p, const bfgx_grid_catalog *c, GatherRanges &gr)
{
    hipStream_t s = p->stream;
    const bool d3 = p->geom.ndim == 3;
    HIP_TRY(hipMemsetAsync(p->pair_total, 0, sizeof(unsigned long long), s));
    HIP_TRY(hipMemsetAsync(p->blk_count, 0, sizeof(int32_t) * (size_t)(p->nblk + 1), s));
    if (int rc = launch_grid_prep(p, c, 0)) return rc;                  // (its work-item table is not used here)
    int64_t total = 0;
    int32_t cnt[2] = {0, 0};
    {
        GridTimer kt(p, BFGX_K_BIN);
        if (c->n > 0) { if (d3) launch_block_lists<3, 0>(p, c->n); else launch_block_lists<2, 0>(p, c->n); }
        hipLaunchKernelGGL(scan_blocks_kernel, dim3(p->nscan_blocks), dim3(kTabThreads), 0, s, p->nblk + 1, (const int32_t *)p->blk_count, p->blk_start, p->blk_bsum, 1);
        hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(kTabThreads), 0, s, p->nscan_blocks, p->blk_bsum, p->blk_total);
        hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)((p->nblk + 1 + 255) / 256)), dim3(256), 0, s, p->nblk + 1, p->blk_start, (const int32_t *)p->blk_bsum);
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
    if (total > p->list_capacity) {
        const int64_t cap = total + total / 4 + 1024;
        HIP_TRY(p->mem.regrow(p->blk_list, (size_t)cap));
        p->list_capacity = cap;
    }
    if (c->n > 0 && total > 0) {
        GridTimer kt(p, BFGX_K_BIN);
        if (d3) launch_block_lists<3, 1>(p, c->n); else launch_block_lists<2, 1>(p, c->n);
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
    if (gr.nnz[r] > 0) { if (p->geom.ndim == 3) launch_gather<3>(p, map_in, map_out, gr.nnz[r], gr.lo[r]); else launch_gather<2>(p, map_in, map_out, gr.nnz[r], gr.lo[r]); }
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
    if (n_pairs_host) {
        unsigned long long np = 0;
        HIP_TRY(hipMemcpyAsync(&np, p->pair_total, sizeof(np), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        *n_pairs_host = (int64_t)np;
    }
    return BFGX_OK;
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
    if (!p) return fail(BFGX_ERR_INVALID, "NULL plan");
    p->timing = on != 0;
    return BFGX_OK;
}

int bfgx_grid_plan_timing_read(bfgx_grid_plan *p, double *ms_sum, int64_t *launches)
{
    if (!p || !ms_sum || !launches) return fail(BFGX_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    for (int k = 0; k < BFGX_NUM_KERNELS; ++k) {
        double tot = 0.0;
        for (auto &e : p->ev[k]) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, e.first, e.second));
            tot += ms;
            p->ev_free.push_back(e);
        }
        ms_sum[k] = tot;
        launches[k] = (int64_t)p->ev[k].size();
        p->ev[k].clear();
    }
    return BFGX_OK;
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
        if (ndim == 3) hipLaunchKernelGGL(pixel_deposit_kernel<3>, dim3(blocks), dim3(256), 0, 0, npix, n, dp, dv, dg);
        else hipLaunchKernelGGL(pixel_deposit_kernel<2>, dim3(blocks), dim3(256), 0, 0, npix, n, dp, dv, dg);
    }
    return c.finish();
}

}  // extern "C"

namespace {

// grow-only workspace of the tiled deposit, one per device (released by bfgx_cache_clear); one deposit in flight per device
struct DepWork {
    PoolBuf keys[2], mass[2], ctr, bsum, total;     // uint32_t keys, double masses, int32_t counters and block sums, one int64_t (slack: an eighth)
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

template <int DIM, bool MASS>
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
    else hipLaunchKernelGGL(deposit_keys_kernel<DIM>, dim3(chunks), dim3(256), 0, s, g, n, x, y, z, edges_dev, keys[0], wg, stride);
    {
        const int nb1 = (int)((nwg + kScanPerBlock - 1) / kScanPerBlock);
        hipLaunchKernelGGL(scan_blocks_kernel, dim3(nb1), dim3(kTabThreads), 0, s, nwg, (const int32_t *)wg, wg, bsum, 1);
        hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(kTabThreads), 0, s, nb1, bsum, total);
        hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)((nwg + 255) / 256)), dim3(256), 0, s, nwg, wg, (const int32_t *)bsum);
    }
    hipLaunchKernelGGL((deposit_split_kernel<1, MASS>), dim3(chunks), dim3(256), 0, s, g, n, (const int32_t *)nullptr, (const uint32_t *)keys[0],
                       mass, (const int32_t *)wg, (int32_t *)nullptr, keys[1], wmass[0], stride);
    const int32_t *nvalid = wg + (nwg - 1);             // particles inside the edges
    hipLaunchKernelGGL(deposit_count_kernel, dim3(chunks), dim3(256), 0, s, g, nvalid, (const uint32_t *)keys[1], c2);
    const int64_t nscan = (int64_t)g.T + 1;
    const int nblocks = (int)((nscan + kScanPerBlock - 1) / kScanPerBlock);
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(nblocks), dim3(kTabThreads), 0, s, nscan, (const int32_t *)c2, s2, bsum, 1);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(kTabThreads), 0, s, nblocks, bsum, total);
    hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)((nscan + 255) / 256)), dim3(256), 0, s, nscan, s2, (const int32_t *)bsum);
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
    bool tiled = n >= (int64_t)1 << 20 && n < ((int64_t)1 << 31) - kDepChunk && g.T < (1 << (32 - kDepLocalBits)) && g.B1 <= 1024 && g.B2 <= kDepHist;
    if (const char *e = std::getenv("BFGX_DEPOSIT")) {
        if (!std::strcmp(e, "atomic")) tiled = false;
        else if (!std::strcmp(e, "tiled")) tiled = n > 0 && n < ((int64_t)1 << 31) - kDepChunk && g.T < (1 << (32 - kDepLocalBits)) && g.B1 <= 1024 && g.B2 <= kDepHist;
    }
    if (keys_by) {             // the keys come from another kernel: the sort is the only form there is
        tiled = n > 0 && n < ((int64_t)1 << 31) - kDepChunk && g.T < (1 << (32 - kDepLocalBits)) && g.B1 <= 1024 && g.B2 <= kDepHist;
        if (n > 0 && !tiled) return fail(BFGX_ERR_UNSUPPORTED, "the fused displace + deposit needs a grid the tile-owned deposit takes (%d tiles): call the displacement and the deposit one after the other", g.T);
    }
    if (tiled) {
        std::lock_guard<std::mutex> lk(g_dep_mu);
        DepWork &w = g_dep[device];
        const size_t nctr = (2 + (size_t)kDepPad) * ((size_t)g.T + 1) + (size_t)g.B1 * (size_t)((n + kDepChunk - 1) / kDepChunk) + 8;
        if (w.keys[0].need(sizeof(uint32_t) * (size_t)n, 8, 0) || w.keys[1].need(sizeof(uint32_t) * (size_t)n, 8, 0)) return alloc_fail("deposit keys");
        if (mass && (w.mass[0].need(sizeof(double) * (size_t)n, 8, 0) || w.mass[1].need(sizeof(double) * (size_t)n, 8, 0))) return alloc_fail("deposit masses");
        if (w.ctr.need(sizeof(int32_t) * nctr, 8, 0) || w.bsum.need(sizeof(int32_t) * (nctr / kScanPerBlock + 2), 8, 0) || w.total.need(sizeof(int64_t), 8, 0))
            return alloc_fail("deposit counters");
        if (ntiles) *ntiles = g.T;
        if (ndim == 3) return mass ? deposit_tiled<3, true>(w, g, s, n, x, y, z, mass, edges_dev, map_out_dev, map_out2_dev, tile_sums_dev, stride, keys_by)
                                   : deposit_tiled<3, false>(w, g, s, n, x, y, z, mass, edges_dev, map_out_dev, map_out2_dev, tile_sums_dev, stride, keys_by);
        return mass ? deposit_tiled<2, true>(w, g, s, n, x, y, z, mass, edges_dev, map_out_dev, map_out2_dev, tile_sums_dev, stride, keys_by)
                    : deposit_tiled<2, false>(w, g, s, n, x, y, z, mass, edges_dev, map_out_dev, map_out2_dev, tile_sums_dev, stride, keys_by);
    }
    HIP_TRY(hipMemsetAsync(map_out_dev, 0, sizeof(double) * ntot, s));
    if (n > 0) {
        const unsigned blocks = (unsigned)((n + 255) / 256);
        if (ndim == 3) hipLaunchKernelGGL(particle_deposit_kernel<3>, dim3(blocks), dim3(256), 0, s, n, x, y, z, mass, n_grid, edges_dev, map_out_dev, plane_lo, plane_n, stride);
        else hipLaunchKernelGGL(particle_deposit_kernel<2>, dim3(blocks), dim3(256), 0, s, n, x, y, z, mass, n_grid, edges_dev, map_out_dev, plane_lo, plane_n, stride);
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

namespace {

// twiddles exp(-2 pi i k / N) and the notebook's k axis / bins (cells 12: fftfreq, linspace), built on the host
struct FftSetup {
    DevBuf dtw, dkl;
    DevBuf dtab, dksb, dcnb;          // the tabulated bins (pk_table_build_kernel), built by the first binned pass when nk <= 254
    bool tab_ready = false;
    int lg = 0, nz = 0, tile = 1, lt = 2, threads = 256;
    unsigned ztiles = 1;
    size_t lds = 0, lds_bin1 = 0, lds_bin2 = 0;
    // the instantiation of the strided kernel for this setup's (lines per tile, threads)
    template <int BIN> const void *strided_fn()
    {
        if (lt == 3) return threads == 1024 ? (const void *)fft_c2c_strided_kernel<BIN, 3, 1024> : threads == 512 ? (const void *)fft_c2c_strided_kernel<BIN, 3, 512> : (const void *)fft_c2c_strided_kernel<BIN, 3, 256>;
        return threads == 1024 ? (const void *)fft_c2c_strided_kernel<BIN, 2, 1024> : threads == 512 ? (const void *)fft_c2c_strided_kernel<BIN, 2, 512> : (const void *)fft_c2c_strided_kernel<BIN, 2, 256>;
    }
    template <int BIN> int strided_attr(size_t bytes)
    {
        HIP_TRY(hipFuncSetAttribute(strided_fn<BIN>(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        return BFGX_OK;
    }
    template <int BIN> int strided_launch(hipStream_t s, unsigned wgs, size_t bytes, double2 *F, int N, int64_t stride, int64_t outer_stride, int nouter,
                                          const PkBins &pb)
    {
        const double2 *twp = dtw.as<double2>();
        int lg_ = lg, nz_ = nz, nzt_ = (int)ztiles;
        PkBins pbv = pb;
        void *args[] = {&F, &N, &lg_, &nz_, &stride, &outer_stride, &twp, &nzt_, &nouter, &pbv};
        HIP_TRY(hipLaunchKernel(strided_fn<BIN>(), dim3(wgs), dim3((unsigned)threads), args, bytes, s));
        return BFGX_OK;
    }
    int n_cu = 256;
    double k_lo = 0, dk = 0;
    int init(int N, double L, int nk)
    {
        lg = ilog2_exact(N);
        if (lg < 3 || N > 1024) return fail(BFGX_ERR_UNSUPPORTED, "power spectrum needs n_grid = 2^m with 8 <= n_grid <= 1024");
        nz = N / 2 + 1;
        std::vector<double> tw(N), klin(N);
        for (int k = 0; k < N / 2; ++k) {
            const long double ang = -2.0L * 3.141592653589793238462643383279502884L * (long double)k / (long double)N;
            tw[2 * k] = (double)cosl(ang); tw[2 * k + 1] = (double)sinl(ang);
        }
        const double two_pi = 2 * 3.141592653589793;
        const double d = 1 / (two_pi / (L)) / N;                       // np.fft.fftfreq(Ngrd, 1 / (2 pi / Lbox) / Ngrd)
        const double val = 1.0 / (N * d);
        for (int i = 0; i < N; ++i) klin[i] = (double)(i < (N + 1) / 2 ? i : i - N) * val;
        k_lo = two_pi / L;
        const double k_hi = two_pi / L * N / 2;                        // np.linspace(k_lo, k_hi, nk + 1)
        const double step = (k_hi - k_lo) / nk;
        const double kb1 = (nk == 1) ? k_hi : (1.0 * step + k_lo);
        dk = kb1 - k_lo;
        if (dtw.up(tw.data(), sizeof(double) * N) || dkl.up(klin.data(), sizeof(double) * N)) return alloc_fail("fft tables");
        lt = kFftTileLog2;
        while (((size_t)N << lt) > 4096 && lt > 2) --lt;                                              // at most 64 KB of tile per workgroup
        tile = 1 << lt;
        // two radix-4 quads per thread and pass where the tile has that many (N = 512, 8 lines)
        const int nq = (N >> 2) << lt;
        threads = nq >= 512 ? 512 : 256;       // (1024 threads: one workgroup per CU, measured 15 % slower at N = 512)
        ztiles = (unsigned)((nz + tile - 1) / tile);
        lds = fft_c2c_lds_bytes(N, lt, 0, 0);
        lds_bin1 = fft_c2c_lds_bytes(N, lt, nk, 1);
        lds_bin2 = fft_c2c_lds_bytes(N, lt, nk, 2);
        if (int rc = strided_attr<0>(lds)) return rc;
        if (int rc = strided_attr<1>(lds_bin1)) return rc;
        if (int rc = strided_attr<2>(lds_bin2)) return rc;
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) n_cu = prop.multiProcessorCount;
        return BFGX_OK;
    }
};

// twiddle / wavenumber tables per (device, n_grid, L, nk): built by the first call, kept until bfgx_cache_clear, so that the
// power-spectrum entry points only enqueue
std::mutex g_fft_mu;
std::map<std::tuple<int, int, double, int>, FftSetup *> g_fft;

int fft_setup(int device, int N, double L, int nk, FftSetup **out)
{
    std::lock_guard<std::mutex> lk(g_fft_mu);
    const auto key = std::make_tuple(device, N, L, nk);
    auto it = g_fft.find(key);
    if (it == g_fft.end()) {
        FftSetup *f = new FftSetup();
        if (int rc = f->init(N, L, nk)) { delete f; return rc; }
        it = g_fft.emplace(key, f).first;
    }
    *out = it->second;
    return BFGX_OK;
}

void fft_release_all()
{
    std::lock_guard<std::mutex> lk(g_fft_mu);
    for (auto &kv : g_fft) { (void)hipSetDevice(std::get<0>(kv.first)); delete kv.second; }
    g_fft.clear();
}

// rows of the half spectrum padded to whole 128-byte lines (8 complex values): a tile of 8 adjacent lines of a strided pass then
// moves exactly one line per row.  nz = 257 unpadded rows start at every multiple of 16 bytes and a 64-byte tile drags in 2.7x
// the bytes it uses (FETCH_SIZE, profiles/r02i_grid3d_summary.txt).
inline int fft_pitch(int N) { return (N / 2 + 1 + 7) & ~7; }

// real lines along the last axis + complex transforms along the middle axis of `planes` planes: map [planes][N][N] -> F [planes][N][pitch]
int fft_planes(FftSetup &f, hipStream_t s, int N, int planes, const double *map_dev, double2 *F, int pitch)
{
    {
        // two line pairs per workgroup of 2 x 128 threads up to N = 512 (a workgroup per pair is launch-bound there: 0.51 -> 0.47 ms at
        // 512^3; 4 pairs, or 64 / 256 threads per pair: 0.52 - 0.60), one pair x 256 threads above (N = 1024: 3.5 ms; 2 x 128: 4.7)
        const size_t npairs = (size_t)planes * N / 2;
        const bool two = N <= 512 && npairs % 2 == 0;
        const unsigned wg = (unsigned)(two ? npairs / 2 : npairs);
        const size_t ldsb = (two ? 2 : 1) * sizeof(double2) * N;
#define BFGX_R2C(P, T) hipLaunchKernelGGL((fft_r2c_lines_kernel<P, T>), dim3(wg), dim3(P * T), ldsb, s, map_dev, F, N, f.lg, f.dtw.as<double2>(), pitch)
        if (two) BFGX_R2C(2, 128);
        else BFGX_R2C(1, 256);
#undef BFGX_R2C
    }
    HIP_TRY(hipGetLastError());
    // axis 1: element (a, i, c) at (a * N + i) * pitch + c
    const unsigned wgs = f.ztiles * (unsigned)planes;
    if (int rc = f.strided_launch<0>(s, wgs, f.lds, F, N, (int64_t)pitch, (int64_t)N * pitch, planes, PkBins{})) return rc;
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

// complex transforms along the FIRST axis of F [N][nb][pitch] (the columns b0 .. b0 + nb of the middle axis) fused with the P(k)
// sums: the transformed tiles are binned from LDS and never written back (F is scratch afterwards)
int fft_axis0_pk(FftSetup &f, hipStream_t s, int N, int nb, int b0, double2 *F, int pitch, int nk, double *pk_sum_dev, double *k_sum_dev,
                 unsigned long long *counts_dev)
{
    HIP_TRY(hipMemsetAsync(pk_sum_dev, 0, sizeof(double) * nk, s));
    HIP_TRY(hipMemsetAsync(k_sum_dev, 0, sizeof(double) * nk, s));
    HIP_TRY(hipMemsetAsync(counts_dev, 0, sizeof(unsigned long long) * nk, s));
    // axis 0: element (i, b, c) at (i * nb + b) * pitch + c.  A fixed number of workgroups strides over the tiles, each flushing
    // its histogram once (3 nk global atomics per workgroup, not per tile)
    const int64_t ntiles = (int64_t)f.ztiles * nb;
    const unsigned wgs = (unsigned)std::min<int64_t>(ntiles, (int64_t)f.n_cu * std::max<size_t>(1, (size_t)(160 * 1024) / f.lds_bin2));
    PkBins pb{f.dkl.as<double>(), f.k_lo, f.dk, 1.0 / f.dk, nk, b0, pk_sum_dev, k_sum_dev, counts_dev, nullptr, pitch};
    // bins, counts and |k| sums are functions of (N, L, nk) alone: tabulated by the first call (one byte per mode), looked up afterwards
    const bool use_tab = nk <= 254;
    if (use_tab && !f.tab_ready) {
        if (f.dtab.up(nullptr, ((size_t)N * f.ztiles * N) << f.lt) || f.dksb.up(nullptr, sizeof(double) * (size_t)N * nk) ||
            f.dcnb.up(nullptr, sizeof(unsigned long long) * (size_t)N * nk))
            return alloc_fail("P(k) bin table");
        PkBins all = pb;
        all.b0 = 0;
        hipLaunchKernelGGL(pk_table_build_kernel, dim3((unsigned)N), dim3(kFftBlock), 16 * (size_t)nk, s, all, N, f.nz, f.lt, (int)f.ztiles, f.dtab.as<uint8_t>(),
                           f.dksb.as<double>(), f.dcnb.as<unsigned long long>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));                    // (built once; later calls on any stream find it complete)
        f.tab_ready = true;
    }
    if (use_tab) {
        pb.tab = f.dtab.as<uint8_t>();
        if (int rc = f.strided_launch<2>(s, wgs, f.lds_bin2, F, N, (int64_t)nb * pitch, (int64_t)pitch, nb, pb)) return rc;
        hipLaunchKernelGGL(pk_table_sums_kernel, dim3((unsigned)nk), dim3(256), 0, s, nk, b0, nb, f.dksb.as<double>(),
                           f.dcnb.as<unsigned long long>(), k_sum_dev, counts_dev);
        HIP_TRY(hipGetLastError());
        return BFGX_OK;
    }
    if (int rc = f.strided_launch<1>(s, wgs, f.lds_bin1, F, N, (int64_t)nb * pitch, (int64_t)pitch, nb, pb)) return rc;
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

}  // namespace

extern "C" {

int32_t bfgx_fft_pitch(int32_t n_grid) { return fft_pitch(n_grid); }

int64_t bfgx_power_spectrum_work_doubles(int32_t n_grid)
{
    return 2 * (int64_t)n_grid * n_grid * fft_pitch(n_grid);
}

int bfgx_power_spectrum_device(int device, void *hip_stream, int32_t n_grid, const double *map_dev, double L, int32_t nk,
                               double *work_dev, double *pk_sum_dev, double *k_sum_dev, unsigned long long *counts_dev)
{
    if (!map_dev || !work_dev || !pk_sum_dev || !k_sum_dev || !counts_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (nk < 1 || nk > 2048 || !(L > 0)) return fail(BFGX_ERR_INVALID, "power spectrum needs 1 <= nk <= 2048, L > 0");
    if (reinterpret_cast<uintptr_t>(work_dev) & 15) return fail(BFGX_ERR_INVALID, "work_dev must be 16-byte aligned (complex values)");
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    FftSetup *f = nullptr;
    if (int rc = fft_setup(device, n_grid, L, nk, &f)) return rc;
    const int pitch = fft_pitch(n_grid);
    if (int rc = fft_planes(*f, s, n_grid, n_grid, map_dev, (double2 *)work_dev, pitch)) return rc;
    return fft_axis0_pk(*f, s, n_grid, n_grid, 0, (double2 *)work_dev, pitch, nk, pk_sum_dev, k_sum_dev, counts_dev);
}

int bfgx_fft_slab_planes_device(int device, void *hip_stream, int32_t n_grid, int32_t planes, const double *map_dev, double *work_dev)
{
    if (!map_dev || !work_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (planes < 1 || planes > n_grid || ((int64_t)planes * n_grid) % 2) return fail(BFGX_ERR_INVALID, "slab of %d planes", planes);
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    FftSetup *f = nullptr;
    if (int rc = fft_setup(device, n_grid, 1.0, 1, &f)) return rc;
    return fft_planes(*f, s, n_grid, planes, map_dev, (double2 *)work_dev, fft_pitch(n_grid));
}

int bfgx_fft_slab_axis0_pk_device(int device, void *hip_stream, int32_t n_grid, int32_t ncols, int32_t col0, double *work_dev, double L,
                                  int32_t nk, double *pk_sum_dev, double *k_sum_dev, unsigned long long *counts_dev)
{
    if (!work_dev || !pk_sum_dev || !k_sum_dev || !counts_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (nk < 1 || nk > 2048 || !(L > 0)) return fail(BFGX_ERR_INVALID, "power spectrum needs 1 <= nk <= 2048, L > 0");
    if (ncols < 1 || col0 < 0 || col0 + ncols > n_grid) return fail(BFGX_ERR_INVALID, "columns [%d, %d) outside the grid", col0, col0 + ncols);
    if (int rc = select_device(device)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    FftSetup *f = nullptr;
    if (int rc = fft_setup(device, n_grid, L, nk, &f)) return rc;
    return fft_axis0_pk(*f, s, n_grid, ncols, col0, (double2 *)work_dev, fft_pitch(n_grid), nk, pk_sum_dev, k_sum_dev, counts_dev);
}

int bfgx_power_spectrum(int device, int32_t n_grid, const double *map, double L, int32_t nk, double *pk, double *kcen, int64_t *counts)
{
    if (!map || !pk || !kcen || !counts) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (ilog2_exact(n_grid) < 3 || n_grid > 1024) return fail(BFGX_ERR_UNSUPPORTED, "power spectrum needs n_grid = 2^m with 8 <= n_grid <= 1024");
    if (nk < 1 || nk > 2048) return fail(BFGX_ERR_INVALID, "power spectrum needs 1 <= nk <= 2048");
    HostCall c(device);
    const size_t N = n_grid;
    std::vector<double> hp(nk), hk(nk);                      // the bins' sums, divided by their counts below
    std::vector<unsigned long long> hc(nk);
    const double *dm = c.in(map, N * N * N);
    double *dw = c.scratch<double>(bfgx_power_spectrum_work_doubles(n_grid)), *dp = c.out(hp.data(), nk), *dk = c.out(hk.data(), nk);
    unsigned long long *dc = c.out(hc.data(), nk);
    if (int rc = c.ready()) return rc;
    if (int rc = bfgx_power_spectrum_device(device, nullptr, n_grid, dm, L, nk, dw, dp, dk, dc)) return rc;
    if (int rc = c.finish()) return rc;
    for (int i = 0; i < nk; ++i) {
        counts[i] = (int64_t)hc[i];
        pk[i] = hp[i] / (double)hc[i];           // 0 / 0 -> NaN for empty bins, as np.bincount(...) / k_c gives
        kcen[i] = hk[i] / (double)hc[i];
    }
    return BFGX_OK;
}

}  // extern "C"
