// bfgx_grid_pairs_api.inc -- C ABI of the regular-grid runners for models that are Python callables (included at the end of bfgx_api.hip,
// after bfgx_callable_api.inc whose bfgx_pairs handle it shares; declared in include/bfgx.h).
//
// BaryonifyGrid / PaintProfilesGrid call model.displacement(r, M_j, a_j) / profile(cosmo, r, M_j, a_j) once per halo on the radii of the halo's
// whole cutout (Map2DRunner.py:534, :577, :801).  begin finds every halo's cutout, radii hands out the radii of a range of halos, the caller
// evaluates its model on them, apply accumulates the values of that range on the device, finish regrids (or returns the painted map).  The
// host holds one batch of radii and values at a time; the device keeps the per-halo geometry and the accumulated offsets.

namespace {

template <int DIM, int MODE>
void launch_grid_pairs_t(bfgx_pairs *h, int64_t j0, int64_t j1, const double *vals, double *out)
{
    bfgx_grid_plan *p = h->gplan;
    const int64_t it0 = h->item0_h[(size_t)j0], it1 = h->item0_h[(size_t)j1];
    const unsigned blocks = (unsigned)std::min<int64_t>(it1 - it0, (int64_t)p->n_cu * 8);
    hipLaunchKernelGGL((grid_pairs_kernel<DIM, MODE>), dim3(blocks), dim3(kGridBlock), 0, p->stream, p->geom, (const GridHaloRec *)p->recs,
                       (const int32_t *)h->item_halo.p, (const int64_t *)h->item0.p, (const int64_t *)h->off.p, it0, it1, h->off_h[(size_t)j0], vals, out);
}

template <int MODE>
int launch_grid_pairs(bfgx_pairs *h, int64_t j0, int64_t j1, const double *vals, double *out)
{
    if (h->item0_h[(size_t)j1] == h->item0_h[(size_t)j0]) return BFGX_OK;
    if (h->gplan->geom.ndim == 3) launch_grid_pairs_t<3, MODE>(h, j0, j1, vals, out);
    else launch_grid_pairs_t<2, MODE>(h, j0, j1, vals, out);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

int grid_pairs_range(const bfgx_pairs *h, int64_t j0, int64_t j1)
{
    if (!h || !h->gplan) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (j0 < 0 || j1 < j0 || j1 > h->n) return fail(BFGX_ERR_INVALID, "halo range [%lld, %lld) outside [0, %lld)", (long long)j0, (long long)j1, (long long)h->n);
    return BFGX_OK;
}

}  // namespace

extern "C" {

void bfgx_grid_pairs_end(bfgx_pairs *h) { bfgx_shell_pairs_end(h); }

int bfgx_grid_pairs_begin(const bfgx_grid_catalog *cat, const bfgx_model *model, const bfgx_grid *grid, int32_t paint, int32_t device, bfgx_pairs **out,
                          int64_t *counts_host)
{
    if (!cat || !model || !grid || !out || (cat->n > 0 && !counts_host)) return fail(BFGX_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (cat->n < 0) return fail(BFGX_ERR_INVALID, "catalog size < 0");
    if (cat->n > INT32_MAX) return fail(BFGX_ERR_INVALID, "more than 2^31 halos");
    if (cat->n > 0 && (!cat->M || !cat->x || !cat->y || (grid->ndim == 3 && !cat->z))) return fail(BFGX_ERR_INVALID, "catalog column pointer is NULL");
    if (model->table.ndim != 3) return fail(BFGX_ERR_INVALID, "the per-pair entries take a model with a (dummy) 3-axis table: halo properties are the callable's business");
    if (cat->rmat && grid->ndim == 3) return fail(BFGX_ERR_UNSUPPORTED, "use_ellipticity is not implemented for 3D maps");
    bfgx_pairs *h = new bfgx_pairs();
    auto bail = [&](int rc) { bfgx_grid_pairs_end(h); return rc; };
    if (int rc = bfgx_grid_plan_create(device, nullptr, grid, std::max<int64_t>(cat->n, 1), model, &h->gplan)) { h->gplan = nullptr; return bail(rc); }
    bfgx_grid_plan *p = h->gplan;
    const int64_t n = cat->n;
    h->n = n; h->paint = paint ? 1 : 0;
    if (int rc = h->gcat.upload(cat, grid->ndim, 0, p->stream)) return bail(rc);
    if (h->counts.alloc(sizeof(int64_t) * (size_t)std::max<int64_t>(n, 1))) return bail(alloc_fail("pair counts"));
    int32_t flags = 0;
    if (hipMemsetAsync(p->counters, 0, 2 * sizeof(int32_t), p->stream) != hipSuccess) return bail(fail(BFGX_ERR_HIP, "memset failed"));
    if (n > 0) {
        GridCatalog gc;
        std::memset(&gc, 0, sizeof(gc));
        const bfgx_grid_catalog &d = h->gcat.d;
        gc.n = n; gc.M = d.M; gc.x = d.x; gc.y = d.y; gc.z = d.z; gc.rmat = d.rmat;
        hipLaunchKernelGGL(grid_pairs_prep_kernel, dim3((unsigned)((n + kGridBlock - 1) / kGridBlock)), dim3(kGridBlock), 0, p->stream, p->model, p->geom,
                           gc, h->paint, p->recs, (int64_t *)h->counts.p, p->counters + 1);
        if (hipGetLastError() != hipSuccess) return bail(fail(BFGX_ERR_HIP, "grid_pairs_prep_kernel launch failed"));
        if (hipMemcpyAsync(counts_host, h->counts.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, p->stream) != hipSuccess)
            return bail(fail(BFGX_ERR_HIP, "copy(pair counts) failed"));
    }
    if (hipMemcpyAsync(&flags, p->counters + 1, sizeof(int32_t), hipMemcpyDeviceToHost, p->stream) != hipSuccess ||
        hipStreamSynchronize(p->stream) != hipSuccess)
        return bail(fail(BFGX_ERR_HIP, "stream sync failed"));
    if (flags & 1) return bail(fail(BFGX_ERR_ASSERT, "Halo offsets are larger than res (Map2DRunner.py:516)"));
    h->off_h.assign((size_t)n + 1, 0);
    h->item0_h.assign((size_t)n + 1, 0);
    for (int64_t j = 0; j < n; ++j) {
        if (counts_host[j] < 0) return bail(fail(BFGX_ERR_HIP, "negative pair count"));
        h->off_h[(size_t)j + 1] = h->off_h[(size_t)j] + counts_host[j];
        h->item0_h[(size_t)j + 1] = h->item0_h[(size_t)j] + (counts_host[j] + kGridChunk - 1) / kGridChunk;
    }
    h->total = h->off_h[(size_t)n];
    const int64_t nitems = h->item0_h[(size_t)n];
    if (nitems > INT32_MAX) return bail(fail(BFGX_ERR_INVALID, "more than 2^31 work items (%d-pixel chunks): catalog too large for one call", kGridChunk));
    if (h->off.alloc(sizeof(int64_t) * ((size_t)n + 1)) || h->item0.alloc(sizeof(int64_t) * ((size_t)n + 1)) ||
        h->item_halo.alloc(sizeof(int32_t) * (size_t)std::max<int64_t>(nitems, 1)))
        return bail(alloc_fail("pair tables"));
    const size_t ntot = (size_t)p->geom.ntot, acc_n = h->paint ? ntot : (size_t)p->geom.ndim * ntot;
    if (h->acc.need(acc_n * sizeof(double))) return bail(alloc_fail("accumulator"));
    if (hipMemcpyAsync(h->off.p, h->off_h.data(), sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, p->stream) != hipSuccess ||
        hipMemcpyAsync(h->item0.p, h->item0_h.data(), sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, p->stream) != hipSuccess ||
        hipMemsetAsync(h->acc.p, 0, acc_n * sizeof(double), p->stream) != hipSuccess)
        return bail(fail(BFGX_ERR_HIP, "copy(pair tables) failed"));
    if (n > 0) {
        hipLaunchKernelGGL(grid_pairs_items_kernel, dim3((unsigned)((n + kGridBlock - 1) / kGridBlock)), dim3(kGridBlock), 0, p->stream, n,
                           (const int64_t *)h->item0.p, (int32_t *)h->item_halo.p);
        if (hipGetLastError() != hipSuccess) return bail(fail(BFGX_ERR_HIP, "grid_pairs_items_kernel launch failed"));
    }
    if (hipStreamSynchronize(p->stream) != hipSuccess) return bail(fail(BFGX_ERR_HIP, "stream sync failed"));    // (off_h / item0_h stay put)
    *out = h;
    return BFGX_OK;
}

int bfgx_grid_pairs_radii(bfgx_pairs *h, int64_t j0, int64_t j1, double *r_host)
{
    if (int rc = grid_pairs_range(h, j0, j1)) return rc;
    const int64_t np = h->off_h[(size_t)j1] - h->off_h[(size_t)j0];
    if (np > 0 && !r_host) return fail(BFGX_ERR_INVALID, "NULL argument");
    bfgx_grid_plan *p = h->gplan;
    HIP_TRY(hipSetDevice(p->device));
    if (np > 0) {
        if (h->batch.need(sizeof(double) * (size_t)np)) return alloc_fail("pair batch");
        if (int rc = launch_grid_pairs<0>(h, j0, j1, nullptr, (double *)h->batch.p)) return rc;
        HIP_TRY(hipMemcpyAsync(r_host, h->batch.p, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, p->stream));
    }
    HIP_TRY(hipStreamSynchronize(p->stream));
    return BFGX_OK;
}

int bfgx_grid_pairs_apply(bfgx_pairs *h, int64_t j0, int64_t j1, const double *vals_host)
{
    if (int rc = grid_pairs_range(h, j0, j1)) return rc;
    const int64_t np = h->off_h[(size_t)j1] - h->off_h[(size_t)j0];
    if (np > 0 && !vals_host) return fail(BFGX_ERR_INVALID, "NULL argument");
    bfgx_grid_plan *p = h->gplan;
    HIP_TRY(hipSetDevice(p->device));
    if (np > 0) {
        if (h->batch.need(sizeof(double) * (size_t)np)) return alloc_fail("pair batch");
        HIP_TRY(hipMemcpyAsync(h->batch.p, vals_host, sizeof(double) * (size_t)np, hipMemcpyHostToDevice, p->stream));
        const int rc = h->paint ? launch_grid_pairs<2>(h, j0, j1, (const double *)h->batch.p, (double *)h->acc.p)
                                : launch_grid_pairs<1>(h, j0, j1, (const double *)h->batch.p, (double *)h->acc.p);
        if (rc) return rc;
    }
    HIP_TRY(hipStreamSynchronize(p->stream));         // (vals_host is the caller's again on return)
    return BFGX_OK;
}

int bfgx_grid_pairs_finish(bfgx_pairs *h, const double *map_in, double *map_out, int32_t check_mass, bfgx_stats *stats)
{
    if (!h || !h->gplan || !map_out || (!h->paint && !map_in)) return fail(BFGX_ERR_INVALID, "NULL argument");
    bfgx_grid_plan *p = h->gplan;
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t s = p->stream;
    const size_t ntot = (size_t)p->geom.ntot;
    double sums[2] = {0, 0};
    if (h->paint) {
        HIP_TRY(hipMemcpyAsync(map_out, h->acc.p, ntot * sizeof(double), hipMemcpyDeviceToHost, s));
    } else {
        if (h->in.need(ntot * sizeof(double)) || h->out.need(ntot * sizeof(double)) || h->sums.need(2 * sizeof(double)))
            return alloc_fail("map buffers");
        HIP_TRY(hipMemcpyAsync(h->in.p, map_in, ntot * sizeof(double), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(h->sums.p, 0, 2 * sizeof(double), s));
        if (int rc = bfgx_grid_regrid_device(p, (const double *)h->in.p, (const double *)h->acc.p, (double *)h->out.p, (double *)h->sums.p)) return rc;
        HIP_TRY(hipMemcpyAsync(map_out, h->out.p, ntot * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(sums, h->sums.p, sizeof(sums), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    fill_stats(stats, sums, h->total, 0, 0, 0);
    return (!h->paint && check_mass) ? ::check_mass(sums[0], sums[1]) : BFGX_OK;      // (Map2DRunner.py:601-605)
}

}  // extern "C"
