// bfgx_grid_pairs_api.inc -- C ABI of the regular-grid runners for models that are Python callables (included at the end of bfgx_api.hip,
// after bfgx_pairs.hpp: the handle is a GridPairs; declared in include/bfgx.h).
//
// BaryonifyGrid / PaintProfilesGrid call model.displacement(r, M_j, a_j) / profile(cosmo, r, M_j, a_j) once per halo on the radii of the halo's
// whole cutout (Map2DRunner.py:534, :577, :801).  begin finds every halo's cutout, radii hands out the radii of a range of halos, the caller
// evaluates its model on them, apply accumulates the values of that range on the device, finish regrids (or returns the painted map).  The
// host holds one batch of radii and values at a time; the device keeps the per-halo geometry and the accumulated offsets.

namespace {

template <int MODE>
int launch_grid_pairs(GridPairs *h, int64_t j0, int64_t j1, const double *vals, double *out)
{
    bfgx_grid_plan *p = h->plan.get();
    const int64_t it0 = h->item0_h[(size_t)j0], it1 = h->item0_h[(size_t)j1];
    if (it1 == it0) return BFGX_OK;
    const unsigned blocks = (unsigned)std::min<int64_t>(it1 - it0, (int64_t)p->n_cu * 8);
    grid_dim(p->geom.ndim, [&](auto dim) {
        hipLaunchKernelGGL((grid_pairs_kernel<decltype(dim)::value, MODE>), dim3(blocks), dim3(kGridBlock), 0, p->stream, p->geom, (const GridHaloRec *)p->recs,
                           (const int32_t *)h->item_halo.p, (const int64_t *)h->item0.p, (const int64_t *)h->off.p, it0, it1, h->off_h[(size_t)j0], vals, out);
    });
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

}  // namespace

extern "C" {

void bfgx_grid_pairs_end(bfgx_pairs *h) { pairs_end(h); }

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
    int32_t flags = 0;                            // (written by a copy on the handle's stream: declared before the handle, so it outlives the handle's drain)
    PairsOwner<GridPairs> h(new GridPairs());
    bfgx_grid_plan *p = nullptr;
    if (int rc = bfgx_grid_plan_create(device, nullptr, grid, std::max<int64_t>(cat->n, 1), model, &p)) return rc;
    h->plan.reset(p);
    h->on(p->device, p->stream);
    const int64_t n = cat->n;
    h->n = n; h->paint = paint ? 1 : 0;
    if (int rc = h->cat.upload(cat, grid->ndim, 0, p->stream)) return rc;
    if (h->counts.alloc(sizeof(int64_t) * (size_t)std::max<int64_t>(n, 1))) return alloc_fail("pair counts");
    HIP_TRY(hipMemsetAsync(p->counters, 0, 2 * sizeof(int32_t), p->stream));
    if (n > 0) {
        GridCatalog gc;
        std::memset(&gc, 0, sizeof(gc));
        const bfgx_grid_catalog &d = h->cat.d;
        gc.n = n; gc.M = d.M; gc.x = d.x; gc.y = d.y; gc.z = d.z; gc.rmat = d.rmat;
        hipLaunchKernelGGL(grid_pairs_prep_kernel, dim3((unsigned)((n + kGridBlock - 1) / kGridBlock)), dim3(kGridBlock), 0, p->stream, p->model, p->geom,
                           gc, h->paint, p->recs, (int64_t *)h->counts.p, p->counters + 1);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(counts_host, h->counts.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, p->stream));
    }
    HIP_TRY(hipMemcpyAsync(&flags, p->counters + 1, sizeof(int32_t), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (flags & 1) return fail(BFGX_ERR_ASSERT, "Halo offsets are larger than res (Map2DRunner.py:516)");
    if (int rc = pairs_offsets(h.get(), counts_host)) return rc;
    h->item0_h.assign((size_t)n + 1, 0);
    for (int64_t j = 0; j < n; ++j) h->item0_h[(size_t)j + 1] = h->item0_h[(size_t)j] + (counts_host[j] + kGridChunk - 1) / kGridChunk;
    const int64_t nitems = h->item0_h[(size_t)n];
    if (nitems > INT32_MAX) return fail(BFGX_ERR_INVALID, "more than 2^31 work items (%d-pixel chunks): catalog too large for one call", kGridChunk);
    if (h->off.alloc(sizeof(int64_t) * ((size_t)n + 1)) || h->item0.alloc(sizeof(int64_t) * ((size_t)n + 1)) ||
        h->item_halo.alloc(sizeof(int32_t) * (size_t)std::max<int64_t>(nitems, 1)))
        return alloc_fail("pair tables");
    const size_t ntot = (size_t)p->geom.ntot, acc_n = h->paint ? ntot : (size_t)p->geom.ndim * ntot;
    if (h->acc.need(acc_n * sizeof(double))) return alloc_fail("accumulator");
    HIP_TRY(hipMemcpyAsync(h->off.p, h->off_h.data(), sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipMemcpyAsync(h->item0.p, h->item0_h.data(), sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipMemsetAsync(h->acc.p, 0, acc_n * sizeof(double), p->stream));
    if (n > 0) {
        hipLaunchKernelGGL(grid_pairs_items_kernel, dim3((unsigned)((n + kGridBlock - 1) / kGridBlock)), dim3(kGridBlock), 0, p->stream, n,
                           (const int64_t *)h->item0.p, (int32_t *)h->item_halo.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(p->stream));     // (off_h / item0_h stay put)
    *out = h.release();
    return BFGX_OK;
}

int bfgx_grid_pairs_radii(bfgx_pairs *handle, int64_t j0, int64_t j1, double *r_host)
{
    GridPairs *h = pairs_as<GridPairs>(handle);
    int64_t np = 0;
    if (int rc = pairs_range(h, j0, j1, &np)) return rc;
    return pairs_to_host(h, h->batch, np, r_host, [&](double *r) { return launch_grid_pairs<0>(h, j0, j1, nullptr, r); });
}

int bfgx_grid_pairs_apply(bfgx_pairs *handle, int64_t j0, int64_t j1, const double *vals_host)
{
    GridPairs *h = pairs_as<GridPairs>(handle);
    int64_t np = 0;
    if (int rc = pairs_range(h, j0, j1, &np)) return rc;
    return pairs_from_host(h, h->batch, np, vals_host, [&](const double *v) {
        return h->paint ? launch_grid_pairs<2>(h, j0, j1, v, (double *)h->acc.p) : launch_grid_pairs<1>(h, j0, j1, v, (double *)h->acc.p);
    });
}

int bfgx_grid_pairs_finish(bfgx_pairs *handle, const double *map_in, double *map_out, int32_t check_mass, bfgx_stats *stats)
{
    GridPairs *h = pairs_as<GridPairs>(handle);
    if (!h) return pairs_refuse<GridPairs>();
    if (!map_out || (!h->paint && !map_in)) return fail(BFGX_ERR_INVALID, "NULL argument");
    bfgx_grid_plan *p = h->plan.get();
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
