// bfgx_callable_api.inc -- C ABI for models that are Python callables (included at the end of bfgx_api.hip; declared in include/bfgx.h).
//
// The reference calls `self.model.displacement(r_sep / a_j, M_j, a_j)` (HealpixRunner.py:321) / `Baryons.projected(cosmo, r_sep / a_j, M_j,
// a_j)` (:441) once per halo on ANY object.  A model without a table is served in that way, exactly: the device finds every halo's pixels
// and their separations, the caller evaluates its model per halo on its slice of them, the device turns the values into pixel offsets /
// painted values and regrids.  Three calls around one handle; nothing here reads a table (the bfgx_model only carries the runner's
// cosmology, mass definition and epsilon_max; its table must be valid and is ignored).

struct bfgx_pairs {
    bfgx_plan *plan = nullptr;
    DevBuf cols[kCatCols];
    bfgx_catalog dcat;
    int64_t n = 0, total = 0;
    int paint = 0;
    DevBuf off, vals, counts;
    PoolBuf acc, in, out, sums;
    // the regular-grid runners' handle (bfgx_grid_pairs_*, bfgx_grid_pairs_api.inc): plan == nullptr, gplan != nullptr
    bfgx_grid_plan *gplan = nullptr;
    GridHostCatalog gcat;
    DevBuf item0, item_halo;
    PoolBuf batch;
    std::vector<int64_t> off_h, item0_h;
    // BaryonifySnapshot's handle (bfgx_snapshot_pairs_*, bfgx_snapshot_pairs_api.inc): sdev >= 0
    int sdev = -1;
    hipStream_t sstream = nullptr;
    SnapGeom sg;
    DevModel smodel;
    DevList smem;
    int64_t snp = 0;
    DevBuf sxyz[3], srecs, skeys, sacc;
};

extern "C" {

void bfgx_shell_pairs_end(bfgx_pairs *h)
{
    if (!h) return;
    if (h->plan) { (void)hipSetDevice(h->plan->device); (void)hipStreamSynchronize(h->plan->stream); }
    if (h->gplan) { (void)hipSetDevice(h->gplan->device); (void)hipStreamSynchronize(h->gplan->stream); }
    if (h->sdev >= 0) { (void)hipSetDevice(h->sdev); (void)hipStreamSynchronize(h->sstream); }
    bfgx_plan *p = h->plan;
    bfgx_grid_plan *gp = h->gplan;
    hipStream_t ss = h->sstream;
    delete h;                       // (device buffers first: they were allocated on the plan's device)
    if (p) bfgx_plan_destroy(p);
    if (gp) bfgx_grid_plan_destroy(gp);
    if (ss) (void)hipStreamDestroy(ss);
}

int bfgx_shell_pairs_begin(const bfgx_catalog *cat, const bfgx_model *model, int64_t nside, int32_t paint, int32_t device, bfgx_pairs **out,
                           int64_t *counts_host)
{
    if (!cat || !model || !out || (cat->n > 0 && !counts_host)) return fail(BFGX_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (cat->n < 0) return fail(BFGX_ERR_INVALID, "catalog size < 0");
    if (model->table.ndim != 3) return fail(BFGX_ERR_INVALID, "the per-pair entries take a model with a (dummy) 3-axis table: halo properties are the callable's business");
    bfgx_pairs *h = new bfgx_pairs();
    auto bail = [&](int rc) { bfgx_shell_pairs_end(h); return rc; };
    if (int rc = bfgx_plan_create(device, nullptr, nside, std::max<int64_t>(cat->n, 1), model, &h->plan)) { h->plan = nullptr; return bail(rc); }
    bfgx_plan *p = h->plan;
    h->n = cat->n; h->paint = paint ? 1 : 0;
    std::vector<double> hostlog;
    if (int rc = upload_catalog(p, cat, h->cols, &h->dcat, hostlog)) return bail(rc);
    if (hipStreamSynchronize(p->stream) != hipSuccess) return bail(fail(BFGX_ERR_HIP, "stream sync failed"));       // (hostlog leaves scope)
    if (h->counts.alloc(sizeof(int64_t) * (size_t)std::max<int64_t>(cat->n, 1))) return bail(alloc_fail("pair counts"));
    // per-halo records for the halo-centric kernels (the < 4-pixel fallback is BaryonifyShell's alone: HealpixRunner.py:309-310 against :432)
    if (int rc = launch_prep(p, &h->dcat, paint ? 0 : 1, false, false, true)) return bail(rc);
    if (int rc = launch_scatter<MODE_COUNT, double>(p, cat->n, (double *)nullptr, (int64_t *)h->counts.p)) return bail(rc);
    if (cat->n > 0 && hipMemcpyAsync(counts_host, h->counts.p, sizeof(int64_t) * (size_t)cat->n, hipMemcpyDeviceToHost, p->stream) != hipSuccess)
        return bail(fail(BFGX_ERR_HIP, "copy(pair counts) failed"));
    if (hipStreamSynchronize(p->stream) != hipSuccess) return bail(fail(BFGX_ERR_HIP, "stream sync failed"));
    std::vector<int64_t> off((size_t)cat->n + 1, 0);
    for (int64_t j = 0; j < cat->n; ++j) {
        if (counts_host[j] < 0) return bail(fail(BFGX_ERR_HIP, "negative pair count"));
        off[(size_t)j + 1] = off[(size_t)j] + counts_host[j];
    }
    h->total = off[(size_t)cat->n];
    if (h->off.alloc(sizeof(int64_t) * off.size()) || h->vals.alloc(sizeof(double) * (size_t)std::max<int64_t>(h->total, 1)))
        return bail(alloc_fail("pair arrays"));
    if (hipMemcpy(h->off.p, off.data(), sizeof(int64_t) * off.size(), hipMemcpyHostToDevice) != hipSuccess) return bail(fail(BFGX_ERR_HIP, "copy(pair offsets) failed"));
    *out = h;
    return BFGX_OK;
}

int bfgx_shell_pairs_radii(bfgx_pairs *h, double *r_host)
{
    if (!h || !h->plan || (h->total > 0 && !r_host)) return fail(BFGX_ERR_INVALID, "NULL argument");
    bfgx_plan *p = h->plan;
    HIP_TRY(hipSetDevice(p->device));
    if (h->n > 0 && h->total > 0) {
        const unsigned grid = (unsigned)((h->n + kWavesPerBlock - 1) / kWavesPerBlock);
        hipLaunchKernelGGL(halo_pairs_kernel<0>, dim3(grid), dim3(kWave * kWavesPerBlock), 0, p->stream, p->hpx, h->n, (const HaloRec *)p->recs,
                           (const int64_t *)h->off.p, (const double *)nullptr, (double *)h->vals.p, (double *)nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(r_host, h->vals.p, sizeof(double) * (size_t)h->total, hipMemcpyDeviceToHost, p->stream));
    }
    HIP_TRY(hipStreamSynchronize(p->stream));
    return BFGX_OK;
}

int bfgx_shell_pairs_apply(bfgx_pairs *h, const double *vals_host, const double *map_in, double *map_out, int32_t check_mass, bfgx_stats *stats)
{
    if (!h || !h->plan || !map_out || (h->total > 0 && !vals_host) || (!h->paint && !map_in)) return fail(BFGX_ERR_INVALID, "NULL argument");
    bfgx_plan *p = h->plan;
    HIP_TRY(hipSetDevice(p->device));
    const size_t npix = (size_t)p->hpx.npix;
    const size_t acc_n = h->paint ? npix : 3 * npix;
    if (h->acc.need(acc_n * sizeof(double)) || (!h->paint && (h->in.need(npix * sizeof(double)) || h->out.need(npix * sizeof(double)) || h->sums.need(40 * sizeof(double)))))
        return alloc_fail("map buffers");
    hipStream_t s = p->stream;
    HIP_TRY(hipMemsetAsync(h->acc.p, 0, acc_n * sizeof(double), s));
    if (h->total > 0) HIP_TRY(hipMemcpyAsync(h->vals.p, vals_host, sizeof(double) * (size_t)h->total, hipMemcpyHostToDevice, s));
    if (h->n > 0 && h->total > 0) {
        const unsigned grid = (unsigned)((h->n + kWavesPerBlock - 1) / kWavesPerBlock);
        if (h->paint)
            hipLaunchKernelGGL(halo_pairs_kernel<2>, dim3(grid), dim3(kWave * kWavesPerBlock), 0, s, p->hpx, h->n, (const HaloRec *)p->recs,
                               (const int64_t *)h->off.p, (const double *)h->vals.p, (double *)nullptr, (double *)h->acc.p);
        else
            hipLaunchKernelGGL(halo_pairs_kernel<1>, dim3(grid), dim3(kWave * kWavesPerBlock), 0, s, p->hpx, h->n, (const HaloRec *)p->recs,
                               (const int64_t *)h->off.p, (const double *)h->vals.p, (double *)nullptr, (double *)h->acc.p);
        HIP_TRY(hipGetLastError());
    }
    double sums[2] = {0, 0};
    if (h->paint) {
        HIP_TRY(hipMemcpyAsync(map_out, h->acc.p, npix * sizeof(double), hipMemcpyDeviceToHost, s));
    } else {
        HIP_TRY(hipMemcpyAsync(h->in.p, map_in, npix * sizeof(double), hipMemcpyHostToDevice, s));
        if (int rc = regrid_impl(p, (const double *)h->in.p, h->acc.p, DispMode{DispMode::F64}, (double *)h->out.p, (double *)h->sums.p, false)) return rc;
        HIP_TRY(hipMemcpyAsync(map_out, h->out.p, npix * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(sums, h->sums.p, sizeof(sums), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    if (!h->paint) if (int rc = bfgx_plan_status(p)) return rc;
    fill_stats(stats, sums, h->total, 0, 0, 0);
    return (!h->paint && check_mass) ? ::check_mass(sums[0], sums[1]) : BFGX_OK;      // (HealpixRunner.py:344-346)
}

}  // extern "C"
