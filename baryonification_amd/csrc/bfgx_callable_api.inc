// bfgx_callable_api.inc -- C ABI for models that are Python callables (included at the end of bfgx_api.hip; declared in include/bfgx.h).
//
// The reference calls `self.model.displacement(r_sep / a_j, M_j, a_j)` (HealpixRunner.py:321) / `Baryons.projected(cosmo, r_sep / a_j, M_j,
// a_j)` (:441) once per halo on ANY object.  A model without a table is served in that way, exactly: the device finds every halo's pixels
// and their separations, the caller evaluates its model per halo on its slice of them, the device turns the values into pixel offsets /
// painted values and regrids.  Three calls around one handle; nothing here reads a table (the bfgx_model only carries the runner's
// cosmology, mass definition and epsilon_max; its table must be valid and is ignored).  The handle is a ShellPairs (bfgx_pairs.hpp).

extern "C" {

void bfgx_shell_pairs_end(bfgx_pairs *h) { pairs_end(h); }

int bfgx_shell_pairs_begin(const bfgx_catalog *cat, const bfgx_model *model, int64_t nside, int32_t paint, int32_t device, bfgx_pairs **out,
                           int64_t *counts_host)
{
    if (!cat || !model || !out || (cat->n > 0 && !counts_host)) return fail(BFGX_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (cat->n < 0) return fail(BFGX_ERR_INVALID, "catalog size < 0");
    if (model->table.ndim != 3) return fail(BFGX_ERR_INVALID, "the per-pair entries take a model with a (dummy) 3-axis table: halo properties are the callable's business");
    std::vector<double> hostlog;                  // (read by upload_catalog's copies: declared before the handle, so it outlives the handle's drain)
    PairsOwner<ShellPairs> h(new ShellPairs());
    bfgx_plan *p = nullptr;
    if (int rc = bfgx_plan_create(device, nullptr, nside, std::max<int64_t>(cat->n, 1), model, &p)) return rc;
    h->plan.reset(p);
    h->on(p->device, p->stream);
    h->n = cat->n; h->paint = paint ? 1 : 0;
    if (int rc = upload_catalog(p, cat, h->cols, &h->dcat, hostlog)) return rc;
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (h->counts.alloc(sizeof(int64_t) * (size_t)std::max<int64_t>(cat->n, 1))) return alloc_fail("pair counts");
    // per-halo records for the halo-centric kernels (the < 4-pixel fallback is BaryonifyShell's alone: HealpixRunner.py:309-310 against :432)
    if (int rc = launch_prep(p, &h->dcat, paint ? 0 : 1, false, false, true)) return rc;
    if (int rc = launch_scatter<MODE_COUNT, double>(p, cat->n, (double *)nullptr, (int64_t *)h->counts.p)) return rc;
    if (cat->n > 0) HIP_TRY(hipMemcpyAsync(counts_host, h->counts.p, sizeof(int64_t) * (size_t)cat->n, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (int rc = pairs_offsets(h.get(), counts_host)) return rc;
    if (h->off.alloc(sizeof(int64_t) * h->off_h.size()) || h->vals.alloc(sizeof(double) * (size_t)std::max<int64_t>(h->total, 1)))
        return alloc_fail("pair arrays");
    HIP_TRY(hipMemcpy(h->off.p, h->off_h.data(), sizeof(int64_t) * h->off_h.size(), hipMemcpyHostToDevice));
    *out = h.release();
    return BFGX_OK;
}

int bfgx_shell_pairs_radii(bfgx_pairs *handle, double *r_host)
{
    ShellPairs *h = pairs_as<ShellPairs>(handle);
    if (!h) return pairs_refuse<ShellPairs>();
    bfgx_plan *p = h->plan.get();
    return pairs_to_host(h, h->vals, h->total, r_host, [&](double *r) {
        const unsigned grid = (unsigned)((h->n + kWavesPerBlock - 1) / kWavesPerBlock);
        hipLaunchKernelGGL(halo_pairs_kernel<0>, dim3(grid), dim3(kWave * kWavesPerBlock), 0, p->stream, p->hpx, h->n, (const HaloRec *)p->recs,
                           (const int64_t *)h->off.p, (const double *)nullptr, r, (double *)nullptr);
        HIP_TRY(hipGetLastError());
        return (int)BFGX_OK;
    });
}

int bfgx_shell_pairs_apply(bfgx_pairs *handle, const double *vals_host, const double *map_in, double *map_out, int32_t check_mass, bfgx_stats *stats)
{
    ShellPairs *h = pairs_as<ShellPairs>(handle);
    if (!h) return pairs_refuse<ShellPairs>();
    if (!map_out || (h->total > 0 && !vals_host) || (!h->paint && !map_in)) return fail(BFGX_ERR_INVALID, "NULL argument");
    bfgx_plan *p = h->plan.get();
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
