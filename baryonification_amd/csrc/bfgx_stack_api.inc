// bfgx_stack_api.inc -- C ABI of the halo-centred profile measurement (included at the end of bfgx_api.hip; declared in include/bfgx.h).
//
// MeasureProfilesShell is the adjoint of PaintProfilesShell: the same discs and separations, a gather where painting scatters.  As for the
// per-pair entries (bfgx_callable_api.inc) the bfgx_model only carries the runner's cosmology, mass definition and epsilon_max; its table must
// be valid and is ignored.  Both entries run on the cached shell plan of (device, nside, model) -- K0 without the < 4-pixel fallback, then
// stack_profiles_kernel over the plan's halo records -- so a second call with the same geometry allocates nothing.

namespace {

// everything that can be refused without a device, before anything is allocated
int stack_validate(const bfgx_catalog *cat, const bfgx_model *model, int64_t nside, const double *map, const double *g1, const double *g2,
                   int32_t nb, const double *r_edges, const StackOut &o)
{
    if (!cat || !model || !map || !r_edges || !o.npix || !o.sum) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = profiles_validate_shear(g1, g2, o)) return rc;
    if (int rc = profiles_validate_bins(nb, r_edges)) return rc;
    if (nside < 1 || nside > 8192) return fail(BFGX_ERR_INVALID, "nside must be 1 .. 8192 (the tile kernels index pixels with 32 bits inside a ring table)");
    if (cat->n < 0) return fail(BFGX_ERR_INVALID, "catalog size < 0");
    if (cat->n > 0 && (!cat->M || !cat->z || !cat->ra || !cat->dec)) return fail(BFGX_ERR_INVALID, "catalog column pointer is NULL");
    return profiles_validate_placeholder(model, false);
}

// K0 (no fallback, full records) + the stacking kernel on p->stream; edges_dev: nb + 1 doubles on the device
int stack_launch(bfgx_plan *p, const bfgx_catalog *dcat, const double *map, const double *g1, const double *g2, int32_t nb, const double *edges_dev,
                 int32_t scaled, const StackOut &o)
{
    if (dcat->n == 0) return BFGX_OK;
    if (int rc = launch_prep(p, dcat, 0, false, false, true)) return rc;
    StackArgs a;
    a.map = map; a.g1 = g1; a.g2 = g2; a.M = dcat->M; a.z = dcat->z; a.edges = edges_dev; a.nb = nb; a.scaled = scaled ? 1 : 0; a.out = o;
    const unsigned grid = (unsigned)((dcat->n + kWavesPerBlock - 1) / kWavesPerBlock);
    if (g1)
        hipLaunchKernelGGL(stack_profiles_kernel<true>, dim3(grid), dim3(kWave * kWavesPerBlock), 0, p->stream, p->hpx, p->model.bg_runner,
                           p->model.md_runner, dcat->n, (const HaloRec *)p->recs, a);
    else
        hipLaunchKernelGGL(stack_profiles_kernel<false>, dim3(grid), dim3(kWave * kWavesPerBlock), 0, p->stream, p->hpx, p->model.bg_runner,
                           p->model.md_runner, dcat->n, (const HaloRec *)p->recs, a);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

// the plan's stream for the duration of a call on the caller's stream
struct StreamSwap {
    bfgx_plan *p; hipStream_t old;
    StreamSwap(bfgx_plan *p_, hipStream_t s) : p(p_), old(p_->stream) { p->stream = s; }
    ~StreamSwap() { p->stream = old; }
};

}  // namespace

extern "C" {

int bfgx_shell_profiles(const bfgx_catalog *cat, const bfgx_model *model, int64_t nside, const double *map, const double *g1, const double *g2,
                        int32_t nb, const double *r_edges, int32_t scaled, int32_t device, int64_t *npix, double *sum, int64_t *npix_shear,
                        double *sum_t, double *sum_x)
{
    const StackOut ho{npix, npix_shear, sum, sum_t, sum_x};
    if (int rc = stack_validate(cat, model, nside, map, g1, g2, nb, r_edges, ho)) return rc;
    bfgx_opts o = entry_opts(nullptr);
    o.device = device;
    std::lock_guard<std::mutex> lk(g_shells.mu);
    ShellEntry *e = nullptr;
    if (int rc = shell_begin(cat, model, nside, o, &e)) return rc;
    bfgx_plan *p = e->plan;
    OneShotCall call(&p->stream, e);                 // (its streams are drained at scope exit)
    const size_t npx = (size_t)p->hpx.npix, cells = (size_t)cat->n * (size_t)nb, nmaps = g1 ? 3 : 1, nout = g1 ? 5 : 2;
    std::vector<double> hostlog;
    bfgx_catalog dcat;
    if (int rc = upload_catalog_pooled(e, cat, &dcat, hostlog, 0)) return rc;
    if (e->in.need(nmaps * npx * sizeof(double)) || e->out.need(std::max<size_t>(nout * cells, 1) * sizeof(double)) ||
        e->sums.need((kStackMaxBins + 1) * sizeof(double)))
        return alloc_fail("profile buffers");
    hipStream_t s = p->stream;
    double *dmap = (double *)e->in.p, *dout = (double *)e->out.p;
    HIP_TRY(hipMemcpyAsync(e->sums.p, r_edges, sizeof(double) * (size_t)(nb + 1), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(dmap, map, npx * sizeof(double), hipMemcpyHostToDevice, s));
    if (g1) {
        HIP_TRY(hipMemcpyAsync(dmap + npx, g1, npx * sizeof(double), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(dmap + 2 * npx, g2, npx * sizeof(double), hipMemcpyHostToDevice, s));
    }
    // device outputs, cells each: npix, sum[, npix_shear, sum_t, sum_x]
    const StackOut dv{(int64_t *)dout, (int64_t *)(dout + 2 * cells), dout + cells, dout + 3 * cells, dout + 4 * cells};
    if (int rc = stack_launch(p, &dcat, dmap, g1 ? dmap + npx : nullptr, g1 ? dmap + 2 * npx : nullptr, nb, (const double *)e->sums.p, scaled, dv)) return rc;
    if (int rc = profiles_copy_back(s, ho, dv, cells, g1 != nullptr)) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return BFGX_OK;
}

int bfgx_shell_profiles_device(int32_t device, void *hip_stream, const bfgx_catalog *cat, const bfgx_model *model, int64_t nside,
                               const double *map_dev, const double *g1_dev, const double *g2_dev, int32_t nb, const double *r_edges,
                               int32_t scaled, int64_t *npix_dev, double *sum_dev, int64_t *npix_shear_dev, double *sum_t_dev, double *sum_x_dev)
{
    const StackOut dv{npix_dev, npix_shear_dev, sum_dev, sum_t_dev, sum_x_dev};
    if (int rc = stack_validate(cat, model, nside, map_dev, g1_dev, g2_dev, nb, r_edges, dv)) return rc;
    bfgx_opts o = entry_opts(nullptr);
    o.device = device;
    std::lock_guard<std::mutex> lk(g_shells.mu);
    ShellEntry *e = nullptr;
    // no call scope (nothing is drained): the host entries leave the cached plan idle, and an earlier call of this entry is waited for on the device (below)
    if (int rc = shell_begin(cat, model, nside, o, &e)) return rc;
    bfgx_plan *p = e->plan;
    hipStream_t s = (hipStream_t)hip_stream;
    StreamSwap swap(p, s);                       // K0 and the catalog copies of this call go to the caller's stream
    if (s != swap.old) HIP_TRY(hipStreamWaitEvent(s, e->ev[3], 0));
    std::vector<double> hostlog;
    bfgx_catalog dcat;
    if (int rc = upload_catalog_pooled(e, cat, &dcat, hostlog, 0)) return rc;
    if (e->sums.need((kStackMaxBins + 1) * sizeof(double))) return alloc_fail("profile buffers");
    // (copies from pageable host memory have left the caller's arrays when hipMemcpyAsync returns)
    HIP_TRY(hipMemcpyAsync(e->sums.p, r_edges, sizeof(double) * (size_t)(nb + 1), hipMemcpyHostToDevice, s));
    if (int rc = stack_launch(p, &dcat, map_dev, g1_dev, g2_dev, nb, (const double *)e->sums.p, scaled, dv)) return rc;
    // the plan's own stream (the next call's) waits for this one: the halo records, the catalog columns and the edges are shared
    if (s != swap.old) {
        HIP_TRY(hipEventRecord(e->ev[3], s));
        HIP_TRY(hipStreamWaitEvent(swap.old, e->ev[3], 0));
    }
    return BFGX_OK;
}

}  // extern "C"
