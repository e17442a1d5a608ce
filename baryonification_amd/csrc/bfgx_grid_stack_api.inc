// bfgx_grid_stack_api.inc -- C ABI of the halo-centred profile measurement on gridded maps (included at the end of bfgx_api.hip; declared
// in include/bfgx.h).
//
// MeasureProfilesGrid is the third measurement: shell, box and grid share one interface.  The ball and its clipping are BaryonifyGrid's
// (grid_pairs_prep_kernel's valid rule, GridGeom::half_box), the separations are true minimum-image distances between pixel centres and
// the halo (bfgx_grid_stack.hpp).  As for the sibling entries the bfgx_model only carries the runner's cosmology, mass definition and
// epsilon_max; its table must be valid and is ignored.  Both entries run grid_profiles_run: halo records, then grid_stack_kernel.

namespace {

// everything that can be refused without a device, before anything is allocated
int grid_profiles_validate(const bfgx_grid_catalog *c, const bfgx_model *model, const bfgx_grid *grid, const double *map, const double *g1,
                           const double *g2, int32_t nb, const double *r_edges, const StackOut &o)
{
    if (!c || !model || !grid || !map || !r_edges || !o.npix || !o.sum) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = profiles_validate_shear(g1, g2, o)) return rc;
    if (!g1 && (o.npix_shear || o.sum_t || o.sum_x)) return fail(BFGX_ERR_INVALID, "npix_shear, sum_t and sum_x go with a shear pair: they must be NULL without one");
    if (int rc = profiles_validate_bins(nb, r_edges)) return rc;
    if (int rc = validate_grid(grid)) return rc;
    if (g1 && grid->ndim == 3) return fail(BFGX_ERR_INVALID, "the shear pair is flat-sky: it is accepted for 2D grids only");
    {
        const double res = grid->bins[1] - grid->bins[0];
        for (int i = 0; i < grid->npix; ++i)
            if (!std::isfinite(grid->bins[i])) return fail(BFGX_ERR_INVALID, "grid bins must be finite");
        for (int i = 1; i < grid->npix; ++i)
            if (!(std::fabs((grid->bins[i] - grid->bins[i - 1]) - res) <= 1e-9 * res))
                return fail(BFGX_ERR_INVALID, "grid bins must be uniformly spaced (to 1e-9 res): the minimum image needs a period");
    }
    if (c->n < 0) return fail(BFGX_ERR_INVALID, "catalog size < 0");
    if (c->n > INT32_MAX) return fail(BFGX_ERR_INVALID, "more than 2^31 halos");
    if (c->n > 0 && (!c->M || !c->x || !c->y || (grid->ndim == 3 && !c->z))) return fail(BFGX_ERR_INVALID, "catalog column pointer is NULL");
    if (int rc = profiles_validate_placeholder(model, true)) return rc;
    if (bfgx_device_count() <= 0) return fail(BFGX_ERR_NO_DEVICE, "no HIP device visible: libbfgx has no CPU fallback");
    return BFGX_OK;
}

// The measurement on stream st: map / g1 / g2 and the outputs are DEVICE pointers; the halo columns, the bins and the edges are host arrays.
// The stream is drained before this returns, on every path: the workspace is released at scope exit.
int grid_profiles_run(hipStream_t st, const bfgx_grid_catalog *c, const bfgx_model *model, const bfgx_grid *grid, const double *map, const double *g1,
                      const double *g2, int32_t nb, const double *r_edges, int32_t scaled, const StackOut &o)
{
    const int64_t nh = c->n;
    if (nh == 0) return BFGX_OK;                   // (there is no cell to write)
    DevBuf hcol[4], recs, edges, bins;
    hipStream_t stream = st;
    DrainOnExit drain;                             // (declared last: the stream is drained before the buffers above are released)
    drain.s[0] = &stream; drain.null_stream = (st == nullptr);
    if (int rc = upload_halo_columns(st, c, grid->ndim, nh, hcol)) return rc;
    if (recs.alloc(sizeof(GridStackRec) * (size_t)nh) || edges.alloc(sizeof(double) * (kStackMaxBins + 1)) ||
        bins.alloc(sizeof(double) * (size_t)grid->npix))
        return alloc_fail("halo records");
    HIP_TRY(hipMemcpyAsync(edges.p, r_edges, sizeof(double) * (size_t)(nb + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(bins.p, grid->bins, sizeof(double) * (size_t)grid->npix, hipMemcpyHostToDevice, st));
    GridGeom g;
    g.ndim = grid->ndim; g.npix = grid->npix; g.bins = bins.as<double>();
    g.res = grid->bins[1] - grid->bins[0];
    double bmax = grid->bins[0];
    for (int i = 1; i < grid->npix; ++i) bmax = std::max(bmax, grid->bins[i]);
    g.half_box = bmax / 2;                         // BaryonifyGrid's clip (Map2DRunner.py:488)
    g.a = 1.0 / (1.0 + grid->redshift);
    g.ntot = 1;
    for (int d = 0; d < grid->ndim; ++d) g.ntot *= grid->npix;
    g.slab_lo = 0; g.slab_n = grid->npix;
    hipLaunchKernelGGL(grid_stack_prep_kernel, dim3((unsigned)((nh + kGridBlock - 1) / kGridBlock)), dim3(kGridBlock), 0, st,
                       make_background(model->cosmo_runner), model->massdef_runner, model->eps_runner, g, nh, hcol[0].as<double>(),
                       hcol[1].as<double>(), hcol[2].as<double>(), hcol[3].as<double>(), recs.as<GridStackRec>());
    HIP_TRY(hipGetLastError());
    GridStackArgs a;
    a.map = map; a.g1 = g1; a.g2 = g2; a.edges = edges.as<double>(); a.nb = nb; a.scaled = scaled ? 1 : 0; a.out = o;
    const dim3 grd((unsigned)std::min<int64_t>(nh, 8192)), block(kGridStackThreads);
    const GridStackRec *rp = recs.as<GridStackRec>();
    if (g.ndim == 3) hipLaunchKernelGGL((grid_stack_kernel<3, false>), grd, block, 0, st, g, nh, rp, a);
    else if (g1) hipLaunchKernelGGL((grid_stack_kernel<2, true>), grd, block, 0, st, g, nh, rp, a);
    else hipLaunchKernelGGL((grid_stack_kernel<2, false>), grd, block, 0, st, g, nh, rp, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return BFGX_OK;
}

}  // namespace

extern "C" {

int bfgx_grid_profiles(const bfgx_grid_catalog *halos_host, const bfgx_model *model, const bfgx_grid *grid, const double *map_host,
                       const double *g1_host, const double *g2_host, int32_t nb, const double *r_edges, int32_t scaled, int32_t device,
                       int64_t *npix, double *sum, int64_t *npix_shear, double *sum_t, double *sum_x)
{
    const StackOut ho{npix, npix_shear, sum, sum_t, sum_x};
    if (int rc = grid_profiles_validate(halos_host, model, grid, map_host, g1_host, g2_host, nb, r_edges, ho)) return rc;
    HIP_TRY(hipSetDevice(device));
    // nothing is left in flight on any return path: `drain` (declared after the device buffers, so destroyed before them) drains the call's
    // stream, then the buffers are released, then `cs` destroys the stream.  The caller's arrays are copied as they are, never page-locked.
    CallStream cs;
    if (hipStreamCreateWithFlags(&cs.s, hipStreamNonBlocking) != hipSuccess) { cs.s = nullptr; return fail(BFGX_ERR_HIP, "hipStreamCreate failed"); }
    hipStream_t st = cs.s;
    size_t ntot = 1;
    for (int d = 0; d < grid->ndim; ++d) ntot *= (size_t)grid->npix;
    const size_t cells = (size_t)halos_host->n * (size_t)nb, mbytes = ntot * sizeof(double);
    DevBuf dmap[3], dn[2], ds[3];
    DrainOnExit drain;
    drain.s[0] = &cs.s;
    const double *src[3] = {map_host, g1_host, g2_host};
    for (int k = 0; k < 3; ++k) {
        if (!src[k]) continue;
        if (dmap[k].alloc(mbytes)) return alloc_fail("map");
        HIP_TRY(hipMemcpyAsync(dmap[k].p, src[k], mbytes, hipMemcpyHostToDevice, st));
    }
    const size_t cb = std::max<size_t>(cells, 1) * 8;
    if (dn[0].alloc(cb) || ds[0].alloc(cb) || (g1_host && (dn[1].alloc(cb) || ds[1].alloc(cb) || ds[2].alloc(cb)))) return alloc_fail("profiles");
    const StackOut dv{dn[0].as<int64_t>(), g1_host ? dn[1].as<int64_t>() : nullptr, ds[0].as<double>(), g1_host ? ds[1].as<double>() : nullptr,
                         g1_host ? ds[2].as<double>() : nullptr};
    if (int rc = grid_profiles_run(st, halos_host, model, grid, dmap[0].as<double>(), g1_host ? dmap[1].as<double>() : nullptr,
                                   g1_host ? dmap[2].as<double>() : nullptr, nb, r_edges, scaled, dv))
        return rc;
    if (int rc = profiles_copy_back(st, ho, dv, cells, g1_host != nullptr)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return BFGX_OK;
}

int bfgx_grid_profiles_device(int32_t device, void *hip_stream, const bfgx_grid_catalog *halos_host, const bfgx_model *model, const bfgx_grid *grid,
                              const double *map_dev, const double *g1_dev, const double *g2_dev, int32_t nb, const double *r_edges, int32_t scaled,
                              int64_t *npix_dev, double *sum_dev, int64_t *npix_shear_dev, double *sum_t_dev, double *sum_x_dev)
{
    const StackOut dv{npix_dev, npix_shear_dev, sum_dev, sum_t_dev, sum_x_dev};
    if (int rc = grid_profiles_validate(halos_host, model, grid, map_dev, g1_dev, g2_dev, nb, r_edges, dv)) return rc;
    HIP_TRY(hipSetDevice(device));
    return grid_profiles_run((hipStream_t)hip_stream, halos_host, model, grid, map_dev, g1_dev, g2_dev, nb, r_edges, scaled, dv);
}

}  // extern "C"
