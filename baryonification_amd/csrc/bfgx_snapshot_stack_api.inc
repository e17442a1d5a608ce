// bfgx_snapshot_stack_api.inc -- C ABI of the halo-centred profile measurement on particle snapshots (included at the end of bfgx_api.hip,
// after bfgx_pairs.hpp whose particle binning it shares; declared in include/bfgx.h).
//
// MeasureProfilesSnapshot looks at the particles where baryonification is defined: the radial profile around the halos.  The ball, its
// clipping and the separations are those of BaryonifySnapshot (snap_pairs_prep_kernel, snap_sep); as for the per-pair entries the bfgx_model
// only carries the runner's cosmology, mass definition and epsilon_max, its table must be valid and is ignored.  Both entries run
// snap_profiles_run: halo records, particle binning, one gather into cell order, snap_stack_kernel.

namespace {

struct SnapProfIn {
    int32_t ndim; double L, redshift; int64_t np;
    const double *x, *y, *z, *w;
};

// everything that can be refused without a device, before anything is allocated
int snap_profiles_validate(const bfgx_grid_catalog *c, const bfgx_model *model, const SnapProfIn &s, int32_t nb, const double *r_edges,
                           const int64_t *npart, const double *sum)
{
    if (!c || !model || !r_edges || !npart) return fail(BFGX_ERR_INVALID, "NULL argument");
    if ((s.w == nullptr) != (sum == nullptr)) return fail(BFGX_ERR_INVALID, "NULL argument: sum goes with the weights (both, or neither for counts only)");
    if (int rc = profiles_validate_bins(nb, r_edges)) return rc;
    if (c->n < 0 || s.np < 0) return fail(BFGX_ERR_INVALID, "catalog / snapshot size < 0");
    if (c->n > INT32_MAX || s.np > (int64_t)UINT32_MAX) return fail(BFGX_ERR_INVALID, "more than 2^31 halos or 2^32 particles");
    if (s.ndim != 2 && s.ndim != 3) return fail(BFGX_ERR_INVALID, "snapshot ndim must be 2 or 3");
    if (!(s.L > 0.0) || !std::isfinite(s.L) || !(s.redshift > -1.0)) return fail(BFGX_ERR_INVALID, "snapshot L must be > 0 and redshift > -1");
    if (c->n > 0 && (!c->M || !c->x || !c->y || (s.ndim == 3 && !c->z))) return fail(BFGX_ERR_INVALID, "catalog column pointer is NULL");
    if (s.np > 0 && (!s.x || !s.y || (s.ndim == 3 && !s.z))) return fail(BFGX_ERR_INVALID, "snapshot coordinate pointer is NULL");
    if (int rc = profiles_validate_placeholder(model, true)) return rc;
    if (bfgx_device_count() <= 0) return fail(BFGX_ERR_NO_DEVICE, "no HIP device visible: libbfgx has no CPU fallback");
    return BFGX_OK;
}

// The measurement on stream st: s holds DEVICE pointers to the particle columns, npart / sum are device outputs; the halo columns and the
// edges are host arrays.  The stream is drained before this returns, on every path: the workspace is released at scope exit.
int snap_profiles_run(hipStream_t st, const bfgx_grid_catalog *c, const bfgx_model *model, const SnapProfIn &s, int32_t nb, const double *r_edges,
                      int32_t scaled, int64_t *npart, double *sum)
{
    const int64_t nh = c->n, np = s.np;
    SnapGeom g;
    g.ndim = s.ndim; g.nc = snap_pairs_cells(s.ndim, np); g.L = s.L; g.inv_cell = (double)g.nc / s.L; g.a = 1.0 / (1.0 + s.redshift);
    g.ncell = 1;
    for (int d = 0; d < g.ndim; ++d) g.ncell *= g.nc;
    DevModel m;                                    // the runner's side of the geometry is all the halo preparation reads
    std::memset(&m, 0, sizeof(m));
    m.bg_runner = m.bg_model = make_background(model->cosmo_runner);
    m.md_runner = m.md_model = model->massdef_runner;
    m.eps_runner = model->eps_runner;
    DevBuf hcol[4], recs, edges, sorted[4];
    SnapBins bins;
    hipStream_t stream = st;
    DrainOnExit drain;                             // (declared last: the stream is drained before the buffers above are released)
    drain.s[0] = &stream; drain.null_stream = (st == nullptr);
    if (int rc = upload_halo_columns(st, c, s.ndim, nh, hcol)) return rc;
    if (recs.alloc(sizeof(SnapHaloRec) * (size_t)std::max<int64_t>(nh, 1)) || edges.alloc(sizeof(double) * (kStackMaxBins + 1))) return alloc_fail("halo records");
    HIP_TRY(hipMemcpyAsync(edges.p, r_edges, sizeof(double) * (size_t)(nb + 1), hipMemcpyHostToDevice, st));
    if (nh > 0) {
        hipLaunchKernelGGL(snap_pairs_prep_kernel, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, st, m, g, nh, hcol[0].as<double>(), hcol[1].as<double>(),
                           hcol[2].as<double>(), hcol[3].as<double>(), recs.as<SnapHaloRec>());
        HIP_TRY(hipGetLastError());
    }
    if (int rc = snap_bin_particles(st, g, np, s.x, s.y, s.z, bins)) return rc;
    if (nh == 0) return BFGX_OK;                   // (the particles have been checked; there is no cell to write)
    // the particle records in cell order: a run of cells is a contiguous run of records
    const size_t npb = sizeof(double) * (size_t)std::max<int64_t>(np, 1);
    if (sorted[0].alloc(npb) || sorted[1].alloc(npb) || (s.ndim == 3 && sorted[2].alloc(npb)) || (s.w && sorted[3].alloc(npb))) return alloc_fail("sorted particles");
    if (np > 0) {
        hipLaunchKernelGGL(snap_stack_gather_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, np, bins.sorted_idx, s.x, s.y,
                           s.ndim == 3 ? s.z : nullptr, s.w, sorted[0].as<double>(), sorted[1].as<double>(), sorted[2].as<double>(), sorted[3].as<double>());
        HIP_TRY(hipGetLastError());
    }
    SnapStackArgs a;
    a.x = sorted[0].as<double>(); a.y = sorted[1].as<double>(); a.z = sorted[2].as<double>(); a.w = s.w ? sorted[3].as<double>() : nullptr;
    a.cell_start = (const uint32_t *)bins.cstart.p; a.M = hcol[0].as<double>(); a.edges = edges.as<double>();
    a.nb = nb; a.scaled = scaled ? 1 : 0; a.out = StackOut{npart, nullptr, sum, nullptr, nullptr};
    const dim3 grid((unsigned)std::min<int64_t>(nh, 8192)), block(kSnapStackThreads);
    const SnapHaloRec *rp = recs.as<SnapHaloRec>();
    if (g.ndim == 3) {
        if (s.w) hipLaunchKernelGGL((snap_stack_kernel<3, true>), grid, block, 0, st, g, m.bg_runner, m.md_runner, nh, rp, a);
        else hipLaunchKernelGGL((snap_stack_kernel<3, false>), grid, block, 0, st, g, m.bg_runner, m.md_runner, nh, rp, a);
    } else {
        if (s.w) hipLaunchKernelGGL((snap_stack_kernel<2, true>), grid, block, 0, st, g, m.bg_runner, m.md_runner, nh, rp, a);
        else hipLaunchKernelGGL((snap_stack_kernel<2, false>), grid, block, 0, st, g, m.bg_runner, m.md_runner, nh, rp, a);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return BFGX_OK;
}

}  // namespace

extern "C" {

int bfgx_snapshot_profiles(const bfgx_grid_catalog *halos_host, const bfgx_model *model, const bfgx_snapshot *snap_host, const double *w_host,
                           int32_t nb, const double *r_edges, int32_t scaled, int32_t device, int64_t *npart, double *sum)
{
    if (!snap_host) return fail(BFGX_ERR_INVALID, "NULL argument");
    const SnapProfIn hs{snap_host->ndim, snap_host->L, snap_host->redshift, snap_host->n, snap_host->x, snap_host->y, snap_host->z, w_host};
    if (int rc = snap_profiles_validate(halos_host, model, hs, nb, r_edges, npart, sum)) return rc;
    HIP_TRY(hipSetDevice(device));
    // nothing is left in flight on any return path: `drain` (declared after the device buffers, so destroyed before them) drains the call's
    // stream, then the buffers are released, then `cs` destroys the stream.  The caller's arrays are copied as they are, never page-locked.
    CallStream cs;
    if (hipStreamCreateWithFlags(&cs.s, hipStreamNonBlocking) != hipSuccess) { cs.s = nullptr; return fail(BFGX_ERR_HIP, "hipStreamCreate failed"); }
    hipStream_t st = cs.s;
    const int64_t np = hs.np;
    const size_t npb = sizeof(double) * (size_t)std::max<int64_t>(np, 1), cells = (size_t)halos_host->n * (size_t)nb;
    DevBuf col[4], dn, ds;
    DrainOnExit drain;
    drain.s[0] = &cs.s;
    const double *src[4] = {hs.x, hs.y, hs.ndim == 3 ? hs.z : nullptr, w_host};
    for (int k = 0; k < 4; ++k) {
        if (!src[k]) continue;
        if (col[k].alloc(npb)) return alloc_fail("particles");
        if (np > 0) HIP_TRY(hipMemcpyAsync(col[k].p, src[k], sizeof(double) * (size_t)np, hipMemcpyHostToDevice, st));
    }
    if (dn.alloc(sizeof(int64_t) * std::max<size_t>(cells, 1)) || (w_host && ds.alloc(sizeof(double) * std::max<size_t>(cells, 1)))) return alloc_fail("profiles");
    SnapProfIn ds_in = hs;
    ds_in.x = col[0].as<double>(); ds_in.y = col[1].as<double>(); ds_in.z = col[2].as<double>(); ds_in.w = w_host ? col[3].as<double>() : nullptr;
    if (int rc = snap_profiles_run(st, halos_host, model, ds_in, nb, r_edges, scaled, dn.as<int64_t>(), w_host ? ds.as<double>() : nullptr)) return rc;
    const StackOut ho{npart, nullptr, sum, nullptr, nullptr}, dv{dn.as<int64_t>(), nullptr, ds.as<double>(), nullptr, nullptr};
    if (int rc = profiles_copy_back(st, ho, dv, cells, false)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return BFGX_OK;
}

int bfgx_snapshot_profiles_device(int32_t device, void *hip_stream, const bfgx_grid_catalog *halos_host, const bfgx_model *model, int32_t ndim,
                                  double L, double redshift, int64_t n_part, const double *x_dev, const double *y_dev, const double *z_dev,
                                  const double *w_dev, int32_t nb, const double *r_edges, int32_t scaled, int64_t *npart_dev, double *sum_dev)
{
    const SnapProfIn s{ndim, L, redshift, n_part, x_dev, y_dev, z_dev, w_dev};
    if (int rc = snap_profiles_validate(halos_host, model, s, nb, r_edges, npart_dev, sum_dev)) return rc;
    HIP_TRY(hipSetDevice(device));
    return snap_profiles_run((hipStream_t)hip_stream, halos_host, model, s, nb, r_edges, scaled, npart_dev, sum_dev);
}

}  // extern "C"
