// bfgx_snapshot_pairs_api.inc -- C ABI of BaryonifySnapshot for models that are Python callables (included at the end of bfgx_api.hip,
// after bfgx_pairs.hpp: the handle is a SnapPairs, and the particle binning lives there; declared in include/bfgx.h).
//
// The reference calls model.displacement(d, M_j, a_j) once per halo on the distances of the particles within R_q of it
// (SnapshotRunner.py:217-245).  begin finds every halo's particles (ascending index within a halo), radii hands out the distances of a range
// of halos, apply accumulates the caller's values of that range as per-particle offsets, finish adds them, re-wraps once and writes x / y / z.

namespace {

template <int MODE>
int launch_snap_pairs(SnapPairs *h, int64_t j0, int64_t j1, const double *vals, double *out)
{
    const int64_t p0 = h->off_h[(size_t)j0], p1 = h->off_h[(size_t)j1];
    if (p1 == p0) return BFGX_OK;
    const unsigned blocks = (unsigned)std::min<int64_t>((p1 - p0 + 255) / 256, 65536);
    const double *x = (const double *)h->xyz[0].p, *y = (const double *)h->xyz[1].p, *z = (const double *)h->xyz[2].p;
    if (h->g.ndim == 3)
        hipLaunchKernelGGL((snap_pairs_kernel<3, MODE>), dim3(blocks), dim3(256), 0, h->stream, h->g, (const SnapHaloRec *)h->recs.p, x, y, z,
                           (const uint64_t *)h->keys.p, p0, p1, vals, out);
    else
        hipLaunchKernelGGL((snap_pairs_kernel<2, MODE>), dim3(blocks), dim3(256), 0, h->stream, h->g, (const SnapHaloRec *)h->recs.p, x, y, z,
                           (const uint64_t *)h->keys.p, p0, p1, vals, out);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

}  // namespace

extern "C" {

void bfgx_snapshot_pairs_end(bfgx_pairs *h) { pairs_end(h); }

int bfgx_snapshot_pairs_begin(const bfgx_grid_catalog *halos_host, const bfgx_model *model, const bfgx_snapshot *snap_host, int32_t device,
                              bfgx_pairs **out, int64_t *counts_host)
{
    if (!halos_host || !model || !snap_host || !out || (halos_host->n > 0 && !counts_host)) return fail(BFGX_ERR_INVALID, "NULL argument");
    *out = nullptr;
    const bfgx_grid_catalog *c = halos_host;
    const bfgx_snapshot *s = snap_host;
    if (c->n < 0 || s->n < 0) return fail(BFGX_ERR_INVALID, "catalog / snapshot size < 0");
    if (c->n > INT32_MAX || s->n > (int64_t)UINT32_MAX) return fail(BFGX_ERR_INVALID, "more than 2^31 halos or 2^32 particles");
    if (s->ndim != 2 && s->ndim != 3) return fail(BFGX_ERR_INVALID, "snapshot ndim must be 2 or 3");
    if (!(s->L > 0.0) || !std::isfinite(s->L) || !(s->redshift > -1.0)) return fail(BFGX_ERR_INVALID, "snapshot L must be > 0 and redshift > -1");
    if (c->n > 0 && (!c->M || !c->x || !c->y || (s->ndim == 3 && !c->z))) return fail(BFGX_ERR_INVALID, "catalog column pointer is NULL");
    if (s->n > 0 && (!s->x || !s->y || (s->ndim == 3 && !s->z))) return fail(BFGX_ERR_INVALID, "snapshot coordinate pointer is NULL");
    if (model->table.ndim != 3) return fail(BFGX_ERR_INVALID, "the per-pair entries take a model with a (dummy) 3-axis table: halo properties are the callable's business");
    if (int rc = validate_model(model)) return rc;
    if (bfgx_device_count() <= 0) return fail(BFGX_ERR_NO_DEVICE, "no HIP device visible: libbfgx has no CPU fallback");
    HIP_TRY(hipSetDevice(device));
    // the workspace of this call alone: declared before the handle, so that on every return it is released after the handle's stream has drained
    DevBuf hcol[4], cursor, keys2, tmp2;
    SnapBins bins;
    PairsOwner<SnapPairs> h(new SnapPairs());
    HIP_TRY(hipStreamCreateWithFlags(&h->own.s, hipStreamNonBlocking));
    h->on(device, h->own.s);
    hipStream_t st = h->stream;
    int NC = 4;
    if (int rc = upload_model(h->mem, st, model, false, h->model, NC)) return rc;
    const int64_t nh = c->n, np = s->n;
    h->n = nh; h->np = np;
    SnapGeom &g = h->g;
    g.ndim = s->ndim; g.nc = snap_pairs_cells(s->ndim, np); g.L = s->L; g.inv_cell = (double)g.nc / s->L; g.a = 1.0 / (1.0 + s->redshift);
    g.ncell = 1;
    for (int d = 0; d < g.ndim; ++d) g.ncell *= g.nc;
    // uploads: halo columns (float32-valued, as HaloNDCatalog keeps them), particle coordinates
    if (int rc = upload_halo_columns(st, c, s->ndim, nh, hcol)) return rc;
    const double *psrc[3] = {s->x, s->y, s->ndim == 3 ? s->z : nullptr};
    for (int k = 0; k < 3; ++k) {
        if (h->xyz[k].alloc(sizeof(double) * (size_t)std::max<int64_t>(np, 1))) return alloc_fail("particles");
        if (np > 0 && psrc[k]) HIP_TRY(hipMemcpyAsync(h->xyz[k].p, psrc[k], sizeof(double) * (size_t)np, hipMemcpyHostToDevice, st));
    }
    if (h->recs.alloc(sizeof(SnapHaloRec) * (size_t)std::max<int64_t>(nh, 1)) || h->counts.alloc(sizeof(int64_t) * (size_t)std::max<int64_t>(nh, 1)) ||
        h->off.alloc(sizeof(int64_t) * ((size_t)nh + 1)) || h->acc.alloc(3 * sizeof(double) * (size_t)std::max<int64_t>(np, 1)))
        return alloc_fail("halo records");
    HIP_TRY(hipMemsetAsync(h->acc.p, 0, 3 * sizeof(double) * (size_t)std::max<int64_t>(np, 1), st));
    if (nh > 0) {
        hipLaunchKernelGGL(snap_pairs_prep_kernel, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, st, h->model, g, nh, (const double *)hcol[0].p,
                           (const double *)hcol[1].p, (const double *)hcol[2].p, (const double *)hcol[3].p, (SnapHaloRec *)h->recs.p);
        HIP_TRY(hipGetLastError());
    }
    const double *px = (const double *)h->xyz[0].p, *py = (const double *)h->xyz[1].p, *pz = (const double *)h->xyz[2].p;
    if (int rc = snap_bin_particles(st, g, np, px, py, pz, bins)) return rc;
    const DevBuf &cstart = bins.cstart;
    const uint32_t *sorted_idx = bins.sorted_idx;
    const unsigned wblocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(nh, 8192));
    if (nh > 0) {
        if (np > 0) {
            if (g.ndim == 3)
                hipLaunchKernelGGL((snap_pairs_walk_kernel<3, 0>), dim3(wblocks), dim3(256), 0, st, g, nh, (const SnapHaloRec *)h->recs.p, px, py, pz,
                                   (const int32_t *)cstart.p, sorted_idx, (int64_t *)h->counts.p, (const int64_t *)nullptr, (int64_t *)nullptr, (uint64_t *)nullptr);
            else
                hipLaunchKernelGGL((snap_pairs_walk_kernel<2, 0>), dim3(wblocks), dim3(256), 0, st, g, nh, (const SnapHaloRec *)h->recs.p, px, py, pz,
                                   (const int32_t *)cstart.p, sorted_idx, (int64_t *)h->counts.p, (const int64_t *)nullptr, (int64_t *)nullptr, (uint64_t *)nullptr);
            HIP_TRY(hipGetLastError());
        } else {
            HIP_TRY(hipMemsetAsync(h->counts.p, 0, sizeof(int64_t) * (size_t)nh, st));
        }
        HIP_TRY(hipMemcpyAsync(counts_host, h->counts.p, sizeof(int64_t) * (size_t)nh, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (int rc = pairs_offsets(h.get(), counts_host)) return rc;
    const size_t nt = (size_t)std::max<int64_t>(h->total, 1);
    if (h->keys.alloc(sizeof(uint64_t) * nt) || keys2.alloc(sizeof(uint64_t) * nt) || cursor.alloc(sizeof(int64_t) * (size_t)std::max<int64_t>(nh, 1)))
        return alloc_fail("pair keys");
    HIP_TRY(hipMemcpyAsync(h->off.p, h->off_h.data(), sizeof(int64_t) * ((size_t)nh + 1), hipMemcpyHostToDevice, st));
    if (h->total > 0) {
        HIP_TRY(hipMemsetAsync(cursor.p, 0, sizeof(int64_t) * (size_t)nh, st));
        if (g.ndim == 3)
            hipLaunchKernelGGL((snap_pairs_walk_kernel<3, 1>), dim3(wblocks), dim3(256), 0, st, g, nh, (const SnapHaloRec *)h->recs.p, px, py, pz,
                               (const int32_t *)cstart.p, sorted_idx, (int64_t *)nullptr, (const int64_t *)h->off.p, (int64_t *)cursor.p, (uint64_t *)h->keys.p);
        else
            hipLaunchKernelGGL((snap_pairs_walk_kernel<2, 1>), dim3(wblocks), dim3(256), 0, st, g, nh, (const SnapHaloRec *)h->recs.p, px, py, pz,
                               (const int32_t *)cstart.p, sorted_idx, (int64_t *)nullptr, (const int64_t *)h->off.p, (int64_t *)cursor.p, (uint64_t *)h->keys.p);
        HIP_TRY(hipGetLastError());
        // halo-major, particle index within a halo: the fill's atomic slots carry no order
        if (h->total > INT32_MAX) return fail(BFGX_ERR_INVALID, "more than 2^31 (halo, particle) pairs: catalog too large for one call");
        size_t b3 = 0;
        hipcub::DoubleBuffer<uint64_t> pk((uint64_t *)h->keys.p, (uint64_t *)keys2.p);
        HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, b3, pk, (int)h->total, 0, 64, st));
        if (tmp2.alloc(b3)) return alloc_fail("sort workspace");
        HIP_TRY(hipcub::DeviceRadixSort::SortKeys(tmp2.p, b3, pk, (int)h->total, 0, 64, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (pk.Current() != (uint64_t *)h->keys.p) std::swap(h->keys.p, keys2.p);
    }
    HIP_TRY(hipStreamSynchronize(st));
    *out = h.release();
    return BFGX_OK;
}

int bfgx_snapshot_pairs_radii(bfgx_pairs *handle, int64_t j0, int64_t j1, double *r_host)
{
    SnapPairs *h = pairs_as<SnapPairs>(handle);
    int64_t np = 0;
    if (int rc = pairs_range(h, j0, j1, &np)) return rc;
    return pairs_to_host(h, h->batch, np, r_host, [&](double *r) { return launch_snap_pairs<0>(h, j0, j1, nullptr, r); });
}

int bfgx_snapshot_pairs_apply(bfgx_pairs *handle, int64_t j0, int64_t j1, const double *vals_host)
{
    SnapPairs *h = pairs_as<SnapPairs>(handle);
    int64_t np = 0;
    if (int rc = pairs_range(h, j0, j1, &np)) return rc;
    return pairs_from_host(h, h->batch, np, vals_host, [&](const double *v) { return launch_snap_pairs<1>(h, j0, j1, v, (double *)h->acc.p); });
}

int bfgx_snapshot_pairs_finish(bfgx_pairs *handle, double *x_out, double *y_out, double *z_out, bfgx_stats *stats)
{
    SnapPairs *h = pairs_as<SnapPairs>(handle);
    if (!h) return pairs_refuse<SnapPairs>();
    if (h->np > 0 && (!x_out || !y_out || (h->g.ndim == 3 && !z_out))) return fail(BFGX_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    const int64_t np = h->np;
    hipStream_t st = h->stream;
    if (np > 0) {
        DevBuf o[3];
        for (int k = 0; k < h->g.ndim; ++k)
            if (o[k].alloc(sizeof(double) * (size_t)np)) return alloc_fail("positions");
        hipLaunchKernelGGL(snap_pairs_finish_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, h->g, np, (const double *)h->acc.p,
                           (const double *)h->xyz[0].p, (const double *)h->xyz[1].p, (const double *)h->xyz[2].p, (double *)o[0].p, (double *)o[1].p,
                           (double *)o[2].p);
        HIP_TRY(hipGetLastError());
        double *dst[3] = {x_out, y_out, z_out};
        for (int k = 0; k < h->g.ndim; ++k) HIP_TRY(hipMemcpyAsync(dst[k], o[k].p, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    fill_stats(stats, nullptr, h->total, 0, 0, 0);
    return BFGX_OK;
}

}  // extern "C"
