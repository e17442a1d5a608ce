// bfgx_snapshot_pairs_api.inc -- C ABI of BaryonifySnapshot for models that are Python callables (included at the end of bfgx_api.hip,
// after bfgx_callable_api.inc whose bfgx_pairs handle it shares; declared in include/bfgx.h).
//
// The reference calls model.displacement(d, M_j, a_j) once per halo on the distances of the particles within R_q of it
// (SnapshotRunner.py:217-245).  begin finds every halo's particles (ascending index within a halo), radii hands out the distances of a range
// of halos, apply accumulates the caller's values of that range as per-particle offsets, finish adds them, re-wraps once and writes x / y / z.
#include <hipcub/hipcub.hpp>

namespace {

int snap_pairs_range(const bfgx_pairs *h, int64_t j0, int64_t j1)
{
    if (!h || h->sdev < 0) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (j0 < 0 || j1 < j0 || j1 > h->n) return fail(BFGX_ERR_INVALID, "halo range [%lld, %lld) outside [0, %lld)", (long long)j0, (long long)j1, (long long)h->n);
    return BFGX_OK;
}

// cells per side of the particle binning: a few particles per cell on average
int snap_pairs_cells(int ndim, int64_t np)
{
    const double per = std::max<double>(1.0, (double)np / 4.0);
    const int nc = (int)(ndim == 3 ? std::cbrt(per) : std::sqrt(per));
    return std::max(1, std::min(nc, ndim == 3 ? 512 : 8192));
}

// The particles of a snapshot binned into the periodic cell grid of g: per-cell counts -> exclusive scan (start[c] .. start[c + 1] are
// cell c's slots) -> stable radix sort of (cell, index), so that a cell lists its particles in ascending index.  Everything is enqueued on
// st; the stream is synchronised once, for the [0, L] check.  x / y / z are device pointers.  No particles: every start is 0.
struct SnapBins {
    DevBuf cell[2], idx[2], ccount, cstart, flags, tmp;
    const uint32_t *sorted_idx = nullptr;         // particle index per slot
    const int32_t *start() const { return (const int32_t *)cstart.p; }
};

int snap_bin_particles(hipStream_t st, const SnapGeom &g, int64_t np, const double *x, const double *y, const double *z, SnapBins &b)
{
    const size_t npb = (size_t)std::max<int64_t>(np, 1);
    if (b.cell[0].alloc(4 * npb) || b.cell[1].alloc(4 * npb) || b.idx[0].alloc(4 * npb) || b.idx[1].alloc(4 * npb) ||
        b.ccount.alloc(sizeof(int32_t) * ((size_t)g.ncell + 1)) || b.cstart.alloc(sizeof(int32_t) * ((size_t)g.ncell + 1)) || b.flags.alloc(sizeof(int32_t)))
        return alloc_fail("particle bins");
    HIP_TRY(hipMemsetAsync(b.ccount.p, 0, sizeof(int32_t) * ((size_t)g.ncell + 1), st));
    HIP_TRY(hipMemsetAsync(b.flags.p, 0, sizeof(int32_t), st));
    b.sorted_idx = (const uint32_t *)b.idx[0].p;
    if (np == 0) {
        HIP_TRY(hipMemsetAsync(b.cstart.p, 0, sizeof(int32_t) * ((size_t)g.ncell + 1), st));
        return BFGX_OK;
    }
    int32_t hflags = 0;
    hipLaunchKernelGGL(snap_pairs_bin_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, g, np, x, y, z, (uint32_t *)b.cell[0].p,
                       (uint32_t *)b.idx[0].p, (int32_t *)b.ccount.p, (int32_t *)b.flags.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&hflags, b.flags.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (hflags & 2) return fail(BFGX_ERR_INVALID, "particle coordinates must lie in [0, L] (scipy's periodic KDTree refuses such data too)");
    size_t b1 = 0, b2 = 0;
    hipcub::DoubleBuffer<uint32_t> kb((uint32_t *)b.cell[0].p, (uint32_t *)b.cell[1].p), vb((uint32_t *)b.idx[0].p, (uint32_t *)b.idx[1].p);
    int end_bit = 1;
    while (end_bit < 32 && ((uint64_t)1 << end_bit) < (uint64_t)g.ncell) ++end_bit;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, b1, kb, vb, (int64_t)np, 0, end_bit, st));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, b2, (const int32_t *)b.ccount.p, (int32_t *)b.cstart.p, (int)g.ncell + 1, st));
    if (b.tmp.alloc(std::max(b1, b2))) return alloc_fail("sort workspace");
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(b.tmp.p, b1, kb, vb, (int64_t)np, 0, end_bit, st));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(b.tmp.p, b2, (const int32_t *)b.ccount.p, (int32_t *)b.cstart.p, (int)g.ncell + 1, st));
    b.sorted_idx = vb.Current();
    return BFGX_OK;
}

template <int MODE>
int launch_snap_pairs(bfgx_pairs *h, int64_t j0, int64_t j1, const double *vals, double *out)
{
    const int64_t p0 = h->off_h[(size_t)j0], p1 = h->off_h[(size_t)j1];
    if (p1 == p0) return BFGX_OK;
    const unsigned blocks = (unsigned)std::min<int64_t>((p1 - p0 + 255) / 256, 65536);
    const double *x = (const double *)h->sxyz[0].p, *y = (const double *)h->sxyz[1].p, *z = (const double *)h->sxyz[2].p;
    if (h->sg.ndim == 3)
        hipLaunchKernelGGL((snap_pairs_kernel<3, MODE>), dim3(blocks), dim3(256), 0, h->sstream, h->sg, (const SnapHaloRec *)h->srecs.p, x, y, z,
                           (const uint64_t *)h->skeys.p, p0, p1, vals, out);
    else
        hipLaunchKernelGGL((snap_pairs_kernel<2, MODE>), dim3(blocks), dim3(256), 0, h->sstream, h->sg, (const SnapHaloRec *)h->srecs.p, x, y, z,
                           (const uint64_t *)h->skeys.p, p0, p1, vals, out);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

}  // namespace

extern "C" {

void bfgx_snapshot_pairs_end(bfgx_pairs *h) { bfgx_shell_pairs_end(h); }

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
    bfgx_pairs *h = new bfgx_pairs();
    auto bail = [&](int rc) { bfgx_snapshot_pairs_end(h); return rc; };
    h->sdev = device;
    if (hipStreamCreateWithFlags(&h->sstream, hipStreamNonBlocking) != hipSuccess) { h->sstream = nullptr; return bail(fail(BFGX_ERR_HIP, "hipStreamCreate failed")); }
    hipStream_t st = h->sstream;
    int NC = 4;
    if (int rc = upload_model(h->smem, st, model, false, h->smodel, NC)) return bail(rc);
    const int64_t nh = c->n, np = s->n;
    h->n = nh; h->snp = np;
    SnapGeom &g = h->sg;
    g.ndim = s->ndim; g.nc = snap_pairs_cells(s->ndim, np); g.L = s->L; g.inv_cell = (double)g.nc / s->L; g.a = 1.0 / (1.0 + s->redshift);
    g.ncell = 1;
    for (int d = 0; d < g.ndim; ++d) g.ncell *= g.nc;
    // uploads: halo columns (float32-valued, as HaloNDCatalog keeps them), particle coordinates
    DevBuf hcol[4];
    if (int rc = upload_halo_columns(st, c, s->ndim, nh, hcol)) return bail(rc);
    const double *psrc[3] = {s->x, s->y, s->ndim == 3 ? s->z : nullptr};
    for (int k = 0; k < 3; ++k) {
        if (h->sxyz[k].alloc(sizeof(double) * (size_t)std::max<int64_t>(np, 1))) return bail(alloc_fail("particles"));
        if (np > 0 && psrc[k] && hipMemcpyAsync(h->sxyz[k].p, psrc[k], sizeof(double) * (size_t)np, hipMemcpyHostToDevice, st) != hipSuccess)
            return bail(fail(BFGX_ERR_HIP, "copy(particles) failed"));
    }
    if (h->srecs.alloc(sizeof(SnapHaloRec) * (size_t)std::max<int64_t>(nh, 1)) || h->counts.alloc(sizeof(int64_t) * (size_t)std::max<int64_t>(nh, 1)) ||
        h->off.alloc(sizeof(int64_t) * ((size_t)nh + 1)) || h->sacc.alloc(3 * sizeof(double) * (size_t)std::max<int64_t>(np, 1)))
        return bail(alloc_fail("halo records"));
    HIP_TRY(hipMemsetAsync(h->sacc.p, 0, 3 * sizeof(double) * (size_t)std::max<int64_t>(np, 1), st));
    if (nh > 0) {
        hipLaunchKernelGGL(snap_pairs_prep_kernel, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, st, h->smodel, g, nh, (const double *)hcol[0].p,
                           (const double *)hcol[1].p, (const double *)hcol[2].p, (const double *)hcol[3].p, (SnapHaloRec *)h->srecs.p);
        HIP_TRY(hipGetLastError());
    }
    SnapBins bins;
    if (int rc = snap_bin_particles(st, g, np, (const double *)h->sxyz[0].p, (const double *)h->sxyz[1].p, (const double *)h->sxyz[2].p, bins)) return bail(rc);
    const DevBuf &cstart = bins.cstart;
    const uint32_t *sorted_idx = bins.sorted_idx;
    const unsigned wblocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(nh, 8192));
    const double *px = (const double *)h->sxyz[0].p, *py = (const double *)h->sxyz[1].p, *pz = (const double *)h->sxyz[2].p;
    if (nh > 0) {
        if (np > 0) {
            if (g.ndim == 3)
                hipLaunchKernelGGL((snap_pairs_walk_kernel<3, 0>), dim3(wblocks), dim3(256), 0, st, g, nh, (const SnapHaloRec *)h->srecs.p, px, py, pz,
                                   (const int32_t *)cstart.p, sorted_idx, (int64_t *)h->counts.p, (const int64_t *)nullptr, (int64_t *)nullptr, (uint64_t *)nullptr);
            else
                hipLaunchKernelGGL((snap_pairs_walk_kernel<2, 0>), dim3(wblocks), dim3(256), 0, st, g, nh, (const SnapHaloRec *)h->srecs.p, px, py, pz,
                                   (const int32_t *)cstart.p, sorted_idx, (int64_t *)h->counts.p, (const int64_t *)nullptr, (int64_t *)nullptr, (uint64_t *)nullptr);
            HIP_TRY(hipGetLastError());
        } else {
            HIP_TRY(hipMemsetAsync(h->counts.p, 0, sizeof(int64_t) * (size_t)nh, st));
        }
        HIP_TRY(hipMemcpyAsync(counts_host, h->counts.p, sizeof(int64_t) * (size_t)nh, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    h->off_h.assign((size_t)nh + 1, 0);
    for (int64_t j = 0; j < nh; ++j) {
        if (counts_host[j] < 0) return bail(fail(BFGX_ERR_HIP, "negative pair count"));
        h->off_h[(size_t)j + 1] = h->off_h[(size_t)j] + counts_host[j];
    }
    h->total = h->off_h[(size_t)nh];
    const size_t nt = (size_t)std::max<int64_t>(h->total, 1);
    DevBuf cursor, keys2;
    if (h->skeys.alloc(sizeof(uint64_t) * nt) || keys2.alloc(sizeof(uint64_t) * nt) || cursor.alloc(sizeof(int64_t) * (size_t)std::max<int64_t>(nh, 1)))
        return bail(alloc_fail("pair keys"));
    HIP_TRY(hipMemcpyAsync(h->off.p, h->off_h.data(), sizeof(int64_t) * ((size_t)nh + 1), hipMemcpyHostToDevice, st));
    if (h->total > 0) {
        HIP_TRY(hipMemsetAsync(cursor.p, 0, sizeof(int64_t) * (size_t)nh, st));
        if (g.ndim == 3)
            hipLaunchKernelGGL((snap_pairs_walk_kernel<3, 1>), dim3(wblocks), dim3(256), 0, st, g, nh, (const SnapHaloRec *)h->srecs.p, px, py, pz,
                               (const int32_t *)cstart.p, sorted_idx, (int64_t *)nullptr, (const int64_t *)h->off.p, (int64_t *)cursor.p, (uint64_t *)h->skeys.p);
        else
            hipLaunchKernelGGL((snap_pairs_walk_kernel<2, 1>), dim3(wblocks), dim3(256), 0, st, g, nh, (const SnapHaloRec *)h->srecs.p, px, py, pz,
                               (const int32_t *)cstart.p, sorted_idx, (int64_t *)nullptr, (const int64_t *)h->off.p, (int64_t *)cursor.p, (uint64_t *)h->skeys.p);
        HIP_TRY(hipGetLastError());
        // halo-major, particle index within a halo: the fill's atomic slots carry no order
        if (h->total > INT32_MAX) return bail(fail(BFGX_ERR_INVALID, "more than 2^31 (halo, particle) pairs: catalog too large for one call"));
        size_t b3 = 0;
        hipcub::DoubleBuffer<uint64_t> pk((uint64_t *)h->skeys.p, (uint64_t *)keys2.p);
        HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, b3, pk, (int)h->total, 0, 64, st));
        DevBuf tmp2;
        if (tmp2.alloc(b3)) return bail(alloc_fail("sort workspace"));
        HIP_TRY(hipcub::DeviceRadixSort::SortKeys(tmp2.p, b3, pk, (int)h->total, 0, 64, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (pk.Current() != (uint64_t *)h->skeys.p) std::swap(h->skeys.p, keys2.p);
    }
    HIP_TRY(hipStreamSynchronize(st));           // (the locals above are freed on return)
    *out = h;
    return BFGX_OK;
}

int bfgx_snapshot_pairs_radii(bfgx_pairs *h, int64_t j0, int64_t j1, double *r_host)
{
    if (int rc = snap_pairs_range(h, j0, j1)) return rc;
    const int64_t np = h->off_h[(size_t)j1] - h->off_h[(size_t)j0];
    if (np > 0 && !r_host) return fail(BFGX_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(h->sdev));
    if (np > 0) {
        if (h->batch.need(sizeof(double) * (size_t)np)) return alloc_fail("pair batch");
        if (int rc = launch_snap_pairs<0>(h, j0, j1, nullptr, (double *)h->batch.p)) return rc;
        HIP_TRY(hipMemcpyAsync(r_host, h->batch.p, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, h->sstream));
    }
    HIP_TRY(hipStreamSynchronize(h->sstream));
    return BFGX_OK;
}

int bfgx_snapshot_pairs_apply(bfgx_pairs *h, int64_t j0, int64_t j1, const double *vals_host)
{
    if (int rc = snap_pairs_range(h, j0, j1)) return rc;
    const int64_t np = h->off_h[(size_t)j1] - h->off_h[(size_t)j0];
    if (np > 0 && !vals_host) return fail(BFGX_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(h->sdev));
    if (np > 0) {
        if (h->batch.need(sizeof(double) * (size_t)np)) return alloc_fail("pair batch");
        HIP_TRY(hipMemcpyAsync(h->batch.p, vals_host, sizeof(double) * (size_t)np, hipMemcpyHostToDevice, h->sstream));
        if (int rc = launch_snap_pairs<1>(h, j0, j1, (const double *)h->batch.p, (double *)h->sacc.p)) return rc;
    }
    HIP_TRY(hipStreamSynchronize(h->sstream));    // (vals_host is the caller's again on return)
    return BFGX_OK;
}

int bfgx_snapshot_pairs_finish(bfgx_pairs *h, double *x_out, double *y_out, double *z_out, bfgx_stats *stats)
{
    if (!h || h->sdev < 0 || (h->snp > 0 && (!x_out || !y_out || (h->sg.ndim == 3 && !z_out)))) return fail(BFGX_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(h->sdev));
    const int64_t np = h->snp;
    hipStream_t st = h->sstream;
    if (np > 0) {
        DevBuf o[3];
        for (int k = 0; k < h->sg.ndim; ++k)
            if (o[k].alloc(sizeof(double) * (size_t)np)) return alloc_fail("positions");
        hipLaunchKernelGGL(snap_pairs_finish_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, h->sg, np, (const double *)h->sacc.p,
                           (const double *)h->sxyz[0].p, (const double *)h->sxyz[1].p, (const double *)h->sxyz[2].p, (double *)o[0].p, (double *)o[1].p,
                           (double *)o[2].p);
        HIP_TRY(hipGetLastError());
        double *dst[3] = {x_out, y_out, z_out};
        for (int k = 0; k < h->sg.ndim; ++k) HIP_TRY(hipMemcpyAsync(dst[k], o[k].p, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    fill_stats(stats, nullptr, h->total, 0, 0, 0);
    return BFGX_OK;
}

}  // extern "C"
