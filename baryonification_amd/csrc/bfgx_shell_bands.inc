// bfgx_shell_bands.inc -- the banded (multi-GPU) passes: a rank owns the bands [band0, band1) of the tiling, a contiguous RING pixel range.
// Band queries, K1 / K3 / K2 restricted to a band range, the fused step of one rank, the far-deposit list.  Needs the launch ladders (bfgx_api.hip).

extern "C" {

int bfgx_plan_bands(bfgx_plan *p, int32_t *nbands, int64_t *band_first_pixel)
{
    if (!p || !nbands) return fail(BFGX_ERR_INVALID, "NULL argument");
    *nbands = p->tiling.nbands;
    if (band_first_pixel)                         // band b = rings [1 + BR b, 1 + BR (b + 1)): a contiguous RING pixel range
        for (int b = 0; b <= p->tiling.nbands; ++b) band_first_pixel[b] = band_range(p, b, b).p0;
    return BFGX_OK;
}

int bfgx_plan_band_apron(bfgx_plan *p, int32_t band0, int32_t band1, int64_t *olo, int64_t *ohi)
{
    if (!p || !olo || !ohi) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = check_band_range(p, band0, band1)) return rc;
    const int64_t i0 = 1 + (int64_t)p->tiling.BR * band0, i1 = 1 + (int64_t)p->tiling.BR * band1;      // rings [i0, i1)
    *olo = ring_first_pixel(p->hpx, i0 - p->band_reach);
    *ohi = ring_first_pixel(p->hpx, i1 + p->band_reach);
    return BFGX_OK;
}

int bfgx_plan_reach_rings(bfgx_plan *p, double max_offset, int32_t *rings)
{
    if (!p || !rings) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (!(max_offset >= 0.0)) return fail(BFGX_ERR_INVALID, "max_offset must be >= 0");
    *rings = regrid_reach_rings(p->hpx.nside, std::min(max_offset * 1.001, regrid_cap(p->hpx.nside)));
    return BFGX_OK;
}

int bfgx_plan_set_band_reach(bfgx_plan *p, int32_t rings)
{
    if (!p) return fail(BFGX_ERR_INVALID, "NULL plan");
    if (rings < 1 || rings > kReachMax) return fail(BFGX_ERR_INVALID, "band reach must be 1 .. %d rings", kReachMax);
    p->band_reach = rings;
    return BFGX_OK;
}

// reset_far = false: the far-deposit list keeps what earlier calls have listed (the one-shot host entry regrids the sphere in several
// band ranges while the map is still arriving, and applies one list at the end).  The list of far SOURCE pixels is consumed by every call
// (regrid_far_eval_kernel turns it into deposits before the call's last launch) and starts every call empty; src_zeroed: the caller's
// memset has seen to that
// m SPLIT (the fused band entry, the one-shot host entry): the low halves of the pixels [olo, ohi) follow their high halves
static int regrid_bands_impl(bfgx_plan *p, int32_t band0, int32_t band1, const double *map_in_dev, const void *offsets_dev,
                             int64_t olo, int64_t ohi, const DispMode &m, double *out_slice_dev, double *sums_dev, bool reset_far,
                             bool sums_later = false, bool src_zeroed = false)
{
    if (p->algo != 1) return fail(BFGX_ERR_UNSUPPORTED, "banded regrid needs the tiled algorithm (algo 1)");
    int64_t need_lo = 0, need_hi = 0;
    if (int rc = bfgx_plan_band_apron(p, band0, band1, &need_lo, &need_hi)) return rc;
    if (band0 == band1) {
        // a rank that owns no band (more ranks than bands): empty buffers, whose data pointers are NULL, are fine
        HIP_TRY(hipSetDevice(p->device));
        if (reset_far) HIP_TRY(hipMemsetAsync(p->far.count, 0, kFarCountersBytes, p->stream));
        if (sums_dev) HIP_TRY(hipMemsetAsync(sums_dev, 0, 2 * sizeof(double), p->stream));
        return BFGX_OK;
    }
    if (!map_in_dev || !offsets_dev || !out_slice_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (olo > need_lo || ohi < need_hi || olo < 0 || ohi > p->hpx.npix)
        return fail(BFGX_ERR_INVALID, "pix_offsets range [%lld, %lld) does not cover the bands and %d ring(s) either side [%lld, %lld)",
                    (long long)olo, (long long)ohi, p->band_reach, (long long)need_lo, (long long)need_hi);
    HIP_TRY(hipSetDevice(p->device));
    if (reset_far) HIP_TRY(hipMemsetAsync(p->far.count, 0, kFarCountersBytes, p->stream));           // both lists
    else if (!src_zeroed) HIP_TRY(hipMemsetAsync(p->far_src.count, 0, sizeof(uint32_t), p->stream));
    const BandRange r = band_range(p, band0, band1);
    {
        KernelTimer kt(p, BFGX_K_REGRID);
        const size_t lds = regrid3_lds_bytes(p->tiling.BR, p->tiling.W, m.fp64() ? sizeof(double) : sizeof(float), p->band_reach > 1,
                                             m.split() ? sizeof(float) : 0);
        // virtual bases: the kernel indexes every array by global pixel number
        double *out_base = out_slice_dev - r.p0;
        // every rank gathers with the same fixed reach (so that all of them classify a source pixel the same way)
        const ReachArgs reach = reach_args(p, regrid_cap_for_rings(p->hpx.nside, p->band_reach));
        hipLaunchKernelGGL(tile_apron_kernel, dim3((r.nt + 255) / 256), dim3(256), 0, p->stream, p->hpx, p->tiling, (const float *)nullptr,
                           p->band_reach, reach.cap, r.t0, r.nt, p->tile_apron, (int32_t *)nullptr);
        double *ts = sums_dev ? p->tile_sums : nullptr;
        const dim3 grid(r.nt), blk(256);
        int *none = nullptr;
#define BFGX_REGRID3(ACC, REAL, SPLIT, OL)                                                                                                     \
        do {                                                                                                                                    \
            const ACC *o = (const ACC *)offsets_dev - 3 * olo;                                                                                  \
            if (p->band_reach == 1) hipLaunchKernelGGL((tile_regrid3_kernel<ACC, REAL, 0, SPLIT>), grid, blk, lds, p->stream, p->hpx, p->tiling, map_in_dev, o, OL, \
                                                       out_base, p->far, p->far_src, reach, ts, r.t0, r.nt, none, (double *)nullptr);           \
            else hipLaunchKernelGGL((tile_regrid3_kernel<ACC, REAL, 2, SPLIT>), grid, blk, lds, p->stream, p->hpx, p->tiling, map_in_dev, o, OL, \
                                    out_base, p->far, p->far_src, reach, ts, r.t0, r.nt, none, (double *)nullptr);                              \
            hipLaunchKernelGGL((regrid_far_eval_kernel<ACC, SPLIT>), dim3(kFarEvalWgs), blk, 0, p->stream, p->hpx, p->tiling.rings, map_in_dev, o, OL, p->far_src, p->far); \
        } while (0)
        if (m.split()) BFGX_REGRID3(float, double, true, m.lo(offsets_dev, ohi - olo) - 3 * olo);
        else if (m.fp64()) BFGX_REGRID3(double, double, false, (const double *)nullptr);
        else BFGX_REGRID3(float, float, false, (const float *)nullptr);
#undef BFGX_REGRID3
        HIP_TRY(hipGetLastError());
    }
    if (sums_dev && !sums_later) {             // (sums_later: the caller's next kernel adds the per-tile sums up)
        KernelTimer kt(p, BFGX_K_SUM);
        if (int rc = launch_tile_sums(p, r.t0, r.nt, sums_dev)) return rc;
        HIP_TRY(hipGetLastError());
    }
    return BFGX_OK;
}

// K0 + K1 for the bands [band0, band1) (band0 < band1) into pix_offsets from the first pixel of band0 (SPLIT: the low halves follow the high ones)
static int offsets_bands(bfgx_plan *p, const bfgx_catalog *cat, int32_t band0, int32_t band1, void *slice, const DispMode &m)
{
    const BandRange r = band_range(p, band0, band1);
    TileLaunch k1;
    k1.tile_lo = r.t0; k1.tile_n = r.nt;
    if (int rc = launch_k0(p, cat, 1, m.fp64())) return rc;
    // K1's flush leaves the largest |offset|^2 of every tile it stores (bfgx_bands_max_offset2_device reduces them: the reach of the
    // regrid then needs no second pass over the slice)
    k1.omax = p->arena.omax;
    return launch_offsets(p, m, slice, r.p0, r.p1, k1);
}

int bfgx_regrid_bands_device(bfgx_plan *p, int32_t band0, int32_t band1, const double *map_in_dev, const void *offsets_dev,
                             int64_t olo, int64_t ohi, int acc_f64, double *out_slice_dev, double *sums_dev)
{
    DispMode m;
    if (int rc = disp_mode(p, acc_f64, true, m)) return rc;
    return regrid_bands_impl(p, band0, band1, map_in_dev, offsets_dev, olo, ohi, m, out_slice_dev, sums_dev, true);
}

int bfgx_offsets_bands_device(bfgx_plan *p, const bfgx_catalog *cat, int32_t band0, int32_t band1, void *offsets_slice_dev, int acc_f64)
{
    if (int rc = check_scatter(p, cat, offsets_slice_dev, false, true, band0, band1)) return rc;
    if (band0 == band1) return BFGX_OK;
    DispMode m;
    if (int rc = disp_mode(p, acc_f64, true, m)) return rc;
    return offsets_bands(p, cat, band0, band1, offsets_slice_dev, m);
}

int bfgx_paint_bands_device(bfgx_plan *p, const bfgx_catalog *cat, int32_t band0, int32_t band1, void *map_slice_dev, int acc_f64)
{
    if (int rc = check_scatter(p, cat, map_slice_dev, true, true, band0, band1)) return rc;
    if (band0 == band1) return BFGX_OK;
    PaintMode m;
    if (int rc = paint_mode(p, acc_f64, m)) return rc;
    const BandRange r = band_range(p, band0, band1);
    TileLaunch k3;
    k3.tile_lo = r.t0; k3.tile_n = r.nt;
    if (int rc = launch_k0(p, cat, 0, m.k0_f64())) return rc;
    return launch_paint(p, m, map_slice_dev, r.p0, k3);
}

// One rank's share of a resident multi-GPU BaryonifyShell step after the routing, as ONE enqueue-only call (Parallelize.py:250-318 has one call
// drive all workers): K0 + binning + K1 for the bands [B0, B1) (the rank's own and, with a route margin, the band either side: the aprons of
// its regrid) into offsets_dev (pixels from the first of band B0), the banded regrid of ITS bands [b0, b1) into out_slice_dev, the listed far
// deposits that fall into its pixels added, the others counted into *foreign_dev, the two sums of the mass check.  One memset (the binning's)
// zeroes every control word; nine launches.
int bfgx_offsets_regrid_bands_device(bfgx_plan *p, const bfgx_catalog *cat, int32_t B0, int32_t B1, void *offsets_dev, int acc_f64,
                                     int32_t b0, int32_t b1, const double *map_in_dev, double *out_slice_dev, double *sums_dev,
                                     unsigned long long *foreign_dev)
{
    if (!p || !cat) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (B0 < 0 || B1 > p->tiling.nbands || B0 > b0 || b1 > B1 || b0 > b1) return fail(BFGX_ERR_INVALID, "band ranges must nest: [B0, B1) around [b0, b1)");
    // the parity-grade mode: both halves of pix_offsets stay on this device (24 bytes per pixel, as fp64 would take)
    DispMode m;
    if (int rc = disp_mode(p, acc_f64, false, m)) return rc;
    const BandRange w = band_range(p, B0, B1), r = band_range(p, b0, b1);      // what K1 writes, what this rank owns
    if (int rc = check_scatter(p, cat, offsets_dev, false, true, B0, B1)) return rc;
    if (B0 < B1) if (int rc = offsets_bands(p, cat, B0, B1, offsets_dev, m)) return rc;      // (its memset also zeroes the far list's counter)
    if (b0 == b1) {
        if (sums_dev) HIP_TRY(hipMemsetAsync(sums_dev, 0, 2 * sizeof(double), p->stream));
        return BFGX_OK;
    }
    if (int rc = regrid_bands_impl(p, b0, b1, map_in_dev, offsets_dev, w.p0, w.p1, m, out_slice_dev, sums_dev, false, true, B0 < B1)) return rc;
    hipLaunchKernelGGL(regrid_far_local_kernel, dim3(64), dim3(256), 0, p->stream, p->far, out_slice_dev, r.p0, r.p1, foreign_dev, r.nt,
                       sums_dev ? (const double *)(p->tile_sums + 2 * (size_t)r.t0) : (const double *)nullptr, sums_dev, (const double *)p->far_src.sums);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

int bfgx_bands_max_offset2_device(bfgx_plan *p, int32_t band0, int32_t band1, float *out_dev)
{
    if (!p || !out_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = check_band_range(p, band0, band1, true)) return rc;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemsetAsync(out_dev, 0, sizeof(float), p->stream));
    const BandRange r = band_range(p, band0, band1);
    if (r.nt > 0) {
        hipLaunchKernelGGL(max_bits_kernel, dim3(1), dim3(1024), 0, p->stream, r.nt, (const unsigned *)p->arena.omax + r.t0, (unsigned *)out_dev);
        HIP_TRY(hipGetLastError());
    }
    return BFGX_OK;
}

int bfgx_plan_far_apply_device(bfgx_plan *p, double *out_slice_dev, int64_t p0, int64_t p1, unsigned long long *foreign_dev)
{
    if (!p || !out_slice_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(p->device));
    hipLaunchKernelGGL(regrid_far_local_kernel, dim3(64), dim3(256), 0, p->stream, p->far, out_slice_dev, p0, p1, foreign_dev);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

int bfgx_plan_far_fetch(bfgx_plan *p, int64_t cap, int64_t *pix_host, double *val_host, int64_t *n_host)
{
    if (!p || !n_host) return fail(BFGX_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(p->device));
    unsigned long long n = 0;
    HIP_TRY(hipMemcpyAsync(&n, p->far.count, sizeof(n), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if ((int64_t)n > p->far.cap) return fail(BFGX_ERR_INVALID, "the regrid's list of far deposits overflowed (%lld entries)", (long long)p->far.cap);
    *n_host = (int64_t)n;
    if (n == 0 || (!pix_host && !val_host)) return BFGX_OK;          // count only
    if ((int64_t)n > cap || !pix_host || !val_host) return fail(BFGX_ERR_INVALID, "far-deposit buffers hold %lld entries, %lld are listed", (long long)cap, (long long)n);
    HIP_TRY(hipMemcpyAsync(pix_host, p->far.pix, sizeof(int64_t) * n, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipMemcpyAsync(val_host, p->far.val, sizeof(double) * n, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return BFGX_OK;
}

int bfgx_plan_regrid_stats(bfgx_plan *p, int64_t *far_listed, int32_t *far_overflowed, int32_t *tiles_walked, int32_t *max_reach_rings)
{
    if (!p) return fail(BFGX_ERR_INVALID, "NULL plan");
    if (p->algo != 1) return fail(BFGX_ERR_UNSUPPORTED, "regrid statistics exist for the tiled algorithm (algo 1) only");
    HIP_TRY(hipSetDevice(p->device));
    RegridCtrl ctrl = {};
    HIP_TRY(hipMemcpyAsync(&ctrl, p->arena.ctrl, sizeof(ctrl), hipMemcpyDeviceToHost, p->stream));
    std::vector<int32_t> apron;
    if (max_reach_rings) {
        apron.resize(2 * (size_t)p->tiling.ntiles);
        HIP_TRY(hipMemcpyAsync(apron.data(), p->tile_apron, sizeof(int32_t) * apron.size(), hipMemcpyDeviceToHost, p->stream));
    }
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (far_listed) *far_listed = (int64_t)ctrl.far_count;
    if (far_overflowed) *far_overflowed = ctrl.far_overflow_full;
    if (tiles_walked) *tiles_walked = ctrl.todo_count;
    if (max_reach_rings) {
        int32_t m = 0;
        for (int t = 0; t < p->tiling.ntiles; ++t) m = std::max(m, apron[2 * (size_t)t]);
        *max_reach_rings = m;
    }
    return BFGX_OK;
}

}  // extern "C"
