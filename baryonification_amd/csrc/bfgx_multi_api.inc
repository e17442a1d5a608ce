// Multi-device entry points of the C ABI (include/bfgx.h, "all GPUs of a node from one call"); included by bfgx_api.hip.
//
// The MI355X counterpart of SplitJoinParallel (BaryonForge/utils/Parallelize.py:191-320) for a caller that only binds the C
// ABI: ONE host thread drives N devices.  SPATIAL sharding, as utils/Parallelize.py's default: the sphere's ring bands are dealt
// out to the devices in contiguous pixel ranges; the halo catalog is cut into N contiguous shards (Parallelize.py:250-266; the
// caller shuffles, :255) that go up over N PCIe links, every device finds the ring range of its shard's discs and packs the rows
// (48 B per halo) by destination, every device PULLS the rows bound for it with peer-to-peer copies over xGMI
// (hipMemcpyPeerAsync: N - 1 small concurrent copies per device) and runs K0 + K1 / K3 for ITS tiles only.  No accumulator
// crosses a link (the halo-sharded form moved 151 MB x (N - 1) / N per device at NSIDE 1024 whatever the halo count).  For
// BaryonifyShell the devices then agree on the reach of the gathering regrid (host max of N floats), pull that many apron rings of
// pix_offsets from their neighbours, regrid the OUTPUT pixels of their bands (disjoint slices) and copy the slice straight into
// the caller's map.  Only 1/N of the input map and of the result cross PCIe per device.  `devices` may name one device several
// times (rehearsal of the exchange on one GPU).

namespace {

// received rows [n][k] -> catalog columns [k][n]
__global__ void __launch_bounds__(256)
rows_to_cols_kernel(int64_t n, int k, const double *__restrict__ rows, double *__restrict__ cols)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n * k; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / k;
        const int c = (int)(i - r * k);
        cols[(int64_t)c * n + r] = rows[i];
    }
}

struct MultiRank {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t packed = nullptr;             // the rank's shard is packed by destination
    hipEvent_t done = nullptr;               // the rank's slice of pix_offsets / of the painted map is complete
    bfgx_plan *plan = nullptr;
    DevList mem;                             // the rank's device buffers, below
    double *cols[kCatCols] = {};
    int32_t *rings = nullptr, *counts = nullptr, *cursor = nullptr;
    double *rows = nullptr, *recv = nullptr, *rcols = nullptr, *map = nullptr, *out = nullptr, *sums = nullptr;
    char *full = nullptr;                    // pix_offsets / painted values of the rank's slice and its widest apron (fp32 or fp64)
    float *omax = nullptr;
    int64_t n0 = 0, n1 = 0;                  // halo shard
    int64_t nrecv = 0;                       // halos routed to this rank
    int32_t b0 = 0, b1 = 0;                  // bands
    int64_t p0 = 0, p1 = 0, flo = 0, fhi = 0, olo = 0, ohi = 0;     // own pixels; widest apron (buffer); apron in use
    std::vector<int64_t> start;              // first packed row per destination
    ~MultiRank()
    {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        if (plan) bfgx_plan_destroy(plan);
        mem.release();
        if (packed) (void)hipEventDestroy(packed);
        if (done) (void)hipEventDestroy(done);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

int copy_between(void *dst, int ddev, const void *src, int sdev, size_t bytes, hipStream_t stream)
{
    if (bytes == 0) return BFGX_OK;
    if (ddev == sdev) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream));
    else HIP_TRY(hipMemcpyPeerAsync(dst, ddev, src, sdev, bytes, stream));
    return BFGX_OK;
}

// band index bounds [N + 1]: contiguous runs of bands balanced by pixel count (utils/Parallelize.py band_partition)
std::vector<int32_t> partition_bands(const std::vector<int64_t> &first, int N)
{
    const int nb = (int)first.size() - 1;
    const int64_t npix = first[nb];
    std::vector<int32_t> cuts(N + 1, 0);
    for (int r = 1; r < N; ++r) {
        const double target = (double)npix * r / N;
        int best = 0;
        for (int b = 1; b <= nb; ++b) if (std::fabs((double)first[b] - target) < std::fabs((double)first[best] - target)) best = b;
        cuts[r] = std::max(best, cuts[r - 1]);
    }
    cuts[N] = nb;
    return cuts;
}

int shell_multi(bool paint, const bfgx_catalog *cat, const bfgx_model *model, int64_t nside, const double *map_in, double *map_out,
                int32_t ndev, const int32_t *devices, const bfgx_opts *opts, bfgx_stats *stats)
{
    if (!cat || !model || !map_out || (!paint && !map_in) || !devices) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (ndev < 1 || ndev > 64) return fail(BFGX_ERR_INVALID, "1 <= ndev <= 64");
    if (cat->n < 0) return fail(BFGX_ERR_INVALID, "catalog size < 0");
    const int navail = bfgx_device_count();
    if (navail <= 0) return fail(BFGX_ERR_NO_DEVICE, "no HIP device visible: libbfgx has no CPU fallback");
    for (int d = 0; d < ndev; ++d) if (devices[d] < 0 || devices[d] >= navail) return fail(BFGX_ERR_INVALID, "device %d is not visible", devices[d]);
    const bfgx_opts o = entry_opts(opts);
    if (o.algo != 1) return fail(BFGX_ERR_UNSUPPORTED, "the multi-device calls use the tiled algorithm (algo 1)");
    const int width = paint ? 1 : 3;
    const int N = ndev;
    const auto t_start = std::chrono::steady_clock::now();

    // peer access between the distinct devices (already-enabled is fine)
    for (int a = 0; a < N; ++a) for (int b = 0; b < N; ++b) if (devices[a] != devices[b]) {
        (void)hipSetDevice(devices[a]);
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, devices[a], devices[b]) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(devices[b], 0);
        (void)hipGetLastError();
    }

    std::vector<MultiRank> R(N);
    // on ANY exit (errors too) every stream is drained before the ranks free their buffers: a peer copy of another rank
    // may still be reading them (declared after R, so it runs first)
    struct DrainAll {
        std::vector<MultiRank> &r;
        ~DrainAll() { for (auto &x : r) if (x.stream) { (void)hipSetDevice(x.device); (void)hipStreamSynchronize(x.stream); } }
    } drain{R};
    const int64_t per = cat->n > 0 ? (cat->n + N - 1) / N : 0;                        // Parallelize.py:250-253
    const int nex = model->table.ndim - 3;
    std::vector<double> hostlog;
    const double *src[kCatCols];
    if (int rc = catalog_columns(cat, nex, hostlog, src)) return rc;
    // the catalog columns that travel with a halo (M, z, ra, dec, property columns, the caller's table coordinates)
    int colidx[kCatCols], ncol = 0;
    for (int i = 0; i < kCatCols; ++i) if (catalog_col_used(i, nex)) colidx[ncol++] = i;
    // ---- phase 1 (all devices concurrently): upload the shard, ring range of every disc, halos per destination
    for (int d = 0; d < N; ++d) {
        MultiRank &r = R[d];
        r.device = devices[d];
        r.n0 = std::min<int64_t>((int64_t)d * per, cat->n);
        r.n1 = std::min<int64_t>(r.n0 + per, cat->n);
        HIP_TRY(hipSetDevice(r.device));
        HIP_TRY(hipStreamCreateWithFlags(&r.stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&r.packed, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&r.done, hipEventDisableTiming));
    }
    // (a plan's workspace is sized for the halos a rank can RECEIVE; that is known after the counts, so the plans are created with
    // room for the whole catalog only when it is small, otherwise after the counting pass -- see below)
    for (int d = 0; d < N; ++d) {
        MultiRank &r = R[d];
        HIP_TRY(hipSetDevice(r.device));
        const int64_t n = r.n1 - r.n0;
        if (int rc = bfgx_plan_create(r.device, r.stream, nside, 16, model, &r.plan)) return rc;      // probe: bands, ring ranges, routing
        for (int q = 0; q < ncol; ++q) {
            const int i = colidx[q];
            HIP_TRY(r.mem.alloc(r.cols[i], (size_t)std::max<int64_t>(n, 1)));
            if (n > 0) HIP_TRY(hipMemcpyAsync(r.cols[i], src[i] + r.n0, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, r.stream));
        }
    }
    // the slices that travel between the devices are ONE array of pix_offsets, so anything wider than fp32 pair math runs as fp64 throughout
    // (as the band-restricted entries resolve it); BFGX_ACC_AUTO is settled by the probe plan, which has read the model's table
    DispMode dm;
    if (!paint) if (int rc = disp_mode(R[0].plan, o.acc_offsets_f64, true, dm)) return rc;
    const size_t esz = (paint || dm.fp64()) ? sizeof(double) : sizeof(float);
    // ---- pixel ownership: contiguous runs of ring bands
    std::vector<int64_t> first((size_t)R[0].plan->tiling.nbands + 1);
    int32_t nb = 0;
    if (int rc = bfgx_plan_bands(R[0].plan, &nb, first.data())) return rc;
    const std::vector<int32_t> cuts = partition_bands(first, N);
    std::vector<int32_t> ring_bounds(N + 1);
    for (int j = 0; j <= N; ++j) ring_bounds[j] = (int32_t)std::min<int64_t>(1 + (int64_t)R[0].plan->tiling.BR * cuts[j], 4 * nside);
    for (int d = 0; d < N; ++d) {
        MultiRank &r = R[d];
        HIP_TRY(hipSetDevice(r.device));
        const int64_t n = r.n1 - r.n0;
        bfgx_catalog dc;
        catalog_view(n, nex, r.cols, &dc);
        HIP_TRY(r.mem.alloc(r.rings, 2 * (size_t)std::max<int64_t>(n, 1)));
        HIP_TRY(r.mem.alloc(r.counts, (size_t)N));
        HIP_TRY(r.mem.alloc(r.cursor, (size_t)N));
        if (int rc = bfgx_disc_rings_device(r.plan, &dc, r.rings)) return rc;
        if (int rc = bfgx_route_count_device(r.plan, n, r.rings, N, ring_bounds.data(), r.counts)) return rc;
    }
    std::vector<std::vector<int32_t>> cnt(N, std::vector<int32_t>(N, 0));          // cnt[i][j]: halos of shard i bound for rank j
    for (int d = 0; d < N; ++d) {
        MultiRank &r = R[d];
        HIP_TRY(hipSetDevice(r.device));
        HIP_TRY(hipMemcpyAsync(cnt[d].data(), r.counts, sizeof(int32_t) * N, hipMemcpyDeviceToHost, r.stream));
    }
    for (int d = 0; d < N; ++d) { HIP_TRY(hipSetDevice(R[d].device)); HIP_TRY(hipStreamSynchronize(R[d].stream)); }
    // ---- phase 2: pack the rows by destination
    for (int d = 0; d < N; ++d) {
        MultiRank &r = R[d];
        HIP_TRY(hipSetDevice(r.device));
        r.start.assign(N + 1, 0);
        for (int j = 0; j < N; ++j) r.start[j + 1] = r.start[j] + cnt[d][j];
        HIP_TRY(r.mem.alloc(r.rows, (size_t)std::max<int64_t>(r.start[N] * ncol, 1)));
        const double *cp[kCatCols];
        for (int q = 0; q < ncol; ++q) cp[q] = r.cols[colidx[q]];
        if (int rc = bfgx_route_fill_device(r.plan, r.n1 - r.n0, r.rings, N, ring_bounds.data(), r.start.data(), ncol, cp, r.cursor, r.rows)) return rc;
        HIP_TRY(hipEventRecord(r.packed, r.stream));
    }
    // ---- phase 3: pull the rows bound for this rank over xGMI, K0 + K1 / K3 for the rank's own tiles
    for (int d = 0; d < N; ++d) {
        MultiRank &r = R[d];
        HIP_TRY(hipSetDevice(r.device));
        r.b0 = cuts[d]; r.b1 = cuts[d + 1];
        r.p0 = first[r.b0]; r.p1 = first[r.b1];
        r.nrecv = 0;
        for (int i = 0; i < N; ++i) r.nrecv += cnt[i][d];
        // the plan proper: workspace for the halos this rank received
        bfgx_plan_destroy(r.plan);
        r.plan = nullptr;
        if (int rc = bfgx_plan_create(r.device, r.stream, nside, std::max<int64_t>(r.nrecv, 1), model, &r.plan)) return rc;
        r.plan->blocking_growth = true;
        HIP_TRY(r.mem.alloc(r.recv, (size_t)std::max<int64_t>(r.nrecv * ncol, 1)));
        HIP_TRY(r.mem.alloc(r.rcols, (size_t)std::max<int64_t>(r.nrecv * ncol, 1)));
        int64_t at = 0;
        for (int i = 0; i < N; ++i) {
            HIP_TRY(hipStreamWaitEvent(r.stream, R[i].packed, 0));
            if (int rc = copy_between(r.recv + at * ncol, r.device, R[i].rows + R[i].start[d] * ncol, R[i].device,
                                      sizeof(double) * (size_t)cnt[i][d] * ncol, r.stream)) return rc;
            at += cnt[i][d];
        }
        if (r.nrecv > 0) {
            const unsigned grid = (unsigned)std::min<int64_t>((r.nrecv * ncol + 255) / 256, 4096);
            hipLaunchKernelGGL(rows_to_cols_kernel, dim3(grid), dim3(256), 0, r.stream, r.nrecv, ncol, (const double *)r.recv, r.rcols);
            HIP_TRY(hipGetLastError());
        }
        bfgx_catalog dc;
        const double *colp[kCatCols] = {};
        for (int q = 0; q < ncol; ++q) colp[colidx[q]] = r.rcols + (int64_t)q * r.nrecv;
        catalog_view(r.nrecv, nex, colp, &dc);
        // the slice is computed in place inside a buffer that also has room for the widest apron (16 rings either side)
        r.flo = r.p0; r.fhi = r.p1;
        if (!paint) {
            if (int rc = bfgx_plan_set_band_reach(r.plan, kReachMax)) return rc;
            if (int rc = bfgx_plan_band_apron(r.plan, r.b0, r.b1, &r.flo, &r.fhi)) return rc;
        }
        const int64_t nown = r.p1 - r.p0;
        HIP_TRY(r.mem.alloc(r.full, (size_t)std::max<int64_t>((r.fhi - r.flo) * width, 1) * esz));
        HIP_TRY(r.mem.alloc(r.omax, 1));
        HIP_TRY(hipMemsetAsync(r.omax, 0, sizeof(float), r.stream));
        void *slice = r.full + (size_t)(r.p0 - r.flo) * width * esz;
        if (nown > 0) {
            if (paint) { if (int rc = bfgx_paint_bands_device(r.plan, &dc, r.b0, r.b1, slice, 1)) return rc; }
            else {
                if (int rc = bfgx_offsets_bands_device(r.plan, &dc, r.b0, r.b1, slice, dm.acc())) return rc;
                if (int rc = bfgx_bands_max_offset2_device(r.plan, r.b0, r.b1, r.omax)) return rc;
            }
        }
        HIP_TRY(hipEventRecord(r.done, r.stream));
        if (paint && nown > 0) HIP_TRY(hipMemcpyAsync(map_out + r.p0, slice, sizeof(double) * (size_t)nown, hipMemcpyDeviceToHost, r.stream));
    }
    // ---- phase 4 (BaryonifyShell): the devices agree on the reach, pull the apron rings from the owners, regrid, slice -> host
    float omax2 = 0.0f;
    for (int d = 0; d < N && !paint; ++d) {
        MultiRank &r = R[d];
        HIP_TRY(hipSetDevice(r.device));
        float m2 = 0.0f;
        HIP_TRY(hipMemcpyAsync(&m2, r.omax, sizeof(float), hipMemcpyDeviceToHost, r.stream));
        HIP_TRY(hipStreamSynchronize(r.stream));
        omax2 = std::max(omax2, m2);
    }
    for (int d = 0; d < N && !paint; ++d) {
        MultiRank &r = R[d];
        HIP_TRY(hipSetDevice(r.device));
        const int64_t nown = r.p1 - r.p0;
        int32_t rings = 1;
        if (int rc = bfgx_plan_reach_rings(r.plan, std::sqrt((double)omax2), &rings)) return rc;
        if (int rc = bfgx_plan_set_band_reach(r.plan, rings)) return rc;
        if (int rc = bfgx_plan_band_apron(r.plan, r.b0, r.b1, &r.olo, &r.ohi)) return rc;
        HIP_TRY(r.mem.alloc(r.out, (size_t)std::max<int64_t>(nown, 1)));
        HIP_TRY(r.mem.alloc(r.sums, 2));
        HIP_TRY(hipMemsetAsync(r.sums, 0, 2 * sizeof(double), r.stream));
        if (nown <= 0) continue;
        // the apron rings [olo, p0) and [p1, ohi) from whichever ranks own them (complete there: nothing is summed)
        for (int s = 0; s < N; ++s) {
            if (s == d) continue;
            const int64_t a0 = std::max(r.olo, R[s].p0), a1 = std::min(r.ohi, R[s].p1);
            if (a1 <= a0) continue;
            HIP_TRY(hipStreamWaitEvent(r.stream, R[s].done, 0));
            if (int rc = copy_between(r.full + (size_t)(a0 - r.flo) * width * esz, r.device,
                                      R[s].full + (size_t)(a0 - R[s].flo) * width * esz, R[s].device, (size_t)(a1 - a0) * width * esz,
                                      r.stream)) return rc;
        }
        HIP_TRY(r.mem.alloc(r.map, (size_t)(r.ohi - r.olo)));
        HIP_TRY(hipMemcpyAsync(r.map, map_in + r.olo, sizeof(double) * (size_t)(r.ohi - r.olo), hipMemcpyHostToDevice, r.stream));
        // the kernel indexes the map by global pixel number: virtual base
        if (int rc = bfgx_regrid_bands_device(r.plan, r.b0, r.b1, (const double *)r.map - r.olo, r.full + (size_t)(r.olo - r.flo) * width * esz,
                                              r.olo, r.ohi, dm.acc(), r.out, r.sums)) return rc;
        HIP_TRY(hipMemcpyAsync(map_out + r.p0, r.out, sizeof(double) * (size_t)nown, hipMemcpyDeviceToHost, r.stream));
    }
    // ---- join: the slices are disjoint; far deposits (global pixel numbers, almost always none) are added on the host
    double sum_in = 0.0, sum_out = 0.0;
    for (int d = 0; d < N; ++d) {
        MultiRank &r = R[d];
        HIP_TRY(hipSetDevice(r.device));
        HIP_TRY(hipStreamSynchronize(r.stream));
        if (int rc = bfgx_plan_status(r.plan)) return rc;
    }
    if (!paint) {
        for (int d = 0; d < N; ++d) {
            MultiRank &r = R[d];
            HIP_TRY(hipSetDevice(r.device));
            double s2[2] = {0, 0};
            HIP_TRY(hipMemcpy(s2, r.sums, sizeof(s2), hipMemcpyDeviceToHost));
            sum_in += s2[0]; sum_out += s2[1];
            int64_t nf = 0;
            if (r.p1 > r.p0) if (int rc = bfgx_plan_far_fetch(r.plan, 0, nullptr, nullptr, &nf)) return rc;
            if (nf > 0) {
                std::vector<int64_t> fp((size_t)nf);
                std::vector<double> fv((size_t)nf);
                if (int rc = bfgx_plan_far_fetch(r.plan, nf, fp.data(), fv.data(), &nf)) return rc;
                for (int64_t i = 0; i < nf; ++i) map_out[fp[i]] += fv[i];          // (already counted in the rank's deposit sum)
            }
        }
    }
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->sum_in = sum_in; stats->sum_out = sum_out; stats->n_pairs = -1;
        stats->ms_kernels = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();   // whole call
    }
    return (!paint && o.check_mass) ? check_mass(sum_in, sum_out) : BFGX_OK;
}

}  // namespace

extern "C" {

int bfgx_baryonify_shell_multi(const bfgx_catalog *cat_host, const bfgx_model *model, int64_t nside, const double *map_in_host,
                               double *map_out_host, int32_t ndev, const int32_t *devices, const bfgx_opts *opts, bfgx_stats *stats)
{
    return shell_multi(false, cat_host, model, nside, map_in_host, map_out_host, ndev, devices, opts, stats);
}

int bfgx_paint_shell_multi(const bfgx_catalog *cat_host, const bfgx_model *model, int64_t nside, double *map_out_host,
                           int32_t ndev, const int32_t *devices, const bfgx_opts *opts, bfgx_stats *stats)
{
    return shell_multi(true, cat_host, model, nside, nullptr, map_out_host, ndev, devices, opts, stats);
}

}  // extern "C"
