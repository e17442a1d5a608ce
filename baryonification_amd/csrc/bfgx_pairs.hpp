// The handles of the per-halo entries for models that are Python callables (bfgx_{shell,grid,snapshot}_pairs_*) and the steps the three
// families share; bfgx_api.hip includes it before bfgx_callable_api.inc.  Needs fail, alloc_fail, HIP_TRY, the owners of bfgx_devmem.hpp,
// CallStream and plan_destroy (bfgx_oneshot.hpp), the shell and grid plans, GridHostCatalog and the kernels of bfgx_snapshot_pairs.hpp.
#pragma once
#include <hipcub/hipcub.hpp>
#include <memory>

enum class PairsKind { Shell, Grid, Snap };

// What bfgx.h declares as the opaque bfgx_pairs: the part the three families share.  `stream` is the one stream every call on the handle
// uses: the plan's (NULL, the default stream, for the plans made here), or the snapshot handle's own, which `own` then destroys.
struct bfgx_pairs {
    const PairsKind kind;
    int device = -1;                              // < 0: no device work has been issued for the handle yet
    hipStream_t stream = nullptr;
    CallStream own;
    int64_t n = 0, total = 0;                     // halos; pairs of all of them
    std::vector<int64_t> off_h;                   // exclusive prefix sum of the per-halo pair counts, n + 1 entries
    DevBuf off, counts;
    explicit bfgx_pairs(PairsKind k) : kind(k) {}
    bfgx_pairs(const bfgx_pairs &) = delete;
    bfgx_pairs &operator=(const bfgx_pairs &) = delete;
    void on(int dev, hipStream_t s) { device = dev; stream = s; }
    void drain() const { if (device >= 0) { (void)hipSetDevice(device); (void)hipStreamSynchronize(stream); } }
protected:
    ~bfgx_pairs() = default;                      // a handle goes as the Pairs<> it is: pairs_end
};

namespace {

struct PlanDelete { template <typename P> void operator()(P *p) const { plan_destroy(p); } };
template <typename P> using PlanPtr = std::unique_ptr<P, PlanDelete>;

// The members of each family.  A plan stands first: it is released after the buffers beside it.
struct ShellBody {
    static constexpr PairsKind kKind = PairsKind::Shell;
    static constexpr const char *kName = "shell";
    PlanPtr<bfgx_plan> plan;
    DevBuf cols[kCatCols];
    bfgx_catalog dcat{};
    int paint = 0;
    DevBuf vals;                                  // one double per pair: the radii going down, the model's values coming up
    PoolBuf acc, in, out, sums;
};

struct GridBody {
    static constexpr PairsKind kKind = PairsKind::Grid;
    static constexpr const char *kName = "grid";
    PlanPtr<bfgx_grid_plan> plan;
    GridHostCatalog cat;
    int paint = 0;
    std::vector<int64_t> item0_h;                 // exclusive prefix sum of the per-halo work items (kGridChunk pixels each)
    DevBuf item0, item_halo;
    PoolBuf batch, acc, in, out, sums;
};

struct SnapBody {
    static constexpr PairsKind kKind = PairsKind::Snap;
    static constexpr const char *kName = "snapshot";
    SnapGeom g{};
    DevModel model{};
    DevList mem;                                  // the model's device arrays
    int64_t np = 0;                               // particles
    DevBuf xyz[3], recs, keys, acc;
    PoolBuf batch;
};

// THE RELEASE RULE, stated once: the handle's stream is drained, with its device selected, before any buffer, plan or stream of the
// handle is released.  It holds by construction: C++ runs a destructor's body before it destroys members and bases, so whichever way a
// handle goes (an `end` entry, or the scope owner of a `begin` that returns early) ~Pairs drains first; then the family's buffers go,
// then its plan, then the base's buffers and, last, a stream of the handle's own.
template <typename Body> struct Pairs final : bfgx_pairs, Body {
    Pairs() : bfgx_pairs(Body::kKind) {}
    ~Pairs() { drain(); }
};
using ShellPairs = Pairs<ShellBody>;
using GridPairs = Pairs<GridBody>;
using SnapPairs = Pairs<SnapBody>;

// the three exported `end` entries; NULL is a no-op
void pairs_end(bfgx_pairs *h)
{
    if (!h) return;
    switch (h->kind) {
    case PairsKind::Shell: delete static_cast<ShellPairs *>(h); break;
    case PairsKind::Grid: delete static_cast<GridPairs *>(h); break;
    case PairsKind::Snap: delete static_cast<SnapPairs *>(h); break;
    }
}

// what `begin` holds its new handle in until it hands it to the caller (release()): every earlier return ends the handle
struct PairsEnd { void operator()(bfgx_pairs *h) const { pairs_end(h); } };
template <typename T> using PairsOwner = std::unique_ptr<T, PairsEnd>;

// The one checked down-cast: nullptr for NULL and for a handle of another family.  Every entry starts here.
template <typename T> T *pairs_as(bfgx_pairs *h) { return h && h->kind == T::kKind ? static_cast<T *>(h) : nullptr; }

template <typename T> int pairs_refuse() { return fail(BFGX_ERR_INVALID, "NULL argument, or not a handle of bfgx_%s_pairs_begin", T::kName); }

// h = pairs_as<T>(handle) and a halo range [j0, j1) of it; np: the pairs of that range
template <typename T> int pairs_range(const T *h, int64_t j0, int64_t j1, int64_t *np)
{
    if (!h) return pairs_refuse<T>();
    if (j0 < 0 || j1 < j0 || j1 > h->n) return fail(BFGX_ERR_INVALID, "halo range [%lld, %lld) outside [0, %lld)", (long long)j0, (long long)j1, (long long)h->n);
    *np = h->off_h[(size_t)j1] - h->off_h[(size_t)j0];
    return BFGX_OK;
}

// the per-halo pair counts `begin` has copied down -> off_h and total
int pairs_offsets(bfgx_pairs *h, const int64_t *counts_host)
{
    h->off_h.assign((size_t)h->n + 1, 0);
    for (int64_t j = 0; j < h->n; ++j) {
        if (counts_host[j] < 0) return fail(BFGX_ERR_HIP, "negative pair count");
        h->off_h[(size_t)j + 1] = h->off_h[(size_t)j] + counts_host[j];
    }
    h->total = h->off_h[(size_t)h->n];
    return BFGX_OK;
}

// the device buffer of a batch of np doubles: the grid and snapshot handles grow theirs, the shell handle's holds all pairs since begin
int pairs_reserve(PoolBuf &b, int64_t np) { return b.need(sizeof(double) * (size_t)np); }
int pairs_reserve(DevBuf &, int64_t) { return 0; }

// The two batch transfers, on the handle's stream, which has drained when they return.  `launch(dev)` enqueues the family's kernel.
// Produce np doubles on the device and hand them to the host:
template <typename Buf, typename Launch> int pairs_to_host(bfgx_pairs *h, Buf &buf, int64_t np, double *host, Launch launch)
{
    if (np > 0 && !host) return fail(BFGX_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    if (np > 0) {
        if (pairs_reserve(buf, np)) return alloc_fail("pair batch");
        if (int rc = launch((double *)buf.p)) return rc;
        HIP_TRY(hipMemcpyAsync(host, buf.p, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    return BFGX_OK;
}

// take np doubles from the host and consume them on the device (`host` is the caller's again on return):
template <typename Buf, typename Launch> int pairs_from_host(bfgx_pairs *h, Buf &buf, int64_t np, const double *host, Launch launch)
{
    if (np > 0 && !host) return fail(BFGX_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    if (np > 0) {
        if (pairs_reserve(buf, np)) return alloc_fail("pair batch");
        HIP_TRY(hipMemcpyAsync(buf.p, host, sizeof(double) * (size_t)np, hipMemcpyHostToDevice, h->stream));
        if (int rc = launch((const double *)buf.p)) return rc;
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    return BFGX_OK;
}

// ---- the particle binning of the snapshot entries (bfgx_snapshot_pairs_begin, and the profile measurement of bfgx_snapshot_stack_api.inc)

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

}  // namespace
