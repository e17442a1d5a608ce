// C ABI of libbfgx.so (see include/bfgx.h for the reference lines each entry point replaces).
// Host code only orchestrates: uploads the model once per plan, then enqueues
//   K0 halo_prep -> K1 halo_scatter<OFFSETS> -> K2 regrid (+ sum2)      (BaryonifyShell.process)
//   K0 halo_prep -> K3 halo_scatter<PAINT>                               (PaintProfilesShell.process)
// on one HIP stream.  There is no CPU fallback: without a visible GPU every compute entry point
// returns BFGX_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "../../include/bfgx.h"

#include "bfgx_devmem.hpp"
#include "bfgx_tile_arena.hpp"
#include "bfgx_cosmo.hpp"
#include "bfgx_kernels.hpp"
#include "bfgx_scatter2.hpp"
#include "bfgx_regrid2.hpp"
#include "bfgx_tables.hpp"
#include "bfgx_scan.hpp"
#include "bfgx_grid.hpp"
#include "bfgx_grid_pairs.hpp"
#include "bfgx_fft.hpp"
#include "bfgx_bispec.hpp"
#include "bfgx_fft2d.hpp"
#include "bfgx_deposit.hpp"
#include "bfgx_deposit_cloud.hpp"
#include "bfgx_snapshot.hpp"
#include "bfgx_snapshot_pairs.hpp"
#include "bfgx_grid_gather.hpp"
#include "bfgx_fftlog.hpp"
#include "bfgx_sht.hpp"
#include "bfgx_hpx.hpp"
#include "bfgx_mapstats.hpp"
#include "bfgx_pcl.hpp"
#include "bfgx_stack_core.hpp"
#include "bfgx_stack.hpp"
#include "bfgx_snapshot_stack.hpp"
#include "bfgx_grid_stack.hpp"
#include "bfgx_math_probe.hpp"

using namespace bfgx;

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int alloc_fail(const char *what) { return fail(BFGX_ERR_HIP, kDevAllocFailed, what); }

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(BFGX_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// every entry that takes a device number starts here: libbfgx has no CPU fallback
int select_device(int device)
{
    if (bfgx_device_count() <= 0) return fail(BFGX_ERR_NO_DEVICE, "no HIP device visible: libbfgx has no CPU fallback");
    HIP_TRY(hipSetDevice(device));
    return BFGX_OK;
}

int validate_cosmo(const bfgx_cosmo &c)
{
    if (!(c.Omega_m > 0) || !(c.h > 0) || !(c.Omega_b >= 0) || c.w0 != c.w0)
        return fail(BFGX_ERR_INVALID, "cosmology needs Omega_m > 0, h > 0, Omega_b >= 0, finite w0");
    return BFGX_OK;
}

int validate_table(const bfgx_table &t)
{
    if (t.ndim < 3 || t.ndim > BFGX_MAX_DIM) return fail(BFGX_ERR_INVALID, "table ndim must be in [3, %d]", BFGX_MAX_DIM);
    if (!t.values) return fail(BFGX_ERR_INVALID, "table values pointer is NULL");
    for (int d = 0; d < t.ndim; ++d) {
        if (t.n[d] < 2) return fail(BFGX_ERR_INVALID, "table axis %d needs >= 2 points", d);
        if (!t.axis[d]) return fail(BFGX_ERR_INVALID, "table axis %d pointer is NULL", d);
        for (int i = 1; i < t.n[d]; ++i)
            if (!(t.axis[d][i] > t.axis[d][i - 1]))
                return fail(BFGX_ERR_INVALID, "table axis %d must be strictly ascending", d);
    }
    double tot = 1.0;
    for (int d = 0; d < t.ndim; ++d) tot *= t.n[d];
    if (tot > 2.0e9) return fail(BFGX_ERR_INVALID, "table too large for 32-bit row offsets");
    return BFGX_OK;
}

// compute units of a device (256, the MI355X's, when the runtime does not say)
int device_cu_count(int device)
{
    hipDeviceProp_t prop;
    return (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
}

// optional per-kernel HIP-event timing of a plan: KernelTimerT brackets a launch with a pair of events, read() sums the pairs per kernel kind
struct KernelEvents {
    using Pair = std::pair<hipEvent_t, hipEvent_t>;
    bool timing = false;
    std::vector<Pair> ev[BFGX_NUM_KERNELS], ev_free;
    int enable(int on) { timing = on != 0; return BFGX_OK; }
    int read(int device, hipStream_t stream, double *ms_sum, int64_t *launches)
    {
        if (!ms_sum || !launches) return fail(BFGX_ERR_INVALID, "NULL argument");
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipStreamSynchronize(stream));
        for (int k = 0; k < BFGX_NUM_KERNELS; ++k) {
            double tot = 0.0;
            for (auto &e : ev[k]) {
                float ms = 0.f;
                HIP_TRY(hipEventElapsedTime(&ms, e.first, e.second));
                tot += ms;
                ev_free.push_back(e);
            }
            ms_sum[k] = tot;
            launches[k] = (int64_t)ev[k].size();
            ev[k].clear();
        }
        return BFGX_OK;
    }
    void destroy()
    {
        for (int k = 0; k < BFGX_NUM_KERNELS; ++k)
            for (auto &e : ev[k]) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
        for (auto &e : ev_free) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    }
};

}  // namespace

struct bfgx_plan {
    int device = 0, num_cus = 256;
    hipStream_t stream = nullptr;
    int64_t nside = 0, max_halos = 0;
    Hpx hpx;
    DevModel model;
    DevList mem;                   // device allocations freed with the plan
    HaloRec *recs = nullptr;
    RowSetX *rowsx = nullptr;      // corner rows when the table has extra parameter axes (NC > 4)
    int NC = 4;
    // tile-owned accumulation (algo 1): tiling tables + halo -> tile binning workspace
    int algo = 1;
    bool blocking_growth = false;   // one-shot host API: grow the entry list on overflow (needs a sync)
    float *k0_work_est = nullptr;   // per K0 workgroup: estimated pixels of its narrow halos (k1_form_kernel)
    int32_t *k1_form = nullptr;     // device word: the fast kernel's form when the halo count does not decide it (1 fluid, 0 barrier per tile)
    int64_t k1_nhalos = 0;          // halos of the catalog the binning step has just listed (the fast kernel's form follows their density)
    int k1_fluid = 1;               // the fast kernel's fluid form (bfgx_scatter2.hpp): 1 = from 2 tiles per CU; BFGX_K1_FLUID at plan creation: 0 = never (the barrier-per-tile form), 2 = always (tests)
    Tiling tiling;
    TileArena arena;                 // everything a step resets, in one allocation: the binning counters, K1's tile counter, the per-tile largest |offset|^2, the regrid's control words (bfgx_tile_arena.hpp)
    int32_t *tile_start = nullptr, *entries = nullptr, *overflow = nullptr;
    // a fast plan's halos over <= 4 tiles are placed by K0 itself into fixed-capacity lists [ntiles][entries_a_cap]; the others (and every
    // halo of a generic plan) are listed per K0 workgroup for the placement pass
    int32_t *entries_a = nullptr, *slow_list = nullptr, *slow_cnt = nullptr;
    int32_t entries_a_cap = 0;
    int32_t cnt_pad = 1;             // words between region A's counters of two tiles (a 128-byte line each up to 8192 tiles): see wave_run_issue
    TileRef *tref = nullptr;
    FarList far;                     // deposits of the gathering regrid that need the generic route (bfgx_regrid2.hpp); count and overflow lie in the arena
    FarSrc far_src;                  // the source pixels of those deposits, listed by the gather kernels for regrid_far_eval_kernel; count in the arena, sums behind tile_sums
    int32_t *regrid_lean = nullptr;  // [0] = count (zeroed by the regrid's last launch), then the tiles of the lean kernel (reach <= 1 ring)
    // precision of the displacement path when the caller leaves it to the plan (BFGX_ACC_AUTO): chosen at plan creation from how far the
    // TABLE can move a pixel (plan_pick_precision): fp32 pair math holds SURVEY 8(d)'s 1e-6 mean(map) while one halo moves a pixel by less
    // than kAutoDispPixels; beyond that the parity-grade mode (BFGX_ACC_PARITY), or fp64 throughout where the fast kernel cannot take the table
    int auto_acc = 0;
    double table_disp_pixels = 0.0;  // largest |d| a / D_A of the table within its model-side cut, in pixel sides of this plan's NSIDE
    int32_t *tile_apron = nullptr;   // [ntiles][2] rings / columns of apron (tile_apron_kernel)
    int band_reach = 1;              // banded regrid: rings of apron every rank uses (bfgx_plan_set_band_reach)
    int route_margin = 0;            // rings by which bfgx_disc_rings_device widens every halo's range (bfgx_plan_set_route_margin)
    int64_t cat_blk_rows = 0, cat_blk_stride = 0;      // K0 reads a blocked catalog (bfgx_plan_set_catalog_blocks)
    ScanScratch scan;                // per-block totals and offsets of the multi-workgroup tile scan
    // fast tiled scatter (bfgx_scatter2.hpp): slim per-halo records + interleaved copies of the table
    bool fast_ok = false;            // 3-axis table with a uniform ln r axis, small enough to interleave
    RowRec *rowrec = nullptr;
    void *pairrec = nullptr;         // PairRecT<float> or PairRecT<double>, whichever the last K0 wrote
    FbRec *fbrec = nullptr;
    const float *tab8f = nullptr;
    const double *tab8d = nullptr;
    unsigned long long *pair_total = nullptr;
    double *tile_sums = nullptr;     // [ntiles + 1][2] per-tile {sum of source values, sum of deposits} of the tiled regrid, then [kFarEvalWgs] deposit totals of the far-pixel evaluator
    std::vector<int32_t> band_tile0_host;   // first tile of every band (+ total)
    int64_t capacity = 0;
    KernelEvents events;             // optional per-kernel HIP-event timing (bfgx_plan_timing_*)
};

namespace {

// brackets one kernel launch with a pair of events on the plan's stream when timing is enabled
template <class Plan>
struct KernelTimerT {
    Plan *p; int kind; KernelEvents::Pair e{nullptr, nullptr};
    KernelTimerT(Plan *p_, int kind_) : p(p_), kind(kind_)
    {
        KernelEvents &k = p->events;
        if (!k.timing) return;
        if (!k.ev_free.empty()) { e = k.ev_free.back(); k.ev_free.pop_back(); }
        else { (void)hipEventCreate(&e.first); (void)hipEventCreate(&e.second); }
        (void)hipEventRecord(e.first, p->stream);
    }
    ~KernelTimerT()
    {
        if (!p->events.timing) return;
        (void)hipEventRecord(e.second, p->stream);
        p->events.ev[kind].push_back(e);
    }
};
using KernelTimer = KernelTimerT<bfgx_plan>;

// a device copy of host[count] (or of a vector), owned by mem, filled on the stream
template <typename T>
static int owned_upload(DevList &mem, hipStream_t stream, const T *host, size_t count, const T *&dev_out)
{
    HIP_TRY(mem.upload(dev_out, host, count, stream));
    return BFGX_OK;
}
template <typename T>
static int owned_upload(DevList &mem, hipStream_t stream, const std::vector<T> &v, const T *&dev_out)
{
    return owned_upload(mem, stream, v.data(), v.size(), dev_out);
}

// a list too small for `needed` entries: a new one with a quarter + 1024 to spare (contents are not kept; the caller has drained the stream)
template <typename T>
static int grow_list(DevList &mem, T *&ptr, int64_t &capacity, int64_t needed)
{
    const int64_t cap = needed + needed / 4 + 1024;
    HIP_TRY(mem.regrow(ptr, (size_t)cap));
    capacity = cap;
    return BFGX_OK;
}

static int validate_model(const bfgx_model *model)
{
    if (int rc = validate_cosmo(model->cosmo_runner)) return rc;
    if (int rc = validate_cosmo(model->cosmo_model)) return rc;
    if (int rc = validate_table(model->table)) return rc;
    if (!(model->eps_runner > 0)) return fail(BFGX_ERR_INVALID, "epsilon_max must be > 0");
    if (!(model->massdef_runner.Delta > 0) || !(model->massdef_model.Delta > 0))
        return fail(BFGX_ERR_INVALID, "mass definition needs numeric Delta > 0");
    return BFGX_OK;
}

// device copy of the model: table axes + values (r innermost), backgrounds, mass definitions; `with_da` adds the
// D_A(z) spline the lightcone runners need.  Synchronises the stream before returning (staging buffers are local).
static int upload_model(DevList &mem, hipStream_t stream, const bfgx_model *model, bool with_da, DevModel &m, int &NC)
{
    const bfgx_table &t = model->table;
    std::memset(&m, 0, sizeof(m));
    m.tab.ndim = t.ndim;
    size_t nvals = 1;
    for (int d = 0; d < t.ndim; ++d) {
        m.tab.n[d] = t.n[d];
        nvals *= (size_t)t.n[d];
        if (int rc = owned_upload(mem, stream, t.axis[d], (size_t)t.n[d], m.tab.axis[d])) return rc;
    }
    {
        // device layout [z][M][p0][p1][r]: the radial row of every (z, M, params) corner is contiguous
        std::vector<double> tr;
        const double *src = t.values;
        if (t.ndim > 3) {
            // host order [z][M][r][p...] (np C order, the extra axes last) -> device order [z][M][p...][r]
            const size_t nz = t.n[0], nm = t.n[1], nr = t.n[2];
            size_t nx = 1;
            for (int d = 3; d < t.ndim; ++d) nx *= (size_t)t.n[d];
            tr.resize(nvals);
            for (size_t zm = 0; zm < nz * nm; ++zm)
                for (size_t ir = 0; ir < nr; ++ir)
                    for (size_t q = 0; q < nx; ++q)
                        tr[(zm * nx + q) * nr + ir] = t.values[(zm * nr + ir) * nx + q];
            src = tr.data();
        }
        if (int rc = owned_upload(mem, stream, src, nvals, m.tab.values)) return rc;
        std::vector<float> v32(nvals);                 // fp32 copy for the mixed-precision pair path (pair_value_fast32)
        for (size_t q = 0; q < nvals; ++q) v32[q] = (float)src[q];
        if (int rc = owned_upload(mem, stream, v32, m.tab.values32)) return rc;
        HIP_TRY(hipStreamSynchronize(stream));
        NC = 4 << (t.ndim - 3);
    }
    m.tab.rdelta = t.rdelta_sampling;
    m.tab.logv = t.log_values;
    m.tab.eps_model = t.eps_model;
    {   // uniform ln r axis -> O(1) index guess
        const double *g = t.axis[2];
        const int n = t.n[2];
        const double step = (g[n - 1] - g[0]) / (n - 1);
        bool uni = true;
        for (int i = 0; i < n; ++i)
            if (std::fabs(g[i] - (g[0] + i * step)) > 1e-9 * std::fabs(step)) { uni = false; break; }
        m.tab.r_uniform = uni ? 1 : 0;
        m.tab.r0 = g[0];
        m.tab.r1 = g[n - 1];
        m.tab.inv_dr = 1.0 / step;
    }
    m.bg_runner = make_background(model->cosmo_runner);
    m.bg_model = make_background(model->cosmo_model);
    m.md_runner = model->massdef_runner;
    m.md_model = model->massdef_model;
    m.eps_runner = model->eps_runner;
    m.same_model = (std::memcmp(&m.bg_runner, &m.bg_model, sizeof(Background)) == 0 && m.md_runner.Delta == m.md_model.Delta &&
                    m.md_runner.rho_type == m.md_model.rho_type) ? 1 : 0;
    if (with_da) {
        std::vector<double> knots, coef;
        da_spline(m.bg_runner, knots, coef);
        if (int rc = owned_upload(mem, stream, coef, m.da_coef)) return rc;
        m.da_step = kDaZmax / (kDaKnots - 1);
        HIP_TRY(hipStreamSynchronize(stream));
    }
    return BFGX_OK;
}

static int check_catalog(const bfgx_plan *p, const bfgx_catalog *c)
{
    if (!p || !c) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (c->n < 0 || c->n > p->max_halos) return fail(BFGX_ERR_INVALID, "catalog size %lld exceeds plan max_halos %lld",
                                                     (long long)c->n, (long long)p->max_halos);
    if (c->n > 0 && (!c->M || !c->z || !c->ra || !c->dec)) return fail(BFGX_ERR_INVALID, "catalog column pointer is NULL");
    for (int k = 0; k < p->model.tab.ndim - 3; ++k)
        if (c->n > 0 && !c->extra[k]) return fail(BFGX_ERR_INVALID, "catalog is missing the column of table parameter axis %d", k);
    return BFGX_OK;
}

static bool use_fast(const bfgx_plan *p) { return p->fast_ok && p->algo == 1; }

// The precision and pix_offsets layout of one displacement call, settled once per entry by disp_mode, and the K1 / K2 instantiations it selects:
//   F32    fp32 pair math, float [n][3]:   launch_tile_scatter<OFFSETS, float>,  tile_regrid3_kernel<float, float>
//   F64    fp64 throughout, double [n][3]: launch_tile_scatter<OFFSETS, double>, tile_regrid3_kernel<double, double>
//   SPLIT  parity-grade: fp64 pair records, float hi [n][3] then lo [n][3]: <OFFSETS, float> + TileLaunch::offsets_lo, <float, double, SPLIT>
struct DispMode {
    enum Kind { F32, F64, SPLIT } kind = F32;
    bool fp64() const { return kind != F32; }                 // fp64 pair records from K0, fp64 geometry in the regrid
    bool split() const { return kind == SPLIT; }
    size_t pixel_bytes() const { return fp64() ? 24 : 12; }
    float *lo(const void *offsets, int64_t n) const { return split() ? (float *)offsets + 3 * (size_t)n : nullptr; }   // of n pixels at `offsets`
    int acc() const { return kind == F32 ? BFGX_ACC_F32 : kind == F64 ? BFGX_ACC_F64 : BFGX_ACC_PARITY; }
};

// BFGX_ACC_AUTO -> what the plan chose from its table; BFGX_ACC_PARITY needs the fast tile kernel (3-axis table, uniform ln r)
// and falls back to fp64 throughout (a superset of its accuracy) elsewhere.  one_array: the caller's pix_offsets are ONE array
// (the band entries, whose slices travel between ranks): the parity-grade mode is served by fp64 throughout there
static int disp_mode(const bfgx_plan *p, int acc, bool one_array, DispMode &m)
{
    if (!p) return fail(BFGX_ERR_INVALID, "NULL plan");
    if (acc != BFGX_ACC_AUTO && acc != BFGX_ACC_F32 && acc != BFGX_ACC_F64 && acc != BFGX_ACC_PARITY)
        return fail(BFGX_ERR_INVALID, "acc_f64 = %d: must be BFGX_ACC_AUTO (-1), 0 (f32), 1 (f64) or BFGX_ACC_PARITY (3)", acc);
    if (acc == BFGX_ACC_AUTO) acc = p->auto_acc;
    const bool parity = acc == BFGX_ACC_PARITY && use_fast(p);
    m.kind = acc == BFGX_ACC_F32 ? DispMode::F32 : (parity && !one_array) ? DispMode::SPLIT : DispMode::F64;
    return BFGX_OK;
}

// The precision of one painting call (acc_f64 0 / 1 / 2), settled once per entry by paint_mode: F32 float map, fp32 pair math; F64 double map,
// fp64 throughout; MIXED fp32 pair math (K0 writes fp32 pair records), fp64 LDS accumulation and map -- F64 where the fast kernel cannot take the table
struct PaintMode {
    enum Kind { F32, F64, MIXED } kind = F64;
    bool map_f64() const { return kind != F32; }              // K3 launch_tile_scatter<PAINT, double>, else <PAINT, float>
    bool k0_f64() const { return kind == F64; }
    bool pair_f32() const { return kind == MIXED; }
};

static int paint_mode(const bfgx_plan *p, int acc, PaintMode &m)
{
    if (!p) return fail(BFGX_ERR_INVALID, "NULL plan");
    if (acc < 0 || acc > 2) return fail(BFGX_ERR_INVALID, "acc_f64 must be 0, 1 or 2");
    m.kind = acc == 0 ? PaintMode::F32 : (acc == 2 && use_fast(p)) ? PaintMode::MIXED : PaintMode::F64;
    return BFGX_OK;
}

// what one K1 / K3 launch does beyond the plan's configuration; the defaults: the whole sphere, one output array
struct TileLaunch {
    float *offsets_lo = nullptr;     // SPLIT pix_offsets: the low halves, indexed like the high ones
    bool paint_pair_f32 = false;     // PaintMode::MIXED
    float *omax = nullptr;           // K1's flush stores the largest |offset|^2 of every tile here (p->arena.omax: the reach of the regrid)
    int tile_lo = 0, tile_n = -1;    // tiles to process (-1: the whole sphere)
    int spread_tiles = -1;           // tiles the binned catalog covers when not the launch's (the density that picks the fast kernel's form)
};

// K0.  bin: also reserve the halo's slots in the tile entry lists; f64: precision of the fast kernel's pair records;
// rec_all: write the full HaloRec of every halo (halo-centric kernels), otherwise only of those the generic tile kernel takes
static int launch_prep(bfgx_plan *p, const bfgx_catalog *c, int fallback4, bool bin, bool f64, bool rec_all)
{
    if (c->n == 0) return BFGX_OK;
    const unsigned grid = (unsigned)((c->n + 255) / 256);
    KernelTimer kt(p, BFGX_K_PREP);
    PrepOut o;
    std::memset(&o, 0, sizeof(o));
    o.rec = p->recs; o.rowsx = p->rowsx;
    o.fast = (bin && use_fast(p)) ? 1 : 0;
    o.rec_all = (rec_all || !o.fast) ? 1 : 0;
    o.rowrec = p->rowrec; o.pairrec = p->pairrec; o.fbrec = p->fbrec;
    if (bin) {
        o.tref = p->tref; o.cnt_a = p->arena.cnt_a_pad; o.cnt_b = p->arena.cnt_b;
        o.cnt_pad = p->cnt_pad;
        o.work_est = o.fast ? p->k0_work_est : nullptr;
        o.entries_a = p->entries_a; o.cap_a = p->entries_a_cap; o.slow_list = p->slow_list; o.slow_cnt = p->slow_cnt;
    }
    o.ncell_m = p->model.tab.n[1] - 1; o.nrm1 = p->model.tab.n[2] - 1;
    o.blk_rows = p->cat_blk_rows; o.blk_stride = p->cat_blk_stride;
    ExtraCols ex;
    for (int k = 0; k < BFGX_MAX_EXTRA; ++k) ex.p[k] = c->extra[k];
#define BFGX_PREP(NCV, REAL)                                                                                        \
    hipLaunchKernelGGL((halo_prep_kernel<NCV, REAL>), dim3(grid), dim3(256), 0, p->stream, p->model, p->hpx, c->n, c->M, c->z, \
                       c->ra, c->dec, ex, c->ln1pz, c->lnM, fallback4, p->tiling, o)
    if (p->NC == 4) { if (f64) BFGX_PREP(4, double); else BFGX_PREP(4, float); }
    else if (p->NC == 8) BFGX_PREP(8, float);
    else if (p->NC == 16) BFGX_PREP(16, float);
    else if (p->NC == 32) BFGX_PREP(32, float);
    else BFGX_PREP(64, float);
#undef BFGX_PREP
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

static int launch_place(bfgx_plan *p, const bfgx_catalog *c)
{
    const unsigned grid = (unsigned)((c->n + 255) / 256);
    hipLaunchKernelGGL(tile_place_kernel, dim3(grid), dim3(256), 0, p->stream, p->hpx, p->tiling, c->n,
                       (const TileRef *)p->tref, (const int32_t *)p->tile_start, p->arena.cur_b, p->entries, p->capacity, p->overflow,
                       (const int32_t *)p->slow_list, (const int32_t *)p->slow_cnt);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

// halo -> tile entry lists: zero counters, K0 (counts), scan, fill
static int launch_prep_and_bin(bfgx_plan *p, const bfgx_catalog *c, int fallback4, bool f64)
{
    p->k1_nhalos = c->n;
    // the step's one memset: the binning counters, K1's tile counter, the per-tile largest |offset|^2 and the regrid's control words
    HIP_TRY(hipMemsetAsync(p->arena.base, 0, p->arena.zeroed_bytes, p->stream));
    if (int rc = launch_prep(p, c, fallback4, true, f64, false)) return rc;
    KernelTimer kt(p, BFGX_K_BIN);
    const int nt_i = p->tiling.ntiles, nsb = (nt_i + kScanTilesPerWg - 1) / kScanTilesPerWg;
    const int32_t *cnt = p->arena.cnt_b;
    if (nsb <= 1 || nsb > 1024) {
        hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(1024), 0, p->stream, nt_i, cnt, p->tile_start);
    } else {        // NSIDE >= 2048: the scan spread over the tiles' blocks (three short launches instead of up to 48 serial rounds)
        int32_t *tot = p->scan.block_tot, *off = p->scan.block_off;
        hipLaunchKernelGGL(tile_scan_part_kernel<0>, dim3(nsb), dim3(1024), 0, p->stream, nt_i, cnt, p->tile_start, tot, (const int32_t *)off);
        hipLaunchKernelGGL(tile_scan_blocks_kernel, dim3(1), dim3(1024), 0, p->stream, nsb, nt_i, (const int32_t *)tot, off, p->tile_start);
        hipLaunchKernelGGL(tile_scan_part_kernel<1>, dim3(nsb), dim3(1024), 0, p->stream, nt_i, cnt, p->tile_start, tot, (const int32_t *)off);
    }
    HIP_TRY(hipGetLastError());
    if (c->n > 0) if (int rc = launch_place(p, c)) return rc;
    return BFGX_OK;
}

template <int MODE, typename ACC>
static int launch_scatter(bfgx_plan *p, int64_t n, ACC *out, int64_t *counts)
{
    if (n == 0) return BFGX_OK;
    const unsigned grid = (unsigned)((n + kWavesPerBlock - 1) / kWavesPerBlock);
    KernelTimer kt(p, MODE == MODE_OFFSETS ? BFGX_K_OFFSETS : (MODE == MODE_PAINT ? BFGX_K_PAINT : BFGX_K_COUNT));
    hipLaunchKernelGGL((halo_scatter_kernel<MODE, ACC>), dim3(grid), dim3(kWave * kWavesPerBlock), 0, p->stream,
                       make_pair_table(p->model.tab), p->hpx, n, (const HaloRec *)p->recs, out, counts);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

template <int MODE, typename ACC, int NC>
static int launch_tile_scatter_nc(bfgx_plan *p, ACC *out, const TileLaunch &k)
{
    constexpr int NCOMP = (MODE == MODE_OFFSETS) ? 3 : 1;
    const size_t lds = tile_lds_bytes<NC>(p->tiling.BR, p->tiling.W, NCOMP);
    auto kern = tile_scatter_kernel<MODE, ACC, NC>;
    HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    KernelTimer kt(p, MODE == MODE_OFFSETS ? BFGX_K_OFFSETS : (MODE == MODE_PAINT ? BFGX_K_PAINT : BFGX_K_COUNT));
    const int grid = k.tile_n < 0 ? p->tiling.ntiles : std::max(k.tile_n, 1);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kWave * kWavesPerBlock), lds, p->stream,
                       make_pair_table(p->model.tab), p->hpx, p->tiling, (const HaloRec *)p->recs, (const RowSetX *)p->rowsx,
                       (const int32_t *)p->tile_start, (const int32_t *)p->entries, p->capacity, out, p->pair_total,
                       (unsigned int *)k.omax, k.tile_lo, k.tile_n);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

// fast kernel: every halo of a fast plan, from the tile's fixed list and its part of the shared list
template <int MODE, typename ACC, typename real, int PM = 0>
static int launch_tile_scatter2(bfgx_plan *p, ACC *out, const TileLaunch &k, ACC *out_lo = nullptr)
{
    constexpr int NCOMP = (MODE == MODE_OFFSETS) ? 3 : 1;
    constexpr int kNP = 1;          // pairs per lane per trip of the fast kernel's pair loop
    const size_t lds = tile2_lds_bytes<real>(p->tiling.BR, p->tiling.W, NCOMP);
    auto kern = tile_scatter2_kernel<MODE, ACC, real, kNP, PM>;
    HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    Tab8T<real> tb;
    tb.v = (sizeof(real) == 4) ? (const real *)p->tab8f : (const real *)p->tab8d;
    tb.r0 = (real)p->model.tab.r0; tb.r1 = (real)p->model.tab.r1; tb.inv_dr = (real)p->model.tab.inv_dr;
    tb.nr = p->model.tab.n[2]; tb._pad = 0;
    // persistent grid: two 512-thread workgroups per CU (LDS and registers allow exactly that) draw tiles from a counter that the
    // binning step has reset
    unsigned int *tile_counter = p->arena.tile_counter;
    const int ntodo = k.tile_n < 0 ? p->tiling.ntiles : std::max(k.tile_n, 1);
    KernelTimer kt(p, MODE == MODE_OFFSETS ? BFGX_K_OFFSETS : (MODE == MODE_PAINT ? BFGX_K_PAINT : BFGX_K_COUNT));
    int32_t *form = nullptr;               // non-NULL: both forms are launched and this device word says which one works
    if constexpr (MODE != MODE_COUNT) {
        // the fluid form (one 1024-thread workgroup per CU, two tile slots, no barrier between tiles): BFGX_K1_FLUID=0 at plan creation keeps the other
        const size_t ldsf = tile2f_lds_bytes<real>(p->tiling.BR, p->tiling.W, NCOMP);
        // (fewer than two tiles per CU -- NSIDE <= 256 -- keep the other form: half as many workgroups cannot balance so few tiles; a rank that owns an eighth of the NSIDE-1024 sphere, 776 tiles, is 4 % faster in the fluid form)
        // ... and a sparse catalog (a patch of the sky, a few thousand halos: most tiles list nothing): sixteen waves walking through an
        // empty slot and one wave's chain of dependent loads per drawn tile cost more than the barrier form's zero-and-store (1e4 halos at
        // NSIDE 4096: 2.34 against 1.37 ms; 1e5 at NSIDE 2048: 0.68 against 0.58).  Work per tile follows the halo DENSITY (a halo's
        // pixels grow with NSIDE^2 as the tiles do): 6e5 halos per sphere of the benchmark's catalog are the crossover (5e5 at NSIDE 1024: 0.278
        // against 0.269 ms; 7e5: 0.319 against 0.342) -- 4800 pairs per tile.  A count of halos does not say how large they are, though (1e5
        // halos at z < 0.05 hold 2300 pixels each: fluid 0.82 / 0.68 ms against 1.03 / 1.09 for displacement / painting): from 6e5 halos
        // per sphere the fluid form is taken outright; below, K0's per-workgroup sums of the halos' estimated pixels decide ON THE DEVICE
        // (k1_form_kernel) and both forms are launched -- the one not chosen returns at once (~5 us).
        const bool eligible = p->k1_fluid && ldsf <= (size_t)160 * 1024 && p->tiling.BR <= kWave && ntodo >= 2 * p->num_cus;
        const int nspread = k.spread_tiles > 0 ? k.spread_tiles : ntodo;      // (the tiles the binned halos cover)
        const bool dense = (double)p->k1_nhalos * (double)p->tiling.ntiles >= 6.0e5 * (double)nspread;
        const bool forced = p->k1_fluid == 2 && ldsf <= (size_t)160 * 1024 && p->tiling.BR <= kWave;
        if (eligible && !dense && !forced && p->k0_work_est && p->k1_nhalos > 0) {
            const int nblk = (int)((p->k1_nhalos + 255) / 256);
            hipLaunchKernelGGL(k1_form_kernel, dim3(1), dim3(1024), 0, p->stream, nblk, (const float *)p->k0_work_est, 4800.0f * (float)nspread, p->k1_form);
            form = p->k1_form;
        }
        if (forced || (eligible && (dense || form))) {
            auto kf = tile_scatter2f_kernel<MODE, ACC, real, PM>;
            HIP_TRY(hipFuncSetAttribute((const void *)kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsf));
            const int gridf = std::min(ntodo, p->num_cus);
            hipLaunchKernelGGL(kf, dim3(std::max(gridf, 1)), dim3(kWave * FluidWaves<real>::n), ldsf, p->stream, tb, p->hpx, p->tiling,
                               (const RowRec *)p->rowrec, (const PairRecT<real> *)p->pairrec, (const FbRec *)p->fbrec,
                               (const int32_t *)p->tile_start, (const int32_t *)p->arena.cnt_a_pad, (const int32_t *)p->arena.cnt_b,
                               (const int32_t *)p->entries, p->capacity, (const int32_t *)p->entries_a, (int)p->entries_a_cap, (int)p->cnt_pad, out, out_lo, tile_counter,
                               (unsigned int *)k.omax, k.tile_lo, k.tile_n, p->overflow, (const int32_t *)form, 1);
            HIP_TRY(hipGetLastError());
            if (!form) return BFGX_OK;
        }
    }
    const int grid = std::min(ntodo, 2 * p->num_cus);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kWave * kW2), lds, p->stream, tb, p->hpx, p->tiling,
                       (const RowRec *)p->rowrec, (const PairRecT<real> *)p->pairrec, (const FbRec *)p->fbrec,
                       (const int32_t *)p->tile_start, (const int32_t *)p->arena.cnt_a_pad, (const int32_t *)p->arena.cnt_b,
                       (const int32_t *)p->entries, p->capacity, (const int32_t *)p->entries_a, (int)p->entries_a_cap, (int)p->cnt_pad, out, out_lo, p->pair_total, tile_counter,
                       (unsigned int *)k.omax, k.tile_lo, k.tile_n, (const int32_t *)form, 0);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

// the tiled scatter: the fast kernel if the table allows, the generic kernel otherwise
template <int MODE, typename ACC>
static int launch_tile_scatter(bfgx_plan *p, ACC *out, const TileLaunch &k)
{
    if (use_fast(p)) {
        using real = typename std::conditional<sizeof(ACC) == 8, double, float>::type;
        if constexpr (MODE == MODE_OFFSETS && sizeof(ACC) == 4) {
            // BFGX_ACC_PARITY: fp64 pair math (K0 wrote fp64 pair records) with the parity-grade functions, pix_offsets as two fp32 arrays
            if (k.offsets_lo) return launch_tile_scatter2<MODE, ACC, double, 1>(p, out, k, (ACC *)k.offsets_lo);
        }
        if constexpr (MODE == MODE_PAINT && sizeof(ACC) == 8) {
            // acc_f64 = 2: the pair phase in fp32 (K0 wrote fp32 pair records), LDS accumulation and the stored map in fp64
            if (k.paint_pair_f32) return launch_tile_scatter2<MODE, ACC, float>(p, out, k);
        }
        return launch_tile_scatter2<MODE, ACC, real>(p, out, k);
    }
    if (p->NC == 4) return launch_tile_scatter_nc<MODE, ACC, 4>(p, out, k);
    if (MODE == MODE_COUNT) return launch_tile_scatter_nc<MODE, ACC, 4>(p, out, k);      // census never reads the rows
    if (p->NC == 8) return launch_tile_scatter_nc<MODE, ACC, 8>(p, out, k);
    if (p->NC == 16) return launch_tile_scatter_nc<MODE, ACC, 16>(p, out, k);
    if (p->NC == 32) return launch_tile_scatter_nc<MODE, ACC, 32>(p, out, k);       // three / four property axes (Tabulate.py:524-561)
    return launch_tile_scatter_nc<MODE, ACC, 64>(p, out, k);
}

// blocking: if the entry list overflowed, grow it to the exact size and redo the fill pass
static int ensure_entry_capacity(bfgx_plan *p, const bfgx_catalog *c)
{
    int32_t ov = 0, total = 0;
    HIP_TRY(hipMemcpyAsync(&ov, p->overflow, sizeof(ov), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipMemcpyAsync(&total, p->tile_start + p->tiling.ntiles, sizeof(total), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (!(ov & 1)) return BFGX_OK;             // (bit 2: the fluid kernel gave up -- bfgx_plan_status reports it)
    HIP_TRY(p->mem.regrow(p->entries, (size_t)total + 16));    // (the stream has just been drained: the old list is freed at once)
    p->capacity = (int64_t)total + 16;
    HIP_TRY(hipMemsetAsync(p->overflow, 0, sizeof(int32_t), p->stream));
    HIP_TRY(hipMemsetAsync(p->arena.cur_b, 0, p->arena.cursor_bytes, p->stream));
    return launch_place(p, c);
}

// interleaved copy of a 3-axis table for the fast kernel (Tab8T): [(nz-1)(nm-1)][nr-1][8] = {A_c, B_c}, c = 2 bz + bm,
// A_c = T[iz+bz][im+bm][i], B_c = T[iz+bz][im+bm][i+1] - A_c  (differences formed in fp64)
template <typename real>
static void build_tab8(const bfgx_table &t, std::vector<real> &out)
{
    const size_t nz = t.n[0], nm = t.n[1], nr = t.n[2];
    out.resize((nz - 1) * (nm - 1) * (nr - 1) * 8);
    for (size_t iz = 0; iz + 1 < nz; ++iz)
        for (size_t im = 0; im + 1 < nm; ++im)
            for (size_t i = 0; i + 1 < nr; ++i) {
                real *o = out.data() + ((iz * (nm - 1) + im) * (nr - 1) + i) * 8;
                for (int c = 0; c < 4; ++c) {
                    const double *row = t.values + ((iz + (c >> 1)) * nm + im + (c & 1)) * nr;
                    o[2 * c] = (real)row[i];
                    o[2 * c + 1] = (real)(row[i + 1] - row[i]);
                }
            }
}

// host-side construction of the tiling tables for one nside
static void build_tiling(int64_t nside, bool paint, int &BR, int &W, std::vector<int32_t> &tile0, std::vector<int32_t> &nphi,
                         std::vector<int32_t> &nrmin, std::vector<int32_t> &tband)
{
    auto pow2_floor = [](int64_t v) { int p = 1; while (2 * p <= v) p *= 2; return p; };
    W = std::max(16, std::min(64, pow2_floor(std::max<int64_t>(1, nside / 2))));
    // the painted map needs 8 B of LDS per pixel, pix_offsets 24 B: taller tiles for painting (fewer duplicated ring phases)
    BR = std::max(4, std::min(paint ? 64 : 32, pow2_floor(std::max<int64_t>(1, nside / 8))));
    if (const char *e = std::getenv("BFGX_TILE_W")) W = pow2_floor(std::max(4, std::min(64, std::atoi(e))));   // tuning knobs (W <= 64, a power of two)
    if (const char *e = std::getenv("BFGX_TILE_BR")) BR = std::max(1, std::min(64, std::atoi(e)));
    const int64_t nrings = 4 * nside - 1;
    const int nbands = (int)((nrings + BR - 1) / BR);
    auto rlen = [&](int64_t ring) { return 4 * (ring < nside ? ring : (ring > 3 * nside ? 4 * nside - ring : nside)); };
    tile0.assign(nbands + 1, 0); nphi.assign(nbands, 1); nrmin.assign(nbands, 4);
    for (int b = 0; b < nbands; ++b) {
        const int64_t i0 = 1 + (int64_t)b * BR, i1 = std::min<int64_t>(i0 + BR, 4 * nside);
        int64_t lmax = 0, lmin = INT64_MAX;
        for (int64_t i = i0; i < i1; ++i) { lmax = std::max(lmax, rlen(i)); lmin = std::min(lmin, rlen(i)); }
        nphi[b] = (int)((lmax + W - 1) / W);
        nrmin[b] = (int)lmin;
        tile0[b + 1] = tile0[b] + nphi[b];
    }
    tband.resize(tile0[nbands]);
    for (int b = 0; b < nbands; ++b)
        for (int t = tile0[b]; t < tile0[b + 1]; ++t) tband[t] = b;
}


// How far can this table move a pixel?  The largest |d(r)| a / D_A(z) over the table's (z, M) nodes within the model-side cut r < eps_model R
// and the runner's disc, in pixel sides of the plan's NSIDE.  fp32 pair math carries ~4e-7 of every contribution, and the bilinear deposit turns
// an error of e pixel sides in a source pixel's position into ~e of its value: 1e-6 mean(map) -- SURVEY 8(d)'s tolerance -- holds while a
// halo moves a pixel by a small fraction of a pixel (measured at config 2, closed-form table scaled: 2.6e-7 / 3.9e-7 / 1.3e-6 / 8.0e-6 mean(map) at 0.03 /
// 0.09 / 0.31 / 0.93 pixel sides per halo; 2.1e-5 on the S19 table, which moves 8.6).  Beyond kAutoDispPixels the plan picks the
// parity-grade mode.
constexpr double kAutoDispPixels = 0.1;
static void plan_pick_precision(bfgx_plan *p, const bfgx_model *model)
{
    const bfgx_table &t = model->table;
    p->auto_acc = BFGX_ACC_F32;
    p->table_disp_pixels = 0.0;
    if (t.log_values) return;                                // a profile table: painting has its own modes
    const Background bgr = make_background(model->cosmo_runner), bgm = make_background(model->cosmo_model);
    const double pix = std::sqrt(4.0 * 3.14159265358979323846 / (double)p->hpx.npix);
    const size_t nz = t.n[0], nm = t.n[1], nr = t.n[2];
    size_t nx = 1;
    for (int d = 3; d < t.ndim; ++d) nx *= (size_t)t.n[d];
    double worst = 0.0;
    for (size_t iz = 0; iz < nz; ++iz) {
        const double z = std::exp(t.axis[0][iz]) - 1.0, a = 1.0 / (1.0 + z);
        const double D = z > 0.0 ? angular_diameter_distance(bgr, z) : 0.0;
        for (size_t im = 0; im < nm; ++im) {
            const double M = std::exp(t.axis[1][im]);
            if (!(M > 0.0) || !(a > 0.0)) continue;
            const double Rm = radius_delta(bgm, model->massdef_model, M, a) / a, Rr = radius_delta(bgr, model->massdef_runner, M, a) / a;
            const double rcut = std::min(t.eps_model * Rm, model->eps_runner * Rr);          // comoving Mpc
            for (size_t ir = 0; ir < nr; ++ir) {
                const double r = std::exp(t.axis[2][ir]) * (t.rdelta_sampling ? Rm : 1.0);
                double m = 0.0;
                const double *v = t.values + ((iz * nm + im) * nr + ir) * nx;
                for (size_t q = 0; q < nx; ++q) if (std::isfinite(v[q])) m = std::max(m, std::fabs(v[q]));
                const double px = (D > 0.0) ? m * a / D / pix : (m > 0.0 ? 1.0e30 : 0.0);
                worst = std::max(worst, px);
                if (r >= rcut) break;                        // (the node that closes the interval holding the cut is the last that counts)
            }
        }
    }
    p->table_disp_pixels = worst;
    if (worst > kAutoDispPixels) p->auto_acc = BFGX_ACC_PARITY;
}

// the steps of bfgx_plan_create follow: each returns an error code, the caller destroys the plan
// fast tiled scatter: possible for a 3-axis table with a uniform ln r axis whose interleaved copy stays small
static int plan_init_fast(bfgx_plan *p, const bfgx_table &t, size_t nh)
{
    const size_t n8 = (size_t)(t.n[0] - 1) * (size_t)(t.n[1] - 1) * (size_t)(t.n[2] - 1) * 8;
    p->fast_ok = (t.ndim == 3) && p->model.tab.r_uniform && n8 * sizeof(double) <= ((size_t)256 << 20);
    if (!p->fast_ok) return BFGX_OK;
    std::vector<float> v32;
    std::vector<double> v64;
    build_tab8<float>(t, v32);
    build_tab8<double>(t, v64);
    if (int rc = owned_upload(p->mem, p->stream, v32, p->tab8f)) return rc;
    if (int rc = owned_upload(p->mem, p->stream, v64, p->tab8d)) return rc;
    if (hipStreamSynchronize(p->stream) != hipSuccess) return fail(BFGX_ERR_HIP, "stream sync failed");
    PairRecT<double> *pairrec = nullptr;
    if (p->mem.alloc(p->rowrec, nh)) return alloc_fail("row records");
    if (p->mem.alloc(pairrec, nh)) return alloc_fail("pair records");
    p->pairrec = pairrec;
    if (p->mem.alloc(p->fbrec, nh)) return alloc_fail("fallback records");
    return BFGX_OK;
}

// tiling tables and halo -> tile binning workspace
static int plan_init_binning(bfgx_plan *p, const bfgx_table &t, size_t nh)
{
    int BR, W;
    std::vector<int32_t> tile0, nphi, nrmin, tband;
    build_tiling(p->nside, t.log_values != 0, BR, W, tile0, nphi, nrmin, tband);
    Tiling &T = p->tiling;
    T.BR = BR; T.W = W; T.nbands = (int)nphi.size(); T.ntiles = (int)tband.size();
    if (int rc = owned_upload(p->mem, p->stream, tile0, T.band_tile0)) return rc;
    p->band_tile0_host = tile0;
    if (int rc = owned_upload(p->mem, p->stream, nphi, T.band_nphi)) return rc;
    if (int rc = owned_upload(p->mem, p->stream, nrmin, T.band_nrmin)) return rc;
    if (int rc = owned_upload(p->mem, p->stream, tband, T.tile_band)) return rc;
    std::vector<int32_t> order(tband.size());
    {   // launch order: tiles by their shortest ring / azimuth slices (~ pixels per tile), descending; stable
        std::vector<double> weight(tband.size());
        for (size_t q = 0; q < tband.size(); ++q) { order[q] = (int32_t)q; weight[q] = (double)nrmin[tband[q]] / (double)nphi[tband[q]]; }
        std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return weight[x] > weight[y]; });
    }
    if (int rc = owned_upload(p->mem, p->stream, order, T.tile_order)) return rc;
    {   // the ring table: geometry of every ring, derived once per plan (NSIDE never changes) instead of per tile and step by K1 and K2
        RingRec *rings = nullptr;
        const size_t nrec = (size_t)(4 * p->nside + 1);
        if (p->mem.alloc(rings, nrec)) return alloc_fail("ring table");
        hipLaunchKernelGGL(ring_table_kernel, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, p->stream, p->hpx, rings);
        if (hipGetLastError() != hipSuccess) return fail(BFGX_ERR_HIP, "ring table launch failed");
        T.rings = rings;
    }
    if (hipStreamSynchronize(p->stream) != hipSuccess) return fail(BFGX_ERR_HIP, "stream sync failed");
    p->capacity = 8 * p->max_halos + 4096;
    if (const char *e = std::getenv("BFGX_K1_FLUID")) p->k1_fluid = std::max(0, std::min(2, std::atoi(e)));
    if (const char *e = std::getenv("BFGX_ENTRY_CAP")) p->capacity = std::max<int64_t>(16, std::atoll(e));   // tests: force regrowth
    // region A's counters: a line each while that array stays below 4 MB (atomics to one line serialise; a larger array costs misses)
    p->cnt_pad = kCntPadMax;
    while (p->cnt_pad > 1 && (size_t)T.ntiles * p->cnt_pad * sizeof(int32_t) > ((size_t)4 << 20)) p->cnt_pad >>= 1;
    // the binning counters and, right behind them (16-byte aligned), the control words of the regrid's far list: ONE memset per step
    // zeroes both (a length that is not a multiple of 16 bytes, or two buffers, cost a fill kernel each: 4.5 us)
    const TileArenaLayout AL = tile_arena_layout((size_t)T.ntiles, (size_t)p->cnt_pad);
    int32_t *arena = nullptr;
    if (p->mem.alloc(arena, AL.total_words) || p->mem.alloc(p->tile_start, (size_t)T.ntiles + 1) ||
        p->mem.alloc(p->entries, (size_t)p->capacity) || p->mem.alloc(p->overflow, 1) || p->mem.alloc(p->pair_total, 1) || p->mem.alloc(p->tref, nh))
        return alloc_fail("binning workspace");
    p->arena.bind(arena, AL);
    // capacity of a tile's fixed list: 16 x the mean entries per tile (a rank of an N-GPU run bins its share of the halos into 1 / N
    // of the tiles; a sky patch does the same), a power of two in [64, 32768] (4 x the mean above 512 entries per tile: a catalog of 1e7 small halos lists 4200 per tile, and what does not fit takes the slow route -- K3 3.7 against 1.4 ms), the whole array at most 1 GB
    const double mean = 1.3 * (double)std::max<int64_t>(p->max_halos, 1) / (double)T.ntiles;
    int cap_a = 64;
    while (cap_a < 32768 && (double)cap_a < (mean > 512.0 ? 4.0 : 16.0) * mean + 64.0) cap_a <<= 1;
    while (cap_a > 64 && (size_t)T.ntiles * cap_a * sizeof(int32_t) > ((size_t)1 << 30)) cap_a >>= 1;
    if (const char *e = std::getenv("BFGX_TILE_LIST_CAP")) cap_a = std::max(1, std::atoi(e));        // tests: force the overflow into region B
    const size_t nblk = (nh + 255) / 256;
    if (p->mem.alloc(p->k0_work_est, nblk) || p->mem.alloc(p->k1_form, 4)) return alloc_fail("work estimate");
    if (p->mem.alloc(p->entries_a, (size_t)T.ntiles * cap_a) || p->mem.alloc(p->slow_list, nblk * 256) || p->mem.alloc(p->slow_cnt, nblk))
        return alloc_fail("tile lists");
    p->entries_a_cap = cap_a;
    return BFGX_OK;
}

// far list and regrid workspace
static int plan_init_regrid(bfgx_plan *p)
{
    const Tiling &T = p->tiling;
    // deposits listed for the generic route: four per pixel that moves beyond the gathering reach (15 rings = 9.9 / NSIDE rad).  At NSIDE
    // 1024 on the S19 table that is 0.2 % of the pixels; at NSIDE 2048 the same field in radians sends 8 % there (16 M entries), and a
    // list that overflows costs a second pass with the generic evaluation under divergence (25 ms): room for half the pixels, 1 GB at most
    // (round 4, second half: at config 4's REAL density -- 1e7 halos on one NSIDE-2048 shell, 43 discs over every pixel -- the S19
    // displacements add up to 15 pixels on average and 58 % of the pixels move beyond the 15-ring reach: 1.4e8 listed deposits,
    // 2.8 per pixel.  A list for half the pixels overflowed into the repair pass: K2 35 ms; with room for four deposits of EVERY
    // pixel, 4.3 GB at most, 10 ms.)
    // Sized from the table (ADVICE, round 4): a listed deposit needs a pixel that moves beyond 9.7 pixel sides in total.  Tables that move a
    // pixel by less than a quarter of a pixel per halo list the pole caps only (a few dozen entries): room for 1 / 16 of the pixels
    // (16 B each: 13 MB at NSIDE 1024 instead of 0.8 GB); up to two pixels per halo: half the pixels; beyond: four deposits of every pixel.
    // A list that overflows all the same (many overlapping discs) is repaired in-stream by the regrid's last pass.
    const int64_t npx = p->hpx.npix;
    const int64_t want = p->table_disp_pixels < 0.25 ? npx / 16 : (p->table_disp_pixels < 2.0 ? npx / 2 : 4 * npx);
    p->far.cap = std::min<int64_t>(std::max<int64_t>((int64_t)1 << 20, want), (int64_t)1 << 28);
    if (const char *e = std::getenv("BFGX_FAR_CAP")) p->far.cap = std::max<int64_t>(1024, std::atoll(e));          // tests: force the overflow
    p->far_src.cap = p->far.cap / 4;                  // four deposits per source pixel
    if (p->mem.alloc(p->far.pix, (size_t)p->far.cap) || p->mem.alloc(p->far.val, (size_t)p->far.cap) ||
        p->mem.alloc(p->far_src.ent, (size_t)p->far_src.cap) || p->mem.alloc(p->tile_apron, 2 * (size_t)(T.ntiles + 1)))
        return alloc_fail("far list");
    if (p->mem.alloc(p->regrid_lean, (size_t)(T.ntiles + 4))) return alloc_fail("lean tile list");
    if (hipMemsetAsync(p->regrid_lean, 0, sizeof(int32_t) * 4, p->stream) != hipSuccess) return fail(BFGX_ERR_HIP, "hipMemset failed");
    // the list's counter and its two overflow flags lie in the arena (the full-map regrid swaps far_overflow_full in: launch_regrid_gather)
    p->far.count = &p->arena.ctrl->far_count;
    p->far_src.count = &p->arena.ctrl->far_src_count;
    p->far.overflow = p->arena.band_overflow;
    if (hipMemsetAsync(p->arena.ctrl, 0, p->arena.tail_bytes, p->stream) != hipSuccess) return fail(BFGX_ERR_HIP, "hipMemset failed");
    return BFGX_OK;
}

}  // namespace

extern "C" {

int bfgx_abi_version(void) { return BFGX_ABI_VERSION; }

const char *bfgx_last_error(void) { return g_err.c_str(); }

int bfgx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ------------------------------------------------------------------------------ host cosmology
int bfgx_cosmo_E2(const bfgx_cosmo *c, int64_t n, const double *a, double *out)
{
    if (!c || !a || !out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = validate_cosmo(*c)) return rc;
    const Background b = make_background(*c);
    for (int64_t i = 0; i < n; ++i) out[i] = E2(b, a[i]);
    return BFGX_OK;
}

int bfgx_cosmo_radius(const bfgx_cosmo *c, const bfgx_massdef *md, int64_t n, const double *M, const double *a, double *out)
{
    if (!c || !md || !M || !a || !out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = validate_cosmo(*c)) return rc;
    const Background b = make_background(*c);
    for (int64_t i = 0; i < n; ++i) out[i] = radius_delta(b, *md, M[i], a[i]);
    return BFGX_OK;
}

int bfgx_cosmo_angular_diameter_distance(const bfgx_cosmo *c, int64_t n, const double *z, double *out)
{
    if (!c || !z || !out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = validate_cosmo(*c)) return rc;
    const Background b = make_background(*c);
    for (int64_t i = 0; i < n; ++i) out[i] = angular_diameter_distance(b, z[i]);
    return BFGX_OK;
}

int bfgx_cosmo_da_spline(const bfgx_cosmo *c, double *knots, double *coef)
{
    if (!c || !knots || !coef) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = validate_cosmo(*c)) return rc;
    std::vector<double> k, cf;
    da_spline(make_background(*c), k, cf);
    std::memcpy(knots, k.data(), k.size() * sizeof(double));
    std::memcpy(coef, cf.data(), cf.size() * sizeof(double));
    return BFGX_OK;
}

int bfgx_cosmo_da_eval(const bfgx_cosmo *c, int64_t n, const double *z, double *out)
{
    if (!c || !z || !out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = validate_cosmo(*c)) return rc;
    std::vector<double> k, cf;
    da_spline(make_background(*c), k, cf);
    for (int64_t i = 0; i < n; ++i) out[i] = da_eval(k, cf, z[i]);
    return BFGX_OK;
}

// ------------------------------------------------------------------------------ plan
int bfgx_plan_create(int device, void *hip_stream, int64_t nside, int64_t max_halos,
                     const bfgx_model *model, bfgx_plan **out)
{
    if (!model || !out) return fail(BFGX_ERR_INVALID, "NULL argument");
    *out = nullptr;
    // (the next power of two, NSIDE 2^14, has 3.2e9 pixels: the tile kernels keep first-pixel-of-ring offsets and per-tile counters in 32 bits -- RowScan.start, the
    // walking regrid; 8192, 8.05e8 pixels / 6.4 GB of fp64 map, is the largest shell that is tested)
    if (nside < 1 || nside > 8192) return fail(BFGX_ERR_INVALID, "nside must be 1 .. 8192 (the tile kernels index pixels with 32 bits inside a ring table)");
    if (max_halos < 0) return fail(BFGX_ERR_INVALID, "max_halos < 0");
    if (int rc = validate_model(model)) return rc;
    if (bfgx_device_count() <= 0)
        return fail(BFGX_ERR_NO_DEVICE, "no HIP device visible: libbfgx has no CPU fallback");
    HIP_TRY(hipSetDevice(device));

    bfgx_plan *p = new bfgx_plan();
    p->device = device;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) p->num_cus = cus;
    }
    p->nside = nside;
    p->max_halos = max_halos;
    p->hpx = make_hpx(nside);
    // hip_stream == NULL means the legacy default stream (what torch's default stream is), so that the
    // plan's kernels stay ordered with the caller's own work; the plan never creates a private stream.
    p->stream = (hipStream_t)hip_stream;
    auto bail = [&](int rc) { bfgx_plan_destroy(p); return rc; };

    const bfgx_table &t = model->table;
    if (int rc = upload_model(p->mem, p->stream, model, true, p->model, p->NC)) return bail(rc);
    plan_pick_precision(p, model);
    const size_t nh = (size_t)(max_halos > 0 ? max_halos : 1);
    if (p->mem.alloc(p->recs, nh)) return bail(alloc_fail("halo records"));
    if (p->NC > 4 && p->mem.alloc(p->rowsx, nh)) return bail(alloc_fail("corner rows"));
    if (int rc = plan_init_fast(p, t, nh)) return bail(rc);
    if (int rc = plan_init_binning(p, t, nh)) return bail(rc);
    if (int rc = plan_init_regrid(p)) return bail(rc);
    const ScanScratchLayout SL = scan_scratch_layout();
    int32_t *scan = nullptr;
    if (p->mem.alloc(scan, SL.total_words)) return bail(alloc_fail("tile scan scratch"));
    p->scan.bind(scan, SL);
    if (p->mem.alloc(p->tile_sums, 2 * (size_t)(p->tiling.ntiles + 1) + kFarEvalWgs)) return bail(alloc_fail("tile sums"));
    p->far_src.sums = p->tile_sums + 2 * (size_t)(p->tiling.ntiles + 1);
    if (hipMemsetAsync(p->far_src.sums, 0, sizeof(double) * kFarEvalWgs, p->stream) != hipSuccess) return bail(fail(BFGX_ERR_HIP, "hipMemset failed"));
    if (hipMemsetAsync(p->overflow, 0, sizeof(int32_t), p->stream) != hipSuccess) return bail(fail(BFGX_ERR_HIP, "hipMemset failed"));
    if (hipStreamSynchronize(p->stream) != hipSuccess) return bail(fail(BFGX_ERR_HIP, "stream sync failed"));
    *out = p;
    return BFGX_OK;
}

int bfgx_plan_timing_enable(bfgx_plan *p, int on)
{
    return p ? p->events.enable(on) : fail(BFGX_ERR_INVALID, "NULL plan");
}

int bfgx_plan_timing_read(bfgx_plan *p, double *ms_sum, int64_t *launches)
{
    return p ? p->events.read(p->device, p->stream, ms_sum, launches) : fail(BFGX_ERR_INVALID, "NULL argument");
}

void bfgx_plan_destroy(bfgx_plan *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    (void)hipStreamSynchronize(p->stream);
    p->events.destroy();
    p->mem.release();
    delete p;
}

int bfgx_plan_set_algo(bfgx_plan *p, int algo)
{
    if (!p || (algo != 0 && algo != 1)) return fail(BFGX_ERR_INVALID, "algo must be 0 (per-halo global atomics) or 1 (LDS tiles)");
    p->algo = algo;
    return BFGX_OK;
}

int bfgx_plan_status(bfgx_plan *p)
{
    if (!p) return fail(BFGX_ERR_INVALID, "NULL plan");
    HIP_TRY(hipSetDevice(p->device));
    int32_t ov = 0;
    HIP_TRY(hipMemcpyAsync(&ov, p->overflow, sizeof(ov), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (ov & 4) {
        // the fluid form of the fast kernel: a wave waited 2^22 sleeps for a tile slot / a flush / a staged tile of its own workgroup and
        // left (the grid drained); never seen outside fault injection
        HIP_TRY(hipMemsetAsync(p->overflow, 0, sizeof(int32_t), p->stream));
        return fail(BFGX_ERR_HIP, "tile_scatter2f_kernel: a wave gave up waiting inside its workgroup; results are incomplete (BFGX_K1_FLUID=0 selects the other form)");
    }
    if (ov) return fail(BFGX_ERR_INVALID, "halo->tile entry list overflowed its capacity (%lld); results are incomplete",
                        (long long)p->capacity);
    int32_t fov = 0;
    HIP_TRY(hipMemcpyAsync(&fov, p->far.overflow, sizeof(fov), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (fov) {
        HIP_TRY(hipMemsetAsync(p->far.overflow, 0, sizeof(int32_t), p->stream));
        return fail(BFGX_ERR_INVALID, "the regrid's list of far deposits overflowed (%lld entries): displacements of many pixels over a large "
                                      "part of the map", (long long)p->far.cap);
    }
    return BFGX_OK;
}

int bfgx_plan_precision(bfgx_plan *p, int acc_requested, int32_t *acc_resolved, double *table_disp_pixels)
{
    DispMode m;
    if (int rc = disp_mode(p, acc_requested, false, m)) return rc;
    if (acc_resolved) *acc_resolved = m.acc();
    if (table_disp_pixels) *table_disp_pixels = p->table_disp_pixels;
    return BFGX_OK;
}

// arguments of the gathering regrid that do not depend on the data
static ReachArgs reach_args(const bfgx_plan *p, double cap)
{
    const double ns = (double)p->hpx.nside, om = 1.0 / (3.0 * ns * ns);        // ring 1: z = 1 - 1 / (3 nside^2)
    const double th1 = std::atan2(std::sqrt(om * (2.0 - om)), 1.0 - om);
    return ReachArgs{p->tile_apron, cap, th1, 3.14159265358979323846 - th1};
}

// first pixel of ring `ring` (1 .. 4 nside - 1), npix beyond
static int64_t ring_first_pixel(const Hpx &h, int64_t ring)
{
    const int64_t ns = h.nside, nl4 = 4 * ns;
    if (ring < 1) return 0;
    if (ring >= nl4) return h.npix;
    const int64_t q = nl4 - ring;
    return (ring < ns) ? 2 * ring * (ring - 1) : (ring < 3 * ns) ? h.ncap + (ring - ns) * 4 * ns : h.npix - 2 * q * (q + 1);
}

// The bands [b0, b1) of the tiling as the launches take them: the RING pixels [p0, p1), the tiles [t0, t0 + nt).  Band b holds the rings
// [1 + BR b, 1 + BR (b + 1)); 0 <= b0 <= b1 <= nbands (check_band_range).  Nothing else reads band_tile0_host or turns a band into a pixel
struct BandRange { int64_t p0, p1; int t0, nt; };
static BandRange band_range(const bfgx_plan *p, int b0, int b1)
{
    const auto first_pixel = [p](int b) { return ring_first_pixel(p->hpx, 1 + (int64_t)p->tiling.BR * b); };
    return BandRange{first_pixel(b0), first_pixel(b1), p->band_tile0_host[b0], p->band_tile0_host[b1] - p->band_tile0_host[b0]};
}

static int check_band_range(const bfgx_plan *p, int32_t b0, int32_t b1, bool tiles = false)      // tiles: for a pass over the range's tiles
{
    if (tiles && p->algo != 1) return fail(BFGX_ERR_UNSUPPORTED, "band-restricted passes need the tiled algorithm (algo 1)");
    return (b0 < 0 || b1 > p->tiling.nbands || b0 > b1) ? fail(BFGX_ERR_INVALID, "band range out of bounds") : BFGX_OK;
}

// the checks of a K0 + K1 / K3 entry: the catalog, the kind of table (paint: a profile table), the output pointer.  bands: a pass over the tiles
// of bands [band0, band1) only; a rank that owns no band (more ranks than bands) passes the data pointer of an empty buffer, which is NULL
static int check_scatter(const bfgx_plan *p, const bfgx_catalog *cat, const void *out, bool paint, bool bands = false, int32_t band0 = 0, int32_t band1 = 0)
{
    if (int rc = check_catalog(p, cat)) return rc;
    if (bands) if (int rc = check_band_range(p, band0, band1, true)) return rc;
    if ((p->model.tab.logv != 0) != paint) return fail(BFGX_ERR_INVALID, paint ? "profile painting needs a table with log_values = 1"
                                                                               : "displacement read-out needs a table with log_values = 0");
    if ((!bands || band0 < band1) && !out) return fail(BFGX_ERR_INVALID, paint ? "map pointer is NULL" : "offsets pointer is NULL");
    return BFGX_OK;
}

// K0 ahead of K1 / K3: with the halo -> tile binning for the tiled algorithm (f64: fp64 pair records), the per-halo records otherwise
static int launch_k0(bfgx_plan *p, const bfgx_catalog *cat, int fallback4, bool f64)
{
    HIP_TRY(hipSetDevice(p->device));
    if (p->algo == 1) {
        if (int rc = launch_prep_and_bin(p, cat, fallback4, f64)) return rc;
        return p->blocking_growth ? ensure_entry_capacity(p, cat) : BFGX_OK;
    }
    if (p->NC != 4) return fail(BFGX_ERR_UNSUPPORTED, "tables with extra parameter axes need algo 1 (LDS tiles)");
    return launch_prep(p, cat, fallback4, false, false, true);
}

// K1 into the pixels [p0, p1) of pix_offsets held at `slice` in m's layout (the kernels index pixels by global number: virtual bases)
static int launch_offsets(bfgx_plan *p, const DispMode &m, void *slice, int64_t p0, int64_t p1, TileLaunch k1)
{
    if (m.split()) k1.offsets_lo = m.lo(slice, p1 - p0) - 3 * p0;
    if (m.kind != DispMode::F64) return launch_tile_scatter<MODE_OFFSETS, float>(p, (float *)slice - 3 * p0, k1);
    return launch_tile_scatter<MODE_OFFSETS, double>(p, (double *)slice - 3 * p0, k1);
}

// K0 + K1 into the whole sphere's pix_offsets
static int offsets_impl(bfgx_plan *p, const bfgx_catalog *cat, void *offsets_dev, const DispMode &m, const TileLaunch &k1)
{
    if (int rc = check_scatter(p, cat, offsets_dev, false)) return rc;
    if (int rc = launch_k0(p, cat, 1, m.fp64())) return rc;
    if (p->algo == 1) return launch_offsets(p, m, offsets_dev, 0, p->hpx.npix, k1);      // (every element is stored: no zero-fill needed)
    if (m.fp64()) return launch_scatter<MODE_OFFSETS, double>(p, cat->n, (double *)offsets_dev, nullptr);
    return launch_scatter<MODE_OFFSETS, float>(p, cat->n, (float *)offsets_dev, nullptr);
}

int bfgx_offsets_device(bfgx_plan *p, const bfgx_catalog *cat, void *offsets_dev, int acc_f64)
{
    DispMode m;
    if (int rc = disp_mode(p, acc_f64, false, m)) return rc;
    return offsets_impl(p, cat, offsets_dev, m, TileLaunch{});
}

// K3 into the map held at `slice` from pixel p0 on (virtual base: the kernels index the output by global pixel number)
static int launch_paint(bfgx_plan *p, const PaintMode &m, void *slice, int64_t p0, TileLaunch k3)
{
    k3.paint_pair_f32 = m.pair_f32();
    if (m.map_f64()) return launch_tile_scatter<MODE_PAINT, double>(p, (double *)slice - p0, k3);
    return launch_tile_scatter<MODE_PAINT, float>(p, (float *)slice - p0, k3);
}

int bfgx_max_offset2_device(bfgx_plan *p, const void *offsets_dev, int64_t npixels, int acc_f64, float *out_dev)
{
    if (!p || !out_dev || (npixels > 0 && !offsets_dev)) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (npixels < 0) return fail(BFGX_ERR_INVALID, "npixels < 0");
    DispMode m;
    if (int rc = disp_mode(p, acc_f64, true, m)) return rc;       // (the band entries' one array: BFGX_ACC_PARITY is read as fp64)
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemsetAsync(out_dev, 0, sizeof(float), p->stream));
    if (npixels > 0) {
        const unsigned grid = (unsigned)std::min<int64_t>((npixels + 255) / 256, 1024);
        if (m.fp64()) hipLaunchKernelGGL(max_offset_kernel<double>, dim3(grid), dim3(256), 0, p->stream, npixels, (const double *)offsets_dev, (unsigned *)out_dev);
        else hipLaunchKernelGGL(max_offset_kernel<float>, dim3(grid), dim3(256), 0, p->stream, npixels, (const float *)offsets_dev, (unsigned *)out_dev);
        HIP_TRY(hipGetLastError());
    }
    return BFGX_OK;
}

// the catalogs of the following K0 launches are BLOCKED: rows halo j's columns at (j / rows) * stride + (j % rows) from the column pointers (what
// an all_to_all of fixed-capacity blocks [block][column][rows] delivers: stride = ncols * rows); rows = 0: plain columns again
int bfgx_plan_set_catalog_blocks(bfgx_plan *p, int64_t rows, int64_t stride)
{
    if (!p) return fail(BFGX_ERR_INVALID, "NULL plan");
    if (rows < 0 || (rows > 0 && stride < rows)) return fail(BFGX_ERR_INVALID, "blocked catalog: rows >= 0, stride >= rows");
    p->cat_blk_rows = rows; p->cat_blk_stride = rows > 0 ? stride : 0;
    return BFGX_OK;
}

int bfgx_plan_tile_shape(bfgx_plan *p, int32_t *rings_per_band, int32_t *max_columns)
{
    if (!p) return fail(BFGX_ERR_INVALID, "NULL plan");
    if (rings_per_band) *rings_per_band = p->tiling.BR;
    if (max_columns) *max_columns = p->tiling.W;
    return BFGX_OK;
}

// K0 + K3 over the whole sphere
static int paint_impl(bfgx_plan *p, const bfgx_catalog *cat, void *map_out_dev, const PaintMode &m)
{
    if (int rc = check_scatter(p, cat, map_out_dev, true)) return rc;
    if (int rc = launch_k0(p, cat, 0, m.k0_f64())) return rc;
    if (p->algo == 1) return launch_paint(p, m, map_out_dev, 0, TileLaunch{});
    if (m.map_f64()) return launch_scatter<MODE_PAINT, double>(p, cat->n, (double *)map_out_dev, nullptr);
    return launch_scatter<MODE_PAINT, float>(p, cat->n, (float *)map_out_dev, nullptr);
}

int bfgx_paint_device(bfgx_plan *p, const bfgx_catalog *cat, void *map_out_dev, int acc_f64)
{
    PaintMode m;
    if (int rc = paint_mode(p, acc_f64, m)) return rc;
    return paint_impl(p, cat, map_out_dev, m);
}

}  // extern "C"

// The two sums of the mass check from the per-tile sums of the tiles [t0, t0 + nt): added up by one workgroup, or -- above kSumTilesOneWg
// tiles, where that single workgroup's loop takes 0.2 - 0.6 ms -- by 64 workgroups into the zeroed sums; the deposit totals the far-pixel
// evaluator left behind the per-tile sums go in with them.  The caller checks the launch
constexpr int kSumTilesOneWg = 16384;
static int launch_tile_sums(bfgx_plan *p, int t0, int nt, double *sums_dev)
{
    const double *ts = p->tile_sums + 2 * (size_t)t0;
    const double *fs = p->far_src.sums;
    if (nt <= kSumTilesOneWg) hipLaunchKernelGGL(sum_tiles_kernel, dim3(1), dim3(256), 0, p->stream, nt, ts, sums_dev, fs, kFarEvalWgs);
    else {
        HIP_TRY(hipMemsetAsync(sums_dev, 0, 2 * sizeof(double), p->stream));
        hipLaunchKernelGGL(sum_tiles_multi_kernel, dim3(64), dim3(256), 0, p->stream, nt, ts, sums_dev, fs, kFarEvalWgs);
    }
    return BFGX_OK;
}

// the gathering regrid (algo 1): [largest |offset|^2 per tile unless K1 left it], aprons, lean gather, gather with the ring
// walk over the tiles that need it, the generic route of the pixels those two listed, far list / repair
template <typename ACC, typename real, bool SPLIT = false>
static void launch_regrid_gather(bfgx_plan *p, const double *map_in_dev, const ACC *o, const ACC *o_lo, double *map_out_dev, double *ts, bool from_k1, double *sums_dev)
{
    const size_t lds = regrid3_lds_bytes(p->tiling.BR, p->tiling.W, sizeof(real)),
                 lds_walk = regrid3_lds_bytes(p->tiling.BR, p->tiling.W, sizeof(real), true, SPLIT ? sizeof(ACC) : sizeof(real));
    FarList far = p->far;
    far.overflow = p->arena.far_overflow_full;
    const int nt = p->tiling.ntiles, nfix = std::min(nt, 2 * p->num_cus), nwalk = std::min(nt, 4 * p->num_cus);
    const ReachArgs reach = reach_args(p, regrid_cap(p->hpx.nside));
    if (!from_k1)
        hipLaunchKernelGGL(tile_reach_kernel<ACC>, dim3(nt), dim3(256), 0, p->stream, p->hpx, p->tiling, o, p->arena.omax);
    hipLaunchKernelGGL(tile_apron_kernel, dim3((nt + 255) / 256), dim3(256), 0, p->stream, p->hpx, p->tiling, (const float *)p->arena.omax, 0,
                       reach.cap, 0, nt, p->tile_apron, p->arena.todo, p->regrid_lean);
    // (the lean kernel: a persistent grid over the tiles whose reach is one ring -- all of them on a table of sub-pixel moves, none on the S19 table)
    hipLaunchKernelGGL((tile_regrid3_kernel<ACC, real, 0, SPLIT>), dim3(std::min(nt, 8 * p->num_cus)), dim3(256), lds, p->stream, p->hpx, p->tiling, map_in_dev, o, o_lo,
                       map_out_dev, far, p->far_src, reach, ts, -1, nt, p->regrid_lean, (double *)nullptr);
    hipLaunchKernelGGL((tile_regrid3_kernel<ACC, real, 2, SPLIT>), dim3(nwalk), dim3(256), lds_walk, p->stream, p->hpx, p->tiling, map_in_dev, o, o_lo,
                       map_out_dev, far, p->far_src, reach, ts, -1, nt, p->arena.todo, (double *)nullptr);
    hipLaunchKernelGGL((regrid_far_eval_kernel<ACC, SPLIT>), dim3(kFarEvalWgs), dim3(256), 0, p->stream, p->hpx, p->tiling.rings, map_in_dev, o, o_lo, p->far_src, far);
    // the two sums of the mass check (ts: the plan's per-tile sums): added up by the last launch, or -- too many tiles for its one
    // workgroup -- by launch_tile_sums afterwards (regrid_impl checks the launches)
    const bool many = nt > kSumTilesOneWg && sums_dev != nullptr && ts != nullptr;
    hipLaunchKernelGGL((tile_regrid3_kernel<ACC, real, 1, SPLIT>), dim3(nfix), dim3(256), lds, p->stream, p->hpx, p->tiling, map_in_dev, o, o_lo,
                       map_out_dev, far, p->far_src, reach, ts, -1, nt, p->arena.todo, many ? (double *)nullptr : sums_dev, p->regrid_lean);
    if (many) (void)launch_tile_sums(p, 0, nt, sums_dev);
}

extern "C" {

static int regrid_impl(bfgx_plan *p, const double *map_in_dev, const void *offsets_dev, const DispMode &m, double *map_out_dev, double *sums_dev,
                       bool from_k1)
{
    HIP_TRY(hipSetDevice(p->device));
    {
    KernelTimer kt(p, BFGX_K_REGRID);
    if (p->algo == 1) {
        // gathering form: every output pixel is stored once by the tile that owns it (no atomics, no zero-fill needed);
        // the few deposits that need the generic route are listed and added afterwards
        // the control words (the fused call's binning step has zeroed them with its counters)
        if (!from_k1) HIP_TRY(hipMemsetAsync(p->arena.ctrl, 0, sizeof(RegridCtrl), p->stream));
        double *ts = sums_dev ? p->tile_sums : nullptr;
        if (m.split())      // pix_offsets as two fp32 arrays (hi, then lo behind the npix high triples), fp64 geometry
            launch_regrid_gather<float, double, true>(p, map_in_dev, (const float *)offsets_dev, m.lo(offsets_dev, p->hpx.npix),
                                                      map_out_dev, ts, from_k1, sums_dev);
        else if (m.fp64()) launch_regrid_gather<double, double>(p, map_in_dev, (const double *)offsets_dev, (const double *)nullptr, map_out_dev, ts, from_k1, sums_dev);
        else launch_regrid_gather<float, float>(p, map_in_dev, (const float *)offsets_dev, (const float *)nullptr, map_out_dev, ts, from_k1, sums_dev);
    } else {
        const unsigned grid = (unsigned)((p->hpx.npix + 255) / 256);
        if (m.fp64())
            hipLaunchKernelGGL(regrid_kernel<double>, dim3(grid), dim3(256), 0, p->stream, p->hpx, map_in_dev,
                               (const double *)offsets_dev, map_out_dev);
        else
            hipLaunchKernelGGL(regrid_kernel<float>, dim3(grid), dim3(256), 0, p->stream, p->hpx, map_in_dev,
                               (const float *)offsets_dev, map_out_dev);
    }
    }
    HIP_TRY(hipGetLastError());
    if (sums_dev) {
        // algo 1: the gather kernels left per-tile {sum of source values, sum of deposits} and the regrid's last launch added them up
        if (p->algo != 1) {
            KernelTimer kt(p, BFGX_K_SUM);
            HIP_TRY(hipMemsetAsync(sums_dev, 0, 2 * sizeof(double), p->stream));
            hipLaunchKernelGGL(sum2_kernel, dim3(1024), dim3(256), 0, p->stream, p->hpx.npix, map_in_dev,
                               (const double *)map_out_dev, sums_dev);
            HIP_TRY(hipGetLastError());
        }
    }
    return BFGX_OK;
}

int bfgx_regrid_device(bfgx_plan *p, const double *map_in_dev, const void *offsets_dev, int acc_f64,
                       double *map_out_dev, double *sums_dev)
{
    if (!p || !map_in_dev || !offsets_dev || !map_out_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    DispMode m;
    if (int rc = disp_mode(p, acc_f64, false, m)) return rc;
    return regrid_impl(p, map_in_dev, offsets_dev, m, map_out_dev, sums_dev, false);
}

int bfgx_baryonify_device(bfgx_plan *p, const bfgx_catalog *cat, const double *map_in_dev, void *offsets_work_dev, int acc_f64,
                          double *map_out_dev, double *sums_dev)
{
    if (!p || !map_in_dev || !offsets_work_dev || !map_out_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    DispMode m;
    if (int rc = disp_mode(p, acc_f64, false, m)) return rc;
    TileLaunch k1;
    const bool fused = p->algo == 1;         // K1's flush leaves the largest |offset|^2 of every tile for the regrid's aprons
    if (fused) k1.omax = p->arena.omax;
    if (int rc = offsets_impl(p, cat, offsets_work_dev, m, k1)) return rc;
    return regrid_impl(p, map_in_dev, offsets_work_dev, m, map_out_dev, sums_dev, fused);
}

int bfgx_count_pairs_device(bfgx_plan *p, const bfgx_catalog *cat, int fallback4, int64_t *counts_dev, int64_t *total_host)
{
    if (int rc = check_catalog(p, cat)) return rc;
    HIP_TRY(hipSetDevice(p->device));
    if (p->algo == 1 && !counts_dev) {       // census through the tile path (checks the binning is complete)
        HIP_TRY(hipMemsetAsync(p->pair_total, 0, sizeof(unsigned long long), p->stream));
        if (int rc = launch_prep_and_bin(p, cat, fallback4, false)) return rc;
        if (int rc = launch_tile_scatter<MODE_COUNT, float>(p, (float *)nullptr, TileLaunch{})) return rc;
        unsigned long long tot = 0;
        HIP_TRY(hipMemcpyAsync(&tot, p->pair_total, sizeof(tot), hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        if (total_host) *total_host = (int64_t)tot;
        return bfgx_plan_status(p);
    }
    int64_t *counts = counts_dev;
    DevBuf tmp;
    if (!counts) {
        HIP_TRY(tmp.alloc(sizeof(int64_t) * (size_t)(cat->n > 0 ? cat->n : 1)));
        counts = tmp.as<int64_t>();
    }
    int rc = launch_prep(p, cat, fallback4, false, false, true);
    if (!rc) rc = launch_scatter<MODE_COUNT, float>(p, cat->n, (float *)nullptr, counts);
    if (!rc && total_host) {
        std::vector<int64_t> h((size_t)cat->n);
        if (hipMemcpyAsync(h.data(), counts, sizeof(int64_t) * (size_t)cat->n, hipMemcpyDeviceToHost, p->stream) != hipSuccess ||
            hipStreamSynchronize(p->stream) != hipSuccess)
            rc = fail(BFGX_ERR_HIP, "count copy-back failed");
        else {
            int64_t tot = 0;
            for (int64_t v : h) tot += v;
            *total_host = tot;
        }
    } else if (!rc) {
        if (hipStreamSynchronize(p->stream) != hipSuccess) rc = fail(BFGX_ERR_HIP, "stream sync failed");
    }
    return rc;
}

}  // extern "C"

// ------------------------------------------------------------------------------ the banded (multi-GPU) passes, the far-deposit list
#include "bfgx_shell_bands.inc"

// ------------------------------------------------------------------------------ halo routing between ranks
#include "bfgx_route_api.inc"

// ------------------------------------------------------------------------------ one-shot host API
#include "bfgx_oneshot.hpp"

namespace {

constexpr int kCatCols = 4 + BFGX_MAX_EXTRA + 2;       // M, z, ra, dec, extra[2], ln1pz, lnM
// column i of them travels for a table with nex extra parameter axes (the extra[] beyond nex stay NULL)
constexpr bool catalog_col_used(int i, int nex) { return i < 4 + nex || i >= 4 + BFGX_MAX_EXTRA; }

// the host columns of a catalog in upload order (M, z, ra, dec, extra[], ln1pz, lnM).  The (z, M) table coordinates are the caller's numpy
// values when given, else libm on the host here (never the device's log: README.md:78-80 puts table edges exactly on the catalog's min/max)
int catalog_columns(const bfgx_catalog *h, int nex, std::vector<double> &hostlog, const double *src[kCatCols])
{
    const double *lnz = h->ln1pz, *lnm = h->lnM;
    if (h->n > 0 && (!lnz || !lnm)) {
        if (!h->M || !h->z) return fail(BFGX_ERR_INVALID, "catalog column pointer is NULL");
        hostlog.resize(2 * (size_t)h->n);
        for (int64_t i = 0; i < h->n; ++i) {
            const double a = 1.0 / (1.0 + h->z[i]);                          // HealpixRunner.py:295
            hostlog[i] = std::log(1.0 / a);                                  // BaryonCorrection.py:364
            hostlog[(size_t)h->n + i] = std::log(h->M[i]);                   // :369
        }
        if (!lnz) lnz = hostlog.data();
        if (!lnm) lnm = hostlog.data() + h->n;
    }
    src[0] = h->M; src[1] = h->z; src[2] = h->ra; src[3] = h->dec;
    for (int k = 0; k < BFGX_MAX_EXTRA; ++k) src[4 + k] = k < nex ? h->extra[k] : nullptr;
    src[4 + BFGX_MAX_EXTRA] = lnz; src[5 + BFGX_MAX_EXTRA] = lnm;
    for (int i = 0; i < kCatCols; ++i)
        if (catalog_col_used(i, nex) && h->n > 0 && !src[i]) return fail(BFGX_ERR_INVALID, "catalog column pointer is NULL");
    return BFGX_OK;
}

// the device catalog of n halos whose columns (upload order) are at col[]
void catalog_view(int64_t n, int nex, const double *const col[kCatCols], bfgx_catalog *d)
{
    std::memset(d, 0, sizeof(*d));
    d->n = n;
    d->M = col[0]; d->z = col[1]; d->ra = col[2]; d->dec = col[3];
    for (int k = 0; k < nex; ++k) d->extra[k] = col[4 + k];
    d->ln1pz = col[4 + BFGX_MAX_EXTRA]; d->lnM = col[5 + BFGX_MAX_EXTRA];
}

// the used columns of a host catalog -> cols[] on the plan's stream, *d their device view; size(buffer, bytes) != 0: no memory
template <class Buf, class Size>
int upload_catalog_columns(bfgx_plan *p, const bfgx_catalog *h, Buf cols[kCatCols], Size size, bfgx_catalog *d, std::vector<double> &hostlog)
{
    const int nex = p->model.tab.ndim - 3;
    const double *src[kCatCols], *dp[kCatCols] = {};
    if (int rc = catalog_columns(h, nex, hostlog, src)) return rc;
    for (int i = 0; i < kCatCols; ++i) {
        if (!catalog_col_used(i, nex)) continue;
        if (size(cols[i], sizeof(double) * (size_t)h->n)) return alloc_fail("catalog");
        if (h->n > 0) HIP_TRY(hipMemcpyAsync(cols[i].p, src[i], sizeof(double) * (size_t)h->n, hipMemcpyHostToDevice, p->stream));
        dp[i] = (const double *)cols[i].p;
    }
    catalog_view(h->n, nex, dp, d);
    return BFGX_OK;
}

// into buffers of the exact size that the caller's handle owns
int upload_catalog(bfgx_plan *p, const bfgx_catalog *h, DevBuf cols[kCatCols], bfgx_catalog *d, std::vector<double> &hostlog)
{
    return upload_catalog_columns(p, h, cols, [](DevBuf &b, size_t bytes) { return b.alloc(bytes) != hipSuccess; }, d, hostlog);
}

struct ShellEntry : CacheEntry<bfgx_plan> {
    PoolBuf cols[kCatCols], in, out, off, sums;
    // the catalog columns of the last call stay on the device under the caller's token (bfgx_opts.catalog_token)
    uint64_t cat_token = 0;
    int64_t cat_n = -1;
    bfgx_catalog cat_dev;
};
PlanCache<ShellEntry, 4> g_shells;

std::atomic<long long> g_catalog_uploads{0};

int upload_catalog_pooled(ShellEntry *e, const bfgx_catalog *h, bfgx_catalog *d, std::vector<double> &hostlog, uint64_t token)
{
    if (token != 0 && token == e->cat_token && h->n == e->cat_n) {      // the same catalog as last time: its columns are still there
        *d = e->cat_dev;
        return BFGX_OK;
    }
    e->cat_token = 0;
    g_catalog_uploads.fetch_add(1);
    auto size = [](PoolBuf &b, size_t bytes) { return b.need(std::max(bytes, sizeof(double))); };      // (an empty catalog: one element per column)
    if (int rc = upload_catalog_columns(e->plan, h, e->cols, size, d, hostlog)) return rc;
    // (the copies above are from pageable memory: they have left the host buffers when hipMemcpyAsync returns)
    e->cat_token = token; e->cat_n = h->n; e->cat_dev = *d;
    return BFGX_OK;
}

// the start of a one-shot entry (g_shells.mu held): the cached plan for (device, nside, model) set to o.algo
int shell_begin(const bfgx_catalog *cat, const bfgx_model *model, int64_t nside, const bfgx_opts &o, ShellEntry **e)
{
    if (o.algo != 0 && o.algo != 1) return fail(BFGX_ERR_INVALID, "opts.algo must be 0 or 1");
    if (cat->n < 0) return fail(BFGX_ERR_INVALID, "catalog size < 0");
    if (int rc = validate_model(model)) return rc;           // before hashing: the table pointers must be readable
    CacheKey key = model_key(o.device, model);
    key.add(nside);
    auto make = [&](int64_t cap, bfgx_plan **p) -> int {
        if (int rc = bfgx_plan_create(o.device, nullptr, nside, cap, model, p)) return rc;
        (*p)->blocking_growth = true;
        return BFGX_OK;
    };
    if (int rc = g_shells.acquire(key, o.device, cat->n, make, [](ShellEntry *) -> int { return BFGX_OK; }, e)) return rc;
    (*e)->plan->algo = o.algo;
    return BFGX_OK;
}

// Large maps travel in band ranges (contiguous RING pixel ranges) of at least 16 MB (8 ranges of 12.6 MB: 4.0 ms per call, 6 of 16.8 MB: 3.3 ms),
// at most kChunksMax.  BFGX_PIPE_CHUNKS sets the count (tests: small maps, through a staging buffer), BFGX_NO_PIPELINE sends every call down one pass.
constexpr int kChunksMax = 16;
struct Chunks {
    int n = 0;
    bool piped = false, stage = false;
    int cb[kChunksMax + 1] = {};     // first band of every range, then nbands
    std::vector<int64_t> bfp;        // first pixel of every band, then npix
};

void chunk_plan(bfgx_plan *p, bool eligible, const PipeKnobs &knobs, Chunks &c)
{
    const size_t npix = (size_t)p->hpx.npix;
    c.n = (int)std::min<size_t>(kChunksMax, npix * sizeof(double) / ((size_t)16 << 20));
    if (knobs.stage) c.n = std::max(2, std::min(kChunksMax, knobs.chunks));
    c.stage = knobs.stage;
    c.piped = eligible && c.n >= 2 && p->tiling.nbands >= 2 * c.n && !knobs.off;
    if (!c.piped) return;
    int nb = 0;
    c.bfp.resize((size_t)p->tiling.nbands + 1);
    (void)bfgx_plan_bands(p, &nb, c.bfp.data());
    c.cb[0] = 0; c.cb[c.n] = nb;
    for (int k = 1; k < c.n; ++k) {
        const int64_t target = (int64_t)(npix * (size_t)k / c.n);
        const int b = (int)(std::lower_bound(c.bfp.begin(), c.bfp.end(), target) - c.bfp.begin());
        c.cb[k] = std::min(std::max(b, c.cb[k - 1] + 1), nb - (c.n - k));
    }
}

constexpr int kOnePass = 1;          // what a streamed route returns (no BFGX_ERR_*: those are negative) to send the call down the one-pass route

// The streamed route of bfgx_baryonify_shell.  Large maps travel in band ranges (chunk_plan): a range is regridded as soon as it and its apron
// have arrived and goes back to the host while the next ones are still coming in, so that the two directions of the link work at the same
// time.  The gathering regrid stores every pixel of a range exactly once; the few deposits it cannot gather (next to a pole) are listed and
// added on the host.  Both host buffers are page-locked for the duration of the call (hipHostRegister: 2 us here) -- from pageable memory
// the copies in and out take turns on the host thread and the one-pass route is faster (4.3 against 4.5 ms), which is also where a map
// goes that cannot be registered.  *first_unsent: the first pixel of the map that has not been uploaded (npix: all of it is on its way).
int shell_streamed(OneShotCall &call, ShellEntry *e, const DispMode &m, const Chunks &ch, double sums[2], int64_t *first_unsent)
{
    bfgx_plan *p = e->plan;
    const int64_t npix = p->hpx.npix;
    const int kChunks = ch.n, *cb = ch.cb;
    const std::vector<int64_t> &bfp = ch.bfp;
    const double *map_in = call.src<double>(); double *map_out = call.dst<double>();
    if (int rc = e->pools(kChunks, kChunks)) return rc;
    if (e->sums.need((2 * kChunks + 2) * sizeof(double))) return alloc_fail("sums");
    double *dsums = (double *)e->sums.p;
    float *domax = (float *)(dsums + 2 * kChunks);
    int sent = 0;
    auto send = [&]() -> int {                           // the next range
        const int64_t lo = bfp[cb[sent]], n = bfp[cb[sent + 1]] - lo;
        HIP_TRY(hipMemcpyAsync((double *)e->in.p + lo, map_in + lo, (size_t)n * sizeof(double), hipMemcpyHostToDevice, e->up));
        HIP_TRY(hipEventRecord(e->ev_up[sent], e->up));
        *first_unsent = bfp[cb[++sent]];
        return BFGX_OK;
    };
    if (int rc = send()) return rc;
    if (int rc = send()) return rc;
    // how many rings a deposit travels: from the largest displacement K1 has seen (by now K1 has finished underneath the two copies)
    float m2 = 0.0f;
    if (int rc = bfgx_bands_max_offset2_device(p, 0, p->tiling.nbands, domax)) return rc;
    HIP_TRY(hipMemcpyAsync(&m2, domax, sizeof(float), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    int32_t rings = kReachMax;
    if (std::isfinite(m2)) { if (int rc = bfgx_plan_reach_rings(p, std::sqrt((double)m2), &rings)) return rc; }
    if (rings > 4) return kOnePass;                      // large displacements: the data-sized aprons and the in-stream repair of regrid_impl
    Restore<int> reach{p->band_reach, p->band_reach};
    p->band_reach = rings;
    int next = 0;
    auto run_ready = [&]() -> int {                      // regrid every range whose apron lies within the ranges sent so far
        while (next < kChunks) {
            int64_t olo = 0, ohi = 0;
            if (int rc = bfgx_plan_band_apron(p, cb[next], cb[next + 1], &olo, &ohi)) return rc;
            int need = next;
            while (need < kChunks - 1 && bfp[cb[need + 1]] < ohi) ++need;
            if (need >= sent) break;
            HIP_TRY(hipStreamWaitEvent(p->stream, e->ev_up[need], 0));
            const int64_t lo = bfp[cb[next]], n = bfp[cb[next + 1]] - lo;
            if (int rc = regrid_bands_impl(p, cb[next], cb[next + 1], (const double *)e->in.p, e->off.p, 0, npix, m,
                                           (double *)e->out.p + lo, dsums + 2 * next, next == 0)) return rc;
            HIP_TRY(hipEventRecord(e->ev_k[next], p->stream));
            HIP_TRY(hipStreamWaitEvent(e->down, e->ev_k[next], 0));
            HIP_TRY(hipMemcpyAsync(map_out + lo, (double *)e->out.p + lo, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, e->down));
            ++next;
        }
        return BFGX_OK;
    };
    int rc = run_ready();
    while (rc == BFGX_OK && sent < kChunks) {
        rc = send();
        if (rc == BFGX_OK) rc = run_ready();
    }
    if (rc) return rc;                                   // (what is in flight is drained by the call scope)
    if ((rc = call.mark(1, e->up)) || (rc = call.mark(2, p->stream))) return rc;
    double hs[2 * kChunksMax];
    HIP_TRY(hipMemcpyAsync(hs, dsums, sizeof(double) * 2 * (size_t)kChunks, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    HIP_TRY(hipStreamSynchronize(e->down));
    if ((rc = call.mark(3, p->stream))) return rc;
    for (int c = 0; c < kChunks; ++c) { sums[0] += hs[2 * c]; sums[1] += hs[2 * c + 1]; }
    // the listed deposits (pixels next to a pole): added on the host; an overflowing list sends the call down the one-pass route
    int64_t nfar = 0;
    if (bfgx_plan_far_fetch(p, 0, nullptr, nullptr, &nfar) != BFGX_OK) return kOnePass;
    if (nfar > 0) {
        std::vector<int64_t> fp((size_t)nfar);
        std::vector<double> fv((size_t)nfar);
        if (int rc = bfgx_plan_far_fetch(p, nfar, fp.data(), fv.data(), &nfar)) return rc;
        for (int64_t i = 0; i < nfar; ++i) if (fp[(size_t)i] >= 0 && fp[(size_t)i] < npix) map_out[fp[(size_t)i]] += fv[(size_t)i];
    }
    return BFGX_OK;
}

// The one-pass route of bfgx_baryonify_shell: what is left of the map goes up on a second stream (a copy from pageable memory occupies the
// host, K0 + K1 run meanwhile), K2 after both, the map -> host
int shell_one_pass(OneShotCall &call, ShellEntry *e, const DispMode &m, bool tiled, const double *map_in, double *map_out, int64_t first_unsent, double sums[2])
{
    bfgx_plan *p = e->plan;
    const size_t npix = (size_t)p->hpx.npix, lo = (size_t)first_unsent;
    if (lo < npix) HIP_TRY(hipMemcpyAsync((double *)e->in.p + lo, map_in + lo, (npix - lo) * sizeof(double), hipMemcpyHostToDevice, e->up));
    if (int rc = call.mark(1, e->up)) return rc;
    HIP_TRY(hipStreamWaitEvent(p->stream, e->ev[1], 0));
    if (int rc = regrid_impl(p, (const double *)e->in.p, e->off.p, m, (double *)e->out.p, (double *)e->sums.p, tiled)) return rc;
    if (int rc = call.mark(2, p->stream)) return rc;
    HIP_TRY(hipMemcpyAsync(map_out, e->out.p, npix * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipMemcpyAsync(sums, e->sums.p, 2 * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    if (int rc = call.mark(3, p->stream)) return rc;
    HIP_TRY(hipStreamSynchronize(p->stream));
    return BFGX_OK;
}

// The streamed route of bfgx_paint_shell: large fp64 maps are painted in band ranges (chunk_plan), each copied back while the next ones
// are painted (map_out page-locked for the call); K0 runs once, K3 on the tiles of each range
int paint_streamed(ShellEntry *e, const bfgx_catalog *dcat, const PaintMode &m, const Chunks &ch, double *map_out)
{
    bfgx_plan *p = e->plan;
    if (int rc = check_scatter(p, dcat, e->out.p, true)) return rc;
    if (int rc = e->pools(ch.n, ch.n)) return rc;
    if (int rc = launch_k0(p, dcat, 0, m.k0_f64())) return rc;
    TileLaunch k3;
    k3.paint_pair_f32 = m.pair_f32();
    k3.spread_tiles = p->tiling.ntiles;                  // K0 has binned the WHOLE catalog; every range launch sees the same density (ADVICE, round 4)
    for (int c = 0; c < ch.n; ++c) {
        const BandRange r = band_range(p, ch.cb[c], ch.cb[c + 1]);
        k3.tile_lo = r.t0; k3.tile_n = r.nt;
        // (the persistent kernel draws its tiles from a counter that the binning step zeroes: once more for every further launch)
        if (c > 0) HIP_TRY(hipMemsetAsync(p->arena.tile_counter, 0, sizeof(unsigned int), p->stream));
        if (int rc = launch_tile_scatter<MODE_PAINT, double>(p, (double *)e->out.p, k3)) return rc;      // (indexed by global pixel number)
        HIP_TRY(hipEventRecord(e->ev_k[c], p->stream));
        HIP_TRY(hipStreamWaitEvent(e->down, e->ev_k[c], 0));
        HIP_TRY(hipMemcpyAsync(map_out + r.p0, (double *)e->out.p + r.p0, (size_t)(r.p1 - r.p0) * sizeof(double), hipMemcpyDeviceToHost, e->down));
    }
    return BFGX_OK;
}

}  // namespace

extern "C" {

long long bfgx_debug_catalog_uploads(void) { return g_catalog_uploads.load(); }

void bfgx_debug_host_spans(long long *pinned_in_place, long long *staged, long long *smallest_pinned_bytes)
{
    if (pinned_in_place) *pinned_in_place = g_host_pinned_in_place.load();
    if (staged) *staged = g_host_staged.load();
    if (smallest_pinned_bytes) *smallest_pinned_bytes = g_host_pin_min_bytes.load();
}

long long bfgx_debug_alloc_count(void) { return (long long)g_dev_allocs.load(); }
long long bfgx_debug_live_allocs(void) { return (long long)g_dev_live.load(); }

int bfgx_debug_ring_table(bfgx_plan *p, int from_functions, int64_t first, int64_t count, void *out)
{
    if (!p || !out) return fail(BFGX_ERR_INVALID, "NULL argument");
    const int64_t nl4 = 4 * p->hpx.nside;
    // (the functions are defined for rings 1 .. 4 nside - 1; the table also holds the two "no such ring" records)
    const int64_t lo = from_functions ? 1 : 0, hi = from_functions ? nl4 - 1 : nl4;
    if (count < 0 || first < lo || first + count - 1 > hi) return fail(BFGX_ERR_INVALID, "ring table: rings [%lld, %lld] only", (long long)lo, (long long)hi);
    if (count == 0) return BFGX_OK;
    HIP_TRY(hipSetDevice(p->device));
    const RingRec *src = p->tiling.rings + first;
    DevBuf tmp;
    if (from_functions) {
        if (tmp.alloc(sizeof(RingRec) * (size_t)count)) return alloc_fail("ring records");
        hipLaunchKernelGGL(ring_functions_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, p->stream, p->hpx, (int)first, (int)count, tmp.as<RingRec>());
        HIP_TRY(hipGetLastError());
        src = tmp.as<RingRec>();
    }
    HIP_TRY(hipMemcpyAsync(out, src, sizeof(RingRec) * (size_t)count, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return BFGX_OK;
}

int bfgx_host_alloc(size_t bytes, void **out)
{
    if (!out) return fail(BFGX_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (bfgx_device_count() <= 0) return fail(BFGX_ERR_NO_DEVICE, "no HIP device visible");
    HIP_TRY(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return BFGX_OK;
}

void bfgx_host_free(void *p) { if (p) (void)hipHostFree(p); }

int bfgx_baryonify_shell(const bfgx_catalog *cat, const bfgx_model *model, int64_t nside,
                         const double *map_in, double *map_out, const bfgx_opts *opts, bfgx_stats *stats)
{
    if (!cat || !model || !map_in || !map_out) return fail(BFGX_ERR_INVALID, "NULL argument");
    const bfgx_opts o = entry_opts(opts);
    std::lock_guard<std::mutex> lk(g_shells.mu);             // one shell call at a time (they share the cached plans)
    ShellEntry *e = nullptr;
    if (int rc = shell_begin(cat, model, nside, o, &e)) return rc;
    bfgx_plan *p = e->plan;
    OneShotCall call(&p->stream, e);
    const size_t npix = (size_t)p->hpx.npix;
    DispMode m;
    if (int rc = disp_mode(p, o.acc_offsets_f64, false, m)) return rc;      // (BFGX_ACC_AUTO: what the plan chose from the model's table)
    const size_t acc_bytes = npix * m.pixel_bytes();
    std::vector<double> hostlog;
    bfgx_catalog dcat;
    // phases: catalog -> device, K0 + K1 launched (enqueue-only), THEN the map -> device (in ranges, or in one piece on a second stream), K2, map -> host
    if (int rc = call.mark(0, p->stream)) return rc;
    if (int rc = upload_catalog_pooled(e, cat, &dcat, hostlog, o.catalog_token)) return rc;
    if (e->in.need(npix * sizeof(double)) || e->out.need(npix * sizeof(double)) || e->off.need(acc_bytes) || e->sums.need(40 * sizeof(double)))
        return alloc_fail("map buffers");
    if (o.algo == 0) {                                       // global-atomic kernels accumulate; the tiled ones store every element once
        HIP_TRY(hipMemsetAsync(e->off.p, 0, acc_bytes, p->stream));
        HIP_TRY(hipMemsetAsync(e->out.p, 0, npix * sizeof(double), p->stream));
    }
    TileLaunch k1;
    if (o.algo == 1) k1.omax = p->arena.omax;                 // K1's flush leaves the largest |offset|^2 of every tile for K2's aprons
    if (int rc = offsets_impl(p, &dcat, e->off.p, m, k1)) return rc;
    double sums[2] = {0, 0};
    Chunks ch;
    chunk_plan(p, o.algo == 1, pipe_knobs(), ch);
    int64_t first_unsent = 0;
    int rc = kOnePass;
    if (ch.piped && call.open(map_in, npix * sizeof(double), map_out, npix * sizeof(double), ch.stage)) {
        map_in = call.src<double>(); map_out = call.dst<double>();       // (from here on: the page-locked views)
        rc = shell_streamed(call, e, m, ch, sums, &first_unsent);
    }
    if (rc == kOnePass) rc = shell_one_pass(call, e, m, o.algo == 1, map_in, map_out, first_unsent, sums);
    if (rc) return rc;
    if (int rc = bfgx_plan_status(p)) return rc;             // far-deposit list / entry list
    call.commit();
    if (int rc = call.finish(stats, sums, -1)) return rc;
    return o.check_mass ? check_mass(sums[0], sums[1]) : BFGX_OK;
}

int bfgx_paint_shell(const bfgx_catalog *cat, const bfgx_model *model, int64_t nside,
                     double *map_out, const bfgx_opts *opts, bfgx_stats *stats)
{
    if (!cat || !model || !map_out) return fail(BFGX_ERR_INVALID, "NULL argument");
    const bfgx_opts o = entry_opts(opts);
    std::lock_guard<std::mutex> lk(g_shells.mu);
    ShellEntry *e = nullptr;
    if (int rc = shell_begin(cat, model, nside, o, &e)) return rc;
    bfgx_plan *p = e->plan;
    OneShotCall call(&p->stream, e);
    PaintMode m;
    if (int rc = paint_mode(p, o.acc_paint_f64, m)) return rc;

    const size_t npix = (size_t)p->hpx.npix;
    std::vector<double> hostlog;
    bfgx_catalog dcat;
    Timer t;
    t.start(p->stream);
    if (int rc = upload_catalog_pooled(e, cat, &dcat, hostlog, o.catalog_token)) return rc;
    if (e->out.need(npix * sizeof(double))) return alloc_fail("map");
    const double ms_h2d = t.lap(p->stream);
    Chunks ch;
    chunk_plan(p, o.algo == 1 && m.map_f64(), pipe_knobs(), ch);
    double ms_k = 0.0;
    if (ch.piped && call.open_out(map_out, npix * sizeof(double), ch.stage)) {
        map_out = call.dst<double>();                        // (from here on: the page-locked view)
        if (int rc = paint_streamed(e, &dcat, m, ch, map_out)) return rc;
        ms_k = t.lap(p->stream);
        HIP_TRY(hipStreamSynchronize(e->down));
    } else {
        if (o.algo == 0) HIP_TRY(hipMemsetAsync(e->out.p, 0, npix * sizeof(double), p->stream));
        if (int rc = paint_impl(p, &dcat, e->out.p, m)) return rc;
        ms_k = t.lap(p->stream);
        if (m.map_f64()) {
            HIP_TRY(hipMemcpyAsync(map_out, e->out.p, npix * sizeof(double), hipMemcpyDeviceToHost, p->stream));
            HIP_TRY(hipStreamSynchronize(p->stream));
        } else {
            std::vector<float> tmp(npix);
            HIP_TRY(hipMemcpyAsync(tmp.data(), e->out.p, npix * sizeof(float), hipMemcpyDeviceToHost, p->stream));
            HIP_TRY(hipStreamSynchronize(p->stream));
            for (size_t i = 0; i < npix; ++i) map_out[i] = (double)tmp[i];
        }
    }
    const double ms_d2h = t.stop(p->stream);
    if (int rc = bfgx_plan_status(p)) return rc;
    call.commit();
    fill_stats(stats, nullptr, -1, ms_h2d, ms_k, ms_d2h);
    return BFGX_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------ synchronous host entries: the call scaffold
#include "bfgx_hostcall.hpp"

// ------------------------------------------------------------------------------ table builders (a6-a8)
#include "bfgx_tables_api.inc"

// ------------------------------------------------------------------------------ all GPUs of a node from one call
#include "bfgx_multi_api.inc"

// ------------------------------------------------------------------------------ pixel-window convolution (8f-3)
#include "bfgx_fftlog_api.inc"

// ------------------------------------------------------------------------------ regular-grid path (8f-1)
#include "bfgx_grid_api.inc"

// particle deposit (ParticleSnapshot.make_map) and particle routing; the fused deposit + regrid needs the grid plan
#include "bfgx_deposit_api.inc"

// CIC / TSC particle deposit (make_map(N, assignment=...)): shares the deposit's sort and workspace
#include "bfgx_deposit_cloud_api.inc"

// what the five Fourier files below share: checks, table cache, kernel attributes, launchers, the 3-D setup and its transform passes
#include "bfgx_fourier_host.inc"

// 3-D FFT and power spectrum of gridded maps
#include "bfgx_fft_api.inc"

// bispectrum of gridded 3-D maps: inverse slab transforms, k-shell fields, triangle sums
#include "bfgx_bispec_api.inc"

// cross power spectrum of two gridded 3-D maps: the cross modes of the last FFT pass, window weights
#include "bfgx_xpk_api.inc"

// interlaced power spectrum of two grids half a cell apart, P(k) straight from particle columns
#include "bfgx_interlace_api.inc"

// 2-D FFTs of gridded flat-sky maps: transform pair, power spectra, filters, Kaiser-Squires
#include "bfgx_fft2d_api.inc"

// ------------------------------------------------------------------------------ particle snapshots (8f-2)
#include "bfgx_snapshot_api.inc"

// ------------------------------------------------------------------------------ models that are Python callables
#include "bfgx_pairs.hpp"
#include "bfgx_callable_api.inc"
#include "bfgx_grid_pairs_api.inc"
#include "bfgx_snapshot_pairs_api.inc"

// spherical-harmonic transforms of HEALPix shells (map2alm / alm2map / alm2cl / anafast)
#include "bfgx_sht_api.inc"

// HEALPix pixel functions (ud_grade / get_interp_weights / get_interp_val / regrid_pixels_hpix)
#include "bfgx_hpx_api.inc"

// map reductions: moments / cross-moments and peak counts of HEALPix maps
#include "bfgx_mapstats_api.inc"

// mode-coupling matrices of a mask: pseudo-C_l of masked spin-0 and spin-2 shells
#include "bfgx_pcl_api.inc"

// halo-centred radial profiles: what the three measurements below share on the host
#include "bfgx_profiles_common.inc"

// halo-centred radial profiles of shell maps (MeasureProfilesShell)
#include "bfgx_stack_api.inc"

// halo-centred radial profiles of particle snapshots (MeasureProfilesSnapshot)
#include "bfgx_snapshot_stack_api.inc"

// halo-centred radial profiles of gridded maps (MeasureProfilesGrid)
#include "bfgx_grid_stack_api.inc"

// device-math probe: one function of bfgx_math.hpp elementwise (test infrastructure)
#include "bfgx_math_probe_api.inc"

extern "C" void bfgx_cache_clear(void)
{
    g_shells.clear();            // plans + device buffers of the one-shot shell entries
    dep_release_all();           // workspace of the tiled particle deposit (bfgx_deposit_api.inc)
    fourier_release_all();       // setups and tables of the 3-D and 2-D transforms and spectra (bfgx_fourier_host.inc)
    g_grids.clear();             // plans + device maps of the one-shot grid entries
    g_snaps.clear();             // plans + device record buffers of the snapshot records entries (bfgx_snapshot_api.inc)
    deprec_release_all();        // device buffers of the deposit's records entry
}
