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
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <functional>
#include <map>
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
#include "bfgx_deposit.hpp"
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
    double *tile_sums = nullptr;     // [ntiles][2] per-tile {sum of source values, sum of deposits} of the tiled regrid
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
    if (p->mem.alloc(p->far.pix, (size_t)p->far.cap) || p->mem.alloc(p->far.val, (size_t)p->far.cap) ||
        p->mem.alloc(p->tile_apron, 2 * (size_t)(T.ntiles + 1)))
        return alloc_fail("far list");
    if (p->mem.alloc(p->regrid_lean, (size_t)(T.ntiles + 4))) return alloc_fail("lean tile list");
    if (hipMemsetAsync(p->regrid_lean, 0, sizeof(int32_t) * 4, p->stream) != hipSuccess) return fail(BFGX_ERR_HIP, "hipMemset failed");
    // the list's counter and its two overflow flags lie in the arena (the full-map regrid swaps far_overflow_full in: launch_regrid_gather)
    p->far.count = &p->arena.ctrl->far_count;
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
    // (NSIDE 16384 has 3.2e9 pixels: the tile kernels keep first-pixel-of-ring offsets and per-tile counters in 32 bits -- RowScan.start, the
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
    if (p->mem.alloc(p->tile_sums, 2 * (size_t)(p->tiling.ntiles + 1))) return bail(alloc_fail("tile sums"));
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

int bfgx_plan_bands(bfgx_plan *p, int32_t *nbands, int64_t *band_first_pixel)
{
    if (!p || !nbands) return fail(BFGX_ERR_INVALID, "NULL argument");
    *nbands = p->tiling.nbands;
    if (band_first_pixel) {                       // band b = rings [1 + BR b, 1 + BR (b + 1)): a contiguous RING pixel range
        const int64_t nl4 = 4 * p->hpx.nside;
        for (int b = 0; b <= p->tiling.nbands; ++b) {
            const int64_t ring = std::min<int64_t>(1 + (int64_t)p->tiling.BR * b, nl4);
            if (ring >= nl4) { band_first_pixel[b] = p->hpx.npix; continue; }
            const int64_t ns = p->hpx.nside, q = nl4 - ring;
            band_first_pixel[b] = (ring < ns) ? 2 * ring * (ring - 1)
                                : (ring < 3 * ns) ? p->hpx.ncap + (ring - ns) * 4 * ns
                                : p->hpx.npix - 2 * q * (q + 1);
        }
    }
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

int bfgx_plan_band_apron(bfgx_plan *p, int32_t band0, int32_t band1, int64_t *olo, int64_t *ohi)
{
    if (!p || !olo || !ohi) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (band0 < 0 || band1 > p->tiling.nbands || band0 > band1) return fail(BFGX_ERR_INVALID, "band range out of bounds");
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
// band ranges while the map is still arriving, and applies one list at the end)
// m SPLIT (the fused band entry, the one-shot host entry): the low halves of the pixels [olo, ohi) follow their high halves
static int regrid_bands_impl(bfgx_plan *p, int32_t band0, int32_t band1, const double *map_in_dev, const void *offsets_dev,
                             int64_t olo, int64_t ohi, const DispMode &m, double *out_slice_dev, double *sums_dev, bool reset_far,
                             bool sums_later = false)
{
    if (p->algo != 1) return fail(BFGX_ERR_UNSUPPORTED, "banded regrid needs the tiled algorithm (algo 1)");
    int64_t need_lo = 0, need_hi = 0;
    if (int rc = bfgx_plan_band_apron(p, band0, band1, &need_lo, &need_hi)) return rc;
    if (band0 == band1) {
        // a rank that owns no band (more ranks than bands): empty buffers, whose data pointers are NULL, are fine
        HIP_TRY(hipSetDevice(p->device));
        if (reset_far) HIP_TRY(hipMemsetAsync(p->far.count, 0, sizeof(unsigned long long), p->stream));
        if (sums_dev) HIP_TRY(hipMemsetAsync(sums_dev, 0, 2 * sizeof(double), p->stream));
        return BFGX_OK;
    }
    if (!map_in_dev || !offsets_dev || !out_slice_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (olo > need_lo || ohi < need_hi || olo < 0 || ohi > p->hpx.npix)
        return fail(BFGX_ERR_INVALID, "pix_offsets range [%lld, %lld) does not cover the bands and %d ring(s) either side [%lld, %lld)",
                    (long long)olo, (long long)ohi, p->band_reach, (long long)need_lo, (long long)need_hi);
    HIP_TRY(hipSetDevice(p->device));
    if (reset_far) HIP_TRY(hipMemsetAsync(p->far.count, 0, sizeof(unsigned long long), p->stream));
    const int64_t p0 = ring_first_pixel(p->hpx, 1 + (int64_t)p->tiling.BR * band0);
    const int t0 = p->band_tile0_host[band0], t1 = p->band_tile0_host[band1];
    {
        KernelTimer kt(p, BFGX_K_REGRID);
        const size_t lds = regrid3_lds_bytes(p->tiling.BR, p->tiling.W, m.fp64() ? sizeof(double) : sizeof(float), p->band_reach > 1,
                                             m.split() ? sizeof(float) : 0);
        // virtual bases: the kernel indexes every array by global pixel number
        double *out_base = out_slice_dev - p0;
        // every rank gathers with the same fixed reach (so that all of them classify a source pixel the same way)
        const ReachArgs reach = reach_args(p, regrid_cap_for_rings(p->hpx.nside, p->band_reach));
        hipLaunchKernelGGL(tile_apron_kernel, dim3((t1 - t0 + 255) / 256), dim3(256), 0, p->stream, p->hpx, p->tiling, (const float *)nullptr,
                           p->band_reach, reach.cap, t0, t1 - t0, p->tile_apron, (int32_t *)nullptr);
        double *ts = sums_dev ? p->tile_sums : nullptr;
        const dim3 grid(t1 - t0), blk(256);
        int *none = nullptr;
#define BFGX_REGRID3(ACC, REAL, SPLIT, OL)                                                                                                     \
        do {                                                                                                                                    \
            const ACC *o = (const ACC *)offsets_dev - 3 * olo;                                                                                  \
            if (p->band_reach == 1) hipLaunchKernelGGL((tile_regrid3_kernel<ACC, REAL, 0, SPLIT>), grid, blk, lds, p->stream, p->hpx, p->tiling, map_in_dev, o, OL, \
                                                       out_base, p->far, reach, ts, t0, t1 - t0, none, (double *)nullptr);                      \
            else hipLaunchKernelGGL((tile_regrid3_kernel<ACC, REAL, 2, SPLIT>), grid, blk, lds, p->stream, p->hpx, p->tiling, map_in_dev, o, OL, \
                                    out_base, p->far, reach, ts, t0, t1 - t0, none, (double *)nullptr);                                         \
        } while (0)
        if (m.split()) BFGX_REGRID3(float, double, true, m.lo(offsets_dev, ohi - olo) - 3 * olo);
        else if (m.fp64()) BFGX_REGRID3(double, double, false, (const double *)nullptr);
        else BFGX_REGRID3(float, float, false, (const float *)nullptr);
#undef BFGX_REGRID3
        HIP_TRY(hipGetLastError());
    }
    if (sums_dev && !sums_later) {             // (sums_later: the caller's next kernel adds the per-tile sums up)
        KernelTimer kt(p, BFGX_K_SUM);
        if (t1 - t0 > 16384) {
            HIP_TRY(hipMemsetAsync(sums_dev, 0, 2 * sizeof(double), p->stream));
            hipLaunchKernelGGL(sum_tiles_multi_kernel, dim3(64), dim3(256), 0, p->stream, t1 - t0, (const double *)(p->tile_sums + 2 * (size_t)t0), sums_dev);
        } else
            hipLaunchKernelGGL(sum_tiles_kernel, dim3(1), dim3(256), 0, p->stream, t1 - t0, (const double *)(p->tile_sums + 2 * (size_t)t0), sums_dev);
        HIP_TRY(hipGetLastError());
    }
    return BFGX_OK;
}

int bfgx_plan_set_route_margin(bfgx_plan *p, int32_t rings)
{
    if (!p) return fail(BFGX_ERR_INVALID, "NULL plan");
    if (rings < 0 || rings > 4 * p->hpx.nside) return fail(BFGX_ERR_INVALID, "route margin must be 0 .. 4 nside rings");
    p->route_margin = rings;
    return BFGX_OK;
}

int bfgx_regrid_bands_device(bfgx_plan *p, int32_t band0, int32_t band1, const double *map_in_dev, const void *offsets_dev,
                             int64_t olo, int64_t ohi, int acc_f64, double *out_slice_dev, double *sums_dev)
{
    DispMode m;
    if (int rc = disp_mode(p, acc_f64, true, m)) return rc;
    return regrid_bands_impl(p, band0, band1, map_in_dev, offsets_dev, olo, ohi, m, out_slice_dev, sums_dev, true);
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
    RegridCtrl ctrl = {0, 0, 0};
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

// the checks of a K0 + K1 / K3 entry: the catalog, the kind of table (paint: a profile table), the output pointer.  bands: a pass over the tiles
// of bands [band0, band1) only; a rank that owns no band (more ranks than bands) passes the data pointer of an empty buffer, which is NULL
static int check_scatter(const bfgx_plan *p, const bfgx_catalog *cat, const void *out, bool paint, bool bands = false, int32_t band0 = 0, int32_t band1 = 0)
{
    if (int rc = check_catalog(p, cat)) return rc;
    if (bands && p->algo != 1) return fail(BFGX_ERR_UNSUPPORTED, "band-restricted passes need the tiled algorithm (algo 1)");
    if (bands && (band0 < 0 || band1 > p->tiling.nbands || band0 > band1)) return fail(BFGX_ERR_INVALID, "band range out of bounds");
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

// K0 + K1 for the bands [band0, band1) (band0 < band1) into pix_offsets from the first pixel of band0 (SPLIT: the low halves follow the high ones)
static int offsets_bands(bfgx_plan *p, const bfgx_catalog *cat, int32_t band0, int32_t band1, void *slice, const DispMode &m)
{
    TileLaunch k1;
    k1.tile_lo = p->band_tile0_host[band0];
    k1.tile_n = p->band_tile0_host[band1] - k1.tile_lo;
    if (int rc = launch_k0(p, cat, 1, m.fp64())) return rc;
    // K1's flush leaves the largest |offset|^2 of every tile it stores (bfgx_bands_max_offset2_device reduces them: the reach of the
    // regrid then needs no second pass over the slice)
    k1.omax = p->arena.omax;
    return launch_offsets(p, m, slice, ring_first_pixel(p->hpx, 1 + (int64_t)p->tiling.BR * band0),
                          ring_first_pixel(p->hpx, 1 + (int64_t)p->tiling.BR * band1), k1);
}

int bfgx_offsets_bands_device(bfgx_plan *p, const bfgx_catalog *cat, int32_t band0, int32_t band1, void *offsets_slice_dev, int acc_f64)
{
    if (int rc = check_scatter(p, cat, offsets_slice_dev, false, true, band0, band1)) return rc;
    if (band0 == band1) return BFGX_OK;
    DispMode m;
    if (int rc = disp_mode(p, acc_f64, true, m)) return rc;
    return offsets_bands(p, cat, band0, band1, offsets_slice_dev, m);
}

// K3 into the map held at `slice` from pixel p0 on (virtual base: the kernels index the output by global pixel number)
static int launch_paint(bfgx_plan *p, const PaintMode &m, void *slice, int64_t p0, TileLaunch k3)
{
    k3.paint_pair_f32 = m.pair_f32();
    if (m.map_f64()) return launch_tile_scatter<MODE_PAINT, double>(p, (double *)slice - p0, k3);
    return launch_tile_scatter<MODE_PAINT, float>(p, (float *)slice - p0, k3);
}

int bfgx_paint_bands_device(bfgx_plan *p, const bfgx_catalog *cat, int32_t band0, int32_t band1, void *map_slice_dev, int acc_f64)
{
    if (int rc = check_scatter(p, cat, map_slice_dev, true, true, band0, band1)) return rc;
    if (band0 == band1) return BFGX_OK;
    PaintMode m;
    if (int rc = paint_mode(p, acc_f64, m)) return rc;
    TileLaunch k3;
    k3.tile_lo = p->band_tile0_host[band0];
    k3.tile_n = p->band_tile0_host[band1] - k3.tile_lo;
    if (int rc = launch_k0(p, cat, 0, m.k0_f64())) return rc;
    return launch_paint(p, m, map_slice_dev, ring_first_pixel(p->hpx, 1 + (int64_t)p->tiling.BR * band0), k3);
}

// One rank's share of a resident multi-GPU BaryonifyShell step after the routing, as ONE enqueue-only call (Parallelize.py:250-318 has one call
// drive all workers): K0 + binning + K1 for the bands [B0, B1) (the rank's own and, with a route margin, the band either side: the aprons of
// its regrid) into offsets_dev (pixels from the first of band B0), the banded regrid of ITS bands [b0, b1) into out_slice_dev, the listed far
// deposits that fall into its pixels added, the others counted into *foreign_dev, the two sums of the mass check.  One memset (the binning's)
// zeroes every control word; eight launches.
int bfgx_offsets_regrid_bands_device(bfgx_plan *p, const bfgx_catalog *cat, int32_t B0, int32_t B1, void *offsets_dev, int acc_f64,
                                     int32_t b0, int32_t b1, const double *map_in_dev, double *out_slice_dev, double *sums_dev,
                                     unsigned long long *foreign_dev)
{
    if (!p || !cat) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (B0 < 0 || B1 > p->tiling.nbands || B0 > b0 || b1 > B1 || b0 > b1) return fail(BFGX_ERR_INVALID, "band ranges must nest: [B0, B1) around [b0, b1)");
    // the parity-grade mode: both halves of pix_offsets stay on this device (24 bytes per pixel, as fp64 would take)
    DispMode m;
    if (int rc = disp_mode(p, acc_f64, false, m)) return rc;
    const int64_t wlo = ring_first_pixel(p->hpx, 1 + (int64_t)p->tiling.BR * B0), whi = ring_first_pixel(p->hpx, 1 + (int64_t)p->tiling.BR * B1);
    if (int rc = check_scatter(p, cat, offsets_dev, false, true, B0, B1)) return rc;
    if (B0 < B1) if (int rc = offsets_bands(p, cat, B0, B1, offsets_dev, m)) return rc;      // (its memset also zeroes the far list's counter)
    if (b0 == b1) {
        if (sums_dev) HIP_TRY(hipMemsetAsync(sums_dev, 0, 2 * sizeof(double), p->stream));
        return BFGX_OK;
    }
    if (int rc = regrid_bands_impl(p, b0, b1, map_in_dev, offsets_dev, wlo, whi, m, out_slice_dev, sums_dev, false, true)) return rc;
    const int64_t p0 = ring_first_pixel(p->hpx, 1 + (int64_t)p->tiling.BR * b0), p1 = ring_first_pixel(p->hpx, 1 + (int64_t)p->tiling.BR * b1);
    const int t0 = p->band_tile0_host[b0], t1 = p->band_tile0_host[b1];
    hipLaunchKernelGGL(regrid_far_local_kernel, dim3(64), dim3(256), 0, p->stream, p->far, out_slice_dev, p0, p1, foreign_dev, t1 - t0,
                       sums_dev ? (const double *)(p->tile_sums + 2 * (size_t)t0) : (const double *)nullptr, sums_dev);
    HIP_TRY(hipGetLastError());
    return BFGX_OK;
}

int bfgx_bands_max_offset2_device(bfgx_plan *p, int32_t band0, int32_t band1, float *out_dev)
{
    if (!p || !out_dev) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (p->algo != 1) return fail(BFGX_ERR_UNSUPPORTED, "band-restricted passes need the tiled algorithm (algo 1)");
    if (band0 < 0 || band1 > p->tiling.nbands || band0 > band1) return fail(BFGX_ERR_INVALID, "band range out of bounds");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemsetAsync(out_dev, 0, sizeof(float), p->stream));
    const int t0 = p->band_tile0_host[band0], nt = p->band_tile0_host[band1] - t0;
    if (nt > 0) {
        hipLaunchKernelGGL(max_bits_kernel, dim3(1), dim3(1024), 0, p->stream, nt, (const unsigned *)p->arena.omax + t0, (unsigned *)out_dev);
        HIP_TRY(hipGetLastError());
    }
    return BFGX_OK;
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

// shared argument checks / set-up of the two routing passes
static int route_args(bfgx_plan *p, const bfgx_catalog *cat, int32_t world, const int32_t *ring_bounds, int32_t ncols, const double *const *cols,
                      RouteArgs &a)
{
    if (!p || !cat || !ring_bounds || !cols) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (world < 1 || world > kRouteMaxRanks) return fail(BFGX_ERR_INVALID, "routing supports 1 .. %d ranks", kRouteMaxRanks);
    if (ncols < 1 || ncols > kRouteMaxCols) return fail(BFGX_ERR_INVALID, "routing packs 1 .. %d columns", kRouteMaxCols);
    if (cat->n < 0) return fail(BFGX_ERR_INVALID, "catalog size < 0");
    std::memset(&a, 0, sizeof(a));
    a.world = world; a.ncols = ncols;
    for (int j = 0; j <= world; ++j) {
        if (j > 0 && ring_bounds[j] < ring_bounds[j - 1]) return fail(BFGX_ERR_INVALID, "ring bounds must ascend");
        a.bounds[j] = ring_bounds[j];
    }
    for (int c = 0; c < ncols; ++c) { if (cat->n > 0 && !cols[c]) return fail(BFGX_ERR_INVALID, "column pointer is NULL"); a.col[c] = cols[c]; }
    return BFGX_OK;
}

int bfgx_route_count_device(bfgx_plan *p, int64_t n, const int32_t *rings_dev, int32_t world, const int32_t *ring_bounds, int32_t *counts_dev)
{
    bfgx_catalog c;
    std::memset(&c, 0, sizeof(c));
    c.n = n;
    RouteArgs a;
    const double *none[1] = {nullptr};
    if (n < 0 || !counts_dev || (n > 0 && !rings_dev)) return fail(BFGX_ERR_INVALID, "NULL argument");
    c.n = 0;                                                    // (no columns are read in the counting pass)
    if (int rc = route_args(p, &c, world, ring_bounds, 1, none, a)) return rc;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemsetAsync(counts_dev, 0, sizeof(int32_t) * world, p->stream));
    if (n > 0) {
        hipLaunchKernelGGL(route_halos_kernel<false>, dim3((unsigned)std::min<int64_t>((n + 255) / 256, kRouteGrid)), dim3(256), 0, p->stream, a, n, rings_dev, counts_dev,
                           (int32_t *)nullptr, (double *)nullptr);
        HIP_TRY(hipGetLastError());
    }
    return BFGX_OK;
}

int bfgx_route_fill_device(bfgx_plan *p, int64_t n, const int32_t *rings_dev, int32_t world, const int32_t *ring_bounds, const int64_t *start,
                           int32_t ncols, const double *const *cols_dev, int32_t *cursor_dev, double *rows_dev)
{
    bfgx_catalog c;
    std::memset(&c, 0, sizeof(c));
    c.n = n;
    RouteArgs a;
    if (n < 0 || !start || !cursor_dev || (n > 0 && (!rings_dev || !rows_dev))) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (int rc = route_args(p, &c, world, ring_bounds, ncols, cols_dev, a)) return rc;
    for (int j = 0; j < world; ++j) a.start[j] = start[j];
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemsetAsync(cursor_dev, 0, sizeof(int32_t) * world, p->stream));
    if (n > 0) {
        hipLaunchKernelGGL(route_halos_kernel<true>, dim3((unsigned)std::min<int64_t>((n + 255) / 256, kRouteGrid)), dim3(256), 0, p->stream, a, n, rings_dev, (int32_t *)nullptr,
                           cursor_dev, rows_dev);
        HIP_TRY(hipGetLastError());
    }
    return BFGX_OK;
}

int bfgx_route_pack_device(bfgx_plan *p, int64_t n, const int32_t *rings_dev, int32_t world, const int32_t *ring_bounds, int64_t blockcap,
                           int32_t ncols, const double *const *cols_dev, int32_t *cursor_dev, double *blocks_dev, int32_t *overflow_dev)
{
    bfgx_catalog c;
    std::memset(&c, 0, sizeof(c));
    c.n = n;
    RouteArgs a;
    if (n < 0 || !cursor_dev || !blocks_dev || !overflow_dev || (n > 0 && !rings_dev)) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (blockcap < 1) return fail(BFGX_ERR_INVALID, "block capacity must be >= 1");
    if (int rc = route_args(p, &c, world, ring_bounds, ncols, cols_dev, a)) return rc;
    a.blockcap = blockcap; a.overflow = overflow_dev;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemsetAsync(cursor_dev, 0, sizeof(int32_t) * world, p->stream));
    hipLaunchKernelGGL(route_blank_kernel, dim3((unsigned)std::min<int64_t>(((int64_t)world * blockcap + 255) / 256, 1024)), dim3(256), 0, p->stream,
                       world, ncols, blockcap, blocks_dev);
    HIP_TRY(hipGetLastError());
    if (n > 0) {
        hipLaunchKernelGGL(route_halos_kernel<true>, dim3((unsigned)std::min<int64_t>((n + 255) / 256, kRouteGrid)), dim3(256), 0, p->stream, a, n, rings_dev, (int32_t *)nullptr,
                           cursor_dev, blocks_dev);
        HIP_TRY(hipGetLastError());
    }
    return BFGX_OK;
}

// The routing of one resident multi-GPU step as ONE call and two launches (bfgx_disc_rings_device + bfgx_route_pack_device were four, with a
// fill): route_prepare_kernel (NaN into column 0 of every block, the cursors zeroed) and route_step_kernel (ring range per halo, rows
// packed by destination).  send_blocks_dev holds (world - 1) blocks [ncols][blockcap] in rank order WITHOUT this rank, recv_blocks_dev
// world blocks: the other ranks' in rank order (what all_to_all_single delivers when the split towards oneself is empty), this rank's
// own rows LAST -- they never enter the collective.  K0 reads the received blocks as they are (bfgx_plan_set_catalog_blocks).
int bfgx_route_step_device(bfgx_plan *p, const bfgx_catalog *cat, int32_t world, int32_t rank, const int32_t *ring_bounds, int64_t blockcap,
                           int32_t ncols, const double *const *cols_dev, int32_t *cursor_dev, double *send_blocks_dev, double *recv_blocks_dev,
                           int32_t *overflow_dev)
{
    if (!p || !cat || !cursor_dev || !recv_blocks_dev || !overflow_dev || (world > 1 && !send_blocks_dev)) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (rank < 0 || rank >= world) return fail(BFGX_ERR_INVALID, "rank out of range");
    if (blockcap < 1) return fail(BFGX_ERR_INVALID, "block capacity must be >= 1");
    if (cat->n > 0 && (!cat->M || !cat->z || !cat->dec)) return fail(BFGX_ERR_INVALID, "catalog column pointer is NULL");
    RouteStepArgs s;
    std::memset(&s, 0, sizeof(s));
    if (int rc = route_args(p, cat, world, ring_bounds, ncols, cols_dev, s.r)) return rc;
    s.r.blockcap = blockcap; s.r.overflow = overflow_dev;
    s.rank = rank; s.margin = p->route_margin;
    s.M = cat->M; s.z = cat->z; s.dec = cat->dec;
    s.send = send_blocks_dev; s.recv = recv_blocks_dev;
    HIP_TRY(hipSetDevice(p->device));
    const int64_t nblank = (int64_t)(2 * world - 1) * blockcap;
    hipLaunchKernelGGL(route_prepare_kernel, dim3((unsigned)std::min<int64_t>((nblank + 255) / 256, 1024)), dim3(256), 0, p->stream, world, ncols, blockcap,
                       send_blocks_dev, recv_blocks_dev, cursor_dev);
    if (cat->n > 0)
        // (2048 workgroups: eight waves per SIMD hide the latency of the strided column stores; each adds to the per-destination cursors once)
        hipLaunchKernelGGL(route_step_kernel, dim3((unsigned)std::min<int64_t>((cat->n + 255) / 256, 4 * kRouteGrid)), dim3(256), 0, p->stream, s, p->model, p->hpx,
                           cat->n, cursor_dev);
    HIP_TRY(hipGetLastError());
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

int bfgx_disc_rings_device(bfgx_plan *p, const bfgx_catalog *cat, int32_t *rings_dev)
{
    // (uses none of the plan's per-halo workspace: the catalog may be larger than the plan's max_halos)
    if (!p || !cat) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (cat->n < 0) return fail(BFGX_ERR_INVALID, "catalog size < 0");
    if (cat->n > 0 && (!cat->M || !cat->z || !cat->dec)) return fail(BFGX_ERR_INVALID, "catalog column pointer is NULL");
    if (cat->n > 0 && !rings_dev) return fail(BFGX_ERR_INVALID, "rings pointer is NULL");
    HIP_TRY(hipSetDevice(p->device));
    if (cat->n > 0) {
        hipLaunchKernelGGL(disc_rings_kernel, dim3((unsigned)((cat->n + 255) / 256)), dim3(256), 0, p->stream, p->model, p->hpx, cat->n, cat->M, cat->z,
                           cat->dec, rings_dev, p->route_margin);
        HIP_TRY(hipGetLastError());
    }
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

// the gathering regrid (algo 1): [largest |offset|^2 per tile unless K1 left it], aprons, lean gather, gather with the ring
// walk over the tiles that need it, far list / repair
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
                       map_out_dev, far, reach, ts, -1, nt, p->regrid_lean, (double *)nullptr);
    hipLaunchKernelGGL((tile_regrid3_kernel<ACC, real, 2, SPLIT>), dim3(nwalk), dim3(256), lds_walk, p->stream, p->hpx, p->tiling, map_in_dev, o, o_lo,
                       map_out_dev, far, reach, ts, -1, nt, p->arena.todo, (double *)nullptr);
    // the two sums of the mass check: added up by the last launch, or -- above 16384 tiles, where that single workgroup's loop
    // takes 0.2 - 0.6 ms -- by 64 workgroups afterwards
    const bool many = nt > 16384 && sums_dev != nullptr && ts != nullptr;
    hipLaunchKernelGGL((tile_regrid3_kernel<ACC, real, 1, SPLIT>), dim3(nfix), dim3(256), lds, p->stream, p->hpx, p->tiling, map_in_dev, o, o_lo,
                       map_out_dev, far, reach, ts, -1, nt, p->arena.todo, many ? (double *)nullptr : sums_dev, p->regrid_lean);
    if (many) {
        (void)hipMemsetAsync(sums_dev, 0, 2 * sizeof(double), p->stream);
        hipLaunchKernelGGL(sum_tiles_multi_kernel, dim3(64), dim3(256), 0, p->stream, nt, (const double *)ts, sums_dev);
    }
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

// ------------------------------------------------------------------------------ one-shot host API
#include "bfgx_oneshot.hpp"

namespace {

constexpr int kCatCols = 4 + BFGX_MAX_EXTRA + 2;       // M, z, ra, dec, extra[2], ln1pz, lnM

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
        if ((i < 4 + nex || i >= 4 + BFGX_MAX_EXTRA) && h->n > 0 && !src[i]) return fail(BFGX_ERR_INVALID, "catalog column pointer is NULL");
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

int upload_catalog(bfgx_plan *p, const bfgx_catalog *h, DevBuf cols[kCatCols], bfgx_catalog *d, std::vector<double> &hostlog)
{
    const int nex = p->model.tab.ndim - 3;
    const double *src[kCatCols], *dp[kCatCols] = {};
    if (int rc = catalog_columns(h, nex, hostlog, src)) return rc;
    for (int i = 0; i < kCatCols; ++i) {
        if (!(i < 4 + nex || i >= 4 + BFGX_MAX_EXTRA)) continue;
        if (cols[i].alloc(sizeof(double) * (size_t)h->n)) return alloc_fail("catalog");
        if (h->n > 0) HIP_TRY(hipMemcpyAsync(cols[i].p, src[i], sizeof(double) * (size_t)h->n, hipMemcpyHostToDevice, p->stream));
        dp[i] = (const double *)cols[i].p;
    }
    catalog_view(h->n, nex, dp, d);
    return BFGX_OK;
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
    bfgx_plan *p = e->plan;
    if (token != 0 && token == e->cat_token && h->n == e->cat_n) {      // the same catalog as last time: its columns are still there
        *d = e->cat_dev;
        return BFGX_OK;
    }
    e->cat_token = 0;
    g_catalog_uploads.fetch_add(1);
    const int nex = p->model.tab.ndim - 3;
    const double *src[kCatCols], *dp[kCatCols] = {};
    if (int rc = catalog_columns(h, nex, hostlog, src)) return rc;
    for (int i = 0; i < kCatCols; ++i) {
        if (!(i < 4 + nex || i >= 4 + BFGX_MAX_EXTRA)) continue;
        if (e->cols[i].need(sizeof(double) * (size_t)std::max<int64_t>(h->n, 1))) return alloc_fail("catalog");
        if (h->n > 0) HIP_TRY(hipMemcpyAsync(e->cols[i].p, src[i], sizeof(double) * (size_t)h->n, hipMemcpyHostToDevice, p->stream));
        dp[i] = (const double *)e->cols[i].p;
    }
    catalog_view(h->n, nex, dp, d);
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
        k3.tile_lo = p->band_tile0_host[ch.cb[c]];
        k3.tile_n = p->band_tile0_host[ch.cb[c + 1]] - k3.tile_lo;
        // (the persistent kernel draws its tiles from a counter that the binning step zeroes: once more for every further launch)
        if (c > 0) HIP_TRY(hipMemsetAsync(p->arena.tile_counter, 0, sizeof(unsigned int), p->stream));
        if (int rc = launch_tile_scatter<MODE_PAINT, double>(p, (double *)e->out.p, k3)) return rc;      // (indexed by global pixel number)
        HIP_TRY(hipEventRecord(e->ev_k[c], p->stream));
        HIP_TRY(hipStreamWaitEvent(e->down, e->ev_k[c], 0));
        const int64_t lo = ch.bfp[ch.cb[c]], n = ch.bfp[ch.cb[c + 1]] - lo;
        HIP_TRY(hipMemcpyAsync(map_out + lo, (double *)e->out.p + lo, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, e->down));
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
extern "C" {

int bfgx_project_profile(int device, int64_t nrows, int32_t nl, const double *l, const double *rho,
                         int64_t nr, const double *r, double scale, double *sigma_out)
{
    if (!l || !rho || !r || !sigma_out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (nrows < 1 || nrows > 65535 || nl < 2 || nl > 2048 || nr < 1) return fail(BFGX_ERR_INVALID, "bad sizes (1 <= nrows <= 65535, 2 <= nl <= 2048)");
    HostCall c(device);
    const double *dl = c.in(l, nl), *drho = c.in(rho, nrows * nl), *dr = c.in(r, nr);
    double *dout = c.out(sigma_out, nrows * nr);
    if (int rc = c.ready()) return rc;
    hipLaunchKernelGGL(project_kernel, dim3((unsigned)((nr + 255) / 256), (unsigned)nrows), dim3(256), 3 * sizeof(double) * nl, 0,
                       nl, dl, drho, nr, dr, scale, dout);
    return c.finish();
}

static int enclosed_mass_rows(int dim, int device, int64_t nrows, int64_t n_int, const double *r_int, const double *Sigma,
                              int32_t nr, const double *r, double *M_f)
{
    if (!r_int || !Sigma || !r || !M_f) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (nrows < 1 || n_int < 3 || nr < 1) return fail(BFGX_ERR_INVALID, "bad sizes");
    HostCall c(device);
    const double *dri = c.in(r_int, n_int), *dS = c.in(Sigma, nrows * n_int), *dr = c.in(r, nr);
    double *dcx = c.scratch<double>(nrows * n_int), *dcy = c.scratch<double>(nrows * n_int), *dM = c.out(M_f, nrows * nr);
    if (int rc = c.ready()) return rc;
    hipLaunchKernelGGL(enclosed_mass_kernel, dim3((unsigned)nrows), dim3(kTabThreads), 0, 0, n_int, dri, dS, nr, dr, dcx, dcy, dM, dim);
    return c.finish();
}

int bfgx_enclosed_mass_from_sigma(int device, int64_t nrows, int64_t n_int, const double *r_int, const double *Sigma,
                                  int32_t nr, const double *r, double *M_f)
{
    return enclosed_mass_rows(2, device, nrows, n_int, r_int, Sigma, nr, r, M_f);
}

int bfgx_enclosed_mass_3d(int device, int64_t nrows, int64_t n_int, const double *r_int, const double *rho,
                          int32_t nr, const double *r, double *M_f)
{
    return enclosed_mass_rows(3, device, nrows, n_int, r_int, rho, nr, r, M_f);
}

int bfgx_enclosed_mass_2d(int device, int64_t nrows, int32_t nl, const double *l, const double *rho, double a,
                          int64_t n_int, const double *r_int, int32_t nr, const double *r, double *M_f)
{
    if (!l || !rho || !r_int || !r || !M_f) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (nrows < 1 || nrows > 65535 || nl < 2 || nl > 2048 || n_int < 3 || nr < 1) return fail(BFGX_ERR_INVALID, "bad sizes");
    HostCall c(device);
    const double *dl = c.in(l, nl), *drho = c.in(rho, nrows * nl), *dri = c.in(r_int, n_int);
    double *dS = c.scratch<double>(nrows * n_int);
    const double *dr = c.in(r, nr);
    double *dcx = c.scratch<double>(nrows * n_int), *dcy = c.scratch<double>(nrows * n_int), *dM = c.out(M_f, nrows * nr);
    if (int rc = c.ready()) return rc;
    // Sigma = model.projected(r_int) * a   (BaryonCorrection.py:646), then the prefix sum + log-log PCHIP
    hipLaunchKernelGGL(project_kernel, dim3((unsigned)((n_int + 255) / 256), (unsigned)nrows), dim3(256), 3 * sizeof(double) * nl, 0,
                       nl, dl, drho, n_int, dri, a, dS);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(enclosed_mass_kernel, dim3((unsigned)nrows), dim3(kTabThreads), 0, 0, n_int, dri, dS, nr, dr, dcx, dcy, dM, 2);
    return c.finish();
}

int bfgx_displacement_rows(int device, int64_t nrows, int32_t nr, const double *r, const double *M_dmo, const double *M_dmb,
                           double *d_out, int32_t *status)
{
    if (!r || !M_dmo || !M_dmb || !d_out || !status) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (nrows < 1 || nr < 3 || nr > kMaxNR) return fail(BFGX_ERR_INVALID, "N_samples_R must be in [3, %d]", kMaxNR);
    HostCall c(device);
    const double *dr = c.in(r, nr), *da = c.in(M_dmo, nrows * nr), *db = c.in(M_dmb, nrows * nr);
    double *dd = c.out(d_out, nrows * nr);
    int32_t *ds = c.out(status, nrows);
    if (int rc = c.ready()) return rc;
    const size_t lds = kDisplacementLdsPerNode * nr;
    HIP_TRY(hipFuncSetAttribute((const void *)displacement_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(displacement_kernel, dim3((unsigned)nrows), dim3(256), lds, 0, nr, dr, da, db, dd, ds);
    return c.finish();
}

int bfgx_pressure_profile(int device, int64_t nrows, const double *r500, const double *rho_tot, const double *rho_gas,
                          int32_t nr_out, const double *r_out, double cutoff, double *P_out)
{
    if (!r500 || !rho_tot || !rho_gas || !r_out || !P_out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (nrows < 1 || nr_out < 1) return fail(BFGX_ERR_INVALID, "bad sizes");
    HostCall c(device);
    const double *dg = c.in(r500, kPressureN), *dt = c.in(rho_tot, nrows * kPressureN), *dgas = c.in(rho_gas, nrows * kPressureN);
    const double *dr = c.in(r_out, nr_out);
    double *dP = c.out(P_out, nrows * nr_out);
    if (int rc = c.ready()) return rc;
    const double G = kGnewt / (kMpcToMeter * kMpcToMeter * kMpcToMeter) * kSolarMass;       // Thermodynamic.py:11
    const double unit = (kSolarMass * 1e3) / (kMpcToMeter * 1e2);                           // :265
    hipLaunchKernelGGL(pressure_kernel, dim3((unsigned)nrows), dim3(256), 0, 0, dg, dt, dgas, nr_out, dr, G, unit, cutoff, dP);
    return c.finish();
}

}  // extern "C"

// ------------------------------------------------------------------------------ all GPUs of a node from one call
#include "bfgx_multi_api.inc"

// ------------------------------------------------------------------------------ pixel-window convolution (8f-3)
#include "bfgx_fftlog_api.inc"

// ------------------------------------------------------------------------------ regular-grid path (8f-1)
#include "bfgx_grid_api.inc"

// particle deposit (ParticleSnapshot.make_map) and particle routing; the fused deposit + regrid needs the grid plan
#include "bfgx_deposit_api.inc"

// 3-D FFT and power spectrum of gridded maps
#include "bfgx_fft_api.inc"

// bispectrum of gridded 3-D maps: inverse slab transforms, k-shell fields, triangle sums
#include "bfgx_bispec_api.inc"

// cross power spectrum of two gridded 3-D maps: the cross modes of the last FFT pass, window weights
#include "bfgx_xpk_api.inc"

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
    fft_release_all();           // twiddle / wavenumber tables of the power spectrum
    bispec_release_all();        // n^2 -> bin tables of the bispectrum (bfgx_bispec_api.inc)
    xpk_release_all();           // window tables of the cross power spectrum (bfgx_xpk_api.inc)
    g_grids.clear();             // plans + device maps of the one-shot grid entries
    g_snaps.clear();             // plans + device record buffers of the snapshot records entries (bfgx_snapshot_api.inc)
    deprec_release_all();        // device buffers of the deposit's records entry
}
