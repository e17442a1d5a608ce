/*
 * bfgx.h -- C ABI of libbfgx.so, the MI355X (gfx950) engine behind
 * baryonification_amd.Runners.{BaryonifyShell,PaintProfilesShell}.process().
 *
 * The reference (BaryonForge, pure Python) has no FFI layer; its de-facto operator
 * interface for this path is the runner/model protocol.  Each entry point below
 * names the reference code it replaces (paths relative to the reference root):
 *
 *   bfgx_baryonify_shell   <- BaryonForge/Runners/HealpixRunner.py:240-349  BaryonifyShell.process
 *   bfgx_paint_shell       <- BaryonForge/Runners/HealpixRunner.py:366-447  PaintProfilesShell.process
 *   bfgx_offsets_device    <- HealpixRunner.py:291-331 (halo loop) + BaryonCorrection.py:324-390 (_readout)
 *   bfgx_regrid_device     <- HealpixRunner.py:333-346 + regrid_pixels_hpix :13-67
 *   bfgx_paint_device      <- HealpixRunner.py:418-445 + utils/Tabulate.py:246-294, 569-621 (_readout)
 *   bfgx_cosmo_*           <- the pyccl calls on the path: HealpixRunner.py:268-280, :296 and
 *                             BaryonCorrection.py:370 (ccl.Cosmology background, angular_diameter_distance,
 *                             MassDef.get_radius)
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a
 * negative bfgx_status, with a thread-local message in bfgx_last_error().  "_host"
 * pointers are caller-owned host memory (numpy); "_dev" pointers are device memory on the
 * plan's device (e.g. a torch tensor's data_ptr()).  Nothing is retained after return
 * except inside an explicit bfgx_plan.  All calls are blocking w.r.t. the host unless noted
 * ("_device" entry points only enqueue on the plan's stream).
 */
#ifndef BFGX_H
#define BFGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BFGX_ABI_VERSION 4

/* Precision of the displacement path (the `acc_f64` argument of the *_device entries, bfgx_opts.acc_offsets_f64).  The reference computes in
 * float64 throughout (HealpixRunner.py:289-341); SURVEY 8(d) states the tolerance a faster mode must hold: |d| <= 1e-6 mean(map) per pixel.
 *   BFGX_ACC_F32    fp32 pair math and fp32 pix_offsets [npix][3] (fp64 ring-row geometry and accumulation).  Holds 1e-6 mean(map) while a halo moves
 *                   a pixel by less than ~0.1 pixel sides (measured: 2.6e-7 / 3.9e-7 / 1.3e-6 / 8e-6 mean(map) at 0.03 / 0.09 / 0.3 / 0.9 pixels per halo, 2e-5 on a table that moves 9).
 *   BFGX_ACC_F64    fp64 throughout, pix_offsets double [npix][3]: the reference's own arithmetic, 1e-10 of the map scale.
 *   BFGX_ACC_PARITY the parity-grade mode: fp64 pair math whose elementary functions carry 1e-11 (fp32 hardware seeds + one Newton step), pix_offsets
 *                   as TWO fp32 arrays -- hi [npix][3], then lo [npix][3] = (float)(o - hi) behind it (24 bytes per pixel, as fp64) --, the regrid scans
 *                   the high halves and evaluates survivors in fp64 on hi + lo.  Within 1e-9 mean(map) of BFGX_ACC_F64 at any displacement.  Needs the fast
 *                   tile kernel (3-axis table, uniform ln r axis); elsewhere it runs as BFGX_ACC_F64.  The split layout is what it means for the full-map
 *                   entries (bfgx_offsets_device, bfgx_regrid_device, bfgx_baryonify_device) and the fused bfgx_offsets_regrid_bands_device;
 *                   bfgx_offsets_bands_device, bfgx_regrid_bands_device and bfgx_max_offset2_device, whose slices travel between ranks as ONE
 *                   array, serve it as BFGX_ACC_F64 (pix_offsets double [n][3]).
 *   BFGX_ACC_AUTO   the plan chooses from its table at creation: BFGX_ACC_F32 while the table cannot move a pixel by more than 0.1 pixel sides of the
 *                   plan's NSIDE (largest |d| a / D_A over the table's (z, M) nodes inside the model-side cut), BFGX_ACC_PARITY beyond.  The default of
 *                   the one-shot host entries and of the Python runners.  Scratch for pix_offsets must then hold 24 bytes per pixel.
 * bfgx_plan_precision tells what a request resolves to and how far the table moves a pixel. */
#define BFGX_ACC_AUTO   (-1)
#define BFGX_ACC_F32    0
#define BFGX_ACC_F64    1
#define BFGX_ACC_PARITY 3
#define BFGX_MAX_EXTRA 4          /* extra (per-halo parameter) table axes, model.p_keys (Tabulate.py:524-561 takes any number; four = 64 corner rows
                                     per halo is what the generic tile kernel is instantiated for; the regular-grid runners take two) */
#define BFGX_MAX_DIM (3 + BFGX_MAX_EXTRA)

typedef enum bfgx_status {
    BFGX_OK = 0,
    BFGX_ERR_INVALID = -1,        /* bad argument (ValueError on the Python side) */
    BFGX_ERR_HIP = -2,            /* HIP runtime error (RuntimeError) */
    BFGX_ERR_NO_DEVICE = -3,      /* no GPU visible (RuntimeError; there is NO CPU fallback) */
    BFGX_ERR_UNSUPPORTED = -4,    /* NotImplementedError */
    BFGX_ERR_MASS = -5,           /* mass-conservation check failed (AssertionError, HealpixRunner.py:344-346) */
    BFGX_ERR_ASSERT = -6          /* another assert of the reference fired (AssertionError), e.g. Map2DRunner.py:516 */
} bfgx_status;

/* cosmology dict of io.py:79-85 plus the pyccl-2.x defaults the reference inherits */
typedef struct bfgx_cosmo {
    double Omega_m, Omega_b, h, sigma8, n_s, w0;
    double T_CMB;                 /* <= 0 -> 2.725 K  */
    double Neff;                  /* <  0 -> 3.046    */
} bfgx_cosmo;

/* ccl.halos.massdef.MassDef(Delta, rho_type) */
typedef struct bfgx_massdef {
    double  Delta;                /* e.g. 200 */
    int32_t rho_type;             /* 0 = 'critical', 1 = 'matter' */
    int32_t _pad;
} bfgx_massdef;

/* a tabulated model: raw_input_* of Baryonification2D/3D (BaryonCorrection.py:309-313) or of
 * TabulatedProfile / ParamTabulatedProfile (utils/Tabulate.py:231-235, 553-558) */
typedef struct bfgx_table {
    int32_t ndim;                         /* 3 + number of extra axes */
    int32_t n[BFGX_MAX_DIM];              /* points per axis */
    const double *axis[BFGX_MAX_DIM];     /* host: ln(1+z), ln M, ln r | ln(r/R_Delta), extra params */
    const double *values;                 /* host, C-order [n0][n1][n2]...; displacement [comoving Mpc],
                                             or ln(projected profile * a) when log_values = 1 */
    int32_t rdelta_sampling;              /* BaryonCorrection.py:374-379 */
    int32_t log_values;                   /* 1: read-out returns exp(interp) (Tabulate.py:285-286) */
    double  eps_model;                    /* model.epsilon_max (BaryonCorrection.py:381); unused for paint */
} bfgx_table;

/* HaloLightConeCatalog.cat columns (io.py:58-60): M [Msun], z, ra/dec [deg] */
typedef struct bfgx_catalog {
    int64_t n;
    const double *M, *z, *ra, *dec;
    const double *extra[BFGX_MAX_EXTRA];  /* cat[p_keys[k]], in table-axis order; NULL if unused */
    /* optional (NULL = derive on the device): the halo's table coordinates as the CALLER's numpy computes them, in exactly the
     * reference's form: `a = 1 / (1 + z); ln1pz = np.log(1 / a)` (NOT np.log(1 + z): the two differ in the last bit) and
     * `lnM = np.log(M)` (BaryonCorrection.py:364-366, Tabulate.py:279-281; the Python binding: _lib.table_coords).  README.md:78-80
     * builds tables whose edges are exactly the catalog's min/max, so whether an edge halo is inside the table hangs on the last bit
     * of these logs.  The one-shot host API fills them itself, in the same form (libm), when they are NULL. */
    const double *ln1pz, *lnM;
} bfgx_catalog;

typedef struct bfgx_model {
    bfgx_table   table;
    bfgx_cosmo   cosmo_runner;            /* catalog.cosmology -> R_j, D_j (HealpixRunner.py:268-297) */
    bfgx_massdef massdef_runner;          /* runner mass_def (HealpixRunner.py:150) */
    bfgx_cosmo   cosmo_model;             /* model.cosmo -> R in _readout (BaryonCorrection.py:370) */
    bfgx_massdef massdef_model;           /* model.mass_def */
    double       eps_runner;              /* runner epsilon_max (HealpixRunner.py:305) */
} bfgx_model;

typedef struct bfgx_opts {
    int32_t device;                       /* HIP device ordinal */
    int32_t acc_offsets_f64;              /* BaryonifyShell precision: BFGX_ACC_AUTO (-1; what a NULL opts selects), BFGX_ACC_F32 (0), BFGX_ACC_F64 (1) or
                                             BFGX_ACC_PARITY (3), see above */
    int32_t acc_paint_f64;                /* painted map: 0 = f32 throughout, 1 = f64 throughout (default for host API),
                                             2 = f32 pair math, f64 accumulation and f64 map (2.3x faster, ~1e-5 relative) */
    int32_t check_mass;                   /* 1: enforce np.isclose(sum(new), sum(old)) like the reference */
    int32_t algo;                         /* 1 = LDS tiles (default), 0 = per-halo global atomics */
    int32_t _pad;
    uint64_t catalog_token;               /* 0: the catalog columns are copied to the device on every call.  Non-zero: the caller's name for
                                             the CONTENT of the catalog (e.g. a hash of its bytes); the one-shot entries keep the columns of
                                             the last call on the device and skip the copy when the same token and size come again.  The
                                             caller vouches that equal tokens mean equal columns (HealpixRunner.py re-reads `cat` on every
                                             call: the Python runner hashes every byte of the catalog) */
} bfgx_opts;

typedef struct bfgx_stats {
    int64_t n_pairs;                      /* (halo, pixel) pairs visited */
    double  sum_in, sum_out;              /* map sums (baryonify only) */
    double  ms_h2d, ms_kernels, ms_d2h;   /* host-API phase timings */
} bfgx_stats;

/* kernel kinds reported by bfgx_plan_timing_read */
enum { BFGX_K_PREP = 0, BFGX_K_OFFSETS = 1, BFGX_K_REGRID = 2, BFGX_K_PAINT = 3, BFGX_K_SUM = 4, BFGX_K_COUNT = 5,
       BFGX_K_BIN = 6, BFGX_K_WIDE = 7, BFGX_NUM_KERNELS = 8 };
/* OFFSETS / PAINT: the tile kernel of the plan, fast or generic; WIDE: never recorded (its slot stays in ABI version 4 and reads 0) */
/* the grid plan reports its kernels under the same kinds: PREP, OFFSETS (halo loop), PAINT, REGRID, SUM */

typedef struct bfgx_plan bfgx_plan;       /* opaque: device, stream, resident model + workspace */

/* ---- library ---------------------------------------------------------------------------- */
int         bfgx_abi_version(void);
const char *bfgx_last_error(void);
int         bfgx_device_count(void);      /* 0 when no GPU is visible */

/* ---- host-side background cosmology (pure CPU, double) ---------------------------------- */
int bfgx_cosmo_E2(const bfgx_cosmo *c, int64_t n, const double *a, double *out);
int bfgx_cosmo_radius(const bfgx_cosmo *c, const bfgx_massdef *md, int64_t n,
                      const double *M, const double *a, double *out_phys_mpc);
int bfgx_cosmo_angular_diameter_distance(const bfgx_cosmo *c, int64_t n, const double *z, double *out_mpc);
/* D_a = CubicSpline(linspace(0,30,1000), D_A) of HealpixRunner.py:279-280 (not-a-knot):
 * knots[1000], coef[999][4] = {c3,c2,c1,c0} of ((c3 t + c2) t + c1) t + c0, t = z - knots[i] */
int bfgx_cosmo_da_spline(const bfgx_cosmo *c, double *knots, double *coef);
int bfgx_cosmo_da_eval(const bfgx_cosmo *c, int64_t n, const double *z, double *out_mpc);

/* ---- one-shot host API (numpy in, numpy out; copies H2D/D2H itself) --------------------- */
int bfgx_baryonify_shell(const bfgx_catalog *cat_host, const bfgx_model *model, int64_t nside,
                         const double *map_in_host, double *map_out_host,
                         const bfgx_opts *opts, bfgx_stats *stats);
int bfgx_paint_shell(const bfgx_catalog *cat_host, const bfgx_model *model, int64_t nside,
                     double *map_out_host, const bfgx_opts *opts, bfgx_stats *stats);

/* ---- all GPUs of one node from ONE call (SURVEY 8b "multi-GPU variant taking a device list") -----------------------
 * The counterpart of SplitJoinParallel (utils/Parallelize.py:191-320) for a binder that has nothing but this C ABI: the
 * catalog (already shuffled by the caller if wanted, Parallelize.py:255) is cut into ndev contiguous shards
 * (ceil(n / ndev) halos, :250-266) that go up to device devices[d]; the ring bands of the sphere are dealt out to the devices and
 * every halo's row (48 B) is pulled, peer to peer over xGMI, by the device(s) whose bands its disc touches; each device computes
 * the pixels it owns (no accumulator crosses a link), pulls the apron rings of pix_offsets the gathering regrid needs from its
 * neighbours, regrids the OUTPUT pixels of its bands and copies its slice straight into map_out_host.  Same arguments, results and
 * errors as the single-device calls; opts->device is ignored, opts->algo must be 1.  `devices` may repeat a device. */
int bfgx_baryonify_shell_multi(const bfgx_catalog *cat_host, const bfgx_model *model, int64_t nside, const double *map_in_host,
                               double *map_out_host, int32_t ndev, const int32_t *devices, const bfgx_opts *opts, bfgx_stats *stats);
int bfgx_paint_shell_multi(const bfgx_catalog *cat_host, const bfgx_model *model, int64_t nside, double *map_out_host,
                           int32_t ndev, const int32_t *devices, const bfgx_opts *opts, bfgx_stats *stats);

/* The one-shot calls keep the plan (model on the device, tiling, binning workspace) and their device buffers in small
 * process-wide caches keyed by (device, model contents, nside / grid / box): a repeated call with the same model performs no
 * device allocation.  The shell, grid and snapshot-records entries each have a cache and a lock of their own.
 * bfgx_cache_clear frees the caches; bfgx_debug_alloc_count = device allocations made so far, bfgx_debug_live_allocs = those of them
 * not yet freed (tests).
 * bfgx_host_alloc / bfgx_host_free: page-locked host memory for map_out (D2H at full PCIe rate; plain memory works too). */
void      bfgx_cache_clear(void);
long long bfgx_debug_alloc_count(void);
long long bfgx_debug_live_allocs(void);
/* catalog copies host -> device made by the one-shot entries so far (tests: a call that repeats bfgx_opts.catalog_token makes none) */
long long bfgx_debug_catalog_uploads(void);
/* how the one-shot host entries have treated the caller's arrays so far (tests): arrays page-locked IN PLACE for a call (hipHostRegister; only
 * arrays of >= 32 MiB, which own their pages -- DESIGN.md section 9 "the two GPU memory faults of round 4"), arrays staged through a page-locked
 * buffer of the library's, and the smallest array ever page-locked in place (-1: none).  Any pointer may be NULL. */
void bfgx_debug_host_spans(long long *pinned_in_place, long long *staged, long long *smallest_pinned_bytes);
/* streamed bfgx_baryonify_grid calls so far that found a cell moving further along the first array axis than their plane ranges allow (2^S - 1 cells:
 * 7 in 3-D, 15 in 2-D) and repeated the regrid in one pass on the uploaded map (tests) */
long long bfgx_debug_grid_pipe_fallbacks(void);
/* the plan's ring table (tests): `count` records of 80 bytes from ring `first` on, copied to `out` -- { double theta, z, sin_theta, dphi, inv_dphi,
 * inv_dtheta_up, inv_dtheta_down; int64 start; int32 nr, shifted }, one per ring 0 .. 4 nside, rings 0 and 4 nside being the "no such ring"
 * records (nr = 0, theta = -1e300 / +1e300).  from_functions != 0: the same records for rings within 1 .. 4 nside - 1 evaluated afresh by the
 * device functions the table was built from, the four quotients (dphi .. inv_dtheta_down) left 0.  Waits for the plan's stream. */
int       bfgx_debug_ring_table(bfgx_plan *plan, int from_functions, int64_t first, int64_t count, void *out);
int       bfgx_host_alloc(size_t bytes, void **out);
void      bfgx_host_free(void *p);

/* ---- resident API (inputs already in HBM; enqueue-only on `hip_stream`) ------------------
 * hip_stream is a hipStream_t; NULL = the legacy default stream (torch's default stream). */
int  bfgx_plan_create(int device, void *hip_stream, int64_t nside, int64_t max_halos,
                      const bfgx_model *model, bfgx_plan **out);
void bfgx_plan_destroy(bfgx_plan *p);
/* accumulation algorithm of K1/K3: 1 (default) = tile-owned LDS accumulators, plain stores, every output
 * element written exactly once (no zero-fill needed); 0 = one wave per halo with global float atomics
 * (output must be zeroed by the caller) */
int  bfgx_plan_set_algo(bfgx_plan *p, int algo);
/* blocking health check of the plan's workspace (entry-list capacity); call outside timed regions */
int  bfgx_plan_status(bfgx_plan *p);
/* what `acc_requested` (BFGX_ACC_*) resolves to on this plan, and the largest displacement of the plan's table in pixel sides of its NSIDE
 * (either pointer may be NULL); HealpixRunner.py has no counterpart: the reference knows one precision */
int  bfgx_plan_precision(bfgx_plan *p, int acc_requested, int32_t *acc_resolved, double *table_disp_pixels);
/* K0 + K1: pix_offsets[npix][3] = sum of the per-halo unit-vector offsets (HealpixRunner.py:291-331); acc_f64 = BFGX_ACC_* selects precision and
 * layout (f32 / f64 [npix][3], or the split hi / lo arrays of BFGX_ACC_PARITY: 24 bytes per pixel) */
int  bfgx_offsets_device(bfgx_plan *p, const bfgx_catalog *cat_dev, void *offsets_dev, int acc_f64);
/* K2: map_out[npix] (f64) = bilinear regrid of the displaced pixels.  algo 1: every pixel of map_out is stored exactly
 * once by the tile that owns it (no zero-fill needed); algo 0: map_out += (must be zeroed by the caller).
 * sums_dev (optional, double[2]) receives {sum(map_in), sum(map_out)} */
int  bfgx_regrid_device(bfgx_plan *p, const double *map_in_dev, const void *offsets_dev, int acc_f64,
                        double *map_out_dev, double *sums_dev);
/* K0 + K1 + K2 in one enqueue-only call (BaryonifyShell.process() on device buffers): offsets_work_dev[npix][3] is the
 * pix_offsets scratch (12 bytes per pixel for BFGX_ACC_F32, 24 otherwise; every element overwritten), the other arguments as above.  Same results as
 * bfgx_offsets_device followed by bfgx_regrid_device; K1 hands the regrid the largest displacement of every tile, which
 * the separate calls have to find with one more pass over pix_offsets. */
int  bfgx_baryonify_device(bfgx_plan *p, const bfgx_catalog *cat_dev, const double *map_in_dev, void *offsets_work_dev,
                           int acc_f64, double *map_out_dev, double *sums_dev);
/* Multi-GPU form of K2: the sphere is cut into bands of consecutive rings (contiguous RING pixel ranges); a rank that
 * owns bands [band0, band1) produces exactly THEIR output pixels.  bfgx_plan_bands returns the number of bands and, in
 * band_first_pixel[nbands + 1] (may be NULL), the first pixel of every band (+ npix).  The gathering regrid evaluates
 * the displaced position of the rank's own pixels and of `rings` rings either side, where `rings` follows the largest
 * displacement of the SUMMED pix_offsets over all ranks: bfgx_plan_reach_rings(max |offset| in radians) -> rings (1 for
 * sub-pixel displacements, at most 16), bfgx_plan_set_band_reach(rings) -- every rank must set the same value (default
 * 1).  bfgx_plan_band_apron then returns the pixel range [olo, ohi) of summed pix_offsets the rank must hold
 * (offsets_dev points at pixel olo, [ohi - olo][3]; a wider range is accepted).
 * out_slice_dev points at the rank's first own pixel ([p1 - p0] values, every one stored exactly once, no zero-fill);
 * map_in_dev is the full map; sums_dev (optional, double[2]) receives {sum of the rank's source pixels, sum of its
 * deposits, the listed far ones included}.  Deposits that need the generic route (pixels next to a pole, displacements
 * beyond what `rings` rings of apron serve) are NOT applied by this call: they are listed with global pixel numbers;
 * bfgx_plan_far_fetch copies the list of the last regrid to the host (blocking; n_host = 0 almost always; NULL
 * buffers: count only) so that the caller can add them to whichever rank's slice holds the pixel.  (bfgx_regrid_device
 * sizes its aprons tile by tile from the data, applies its own list, and repairs an overflowing list in-stream.) */
int  bfgx_plan_bands(bfgx_plan *p, int32_t *nbands, int64_t *band_first_pixel);
/* the same maximum for the slice bfgx_offsets_bands_device has JUST written for the bands [band0, band1): reduced from the per-tile
 * maxima K1's flush leaves behind (a few thousand values) instead of a second pass over the slice.  Valid only while nothing
 * else has been added to that slice (spatial sharding: every rank computes its own pixels). */
int  bfgx_bands_max_offset2_device(bfgx_plan *p, int32_t band0, int32_t band1, float *out_dev);
/* *out_dev (float, device) = largest |offset|^2 of npixels pixels of pix_offsets (enqueue-only): what the ranks all-reduce (MAX).  acc_f64 reads
 * the array as the band entries write it: BFGX_ACC_F32 fp32 [n][3], BFGX_ACC_F64 and BFGX_ACC_PARITY fp64 [n][3], BFGX_ACC_AUTO as the plan
 * resolves it; any other value is refused with BFGX_ERR_INVALID before anything is enqueued. */
int  bfgx_max_offset2_device(bfgx_plan *p, const void *offsets_dev, int64_t npixels, int acc_f64, float *out_dev);
int  bfgx_plan_reach_rings(bfgx_plan *p, double max_offset, int32_t *rings);
int  bfgx_plan_set_band_reach(bfgx_plan *p, int32_t rings);
int  bfgx_plan_band_apron(bfgx_plan *p, int32_t band0, int32_t band1, int64_t *olo, int64_t *ohi);
int  bfgx_regrid_bands_device(bfgx_plan *p, int32_t band0, int32_t band1, const double *map_in_dev,
                              const void *offsets_dev, int64_t olo, int64_t ohi, int acc_f64, double *out_slice_dev, double *sums_dev);
/* A rank's share of one resident multi-GPU step in TWO calls (Parallelize.py:250-318: one call drives all workers).
 * bfgx_route_step_device: the routing -- per local halo the ring range its disc can touch (+ the plan's route margin) and its rows packed by
 * destination into fixed-capacity blocks [ncols][blockcap] (column 0 = M; rows nobody fills keep M = NaN, which K0 drops).  send_blocks_dev:
 * (world - 1) blocks in rank order WITHOUT this rank -- the input of ONE all_to_all_single whose split towards oneself is empty;
 * recv_blocks_dev: world blocks, the other ranks' in rank order first (where that all_to_all puts them), this rank's own rows LAST: they are
 * written there directly and never enter the collective.  *overflow_dev is set when a block was too small.  Two launches, nothing read back.
 * bfgx_plan_set_catalog_blocks(rows, stride): the catalogs of the following K0 launches are such blocks -- halo j's columns at
 * (j / rows) * stride + (j % rows) from the column pointers of block 0 (stride = ncols * blockcap); rows = 0: plain columns again.
 * bfgx_offsets_regrid_bands_device: K0 + binning + K1 for the bands [B0, B1) (the rank's own [b0, b1) and, with a route margin of one band, the
 * band either side: the aprons of its regrid, computed locally) into offsets_dev (pixels from the first pixel of band B0: [pixels][3] f32 or f64;
 * BFGX_ACC_PARITY -- or BFGX_ACC_AUTO on a table that asks for it -- keeps the parity-grade mode here, since nothing of pix_offsets leaves the
 * device: [pixels][3] f32 high halves followed by [pixels][3] f32 low halves, 24 bytes per pixel like f64), the banded regrid of [b0, b1) into out_slice_dev, the listed far deposits that fall into those
 * pixels added (the others counted into *foreign_dev, which the caller zeroes once), the two sums of the mass check.  One memset, eight launches. */
int  bfgx_route_step_device(bfgx_plan *p, const bfgx_catalog *cat_dev, int32_t world, int32_t rank, const int32_t *ring_bounds, int64_t blockcap,
                            int32_t ncols, const double *const *cols_dev, int32_t *cursor_dev, double *send_blocks_dev, double *recv_blocks_dev,
                            int32_t *overflow_dev);
int  bfgx_plan_set_catalog_blocks(bfgx_plan *p, int64_t rows, int64_t stride);
int  bfgx_offsets_regrid_bands_device(bfgx_plan *p, const bfgx_catalog *cat_dev, int32_t B0, int32_t B1, void *offsets_dev, int acc_f64,
                                      int32_t b0, int32_t b1, const double *map_in_dev, double *out_slice_dev, double *sums_dev,
                                      unsigned long long *foreign_dev);
int  bfgx_plan_far_fetch(bfgx_plan *p, int64_t cap, int64_t *pix_host, double *val_host, int64_t *n_host);
/* What the LAST full-map regrid (bfgx_regrid_device / bfgx_baryonify_device) did, read back from its control words (blocking;
 * diagnostics for tests and bench lines -- regrid_pixels_hpix, HealpixRunner.py:13-67, has no counterpart): deposits listed for the
 * generic route, whether that list overflowed (then repaired in-stream), tiles whose reach exceeded one ring (run by the walking
 * kernel), the largest reach of any tile in rings.  Any pointer may be NULL. */
int  bfgx_plan_regrid_stats(bfgx_plan *p, int64_t *far_listed, int32_t *far_overflowed, int32_t *tiles_walked, int32_t *max_reach_rings);
/* enqueue-only alternative: adds the listed deposits whose pixel lies in [p0, p1) to out_slice_dev (which starts at pixel
 * p0) and adds the number of the others to *foreign_dev (optional device counter the caller inspects later) */
int  bfgx_plan_far_apply_device(bfgx_plan *p, double *out_slice_dev, int64_t p0, int64_t p1, unsigned long long *foreign_dev);
/* Spatially sharded multi-GPU runs: a rank that owns the bands [band0, band1) (bfgx_plan_bands) takes every halo whose disc can
 * touch them -- bfgx_disc_rings_device gives, per halo, the ring range [first, last] (1-based, inclusive; first > last: nothing,
 * always as (1, 0)): the rings whose colatitude lies within the disc's colatitude band theta -+ radius (query_disc's irmin .. irmax),
 * widened by 2 rings either side and by the route margin, clipped to [1, 4 nside - 1]; a band that holds no ring (a disc between two
 * rings: the 4-pixel fallback) gives the 2 rings either side of the gap.  Every touched pixel lies within 1 ring of the band; the first
 * or last ring of the band may hold no pixel centre inside the disc, so the range exceeds the rings of the touched PIXELS by at most 3
 * (tests/test_gpu_route_step.py) -- and runs K0 + K1 (or K3) for ITS tiles only: offsets_slice_dev / map_slice_dev point at the first
 * pixel of band0 ([p1 - p0][3] resp. [p1 - p0] elements, every one stored exactly once); halos that reach into other bands are
 * clipped.  No accumulator travels between the ranks; the regrid then needs the neighbours' apron rings as above. */
int  bfgx_plan_tile_shape(bfgx_plan *p, int32_t *rings_per_band, int32_t *max_columns);     /* band b = rings [1 + b R, 1 + (b + 1) R) */
int  bfgx_disc_rings_device(bfgx_plan *p, const bfgx_catalog *cat_dev, int32_t *rings_dev /* [n][2]; n may exceed the plan's max_halos */);
/* rings by which bfgx_disc_rings_device widens every (non-empty) range from now on (default 0).  With a margin of one band
 * (bfgx_plan_tile_shape) a rank receives the halos of the bands next to its own as well and can compute the apron rows of its regrid
 * itself (bfgx_offsets_bands_device over [band0 - 1, band1 + 1)) instead of exchanging them with its neighbours: one collective less
 * per pass for ~2 bands of extra K1 work (valid while the reach, at most 16 rings, fits into a band). */
int  bfgx_plan_set_route_margin(bfgx_plan *p, int32_t rings);
/* Routing of halos that start out scattered over the ranks: ring_bounds[j] (host, world + 1 ascending entries) = first ring of rank
 * j's run of bands; a halo goes to every rank whose rings its range [first, last] (rings_dev, bfgx_disc_rings_device) touches.
 * Pass 1 counts the halos per destination (counts_dev[world]); the caller forms the exclusive prefix `start` (host) and exchanges the
 * counts; pass 2 packs the rows (ncols doubles per halo, from the ncols device columns cols_dev[]) into rows_dev, destination by
 * destination, ready for ONE all_to_all.  cursor_dev: int32[world] scratch.  At most 64 ranks, 8 columns. */
int  bfgx_route_count_device(bfgx_plan *p, int64_t n, const int32_t *rings_dev, int32_t world, const int32_t *ring_bounds, int32_t *counts_dev);
int  bfgx_route_fill_device(bfgx_plan *p, int64_t n, const int32_t *rings_dev, int32_t world, const int32_t *ring_bounds, const int64_t *start,
                            int32_t ncols, const double *const *cols_dev, int32_t *cursor_dev, double *rows_dev);
/* The same in ONE pass and with nothing read back by the host (a resident step: Parallelize.py:255-273 shuffles the catalog, so the counts
 * per destination are close to n / world): fixed-capacity blocks blocks_dev[world][ncols][blockcap], column-major inside a block, the
 * equal splits of ONE all_to_all.  Rows a destination does not receive keep M = NaN (column 0), which K0 drops as invalid halos;
 * *overflow_dev (int32, zeroed by the caller) is set when a destination would receive more than blockcap halos. */
int  bfgx_route_pack_device(bfgx_plan *p, int64_t n, const int32_t *rings_dev, int32_t world, const int32_t *ring_bounds, int64_t blockcap,
                            int32_t ncols, const double *const *cols_dev, int32_t *cursor_dev, double *blocks_dev, int32_t *overflow_dev);
int  bfgx_offsets_bands_device(bfgx_plan *p, const bfgx_catalog *cat_dev, int32_t band0, int32_t band1, void *offsets_slice_dev, int acc_f64);
int  bfgx_paint_bands_device(bfgx_plan *p, const bfgx_catalog *cat_dev, int32_t band0, int32_t band1, void *map_slice_dev, int acc_f64);
/* K0 + K3: map_out[npix] += painted profile; accumulator f32 or f64 */
/* acc_f64: 0 = float map, fp32 pair math; 1 = double map, fp64 throughout; 2 = double map and fp64 LDS accumulation with the pair
 * phase (chord, ln r, table read-out, exp) in fp32 -- the stated fp64 -> fp32 tolerance of this mode: 5e-5 of the pixel value */
int  bfgx_paint_device(bfgx_plan *p, const bfgx_catalog *cat_dev, void *map_out_dev, int acc_f64);
/* optional per-kernel timing with HIP events recorded on the plan's stream around every launch.
 * bfgx_plan_timing_read synchronises the stream, returns summed milliseconds and launch counts per
 * kernel kind (arrays of BFGX_NUM_KERNELS) since the previous read, and resets the counters. */
int  bfgx_plan_timing_enable(bfgx_plan *p, int on);
int  bfgx_plan_timing_read(bfgx_plan *p, double *ms_sum, int64_t *launches);

/* pair census (same enumeration as K1/K3, no scatter): counts_dev int64[n] or NULL; fallback4 = 1
 * counts the <4-pixel fallback of BaryonifyShell (HealpixRunner.py:309-310). Blocking. */
int  bfgx_count_pairs_device(bfgx_plan *p, const bfgx_catalog *cat_dev, int fallback4,
                             int64_t *counts_dev, int64_t *total_host);

/* ---- table builders: host arrays in, host arrays out, run once per model ----
 * The profile physics stays on the host: these take 3-D densities SAMPLED on the radial grids the
 * reference uses.  All double.  Replaces:
 *   bfgx_project_profile          SchneiderProfiles._projected_realspace, Profiles/Schneider19.py:245-252
 *                                 sigma[row][j] = scale * 2 trapz(interp(sqrt(l^2 + r_j^2), l, rho_row), l)
 *   bfgx_enclosed_mass_2d         Baryonification2D.get_masses, Profiles/BaryonCorrection.py:639-661
 *                                 (projection onto r_int times a, Sigma<0 -> 0, prefix sum, log-log PCHIP at r)
 *   bfgx_enclosed_mass_from_sigma the same from a projected profile the caller computed some other way
 *   bfgx_enclosed_mass_3d         Baryonification3D.get_masses, Profiles/BaryonCorrection.py:519-546: rho sampled on
 *                                 r_int = geomspace(min(r,1e-6)/1.2, max(r,1000)*1.2, 50 000), rho<0 -> 0,
 *                                 cumsum(4 pi r^3 rho dlnr), log-log PCHIP at r over the points with rho > 0
 *   bfgx_displacement_rows        setup_interpolator's per-mass loop body, BaryonCorrection.py:226-301;
 *                                 3 <= N_R <= 2511 (a row is held in one workgroup's 160 KiB of LDS, 64 B per node
 *                                 behind 3104 B of reduction arrays), anything else is BFGX_ERR_INVALID;
 *                                 status[row]: 0 ok, 1 mass profile nearly constant (iterate > 30),
 *                                 2 fewer than 5 usable points -- both give d = 0 and warrant the reference's warning
 *   bfgx_pressure_profile         Pressure._real, Profiles/Thermodynamic.py:240-271 (cgs), r500 = geomspace(1e-6,1e3,500) */
int bfgx_project_profile(int device, int64_t nrows, int32_t nl, const double *l, const double *rho,
                         int64_t nr, const double *r, double scale, double *sigma_out);
int bfgx_enclosed_mass_2d(int device, int64_t nrows, int32_t nl, const double *l, const double *rho, double a,
                          int64_t n_int, const double *r_int, int32_t nr, const double *r, double *M_f);
int bfgx_enclosed_mass_from_sigma(int device, int64_t nrows, int64_t n_int, const double *r_int, const double *Sigma,
                                  int32_t nr, const double *r, double *M_f);
int bfgx_enclosed_mass_3d(int device, int64_t nrows, int64_t n_int, const double *r_int, const double *rho,
                          int32_t nr, const double *r, double *M_f);
int bfgx_displacement_rows(int device, int64_t nrows, int32_t nr, const double *r, const double *M_dmo,
                           const double *M_dmb, double *d_out, int32_t *status);
int bfgx_pressure_profile(int device, int64_t nrows, const double *r500, const double *rho_tot, const double *rho_gas,
                          int32_t nr_out, const double *r_out, double cutoff, double *P_out);

/* ---- pixel-window convolution ---------------------------------------------------
 * BaryonForge/utils/Pixel.py: ConvolvedProfile.real (:106-157) / .projected (:160-224) = FFTLog forward, x pixel window,
 * FFTLog back, PCHIP in ln r.  The transform is pyccl.pyutils._fftlog_transform(rs, frs, dim, mu, power_law_index)
 * (pyccl 2.8.0, a C port of Hamilton's FFTLog); pyccl is absent here, so what is implemented is the published algorithm
 * (Hamilton 2000, App. B) with the bias exponent q = dim/2 + power_law_index and the low-ringing k r nearest to 1:
 *   dim 3: F(k) = (2 pi)^-3 int d^3r f(r) j_mu(k r)-kernel;   dim 2: F(k) = (2 pi)^-2 int d^2r f(r) J_mu(k r).
 * Host arrays in / out; f and prof are [nrows][n] on the log grid r (positive, ascending, log-uniform). */
/* the output grid of one transform (pure CPU): k_j = (k r)_lowring / r[n-1-j] */
int bfgx_fftlog_kgrid(int32_t n, const double *r, int32_t dim, double mu, double plaw, double *k_out);
/* the coefficients of that transform (pure CPU): u_out holds u_m, m = 0 .. n/2, as (re, im) pairs -- exactly what the kernel
 * multiplies the half spectrum by -- and *lnkr_out = ln(k r)_lowring */
int bfgx_fftlog_u(int32_t n, const double *r, int32_t dim, double mu, double plaw, double *u_out, double *lnkr_out);
/* out[row][i] = scipy PchipInterpolator(x[n], y[row][n], extrapolate=False)(q[i]), and 0 where q[i] is outside [x[0], x[n-1]] or NaN
 * (the last step of bfgx_fftlog_convolve, alone).  x strictly ascending, n >= 2, nq >= 1, 1 <= nrows <= 65535 */
int bfgx_pchip_rows(int device, int64_t nrows, int32_t n, const double *x, const double *y, int32_t nq, const double *q, double *out);
/* ks, fks = _fftlog_transform(rs, frs, dim, mu, plaw) */
int bfgx_fftlog_transform(int device, int64_t nrows, int32_t n, const double *r, const double *f, int32_t dim, double mu,
                          double plaw, double *k_out, double *F_out);
/* Pixel.py:146-155 / :208-222 in one call: transform(prof; plaw_fwd) * window -> transform(.; plaw_back) ->
 * PchipInterpolator(ln(r_out * r_scale), ., extrapolate=False)(ln r_eval), NaN -> 0, x (2 pi)^dim.
 * window[n] = Pixel.real / Pixel.projected evaluated by the caller at bfgx_fftlog_kgrid(r_fft, plaw_fwd); r_eval[nq] is
 * already clipped at pixel_size / 5 (:153, :217-219); r_scale = D_A for harmonic pixels (r_fft given in radians), else 1 */
int bfgx_fftlog_convolve(int device, int64_t nrows, int32_t n, const double *r_fft, const double *prof, int32_t dim, double mu,
                         double plaw_fwd, double plaw_back, const double *window, int32_t nq, const double *r_eval, double r_scale,
                         double *out);

/* ---- regular-grid path: periodic square / cubic maps ---------------------------------
 * Replaces BaryonForge/Runners/Map2DRunner.py: BaryonifyGrid.process :431-607, PaintProfilesGrid.process :676-817,
 * regrid_pixels_2D :14-83, regrid_pixels_3D :86-163; utils/io.py ParticleSnapshot.make_map :622-670; and the FFT
 * P(k) summary of examples/10_Reproduce_Schneider_deltaPk.ipynb cells 12, 15.
 * Maps are C-order [npix]^ndim doubles.  The grid runners build ccl.Cosmology WITHOUT w0 (Map2DRunner.py:456-459):
 * callers pass cosmo_runner with w0 = -1.  HaloNDCatalog stores float32 columns (io.py:205): the caller passes those
 * values widened to double, plus (optionally) lnM = the float32 logarithm the reference's read-out takes of the mass
 * (BaryonCorrection.py:369, Tabulate.py:283), evaluated with the caller's numpy so that its last bit agrees. */
typedef struct bfgx_grid {
    int32_t ndim;                         /* 2 or 3 */
    int32_t npix;                         /* pixels per side, >= 5 */
    const double *bins;                   /* [npix] pixel-centre coordinates, comoving Mpc, strictly ascending */
    double redshift;
} bfgx_grid;

typedef struct bfgx_grid_catalog {
    int64_t n;
    const double *M, *x, *y, *z;          /* z (a Cartesian coordinate) may be NULL for 2D maps */
    const double *lnM;                    /* optional, see above; NULL -> (double)logf((float)M) on the device */
    const double *rmat;                   /* optional [n][4]: row-major 2x2 matrices of DefaultRunnerGrid.build_Rmat
                                             (use_ellipticity = True, 2D maps only) */
    const double *extra[BFGX_MAX_EXTRA];
} bfgx_grid_catalog;

typedef struct bfgx_grid_plan bfgx_grid_plan;

/* one-shot host API.  bfgx_paint_grid reads the LOG of raw_input_2D (2D maps) / raw_input_3D (3D maps) as table. */
int bfgx_baryonify_grid(const bfgx_grid_catalog *cat_host, const bfgx_model *model, const bfgx_grid *grid,
                        const double *map_in_host, double *map_out_host, const bfgx_opts *opts, bfgx_stats *stats);
int bfgx_paint_grid(const bfgx_grid_catalog *cat_host, const bfgx_model *model, const bfgx_grid *grid,
                    double *map_out_host, const bfgx_opts *opts, bfgx_stats *stats);
/* regrid_pixels_2D / regrid_pixels_3D: grid[npix]^ndim += overlap-weighted values; positions [n][ndim] */
int bfgx_regrid_pixels(int device, int32_t ndim, int32_t npix, int64_t n, const double *positions_host,
                       const double *values_host, double *grid_inout_host);
/* ParticleSnapshot.make_map: histogramdd of n particles on edges = linspace(0, L, n_grid + 1) (edges [n_grid + 1]
 * given by the caller), weights = mass (NULL -> 1).  x, y, z host arrays; z NULL for 2D. */
int bfgx_deposit_particles(int device, int32_t ndim, int64_t n, const double *x, const double *y, const double *z,
                           const double *mass, int32_t n_grid, const double *edges, double *map_out_host);
/* The same on the snapshot's RECORDS (io.py:378-470: one structured array with float64 fields M, x, y, z): records [n][itemsize bytes] go
 * to the device as they are and the kernels read the fields at byte offsets off_x / off_y / off_z (ignored in 2-D) / off_mass (< 0: unit
 * masses) -- the four strided column gathers of make_map's host side (io.py:640-650) do not happen.  itemsize and the offsets must be
 * multiples of 8.  Device buffers are kept between calls (bfgx_cache_clear). */
int bfgx_deposit_particles_records(int device, int32_t ndim, int64_t n, const void *records, int32_t itemsize, int32_t off_x, int32_t off_y,
                                   int32_t off_z, int32_t off_mass, int32_t n_grid, const double *edges, double *map_out);
/* ParticleSnapshot.make_map(N, assignment='cic' | 'tsc'): cloud-in-cell (order 2) or triangular-shaped-cloud (order 3) mass assignment
 * of n particles on the periodic box [0, L]^ndim with n_grid cells per axis (cell centres at (i + 1/2) L / n_grid); `order` as
 * window_order of bfgx_cross_power_spectrum, which divides the matching window out.  Per axis, with t = v n_grid / L: CIC u = t - 1/2,
 * i = floor(u), f = u - i: cells i and i + 1 (mod n_grid) get 1 - f and f; TSC i = min(floor(t), n_grid - 1), d = t - i - 1/2: cells
 * i - 1, i, i + 1 (mod n_grid) get (1/2 - d)^2 / 2, 3/4 - d^2, (1/2 + d)^2 / 2.  A particle with a coordinate outside [0, L] (or NaN) is
 * dropped as np.histogramdd drops it.  mass NULL -> 1; z NULL for 2D.  order must be 2 or 3 (BFGX_ERR_INVALID otherwise: nearest grid
 * point is bfgx_deposit_particles).  x, y, z, mass host arrays. */
int bfgx_deposit_cloud(int device, int32_t ndim, int64_t n, const double *x, const double *y, const double *z, const double *mass,
                       int32_t n_grid, double L, int32_t order, double *map_out_host);
/* The same on the snapshot's records (see bfgx_deposit_particles_records: same layout rules, same device-side NaN test of the masses
 * with the same BFGX_ERR_ASSERT, same buffers kept between calls). */
int bfgx_deposit_cloud_records(int device, int32_t ndim, int64_t n, const void *records, int32_t itemsize, int32_t off_x, int32_t off_y,
                               int32_t off_z, int32_t off_mass, int32_t n_grid, double L, int32_t order, double *map_out);
/* |FFT(map)|^2 averaged in nk linear k-bins between 2 pi / L and the Nyquist frequency (3D, n_grid a power of two):
 * pk[nk], kcen[nk] (mean |k| per bin), counts[nk] (modes per bin).  Empty bins give NaN as in the notebook. */
int bfgx_power_spectrum(int device, int32_t n_grid, const double *map_host, double L, int32_t nk,
                        double *pk, double *kcen, int64_t *counts);

/* resident API: inputs already in HBM; enqueue-only except for one small read-back of the work-item count */
int  bfgx_grid_plan_create(int device, void *hip_stream, const bfgx_grid *grid_host_bins, int64_t max_halos,
                           const bfgx_model *model, bfgx_grid_plan **out);
void bfgx_grid_plan_destroy(bfgx_grid_plan *p);
/* halo loop of BaryonifyGrid: offsets_dev [npix^ndim][ndim] f64 is zeroed and filled; n_pairs_host optional */
int  bfgx_grid_offsets_device(bfgx_grid_plan *p, const bfgx_grid_catalog *cat_dev, double *offsets_dev, int64_t *n_pairs_host);
/* halo loop of PaintProfilesGrid: map_out_dev [npix^ndim] f64 is zeroed and filled */
int  bfgx_grid_paint_device(bfgx_grid_plan *p, const bfgx_grid_catalog *cat_dev, double *map_out_dev, int64_t *n_pairs_host);
/* post-loop regrid; map_out_dev is zeroed by the call; sums_dev (optional, double[2], zeroed by the caller)
 * receives {sum(map_in), sum(map_out)} */
int  bfgx_grid_regrid_device(bfgx_grid_plan *p, const double *map_in_dev, const double *offsets_dev,
                             double *map_out_dev, double *sums_dev);
/* Slab decomposition over GPUs (BASELINE config 5): a plan may own the planes [plane_lo, plane_lo + plane_n) of the FIRST
 * array axis.  bfgx_grid_offsets_device / _paint_device then fill plane_n x npix (x npix) cells (every rank passes the
 * whole catalog; cutouts are clipped to the slab), and bfgx_grid_regrid_slab_device regrids the slab's source cells
 * (map_in, offsets: the slab) into map_out = the slab + `apron` planes either side ([plane_n + 2 apron] planes, zeroed by
 * the call, periodic): the caller adds the apron planes to the neighbours' slabs.  *missed_dev (optional, zeroed by the
 * caller) is set when a deposit fell outside the buffer (apron too small). */
int  bfgx_grid_plan_set_slab(bfgx_grid_plan *p, int32_t plane_lo, int32_t plane_n);
int  bfgx_grid_regrid_slab_device(bfgx_grid_plan *p, const double *map_in_dev, const double *offsets_dev, int32_t apron,
                                  double *map_out_dev, double *sums_dev, int32_t *missed_dev);
/* BaryonifyGrid.process() on device arrays, single GPU: the halo loop (Map2DRunner.py:476-575) and the regrid (:577-605) as ONE
 * cell-owned pass -- halos are listed per block of cells, every cell sums its offsets in registers and is regridded at once, so no
 * pix_offsets array exists.  map_out [npix^ndim] is zeroed by the call; sums_dev [2] (optional, zeroed by the caller) receives
 * {sum(map_in), sum(map_out)}.  Same result as bfgx_grid_offsets_device + bfgx_grid_regrid_device up to the order of fp64 sums. */
int  bfgx_grid_baryonify_device(bfgx_grid_plan *p, const bfgx_grid_catalog *cat_dev, const double *map_in_dev, double *map_out_dev,
                                double *sums_dev, int64_t *n_pairs_host);
/* ParticleSnapshot.make_map (io.py:622-670) + BaryonifyGrid.process (Map2DRunner.py:431-607) in one call, all pointers device, the
 * whole grid on one GPU: the particles (x, y[, z], optional mass; unit mass when NULL) are histogrammed on the plan's grid with
 * np.histogramdd's bin rule against edges_dev [npix + 1] -> map_in_dev, and the cell-owned pass of bfgx_grid_baryonify_device turns it
 * into map_out_dev.  Same results as bfgx_deposit_particles_device followed by bfgx_grid_baryonify_device; the deposit stores map_out's
 * start value and the map's sum along with map_in, so the map is not read again to copy it.  sums_dev as above. */
int  bfgx_grid_deposit_baryonify_device(bfgx_grid_plan *p, const bfgx_grid_catalog *cat_dev, int64_t n_particles, const double *x,
                                        const double *y, const double *z, const double *mass, const double *edges_dev, double *map_in_dev,
                                        double *map_out_dev, double *sums_dev, int64_t *n_pairs_host);
int  bfgx_grid_plan_timing_enable(bfgx_grid_plan *p, int on);
int  bfgx_grid_plan_timing_read(bfgx_grid_plan *p, double *ms_sum, int64_t *launches);
/* device-resident variants of the two deposit kernels and the P(k) summary (all pointers device) */
int  bfgx_deposit_particles_device(int device, void *hip_stream, int32_t ndim, int64_t n, const double *x, const double *y,
                                   const double *z, const double *mass, int32_t n_grid, const double *edges_dev,
                                   double *map_out_dev);
/* the same for the planes [plane_lo, plane_lo + plane_n) of the FIRST axis only (slab decomposition over GPUs): map_out_dev
 * holds plane_n x n_grid (x n_grid) cells, particles of other planes are dropped */
int  bfgx_deposit_particles_slab_device(int device, void *hip_stream, int32_t ndim, int64_t n, const double *x, const double *y,
                                        const double *z, const double *mass, int32_t n_grid, const double *edges_dev,
                                        int32_t plane_lo, int32_t plane_n, double *map_out_dev);
/* bfgx_deposit_cloud on device-resident columns, enqueue-only: map_out_dev [n_grid^ndim] is stored whole (no need to zero it).  The
 * tile-owned form (n >= 2^20 on a grid the NGP tiles take; BFGX_DEPOSIT=atomic / tiled forces a form) keeps a grow-only workspace per
 * device, the per-tile halo scratch included, that bfgx_cache_clear releases; one deposit in flight per device. */
int  bfgx_deposit_cloud_device(int device, void *hip_stream, int32_t ndim, int64_t n, const double *x, const double *y, const double *z,
                               const double *mass, int32_t n_grid, double L, int32_t order, double *map_out_dev);
/* The same with shift = 1 on the grid displaced by half a cell, the second grid of an interlaced pair: every particle moved by
 * +L / (2 n_grid) along every axis, periodically, defined in cell units.  Per axis, with t = v n_grid / L: CIC i = floor(t) (0 .. n_grid),
 * f = t - i: cells i and i + 1 (mod n_grid) get 1 - f and f; TSC t2 = t + 1/2, i = floor(t2), d = t2 - i - 1/2: cells i - 1, i, i + 1 (mod
 * n_grid) get (1/2 - d)^2 / 2, 3/4 - d^2, (1/2 + d)^2 / 2.  Which particles are kept does not change (v = L is inside and lands in cell 0).
 * shift = 0 is bfgx_deposit_cloud_device; any other value is BFGX_ERR_INVALID. */
int  bfgx_deposit_cloud_shifted_device(int device, void *hip_stream, int32_t ndim, int64_t n, const double *x, const double *y, const double *z,
                                       const double *mass, int32_t n_grid, double L, int32_t order, int32_t shift, double *map_out_dev);
/* work_dev: scratch of bfgx_power_spectrum_work_doubles(n_grid) doubles (the half spectrum, complex [n_grid][n_grid][pitch] with
 * rows padded to whole 128-byte lines; its content is undefined afterwards: the last FFT pass bins |F|^2 straight from LDS) */
int64_t bfgx_power_spectrum_work_doubles(int32_t n_grid);
/* complex values per row of the half spectrum in every work array below: n_grid/2 + 1 rounded up to a multiple of 8 */
int32_t bfgx_fft_pitch(int32_t n_grid);
/* routing of particles to the ranks that own their planes (slab decomposition: rank r owns the planes [r n/world, (r + 1) n/world) of
 * the first axis; bin rule of np.histogramdd on x, particles outside the edges are dropped).  Pass 1 (enqueue-only): owner_dev[n]
 * (uint8 scratch) and counts_dev[world] (int32) = particles bound for every rank.  Pass 2, after the caller has read the counts:
 * cols_out_dev[c][start[d] + ...] = column c of the particles bound for rank d (ncols <= 4 columns of `total` = sum(counts) kept
 * particles each, any order inside a destination); cursor_dev[world] int32 scratch. */
int  bfgx_route_particles_count_device(int device, void *hip_stream, int64_t n, const double *x_dev, int32_t n_grid, const double *edges_dev,
                                       int32_t world, uint8_t *owner_dev, int32_t *counts_dev);
int  bfgx_route_particles_fill_device(int device, void *hip_stream, int64_t n, int32_t ncols, const double *const *cols_dev,
                                      const uint8_t *owner_dev, int32_t world, const int64_t *start_host, int64_t total,
                                      int32_t *cursor_dev, double *cols_out_dev);
int  bfgx_power_spectrum_device(int device, void *hip_stream, int32_t n_grid, const double *map_dev, double L, int32_t nk,
                                double *work_dev, double *pk_sum_dev, double *k_sum_dev, unsigned long long *counts_dev);

/* The same P(k) summary for a grid that is slab-decomposed over GPUs: (1) every rank transforms its `planes` planes of the
 * first axis along the last two axes (map [planes][n][n] -> complex work [planes][n][pitch], pitch = bfgx_fft_pitch(n): the pad
 * columns hold nothing and are never looked at); (2) the caller transposes between the ranks (all_to_all) so that every rank holds
 * all n planes of `ncols` columns of the MIDDLE axis, work [n][ncols][pitch]; (3) every rank transforms along the first axis and bins its modes (col0 = its first column; work is
 * scratch afterwards): the three sums are partial and are added over the ranks by the caller. */
int  bfgx_fft_slab_planes_device(int device, void *hip_stream, int32_t n_grid, int32_t planes, const double *map_dev, double *work_dev);
int  bfgx_fft_slab_axis0_pk_device(int device, void *hip_stream, int32_t n_grid, int32_t ncols, int32_t col0, double *work_dev, double L,
                                   int32_t nk, double *pk_sum_dev, double *k_sum_dev, unsigned long long *counts_dev);

/* ---- bispectrum of a gridded 3-D map (FFT estimator of Scoccimarro 2000) ---------------------------------
 * Units of bfgx_power_spectrum: F = the unnormalised np.fft.fftn(map), no volume factors.  A mode with integer wavevector n (fftfreq(N) N
 * per axis) has k = 2 pi / L sqrt(n^2) and lies in bin i when k_edges[i] <= k < k_edges[i + 1] (k_edges[nbins + 1] finite, non-negative,
 * strictly ascending; the rule is evaluated once per n^2 on the host, np.searchsorted(k_edges, k, 'right') - 1; modes outside every bin are
 * dropped).  With the unnormalised inverse transforms I_i(x) = sum_{k in i} F(k) e^{+ikx} and U_i(x) = sum_{k in i} e^{+ikx}, a triangle
 * (i, j, l) of bin indices gets
 *   b_sum = sum_x I_i I_j I_l / N^3 = the sum of F(k1) F(k2) F(k3) over the closed triples k1 + k2 + k3 = 0, k1 in i, k2 in j, k3 in l,
 *   n_tri = sum_x U_i U_j U_l / N^3 = their number (an integer up to the rounding of the fp64 transforms),
 * and a bin pk_sum = sum_x I_i^2 / N^3 = sum_{k in i} |F|^2 and n_modes = sum_x U_i^2 / N^3.  B = b_sum / n_tri, P = pk_sum / n_modes.
 * Limits: n_grid a power of two in [8, 1024] (else BFGX_ERR_UNSUPPORTED), 1 <= nbins <= 32, 1 <= ntri <= 8192.  Results are bitwise
 * reproducible from call to call (fixed-order sums, no floating-point atomics).  Tables are kept per (device, n_grid, L, k_edges) until
 * bfgx_cache_clear.  All complex arrays are half spectra with rows of bfgx_fft_pitch(n_grid) values and must be 16-byte aligned. */
/* in-place complex transforms along the FIRST axis of work [n][ncols][pitch]; inverse != 0: exponent +i, unnormalised.  Pad columns are
 * transformed as lines of their own. */
int  bfgx_fft_slab_axis0_device(int device, void *hip_stream, int32_t n_grid, int32_t ncols, double *work_dev, int32_t inverse);
/* inverse along the middle axis, then complex-to-real along the last: work [planes][n][pitch] -> map_out [planes][n][n], unnormalised
 * (planes * n even); pad columns are never read, the imaginary parts of the columns 0 and n/2 are ignored as numpy.irfft ignores them;
 * work is scratch afterwards */
int  bfgx_ifft_slab_planes_device(int device, void *hip_stream, int32_t n_grid, int32_t planes, double *work_dev, double *map_out_dev);
/* doubles of scratch bfgx_bispectrum_device needs: two half spectra, nbins real fields, the partial sums of the triangle kernel
 * (host arithmetic; 0 for sizes outside the limits) */
int64_t bfgx_bispectrum_work_doubles(int32_t n_grid, int32_t nbins);
/* the filtered fields alone: spec_dev = the full half spectrum [n][n][pitch] (kept), scratch_spec_dev another one, fields_dev
 * [nbins][n][n][n]; unit != 0: U_i instead of I_i */
int  bfgx_bispectrum_shell_fields_device(int device, void *hip_stream, int32_t n_grid, double L, int32_t nbins, const double *k_edges_host,
                                         const double *spec_dev, int32_t unit, double *scratch_spec_dev, double *fields_dev);
/* map_dev [n][n][n] -> b_sum_dev[ntri], n_tri_dev[ntri], pk_sum_dev[nbins], n_modes_dev[nbins]; tri_host[ntri][3] bin indices;
 * work_dev: bfgx_bispectrum_work_doubles(n_grid, nbins) doubles.  Enqueue-only once the tables of (n_grid, L, k_edges) exist. */
int  bfgx_bispectrum_device(int device, void *hip_stream, int32_t n_grid, const double *map_dev, double L, int32_t nbins,
                            const double *k_edges_host, int32_t ntri, const int32_t *tri_host, double *work_dev, double *b_sum_dev,
                            double *n_tri_dev, double *pk_sum_dev, double *n_modes_dev);
/* the same on host arrays (synchronous) */
int  bfgx_bispectrum(int device, int32_t n_grid, const double *map_host, double L, int32_t nbins, const double *k_edges, int32_t ntri,
                     const int32_t *tri, double *b_sum, double *n_tri, double *pk_sum, double *n_modes);

/* ---- cross power spectrum of two gridded 3-D maps -----------------------------------------------------------
 * Units and bins of bfgx_power_spectrum: F = the unnormalised np.fft.fftn(map), nk linear bins between 2 pi / L and the Nyquist
 * frequency; counts and the sums of |k| are those of the auto spectrum.  Per bin, over the modes in it (the mirrored half of the spectrum
 * through a weight of 2):  paa_sum = sum w |F_A|^2,  pbb_sum = sum w |F_B|^2,  pab_sum = sum w Re(F_A conj F_B).
 * window_order p = 0, 1, 2, 3 (none, NGP, CIC, TSC) divides out the mass-assignment window: for a mode with integer wave numbers
 * (n_a, n_b, n_c) (fftfreq(N) N per axis) and s(n) = sin(pi n / N) / (pi n / N), s(0) = 1, w = [s(n_a) s(n_b) s(n_c)]^(-2p); k_sum and
 * counts are not weighted.  Map A is transformed along all three axes and kept; the last FFT pass of map B reads A's coefficient as B's
 * leaves the butterflies, so B's spectrum is never stored.  The sums are added by floating-point atomics: correct to rounding, not bitwise
 * reproducible from call to call (counts, and k_sum for nk <= 254, are).  Limits: n_grid a power of two in [8, 1024] (else
 * BFGX_ERR_UNSUPPORTED), 1 <= nk <= 2048, L > 0; complex arrays 16-byte aligned, rows of bfgx_fft_pitch(n_grid) values whose pad columns
 * may hold anything.  Tables are kept per (device, n_grid, L, nk) and (device, n_grid, p) until bfgx_cache_clear. */
/* doubles of scratch bfgx_cross_power_spectrum_device needs: two half spectra (host arithmetic) */
int64_t bfgx_cross_power_spectrum_work_doubles(int32_t n_grid);
/* map_a_dev, map_b_dev [n][n][n] (they may be the same map) -> the five sums [nk], all pointers device.  Enqueue-only once the tables
 * exist. */
int  bfgx_cross_power_spectrum_device(int device, void *hip_stream, int32_t n_grid, const double *map_a_dev, const double *map_b_dev, double L,
                                      int32_t nk, int32_t window_order, double *work_dev, double *paa_sum_dev, double *pbb_sum_dev,
                                      double *pab_sum_dev, double *k_sum_dev, unsigned long long *counts_dev);
/* the last pass alone on the columns [col0, col0 + ncols) of the middle axis, the counterpart of bfgx_fft_slab_axis0_pk_device: spec_a_dev
 * [n][ncols][pitch] = map A's spectrum of these columns, transformed along all three axes (read-only); work_b_dev [n][ncols][pitch] = map
 * B's before the axis-0 pass (read, not changed).  The two ranges must not overlap.  The sums are partial: a caller that splits the
 * columns adds them up. */
int  bfgx_fft_slab_axis0_xpk_device(int device, void *hip_stream, int32_t n_grid, int32_t ncols, int32_t col0, const double *spec_a_dev,
                                    double *work_b_dev, double L, int32_t nk, int32_t window_order, double *paa_sum_dev, double *pbb_sum_dev,
                                    double *pab_sum_dev, double *k_sum_dev, unsigned long long *counts_dev);
/* the same on host arrays (synchronous): paa, pbb, pab = the sums divided by counts, kcen = mean |k| per bin, NaN for empty bins as in
 * bfgx_power_spectrum */
int  bfgx_cross_power_spectrum(int device, int32_t n_grid, const double *map_a_host, const double *map_b_host, double L, int32_t nk,
                               int32_t window_order, double *paa, double *pbb, double *pab, double *kcen, int64_t *counts);

/* ---- interlaced power spectrum ------------------------------------------------------------------------------
 * Two grids of one particle set, the second deposited half a cell away (bfgx_deposit_cloud_shifted_device), combined in Fourier space so
 * that the odd aliased images cancel: with F1, F2 the unnormalised fftn of the grids and phi[i] = exp(+i pi n_i / N) per axis (n =
 * fftfreq(N) N; phi[N/2] = 1, a definition that keeps the combined field real), C = (F1 + phi[a] phi[b] phi[c] F2) / 2.  Per linear
 * k-bin of bfgx_power_spectrum, p_sum = sum w |C|^2 and p1_sum = sum w |F1|^2 (grid 1 alone, the aliased estimate), w the window weights of
 * bfgx_cross_power_spectrum; k_sum and counts as there.  Limits, alignment and messages are those of the cross power spectrum; the phase
 * table is kept per (device, n_grid) until bfgx_cache_clear.  Sums by floating-point atomics, as there. */
/* map1_dev, map2_dev [n][n][n] -> the four sums [nk], all pointers device; work_dev: bfgx_cross_power_spectrum_work_doubles(n_grid)
 * doubles.  Enqueue-only once the tables exist. */
int  bfgx_interlaced_power_spectrum_device(int device, void *hip_stream, int32_t n_grid, const double *map1_dev, const double *map2_dev, double L,
                                           int32_t nk, int32_t window_order, double *work_dev, double *p_sum_dev, double *p1_sum_dev,
                                           double *k_sum_dev, unsigned long long *counts_dev);
/* doubles of scratch bfgx_particle_power_spectrum_device needs: the two maps and the two half spectra (host arithmetic) */
int64_t bfgx_particle_power_spectrum_work_doubles(int32_t n_grid);
/* Particle columns (device, 3-D; mass NULL -> 1) -> the same four sums: the deposit of `order` (2 = CIC, 3 = TSC; anything else, nearest
 * grid point included, is BFGX_ERR_INVALID), the shifted deposit, the interlaced spectrum with that order's window divided out; nothing
 * leaves the device.  interlace = 0: one deposit and the windowed auto spectrum, p_sum = p1_sum.  One call in flight per device (the
 * deposit's workspace). */
int  bfgx_particle_power_spectrum_device(int device, void *hip_stream, int64_t n, const double *x, const double *y, const double *z,
                                         const double *mass, int32_t n_grid, double L, int32_t order, int32_t interlace, int32_t nk,
                                         double *work_dev, double *p_sum_dev, double *p1_sum_dev, double *k_sum_dev,
                                         unsigned long long *counts_dev);
/* the same on host columns (synchronous): pk, pk_grid1 = the sums divided by counts, kcen = mean |k| per bin, NaN for empty bins */
int  bfgx_particle_power_spectrum(int device, int64_t n, const double *x, const double *y, const double *z, const double *mass, int32_t n_grid,
                                  double L, int32_t order, int32_t interlace, int32_t nk, double *pk, double *pk_grid1, double *kcen,
                                  int64_t *counts);

/* ---- flat-sky maps: 2-D FFTs, power spectra, filters, Kaiser-Squires ------------------------------------------
 * A real map [n][n] (C order, axis 0 = x, axis 1 = y) and its half spectrum [n][pitch] of complex values, pitch = bfgx_fft_pitch(n), the
 * coefficients c <= n/2 of axis 1: one plane of the layout above.  Transforms are unnormalised with exponent -i forward; n a power of two
 * in [8, 4096] (else BFGX_ERR_UNSUPPORTED).  Every _device entry takes work_dev, bfgx_fft2_work_doubles(n) doubles of scratch (three half
 * spectra), 16-byte aligned like every complex array, and only enqueues once the twiddles of (device, n) exist; they are kept until
 * bfgx_cache_clear.  Pad columns c > n/2 are never read; what the entries store there is undefined.  The transforms use no atomics and
 * repeat bitwise. */
/* doubles of scratch of the entries below (host arithmetic; 0 for an unsupported n) */
int64_t bfgx_fft2_work_doubles(int32_t n);
/* map_dev [n][n] -> spec_out_dev [n][pitch] */
int  bfgx_rfft2_device(int device, void *hip_stream, int32_t n, const double *map_dev, double *work_dev, double *spec_out_dev);
/* spec_dev [n][pitch] (kept) -> map_out_dev [n][n] = scale * sum_k spec e^{+ikx}; the spectrum of a real field: the imaginary parts that
 * break Hermitian symmetry in the columns 0 and n/2 are ignored, as numpy.irfft ignores them */
int  bfgx_irfft2_device(int device, void *hip_stream, int32_t n, const double *spec_dev, double scale, double *work_dev, double *map_out_dev);
/* Auto and cross spectra of two maps (which may be the same) in the bins, units and window weights of bfgx_cross_power_spectrum with the
 * third wave number at 0: k = sqrt(klin[a]^2 + klin[c]^2), nk linear bins from 2 pi / L to pi n / L, bin = floor((k - k0) / dk), w =
 * win[a] win[c]; the five sums [nk] as there (floating-point atomics; counts exact).  1 <= nk <= 2048, L > 0, window_order 0 .. 3. */
int  bfgx_power_spectrum_2d_device(int device, void *hip_stream, int32_t n, const double *map_a_dev, const double *map_b_dev, double L, int32_t nk,
                                   int32_t window_order, double *work_dev, double *paa_sum_dev, double *pbb_sum_dev, double *pab_sum_dev,
                                   double *k_sum_dev, unsigned long long *counts_dev);
/* map_out = irfft2(rfft2(map) b(k)) / n^2, k = 2 pi / L sqrt(n0^2 + n1^2) (fftfreq's wave numbers).  kind 0: Gaussian, b = exp(-k^2
 * param^2 / 2); 1: top hat of radius param, b = 2 J1(k param) / (k param), 1 at 0; 2: the table (table_k, table_b)[ntable] (HOST arrays;
 * k finite and strictly ascending, at most min(65536, n pitch) nodes), interpolated linearly and held at its end values (np.interp).
 * param >= 0.  map_out_dev may be map_dev. */
int  bfgx_filter_map_2d_device(int device, void *hip_stream, int32_t n, const double *map_dev, double L, int32_t kind, double param,
                               const double *table_k_host, const double *table_b_host, int32_t ntable, double *work_dev, double *map_out_dev);
/* The derivatives of a filtered map from its half spectrum spec_dev [n][pitch] (what bfgx_rfft2_device leaves; kept, 16-byte aligned):
 * ders_out_dev[nder][n][n], map d = irfft2(spec m_d b(k)) / n^2.  With fftfreq's n0 (axis 0, x), n1 = c (axis 1, y), g = 2 pi / L n and
 * h = n / 2 the multipliers are  u: 1;  u_x: i g0 (0 where a == h);  u_y: i g1 (0 where c == h);  u_xx: -g0^2;  u_xy: -g0 g1 (0 where
 * a == h or c == h);  u_yy: -g1^2 -- a factor odd in an index is 0 at that index's Nyquist value, as s2 below.  spin_form == 0:
 * [u, u_x, u_y, u_xx, u_xy, u_yy]; spin_form != 0: [u, u_x, u_y, lap = u_xx + u_yy, q_plus = u_xx - u_yy, q_cross = 2 u_xy], the six maps
 * bfgx_mapstats_minkowski_device takes.  nder = 6, or 1 for the filtered map alone.  kind, param and the table as in
 * bfgx_filter_map_2d_device, and kind 3: no filter (b = 1; param and the table are ignored).  work_dev:
 * bfgx_derivatives_2d_work_doubles(n, nder) = 2 n pitch (nder + 1) doubles (host arithmetic; 0 for an unsupported n or nder): the nder
 * products, then the scratch of the out-of-place column pass, in which the beam table rides until the products are formed.  The
 * spectrum is read once, b(k) is evaluated once per mode; no atomics: a repeated call gives the same bits. */
int64_t bfgx_derivatives_2d_work_doubles(int32_t n, int32_t nder);
int  bfgx_derivatives_2d_device(int device, void *hip_stream, int32_t n, const double *spec_dev, double L, int32_t kind, double param,
                                const double *table_k_host, const double *table_b_host, int32_t ntable, int32_t nder, int32_t spin_form,
                                double *work_dev, double *ders_out_dev);
/* Kaiser-Squires.  With fftfreq's integer wave numbers n0 (axis 0) and n1 = c (axis 1): c2 = (n0^2 - n1^2) / (n0^2 + n1^2), s2 = 2 n0 n1 /
 * (n0^2 + n1^2), both 0 at the zero mode, s2 = 0 where either index is the Nyquist index.  g1^ = c2 kappa^, g2^ = s2 kappa^; back:
 * kappa_E^ = c2 g1^ + s2 g2^, kappa_B^ = -s2 g1^ + c2 g2^.  Outputs may be the inputs. */
int  bfgx_kappa_to_shear_2d_device(int device, void *hip_stream, int32_t n, const double *kappa_dev, double *work_dev, double *g1_out_dev,
                                   double *g2_out_dev);
int  bfgx_shear_to_kappa_2d_device(int device, void *hip_stream, int32_t n, const double *g1_dev, const double *g2_dev, double *work_dev,
                                   double *kappa_e_out_dev, double *kappa_b_out_dev);
/* the same on host arrays (synchronous); the spectra divided by counts, kcen = mean |k| per bin, NaN for empty bins */
int  bfgx_power_spectrum_2d(int device, int32_t n, const double *map_a_host, const double *map_b_host, double L, int32_t nk, int32_t window_order,
                            double *paa, double *pbb, double *pab, double *kcen, int64_t *counts);
int  bfgx_filter_map_2d(int device, int32_t n, const double *map_host, double L, int32_t kind, double param, const double *table_k,
                        const double *table_b, int32_t ntable, double *map_out);
int  bfgx_kappa_to_shear_2d(int device, int32_t n, const double *kappa_host, double *g1, double *g2);
int  bfgx_shear_to_kappa_2d(int device, int32_t n, const double *g1_host, const double *g2_host, double *kappa_e, double *kappa_b);

/* ---- particle-snapshot path ----------------------------------------------------------
 * Replaces BaryonifySnapshot.process, BaryonForge/Runners/SnapshotRunner.py:173-262: every particle within
 * R_q = clip(epsilon_max R200c / a, 0, L/2) of a halo (periodic box) moves radially by displacement(d, M, a) * a;
 * positions are re-wrapped into [0, L] once.  Halos are given as bfgx_grid_catalog (float32-valued columns, lnM as
 * for the grid runners; rmat / extra unused).  cosmo_runner.w0 = -1 (SnapshotRunner.py:204-207 does not pass w0). */
typedef struct bfgx_snapshot {
    int32_t ndim;                         /* 2 or 3 */
    int32_t _pad;
    int64_t n;                            /* particles */
    const double *x, *y, *z;              /* coordinates in [0, L]; z may be NULL for 2D */
    double L;                             /* box size, comoving Mpc */
    double redshift;
} bfgx_snapshot;

int bfgx_baryonify_snapshot(const bfgx_grid_catalog *halos_host, const bfgx_model *model, const bfgx_snapshot *snap_host,
                            double *x_out_host, double *y_out_host, double *z_out_host, const bfgx_opts *opts, bfgx_stats *stats);
/* The same on the snapshot's RECORDS as ParticleSnapshot keeps them (io.py:378-470: one structured array `cat` with float64 fields M, x, y,
 * z): records_in [n][itemsize bytes] is copied to the device in chunks, the coordinate fields at byte offsets off_x / off_y / off_z (off_z
 * ignored in 2-D) are displaced in place, and the records -- every other field untouched -- arrive in records_out (may not alias
 * records_in): what `new_cat = cat.copy(); new_cat['x'] = ...` (SnapshotRunner.py:254-262) leaves, without a strided gather or scatter
 * of the columns on the host.  Upload, displacement and download of successive chunks overlap; plan and device buffer are cached
 * (bfgx_cache_clear).  itemsize and the offsets must be multiples of 8. */
int bfgx_baryonify_snapshot_records(const bfgx_grid_catalog *halos_host, const bfgx_model *model, int32_t ndim, double L, double redshift,
                                    int64_t n, const void *records_in, void *records_out, int32_t itemsize, int32_t off_x, int32_t off_y,
                                    int32_t off_z, const bfgx_opts *opts, bfgx_stats *stats);
/* ParticleSnapshot(cat = BaryonifySnapshot(...).process()).make_map(n_grid) in one call (SnapshotRunner.py:173-262 then io.py:622-670), for a
 * caller who wants the map of the displaced particles only: the records go up once, the displaced coordinates are never stored or sent back,
 * map_out [n_grid^ndim] float64 (host) = np.histogramdd of the displaced positions on edges [n_grid + 1] (host) with the weights of the float64
 * field at off_mass (off_mass < 0: unit masses; NaN masses -> BFGX_ERR_ASSERT, io.py:636).  Same record rules as above. */
int bfgx_baryonify_snapshot_records_map(const bfgx_grid_catalog *halos_host, const bfgx_model *model, int32_t ndim, double L, double redshift,
                                        int64_t n, const void *records_in, int32_t itemsize, int32_t off_x, int32_t off_y, int32_t off_z,
                                        int32_t off_mass, int32_t n_grid, const double *edges, double *map_out, const bfgx_opts *opts,
                                        bfgx_stats *stats);
/* resident form: the model and the halo-cell workspace live in a plan (one per box / redshift / model); all columns and
 * outputs are device pointers (out may not alias in); blocking (two small read-backs) */
typedef struct bfgx_snapshot_plan bfgx_snapshot_plan;
int  bfgx_snapshot_plan_create(int device, void *hip_stream, const bfgx_model *model, int32_t ndim, double L, double redshift,
                               int64_t max_halos, bfgx_snapshot_plan **out);
void bfgx_snapshot_plan_destroy(bfgx_snapshot_plan *p);
int  bfgx_snapshot_displace_device(bfgx_snapshot_plan *p, const bfgx_grid_catalog *halos_dev, int64_t n_part, const double *x_dev,
                                   const double *y_dev, const double *z_dev, double *x_out_dev, double *y_out_dev, double *z_out_dev,
                                   int64_t *n_pairs_host);
/* BaryonifySnapshot.process() (SnapshotRunner.py:173-262) followed by ParticleSnapshot.make_map(n_grid) (io.py:622-670) of the result,
 * for a caller who wants the MAP of the displaced particles and not the particles: map_out_dev [n_grid^ndim] float64 = np.histogramdd of the
 * displaced, re-wrapped positions on edges_dev [n_grid + 1] with weights mass_dev (NULL: unit masses).  The displaced coordinates are never
 * stored: the displacement kernel writes the deposit's sort keys.  BFGX_ERR_UNSUPPORTED for grids the tile-owned deposit does not take
 * (call bfgx_snapshot_displace_device + bfgx_deposit_particles_device then).  Blocking like bfgx_snapshot_displace_device. */
int  bfgx_snapshot_displace_deposit_device(bfgx_snapshot_plan *p, const bfgx_grid_catalog *halos_dev, int64_t n_part, const double *x_dev,
                                           const double *y_dev, const double *z_dev, const double *mass_dev, int32_t n_grid,
                                           const double *edges_dev, double *map_out_dev, int64_t *n_pairs_host);
/* one call = plan create + displace + destroy */
int bfgx_baryonify_snapshot_device(int device, void *hip_stream, const bfgx_grid_catalog *halos_dev, const bfgx_model *model,
                                   const bfgx_snapshot *snap_dev, double *x_out_dev, double *y_out_dev, double *z_out_dev,
                                   int64_t *n_pairs_host);

/* ---- models that are Python callables --------------------------------------------------------------
 * The reference calls model.displacement(r_sep / a_j, M_j, a_j) (HealpixRunner.py:321) / model.projected(cosmo, r_sep / a_j, M_j, a_j)
 * (:441) once per halo on ANY object.  For a model that carries no table the binding serves it exactly so:
 *   begin   the halos' discs on the device (`model` carries the runner's cosmology / mass definition / epsilon_max; its 3-axis table must be
 *           valid and is ignored); counts_host[n] = pixels of every halo's disc (4 for BaryonifyShell's < 4-pixel fallback, :309-310)
 *   radii   r_host[sum counts] = r_sep / a_j of every (halo, pixel) pair, halo j's at the exclusive prefix sum of the counts
 *   (the caller evaluates its model per halo on that halo's slice of r_host)
 *   apply   vals_host[sum counts] = what the model returned.  paint = 0: offset = value a diff / r_sep, non-finite components -> 0, accumulated
 *           in the pixels' unit vectors (:321-331), then the regrid of map_in into map_out (:333-341) and the mass check (:344-346: BFGX_ERR_MASS);
 *           paint = 1: map_out[pixel] += value, non-finite -> 0 (:441-445; map_in ignored).  fp64 throughout.
 *   end     frees the handle (also after an error). */
typedef struct bfgx_pairs bfgx_pairs;
int  bfgx_shell_pairs_begin(const bfgx_catalog *cat_host, const bfgx_model *model, int64_t nside, int32_t paint, int32_t device, bfgx_pairs **out,
                            int64_t *counts_host);
int  bfgx_shell_pairs_radii(bfgx_pairs *h, double *r_host);
int  bfgx_shell_pairs_apply(bfgx_pairs *h, const double *vals_host, const double *map_in, double *map_out, int32_t check_mass, bfgx_stats *stats);
void bfgx_shell_pairs_end(bfgx_pairs *h);

/* The regular-grid runners serve such a model the same way, through a bfgx_pairs handle of their own: BaryonifyGrid calls
 * model.displacement(r, M_j, a_j) and PaintProfilesGrid profile(cosmo, r, M_j, a_j) once per halo on r_grid.flatten() of the halo's WHOLE
 * Nsize^d cutout (Map2DRunner.py:534, :577, :801; no cut: a callable declares none), in the reference's order (meshgrid indexing='xy', first
 * axis around x_cen).  Halo ranges [j0, j1) let the caller hold one batch of radii / values at a time.
 *   begin   paint = 0: BaryonifyGrid (R_q clipped to max(bins)/2, halos with Nsize < 2 skipped: count 0, :487-498); paint = 1: PaintProfilesGrid
 *           (Nsize clipped to [2, npix/2], :726-728).  counts_host[n] = Nsize^ndim of every halo.  cat_host->rmat = use_ellipticity (2D only);
 *           `model` as for the shell entries (grid runners: cosmo_runner with w0 = -1).  BFGX_ERR_ASSERT: the 2D offset assert (:516, :747)
 *   radii   r_host[off[j1] - off[j0]] = the radii of halos [j0, j1) (sheared with use_ellipticity, :525-530), off = exclusive prefix sum of
 *           the counts; bit for bit numpy's without ellipticity
 *   apply   vals_host (same layout) = what the model returned for halos [j0, j1); accumulated on the device, once per range: paint = 0:
 *           value / res along the unsheared unit vector (:534-536, :577-579); paint = 1: value where isfinite(value) & r < eps * R_j (:800-812)
 *   finish  paint = 0: non-finite offsets -> 0, regrid of map_in into map_out (:577-599), mass check (:601-605: BFGX_ERR_MASS);
 *           paint = 1: map_out = the painted map (map_in ignored)
 *   end     bfgx_shell_pairs_end's twin: frees the handle (also after an error). */
int  bfgx_grid_pairs_begin(const bfgx_grid_catalog *cat_host, const bfgx_model *model, const bfgx_grid *grid, int32_t paint, int32_t device,
                           bfgx_pairs **out, int64_t *counts_host);
int  bfgx_grid_pairs_radii(bfgx_pairs *h, int64_t j0, int64_t j1, double *r_host);
int  bfgx_grid_pairs_apply(bfgx_pairs *h, int64_t j0, int64_t j1, const double *vals_host);
int  bfgx_grid_pairs_finish(bfgx_pairs *h, const double *map_in, double *map_out, int32_t check_mass, bfgx_stats *stats);
void bfgx_grid_pairs_end(bfgx_pairs *h);

/* BaryonifySnapshot calls model.displacement(d, M_j, a_j) once per halo on the distances of the particles within R_q = clip(eps * R_j / a,
 * 0, L/2) of it (SnapshotRunner.py:217-245), every halo, an empty array when none is inside.  Same five-call shape:
 *   begin   halos_host as for bfgx_baryonify_snapshot (float32-valued columns; lnM / rmat / extra ignored), `model` as for the shell entries
 *           (cosmo_runner with w0 = -1); counts_host[n] = particles of every halo: the containment test and the minimum-image separations are
 *           those of bfgx_baryonify_snapshot (d^2 <= R_q^2); within a halo the particles come in ascending index.  Particles outside [0, L]:
 *           BFGX_ERR_INVALID
 *   radii   r_host[off[j1] - off[j0]] = d of the pairs of halos [j0, j1), off = exclusive prefix sum of the counts
 *   apply   vals_host (same layout) = what the model returned; offset = value * a, non-finite -> 0, along the min-image unit vector, accumulated
 *           per particle on the device (once per range)
 *   finish  x / y (/ z) _out[n_particles] = position + offset, re-wrapped into [0, L] once (:254-262)
 *   end     frees the handle (also after an error). */
int  bfgx_snapshot_pairs_begin(const bfgx_grid_catalog *halos_host, const bfgx_model *model, const bfgx_snapshot *snap_host, int32_t device,
                               bfgx_pairs **out, int64_t *counts_host);
int  bfgx_snapshot_pairs_radii(bfgx_pairs *h, int64_t j0, int64_t j1, double *r_host);
int  bfgx_snapshot_pairs_apply(bfgx_pairs *h, int64_t j0, int64_t j1, const double *vals_host);
int  bfgx_snapshot_pairs_finish(bfgx_pairs *h, double *x_out, double *y_out, double *z_out, bfgx_stats *stats);
void bfgx_snapshot_pairs_end(bfgx_pairs *h);

/* ---- spherical-harmonic transforms of RING-ordered HEALPix maps (healpy.sphtfunc, spin 0, fp64) -------------------------
 * alm are complex128 in healpy order, index m (2 lmax + 1 - m) / 2 + l for 0 <= m <= mmax, m <= l <= lmax, stored as
 * interleaved (re, im) doubles.  1 <= nside <= 2048, 0 <= mmax <= lmax.  map2alm: alm = A(map), then `iter` times
 * alm += A(map - S(alm)), A(m) = 4 pi / Npix sum_p m_p Y*_lm(p); pixels within healpy's mask_bad tolerance of UNSEEN count as 0.
 * alm2map: map = sum_l a_l0 lambda_l0 + 2 Re sum_{m>0} a_lm lambda_lm e^{i m phi} (Im a_l0 ignored).
 * alm2cl: cl[l] = (Re a_l0 b*_l0 + 2 sum_{m=1}^{min(l, mmax)} Re a_lm b*_lm) / (2l + 1) for l <= min(lmax, lmax_out), 0 beyond
 * (alm2 NULL: auto-spectrum).
 * Device entries: work_dev holds bfgx_sht_work_doubles(nside, lmax, mmax) doubles (16-byte aligned; -1 = invalid shape), filled once
 * by bfgx_sht_prepare_device and reused by every transform of the same (nside, lmax, mmax); enqueue-only on hip_stream. */
int64_t bfgx_sht_work_doubles(int32_t nside, int32_t lmax, int32_t mmax);
int  bfgx_sht_prepare_device(int device, void *hip_stream, int32_t nside, int32_t lmax, int32_t mmax, double *work_dev);
int  bfgx_sht_map2alm_device(int device, void *hip_stream, int32_t nside, int32_t lmax, int32_t mmax, int32_t iter, const double *map_dev,
                             double *alm_dev, double *work_dev);
int  bfgx_sht_alm2map_device(int device, void *hip_stream, int32_t nside, int32_t lmax, int32_t mmax, const double *alm_dev,
                             double *map_dev, double *work_dev);
int  bfgx_sht_alm2cl_device(int device, void *hip_stream, int32_t lmax, int32_t mmax, int32_t lmax_out, const double *alm1_dev,
                            const double *alm2_dev, double *cl_dev);
/* almxfl (healpy.almxfl): alm_out[idx(l, m)] = alm_in[idx(l, m)] * fl[l], fl real, fl[l] = 0 for l >= nfl (entries beyond lmax are
 * ignored); one fp64 multiply per component.  alm_out may be alm_in.  0 <= mmax <= lmax <= 32767, nfl >= 0. */
int  bfgx_sht_almxfl_device(int device, void *hip_stream, int32_t lmax, int32_t mmax, int64_t nfl, const double *fl_dev,
                            const double *alm_in_dev, double *alm_out_dev);
int  bfgx_sht_almxfl(int device, int32_t lmax, int32_t mmax, int64_t nfl, const double *fl_host, const double *alm_in_host,
                     double *alm_out_host);
/* one-shot host entries (host arrays, PCIe included).  anafast: cl[lmax + 1]; alm1_out / alm2_out (optional) receive the alm */
int  bfgx_sht_map2alm(int device, int32_t nside, int32_t lmax, int32_t mmax, int32_t iter, const double *map_host, double *alm_host);
int  bfgx_sht_alm2map(int device, int32_t nside, int32_t lmax, int32_t mmax, const double *alm_host, double *map_host);
int  bfgx_sht_alm2cl(int device, int32_t lmax, int32_t mmax, int32_t lmax_out, const double *alm1_host, const double *alm2_host,
                     double *cl_host);
int  bfgx_sht_anafast(int device, int32_t nside, int32_t lmax, int32_t mmax, int32_t iter, const double *map1_host,
                      const double *map2_host, double *cl_host, double *alm1_out, double *alm2_out);

/* ---- spin-weighted transforms of a pair of RING maps (healpy.map2alm_spin / alm2map_spin, HEALPix/libsharp convention) ---------
 * map0 + i map1 = -sum_{l >= spin} sum_{m = -l..l} (G_lm + i C_lm) sY_lm, sY_lm = sqrt((l - s)! / (l + s)!) edth^s Y_lm; G and C are
 * the coefficients of real fields, stored like the spin-0 alm.  maps = map0 | map1 (2 npix doubles), alms = G | C (2 x alm size
 * complex128).  1 <= spin <= lmax; output alm with l < spin are 0, input alm with l < spin are ignored; no iterations (plain
 * quadrature, as healpy).  Device entries: work_dev as for the spin-0 entries (prepared by bfgx_sht_prepare_device), spin_work_dev
 * bfgx_sht_spin_work_doubles(nside, lmax, mmax) doubles of scratch (16-byte aligned; -1 = invalid shape); enqueue-only. */
int64_t bfgx_sht_spin_work_doubles(int32_t nside, int32_t lmax, int32_t mmax);
int  bfgx_sht_map2alm_spin_device(int device, void *hip_stream, int32_t nside, int32_t lmax, int32_t mmax, int32_t spin,
                                  const double *maps_dev, double *alms_dev, double *work_dev, double *spin_work_dev);
int  bfgx_sht_alm2map_spin_device(int device, void *hip_stream, int32_t nside, int32_t lmax, int32_t mmax, int32_t spin,
                                  const double *alms_dev, double *maps_dev, double *work_dev, double *spin_work_dev);
int  bfgx_sht_map2alm_spin(int device, int32_t nside, int32_t lmax, int32_t mmax, int32_t spin, const double *maps_host, double *alms_host);
int  bfgx_sht_alm2map_spin(int device, int32_t nside, int32_t lmax, int32_t mmax, int32_t spin, const double *alms_host, double *maps_host);

/* ---- HEALPix pixel functions (healpy.ud_grade, get_interp_weights, get_interp_val; the reference's regrid_pixels_hpix) ------------
 * Pixel indices are int64.  Map element types: dtype 0 = float32, 1 = float64.  Device entries take device pointers and enqueue on
 * hip_stream; host entries copy in and out (PCIe included).  Every argument is checked before any device call (BFGX_ERR_INVALID
 * names the limit); without a GPU the entries return BFGX_ERR_NO_DEVICE.
 * ud_grade: nmaps maps of 12 nside_in^2 pixels (row after row) -> nmaps maps of 12 nside_out^2 pixels; both nsides powers of two in
 *   [1, 8192]; nest_in / nest_out: 0 = RING, 1 = NEST.  Degrade: output = (sum of the good children) * ratio / (good children), where
 *   a child is bad if it is within healpy.mask_bad's tolerance of UNSEEN (-1.6375e30) or not finite; UNSEEN where no child is good
 *   (pess != 0: where any child is bad).  Sums are fp64 in a fixed order (bit-reproducible).  Upgrade: every child = parent * ratio.
 *   ratio = (nside_out / nside_in)^power, 1 without a power.
 * interp_weights: healpix_cxx get_interpol.  Points are (theta_dev[i], phi_dev[i]) in radians, or the centres of ipix_dev[i] (pixel
 *   indices in the ordering of nest) when theta and phi are NULL.  pix[4][n], w[4][n]; nest != 0 returns NEST indices and needs a
 *   power-of-two nside, RING takes any 1 <= nside <= 8192.  phi is reduced to [0, 2 pi).  Host entries refuse theta outside [0, pi],
 *   a non-finite phi and pixel indices outside [0, npix); device entries give such points pixels -1 and weights NaN.
 * interp_val: out[m][i] = sum_k maps[m][pix_k] w_k with the weights above (maps in the ordering of nest); NaN for invalid points
 *   on the device entry.
 * scatter_add: hmap[pix[i][j]] += w[i][j] * vals[i] for i < n, j < 4 (pix, w: [n][4]), fp64 atomic adds, so the last bits of a sum
 *   can differ from run to run.  Indices in [-npix, 0) wrap; the host entry refuses any other index outside [0, npix), the device
 *   entry skips it.
 * neighbours (healpy.get_all_neighbours of pixel indices): out[8][n], the neighbours of ipix[i] in the order SW, W, NW, N, NE, E, SE, S
 *   (healpix_cxx neighbors()), -1 where there is none (24 entries of a whole map).  nest / nside as for interp_weights.  The host entry
 *   refuses an index outside [0, npix); the device entry writes -1 for all 8. */
int  bfgx_hpx_neighbours_device(int device, void *hip_stream, int64_t nside, int32_t nest, int64_t n, const int64_t *ipix_dev,
                                int64_t *out_dev);
int  bfgx_hpx_neighbours(int device, int64_t nside, int32_t nest, int64_t n, const int64_t *ipix_host, int64_t *out_host);
int  bfgx_hpx_ud_grade_device(int device, void *hip_stream, int64_t nside_in, int64_t nside_out, int64_t nmaps, int32_t nest_in,
                              int32_t nest_out, int32_t pess, double ratio, int32_t dtype_in, int32_t dtype_out, const void *map_in_dev,
                              void *map_out_dev);
int  bfgx_hpx_ud_grade(int device, int64_t nside_in, int64_t nside_out, int64_t nmaps, int32_t nest_in, int32_t nest_out, int32_t pess,
                       double ratio, int32_t dtype_in, int32_t dtype_out, const void *map_in_host, void *map_out_host);
int  bfgx_hpx_interp_weights_device(int device, void *hip_stream, int64_t nside, int32_t nest, int64_t n, const double *theta_dev,
                                    const double *phi_dev, const int64_t *ipix_dev, int64_t *pix_dev, double *w_dev);
int  bfgx_hpx_interp_weights(int device, int64_t nside, int32_t nest, int64_t n, const double *theta_host, const double *phi_host,
                             const int64_t *ipix_host, int64_t *pix_host, double *w_host);
int  bfgx_hpx_interp_val_device(int device, void *hip_stream, int64_t nside, int32_t nest, int64_t nmaps, int32_t dtype, const void *maps_dev,
                                int64_t n, const double *theta_dev, const double *phi_dev, double *out_dev);
int  bfgx_hpx_interp_val(int device, int64_t nside, int32_t nest, int64_t nmaps, int32_t dtype, const void *maps_host, int64_t n,
                         const double *theta_host, const double *phi_host, double *out_host);
int  bfgx_hpx_scatter_add_device(int device, void *hip_stream, int64_t npix, double *hmap_dev, int64_t n, const double *vals_dev,
                                 const int64_t *pix_dev, const double *w_dev);
int  bfgx_hpx_scatter_add(int device, int64_t npix, double *hmap_host, int64_t n, const double *vals_host, const int64_t *pix_host,
                          const double *w_host);

/* ---- reductions over HEALPix maps: moments, cross-moments, peak counts, Minkowski sums (device entries, enqueue-only on hip_stream) -------------
 * A pixel is good if every map is finite and not UNSEEN there (healpy.mask_bad's tolerance) and mask_dev (optional, one byte per
 * pixel) is nonzero.
 * moments: maps_dev = nmaps maps of npix doubles, row after row, 1 <= nmaps <= 3, 2 <= order <= 4.  *n_dev = good pixels (exact);
 *   out_dev = mean[nmaps] | central[bfgx_mapstats_moment_terms(nmaps, order)], central = mean over the good pixels of
 *   prod_a (x_a - mean_a)^{e_a}.  THE ORDER of the exponent tuples (e_0, .., e_{nmaps-1}): total degree d = 2, 3, .., order; within a
 *   degree e_0 descending, then e_1 descending (e_{nmaps-1} = d - the rest).  nmaps = 2, order = 3: (2,0) (1,1) (0,2) (3,0) (2,1)
 *   (1,2) (0,3).  That is 3 values for nmaps = 1, 12 for 2 and 31 for 3 at order 4; bfgx_mapstats_moment_terms returns the number
 *   (-1 = invalid nmaps / order).  Two passes (means, then central products), fp64 block partials combined in a fixed order over a grid
 *   that depends on npix alone, no float atomics: a repeated call gives the same bits.  No good pixel: n = 0, every value NaN.
 *   work_dev: BFGX_MAPSTATS_WORK_DOUBLES doubles of scratch.
 * peaks: a pixel of a map (RING, or NEST with nest != 0 and a power-of-two nside; 1 <= nside <= 8192) is a maximum if it is strictly
 *   greater than every existing neighbour (bfgx_hpx_neighbours), a minimum if strictly less, and only if it and all of them are good.
 *   counts_dev[2][nb] (zeroed by the entry) = maxima | minima with edges[b] <= value < edges[b + 1]; values outside the edges are not
 *   counted.  edges_dev: nb + 1 ascending finite doubles on the device (1 <= nb <= 4096; the order is the caller's to check).
 *   flags_dev (optional, one int8 per pixel): +1 maximum, -1 minimum, 0 neither.  Integer atomics: the counts are exact.
 * peaks_2d: the same outputs for a square grid map_dev [n][n] (C order), 3 <= n <= 16384 (any n): the 8 neighbours of pixel (i, j) are
 *   (i + di, j + dj); periodic != 0 wraps both axes, periodic == 0 makes a pixel on the border never an extremum.  A pixel counts only
 *   if it and all 8 neighbours are good.  counts_dev, edges_dev, nb and flags_dev as for peaks.
 * minkowski: ders_dev = six maps of npix doubles, row after row, the derivatives of a map u in the orthonormal basis (e_theta, e_phi) in
 *   spin form: u, u_t, u_p, lap = u;tt + u;pp, q_plus = u;tt - u;pp, q_cross = 2 u;tp.  A pixel is good if all six are finite, u is not UNSEEN and the mask is nonzero.  With
 *   g2 = u_t^2 + u_p^2 and c = u_t u_p q_cross - lap g2 / 2 + q_plus (u_t^2 - u_p^2) / 2 (= 2 u_t u_p u;tp - u_t^2 u;pp - u_p^2 u;tt),
 *   over the good pixels with edges[b] <= u < edges[b + 1]:  counts_dev[b] = their number, sums_dev[0][b] = sum sqrt(g2),
 *   sums_dev[1][b] = sum c / g2 (a pixel with g2 = 0 adds 0); counts_dev[nb] = good pixels below edges[0], counts_dev[nb + 1] = at or
 *   above edges[nb], counts_dev[nb + 2] = all good pixels (int64 [nb + 3], zeroed by the entry; double [2][nb]).  edges_dev: nb + 1
 *   ascending finite doubles on the device, 1 <= nb <= 512.  The sums are fp64 block partials over a grid that depends on npix alone,
 *   added in a fixed order, no float atomics: a repeated call gives the same bits.  work_dev:
 *   bfgx_mapstats_minkowski_work_doubles(npix, nb) doubles of scratch (host arithmetic; -1 = invalid npix / nb). */
#define BFGX_MAPSTATS_WORK_DOUBLES 32768
int32_t bfgx_mapstats_moment_terms(int32_t nmaps, int32_t order);
int  bfgx_mapstats_moments_device(int device, void *hip_stream, int64_t npix, int32_t nmaps, int32_t order, const double *maps_dev,
                                  const uint8_t *mask_dev, int64_t *n_dev, double *out_dev, double *work_dev);
int  bfgx_mapstats_peaks_device(int device, void *hip_stream, int64_t nside, int32_t nest, const double *map_dev, const uint8_t *mask_dev,
                                int32_t nb, const double *edges_dev, int64_t *counts_dev, int8_t *flags_dev);
int  bfgx_mapstats_peaks_2d_device(int device, void *hip_stream, int64_t n, int32_t periodic, const double *map_dev, const uint8_t *mask_dev,
                                   int32_t nb, const double *edges_dev, int64_t *counts_dev, int8_t *flags_dev);
int64_t bfgx_mapstats_minkowski_work_doubles(int64_t npix, int32_t nb);
int  bfgx_mapstats_minkowski_device(int device, void *hip_stream, int64_t npix, const double *ders_dev, const uint8_t *mask_dev, int32_t nb,
                                    const double *edges_dev, int64_t *counts_dev, double *sums_dev, double *work_dev);

/* ---- mode-coupling matrices of a mask: pseudo-C_l of masked spin-0 and spin-2 maps ------------------------------
 * wl = W_0 .. W_lw, the (cross-)spectrum of the mask(s), 0 beyond lw.  With (l l' j; a b c) the Wigner 3j symbol, L = l + l' + j and
 * j from |l - l'| to min(l + l', lw):
 *   kind 0:  m0 = M00[l,l'] = (2l'+1)/(4 pi) sum (2j+1) W_j (l l' j; 0 0 0)^2
 *   kind 1:  m0 = M0+[l,l'] = (2l'+1)/(4 pi) sum (2j+1) W_j (l l' j; 0 0 0) (l l' j; 2 -2 0)
 *   kind 2:  m0 = M++[l,l'] = (2l'+1)/(4 pi) sum (2j+1) W_j (l l' j; 2 -2 0)^2 over even L,  m1 = M--: the same over odd L
 * so that <pseudo C^00> = M00 C^00, <C^0E> = M0+ C^0E, <C^EE> = M++ C^EE + M-- C^BB, <C^BB> = M-- C^EE + M++ C^BB and
 * <C^EB> = (M++ - M--) C^EB.  The matrices are (lmax + 1) x (lmax + 1) doubles, row-major; entries with |l - l'| > lw, and for kinds 1
 * and 2 rows and columns below 2, are exactly 0.  0 <= lmax <= 8191, 0 <= lw <= 16383; m1 is used by kind 2 alone (NULL otherwise).
 * fp64; every entry is computed once in a fixed order (no atomics): a repeated call gives the same bits.
 *   bfgx_pcl_coupling_device   wl and the matrices are device pointers; enqueue-only on hip_stream
 *   bfgx_pcl_coupling          host arrays: upload + kernel + download */
int  bfgx_pcl_coupling_device(int device, void *hip_stream, int32_t lmax, int32_t lw, int32_t kind, const double *wl_dev, double *m0_dev,
                              double *m1_dev);
int  bfgx_pcl_coupling(int device, int32_t lmax, int32_t lw, int32_t kind, const double *wl, double *m0, double *m1);

/* ---- halo-centred radial profiles of shell maps (MeasureProfilesShell) ------------------------------
 * The adjoint of PaintProfilesShell: for halo j the pixels of query_disc(nside, vec_j, R_j epsilon_max / D_j) (RING, no < 4-pixel fallback) at
 * separation r_sep = D_j |vec_pix - vec_j| (HealpixRunner.py:418-438) are binned in x = r_sep / a_j (comoving Mpc, :441) or, scaled != 0,
 * x = r_sep / R_j: pixel in bin b iff r_edges[b] <= x < r_edges[b + 1]; nb + 1 finite ascending edges >= 0, 1 <= nb <= 64.  A pixel counts
 * if its value is finite and not UNSEEN (healpy's mask_bad rule); for the shear pair both maps must pass.  Outputs, [n][nb] each:
 *   npix, sum                  counted pixels and the sum of map[pix]
 *   npix_shear, sum_t, sum_x   (g1 != NULL) gamma_t + i gamma_x = -(g1 + i g2) e^{-2 i phi}, (g1, g2) on (e_theta, e_phi) as map2alm_spin takes
 *                              them, phi the position angle of the direction towards the halo at the pixel; a pixel the halo sits on is left out
 * Invalid halos (disc radius not positive / finite, colatitude outside [0, pi], M not positive / finite, z <= -1) and empty discs give
 * all-zero rows.  `model` carries the runner's cosmology / mass definition / epsilon_max; its 3-axis table must be valid and is ignored.
 * fp64 throughout; every cell is written once (no atomics on the outputs).  The plan behind both entries is cached: a second call with the
 * same (device, nside, model) allocates nothing.
 *   bfgx_shell_profiles          catalog, maps, edges and outputs in host memory: upload + kernels + download
 *   bfgx_shell_profiles_device   maps and outputs are device pointers, the kernels run on hip_stream; catalog columns and r_edges are host
 *                                arrays (copied before the call returns); no host synchronisation of its own */
int  bfgx_shell_profiles(const bfgx_catalog *cat_host, const bfgx_model *model, int64_t nside, const double *map_host, const double *g1_host,
                         const double *g2_host, int32_t nb, const double *r_edges, int32_t scaled, int32_t device, int64_t *npix_host,
                         double *sum_host, int64_t *npix_shear_host, double *sum_t_host, double *sum_x_host);
int  bfgx_shell_profiles_device(int32_t device, void *hip_stream, const bfgx_catalog *cat_host, const bfgx_model *model, int64_t nside,
                                const double *map_dev, const double *g1_dev, const double *g2_dev, int32_t nb, const double *r_edges,
                                int32_t scaled, int64_t *npix_dev, double *sum_dev, int64_t *npix_shear_dev, double *sum_t_dev,
                                double *sum_x_dev);

/* ---- halo-centred radial profiles of particle snapshots (MeasureProfilesSnapshot) ------------------------------
 * The box counterpart of bfgx_shell_profiles.  For halo j the particles of BaryonifySnapshot's query ball -- minimum-image separation d with
 * the reference's roundings, d^2 <= R_q^2, R_q = clip(eps R_j / a, 0, L / 2), a = 1 / (1 + redshift), R_j / a the comoving radius of the mass
 * definition (SnapshotRunner.py:217-228) -- are binned in x = d (comoving Mpc, the box's unit) or, scaled != 0, x = d / (R_j / a): a particle is
 * in bin b iff r_edges[b] <= x < r_edges[b + 1]; nb + 1 finite ascending edges >= 0, 1 <= nb <= 64.  Outputs, row-major [n_halo][nb]:
 *   npart   particles of the cell (a particle with a non-finite weight is counted)
 *   sum     sum of the finite weights of the cell; NULL if and only if the weights are NULL (counts only)
 * Every (halo, bin) cell is written exactly once -- also for invalid halos (M not positive / finite, a non-finite coordinate: all-zero rows), halos
 * without particles and n_part = 0 -- so the outputs need no zero-fill; no atomics touch them: counts are exact and reproducible, sums are fp64 in
 * an order that can differ from run to run.  halos_host as for bfgx_snapshot_pairs_begin (float32-valued columns; lnM / rmat / extra ignored);
 * `model` carries the runner's cosmology (w0 = -1) / mass definition / epsilon_max, its 3-axis table must be valid and is ignored.  At most
 * 2^31 - 1 halos and 2^32 - 1 particles.  Particles outside [0, L] (NaN included): BFGX_ERR_INVALID, as for bfgx_snapshot_pairs_begin.
 *   bfgx_snapshot_profiles          everything in host memory: upload + kernels + download; nothing is in flight when it returns
 *   bfgx_snapshot_profiles_device   particle columns x / y (/ z, ndim 3) / w [n_part] and the outputs are device pointers, the kernels run on
 *                                   hip_stream; halo columns and r_edges are host arrays.  hip_stream is synchronised before the call returns
 *                                   (once for the [0, L] check, once before the workspace is released): the outputs are complete on return */
int  bfgx_snapshot_profiles(const bfgx_grid_catalog *halos_host, const bfgx_model *model, const bfgx_snapshot *snap_host,
                            const double *w_host /* NULL: counts only */, int32_t nb, const double *r_edges, int32_t scaled, int32_t device,
                            int64_t *npart /* [n_halo][nb] */, double *sum /* NULL iff w_host is NULL */);
int  bfgx_snapshot_profiles_device(int32_t device, void *hip_stream, const bfgx_grid_catalog *halos_host, const bfgx_model *model, int32_t ndim,
                                   double L, double redshift, int64_t n_part, const double *x_dev, const double *y_dev, const double *z_dev,
                                   const double *w_dev, int32_t nb, const double *r_edges, int32_t scaled, int64_t *npart_dev, double *sum_dev);

/* ---- halo-centred radial profiles of gridded maps (MeasureProfilesGrid) ----------------------------------------
 * The regular-grid counterpart of bfgx_shell_profiles and bfgx_snapshot_profiles.  map[i0, i1(, i2)] (C order, [npix]^ndim doubles) is the
 * pixel whose centre is (x, y(, z)) = (bins[i0], bins[i1](, bins[i2])): where the grid runners put a halo, and what ParticleSnapshot.make_map
 * produces.  res = bins[1] - bins[0]; the bins must be uniformly spaced (to 1e-9 res): the period is L = npix res.  a = 1 / (1 + redshift).
 * A halo is valid iff M > 0 and M and its coordinates in use are finite; R_com = radius of the mass definition / a and
 * R_q = clip(eps R_com, 0, max(bins) / 2), BaryonifyGrid's own clip.  Per axis Delta_k = bins[i_k] - x_k, minus L where Delta_k > L / 2, plus L
 * where Delta_k < -L / 2; d = sqrt(sum Delta_k^2), the true minimum-image distance (NOT the reference's cutout linspace(-N/2, N/2, N) res,
 * which stretches radii by N / (N - 1) and swaps the sub-pixel dx and dy).  A pixel belongs to halo j iff d^2 <= R_q^2 (at most once:
 * R_q < L / 2); x = d (comoving Mpc) or, scaled != 0, d / R_com; it is in bin b iff r_edges[b] <= x < r_edges[b + 1]; nb + 1 finite ascending
 * edges >= 0, 1 <= nb <= 64.  Outputs, row-major [n_halo][nb]:
 *   npix, sum                  pixels of the cell whose map value is finite, and the sum of those values
 *   npix_shear, sum_t, sum_x   2D grids with a pair (g1, g2): pixels with finite g1 and g2 and d > 0, and the sums of
 *                              gamma_t = -(g1 c2 + g2 s2), gamma_x = g1 s2 - g2 c2, c2 = (Dx^2 - Dy^2) / d^2, s2 = 2 Dx Dy / d^2, i.e.
 *                              gamma_t + i gamma_x = -(g1 + i g2) e^{-2 i phi}, phi from +x towards +y: a mass peak has gamma_t > 0.
 *                              All three NULL if and only if g1 and g2 are NULL; a pair on a 3D grid is refused
 * Every (halo, bin) cell of every output is written exactly once -- also for invalid halos (all-zero rows) and halos without pixels -- so the
 * outputs need no zero-fill; no atomics touch them: counts are exact and reproducible, sums are fp64 in an order that can differ from run to
 * run.  halos_host: float32-valued columns M, x, y(, z) (lnM / rmat / extra ignored); `model` carries the runner's cosmology (w0 = -1) / mass
 * definition / epsilon_max, its 3-axis table must be valid and is ignored.  At most 2^31 - 1 halos.
 *   bfgx_grid_profiles          everything in host memory: upload + kernels + download; nothing is in flight when it returns
 *   bfgx_grid_profiles_device   the maps and the outputs are device pointers, the kernels run on hip_stream; halo columns, bins and r_edges
 *                               are host arrays.  hip_stream is synchronised before the call returns (the workspace is released): the
 *                               outputs are complete on return */
int  bfgx_grid_profiles(const bfgx_grid_catalog *halos_host, const bfgx_model *model, const bfgx_grid *grid, const double *map_host,
                        const double *g1_host, const double *g2_host, int32_t nb, const double *r_edges, int32_t scaled, int32_t device,
                        int64_t *npix, double *sum, int64_t *npix_shear, double *sum_t, double *sum_x);
int  bfgx_grid_profiles_device(int32_t device, void *hip_stream, const bfgx_grid_catalog *halos_host, const bfgx_model *model,
                               const bfgx_grid *grid, const double *map_dev, const double *g1_dev, const double *g2_dev, int32_t nb,
                               const double *r_edges, int32_t scaled, int64_t *npix_dev, double *sum_dev, int64_t *npix_shear_dev,
                               double *sum_t_dev, double *sum_x_dev);

/* ---- device math probe (test infrastructure) --------------------------------------------------------
 * Evaluates ONE of the fp64 device functions of csrc/bfgx_math.hpp elementwise, one thread per element, every argument loaded from
 * memory, so that tests can hold each function to its stated bound against a high-precision reference.  No product path calls it.
 * a, b, out0, out1: host arrays of n doubles.  b is needed by the two-argument functions only (NULL otherwise), out1 by the
 * sincos functions only (out0 = sin, out1 = cos).  Checked before any device call, BFGX_ERR_INVALID: a NULL pointer among those
 * the function needs, an unknown fn, n < 0 or n > 2^22.  n == 0 returns BFGX_OK and launches nothing. */
enum bfgx_math_fn {
    BFGX_MATH_RCP = 0,               /* fast_rcp(a) */
    BFGX_MATH_RSQ = 1,               /* fast_rsq(a) */
    BFGX_MATH_SQRT = 2,              /* fast_sqrt(a) */
    BFGX_MATH_LOG = 3,               /* fast_log(a), literal constants */
    BFGX_MATH_LOG_KREG = 4,          /* fast_log(a), constants held in registers */
    BFGX_MATH_EXP = 5,               /* fast_exp(a) */
    BFGX_MATH_SINCOS_SMALL = 6,      /* sincos_small(a), literal constants */
    BFGX_MATH_SINCOS_SMALL_KREG = 7, /* sincos_small(a), constants held in registers */
    BFGX_MATH_SINCOS_BOUNDED = 8,    /* sincos_bounded(a) */
    BFGX_MATH_SINCOS_DPHI = 9,       /* sincos_dphi(a) */
    BFGX_MATH_ATAN_SMALL = 10,       /* atan_small(a) */
    BFGX_MATH_ASIN_SMALL = 11,       /* asin_small(a) */
    BFGX_MATH_ATAN2 = 12,            /* atan2_generic(y = a, x = b) */
    BFGX_MATH_MUL_ADD_NC = 13,       /* add_nc(mul_nc(a, b), c), c = out0 on input */
    BFGX_MATH_RING_THETA = 14        /* ring_theta_nolibm(nside = a, ring = b), 1 <= ring <= 4 nside - 1 */
};
int  bfgx_math_probe(int device, int32_t fn, int64_t n, const double *a, const double *b, double *out0, double *out1);

#ifdef __cplusplus
}
#endif
#endif /* BFGX_H */
