"""
Resident (inputs-already-in-HBM) front-end of the C ABI: a thin object around `bfgx_plan`.
Pointers are plain integers (e.g. `tensor.data_ptr()`), the stream a raw hipStream_t handle
(e.g. `torch.cuda.current_stream().cuda_stream`); this module does not import torch.

Used by bench.py and by the multi-GPU driver (parallel.py); the drop-in runners use the one-shot
host entry points instead.
"""
import ctypes as C

import numpy as np

from . import _lib


class ShellPlan(object):

    def __init__(self, model, keepalive, nside, max_halos, device=0, stream=0):
        self._keep = keepalive
        self.nside = int(nside)
        self.npix = 12 * self.nside * self.nside
        self.max_halos = int(max_halos)
        h = C.c_void_p()
        _lib.check(_lib.load().bfgx_plan_create(int(device), C.c_void_p(int(stream) or None), self.nside,
                                               self.max_halos, C.byref(model), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, '_h', None):
            try:
                _lib.load().bfgx_plan_destroy(self._h)
            except Exception:          # interpreter shutdown: module globals may already be gone
                pass
            self._h = None

    __del__ = close

    def offsets(self, cat_dev, offsets_ptr, acc_f64=False):
        """K0 + K1 (HealpixRunner.py:291-331): offsets[npix][3] += ..."""
        _lib.check(_lib.load().bfgx_offsets_device(self._h, C.byref(cat_dev), C.c_void_p(int(offsets_ptr)), int(acc_f64)))

    def regrid(self, map_in_ptr, offsets_ptr, map_out_ptr, sums_ptr=0, acc_f64=False):
        """K2 (HealpixRunner.py:333-346): map_out[npix] (zeroed) += regrid; sums[2] optional"""
        _lib.check(_lib.load().bfgx_regrid_device(self._h, C.c_void_p(int(map_in_ptr)), C.c_void_p(int(offsets_ptr)),
                                                 int(acc_f64), C.c_void_p(int(map_out_ptr)),
                                                 C.c_void_p(int(sums_ptr) or None)))

    def baryonify(self, cat_dev, map_in_ptr, offsets_work_ptr, map_out_ptr, sums_ptr=0, acc_f64=False):
        """K0 + K1 + K2 in one enqueue-only call (HealpixRunner.py:291-346 on device buffers); offsets_work: [npix][3] scratch"""
        _lib.check(_lib.load().bfgx_baryonify_device(self._h, C.byref(cat_dev), C.c_void_p(int(map_in_ptr)), C.c_void_p(int(offsets_work_ptr)),
                                                    int(acc_f64), C.c_void_p(int(map_out_ptr)), C.c_void_p(int(sums_ptr) or None)))

    def route_count(self, n, rings_ptr, ring_bounds, counts_ptr):
        """routing pass 1 (enqueue-only): counts[world] (int32, device) = halos whose ring range touches each rank's rings"""
        rb = np.ascontiguousarray(ring_bounds, dtype=np.int32)
        _lib.check(_lib.load().bfgx_route_count_device(self._h, int(n), C.c_void_p(int(rings_ptr) or None), int(rb.size - 1), rb.ctypes.data,
                                                      C.c_void_p(int(counts_ptr))))

    def route_fill(self, n, rings_ptr, ring_bounds, start, col_ptrs, cursor_ptr, rows_ptr):
        """routing pass 2 (enqueue-only): rows[start[j] ...] = packed rows (len(col_ptrs) doubles per halo) bound for rank j"""
        rb = np.ascontiguousarray(ring_bounds, dtype=np.int32)
        st = np.ascontiguousarray(start, dtype=np.int64)
        cols = (C.c_void_p * len(col_ptrs))(*[int(c) for c in col_ptrs])
        _lib.check(_lib.load().bfgx_route_fill_device(self._h, int(n), C.c_void_p(int(rings_ptr) or None), int(rb.size - 1), rb.ctypes.data,
                                                     st.ctypes.data, len(col_ptrs), cols, C.c_void_p(int(cursor_ptr)),
                                                     C.c_void_p(int(rows_ptr) or None)))

    def route_pack(self, n, rings_ptr, ring_bounds, blockcap, col_ptrs, cursor_ptr, blocks_ptr, overflow_ptr):
        """routing in one pass with nothing read back (enqueue-only): blocks[world][len(col_ptrs)][blockcap], rows a destination does not
        receive keep M = NaN (column 0); *overflow (int32, device, zeroed by the caller) is set when a block is too small"""
        rb = np.ascontiguousarray(ring_bounds, dtype=np.int32)
        cols = (C.c_void_p * len(col_ptrs))(*[int(c) for c in col_ptrs])
        _lib.check(_lib.load().bfgx_route_pack_device(self._h, int(n), C.c_void_p(int(rings_ptr) or None), int(rb.size - 1), rb.ctypes.data,
                                                     int(blockcap), len(col_ptrs), cols, C.c_void_p(int(cursor_ptr)), C.c_void_p(int(blocks_ptr)),
                                                     C.c_void_p(int(overflow_ptr))))

    def route_step(self, cat_dev, rank, ring_bounds, blockcap, col_ptrs, cursor_ptr, send_ptr, recv_ptr, overflow_ptr):
        """the routing of one resident multi-GPU step in one call (ring ranges + packing; two launches): send = (world - 1) blocks
        [len(col_ptrs)][blockcap] in rank order without this rank, recv = world blocks with this rank's own rows written into the LAST one"""
        rb = np.ascontiguousarray(ring_bounds, dtype=np.int32)
        cols = (C.c_void_p * len(col_ptrs))(*[int(c) for c in col_ptrs])
        _lib.check(_lib.load().bfgx_route_step_device(self._h, C.byref(cat_dev), int(rb.size - 1), int(rank), rb.ctypes.data, int(blockcap), len(col_ptrs), cols,
                                                     C.c_void_p(int(cursor_ptr)), C.c_void_p(int(send_ptr) or None), C.c_void_p(int(recv_ptr)),
                                                     C.c_void_p(int(overflow_ptr))))

    def set_catalog_blocks(self, rows, stride):
        """the catalogs of the following K0 launches are blocks [block][column][rows] (stride = columns x rows); rows = 0: plain columns"""
        _lib.check(_lib.load().bfgx_plan_set_catalog_blocks(self._h, int(rows), int(stride)))

    def offsets_regrid_bands(self, cat_dev, B0, B1, offsets_ptr, band0, band1, map_in_ptr, out_slice_ptr, sums_ptr=0, foreign_ptr=0, acc_f64=False):
        """K0 + K1 for the bands [B0, B1), the banded regrid of [band0, band1) into the slice, far deposits applied, sums: one enqueue-only call"""
        _lib.check(_lib.load().bfgx_offsets_regrid_bands_device(self._h, C.byref(cat_dev), int(B0), int(B1), C.c_void_p(int(offsets_ptr)), int(acc_f64),
                                                               int(band0), int(band1), C.c_void_p(int(map_in_ptr)), C.c_void_p(int(out_slice_ptr)),
                                                               C.c_void_p(int(sums_ptr) or None), C.c_void_p(int(foreign_ptr) or None)))

    def bands_max_offset2(self, band0, band1, out_ptr):
        """largest |offset|^2 (float32, device) of the slice offsets_bands() has just written for the bands [band0, band1): reduced
        from the per-tile maxima K1 leaves, no pass over the slice"""
        _lib.check(_lib.load().bfgx_bands_max_offset2_device(self._h, int(band0), int(band1), C.c_void_p(int(out_ptr))))

    def max_offset2(self, offsets_ptr, npixels, out_ptr, acc_f64=False):
        """enqueue-only: *out (float32, device) = largest |offset|^2 over npixels pixels of pix_offsets"""
        _lib.check(_lib.load().bfgx_max_offset2_device(self._h, C.c_void_p(int(offsets_ptr) or None), int(npixels), int(acc_f64),
                                                      C.c_void_p(int(out_ptr))))

    def tile_shape(self):
        """(rings per band, columns per tile): band b holds the rings [1 + b R, 1 + (b + 1) R)"""
        br, w = C.c_int32(0), C.c_int32(0)
        _lib.check(_lib.load().bfgx_plan_tile_shape(self._h, C.byref(br), C.byref(w)))
        return int(br.value), int(w.value)

    def disc_rings(self, cat_dev, rings_ptr):
        """per halo the ring range [first, last] (1-based, inclusive, 2 rings of margin) its disc can touch -> int32 [n][2]"""
        _lib.check(_lib.load().bfgx_disc_rings_device(self._h, C.byref(cat_dev), C.c_void_p(int(rings_ptr) or None)))

    def set_route_margin(self, rings):
        """disc_rings widens every halo's ring range by `rings` from now on (a rank that computes the bands next to its own as well)"""
        _lib.check(_lib.load().bfgx_plan_set_route_margin(self._h, int(rings)))

    def offsets_bands(self, cat_dev, band0, band1, offsets_slice_ptr, acc_f64=False):
        """K0 + K1 for the tiles of bands [band0, band1) only; the slice starts at the first pixel of band0 ([p1 - p0][3])"""
        _lib.check(_lib.load().bfgx_offsets_bands_device(self._h, C.byref(cat_dev), int(band0), int(band1), C.c_void_p(int(offsets_slice_ptr)),
                                                        int(acc_f64)))

    def paint_bands(self, cat_dev, band0, band1, map_slice_ptr, acc_f64=True):
        """K0 + K3 for the tiles of bands [band0, band1) only; the slice starts at the first pixel of band0"""
        _lib.check(_lib.load().bfgx_paint_bands_device(self._h, C.byref(cat_dev), int(band0), int(band1), C.c_void_p(int(map_slice_ptr)),
                                                      int(acc_f64)))

    def bands(self):
        """first RING pixel of every band of rings the tiling uses (+ npix): the unit of multi-GPU pixel ownership"""
        nb = C.c_int32(0)
        _lib.check(_lib.load().bfgx_plan_bands(self._h, C.byref(nb), None))
        first = np.zeros(nb.value + 1, dtype=np.int64)
        _lib.check(_lib.load().bfgx_plan_bands(self._h, C.byref(nb), first.ctypes.data))
        return first

    def reach_rings(self, max_offset):
        """rings of apron the banded regrid needs for summed pix_offsets whose largest |offset| is `max_offset` [rad]"""
        r = C.c_int32(0)
        _lib.check(_lib.load().bfgx_plan_reach_rings(self._h, float(max_offset), C.byref(r)))
        return int(r.value)

    def set_band_reach(self, rings):
        """every rank of a banded regrid must use the same apron (default 1 ring): see reach_rings"""
        _lib.check(_lib.load().bfgx_plan_set_band_reach(self._h, int(rings)))

    def band_apron(self, band0, band1):
        """pixel range [olo, ohi) of summed pix_offsets the owner of bands [band0, band1) needs: its pixels + the band
        reach (set_band_reach) in rings either side"""
        lo, hi = C.c_int64(0), C.c_int64(0)
        _lib.check(_lib.load().bfgx_plan_band_apron(self._h, int(band0), int(band1), C.byref(lo), C.byref(hi)))
        return int(lo.value), int(hi.value)

    def regrid_bands(self, band0, band1, map_in_ptr, offsets_ptr, olo, ohi, out_slice_ptr, sums_ptr=0, acc_f64=False):
        """K2 for the OUTPUT pixels of bands [band0, band1): offsets_ptr -> summed pix_offsets of pixels [olo, ohi) (band_apron),
        out_slice_ptr -> the bands' own pixels (stored once, no zero-fill).  Far deposits: far_fetch()."""
        _lib.check(_lib.load().bfgx_regrid_bands_device(self._h, int(band0), int(band1), C.c_void_p(int(map_in_ptr)),
                                                       C.c_void_p(int(offsets_ptr)), int(olo), int(ohi), int(acc_f64),
                                                       C.c_void_p(int(out_slice_ptr)), C.c_void_p(int(sums_ptr) or None)))

    def far_apply(self, out_slice_ptr, p0, p1, foreign_ptr=0):
        """enqueue-only: add the listed deposits that fall into pixels [p0, p1) to the slice; count the others into *foreign_ptr"""
        _lib.check(_lib.load().bfgx_plan_far_apply_device(self._h, C.c_void_p(int(out_slice_ptr)), int(p0), int(p1),
                                                         C.c_void_p(int(foreign_ptr) or None)))

    def far_fetch(self):
        """(pixels, values) of the deposits the last regrid listed instead of applying (banded regrid only); blocking"""
        n = C.c_int64(0)
        _lib.check(_lib.load().bfgx_plan_far_fetch(self._h, 0, None, None, C.byref(n)))
        if n.value == 0:
            return np.zeros(0, dtype=np.int64), np.zeros(0)
        pix, val = np.zeros(n.value, dtype=np.int64), np.zeros(n.value)
        _lib.check(_lib.load().bfgx_plan_far_fetch(self._h, n.value, pix.ctypes.data, val.ctypes.data, C.byref(n)))
        return pix, val

    def paint(self, cat_dev, map_out_ptr, acc_f64=True):
        """K0 + K3 (HealpixRunner.py:418-445).  acc_f64: True / 1 = fp64 throughout (double map), False / 0 = fp32 (float map),
        2 = fp32 pair math accumulated in fp64 into a double map"""
        _lib.check(_lib.load().bfgx_paint_device(self._h, C.byref(cat_dev), C.c_void_p(int(map_out_ptr)), int(acc_f64)))

    def count_pairs(self, cat_dev, fallback4=True, counts_ptr=0):
        tot = C.c_int64(0)
        _lib.check(_lib.load().bfgx_count_pairs_device(self._h, C.byref(cat_dev), int(fallback4),
                                                      C.c_void_p(int(counts_ptr) or None), C.byref(tot)))
        return int(tot.value)

    def precision(self, acc_f64=-1):
        """(BFGX_ACC_* a request resolves to on this plan, largest displacement of the plan's table in pixel sides of its NSIDE)"""
        r, d = C.c_int32(0), C.c_double(0.0)
        _lib.check(_lib.load().bfgx_plan_precision(self._h, int(acc_f64), C.byref(r), C.byref(d)))
        return int(r.value), float(d.value)

    def set_algo(self, algo):
        """1 = tile-owned LDS accumulators (default), 0 = one wave per halo + global float atomics"""
        _lib.check(_lib.load().bfgx_plan_set_algo(self._h, int(algo)))

    def status(self):
        _lib.check(_lib.load().bfgx_plan_status(self._h))

    def regrid_stats(self):
        """what the last full-map regrid did (blocking): far deposits listed, list overflowed, tiles run by the walking kernel, largest reach"""
        far, ovf, walked, reach = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _lib.check(_lib.load().bfgx_plan_regrid_stats(self._h, C.byref(far), C.byref(ovf), C.byref(walked), C.byref(reach)))
        return {"far_listed": int(far.value), "far_overflowed": bool(ovf.value), "tiles_walked": int(walked.value), "max_reach_rings": int(reach.value)}

    def ring_table(self, first=0, count=None, from_functions=False):
        """records [first, first + count) of the plan's ring table (bfgx_debug_ring_table; blocking) as a structured array; from_functions:
        the same rings evaluated afresh by the device functions the table was built from, the quotients (dphi .. inv_dth_dn) left 0"""
        if count is None:
            count = 4 * self.nside + 1 - first
        out = np.zeros(int(count), dtype=_lib.RING_REC)
        _lib.check(_lib.load().bfgx_debug_ring_table(self._h, int(bool(from_functions)), int(first), int(count), out.ctypes.data))
        return out

    def timing_enable(self, on=True):
        _lib.check(_lib.load().bfgx_plan_timing_enable(self._h, int(on)))

    def timing_read(self):
        """{kernel kind: (summed ms, launches)} since the last read; synchronises the stream"""
        ms = np.zeros(len(_lib.KERNEL_KINDS))
        n = np.zeros(len(_lib.KERNEL_KINDS), dtype=np.int64)
        _lib.check(_lib.load().bfgx_plan_timing_read(self._h, ms.ctypes.data, n.ctypes.data))
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(_lib.KERNEL_KINDS)}


def model_from_tables(axes, values, cosmo, eps_runner, eps_model=None, rdelta_sampling=False, log_values=False,
                      cosmo_model=None, massdef=(200.0, 'critical'), massdef_model=None):
    """bfgx_model from raw arrays: axes = [ln(1+z), ln M, ln r], values C-order."""
    table, keep = _lib.make_table(axes, values, rdelta_sampling, log_values,
                                  eps_model if eps_model is not None else eps_runner)
    m = _lib.bfgx_model()
    m.table = table
    m.cosmo_runner = _lib.make_cosmo(cosmo)
    m.cosmo_model = _lib.make_cosmo(cosmo_model if cosmo_model is not None else cosmo)
    m.massdef_runner = _lib.make_massdef(*massdef)
    m.massdef_model = _lib.make_massdef(*(massdef_model if massdef_model is not None else massdef))
    m.eps_runner = float(eps_runner)
    return m, keep


class GridPlan(object):
    """Resident front-end of the regular-grid path (`bfgx_grid_plan`): periodic 2D / 3D maps at one redshift."""

    def __init__(self, model, keepalive, bins, ndim, redshift, max_halos, device=0, stream=0):
        self._keep = keepalive
        self.ndim = int(ndim)
        self.npix = int(len(bins))
        self.ntot = self.npix ** self.ndim
        self.max_halos = int(max_halos)
        self.device = int(device)
        self.stream = int(stream)
        grid, gkeep = _lib.make_grid(bins, ndim, redshift)
        h = C.c_void_p()
        _lib.check(_lib.load().bfgx_grid_plan_create(self.device, C.c_void_p(self.stream or None), C.byref(grid),
                                                    self.max_halos, C.byref(model), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, '_h', None):
            try:
                _lib.load().bfgx_grid_plan_destroy(self._h)
            except Exception:
                pass
            self._h = None

    __del__ = close

    def offsets(self, cat_dev, offsets_ptr):
        """halo loop of BaryonifyGrid (Map2DRunner.py:476-575): offsets[npix^d][d] f64, zeroed then filled.
        Returns the number of contributing (halo, pixel) pairs."""
        n = C.c_int64(0)
        _lib.check(_lib.load().bfgx_grid_offsets_device(self._h, C.byref(cat_dev), C.c_void_p(int(offsets_ptr)), C.byref(n)))
        return int(n.value)

    def paint(self, cat_dev, map_out_ptr):
        """halo loop of PaintProfilesGrid (Map2DRunner.py:708-812)"""
        n = C.c_int64(0)
        _lib.check(_lib.load().bfgx_grid_paint_device(self._h, C.byref(cat_dev), C.c_void_p(int(map_out_ptr)), C.byref(n)))
        return int(n.value)

    def regrid(self, map_in_ptr, offsets_ptr, map_out_ptr, sums_ptr=0):
        """post-loop regrid (Map2DRunner.py:577-605): map_out zeroed then filled; sums[2] optional (zeroed by caller)"""
        _lib.check(_lib.load().bfgx_grid_regrid_device(self._h, C.c_void_p(int(map_in_ptr)), C.c_void_p(int(offsets_ptr)),
                                                      C.c_void_p(int(map_out_ptr)), C.c_void_p(int(sums_ptr) or None)))

    def baryonify(self, cat_dev, map_in_ptr, map_out_ptr, sums_ptr=0):
        """BaryonifyGrid.process() on device arrays as one cell-owned pass (no pix_offsets array): halos listed per block of cells,
        every cell sums its offsets in registers and is regridded at once.  Same map_out as offsets() + regrid() up to the order
        of fp64 sums.  Returns the number of contributing (halo, pixel) pairs."""
        n = C.c_int64(0)
        _lib.check(_lib.load().bfgx_grid_baryonify_device(self._h, C.byref(cat_dev), C.c_void_p(int(map_in_ptr)), C.c_void_p(int(map_out_ptr)),
                                                         C.c_void_p(int(sums_ptr) or None), C.byref(n)))
        return int(n.value)

    def deposit_baryonify(self, cat_dev, n_particles, x_ptr, y_ptr, z_ptr, mass_ptr, edges_ptr, map_in_ptr, map_out_ptr, sums_ptr=0):
        """ParticleSnapshot.make_map + BaryonifyGrid.process() in one call (device arrays): the histogram of the particles goes to
        map_in AND, as the start value of the cell-owned pass, to map_out while it is being stored -- the map is not read again to copy
        and sum it.  Returns the number of contributing (halo, pixel) pairs."""
        n = C.c_int64(0)
        _lib.check(_lib.load().bfgx_grid_deposit_baryonify_device(
            self._h, C.byref(cat_dev), int(n_particles), C.c_void_p(int(x_ptr)), C.c_void_p(int(y_ptr)), C.c_void_p(int(z_ptr) or None),
            C.c_void_p(int(mass_ptr) or None), C.c_void_p(int(edges_ptr)), C.c_void_p(int(map_in_ptr)), C.c_void_p(int(map_out_ptr)),
            C.c_void_p(int(sums_ptr) or None), C.byref(n)))
        return int(n.value)

    def set_slab(self, plane_lo, plane_n):
        """slab decomposition over GPUs: this plan owns the planes [plane_lo, plane_lo + plane_n) of the first array axis;
        offsets() / paint() then fill plane_n x npix (x npix) cells (pass the whole catalog), regrid_slab() regrids them"""
        _lib.check(_lib.load().bfgx_grid_plan_set_slab(self._h, int(plane_lo), int(plane_n)))

    def regrid_slab(self, map_in_ptr, offsets_ptr, apron, map_out_ptr, sums_ptr=0, missed_ptr=0):
        """regrid of the slab's source cells into map_out = slab + `apron` planes either side (zeroed by the call, periodic);
        *missed (int32, zeroed by the caller) is set if a deposit fell outside that buffer"""
        _lib.check(_lib.load().bfgx_grid_regrid_slab_device(self._h, C.c_void_p(int(map_in_ptr)), C.c_void_p(int(offsets_ptr)), int(apron),
                                                           C.c_void_p(int(map_out_ptr)), C.c_void_p(int(sums_ptr) or None),
                                                           C.c_void_p(int(missed_ptr) or None)))

    def timing_enable(self, on=True):
        _lib.check(_lib.load().bfgx_grid_plan_timing_enable(self._h, int(on)))

    def timing_read(self):
        ms = np.zeros(len(_lib.KERNEL_KINDS))
        n = np.zeros(len(_lib.KERNEL_KINDS), dtype=np.int64)
        _lib.check(_lib.load().bfgx_grid_plan_timing_read(self._h, ms.ctypes.data, n.ctypes.data))
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(_lib.KERNEL_KINDS)}


def deposit_particles_slab_device(x_ptr, y_ptr, z_ptr, mass_ptr, n, n_grid, edges_ptr, plane_lo, plane_n, map_out_ptr, ndim=3, device=0, stream=0):
    """ParticleSnapshot.make_map for the planes [plane_lo, plane_lo + plane_n) of the first axis (particles elsewhere are dropped)"""
    _lib.check(_lib.load().bfgx_deposit_particles_slab_device(int(device), C.c_void_p(int(stream) or None), int(ndim), int(n),
                                                             C.c_void_p(int(x_ptr)), C.c_void_p(int(y_ptr)), C.c_void_p(int(z_ptr) or None),
                                                             C.c_void_p(int(mass_ptr) or None), int(n_grid), C.c_void_p(int(edges_ptr)),
                                                             int(plane_lo), int(plane_n), C.c_void_p(int(map_out_ptr))))


def fft_slab_planes_device(map_ptr, n_grid, planes, work_ptr, device=0, stream=0):
    """slab P(k), step 1: transforms along the last two axes of `planes` planes; work = complex128 [planes][n][n/2+1]"""
    _lib.check(_lib.load().bfgx_fft_slab_planes_device(int(device), C.c_void_p(int(stream) or None), int(n_grid), int(planes),
                                                      C.c_void_p(int(map_ptr)), C.c_void_p(int(work_ptr))))


def fft_slab_axis0_pk_device(work_ptr, n_grid, ncols, col0, L, nk, pk_sum_ptr, k_sum_ptr, counts_ptr, device=0, stream=0):
    """slab P(k), step 3 (after the transpose): transform along the first axis of work [n][ncols][n/2+1] + partial bin sums"""
    _lib.check(_lib.load().bfgx_fft_slab_axis0_pk_device(int(device), C.c_void_p(int(stream) or None), int(n_grid), int(ncols), int(col0),
                                                        C.c_void_p(int(work_ptr)), float(L), int(nk), C.c_void_p(int(pk_sum_ptr)),
                                                        C.c_void_p(int(k_sum_ptr)), C.c_void_p(int(counts_ptr))))


def deposit_particles_device(x_ptr, y_ptr, z_ptr, mass_ptr, n, n_grid, edges_ptr, map_out_ptr, ndim=3, device=0, stream=0):
    """ParticleSnapshot.make_map on device-resident columns (io.py:622-670)"""
    _lib.check(_lib.load().bfgx_deposit_particles_device(int(device), C.c_void_p(int(stream) or None), int(ndim), int(n),
                                                        C.c_void_p(int(x_ptr)), C.c_void_p(int(y_ptr)),
                                                        C.c_void_p(int(z_ptr) or None), C.c_void_p(int(mass_ptr) or None),
                                                        int(n_grid), C.c_void_p(int(edges_ptr)), C.c_void_p(int(map_out_ptr))))


def deposit_cloud_device(x_ptr, y_ptr, z_ptr, mass_ptr, n, n_grid, L, order, map_out_ptr, ndim=3, device=0, stream=0, shift=0):
    """CIC (order 2) / TSC (order 3) mass assignment of device-resident columns on the periodic box [0, L]^ndim, enqueue-only; order as in
    WINDOW_ORDERS (a name is taken too).  map_out [n_grid^ndim] is stored whole.  shift=1: on the grid displaced by half a cell (every
    particle moved by +L / (2 n_grid) along every axis), the second grid of interlaced_power_spectrum."""
    if isinstance(order, str):
        order = WINDOW_ORDERS.get(order.lower(), 0)
    _lib.check(_lib.load().bfgx_deposit_cloud_shifted_device(int(device), C.c_void_p(int(stream) or None), int(ndim), int(n),
                                                            C.c_void_p(int(x_ptr) or None), C.c_void_p(int(y_ptr) or None),
                                                            C.c_void_p(int(z_ptr) or None), C.c_void_p(int(mass_ptr) or None),
                                                            int(n_grid), float(L), int(order), int(shift), C.c_void_p(int(map_out_ptr))))


def route_particles_count_device(x_ptr, n, n_grid, edges_ptr, world, owner_ptr, counts_ptr, device=0, stream=0):
    """pass 1 of the particle routing of a slab-decomposed grid (enqueue-only): owner[n] uint8, counts[world] int32"""
    _lib.check(_lib.load().bfgx_route_particles_count_device(int(device), C.c_void_p(int(stream) or None), int(n), C.c_void_p(int(x_ptr) or None), int(n_grid),
                                                            C.c_void_p(int(edges_ptr)), int(world), C.c_void_p(int(owner_ptr) or None), C.c_void_p(int(counts_ptr))))


def route_particles_fill_device(col_ptrs, n, owner_ptr, world, start, total, cursor_ptr, cols_out_ptr, device=0, stream=0):
    """pass 2: cols_out[c][start[d] + ...] = column c of the particles bound for rank d (len(col_ptrs) <= 4 columns)"""
    st = np.ascontiguousarray(start, dtype=np.int64)
    cp = (C.c_void_p * len(col_ptrs))(*[int(q) for q in col_ptrs])
    _lib.check(_lib.load().bfgx_route_particles_fill_device(int(device), C.c_void_p(int(stream) or None), int(n), len(col_ptrs), cp, C.c_void_p(int(owner_ptr) or None),
                                                           int(world), st.ctypes.data, int(total), C.c_void_p(int(cursor_ptr)), C.c_void_p(int(cols_out_ptr) or None)))


def fft_pitch(n_grid):
    """complex values per row of the half-spectrum work arrays: n/2 + 1 rounded up to whole 128-byte lines"""
    return int(_lib.load().bfgx_fft_pitch(int(n_grid)))


def power_spectrum_work_doubles(n_grid):
    """doubles of scratch power_spectrum_device needs (half spectrum, rows padded to whole 128-byte lines)"""
    return int(_lib.load().bfgx_power_spectrum_work_doubles(int(n_grid)))


def power_spectrum_device(map_ptr, n_grid, L, nk, work_ptr, pk_sum_ptr, k_sum_ptr, counts_ptr, device=0, stream=0):
    """FFT + |F|^2 + linear k-bins on a device-resident map; work = power_spectrum_work_doubles(n_grid) doubles of scratch"""
    _lib.check(_lib.load().bfgx_power_spectrum_device(int(device), C.c_void_p(int(stream) or None), int(n_grid),
                                                     C.c_void_p(int(map_ptr)), float(L), int(nk), C.c_void_p(int(work_ptr)),
                                                     C.c_void_p(int(pk_sum_ptr)), C.c_void_p(int(k_sum_ptr)),
                                                     C.c_void_p(int(counts_ptr))))


def power_spectrum(Map, Lbox, Nk=180, device=0):
    """P(k) summary of a cubic map as in examples/10_Reproduce_Schneider_deltaPk.ipynb (cells 12, 15): |FFT|^2 averaged in
    Nk linear bins between the fundamental and the Nyquist frequency.  Returns (k_cen, Pk, k_count)."""
    Map = _lib.f8(Map)
    if Map.ndim != 3 or len(set(Map.shape)) != 1:
        raise ValueError("power_spectrum needs a cubic 3-D map")
    pk, kc = np.empty(Nk), np.empty(Nk)
    cnt = np.empty(Nk, dtype=np.int64)
    _lib.check(_lib.load().bfgx_power_spectrum(int(device), Map.shape[0], Map.ctypes.data, float(Lbox), int(Nk),
                                              pk.ctypes.data, kc.ctypes.data, cnt.ctypes.data))
    return kc, pk, cnt


def _cuda_f8_cube(Map, what):
    """a CUDA float64 tensor holding a cubic 3-D map, contiguous (ValueError otherwise)"""
    import torch
    if not isinstance(Map, torch.Tensor) or not Map.is_cuda or Map.dtype != torch.float64:
        raise ValueError("%s needs a CUDA float64 tensor" % what)
    if Map.dim() != 3 or len(set(Map.shape)) != 1:
        raise ValueError("%s needs a cubic 3-D map" % what)
    return Map.contiguous()


def power_spectrum_tensor(Map, Lbox, Nk=180):
    """power_spectrum for a CUDA float64 tensor, analysed where it lies on the current stream.  Returns (k_cen, Pk, k_count) as numpy
    arrays, empty bins NaN."""
    import torch
    Map = _cuda_f8_cube(Map, "power_spectrum_tensor")
    N, Nk = int(Map.shape[0]), int(Nk)
    work = torch.empty(power_spectrum_work_doubles(N), dtype=torch.float64, device=Map.device)
    sums = torch.empty((2, max(Nk, 1)), dtype=torch.float64, device=Map.device)
    cnt = torch.empty(max(Nk, 1), dtype=torch.int64, device=Map.device)
    power_spectrum_device(Map.data_ptr(), N, Lbox, Nk, work.data_ptr(), sums[0].data_ptr(), sums[1].data_ptr(), cnt.data_ptr(),
                          device=Map.device.index or 0, stream=torch.cuda.current_stream(Map.device).cuda_stream)
    s, c = sums.cpu().numpy(), cnt.cpu().numpy()
    with np.errstate(divide='ignore', invalid='ignore'):
        return s[1] / c, s[0] / c, c


def cross_power_spectrum_work_doubles(n_grid):
    """doubles of scratch cross_power_spectrum_device needs (two half spectra)"""
    return int(_lib.load().bfgx_cross_power_spectrum_work_doubles(int(n_grid)))


def cross_power_spectrum_device(map_a_ptr, map_b_ptr, n_grid, L, nk, window_order, work_ptr, paa_sum_ptr, pbb_sum_ptr, pab_sum_ptr, k_sum_ptr,
                                counts_ptr, device=0, stream=0):
    """the sums of |F_A|^2, |F_B|^2, Re(F_A conj F_B), |k| and the counts per linear k-bin of two device-resident maps (which may be the
    same); work = cross_power_spectrum_work_doubles(n_grid) doubles of scratch; window_order 0, 1, 2, 3 = none, NGP, CIC, TSC"""
    _lib.check(_lib.load().bfgx_cross_power_spectrum_device(int(device), C.c_void_p(int(stream) or None), int(n_grid), C.c_void_p(int(map_a_ptr)),
                                                           C.c_void_p(int(map_b_ptr)), float(L), int(nk), int(window_order),
                                                           C.c_void_p(int(work_ptr)), C.c_void_p(int(paa_sum_ptr)), C.c_void_p(int(pbb_sum_ptr)),
                                                           C.c_void_p(int(pab_sum_ptr)), C.c_void_p(int(k_sum_ptr)), C.c_void_p(int(counts_ptr))))


def fft_slab_axis0_xpk_device(spec_a_ptr, work_b_ptr, n_grid, ncols, col0, L, nk, window_order, paa_sum_ptr, pbb_sum_ptr, pab_sum_ptr, k_sum_ptr,
                              counts_ptr, device=0, stream=0):
    """the last pass of a cross spectrum alone: spec_a [n][ncols][fft_pitch(n)] = map A's finished spectrum of the columns col0 .. of the
    middle axis, work_b = map B's before the transform along the first axis (neither is changed) -> partial bin sums"""
    _lib.check(_lib.load().bfgx_fft_slab_axis0_xpk_device(int(device), C.c_void_p(int(stream) or None), int(n_grid), int(ncols), int(col0),
                                                         C.c_void_p(int(spec_a_ptr)), C.c_void_p(int(work_b_ptr)), float(L), int(nk),
                                                         int(window_order), C.c_void_p(int(paa_sum_ptr)), C.c_void_p(int(pbb_sum_ptr)),
                                                         C.c_void_p(int(pab_sum_ptr)), C.c_void_p(int(k_sum_ptr)), C.c_void_p(int(counts_ptr))))


WINDOW_ORDERS = {'none': 0, 'ngp': 1, 'cic': 2, 'tsc': 3}


def cross_power_spectrum(MapA, MapB, Lbox, Nk=180, window=0, device=0):
    """Auto and cross power spectra of two cubic 3-D maps of one shape in the bins and units of power_spectrum (the unnormalised fftn).
    MapA, MapB: two numpy arrays, or two CUDA float64 torch tensors, which are analysed where they lie on the current stream.  window:
    0, 1, 2, 3 or 'none', 'ngp', 'cic', 'tsc' divides the mass-assignment window of that order out of every mode.  Returns a dict of numpy
    arrays: k (mean |k| per bin), paa, pbb, pab = <Re(F_A conj F_B)>, r = pab / sqrt(paa pbb), counts (modes per bin); empty bins NaN."""
    if isinstance(window, str):
        if window.lower() not in WINDOW_ORDERS:
            raise ValueError("cross_power_spectrum: window must be 0, 1, 2, 3 or 'none', 'ngp', 'cic', 'tsc'")
        p = WINDOW_ORDERS[window.lower()]
    else:
        if isinstance(window, bool) or window not in (0, 1, 2, 3):
            raise ValueError("cross_power_spectrum: window must be 0, 1, 2, 3 or 'none', 'ngp', 'cic', 'tsc'")
        p = int(window)
    Nk = int(Nk)
    dev_a = hasattr(MapA, 'data_ptr') and not isinstance(MapA, np.ndarray)
    dev_b = hasattr(MapB, 'data_ptr') and not isinstance(MapB, np.ndarray)
    if dev_a != dev_b:
        raise ValueError("cross_power_spectrum needs two numpy arrays or two CUDA float64 tensors, not one of each")
    if not dev_a:
        MapA, MapB = _lib.f8(MapA), _lib.f8(MapB)
        if MapA.ndim != 3 or len(set(MapA.shape)) != 1:
            raise ValueError("cross_power_spectrum needs cubic 3-D maps")
        if MapA.shape != MapB.shape:
            raise ValueError("cross_power_spectrum needs two maps of one shape")
        out = np.empty((4, max(Nk, 1)))
        cnt = np.empty(max(Nk, 1), dtype=np.int64)
        _lib.check(_lib.load().bfgx_cross_power_spectrum(int(device), MapA.shape[0], MapA.ctypes.data, MapB.ctypes.data, float(Lbox), Nk, p,
                                                        out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, out[3].ctypes.data,
                                                        cnt.ctypes.data))
        paa, pbb, pab, k = out
    else:
        import torch
        MapA, MapB = _cuda_f8_cube(MapA, "cross_power_spectrum"), _cuda_f8_cube(MapB, "cross_power_spectrum")
        if MapA.shape != MapB.shape or MapA.device != MapB.device:
            raise ValueError("cross_power_spectrum needs two maps of one shape on one device")
        N = int(MapA.shape[0])
        work = torch.empty(cross_power_spectrum_work_doubles(N), dtype=torch.float64, device=MapA.device)
        sums = torch.empty((4, max(Nk, 1)), dtype=torch.float64, device=MapA.device)
        cntd = torch.empty(max(Nk, 1), dtype=torch.int64, device=MapA.device)
        cross_power_spectrum_device(MapA.data_ptr(), MapB.data_ptr(), N, Lbox, Nk, p, work.data_ptr(), sums[0].data_ptr(), sums[1].data_ptr(),
                                    sums[2].data_ptr(), sums[3].data_ptr(), cntd.data_ptr(), device=MapA.device.index or 0,
                                    stream=torch.cuda.current_stream(MapA.device).cuda_stream)
        s, cnt = sums.cpu().numpy(), cntd.cpu().numpy()
        with np.errstate(divide='ignore', invalid='ignore'):
            paa, pbb, pab, k = s[0] / cnt, s[1] / cnt, s[2] / cnt, s[3] / cnt
    with np.errstate(divide='ignore', invalid='ignore'):
        r = pab / np.sqrt(paa * pbb)
    return {'k': k, 'paa': paa, 'pbb': pbb, 'pab': pab, 'r': r, 'counts': cnt}


def fft2_work_doubles(n):
    """doubles of scratch the 2-D entries below need (three half spectra [n][fft_pitch(n)]); 0 for an unsupported n"""
    return int(_lib.load().bfgx_fft2_work_doubles(int(n)))


def rfft2_device(map_ptr, n, work_ptr, spec_out_ptr, device=0, stream=0):
    """map [n][n] -> its half spectrum [n][fft_pitch(n)] complex, unnormalised (enqueue-only, like all 2-D entries here)"""
    _lib.check(_lib.load().bfgx_rfft2_device(int(device), C.c_void_p(int(stream) or None), int(n), C.c_void_p(int(map_ptr)),
                                            C.c_void_p(int(work_ptr)), C.c_void_p(int(spec_out_ptr))))


def irfft2_device(spec_ptr, n, scale, work_ptr, map_out_ptr, device=0, stream=0):
    """half spectrum [n][fft_pitch(n)] (kept) -> map [n][n], times `scale` (1 / n^2 inverts rfft2_device)"""
    _lib.check(_lib.load().bfgx_irfft2_device(int(device), C.c_void_p(int(stream) or None), int(n), C.c_void_p(int(spec_ptr)), float(scale),
                                             C.c_void_p(int(work_ptr)), C.c_void_p(int(map_out_ptr))))


def power_spectrum_2d_device(map_a_ptr, map_b_ptr, n, L, nk, window_order, work_ptr, paa_sum_ptr, pbb_sum_ptr, pab_sum_ptr, k_sum_ptr,
                             counts_ptr, device=0, stream=0):
    """cross_power_spectrum_device for two square 2-D maps (which may be the same): the five sums per linear k-bin"""
    _lib.check(_lib.load().bfgx_power_spectrum_2d_device(int(device), C.c_void_p(int(stream) or None), int(n), C.c_void_p(int(map_a_ptr)),
                                                        C.c_void_p(int(map_b_ptr)), float(L), int(nk), int(window_order),
                                                        C.c_void_p(int(work_ptr)), C.c_void_p(int(paa_sum_ptr)), C.c_void_p(int(pbb_sum_ptr)),
                                                        C.c_void_p(int(pab_sum_ptr)), C.c_void_p(int(k_sum_ptr)), C.c_void_p(int(counts_ptr))))


FILTER_KINDS_2D = {'gauss': 0, 'tophat': 1, 'table': 2}


def filter_map_2d_device(map_ptr, n, L, kind, param, table_k, table_b, work_ptr, map_out_ptr, device=0, stream=0):
    """map_out = irfft2(rfft2(map) b(k)); kind as in FILTER_KINDS_2D, param = sigma or R, (table_k, table_b) host arrays for 'table'"""
    kind = FILTER_KINDS_2D[kind] if isinstance(kind, str) else int(kind)
    tk = None if table_k is None else np.ascontiguousarray(table_k, dtype=np.float64)
    tb = None if table_b is None else np.ascontiguousarray(table_b, dtype=np.float64)
    _lib.check(_lib.load().bfgx_filter_map_2d_device(int(device), C.c_void_p(int(stream) or None), int(n), C.c_void_p(int(map_ptr)), float(L),
                                                    kind, float(param), None if tk is None else tk.ctypes.data,
                                                    None if tb is None else tb.ctypes.data, 0 if tk is None else int(tk.size),
                                                    C.c_void_p(int(work_ptr)), C.c_void_p(int(map_out_ptr))))


DERIVATIVE_KINDS_2D = dict(FILTER_KINDS_2D, unit=3)


def derivatives_2d_work_doubles(n, nder=6):
    """doubles of scratch of derivatives_2d_device: nder + 1 half spectra [n][fft_pitch(n)]; 0 for an unsupported n or nder"""
    return int(_lib.load().bfgx_derivatives_2d_work_doubles(int(n), int(nder)))


def derivatives_2d_device(spec_ptr, n, L, kind, param, table_k, table_b, nder, spin_form, work_ptr, ders_out_ptr, device=0, stream=0):
    """half spectrum [n][fft_pitch(n)] (kept) -> ders_out [nder][n][n], nder = 6: [u, u_x, u_y, u_xx, u_xy, u_yy] of the filtered map (or
    [u, u_x, u_y, lap, q_plus, q_cross] with spin_form), nder = 1: u alone; kind as in DERIVATIVE_KINDS_2D ('unit': no filter)"""
    kind = DERIVATIVE_KINDS_2D[kind] if isinstance(kind, str) else int(kind)
    tk = None if table_k is None else np.ascontiguousarray(table_k, dtype=np.float64)
    tb = None if table_b is None else np.ascontiguousarray(table_b, dtype=np.float64)
    _lib.check(_lib.load().bfgx_derivatives_2d_device(int(device), C.c_void_p(int(stream) or None), int(n), C.c_void_p(int(spec_ptr)), float(L),
                                                     kind, float(param), None if tk is None else tk.ctypes.data,
                                                     None if tb is None else tb.ctypes.data, 0 if tk is None else int(tk.size), int(nder),
                                                     int(bool(spin_form)), C.c_void_p(int(work_ptr)), C.c_void_p(int(ders_out_ptr))))


def peaks_2d_device(map_ptr, n, periodic, mask_ptr, nb, edges_ptr, counts_ptr, flags_ptr=0, device=0, stream=0):
    """maxima | minima of a square grid [n][n] per bin of their value: counts int64 [2][nb], optional int8 flags [n][n]"""
    _lib.check(_lib.load().bfgx_mapstats_peaks_2d_device(int(device), C.c_void_p(int(stream) or None), int(n), int(bool(periodic)),
                                                        C.c_void_p(int(map_ptr)), C.c_void_p(int(mask_ptr) or None), int(nb),
                                                        C.c_void_p(int(edges_ptr)), C.c_void_p(int(counts_ptr)),
                                                        C.c_void_p(int(flags_ptr) or None)))


def kappa_to_shear_2d_device(kappa_ptr, n, work_ptr, g1_out_ptr, g2_out_ptr, device=0, stream=0):
    """Kaiser-Squires, convergence [n][n] -> shear (g1, g2)"""
    _lib.check(_lib.load().bfgx_kappa_to_shear_2d_device(int(device), C.c_void_p(int(stream) or None), int(n), C.c_void_p(int(kappa_ptr)),
                                                        C.c_void_p(int(work_ptr)), C.c_void_p(int(g1_out_ptr)), C.c_void_p(int(g2_out_ptr))))


def shear_to_kappa_2d_device(g1_ptr, g2_ptr, n, work_ptr, kappa_e_out_ptr, kappa_b_out_ptr, device=0, stream=0):
    """Kaiser-Squires, shear (g1, g2) -> convergence E and B modes"""
    _lib.check(_lib.load().bfgx_shear_to_kappa_2d_device(int(device), C.c_void_p(int(stream) or None), int(n), C.c_void_p(int(g1_ptr)),
                                                        C.c_void_p(int(g2_ptr)), C.c_void_p(int(work_ptr)), C.c_void_p(int(kappa_e_out_ptr)),
                                                        C.c_void_p(int(kappa_b_out_ptr))))


def _window_order(window, what):
    """0 .. 3 of a window given as that number or as a name of WINDOW_ORDERS (ValueError otherwise)"""
    if isinstance(window, str):
        if window.lower() in WINDOW_ORDERS:
            return WINDOW_ORDERS[window.lower()]
    elif not isinstance(window, bool) and window in (0, 1, 2, 3):
        return int(window)
    raise ValueError("%s: window must be 0, 1, 2, 3 or 'none', 'ngp', 'cic', 'tsc'" % what)


def interlaced_power_spectrum_device(map1_ptr, map2_ptr, n_grid, L, nk, window_order, work_ptr, p_sum_ptr, p1_sum_ptr, k_sum_ptr, counts_ptr,
                                     device=0, stream=0):
    """the sums of w |F1 + Phi F2|^2 / 4 (p_sum) and of w |F1|^2 (p1_sum), of |k| and the counts per linear k-bin of two device-resident
    grids, the second deposited half a cell away; work = cross_power_spectrum_work_doubles(n_grid) doubles of scratch"""
    _lib.check(_lib.load().bfgx_interlaced_power_spectrum_device(int(device), C.c_void_p(int(stream) or None), int(n_grid), C.c_void_p(int(map1_ptr)),
                                                                C.c_void_p(int(map2_ptr)), float(L), int(nk), int(window_order),
                                                                C.c_void_p(int(work_ptr)), C.c_void_p(int(p_sum_ptr)), C.c_void_p(int(p1_sum_ptr)),
                                                                C.c_void_p(int(k_sum_ptr)), C.c_void_p(int(counts_ptr))))


def interlaced_power_spectrum(Map1, Map2, Lbox, Nk=180, window='tsc'):
    """P(k) of two grids of ONE particle set, Map2 deposited half a cell away from Map1 (deposit_cloud_device(..., shift=1)), combined in
    Fourier space so that the odd aliased images cancel, in the bins and units of power_spectrum; `window` as in cross_power_spectrum.
    Two numpy cubes (uploaded to device 0) or two CUDA float64 tensors, which are analysed where they lie on the current stream.  Returns
    a dict of numpy arrays: k, pk (the interlaced estimate), pk_grid1 (Map1 alone: the aliased estimate), counts; empty bins NaN."""
    import torch
    p = _window_order(window, "interlaced_power_spectrum")
    Nk = int(Nk)
    dev1 = hasattr(Map1, 'data_ptr') and not isinstance(Map1, np.ndarray)
    dev2 = hasattr(Map2, 'data_ptr') and not isinstance(Map2, np.ndarray)
    if dev1 != dev2:
        raise ValueError("interlaced_power_spectrum needs two numpy arrays or two CUDA float64 tensors, not one of each")
    if not dev1:
        Map1, Map2 = _lib.f8(Map1), _lib.f8(Map2)
        if Map1.ndim != 3 or len(set(Map1.shape)) != 1:
            raise ValueError("interlaced_power_spectrum needs cubic 3-D maps")
        if Map1.shape != Map2.shape:
            raise ValueError("interlaced_power_spectrum needs two maps of one shape")
        # (torch takes no read-only array: such a map is copied first)
        Map1, Map2 = (torch.from_numpy(m if m.flags.writeable else m.copy()).to('cuda:0') for m in (Map1, Map2))
    Map1, Map2 = _cuda_f8_cube(Map1, "interlaced_power_spectrum"), _cuda_f8_cube(Map2, "interlaced_power_spectrum")
    if Map1.shape != Map2.shape or Map1.device != Map2.device:
        raise ValueError("interlaced_power_spectrum needs two maps of one shape on one device")
    N = int(Map1.shape[0])
    work = torch.empty(cross_power_spectrum_work_doubles(N), dtype=torch.float64, device=Map1.device)
    sums = torch.empty((3, max(Nk, 1)), dtype=torch.float64, device=Map1.device)
    cntd = torch.empty(max(Nk, 1), dtype=torch.int64, device=Map1.device)
    interlaced_power_spectrum_device(Map1.data_ptr(), Map2.data_ptr(), N, Lbox, Nk, p, work.data_ptr(), sums[0].data_ptr(), sums[1].data_ptr(),
                                     sums[2].data_ptr(), cntd.data_ptr(), device=Map1.device.index or 0,
                                     stream=torch.cuda.current_stream(Map1.device).cuda_stream)
    s, cnt = sums.cpu().numpy(), cntd.cpu().numpy()
    with np.errstate(divide='ignore', invalid='ignore'):
        return {'k': s[2] / cnt, 'pk': s[0] / cnt, 'pk_grid1': s[1] / cnt, 'counts': cnt}


def particle_power_spectrum_work_doubles(n_grid):
    """doubles of scratch particle_power_spectrum_device needs (two maps and two half spectra)"""
    return int(_lib.load().bfgx_particle_power_spectrum_work_doubles(int(n_grid)))


def particle_power_spectrum_device(x_ptr, y_ptr, z_ptr, mass_ptr, n, n_grid, L, order, interlace, nk, work_ptr, p_sum_ptr, p1_sum_ptr, k_sum_ptr,
                                   counts_ptr, device=0, stream=0):
    """device-resident particle columns -> the four sums of interlaced_power_spectrum_device: deposit, shifted deposit, spectrum, enqueue-only;
    order 2 (CIC) or 3 (TSC), whose window is divided out; interlace=0: one deposit, the windowed auto spectrum in both p_sum and p1_sum"""
    _lib.check(_lib.load().bfgx_particle_power_spectrum_device(int(device), C.c_void_p(int(stream) or None), int(n), C.c_void_p(int(x_ptr) or None),
                                                              C.c_void_p(int(y_ptr) or None), C.c_void_p(int(z_ptr) or None),
                                                              C.c_void_p(int(mass_ptr) or None), int(n_grid), float(L), int(order), int(interlace),
                                                              int(nk), C.c_void_p(int(work_ptr)), C.c_void_p(int(p_sum_ptr)),
                                                              C.c_void_p(int(p1_sum_ptr)), C.c_void_p(int(k_sum_ptr)), C.c_void_p(int(counts_ptr))))


def particle_power_spectrum(coords, mass, N_grid, Lbox, Nk=180, assignment='tsc', interlace=True, normalize=False, subtract_shot_noise=False,
                            device=0):
    """P(k) of particles of the periodic box [0, Lbox]^3 up to the Nyquist frequency of a grid of N_grid cells per axis, without the maps
    ever leaving the device: CIC or TSC deposit (`assignment`), with interlace=True a second deposit half a cell away and the two grids
    combined in Fourier space (the odd aliased images cancel), the assignment's window divided out.  coords = (x, y, z) as numpy arrays
    or as CUDA float64 tensors (analysed where they lie on the current stream; `device` is then theirs); mass: likewise, or None for unit
    masses.  Particles with a coordinate outside [0, Lbox] are dropped, as make_map drops them.
    Returns a dict of numpy arrays k, pk, pk_grid1 (the first grid alone: the aliased estimate; equal to pk without interlacing), counts,
    and the floats shot_noise = sum m^2 and mass = sum m over the kept particles.  The defaults are in the units of power_spectrum (the
    unnormalised fftn of the mass grid); normalize=True multiplies pk, pk_grid1 and shot_noise by Lbox^3 / mass^2 (the spectrum of the
    density contrast); subtract_shot_noise=True subtracts shot_noise from pk and pk_grid1."""
    order = WINDOW_ORDERS.get(assignment.lower(), -1) if isinstance(assignment, str) else -1
    if order < 1:
        raise ValueError("particle_power_spectrum: assignment must be 'cic' or 'tsc', not %r" % (assignment,))
    if order == 1:
        raise ValueError("particle_power_spectrum: assignment 'ngp' has no interlaced form%s; use 'cic' or 'tsc'" % (
            "" if interlace else " and no entry here (make_map and power_spectrum give its spectrum)"))
    if len(coords) != 3:
        raise ValueError("particle_power_spectrum needs coords = (x, y, z): the spectra here are 3-D")
    Nk, N_grid, Lbox = int(Nk), int(N_grid), float(Lbox)
    on_dev = [hasattr(c, 'data_ptr') and not isinstance(c, np.ndarray) for c in coords]
    m_dev = mass is not None and hasattr(mass, 'data_ptr') and not isinstance(mass, np.ndarray)
    if any(on_dev) != all(on_dev) or (mass is not None and m_dev != on_dev[0]):
        raise ValueError("particle_power_spectrum needs numpy arrays or CUDA float64 tensors, not some of each")
    out = np.empty((3, max(Nk, 1)))
    cnt = np.empty(max(Nk, 1), dtype=np.int64)
    if not on_dev[0]:
        x, y, z = (_lib.f8(c).ravel() for c in coords)
        m = None if mass is None else _lib.f8(mass).ravel()
        if not (x.size == y.size == z.size and (m is None or m.size == x.size)):
            raise ValueError("particle_power_spectrum needs columns of one length")
        _lib.check(_lib.load().bfgx_particle_power_spectrum(int(device), x.size, x.ctypes.data, y.ctypes.data, z.ctypes.data,
                                                           None if m is None else m.ctypes.data, N_grid, Lbox, order, int(bool(interlace)), Nk,
                                                           out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, cnt.ctypes.data))
        pk, pk1, k = out
        with np.errstate(invalid='ignore'):
            keep = (x >= 0) & (x <= Lbox) & (y >= 0) & (y <= Lbox) & (z >= 0) & (z <= Lbox)
        mk = np.ones(int(keep.sum())) if m is None else m[keep]
        m_tot, shot = float(mk.sum()), float((mk * mk).sum())
    else:
        import torch
        cols = list(coords) + ([] if mass is None else [mass])
        for c in cols:
            if not isinstance(c, torch.Tensor) or not c.is_cuda or c.dtype != torch.float64 or c.dim() != 1:
                raise ValueError("particle_power_spectrum needs 1-D CUDA float64 tensors")
        if any(c.shape != cols[0].shape or c.device != cols[0].device for c in cols):
            raise ValueError("particle_power_spectrum needs columns of one length on one device")
        cols = [c.contiguous() for c in cols]
        x, y, z = cols[:3]
        m = None if mass is None else cols[3]
        dev = x.device
        n = int(x.shape[0])
        work = torch.empty(particle_power_spectrum_work_doubles(N_grid), dtype=torch.float64, device=dev)
        sums = torch.empty((3, max(Nk, 1)), dtype=torch.float64, device=dev)
        cntd = torch.empty(max(Nk, 1), dtype=torch.int64, device=dev)
        particle_power_spectrum_device(x.data_ptr() if n else 0, y.data_ptr() if n else 0, z.data_ptr() if n else 0,
                                       m.data_ptr() if (m is not None and n) else 0, n, N_grid, Lbox, order, int(bool(interlace)), Nk,
                                       work.data_ptr(), sums[0].data_ptr(), sums[1].data_ptr(), sums[2].data_ptr(), cntd.data_ptr(),
                                       device=dev.index or 0, stream=torch.cuda.current_stream(dev).cuda_stream)
        s, cnt = sums.cpu().numpy(), cntd.cpu().numpy()
        with np.errstate(divide='ignore', invalid='ignore'):
            pk, pk1, k = s[0] / cnt, s[1] / cnt, s[2] / cnt
        keep = (x >= 0) & (x <= Lbox) & (y >= 0) & (y <= Lbox) & (z >= 0) & (z <= Lbox)
        mk = keep.to(torch.float64) if m is None else torch.where(keep, m, torch.zeros_like(m))
        m_tot, shot = float(mk.sum()), float((mk * mk).sum())
    if subtract_shot_noise:
        pk, pk1 = pk - shot, pk1 - shot
    if normalize:
        norm = Lbox ** 3 / m_tot ** 2 if m_tot != 0 else float('nan')
        pk, pk1, shot = pk * norm, pk1 * norm, shot * norm
    return {'k': k, 'pk': pk, 'pk_grid1': pk1, 'counts': cnt, 'shot_noise': shot, 'mass': m_tot}


def fft_slab_axis0_device(work_ptr, n_grid, ncols, inverse=0, device=0, stream=0):
    """in-place complex transforms along the first axis of work [n][ncols][fft_pitch(n)]; inverse: exponent +i, unnormalised"""
    _lib.check(_lib.load().bfgx_fft_slab_axis0_device(int(device), C.c_void_p(int(stream) or None), int(n_grid), int(ncols),
                                                     C.c_void_p(int(work_ptr)), int(inverse)))


def ifft_slab_planes_device(work_ptr, n_grid, planes, map_out_ptr, device=0, stream=0):
    """the inverse of fft_slab_planes_device, unnormalised: complex work [planes][n][fft_pitch(n)] -> real map_out [planes][n][n];
    work is scratch afterwards"""
    _lib.check(_lib.load().bfgx_ifft_slab_planes_device(int(device), C.c_void_p(int(stream) or None), int(n_grid), int(planes),
                                                       C.c_void_p(int(work_ptr)), C.c_void_p(int(map_out_ptr))))


def bispectrum_work_doubles(n_grid, nbins):
    """doubles of scratch bispectrum_device needs (two half spectra, nbins real fields, partial sums); 0 outside the limits"""
    return int(_lib.load().bfgx_bispectrum_work_doubles(int(n_grid), int(nbins)))


def bispectrum_shell_fields_device(spec_ptr, n_grid, L, k_edges, unit, scratch_spec_ptr, fields_ptr, device=0, stream=0):
    """fields [nbins][n][n][n] = the unnormalised inverse transforms of the half spectrum spec [n][n][fft_pitch(n)] restricted to each
    k-bin (unit: of a spectrum of ones); scratch_spec: another half spectrum"""
    e = _lib.f8(k_edges)
    _lib.check(_lib.load().bfgx_bispectrum_shell_fields_device(int(device), C.c_void_p(int(stream) or None), int(n_grid), float(L), e.size - 1,
                                                              e.ctypes.data, C.c_void_p(int(spec_ptr)), int(unit),
                                                              C.c_void_p(int(scratch_spec_ptr)), C.c_void_p(int(fields_ptr))))


def bispectrum_device(map_ptr, n_grid, L, k_edges, triangles, work_ptr, b_sum_ptr, n_tri_ptr, pk_sum_ptr, n_modes_ptr, device=0, stream=0):
    """FFT bispectrum estimator on a device-resident map: b_sum[ntri], n_tri[ntri], pk_sum[nbins], n_modes[nbins] (device arrays);
    work = bispectrum_work_doubles(n_grid, nbins) doubles of scratch; k_edges and triangles [ntri][3] are host arrays"""
    e = _lib.f8(k_edges)
    t = np.ascontiguousarray(triangles, dtype=np.int32)
    _lib.check(_lib.load().bfgx_bispectrum_device(int(device), C.c_void_p(int(stream) or None), int(n_grid), C.c_void_p(int(map_ptr)), float(L),
                                                 e.size - 1, e.ctypes.data, t.size // 3, t.ctypes.data, C.c_void_p(int(work_ptr)),
                                                 C.c_void_p(int(b_sum_ptr)), C.c_void_p(int(n_tri_ptr)), C.c_void_p(int(pk_sum_ptr)),
                                                 C.c_void_p(int(n_modes_ptr))))


BISPECTRUM_MAX_BINS, BISPECTRUM_MAX_TRIANGLES = 32, 8192


def bispectrum_triangles(k_edges, kind='all'):
    """The bin triples i <= j <= l (int32 [ntri][3]) whose bins can hold a closed triangle: k_edges[l] < k_edges[i + 1] + k_edges[j + 1].
    kind: 'all', 'equilateral' (i = j = l) or 'isosceles' (i = j <= l)."""
    if kind not in ('all', 'equilateral', 'isosceles'):
        raise ValueError("bispectrum_triangles: kind must be 'all', 'equilateral' or 'isosceles'")
    e = _lib.f8(k_edges)
    nb = e.size - 1
    out = [(i, j, l) for i in range(nb) for j in range(i, nb) for l in range(j, nb)
           if e[l] < e[i + 1] + e[j + 1] and (kind == 'all' or (i == j and (kind == 'isosceles' or j == l)))]
    return np.array(out, dtype=np.int32).reshape(-1, 3)


def bispectrum(Map, Lbox, k_edges, triangles='all', normalize=False, device=0):
    """Bispectrum of a cubic 3-D map in the k-bins k_edges (FFT estimator; units of power_spectrum: the unnormalised fftn, no volume
    factors, unless normalize).  Map: a numpy array, or a CUDA float64 torch tensor, which is analysed where it lies.  triangles: a kind
    of bispectrum_triangles or an integer array [ntri][3] of bin indices.  Returns a dict of numpy arrays: k (bin centres), triangles,
    B = b_sum / n_tri (NaN where no closed triangle exists), n_tri, pk = pk_sum / n_modes (NaN for empty bins), n_modes.
    normalize: B times L^6 / N^9, pk times L^3 / N^6."""
    e = _lib.f8(k_edges)
    if e.ndim != 1 or e.size < 2:
        raise ValueError("bispectrum needs at least two bin edges")
    nb = e.size - 1
    if nb > BISPECTRUM_MAX_BINS:
        raise ValueError("bispectrum needs 1 <= nbins <= %d" % BISPECTRUM_MAX_BINS)
    tri = bispectrum_triangles(e, triangles) if isinstance(triangles, str) else np.ascontiguousarray(triangles, dtype=np.int32)
    if tri.ndim != 2 or tri.shape[1] != 3 or not 1 <= tri.shape[0] <= BISPECTRUM_MAX_TRIANGLES:
        raise ValueError("bispectrum needs triangles [ntri][3] with 1 <= ntri <= %d" % BISPECTRUM_MAX_TRIANGLES)
    on_device = hasattr(Map, 'data_ptr') and not isinstance(Map, np.ndarray)
    if not on_device:
        Map = _lib.f8(Map)
    if len(Map.shape) != 3 or len(set(Map.shape)) != 1:
        raise ValueError("bispectrum needs a cubic 3-D map")
    N, ntri = int(Map.shape[0]), tri.shape[0]
    if not on_device:
        b_sum, n_tri, pk_sum, n_modes = np.empty(ntri), np.empty(ntri), np.empty(nb), np.empty(nb)
        _lib.check(_lib.load().bfgx_bispectrum(int(device), N, Map.ctypes.data, float(Lbox), nb, e.ctypes.data, ntri, tri.ctypes.data,
                                              b_sum.ctypes.data, n_tri.ctypes.data, pk_sum.ctypes.data, n_modes.ctypes.data))
    else:
        import torch
        if not Map.is_cuda or Map.dtype != torch.float64:
            raise ValueError("bispectrum needs a numpy array or a CUDA float64 tensor")
        Map = Map.contiguous()
        nw = bispectrum_work_doubles(N, nb)
        if nw <= 0:
            raise NotImplementedError("n_grid must be a power of two with 8 <= n_grid <= 1024")
        work = torch.empty(nw, dtype=torch.float64, device=Map.device)
        res = torch.empty(2 * ntri + 2 * nb, dtype=torch.float64, device=Map.device)
        bispectrum_device(Map.data_ptr(), N, Lbox, e, tri, work.data_ptr(), res[:ntri].data_ptr(), res[ntri:2 * ntri].data_ptr(),
                          res[2 * ntri:2 * ntri + nb].data_ptr(), res[2 * ntri + nb:].data_ptr(), device=Map.device.index or 0,
                          stream=torch.cuda.current_stream(Map.device).cuda_stream)
        r = res.cpu().numpy()
        b_sum, n_tri, pk_sum, n_modes = r[:ntri], r[ntri:2 * ntri], r[2 * ntri:2 * ntri + nb], r[2 * ntri + nb:]
    with np.errstate(divide='ignore', invalid='ignore'):
        # (the counts are integers up to the rounding of the transforms: "none" is less than half a triangle)
        B = np.where(np.abs(n_tri) < 0.5, np.nan, b_sum / n_tri)
        pk = np.where(np.abs(n_modes) < 0.5, np.nan, pk_sum / n_modes)
    if normalize:
        B = B * (float(Lbox) ** 6 / float(N) ** 9)
        pk = pk * (float(Lbox) ** 3 / float(N) ** 6)
    return {'k': 0.5 * (e[:-1] + e[1:]), 'triangles': tri, 'B': B, 'n_tri': n_tri, 'pk': pk, 'n_modes': n_modes}


def baryonify_snapshot_device(model, halos_dev, part_ptrs, n_part, L, redshift, out_ptrs, device=0, stream=0):
    """BaryonifySnapshot on device-resident columns: part_ptrs / out_ptrs = (x, y[, z]) device pointers.
    Returns the number of displaced (halo, particle) pairs."""
    ndim = len(part_ptrs)
    s = _lib.bfgx_snapshot(ndim, 0, int(n_part), int(part_ptrs[0]), int(part_ptrs[1]), int(part_ptrs[2]) if ndim == 3 else None,
                           float(L), float(redshift))
    n = C.c_int64(0)
    _lib.check(_lib.load().bfgx_baryonify_snapshot_device(int(device), C.c_void_p(int(stream) or None), C.byref(halos_dev), C.byref(model),
                                                         C.byref(s), C.c_void_p(int(out_ptrs[0])), C.c_void_p(int(out_ptrs[1])),
                                                         C.c_void_p(int(out_ptrs[2])) if ndim == 3 else None, C.byref(n)))
    return int(n.value)


class SnapshotPlan(object):
    """Resident front-end of the particle-snapshot path (`bfgx_snapshot_plan`): the model and the halo-cell workspace stay
    on the device between calls."""

    def __init__(self, model, keepalive, ndim, L, redshift, max_halos, device=0, stream=0):
        self._keep = keepalive
        self.ndim = int(ndim)
        h = C.c_void_p()
        _lib.check(_lib.load().bfgx_snapshot_plan_create(int(device), C.c_void_p(int(stream) or None), C.byref(model), self.ndim,
                                                        float(L), float(redshift), int(max_halos), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, '_h', None):
            try:
                _lib.load().bfgx_snapshot_plan_destroy(self._h)
            except Exception:
                pass
            self._h = None

    __del__ = close

    def displace(self, halos_dev, n_part, part_ptrs, out_ptrs):
        """BaryonifySnapshot.process (SnapshotRunner.py:199-262) on device columns; returns the number of displaced pairs"""
        n = C.c_int64(0)
        z_in = C.c_void_p(int(part_ptrs[2])) if self.ndim == 3 else None
        z_out = C.c_void_p(int(out_ptrs[2])) if self.ndim == 3 else None
        _lib.check(_lib.load().bfgx_snapshot_displace_device(self._h, C.byref(halos_dev), int(n_part), C.c_void_p(int(part_ptrs[0])),
                                                            C.c_void_p(int(part_ptrs[1])), z_in, C.c_void_p(int(out_ptrs[0])),
                                                            C.c_void_p(int(out_ptrs[1])), z_out, C.byref(n)))
        return int(n.value)

    def displace_deposit(self, halos_dev, n_part, part_ptrs, mass_ptr, n_grid, edges_ptr, map_out_ptr):
        """BaryonifySnapshot.process() followed by ParticleSnapshot.make_map(n_grid) of the result (SnapshotRunner.py:173-262, io.py:622-670)
        when only the map is wanted: map_out [n_grid^ndim] float64 on the device; the displaced coordinates are never stored.  mass_ptr 0 =
        unit masses.  Returns the number of displaced pairs."""
        n = C.c_int64(0)
        z_in = C.c_void_p(int(part_ptrs[2])) if self.ndim == 3 else None
        _lib.check(_lib.load().bfgx_snapshot_displace_deposit_device(self._h, C.byref(halos_dev), int(n_part), C.c_void_p(int(part_ptrs[0])),
                                                                    C.c_void_p(int(part_ptrs[1])), z_in, C.c_void_p(int(mass_ptr) or None),
                                                                    int(n_grid), C.c_void_p(int(edges_ptr)), C.c_void_p(int(map_out_ptr)), C.byref(n)))
        return int(n.value)


# ---------------------------------------------------------------------------------------------- spherical-harmonic transforms
def sht_alm_size(lmax, mmax):
    """complex coefficients of healpy's alm layout: index m (2 lmax + 1 - m) / 2 + l, 0 <= m <= mmax, m <= l <= lmax"""
    return (mmax + 1) * (2 * lmax + 2 - mmax) // 2


def sht_work_doubles(nside, lmax, mmax):
    """doubles of the transform workspace (ring geometry, Bluestein kernels, lambda_mm prefactors, F_m per ring, one scratch map)"""
    n = int(_lib.load().bfgx_sht_work_doubles(int(nside), int(lmax), int(mmax)))
    if n < 0:
        raise ValueError(_lib.load().bfgx_last_error().decode('utf-8', 'replace'))
    return n


def sht_spin_work_doubles(nside, lmax, mmax):
    """doubles of the extra workspace of the spin transforms (F_m per ring of the second map)"""
    n = int(_lib.load().bfgx_sht_spin_work_doubles(int(nside), int(lmax), int(mmax)))
    if n < 0:
        raise ValueError(_lib.load().bfgx_last_error().decode('utf-8', 'replace'))
    return n


class ShtPlan(object):
    """Resident spherical-harmonic transforms of one shape (nside, lmax, mmax) on one device: the workspace (ring geometry,
    Bluestein kernels of the ring FFTs, recurrence prefactors, per-ring F_m and a scratch map) is allocated and filled once;
    the transforms below then allocate only their outputs (or nothing, with out=)."""

    def __init__(self, nside, lmax, mmax, device=0):
        import torch
        self.nside, self.lmax, self.mmax, self.device = int(nside), int(lmax), int(mmax), int(device)
        self.npix = 12 * self.nside * self.nside
        self.nalm = sht_alm_size(self.lmax, self.mmax)
        nw = sht_work_doubles(self.nside, self.lmax, self.mmax)
        L = _lib.load()
        if L.bfgx_device_count() <= 0:
            raise _lib.BfgxError("bfgx: no HIP device visible: libbfgx has no CPU fallback")
        self.dev = torch.device('cuda', self.device)
        self.work = torch.empty(nw, dtype=torch.float64, device=self.dev)
        self.spin_work = None                                 # F of a spin transform's second map, on the first spin call
        self.der_scratch = None                               # l-factors and scaled alm of alm2map_der_device, on its first call
        _lib.check(L.bfgx_sht_prepare_device(self.device, self._stream(), self.nside, self.lmax, self.mmax, C.c_void_p(self.work.data_ptr())))

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream or None)

    def map2alm_device(self, map_dev, iter=3, out=None):
        """complex128 alm [nalm] of a float64 RING map [npix] on the device"""
        import torch
        alm = out if out is not None else torch.empty(self.nalm, dtype=torch.complex128, device=self.dev)
        _lib.check(_lib.load().bfgx_sht_map2alm_device(self.device, self._stream(), self.nside, self.lmax, self.mmax, int(iter),
                                                      C.c_void_p(map_dev.data_ptr()), C.c_void_p(alm.data_ptr()),
                                                      C.c_void_p(self.work.data_ptr())))
        return alm

    def alm2map_device(self, alm_dev, out=None):
        """float64 RING map [npix] of complex128 alm [nalm] on the device"""
        import torch
        m = out if out is not None else torch.empty(self.npix, dtype=torch.float64, device=self.dev)
        _lib.check(_lib.load().bfgx_sht_alm2map_device(self.device, self._stream(), self.nside, self.lmax, self.mmax,
                                                      C.c_void_p(alm_dev.data_ptr()), C.c_void_p(m.data_ptr()),
                                                      C.c_void_p(self.work.data_ptr())))
        return m

    def almxfl_device(self, alm_dev, fl_dev, out=None):
        """alm [nalm] times fl[l] (a float64 device tensor; fl[l] = 0 beyond its end): healpy.almxfl.  out=alm_dev filters in place"""
        return almxfl_device(alm_dev, fl_dev, self.lmax, self.mmax, out=out, device=self.device)

    def alm2cl_device(self, alm1_dev, alm2_dev=None, lmax_out=None, out=None):
        """cl [lmax_out + 1] (auto- or cross-spectrum) of device alm"""
        return alm2cl_device(alm1_dev, alm2_dev, self.lmax, self.mmax, lmax_out, out=out, device=self.device)

    def _spin_work(self):
        if self.spin_work is None:
            import torch
            self.spin_work = torch.empty(sht_spin_work_doubles(self.nside, self.lmax, self.mmax), dtype=torch.float64, device=self.dev)
        return self.spin_work

    def map2alm_spin_device(self, maps_dev, spin, out=None):
        """complex128 [G, C] [2, nalm] of a pair of float64 RING maps [2, npix] on the device (spin >= 1)"""
        import torch
        alms = out if out is not None else torch.empty((2, self.nalm), dtype=torch.complex128, device=self.dev)
        _lib.check(_lib.load().bfgx_sht_map2alm_spin_device(self.device, self._stream(), self.nside, self.lmax, self.mmax, int(spin),
                                                           C.c_void_p(maps_dev.data_ptr()), C.c_void_p(alms.data_ptr()),
                                                           C.c_void_p(self.work.data_ptr()), C.c_void_p(self._spin_work().data_ptr())))
        return alms

    def alm2map_spin_device(self, alms_dev, spin, out=None):
        """float64 RING maps [2, npix] of complex128 [G, C] [2, nalm] on the device (spin >= 1)"""
        import torch
        maps = out if out is not None else torch.empty((2, self.npix), dtype=torch.float64, device=self.dev)
        _lib.check(_lib.load().bfgx_sht_alm2map_spin_device(self.device, self._stream(), self.nside, self.lmax, self.mmax, int(spin),
                                                           C.c_void_p(alms_dev.data_ptr()), C.c_void_p(maps.data_ptr()),
                                                           C.c_void_p(self.work.data_ptr()), C.c_void_p(self._spin_work().data_ptr())))
        return maps

    def _der_scratch(self):
        """(fl [3, lmax + 1], alms [2, nalm]): the factors sqrt(l(l+1)), -l(l+1), -sqrt((l+2)(l+1)l(l-1)) that turn the alm of u into
        those of its gradient, Laplacian and trace-free Hessian, and one [G, C] pair whose C stays 0; made on the first call"""
        if self.der_scratch is None:
            import torch
            l = np.arange(self.lmax + 1, dtype=np.float64)
            fl = np.stack([np.sqrt(l * (l + 1.0)), -l * (l + 1.0), -np.sqrt((l + 2.0) * (l + 1.0) * l * np.maximum(l - 1.0, 0.0))])
            self.der_scratch = (torch.from_numpy(fl).to(self.dev), torch.zeros((2, self.nalm), dtype=torch.complex128, device=self.dev))
        return self.der_scratch

    def alm2map_der_device(self, alm_dev, out):
        """the derivatives of the map u of complex128 alm [nalm] in the orthonormal basis (e_theta, e_phi), written into the float64
        RING maps out [3, npix] = [u, u_t, u_p] (u_t = d_theta u, u_p = d_phi u / sin theta) or out [6, npix] = those and the second
        covariant derivatives in spin form, lap = u;tt + u;pp, q_plus = u;tt - u;pp, q_cross = 2 u;tp: one spin-0, one spin-1 and,
        for six maps, another spin-0 and one spin-2 synthesis of the scaled alm.  Nothing is allocated after the first call."""
        fl, pair = self._der_scratch()
        self.alm2map_device(alm_dev, out=out[0])
        if self.lmax >= 1:
            self.almxfl_device(alm_dev, fl[0], out=pair[0])
            self.alm2map_spin_device(pair, 1, out=out[1:3])
        else:
            out[1:3].zero_()
        if out.shape[0] == 6:
            self.almxfl_device(alm_dev, fl[1], out=pair[0])
            self.alm2map_device(pair[0], out=out[3])
            if self.lmax >= 2:
                self.almxfl_device(alm_dev, fl[2], out=pair[0])
                self.alm2map_spin_device(pair, 2, out=out[4:6])
            else:
                out[4:6].zero_()
        return out


def alm2cl_device(alm1_dev, alm2_dev, lmax, mmax, lmax_out=None, out=None, device=0):
    import torch
    lmax_out = int(lmax) if lmax_out is None else int(lmax_out)
    cl = out if out is not None else torch.empty(lmax_out + 1, dtype=torch.float64, device=alm1_dev.device)
    stream = torch.cuda.current_stream(alm1_dev.device).cuda_stream
    _lib.check(_lib.load().bfgx_sht_alm2cl_device(int(device), C.c_void_p(stream or None), int(lmax), int(mmax), lmax_out,
                                                 C.c_void_p(alm1_dev.data_ptr()),
                                                 C.c_void_p(alm2_dev.data_ptr()) if alm2_dev is not None else None,
                                                 C.c_void_p(cl.data_ptr())))
    return cl


def almxfl_device(alm_dev, fl_dev, lmax, mmax, out=None, device=0):
    import torch
    res = out if out is not None else torch.empty_like(alm_dev)
    stream = torch.cuda.current_stream(alm_dev.device).cuda_stream
    _lib.check(_lib.load().bfgx_sht_almxfl_device(int(device), C.c_void_p(stream or None), int(lmax), int(mmax), int(fl_dev.numel()),
                                                 C.c_void_p(fl_dev.data_ptr()), C.c_void_p(alm_dev.data_ptr()),
                                                 C.c_void_p(res.data_ptr())))
    return res


_SHT_PLANS = {}


def sht_plan(nside, lmax, mmax, device=0):
    """the cached ShtPlan of a shape: a repeated call of the same shape allocates no new workspace"""
    key = (int(nside), int(lmax), int(mmax), int(device))
    p = _SHT_PLANS.get(key)
    if p is None:
        p = _SHT_PLANS[key] = ShtPlan(*key)
    return p


def sht_map2alm_host(map_, nside, lmax, mmax, iter, device=0):
    """one-shot host entry (map and alm cross PCIe)"""
    alm = np.empty(sht_alm_size(lmax, mmax), dtype=np.complex128)
    _lib.check(_lib.load().bfgx_sht_map2alm(int(device), int(nside), int(lmax), int(mmax), int(iter), map_.ctypes.data, alm.ctypes.data))
    return alm


def sht_alm2map_host(alm, nside, lmax, mmax, device=0):
    m = np.empty(12 * int(nside) ** 2)
    a = np.ascontiguousarray(alm, dtype=np.complex128)
    _lib.check(_lib.load().bfgx_sht_alm2map(int(device), int(nside), int(lmax), int(mmax), a.ctypes.data, m.ctypes.data))
    return m


def sht_map2alm_spin_host(maps, nside, lmax, mmax, spin, device=0):
    """one-shot host entry of map2alm_spin: float64 [2, npix] in, complex128 [G, C] [2, nalm] out (PCIe included)"""
    m = np.ascontiguousarray(maps, dtype=np.float64)
    alms = np.empty((2, sht_alm_size(lmax, mmax)), dtype=np.complex128)
    _lib.check(_lib.load().bfgx_sht_map2alm_spin(int(device), int(nside), int(lmax), int(mmax), int(spin), m.ctypes.data, alms.ctypes.data))
    return alms


def sht_alm2map_spin_host(alms, nside, lmax, mmax, spin, device=0):
    """one-shot host entry of alm2map_spin: complex128 [G, C] [2, nalm] in, float64 [2, npix] out"""
    a = np.ascontiguousarray(alms, dtype=np.complex128)
    m = np.empty((2, 12 * int(nside) ** 2))
    _lib.check(_lib.load().bfgx_sht_alm2map_spin(int(device), int(nside), int(lmax), int(mmax), int(spin), a.ctypes.data, m.ctypes.data))
    return m


def sht_almxfl_host(alm, fl, lmax, mmax, out=None, device=0):
    """one-shot host entry of almxfl: complex128 alm and float64 fl in, the filtered alm out (`out` may be `alm`)"""
    res = out if out is not None else np.empty(sht_alm_size(lmax, mmax), dtype=np.complex128)
    _lib.check(_lib.load().bfgx_sht_almxfl(int(device), int(lmax), int(mmax), int(fl.size), fl.ctypes.data, alm.ctypes.data, res.ctypes.data))
    return res


def sht_alm2cl_host(alm1, alm2, lmax, mmax, lmax_out, device=0):
    a = np.ascontiguousarray(alm1, dtype=np.complex128)
    b = None if alm2 is None else np.ascontiguousarray(alm2, dtype=np.complex128)
    cl = np.empty(int(lmax_out) + 1)
    _lib.check(_lib.load().bfgx_sht_alm2cl(int(device), int(lmax), int(mmax), int(lmax_out), a.ctypes.data,
                                          None if b is None else b.ctypes.data, cl.ctypes.data))
    return cl


def sht_anafast_host(map1, map2, nside, lmax, mmax, iter, want_alm=False, device=0):
    cl = np.empty(int(lmax) + 1)
    n = sht_alm_size(lmax, mmax)
    a1 = np.empty(n, dtype=np.complex128) if want_alm else None
    a2 = np.empty(n, dtype=np.complex128) if (want_alm and map2 is not None) else None
    _lib.check(_lib.load().bfgx_sht_anafast(int(device), int(nside), int(lmax), int(mmax), int(iter), map1.ctypes.data,
                                           None if map2 is None else map2.ctypes.data, cl.ctypes.data,
                                           None if a1 is None else a1.ctypes.data, None if a2 is None else a2.ctypes.data))
    return cl, a1, a2


# ---------------------------------------------------------------------------------------------- mode-coupling matrices of a mask
PCL_MAX_LMAX, PCL_MAX_LW = 8191, 16383      # include/bfgx.h bfgx_pcl_coupling


def pcl_coupling_host(wl, lmax, kind, device=0):
    """one-shot host entry: float64 wl [lw + 1] in, the matrix [lmax + 1, lmax + 1] of kind 0 (M00) or 1 (M0+), or the pair (M++, M--) of
    kind 2, out (PCIe included)"""
    w = np.ascontiguousarray(wl, dtype=np.float64)
    n = int(lmax) + 1
    m0 = np.empty((n, n))
    m1 = np.empty_like(m0) if int(kind) == 2 else None
    _lib.check(_lib.load().bfgx_pcl_coupling(int(device), int(lmax), w.size - 1, int(kind), w.ctypes.data, m0.ctypes.data,
                                            None if m1 is None else m1.ctypes.data))
    return m0 if m1 is None else (m0, m1)


def pcl_coupling_device(wl_dev, lmax, kind, device=0):
    """the same on the device: wl_dev a contiguous float64 CUDA tensor, the matrices CUDA tensors; enqueued on torch's current stream.
    (utils.pseudocl checks lmax against PCL_MAX_LMAX before it comes here, so that a call the C entry refuses allocates nothing.)"""
    import torch
    n = int(lmax) + 1
    m0 = torch.empty((n, n), dtype=torch.float64, device=wl_dev.device)
    m1 = torch.empty_like(m0) if int(kind) == 2 else None
    stream = torch.cuda.current_stream(wl_dev.device).cuda_stream
    _lib.check(_lib.load().bfgx_pcl_coupling_device(int(device), C.c_void_p(stream or None), int(lmax), wl_dev.numel() - 1, int(kind),
                                                   C.c_void_p(wl_dev.data_ptr()), C.c_void_p(m0.data_ptr()),
                                                   None if m1 is None else C.c_void_p(m1.data_ptr())))
    return m0 if m1 is None else (m0, m1)


def math_probe(fn_name, a, b=None, c=None, device=0):
    """One function of csrc/bfgx_math.hpp evaluated elementwise on the GPU (bfgx_math_probe; names in _lib.MATH_FN).  Returns one array,
    or (sin, cos) for the sincos functions.  'atan2' takes (a, b) = (y, x), 'mul_add_nc' computes a * b + c without contraction,
    'ring_theta' takes a = nside, b = ring.  Test infrastructure: no product path calls it."""
    if fn_name not in _lib.MATH_FN:
        raise ValueError("math_probe: unknown function %r" % (fn_name,))
    a = _lib.f8(a).ravel()
    two = fn_name in _lib.MATH_FN_TWO_ARGS
    if two != (b is not None) or (fn_name == 'mul_add_nc') != (c is not None):
        raise ValueError("math_probe: %s takes %s" % (fn_name, "(a, b, c)" if fn_name == 'mul_add_nc' else "(a, b)" if two else "(a)"))
    b = _lib.f8(b).ravel() if two else None
    out0 = _lib.f8(c).ravel().copy() if c is not None else np.empty(a.size)
    out1 = np.empty(a.size) if fn_name in _lib.MATH_FN_TWO_RESULTS else None
    if (two and b.size != a.size) or out0.size != a.size:
        raise ValueError("math_probe: arguments differ in length")
    _lib.check(_lib.load().bfgx_math_probe(int(device), _lib.MATH_FN[fn_name], a.size, a.ctypes.data, None if b is None else b.ctypes.data,
                                           out0.ctypes.data, None if out1 is None else out1.ctypes.data))
    return out0 if out1 is None else (out0, out1)
