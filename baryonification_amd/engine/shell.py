"""The HEALPix-shell path on device-resident inputs: `ShellPlan` around `bfgx_plan`, and the model record the plans are made from."""
import ctypes as C

import numpy as np

from .. import _lib
from ._plan import TimedPlan


def _ring_bounds(ring_bounds):
    """(world, address, keepalive) of the ring bounds of the ranks, int32 [world + 1]"""
    rb = np.ascontiguousarray(ring_bounds, dtype=np.int32)
    return rb.size - 1, rb.ctypes.data, rb


def _columns(col_ptrs):
    return (C.c_void_p * len(col_ptrs))(*[int(c) for c in col_ptrs])


class ShellPlan(TimedPlan):
    _destroy, _timing = 'bfgx_plan_destroy', 'bfgx_plan_timing'

    def __init__(self, model, keepalive, nside, max_halos, device=0, stream=0):
        self._keep = keepalive
        self.nside = int(nside)
        self.npix = 12 * self.nside * self.nside
        self.max_halos = int(max_halos)
        self._create('bfgx_plan_create', device, stream, self.nside, self.max_halos, model)

    def offsets(self, cat_dev, offsets_ptr, acc_f64=False):
        """K0 + K1 (HealpixRunner.py:291-331): offsets[npix][3] += ..."""
        _lib.call('bfgx_offsets_device', self._h, cat_dev, offsets_ptr, acc_f64)

    def regrid(self, map_in_ptr, offsets_ptr, map_out_ptr, sums_ptr=0, acc_f64=False):
        """K2 (HealpixRunner.py:333-346): map_out[npix] (zeroed) += regrid; sums[2] optional"""
        _lib.call('bfgx_regrid_device', self._h, map_in_ptr, offsets_ptr, acc_f64, map_out_ptr, sums_ptr)

    def baryonify(self, cat_dev, map_in_ptr, offsets_work_ptr, map_out_ptr, sums_ptr=0, acc_f64=False):
        """K0 + K1 + K2 in one enqueue-only call (HealpixRunner.py:291-346 on device buffers); offsets_work: [npix][3] scratch"""
        _lib.call('bfgx_baryonify_device', self._h, cat_dev, map_in_ptr, offsets_work_ptr, acc_f64, map_out_ptr, sums_ptr)

    def route_count(self, n, rings_ptr, ring_bounds, counts_ptr):
        """routing pass 1 (enqueue-only): counts[world] (int32, device) = halos whose ring range touches each rank's rings"""
        world, rb_ptr, rb = _ring_bounds(ring_bounds)
        _lib.call('bfgx_route_count_device', self._h, n, rings_ptr, world, rb_ptr, counts_ptr)

    def route_fill(self, n, rings_ptr, ring_bounds, start, col_ptrs, cursor_ptr, rows_ptr):
        """routing pass 2 (enqueue-only): rows[start[j] ...] = packed rows (len(col_ptrs) doubles per halo) bound for rank j"""
        world, rb_ptr, rb = _ring_bounds(ring_bounds)
        st = np.ascontiguousarray(start, dtype=np.int64)
        _lib.call('bfgx_route_fill_device', self._h, n, rings_ptr, world, rb_ptr, st.ctypes.data, len(col_ptrs), _columns(col_ptrs),
                  cursor_ptr, rows_ptr)

    def route_pack(self, n, rings_ptr, ring_bounds, blockcap, col_ptrs, cursor_ptr, blocks_ptr, overflow_ptr):
        """routing in one pass with nothing read back (enqueue-only): blocks[world][len(col_ptrs)][blockcap], rows a destination does not
        receive keep M = NaN (column 0); *overflow (int32, device, zeroed by the caller) is set when a block is too small"""
        world, rb_ptr, rb = _ring_bounds(ring_bounds)
        _lib.call('bfgx_route_pack_device', self._h, n, rings_ptr, world, rb_ptr, blockcap, len(col_ptrs), _columns(col_ptrs), cursor_ptr,
                  blocks_ptr, overflow_ptr)

    def route_step(self, cat_dev, rank, ring_bounds, blockcap, col_ptrs, cursor_ptr, send_ptr, recv_ptr, overflow_ptr):
        """the routing of one resident multi-GPU step in one call (ring ranges + packing; two launches): send = (world - 1) blocks
        [len(col_ptrs)][blockcap] in rank order without this rank, recv = world blocks with this rank's own rows written into the LAST one"""
        world, rb_ptr, rb = _ring_bounds(ring_bounds)
        _lib.call('bfgx_route_step_device', self._h, cat_dev, world, rank, rb_ptr, blockcap, len(col_ptrs), _columns(col_ptrs), cursor_ptr,
                  send_ptr, recv_ptr, overflow_ptr)

    def set_catalog_blocks(self, rows, stride):
        """the catalogs of the following K0 launches are blocks [block][column][rows] (stride = columns x rows); rows = 0: plain columns"""
        _lib.call('bfgx_plan_set_catalog_blocks', self._h, rows, stride)

    def offsets_regrid_bands(self, cat_dev, B0, B1, offsets_ptr, band0, band1, map_in_ptr, out_slice_ptr, sums_ptr=0, foreign_ptr=0, acc_f64=False):
        """K0 + K1 for the bands [B0, B1), the banded regrid of [band0, band1) into the slice, far deposits applied, sums: one enqueue-only call"""
        _lib.call('bfgx_offsets_regrid_bands_device', self._h, cat_dev, B0, B1, offsets_ptr, acc_f64, band0, band1, map_in_ptr, out_slice_ptr,
                  sums_ptr, foreign_ptr)

    def bands_max_offset2(self, band0, band1, out_ptr):
        """largest |offset|^2 (float32, device) of the slice offsets_bands() has just written for the bands [band0, band1): reduced
        from the per-tile maxima K1 leaves, no pass over the slice"""
        _lib.call('bfgx_bands_max_offset2_device', self._h, band0, band1, out_ptr)

    def max_offset2(self, offsets_ptr, npixels, out_ptr, acc_f64=False):
        """enqueue-only: *out (float32, device) = largest |offset|^2 over npixels pixels of pix_offsets"""
        _lib.call('bfgx_max_offset2_device', self._h, offsets_ptr, npixels, acc_f64, out_ptr)

    def tile_shape(self):
        """(rings per band, columns per tile): band b holds the rings [1 + b R, 1 + (b + 1) R)"""
        br, w = C.c_int32(0), C.c_int32(0)
        _lib.call('bfgx_plan_tile_shape', self._h, C.byref(br), C.byref(w))
        return int(br.value), int(w.value)

    def disc_rings(self, cat_dev, rings_ptr):
        """per halo the ring range [first, last] (1-based, inclusive: the disc's colatitude band + 2 rings + the route margin) its disc can touch -> int32 [n][2]"""
        _lib.call('bfgx_disc_rings_device', self._h, cat_dev, rings_ptr)

    def set_route_margin(self, rings):
        """disc_rings widens every halo's ring range by `rings` from now on (a rank that computes the bands next to its own as well)"""
        _lib.call('bfgx_plan_set_route_margin', self._h, rings)

    def offsets_bands(self, cat_dev, band0, band1, offsets_slice_ptr, acc_f64=False):
        """K0 + K1 for the tiles of bands [band0, band1) only; the slice starts at the first pixel of band0 ([p1 - p0][3])"""
        _lib.call('bfgx_offsets_bands_device', self._h, cat_dev, band0, band1, offsets_slice_ptr, acc_f64)

    def paint_bands(self, cat_dev, band0, band1, map_slice_ptr, acc_f64=True):
        """K0 + K3 for the tiles of bands [band0, band1) only; the slice starts at the first pixel of band0"""
        _lib.call('bfgx_paint_bands_device', self._h, cat_dev, band0, band1, map_slice_ptr, acc_f64)

    def bands(self):
        """first RING pixel of every band of rings the tiling uses (+ npix): the unit of multi-GPU pixel ownership"""
        nb = C.c_int32(0)
        _lib.call('bfgx_plan_bands', self._h, C.byref(nb), None)
        first = np.zeros(nb.value + 1, dtype=np.int64)
        _lib.call('bfgx_plan_bands', self._h, C.byref(nb), first.ctypes.data)
        return first

    def reach_rings(self, max_offset):
        """rings of apron the banded regrid needs for summed pix_offsets whose largest |offset| is `max_offset` [rad]"""
        r = C.c_int32(0)
        _lib.call('bfgx_plan_reach_rings', self._h, max_offset, C.byref(r))
        return int(r.value)

    def set_band_reach(self, rings):
        """every rank of a banded regrid must use the same apron (default 1 ring): see reach_rings"""
        _lib.call('bfgx_plan_set_band_reach', self._h, rings)

    def band_apron(self, band0, band1):
        """pixel range [olo, ohi) of summed pix_offsets the owner of bands [band0, band1) needs: its pixels + the band
        reach (set_band_reach) in rings either side"""
        lo, hi = C.c_int64(0), C.c_int64(0)
        _lib.call('bfgx_plan_band_apron', self._h, band0, band1, C.byref(lo), C.byref(hi))
        return int(lo.value), int(hi.value)

    def regrid_bands(self, band0, band1, map_in_ptr, offsets_ptr, olo, ohi, out_slice_ptr, sums_ptr=0, acc_f64=False):
        """K2 for the OUTPUT pixels of bands [band0, band1): offsets_ptr -> summed pix_offsets of pixels [olo, ohi) (band_apron),
        out_slice_ptr -> the bands' own pixels (stored once, no zero-fill).  Far deposits: far_fetch()."""
        _lib.call('bfgx_regrid_bands_device', self._h, band0, band1, map_in_ptr, offsets_ptr, olo, ohi, acc_f64, out_slice_ptr, sums_ptr)

    def far_apply(self, out_slice_ptr, p0, p1, foreign_ptr=0):
        """enqueue-only: add the listed deposits that fall into pixels [p0, p1) to the slice; count the others into *foreign_ptr"""
        _lib.call('bfgx_plan_far_apply_device', self._h, out_slice_ptr, p0, p1, foreign_ptr)

    def far_fetch(self):
        """(pixels, values) of the deposits the last regrid listed instead of applying (banded regrid only); blocking"""
        n = C.c_int64(0)
        _lib.call('bfgx_plan_far_fetch', self._h, 0, None, None, C.byref(n))
        if n.value == 0:
            return np.zeros(0, dtype=np.int64), np.zeros(0)
        pix, val = np.zeros(n.value, dtype=np.int64), np.zeros(n.value)
        _lib.call('bfgx_plan_far_fetch', self._h, n.value, pix.ctypes.data, val.ctypes.data, C.byref(n))
        return pix, val

    def paint(self, cat_dev, map_out_ptr, acc_f64=True):
        """K0 + K3 (HealpixRunner.py:418-445).  acc_f64: True / 1 = fp64 throughout (double map), False / 0 = fp32 (float map),
        2 = fp32 pair math accumulated in fp64 into a double map"""
        _lib.call('bfgx_paint_device', self._h, cat_dev, map_out_ptr, acc_f64)

    def count_pairs(self, cat_dev, fallback4=True, counts_ptr=0):
        tot = C.c_int64(0)
        _lib.call('bfgx_count_pairs_device', self._h, cat_dev, fallback4, counts_ptr, C.byref(tot))
        return int(tot.value)

    def precision(self, acc_f64=-1):
        """(BFGX_ACC_* a request resolves to on this plan, largest displacement of the plan's table in pixel sides of its NSIDE)"""
        r, d = C.c_int32(0), C.c_double(0.0)
        _lib.call('bfgx_plan_precision', self._h, acc_f64, C.byref(r), C.byref(d))
        return int(r.value), float(d.value)

    def set_algo(self, algo):
        """1 = tile-owned LDS accumulators (default), 0 = one wave per halo + global float atomics"""
        _lib.call('bfgx_plan_set_algo', self._h, algo)

    def status(self):
        _lib.call('bfgx_plan_status', self._h)

    def regrid_stats(self):
        """what the last full-map regrid did (blocking): far deposits listed, list overflowed, tiles run by the walking kernel, largest reach"""
        far, ovf, walked, reach = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _lib.call('bfgx_plan_regrid_stats', self._h, C.byref(far), C.byref(ovf), C.byref(walked), C.byref(reach))
        return {"far_listed": int(far.value), "far_overflowed": bool(ovf.value), "tiles_walked": int(walked.value), "max_reach_rings": int(reach.value)}

    def ring_table(self, first=0, count=None, from_functions=False):
        """records [first, first + count) of the plan's ring table (bfgx_debug_ring_table; blocking) as a structured array; from_functions:
        the same rings evaluated afresh by the device functions the table was built from, the quotients (dphi .. inv_dth_dn) left 0"""
        if count is None:
            count = 4 * self.nside + 1 - first
        out = np.zeros(int(count), dtype=_lib.RING_REC)
        _lib.call('bfgx_debug_ring_table', self._h, bool(from_functions), first, count, out.ctypes.data)
        return out


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
