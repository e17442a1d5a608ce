"""The regular-grid path on device-resident inputs: `GridPlan` around `bfgx_grid_plan`, the particle deposits and the particle
routing of a slab-decomposed grid."""
import ctypes as C

import numpy as np

from .. import _lib
from ._plan import TimedPlan
from .fourier import WINDOW_ORDERS


class GridPlan(TimedPlan):
    """Resident front-end of the regular-grid path (`bfgx_grid_plan`): periodic 2D / 3D maps at one redshift."""
    _destroy, _timing = 'bfgx_grid_plan_destroy', 'bfgx_grid_plan_timing'

    def __init__(self, model, keepalive, bins, ndim, redshift, max_halos, device=0, stream=0):
        self._keep = keepalive
        self.ndim = int(ndim)
        self.npix = int(len(bins))
        self.ntot = self.npix ** self.ndim
        self.max_halos = int(max_halos)
        self.device = int(device)
        self.stream = int(stream)
        grid, gkeep = _lib.make_grid(bins, ndim, redshift)
        self._create('bfgx_grid_plan_create', self.device, self.stream, grid, self.max_halos, model)

    def _pairs(self, symbol, *args):
        """the call whose last argument receives the number of contributing (halo, pixel) pairs, returned"""
        n = C.c_int64(0)
        _lib.call(symbol, self._h, *(args + (C.byref(n),)))
        return int(n.value)

    def offsets(self, cat_dev, offsets_ptr):
        """halo loop of BaryonifyGrid (Map2DRunner.py:476-575): offsets[npix^d][d] f64, zeroed then filled.
        Returns the number of contributing (halo, pixel) pairs."""
        return self._pairs('bfgx_grid_offsets_device', cat_dev, offsets_ptr)

    def paint(self, cat_dev, map_out_ptr):
        """halo loop of PaintProfilesGrid (Map2DRunner.py:708-812)"""
        return self._pairs('bfgx_grid_paint_device', cat_dev, map_out_ptr)

    def regrid(self, map_in_ptr, offsets_ptr, map_out_ptr, sums_ptr=0):
        """post-loop regrid (Map2DRunner.py:577-605): map_out zeroed then filled; sums[2] optional (zeroed by caller)"""
        _lib.call('bfgx_grid_regrid_device', self._h, map_in_ptr, offsets_ptr, map_out_ptr, sums_ptr)

    def baryonify(self, cat_dev, map_in_ptr, map_out_ptr, sums_ptr=0):
        """BaryonifyGrid.process() on device arrays as one cell-owned pass (no pix_offsets array): halos listed per block of cells,
        every cell sums its offsets in registers and is regridded at once.  Same map_out as offsets() + regrid() up to the order
        of fp64 sums.  Returns the number of contributing (halo, pixel) pairs."""
        return self._pairs('bfgx_grid_baryonify_device', cat_dev, map_in_ptr, map_out_ptr, sums_ptr)

    def deposit_baryonify(self, cat_dev, n_particles, x_ptr, y_ptr, z_ptr, mass_ptr, edges_ptr, map_in_ptr, map_out_ptr, sums_ptr=0):
        """ParticleSnapshot.make_map + BaryonifyGrid.process() in one call (device arrays): the histogram of the particles goes to
        map_in AND, as the start value of the cell-owned pass, to map_out while it is being stored -- the map is not read again to copy
        and sum it.  Returns the number of contributing (halo, pixel) pairs."""
        return self._pairs('bfgx_grid_deposit_baryonify_device', cat_dev, n_particles, x_ptr, y_ptr, z_ptr, mass_ptr, edges_ptr, map_in_ptr,
                           map_out_ptr, sums_ptr)

    def set_slab(self, plane_lo, plane_n):
        """slab decomposition over GPUs: this plan owns the planes [plane_lo, plane_lo + plane_n) of the first array axis;
        offsets() / paint() then fill plane_n x npix (x npix) cells (pass the whole catalog), regrid_slab() regrids them"""
        _lib.call('bfgx_grid_plan_set_slab', self._h, plane_lo, plane_n)

    def regrid_slab(self, map_in_ptr, offsets_ptr, apron, map_out_ptr, sums_ptr=0, missed_ptr=0):
        """regrid of the slab's source cells into map_out = slab + `apron` planes either side (zeroed by the call, periodic);
        *missed (int32, zeroed by the caller) is set if a deposit fell outside that buffer"""
        _lib.call('bfgx_grid_regrid_slab_device', self._h, map_in_ptr, offsets_ptr, apron, map_out_ptr, sums_ptr, missed_ptr)


def deposit_particles_slab_device(x_ptr, y_ptr, z_ptr, mass_ptr, n, n_grid, edges_ptr, plane_lo, plane_n, map_out_ptr, ndim=3, device=0, stream=0):
    """ParticleSnapshot.make_map for the planes [plane_lo, plane_lo + plane_n) of the first axis (particles elsewhere are dropped)"""
    _lib.call('bfgx_deposit_particles_slab_device', device, stream, ndim, n, x_ptr, y_ptr, z_ptr, mass_ptr, n_grid, edges_ptr, plane_lo, plane_n,
              map_out_ptr)


def deposit_particles_device(x_ptr, y_ptr, z_ptr, mass_ptr, n, n_grid, edges_ptr, map_out_ptr, ndim=3, device=0, stream=0):
    """ParticleSnapshot.make_map on device-resident columns (io.py:622-670)"""
    _lib.call('bfgx_deposit_particles_device', device, stream, ndim, n, x_ptr, y_ptr, z_ptr, mass_ptr, n_grid, edges_ptr, map_out_ptr)


def deposit_cloud_device(x_ptr, y_ptr, z_ptr, mass_ptr, n, n_grid, L, order, map_out_ptr, ndim=3, device=0, stream=0, shift=0):
    """CIC (order 2) / TSC (order 3) mass assignment of device-resident columns on the periodic box [0, L]^ndim, enqueue-only; order as in
    WINDOW_ORDERS (a name is taken too).  map_out [n_grid^ndim] is stored whole.  shift=1: on the grid displaced by half a cell (every
    particle moved by +L / (2 n_grid) along every axis), the second grid of interlaced_power_spectrum."""
    if isinstance(order, str):
        order = WINDOW_ORDERS.get(order.lower(), 0)
    _lib.call('bfgx_deposit_cloud_shifted_device', device, stream, ndim, n, x_ptr, y_ptr, z_ptr, mass_ptr, n_grid, L, order, shift, map_out_ptr)


def route_particles_count_device(x_ptr, n, n_grid, edges_ptr, world, owner_ptr, counts_ptr, device=0, stream=0):
    """pass 1 of the particle routing of a slab-decomposed grid (enqueue-only): owner[n] uint8, counts[world] int32"""
    _lib.call('bfgx_route_particles_count_device', device, stream, n, x_ptr, n_grid, edges_ptr, world, owner_ptr, counts_ptr)


def route_particles_fill_device(col_ptrs, n, owner_ptr, world, start, total, cursor_ptr, cols_out_ptr, device=0, stream=0):
    """pass 2: cols_out[c][start[d] + ...] = column c of the particles bound for rank d (len(col_ptrs) <= 4 columns)"""
    st = np.ascontiguousarray(start, dtype=np.int64)
    cp = (C.c_void_p * len(col_ptrs))(*[int(q) for q in col_ptrs])
    _lib.call('bfgx_route_particles_fill_device', device, stream, n, len(col_ptrs), cp, owner_ptr, world, st.ctypes.data, total, cursor_ptr,
              cols_out_ptr)
