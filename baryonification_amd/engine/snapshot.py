"""The particle-snapshot path on device-resident columns: the one-shot entry and `SnapshotPlan` around `bfgx_snapshot_plan`."""
import ctypes as C

from .. import _lib
from ._plan import Plan


def _z(ptrs, ndim):
    """the third column's pointer of (x, y[, z]), None (NULL) in 2-D"""
    return int(ptrs[2]) if ndim == 3 else None


def baryonify_snapshot_device(model, halos_dev, part_ptrs, n_part, L, redshift, out_ptrs, device=0, stream=0):
    """BaryonifySnapshot on device-resident columns: part_ptrs / out_ptrs = (x, y[, z]) device pointers.
    Returns the number of displaced (halo, particle) pairs."""
    ndim = len(part_ptrs)
    s = _lib.bfgx_snapshot(ndim, 0, int(n_part), int(part_ptrs[0]), int(part_ptrs[1]), _z(part_ptrs, ndim), float(L), float(redshift))
    n = C.c_int64(0)
    _lib.call('bfgx_baryonify_snapshot_device', device, stream, halos_dev, model, s, out_ptrs[0], out_ptrs[1], _z(out_ptrs, ndim), C.byref(n))
    return int(n.value)


class SnapshotPlan(Plan):
    """Resident front-end of the particle-snapshot path (`bfgx_snapshot_plan`): the model and the halo-cell workspace stay
    on the device between calls."""
    _destroy = 'bfgx_snapshot_plan_destroy'

    def __init__(self, model, keepalive, ndim, L, redshift, max_halos, device=0, stream=0):
        self._keep = keepalive
        self.ndim = int(ndim)
        self._create('bfgx_snapshot_plan_create', device, stream, model, self.ndim, L, redshift, max_halos)

    def displace(self, halos_dev, n_part, part_ptrs, out_ptrs):
        """BaryonifySnapshot.process (SnapshotRunner.py:199-262) on device columns; returns the number of displaced pairs"""
        n = C.c_int64(0)
        _lib.call('bfgx_snapshot_displace_device', self._h, halos_dev, n_part, part_ptrs[0], part_ptrs[1], _z(part_ptrs, self.ndim),
                  out_ptrs[0], out_ptrs[1], _z(out_ptrs, self.ndim), C.byref(n))
        return int(n.value)

    def displace_deposit(self, halos_dev, n_part, part_ptrs, mass_ptr, n_grid, edges_ptr, map_out_ptr):
        """BaryonifySnapshot.process() followed by ParticleSnapshot.make_map(n_grid) of the result (SnapshotRunner.py:173-262, io.py:622-670)
        when only the map is wanted: map_out [n_grid^ndim] float64 on the device; the displaced coordinates are never stored.  mass_ptr 0 =
        unit masses.  Returns the number of displaced pairs."""
        n = C.c_int64(0)
        _lib.call('bfgx_snapshot_displace_deposit_device', self._h, halos_dev, n_part, part_ptrs[0], part_ptrs[1], _z(part_ptrs, self.ndim),
                  mass_ptr, n_grid, edges_ptr, map_out_ptr, C.byref(n))
        return int(n.value)
