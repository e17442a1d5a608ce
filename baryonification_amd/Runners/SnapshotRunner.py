"""
Particle-snapshot runner: drop-in for BaryonForge/Runners/SnapshotRunner.py (`DefaultRunnerSnapshot` :9-92,
`BaryonifySnapshot` :95-262).  Same constructor and attributes; `process()` returns a copy of the snapshot's
structured array with displaced, periodically re-wrapped x, y(, z).  No KD-tree is built: the HIP path bins the halos
into a periodic cell grid and gathers per particle (csrc/bfgx_snapshot.hpp); `KDTree_kwargs` is accepted and ignored,
`tree` is None.  There is no CPU fallback.

A model that is a plain Python callable (displacement(r, M, a), no table) is tabulated once (with a RuntimeWarning) unless it sets
`bfgx_exact = True`: then it is called once per halo, every halo, on the distances of the particles within R_q (ascending particle
index within a halo), with M = cat['M'][j] and a = 1/(1+z), as the reference's loop does (:228, :245; bfgx_snapshot_pairs_*,
csrc/bfgx_snapshot_pairs.hpp).

`MeasureProfilesSnapshot` (not in the reference) measures what baryonification is defined by: the radial profile of the particles around the
halos, before and after (csrc/bfgx_snapshot_stack.hpp).
"""
import ctypes as C

import numpy as np

from .. import _lib, _tensors
from ..utils.cosmology import MassDef, cosmo_to_dict
from ._model import _placeholder_model, build_model, process_snapshot_exact, wants_exact
from ._profiles import MAX_PROFILE_BINS, _is_cuda_tensor, check_r_edges, halo_radii, ratio      # noqa: F401 (MAX_PROFILE_BINS: importable from here)

__all__ = ['DefaultRunnerSnapshot', 'BaryonifySnapshot', 'MeasureProfilesSnapshot', 'SnapshotProfiles']


class DefaultRunnerSnapshot(object):

    def __init__(self, HaloNDCatalog, ParticleSnapshot, epsilon_max, model, mass_def=MassDef(200, 'critical'), verbose=True,
                 KDTree_kwargs={}):
        self.HaloNDCatalog = HaloNDCatalog
        self.ParticleSnapshot = ParticleSnapshot
        self.epsilon_max = epsilon_max
        self.cosmo = HaloNDCatalog.cosmology
        self.model = model
        self.mass_def = mass_def
        self.verbose = verbose
        self.tree = None               # the reference keeps a scipy KDTree here; the GPU path needs none
        self.device = 0
        self.use_records = True        # engine knob: hand the structured array to the library as it is (False: gather the columns on the host)
        self.last_stats = None

    def enforce_periodicity(self, dx):
        L = self.ParticleSnapshot.L
        dx = np.where(dx > L / 2, dx - L, dx)
        dx = np.where(dx < -L / 2, dx + L, dx)
        return dx

    def compute_distance(self, *args):
        d = 0
        for dx in args:
            d = d + self.enforce_periodicity(dx) ** 2
        return np.sqrt(d)


class BaryonifySnapshot(DefaultRunnerSnapshot):
    """Moves every particle within epsilon_max * R200c of a halo radially by the model's displacement."""

    def _setup(self):
        snap = self.ParticleSnapshot
        hcat = self.HaloNDCatalog.cat
        is2D = snap.is2D
        cosmo = dict(self.cosmo)
        cosmo['w0'] = -1.0                                            # SnapshotRunner.py:204-207 does not pass w0
        model, p_keys, keep = build_model(self, 'displacement', cosmo)
        if p_keys:
            raise NotImplementedError("BaryonifySnapshot passes no halo properties to the model (SnapshotRunner.py:240)")
        with np.errstate(invalid='ignore', divide='ignore'):
            lnM = np.log(np.asarray(hcat['M'], dtype=np.float32)).astype(np.float64)     # float32 log, as BaryonifyGrid
        cat, cols = _lib.make_grid_catalog_host(hcat['M'], hcat['x'], hcat['y'], None if is2D else hcat['z'], lnM)
        return snap, is2D, model, keep, cat, cols

    def process_make_map(self, N_grid, assignment='ngp'):
        """`ParticleSnapshot(cat=self.process(), ...).make_map(N_grid)` (SnapshotRunner.py:173-262 followed by io.py:622-670) as ONE call for
        the common case that only the map of the baryonified particles is wanted (the reference's notebook 10): the records go to the device
        once, the displaced coordinates exist only as the deposit's sort keys, the map comes back.  Not in the reference's API; the result
        equals the two calls (cell for cell with unit masses, to the order of the sums inside a cell otherwise).  Snapshots whose `cat` is
        not one C-contiguous structured array of float64 fields take the two calls.  The fused displace + deposit is nearest grid point
        only: assignment='cic' or 'tsc' (see ParticleSnapshot.make_map) takes the two calls, process() and then make_map(N_grid, assignment)."""
        if not isinstance(assignment, str) or assignment.lower() != 'ngp':
            from .. import engine
            if not isinstance(assignment, str) or engine.WINDOW_ORDERS.get(assignment.lower(), 0) < 1:      # (before any work, as make_map says it)
                raise ValueError("make_map: assignment must be 'ngp', 'cic' or 'tsc', not %r" % (assignment,))
            return self._map_of(self.process(), N_grid, assignment)
        if wants_exact(self, 'displacement'):            # a plain-Python model with bfgx_exact = True: the two calls
            return self._map_of(self.process(), N_grid)
        snap, is2D, model, keep, cat, cols = self._setup()
        rec = snap.cat
        fields = rec.dtype.fields or {}
        need = ('x', 'y', 'M') if is2D else ('x', 'y', 'z', 'M')
        ndim = 2 if is2D else 3
        ok = (isinstance(rec, np.ndarray) and rec.ndim == 1 and rec.flags.c_contiguous and rec.dtype.itemsize % 8 == 0 and rec.dtype.itemsize >= 16 and
              all(k in fields and fields[k][0] == np.float64 and fields[k][1] % 8 == 0 for k in need))
        if ok:
            edges = np.linspace(0, snap.L, N_grid + 1)                # io.py:640
            out = _lib.pinned_empty(N_grid ** ndim).reshape((N_grid,) * ndim)
            opts = _lib.bfgx_opts(int(self.device), 1, 1, 0, 1, 0)
            stats = _lib.bfgx_stats()
            rc = _lib.load().bfgx_baryonify_snapshot_records_map(
                C.byref(cat), C.byref(model), ndim, float(snap.L), float(self.HaloNDCatalog.redshift), rec.size,
                rec.ctypes.data if rec.size else None, rec.dtype.itemsize, fields['x'][1], fields['y'][1], 0 if is2D else fields['z'][1],
                fields['M'][1], int(N_grid), edges.ctypes.data, out.ctypes.data, C.byref(opts), C.byref(stats))
            if rc == _lib.ERR_UNSUPPORTED:
                ok = False                                            # (a grid the tile-owned deposit does not take)
            else:
                _lib.check(rc)
                self.last_stats = {k: getattr(stats, k) for k, _ in stats._fields_}
                del keep, cols
                return out
        return self._map_of(self.process(), N_grid)

    def _map_of(self, new_cat, N_grid, assignment='ngp'):
        """ParticleSnapshot(cat=new_cat, ...).make_map(N_grid, assignment) with the snapshot's other attributes"""
        from ..utils.io import ParticleSnapshot
        new = ParticleSnapshot.__new__(ParticleSnapshot)
        new.__dict__.update(self.ParticleSnapshot.__dict__)
        new.cat = new_cat
        return new.make_map(N_grid, assignment)

    def process(self):
        if wants_exact(self, 'displacement'):            # a plain-Python model with bfgx_exact = True: called per halo (:228, :245)
            return process_snapshot_exact(self)
        snap, is2D, model, keep, cat, cols = self._setup()
        opts = _lib.bfgx_opts(int(self.device), 1, 1, 0, 1, 0)
        stats = _lib.bfgx_stats()
        rec = snap.cat
        fields = rec.dtype.fields or {}
        ok = (getattr(self, 'use_records', True) and isinstance(rec, np.ndarray) and rec.ndim == 1 and rec.flags.c_contiguous and rec.dtype.itemsize % 8 == 0 and rec.dtype.itemsize >= 16 and
              all(k in fields and fields[k][0] == np.float64 and fields[k][1] % 8 == 0 for k in (('x', 'y') if is2D else ('x', 'y', 'z'))))
        if ok:
            # the records as they are: uploaded in chunks, displaced in place on the device, downloaded into the new catalog -- the host
            # neither gathers the strided columns nor scatters them back (`new_cat = cat.copy(); new_cat['x'] = ...`, SnapshotRunner.py:254-262)
            new_cat = _lib.pinned_empty(rec.size * rec.dtype.itemsize, np.uint8).view(rec.dtype) if rec.size else rec.copy()
            _lib.call('bfgx_baryonify_snapshot_records', cat, model, 2 if is2D else 3, snap.L, self.HaloNDCatalog.redshift, rec.size,
                      rec.ctypes.data if rec.size else None, new_cat.ctypes.data if rec.size else None, rec.dtype.itemsize, fields['x'][1],
                      fields['y'][1], 0 if is2D else fields['z'][1], opts, stats)
            self.last_stats = {k: getattr(stats, k) for k, _ in stats._fields_}
            del keep, cols
            return new_cat
        x, y = _lib.f8(snap.cat['x']), _lib.f8(snap.cat['y'])
        z = None if is2D else _lib.f8(snap.cat['z'])
        s = _lib.bfgx_snapshot(2 if is2D else 3, 0, x.size, x.ctypes.data, y.ctypes.data, None if is2D else z.ctypes.data,
                               float(snap.L), float(self.HaloNDCatalog.redshift))
        ox, oy = np.empty_like(x), np.empty_like(y)
        oz = None if is2D else np.empty_like(z)
        _lib.call('bfgx_baryonify_snapshot', cat, model, s, ox.ctypes.data, oy.ctypes.data, None if is2D else oz.ctypes.data, opts, stats)
        self.last_stats = {k: getattr(stats, k) for k, _ in stats._fields_}
        new_cat = snap.cat.copy()
        new_cat['x'], new_cat['y'] = ox, oy
        if not is2D:
            new_cat['z'] = oz
        del keep, cols
        return new_cat


class SnapshotProfiles(object):
    """What MeasureProfilesSnapshot.process() returns.  Per (halo, bin), shape (n_halo, nb): `npart`, the particles with
    r_edges[b] <= x < r_edges[b + 1] inside the halo's ball, and `sum`, the sum of their finite weights (None for a counts-only
    measurement: `density`, `enclosed` and `stack` then work on the counts).  numpy arrays, or torch tensors on the particles' device when
    the particles were CUDA tensors.  `R` is the comoving halo radius R_com = mass_def.get_radius(M, a) / a and `R_q` =
    clip(epsilon_max R_com, 0, L / 2) the radius of the ball, per halo (numpy; NaN and 0 for an invalid halo); x is the comoving distance,
    or distance / R_com when `scaled`."""

    def __init__(self, r_edges, npart, sum=None, scaled=False, ndim=3, R=None, R_q=None):
        self.r_edges, self.scaled, self.ndim = np.asarray(r_edges, dtype=np.float64), bool(scaled), int(ndim)
        self.npart, self.sum = npart, sum
        self.R, self.R_q = R, R_q

    def _like(self, a):
        """a host array as the kind of array the measurement came back as"""
        if isinstance(self.npart, np.ndarray):
            return a
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.npart.device)

    def _total(self):
        if self.sum is not None:
            return self.sum
        return self.npart.astype(np.float64) if isinstance(self.npart, np.ndarray) else self.npart.double()

    @property
    def mean(self):
        """sum / npart, NaN where npart is 0 (None for a counts-only measurement)"""
        return None if self.sum is None else ratio(self.sum, self.npart)

    @property
    def volume(self):
        """The part of bin b's spherical shell (3-D; annulus in 2-D) that lies inside the halo's ball:
        V(min(hi s, R_q)) - V(min(lo s, R_q)), s = R_com when scaled, else 1, V = 4 pi r^3 / 3 or pi r^2."""
        s = np.asarray(self.R, dtype=np.float64)[:, None] if self.scaled else 1.0
        with np.errstate(invalid='ignore'):
            r = np.minimum(self.r_edges[None, :] * s, np.asarray(self.R_q, dtype=np.float64)[:, None])
        V = 4.0 * np.pi / 3.0 * r ** 3 if self.ndim == 3 else np.pi * r ** 2
        return self._like(V[:, 1:] - V[:, :-1])

    @property
    def density(self):
        """sum / volume (NaN where the bin lies outside the ball)"""
        return ratio(self._total(), self.volume)

    @property
    def enclosed(self):
        """cumsum(sum, axis=1): the sum over the bins up to b.  This is M(< r_edges[b + 1]) only when r_edges[0] == 0."""
        return self._total().cumsum(1)

    def stack(self, select=None, weights=None):
        """The halo-weighted profile over the chosen halos per bin: 'mean' = sum_j w_j sum[j] / sum_j w_j npart[j] and 'density' =
        sum_j w_j sum[j] / sum_j w_j volume[j] (NaN where the denominator is 0).  select: anything that indexes the halo axis; weights:
        one per chosen halo (default 1)."""
        sel = slice(None) if select is None else select
        host = isinstance(self.npart, np.ndarray)
        s, vol = self._total()[sel], self.volume[sel]
        n = self.npart[sel].astype(np.float64) if host else self.npart[sel].to(s.dtype)
        if weights is not None:
            w = np.asarray(weights, dtype=np.float64) if host else weights
            s, n, vol = s * w[:, None], n * w[:, None], vol * w[:, None]
        nansum = (lambda v: np.nansum(v, axis=0)) if host else (lambda v: v.nansum(0))
        out = {'density': ratio(s.sum(0), nansum(vol))}              # (an invalid halo has an all-zero row and no volume)
        if self.sum is not None:
            out['mean'] = ratio(s.sum(0), n.sum(0))
        return out


class MeasureProfilesSnapshot(DefaultRunnerSnapshot):
    """Measures halo-centred radial profiles of the particles of a snapshot: the box counterpart of MeasureProfilesShell.  For halo j the
    particles within BaryonifySnapshot's ball -- minimum-image distance d <= R_q = clip(epsilon_max R_com, 0, L / 2), R_com the comoving
    radius of `mass_def` -- are binned in x = d (comoving Mpc) or, scaled=True, x = d / R_com: bin b holds r_edges[b] <= x < r_edges[b + 1].
    A particle adds 1 to npart[j, b] and its weight (the 'M' column by default) to sum[j, b].  fp64 throughout; counts are exact.
    `model` must be None: there is nothing to tabulate.  `process(cat=runner.process())` of a BaryonifySnapshot runner measures the
    displaced particles with the same object."""

    def __init__(self, HaloNDCatalog, ParticleSnapshot, epsilon_max, model=None, mass_def=MassDef(200, 'critical'), verbose=True,
                 KDTree_kwargs={}, *, r_edges, scaled=False):
        if model is not None:
            raise TypeError("MeasureProfilesSnapshot takes model=None: it measures the particles, there is nothing to tabulate")
        super().__init__(HaloNDCatalog, ParticleSnapshot, epsilon_max, model, mass_def, verbose, KDTree_kwargs)
        self.r_edges = check_r_edges(r_edges)
        self.scaled = bool(scaled)

    def _cosmo_dict(self):
        cosmo = dict(cosmo_to_dict(self.cosmo))
        cosmo['w0'] = -1.0                                            # as BaryonifySnapshot: SnapshotRunner.py:204-207 does not pass w0
        return cosmo

    def radii(self):
        """(R_com, R_q) per halo on the host: the comoving radius of the mass definition and the radius of the ball (SnapshotRunner.py:219-222);
        NaN and 0 for a halo the measurement skips (M not positive / finite, a non-finite coordinate)."""
        return halo_radii(self.HaloNDCatalog.cat, ('x', 'y') if self.ParticleSnapshot.is2D else ('x', 'y', 'z'), self.HaloNDCatalog.redshift,
                          self.mass_def, self._cosmo_dict(), self.epsilon_max, float(self.ParticleSnapshot.L) / 2)

    def process(self, cat=None, weights=None):
        """SnapshotProfiles of the snapshot's own particles, or of `cat`: a structured array with the snapshot's fields (what
        BaryonifySnapshot.process() returns), or a tuple (x, y[, z]) of 1-D CUDA float64 torch tensors, which are measured where they lie
        (on torch's current stream) with tensors on that device as the result.  weights: None = the 'M' column of what is measured
        (device tensors: counts only), an array / tensor of one weight per particle, or False = counts only."""
        snap = self.ParticleSnapshot
        is2D = snap.is2D
        ndim = 2 if is2D else 3
        hcat = self.HaloNDCatalog.cat
        model, keep = _placeholder_model(self, self._cosmo_dict())
        c, ckeep = _lib.make_grid_catalog_host(hcat['M'], hcat['x'], hcat['y'], None if is2D else hcat['z'])
        edges, nb, n = self.r_edges, self.r_edges.size - 1, int(hcat.size)
        L, zr = float(snap.L), float(self.HaloNDCatalog.redshift)
        if isinstance(cat, (tuple, list)):
            import torch
            cols = list(cat)
            if len(cols) != ndim or not all(_is_cuda_tensor(t) for t in cols):
                raise ValueError("device particles are a tuple of %d CUDA tensors (x, y%s)" % (ndim, '' if is2D else ', z'))
            dev, npart = cols[0].device, cols[0].numel()
            if weights is not None and weights is not False:
                if not _is_cuda_tensor(weights):
                    raise ValueError("the weights of device particles must be a CUDA tensor")
                cols.append(weights)
            for t in cols:
                if t.dtype != torch.float64 or t.dim() != 1 or t.numel() != npart or t.device != dev:
                    raise ValueError("device particles and weights must be 1-D float64 tensors of one length on one device")
            cols = [t.contiguous() for t in cols]
            has_w = len(cols) > ndim
            out_n = torch.empty((n, nb), dtype=torch.int64, device=dev)
            out_s = torch.empty((n, nb), dtype=torch.float64, device=dev) if has_w else None
            ptr = [t.data_ptr() for t in cols[:ndim]] + [None] * (3 - ndim)
            _lib.call('bfgx_snapshot_profiles_device', _tensors.device_index(dev), _tensors.stream(dev), c, model, ndim, L, zr, npart, ptr[0], ptr[1],
                      ptr[2], cols[ndim].data_ptr() if has_w else None, nb, edges.ctypes.data, self.scaled, out_n.data_ptr(), _tensors.ptr(out_s))
        else:
            rec = snap.cat if cat is None else cat
            x, y = _lib.f8(rec['x']), _lib.f8(rec['y'])
            z = None if is2D else _lib.f8(rec['z'])
            if weights is False:
                w = None
            else:
                w = _lib.f8(rec['M'] if weights is None else weights).reshape(-1)
                if w.size != x.size:
                    raise ValueError("weights must hold one weight per particle (%d): got %d" % (x.size, w.size))
            s = _lib.bfgx_snapshot(ndim, 0, x.size, x.ctypes.data, y.ctypes.data, None if is2D else z.ctypes.data, L, zr)
            out_n = np.empty((n, nb), dtype=np.int64)                 # (every cell is written by the library: no zero-fill)
            out_s = None if w is None else np.empty((n, nb), dtype=np.float64)
            _lib.call('bfgx_snapshot_profiles', c, model, s, _tensors.ptr(w), nb, edges.ctypes.data, self.scaled, self.device, out_n.ctypes.data,
                      _tensors.ptr(out_s))
        del keep, ckeep
        R, R_q = self.radii()
        return SnapshotProfiles(edges.copy(), out_n, out_s, self.scaled, ndim, R, R_q)
