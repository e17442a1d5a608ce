"""
Regular-grid runners: drop-in for BaryonForge/Runners/Map2DRunner.py (`regrid_pixels_2D` :14-83, `regrid_pixels_3D`
:86-163, `DefaultRunnerGrid` :168-375, `BaryonifyGrid` :379-607, `PaintProfilesGrid` :610-817).  Same constructor
(positional order, attribute names), same `process()` return value (float64 array of the map's shape) and the same
exceptions.  `process()` does no per-halo work in Python except the 2x2 shear matrices of `use_ellipticity = True`:
catalog, map and the model's raw table go through the C ABI (include/bfgx.h, "regular-grid path") to the HIP kernels
in csrc/bfgx_grid.hpp.  There is no CPU fallback.

A model that is a plain Python callable (displacement(r, M, a) / projected or real(cosmo, r, M, a), no table) is tabulated once
(with a RuntimeWarning) unless it sets `bfgx_exact = True`: then it is called once per halo on r_grid.flatten() of the halo's whole
cutout, with M = cat['M'][j] and a = 1/(1+z), as the reference's loop does (:534, :577, :801).  The device makes the cutouts' radii
and applies the values (bfgx_grid_pairs_*, csrc/bfgx_grid_pairs.hpp); the host holds one batch of them at a time
(_model.EXACT_BATCH_PAIRS).

Not built: `PaintProfilesAnisGrid` (:820-942).

`MeasureProfilesGrid` (not in the reference) measures a gridded map where baryonification and painting are defined: the radial profile
around the halos, with the constructor keywords, the (n_halo, n_bins) results and the `stack()` of MeasureProfilesShell and
MeasureProfilesSnapshot (csrc/bfgx_grid_stack.hpp).
"""
import numpy as np

from .. import _lib, _tensors
from ..utils.cosmology import MassDef
from ..utils.Tabulate import ParamTabulatedProfile
from ._model import _placeholder_model, build_model, process_grid_exact, wants_exact
from ._profiles import (MAX_PROFILE_BINS, _MapProfiles, _is_cuda_tensor, alloc_profile_outs, check_r_edges, halo_radii,      # noqa: F401
                        ratio)                                       # (MAX_PROFILE_BINS: importable from here)

__all__ = ['DefaultRunnerGrid', 'BaryonifyGrid', 'PaintProfilesGrid', 'MeasureProfilesGrid', 'GridProfiles', 'regrid_pixels_2D',
           'regrid_pixels_3D']


def _regrid(grid, pix_positions, pix_values, ndim, device=0):
    if not (isinstance(grid, np.ndarray) and grid.dtype == np.float64 and grid.flags.c_contiguous and grid.ndim == ndim):
        raise ValueError("grid must be a C-contiguous float64 array with %d equal axes" % ndim)
    if len(set(grid.shape)) != 1:
        raise ValueError("grid must be square / cubic")
    pos = _lib.f8(pix_positions)
    val = _lib.f8(pix_values)
    if pos.shape != (val.size, ndim):
        raise ValueError("pix_positions must have shape (N, %d)" % ndim)
    _lib.call('bfgx_regrid_pixels', device, ndim, grid.shape[0], val.size, pos.ctypes.data, val.ctypes.data, grid.ctypes.data)


def regrid_pixels_2D(grid, pix_positions, pix_values):
    """Adds `pix_values`, spread over the unit squares at `pix_positions` (x, y), to the periodic square `grid`
    IN PLACE (grid[i, j]: i from y, j from x), as Map2DRunner.py:14-83."""
    _regrid(grid, pix_positions, pix_values, 2)


def regrid_pixels_3D(grid, pix_positions, pix_values):
    """3-D version (grid[i, j, k]: i from y, j from x, k from z), as Map2DRunner.py:86-163."""
    _regrid(grid, pix_positions, pix_values, 3)


class DefaultRunnerGrid(object):

    def __init__(self, HaloNDCatalog, GriddedMap, epsilon_max, model, use_ellipticity=False,
                 mass_def=MassDef(200, 'critical'), verbose=True):
        self.HaloNDCatalog = HaloNDCatalog
        self.GriddedMap = GriddedMap
        self.cosmo = HaloNDCatalog.cosmology
        self.model = model
        self.epsilon_max = epsilon_max
        self.mass_def = mass_def
        self.verbose = verbose
        self.use_ellipticity = use_ellipticity
        self.device = 0                # engine knobs (not in the reference): plain attributes, picklable
        self.last_stats = None
        if use_ellipticity:            # Map2DRunner.py:271-277
            names = HaloNDCatalog.cat.dtype.names
            assert 'q_ell' in names, "The 'q_ell' column is missing, but you set use_ellipticity = True"
            if not GriddedMap.is2D:
                assert 'c_ell' in names, "The 'c_ell' column is missing, but you set use_ellipticity = True"
            assert 'A_ell' in names, "The 'A_ell' column is missing, but you set use_ellipticity = True"

    def build_Rmat(self, A, q):
        """Shear matrix of a halo with orientation vector A (normalised IN PLACE) and axis ratio q: the reduced shear g of galsim's
        Shear(q, beta), |g| = tanh(eta / 2) with eta = -ln q, as [[1 + g1, g2], [g2, 1 - g1]] / sqrt(1 - |g|^2) (Map2DRunner.py:283-337).
        The operations and their order are the reference's: the matrices enter the parity tests bit for bit."""
        A /= np.linalg.norm(A)
        ndim = len(A)
        if ndim == 1:
            raise ValueError("Can't rotate a 1-dimensional vector")
        if ndim != 2:
            raise NotImplementedError("This method has not yet been verified. Use 2D ellipticity method instead")
        beta = np.arccos(np.dot(A, np.array([1., 0.])))                 # position angle against the first axis
        eta = -np.log(q)
        if eta > 1e-4:
            ratio = np.tanh(0.5 * eta) / eta                             # |g| / eta
        else:                                                            # its series about eta = 0
            e2 = eta * eta
            ratio = 0.5 + e2 * ((-1 / 24) + e2 * (1 / 240))
        g = ratio * eta * np.exp(2j * beta)
        return np.array([[1 + g.real, g.imag], [g.imag, 1 - g.real]]) / np.sqrt(1 - np.abs(g) ** 2)

    def coord_array(self, *args):
        """(N, len(args)) array of the flattened arguments, one per column (Map2DRunner.py:340-358)"""
        return np.stack([np.ravel(a) for a in args], axis=1)

    def pick_indices(self, center, width, Npix):
        """the 2 width indices around `center` on a periodic axis of Npix cells, wrapped once either way (Map2DRunner.py:361-391)"""
        idx = np.arange(center - width, center + width)
        idx = idx + Npix * (idx < 0)
        return idx - Npix * (idx >= Npix)

    # -- shared plumbing -----------------------------------------------------------------------
    def _check_keys(self, keys):
        if len(keys) > 0:                                             # Map2DRunner.py:471-474, :703-706
            txt = (f"You asked to use {keys} properties in Baryonification. You must pass a ParamTabulatedProfile"
                   f"as the model. You have passed {type(self.model)} instead")
            ok = isinstance(self.model, ParamTabulatedProfile) or type(self.model).__name__ == 'ParamTabulatedProfile'
            assert ok, txt

    def _runner_cosmo(self):
        """ccl.Cosmology(Omega_c, Omega_b, h, sigma8, n_s) of Map2DRunner.py:456-459: w0 is NOT passed on"""
        d = dict(self.cosmo)
        d['w0'] = -1.0
        return d

    def _rmats(self, what):
        """per-halo shear matrices, evaluated exactly as the runner does (float32 catalog columns, :490-493, :528)"""
        cat = self.HaloNDCatalog.cat
        out = np.zeros((cat.size, 2, 2))
        for j in range(cat.size):
            q_j = cat['q_ell'][j]
            A_j = cat['A_ell'][j]
            A_j = A_j / np.sqrt(np.sum(A_j ** 2))
            assert q_j > 0, "The axis ratio in halo %d is %s" % (j, what)
            out[j] = self.build_Rmat(A_j, q_j)
        return out

    def _catalog(self, keys, rmat):
        cat = self.HaloNDCatalog.cat
        is2D = self.GriddedMap.is2D
        # the read-out takes np.log of the float32 catalog mass, i.e. a float32 logarithm (BaryonCorrection.py:369,
        # Tabulate.py:283); evaluated here with the caller's numpy so that its last bit is the reference's
        with np.errstate(invalid='ignore', divide='ignore'):      # invalid masses are skipped by the kernels
            lnM = np.log(np.asarray(cat['M'], dtype=np.float32)).astype(np.float64)
        return _lib.make_grid_catalog_host(cat['M'], cat['x'], cat['y'], None if is2D else cat['z'], lnM, rmat,
                                           [cat[k] for k in keys])

    def _grid(self):
        G = self.GriddedMap
        if len(G.bins) != G.Npix:
            raise ValueError("GriddedMap.bins must hold one pixel-centre coordinate per pixel (%d != %d)" % (len(G.bins), G.Npix))
        return _lib.make_grid(G.bins, 2 if G.is2D else 3, self.HaloNDCatalog.redshift)


class BaryonifyGrid(DefaultRunnerGrid):
    """Displaces the mass of a periodic 2D / 3D grid around every halo (the grid must hold MASS, not density:
    pixels equal to 0 are empty, Map2DRunner.py:387-388)."""

    def process(self):
        keys = vars(self.model).get('p_keys', [])
        self._check_keys(keys)
        rmat = None
        if self.use_ellipticity:
            if not self.GriddedMap.is2D:
                raise NotImplementedError("Currently not able to ellipticities with 3D maps.")    # :559
            rmat = self._rmats("not positive")
        if wants_exact(self, 'displacement'):            # a plain-Python model with bfgx_exact = True: called per halo, as the reference does
            return process_grid_exact(self, 'displacement', rmat)
        model, p_keys, keep = build_model(self, 'displacement', self._runner_cosmo())
        cat, cols = self._catalog(p_keys, rmat)
        grid, gkeep = self._grid()
        orig_map = _lib.f8(self.GriddedMap.map)
        new_map = _lib.pinned_empty(orig_map.size).reshape(orig_map.shape)     # page-locked and pooled: the copy back runs at the PCIe rate
        opts = _lib.bfgx_opts(int(self.device), 1, 1, 1, 1, 0)
        stats = _lib.bfgx_stats()
        _lib.call('bfgx_baryonify_grid', cat, model, grid, orig_map.ctypes.data, new_map.ctypes.data, opts, stats)
        self.last_stats = {k: getattr(stats, k) for k, _ in stats._fields_}
        del keep, cols, gkeep
        return new_map


class PaintProfilesGrid(DefaultRunnerGrid):
    """Paints a tabulated profile around every halo into an empty grid: the projected profile on 2D maps, the real
    (3-D) profile on 3D maps (Map2DRunner.py:750, :776)."""

    def process(self):
        keys = vars(self.model).get('p_keys', []) if self.model is not None else []
        self._check_keys(keys)
        assert self.model is not None, "You must provide a model"
        rmat = None
        if self.use_ellipticity:
            if not self.GriddedMap.is2D:
                raise ValueError("use_ellipticity is not implemented for 3D maps")                # :784
            rmat = self._rmats("zero")
        kind = 'projected' if self.GriddedMap.is2D else 'real'
        if wants_exact(self, kind):
            return process_grid_exact(self, kind, rmat)
        model, p_keys, keep = build_model(self, kind, self._runner_cosmo())
        cat, cols = self._catalog(p_keys, rmat)
        grid, gkeep = self._grid()
        new_map = _lib.pinned_empty(int(np.prod(self.GriddedMap.map.shape))).reshape(self.GriddedMap.map.shape)
        opts = _lib.bfgx_opts(int(self.device), 1, 1, 0, 1, 0)
        stats = _lib.bfgx_stats()
        _lib.call('bfgx_paint_grid', cat, model, grid, new_map.ctypes.data, opts, stats)
        self.last_stats = {k: getattr(stats, k) for k, _ in stats._fields_}
        del keep, cols, gkeep
        return new_map


class GridProfiles(_MapProfiles):
    """What MeasureProfilesGrid.process() returns.  Per (halo, bin), shape (n_halo, nb): `npix`, the pixels with a finite value and
    r_edges[b] <= x < r_edges[b + 1] inside the halo's ball, and `sum`, the sum of their values; with a shear pair `npix_shear`, `sum_t`
    and `sum_x` (None without one).  numpy arrays, or torch tensors on the maps' device when the maps were CUDA tensors.  `R` is the
    comoving halo radius R_com = mass_def.get_radius(M, a) / a and `R_q` = clip(epsilon_max R_com, 0, max(bins) / 2) the radius of the ball,
    per halo (numpy; NaN and 0 for an invalid halo); x is the comoving distance, or distance / R_com when `scaled`; `res` is the pixel size
    and `ndim` the map's dimension."""

    def __init__(self, r_edges, npix, sum, npix_shear=None, sum_t=None, sum_x=None, scaled=False, ndim=3, res=1.0, R=None, R_q=None):
        super().__init__(np.asarray(r_edges, dtype=np.float64), npix, sum, npix_shear, sum_t, sum_x, bool(scaled))
        self.ndim, self.res = int(ndim), float(res)
        self.R, self.R_q = R, R_q

    @property
    def density(self):
        """sum / (npix res^ndim), for maps that hold mass per pixel: the mean density of the counted pixels (NaN where npix is 0)"""
        return ratio(self.sum, self.npix * self.res ** self.ndim)

    @property
    def enclosed(self):
        """cumsum(sum, axis=1): the sum over the bins up to b.  This is M(< r_edges[b + 1]) only when r_edges[0] == 0."""
        return self.sum.cumsum(1)

    def stack(self, select=None, weights=None):
        """The pixel-weighted profile over the chosen halos per bin, sum_j w_j sum[j] / sum_j w_j npix[j] (NaN where the denominator is 0):
        a dict with 'mean', 'density' = 'mean' / res^ndim and, with shear, 'mean_t' and 'mean_x'.  select: anything that indexes the halo
        axis; weights: one per chosen halo (default 1)."""
        out = super().stack(select, weights)
        out['density'] = out['mean'] / self.res ** self.ndim
        return out


class MeasureProfilesGrid(DefaultRunnerGrid):
    """Measures halo-centred radial profiles of a gridded map: the regular-grid counterpart of MeasureProfilesShell and
    MeasureProfilesSnapshot, for what BaryonifyGrid, PaintProfilesGrid and ParticleSnapshot.make_map produce.

    Geometry.  map[i0, i1(, i2)] is the pixel whose centre is (x, y(, z)) = (bins[i0], bins[i1](, bins[i2])): where the grid runners put
    a halo (inds[x_inds, :][:, y_inds]) and what make_map produces.  res = bins[1] - bins[0], period L = Npix res,
    a = 1 / (1 + HaloNDCatalog.redshift); the cosmology is `_runner_cosmo()` (w0 is not passed on, as the grid runners have it).  A halo
    is valid iff M > 0 and M and its coordinates in use are finite; R_com = mass_def.get_radius(M, a) / a and
    R_q = clip(epsilon_max R_com, 0, max(bins) / 2), BaryonifyGrid's own clip.  Per axis Delta_k = bins[i_k] - x_k, minus L where
    Delta_k > L / 2, plus L where Delta_k < -L / 2, and d = sqrt(sum Delta_k^2) in fp64: the TRUE minimum-image distance, deliberately not
    the reference's cutout linspace(-N/2, N/2, N) res, which stretches radii by N / (N - 1) and swaps the sub-pixel dx and dy -- a
    measurement inherits neither quirk.  A pixel belongs to halo j iff d^2 <= R_q^2 (R_q < L / 2: at most once).  x = d (comoving Mpc) or,
    scaled=True, d / R_com; bin b holds r_edges[b] <= x < r_edges[b + 1].  A finite map value adds 1 to npix[j, b] and its value to
    sum[j, b]; a non-finite one is not counted.  shear=(g1, g2), a pair of 2D maps of the GriddedMap's shape, adds for every pixel with
    finite g1 and g2 and d > 0 one to npix_shear[j, b] and the flat-sky tangential and cross components about the halo,
    gamma_t + i gamma_x = -(g1 + i g2) exp(-2 i phi) with phi measured from +x towards +y, to sum_t and sum_x: a mass peak has gamma_t > 0.
    Invalid halos and halos without pixels get all-zero rows.  fp64 throughout; counts are exact.

    `model` must be None: there is nothing to tabulate.  `m.process(map=BaryonifyGrid(...).process())` measures the displaced map with the
    same object."""

    def __init__(self, HaloNDCatalog, GriddedMap, epsilon_max, model=None, use_ellipticity=False,
                 mass_def=MassDef(200, 'critical'), verbose=True, *, r_edges, scaled=False, shear=None):
        if model is not None:
            raise TypeError("MeasureProfilesGrid takes model=None: it measures the map, there is nothing to tabulate")
        if use_ellipticity:
            raise NotImplementedError("MeasureProfilesGrid measures in circular (spherical) bins: use_ellipticity is not implemented")
        super().__init__(HaloNDCatalog, GriddedMap, epsilon_max, model, use_ellipticity, mass_def, verbose)
        self.r_edges = check_r_edges(r_edges)
        self.scaled = bool(scaled)
        G = GriddedMap
        bins = np.asarray(G.bins, dtype=np.float64)
        if bins.ndim != 1 or bins.size != G.Npix:
            raise ValueError("GriddedMap.bins must hold one pixel-centre coordinate per pixel (%d != %d)" % (bins.size, G.Npix))
        res = bins[1] - bins[0]
        if not (np.all(np.isfinite(bins)) and res > 0 and np.all(np.abs(np.diff(bins) - res) <= 1e-9 * res)):
            raise ValueError("GriddedMap.bins must be uniformly spaced (to 1e-9 res): the minimum image needs a period")
        self.shape = (int(G.Npix),) * (2 if G.is2D else 3)
        self.shear = self._shear_pair(shear)

    def _shear_pair(self, shear):
        if shear is None:
            return None
        if len(shear) != 2:
            raise ValueError("shear must be a pair of maps (g1, g2)")
        if not self.GriddedMap.is2D:
            raise ValueError("shear is the flat-sky pair of a 2D map: it is not accepted for 3D maps")
        for g in shear:
            if tuple(g.shape if _is_cuda_tensor(g) else np.shape(g)) != self.shape:
                raise ValueError("shear maps must have the shape of the GriddedMap %s" % (self.shape,))
        return tuple(shear)

    def radii(self):
        """(R_com, R_q) per halo on the host: the comoving radius of the mass definition and the radius of the ball; NaN and 0 for a halo
        the measurement skips (M not positive / finite, a non-finite coordinate)."""
        return halo_radii(self.HaloNDCatalog.cat, ('x', 'y') if self.GriddedMap.is2D else ('x', 'y', 'z'), self.HaloNDCatalog.redshift, self.mass_def,
                          self._runner_cosmo(), self.epsilon_max, float(np.max(np.asarray(self.GriddedMap.bins, dtype=np.float64))) / 2)

    def process(self, map=None, shear=None):
        """GridProfiles of GriddedMap.map (and the constructor's shear pair), or of `map` / `shear` given here.  numpy in gives numpy out;
        C-contiguous CUDA float64 torch tensors of the map's shape are measured where they lie (on torch's current stream) and the result
        arrays are tensors on that device.  All inputs must be numpy arrays, or all CUDA tensors."""
        G = self.GriddedMap
        m = G.map if map is None else map
        pair = self.shear if shear is None else self._shear_pair(shear)
        maps = [m] + list(pair or ())
        on_dev = [_is_cuda_tensor(x) for x in maps]
        if any(on_dev) and not all(on_dev):
            raise ValueError("the map and the shear pair must all be numpy arrays or all CUDA tensors")
        hcat = self.HaloNDCatalog.cat
        model, keep = _placeholder_model(self, self._runner_cosmo())
        c, ckeep = _lib.make_grid_catalog_host(hcat['M'], hcat['x'], hcat['y'], None if G.is2D else hcat['z'])
        grid, gkeep = self._grid()
        edges, nb, n = self.r_edges, self.r_edges.size - 1, int(hcat.size)
        if all(on_dev):
            import torch
            dev = maps[0].device
            for x in maps:
                if x.dtype != torch.float64 or tuple(x.shape) != self.shape or x.device != dev or not x.is_contiguous():
                    raise ValueError("device maps must be C-contiguous float64 tensors of shape %s on one device" % (self.shape,))
            outs, optr = alloc_profile_outs(n, nb, pair, dev)
            ptr = [x.data_ptr() for x in maps] + [None] * (3 - len(maps))
            _lib.call('bfgx_grid_profiles_device', _tensors.device_index(dev), _tensors.stream(dev), c, model, grid, ptr[0], ptr[1], ptr[2], nb,
                      edges.ctypes.data, self.scaled, *optr)
        else:
            maps = [_lib.f8(x) for x in maps]
            for x in maps:
                if x.shape != self.shape:
                    raise ValueError("the map must have the shape of the GriddedMap %s: got %s" % (self.shape, x.shape))
            outs, optr = alloc_profile_outs(n, nb, pair)
            ptr = [x.ctypes.data for x in maps] + [None] * (3 - len(maps))
            _lib.call('bfgx_grid_profiles', c, model, grid, ptr[0], ptr[1], ptr[2], nb, edges.ctypes.data, self.scaled, self.device, *optr)
        del keep, ckeep, gkeep
        R, R_q = self.radii()
        return GridProfiles(edges.copy(), *outs, *([None] * (5 - len(outs))), scaled=self.scaled, ndim=len(self.shape), res=float(G.bins[1] - G.bins[0]),
                            R=R, R_q=R_q)
