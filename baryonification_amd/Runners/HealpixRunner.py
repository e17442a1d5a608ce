"""
HEALPix-shell runners: drop-in for BaryonForge/Runners/HealpixRunner.py (`DefaultRunner` :74-221,
`BaryonifyShell` :223-349, `PaintProfilesShell` :352-447).  Same constructor (positional order and
attribute names, as SplitJoinParallel re-instantiates runners positionally -- Parallelize.py:237-271),
same `process()` return value (float64 map of shape (Npix,)) and the same exceptions.

`process()` does no per-halo work in Python: the catalog, the shell and the model's raw table go
through the C ABI (include/bfgx.h) to the HIP kernels in csrc/.  There is no CPU fallback.
"""
import numpy as np

from .. import _lib, _tensors
from ..utils.cosmology import MassDef
from ..utils.Tabulate import ParamTabulatedProfile
from ..utils.pixelfunc import scatter_add
from ._model import _placeholder_model, build_model, cosmo_to_dict, process_callable_exact, wants_exact
from ._profiles import MAX_PROFILE_BINS, _MapProfiles, _is_cuda_tensor, alloc_profile_outs, check_r_edges      # noqa: F401 (MAX_PROFILE_BINS: importable from here)

__all__ = ['DefaultRunner', 'BaryonifyShell', 'PaintProfilesShell', 'MeasureProfilesShell', 'regrid_pixels_hpix']


def regrid_pixels_hpix(hmap, parent_pix_vals, child_pix, child_weights):
    """hmap[child_pix[i, j]] += child_weights[i, j] * parent_pix_vals[i] for j < 4, IN PLACE, and returns hmap
    (HealpixRunner.py:14-67).  hmap: a C-contiguous 1-D float64 numpy array or a CUDA float64 tensor.  child_pix (any integer dtype)
    and child_weights have shape (N, 4): transpose what get_interp_weights returns.  Indices in [-npix, npix) wrap as Python indices
    do; any other index raises IndexError before anything runs.  Duplicate targets accumulate, by fp64 atomic adds on the GPU, so
    the last bits of a pixel's sum can differ from run to run."""
    return scatter_add(hmap, parent_pix_vals, child_pix, child_weights)


class DefaultRunner(object):

    def __init__(self, HaloLightConeCatalog, LightconeShell, epsilon_max, model, use_ellipticity=False,
                 mass_def=MassDef(200, 'critical'), verbose=True):
        self.HaloLightConeCatalog = HaloLightConeCatalog
        self.LightconeShell = LightconeShell
        self.cosmo = HaloLightConeCatalog.cosmology
        self.model = model
        self.epsilon_max = epsilon_max
        self.mass_def = mass_def
        self.verbose = verbose
        self.use_ellipticity = use_ellipticity
        # engine knobs (not in the reference): plain attributes so the runner stays picklable
        self.device = 0
        self.acc_f64 = None            # None -> per-runner default
        self.algo = 1                  # 1 = LDS tiles, 0 = per-halo global atomics
        self.last_stats = None
        if use_ellipticity:
            raise NotImplementedError("You have set use_ellipticity = True, but this not yet implemented for HealpixRunner")

    def build_Rmat(self, A, ref):
        """2 x 2 rotation by the angle between A and ref (HealpixRunner.py:170-197); both are normalised IN PLACE, as there."""
        for v in (A, ref):
            v /= np.linalg.norm(v)
        angle = np.arccos(np.dot(A, ref))
        c, s = np.cos(angle), np.sin(angle)
        return np.array([[c, -s], [s, c]])

    def coord_array(self, *args):
        """(N, len(args)) array of the flattened arguments, one per column (HealpixRunner.py:200-218)"""
        return np.stack([np.ravel(a) for a in args], axis=1)

    # -- shared plumbing -----------------------------------------------------------------------
    def _check_keys(self, keys):
        if len(keys) > 0:                                             # HealpixRunner.py:284-287, :409-412
            txt = (f"You asked to use {keys} properties in Baryonification. You must pass a ParamTabulatedProfile"
                   f"as the model. You have passed {type(self.model)} instead")
            ok = isinstance(self.model, ParamTabulatedProfile) or type(self.model).__name__ == 'ParamTabulatedProfile'
            assert ok, txt

    def _catalog(self, keys):
        """(bfgx_catalog over contiguous float64 columns, keep-alive, verify).  The catalog is a structured array (strided columns), so
        every process() call would gather M, z, ra, dec into contiguous buffers and take two numpy logs over all halos (the table
        coordinates np.log(1/a), np.log(M)): ~20 ms per 1e6 halos.  These are kept on the catalog object between calls, keyed by a hash
        of the WHOLE record buffer (xxh3 over every byte of every halo), so that any in-place edit of the catalog -- one halo, a swap
        that leaves sums unchanged -- is seen, as it is by the reference, which re-reads `cat` on every call.  The hash (~2 ms per 1e6
        halos) is taken by a worker thread WHILE the GPU call runs on the cached columns (ctypes releases the GIL); `verify()` joins
        it after the call and returns False if the catalog has changed, in which case the caller drops the result, and the call is
        repeated on fresh columns.  (xxhash is optional: hashlib.blake2b stands in.)"""
        cat = self.HaloLightConeCatalog.cat
        names = ['M', 'z', 'ra', 'dec'] + list(keys)
        cached = getattr(self.HaloLightConeCatalog, '_bfgx_columns', None)
        verify = None
        if cached is not None and cached[0] is not None and cached[0][:3] == (cat.size, str(cat.dtype), tuple(names)):
            fut = _hash_pool().submit(_catalog_fingerprint, cat, names)
            expect = cached[0]
            verify = lambda: fut.result() == expect                               # noqa: E731
        else:
            cached = self._catalog_rebuild(cat, names)
        cols = cached[1]
        c, keep = _lib.make_catalog_host(cols[0], cols[1], cols[2], cols[3], cols[4:], coords=cached[2])
        # bfgx_opts.catalog_token: the columns stay on the device between calls under the hash of the bytes they were made from
        self._catalog_token = 0 if cached[0] is None else ((cached[0][3] ^ (hash(cached[0][2]) & 0xFFFFFFFFFFFFFFFF)) & 0xFFFFFFFFFFFFFFFF) | 1
        return c, keep, verify

    def _catalog_rebuild(self, cat, names):
        finger = _catalog_fingerprint(cat, names)
        cols = [_lib.f8(cat[k]) for k in names]
        cached = (finger, cols, _lib.table_coords(cols[0], cols[1]))
        if finger is not None:
            try:
                self.HaloLightConeCatalog._bfgx_columns = cached
            except AttributeError:
                pass
        return cached

    def _call_with_catalog(self, keys, call):
        """call(bfgx_catalog) with the cached columns; repeated on fresh ones if the catalog turns out to have been edited in place"""
        cat, cols, verify = self._catalog(keys)
        try:
            out = call(cat)
        except Exception:
            if verify is None or verify():
                raise                                 # the columns were current: the error is real
            out = None
        if verify is not None and not verify():
            try:
                del self.HaloLightConeCatalog._bfgx_columns
            except AttributeError:
                pass
            cat, cols, _ = self._catalog(keys)
            out = call(cat)
        del cols
        return out


_HASH_POOL = None


def _hash_pool():
    global _HASH_POOL
    if _HASH_POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _HASH_POOL = ThreadPoolExecutor(1, thread_name_prefix='bfgx-catalog-hash')
    return _HASH_POOL


def _catalog_fingerprint(cat, names):
    """(size, dtype, column names, 64-bit hash of all record bytes): xxh3 where the (optional) xxhash module is present (~2 ms per 1e6
    halos), hashlib's blake2b otherwise (~25 ms: still hidden behind the GPU call by the worker thread, and the columns are still cached)"""
    buf = cat if cat.flags.c_contiguous else np.ascontiguousarray(cat)
    if not cat.size:
        return (cat.size, str(cat.dtype), tuple(names), 0)
    try:
        import xxhash
        digest = xxhash.xxh3_64(buf.view(np.uint8)).intdigest()
    except ImportError:
        import hashlib
        digest = int.from_bytes(hashlib.blake2b(buf.view(np.uint8), digest_size=8).digest(), 'little')
    return (cat.size, str(cat.dtype), tuple(names), digest)


class BaryonifyShell(DefaultRunner):
    """Displaces the mass of a HEALPix shell around every halo (map must be a MASS map: pixels equal
    to 0 are treated as empty, HealpixRunner.py:231-232, :335)."""

    def process(self):
        keys = vars(self.model).get('p_keys', [])
        self._check_keys(keys)
        if wants_exact(self, 'displacement'):        # a plain Python callable on a small catalog: called per halo, as the reference does (:321)
            return process_callable_exact(self, 'displacement', self.LightconeShell.map)
        model, p_keys, keep = build_model(self, 'displacement')
        orig_map = _lib.f8(self.LightconeShell.map)
        nside = int(self.LightconeShell.NSIDE)
        new_map = _lib.pinned_empty(orig_map.size)          # page-locked: the D2H copy of the result runs at PCIe rate
        # acc_f64: None (default) / 'auto' = the engine picks the precision from the model's table -- fp32 pair math while the table moves a pixel
        # by less than 0.1 pixel sides, the parity-grade mode (fp64 pair math, split fp32 pix_offsets, fp64 regrid geometry) beyond: either way
        # within SURVEY 8(d)'s 1e-6 mean(map) of the fp64 reference; True = fp64 throughout (1e-10), False = fp32 pair math whatever the table,
        # 'parity' = the parity-grade mode whatever the table (include/bfgx.h BFGX_ACC_*)
        opts = _lib.bfgx_opts(int(self.device), _lib.acc_mode(self.acc_f64), 1, 1, int(self.algo), 0)
        stats = _lib.bfgx_stats()

        def call(cat):
            opts.catalog_token = self._catalog_token
            _lib.call('bfgx_baryonify_shell', cat, model, nside, orig_map.ctypes.data, new_map.ctypes.data, opts, stats)
        self._call_with_catalog(p_keys, call)
        self.last_stats = {k: getattr(stats, k) for k, _ in stats._fields_}
        del keep
        return new_map


class PaintProfilesShell(DefaultRunner):
    """Paints a tabulated projected profile around every halo into an empty map."""

    def process(self):
        keys = vars(self.model).get('p_keys', []) if self.model is not None else []
        self._check_keys(keys)
        assert self.model is not None, "You must provide a model"     # HealpixRunner.py:415
        if wants_exact(self, 'projected'):           # (:441)
            return process_callable_exact(self, 'projected')
        model, p_keys, keep = build_model(self, 'projected')
        nside = int(self.LightconeShell.NSIDE)
        new_map = _lib.pinned_empty(self.LightconeShell.map.size)
        # acc_f64: None (default) / 2 / 'mixed' = fp32 pair math (chord, ln r, read-out, exp) accumulated in fp64 into the fp64 map -- the
        # same split BaryonifyShell's default has, what bench.py --mode paint times; stated fp64 -> fp32 tolerance: 5e-5 of the pixel's
        # value.  True = fp64 throughout (1e-10 parity with the reference, 2.3x slower); False = fp32 map
        acc64 = 2 if (self.acc_f64 is None or self.acc_f64 in (2, 'mixed')) else int(bool(self.acc_f64))
        opts = _lib.bfgx_opts(int(self.device), 0, acc64, 0, int(self.algo), 0)
        stats = _lib.bfgx_stats()

        def call(cat):
            opts.catalog_token = self._catalog_token
            _lib.call('bfgx_paint_shell', cat, model, nside, new_map.ctypes.data, opts, stats)
        self._call_with_catalog(p_keys, call)
        self.last_stats = {k: getattr(stats, k) for k, _ in stats._fields_}
        del keep
        return new_map


class ShellProfiles(_MapProfiles):
    """What MeasureProfilesShell.process() returns: per (halo, bin) the counted pixels and the sums, shape (n_halo, nb); the shear fields
    are None without a shear pair.  numpy arrays, or torch tensors on the maps' device when the maps were CUDA tensors."""


class MeasureProfilesShell(DefaultRunner):
    """Measures halo-centred radial profiles of a shell map: the adjoint of PaintProfilesShell (same discs, same separations, a gather
    where painting scatters).  For halo j the pixels of query_disc(NSIDE, vec_j, R_j epsilon_max / D_j) are binned in r_sep / a_j
    (comoving Mpc, what the profile models are called with) or, scaled=True, in r_sep / R_j: bin b holds r_edges[b] <= x < r_edges[b + 1].
    LightconeShell.map is the scalar map (y, kappa, density contrast); shear=(g1, g2) adds a spin-2 pair in the convention of
    utils.sphtfunc (HEALPix: components on e_theta, e_phi) whose tangential and cross components about the halo,
    gamma_t + i gamma_x = -(g1 + i g2) exp(-2 i phi), are summed too: a mass peak has gamma_t > 0, a pure E field gamma_x = 0.
    Pixels that are not finite or UNSEEN are not counted.  fp64 throughout.  `model` must be None: there is nothing to tabulate."""

    def __init__(self, HaloLightConeCatalog, LightconeShell, epsilon_max, model=None, use_ellipticity=False,
                 mass_def=MassDef(200, 'critical'), verbose=True, *, r_edges, scaled=False, shear=None):
        if model is not None:
            raise TypeError("MeasureProfilesShell takes model=None: it measures the map, there is nothing to tabulate")
        super().__init__(HaloLightConeCatalog, LightconeShell, epsilon_max, model, use_ellipticity, mass_def, verbose)
        self.r_edges = check_r_edges(r_edges)
        self.scaled = bool(scaled)
        self.shear = self._shear_pair(shear, int(LightconeShell.NSIDE))

    @staticmethod
    def _shear_pair(shear, nside):
        if shear is None:
            return None
        if len(shear) != 2:
            raise ValueError("shear must be a pair of maps (g1, g2)")
        for g in shear:
            n = g.numel() if _is_cuda_tensor(g) else np.asarray(g).size
            if n != 12 * nside * nside:
                raise ValueError("shear maps must have the NSIDE of the shell (%d): got %d pixels" % (nside, n))
        return tuple(shear)

    def process(self, map=None, shear=None):
        """ShellProfiles of the shell's map (and the constructor's shear pair), or of `map` / `shear` given here.  CUDA float64 torch tensors
        given here are measured where they lie and the result arrays are tensors on that device."""
        nside = int(self.LightconeShell.NSIDE)
        m = self.LightconeShell.map if map is None else map
        pair = self.shear if shear is None else self._shear_pair(shear, nside)
        maps = [m] + list(pair or ())
        on_dev = [_is_cuda_tensor(x) for x in maps]
        if any(on_dev) and not all(on_dev):
            raise ValueError("the map and the shear pair must all be numpy arrays or all CUDA tensors")
        model, keep = _placeholder_model(self, cosmo_to_dict(self.cosmo))
        edges, nb = self.r_edges, self.r_edges.size - 1
        n = int(self.HaloLightConeCatalog.cat.size)
        if all(on_dev):
            import torch
            dev = maps[0].device
            for x in maps:
                if x.dtype != torch.float64 or x.dim() != 1 or x.numel() != 12 * nside * nside or x.device != dev:
                    raise ValueError("device maps must be 1-D float64 tensors of 12 NSIDE^2 pixels on one device")
            maps = [x.contiguous() for x in maps]
            outs, optr = alloc_profile_outs(n, nb, pair, dev)
            ptr = [x.data_ptr() for x in maps] + [None] * (3 - len(maps))

            def call(cat):
                _lib.call('bfgx_shell_profiles_device', _tensors.device_index(dev), _tensors.stream(dev), cat, model, nside, ptr[0], ptr[1],
                          ptr[2], nb, edges.ctypes.data, self.scaled, *optr)
        else:
            maps = [_lib.f8(x).reshape(-1) for x in maps]
            if maps[0].size != 12 * nside * nside:
                raise ValueError("the map must have 12 NSIDE^2 = %d pixels" % (12 * nside * nside))
            outs, optr = alloc_profile_outs(n, nb, pair)
            ptr = [x.ctypes.data for x in maps] + [None] * (3 - len(maps))

            def call(cat):
                _lib.call('bfgx_shell_profiles', cat, model, nside, ptr[0], ptr[1], ptr[2], nb, edges.ctypes.data, self.scaled, self.device, *optr)
        self._call_with_catalog([], call)
        del keep
        return ShellProfiles(edges.copy(), *outs, scaled=self.scaled)
