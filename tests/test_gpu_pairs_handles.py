"""
GPU tests of the handles behind the per-halo entries bfgx_{shell,grid,snapshot}_pairs_* (csrc/bfgx_pairs.hpp): a handle of one family is
refused by the entries of the other two and is none the worse for it; `end` gives back every device allocation of the handle, also right
after `begin` and when `begin` itself is refused after the handle exists; an empty catalog goes through every call; batches that split
the catalog between halos give the one-batch result.

Shapes: shell NSIDE 16 with 4 halos, grid 2-D npix 32 and 3-D npix 16 with 3 halos, snapshot 3-D with 300 particles strictly inside
(0, L) and 3 halos.  The halos stand apart (no pixel or particle belongs to two of them) and the shell and grid handles paint, so every
accumulated sum has one term and no regrid follows: the result does not depend on the order of the device's atomic additions, and two
runs on the same inputs are compared bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import callable_models as CM

EPS = {'shell': 10.0, 'grid': 4.0, 'snapshot': 4.0}
L_BOX = 32.0
FAMILIES = ['shell', 'grid2', 'grid3', 'snapshot']


def _placeholder(eps):
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    from baryonification_amd.Runners._model import _placeholder_model

    class R(object):
        mass_def = bfg.utils.MassDef(200, 'critical')
        epsilon_max = eps
    return _placeholder_model(R, syn.COSMO)


def _particles(n=300, x0=None):
    rng = np.random.default_rng(7)
    P = rng.uniform(0.01 * L_BOX, 0.99 * L_BOX, (3, n))
    if x0 is not None:
        P[0, 0] = x0
    return P


class _Family(object):
    """the fixed tiny inputs of one family and its calls; n: halos kept (0: the empty catalog); paint: shell and grid only"""

    def __init__(self, which, n=None, paint=1, refuse=False):
        from baryonification_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.which, self.family = which, 'grid' if which.startswith('grid') else which
        self.paint = paint
        self.model, self._keep = _placeholder(EPS[self.family])
        if refuse and self.family != 'snapshot':
            self.model.eps_runner = 0.0                  # refused by the plan's validation, which begin reaches with the handle in hand
        if which == 'shell':
            n = 4 if n is None else n
            cols = [np.full(4, 1e15), np.array([0.03, 0.04, 0.05, 0.035]), np.array([10.0, 100.0, 190.0, 280.0]), np.array([0.0, 30.0, -30.0, 60.0])]
            self.cat, self._ckeep = _lib.make_catalog_host(*[c[:n] for c in cols])
            self.size = 12 * 16 * 16
        else:
            n = 3 if n is None else n
            self.ndim = 2 if which == 'grid2' else 3
            M = np.array([1e14, 2e14, 1.5e14])[:n]
            x, y, z = (np.array(v)[:n] for v in ([6.0, 16.0, 26.0], [6.0, 24.0, 8.0], [7.0, 25.0, 16.0]))
            self.cat, self._ckeep = _lib.make_grid_catalog_host(M, x, y, z if self.ndim == 3 else None)
            if self.family == 'grid':
                npix = 32 if self.ndim == 2 else 16
                self.grid, self._gkeep = _lib.make_grid((np.arange(npix) + 0.5) * (L_BOX / npix), self.ndim, 0.2)
                self.size = npix ** self.ndim
            else:
                self.P = _particles(x0=1.5 * L_BOX if refuse else None)
                self.snap = _lib.bfgx_snapshot(3, 0, self.P.shape[1], self.P[0].ctypes.data, self.P[1].ctypes.data, self.P[2].ctypes.data, L_BOX, 0.0)
                self.size = self.P.shape[1]
        self.n = n
        self.h = C.c_void_p()
        self.counts = np.zeros(max(n, 1), dtype=np.int64)

    def begin(self):
        a = (C.byref(self.cat), C.byref(self.model))
        out = (C.byref(self.h), self.counts.ctypes.data)
        if self.which == 'shell':
            return self.lib.bfgx_shell_pairs_begin(*a, 16, self.paint, 0, *out)
        if self.family == 'grid':
            return self.lib.bfgx_grid_pairs_begin(*a, C.byref(self.grid), self.paint, 0, *out)
        return self.lib.bfgx_snapshot_pairs_begin(*a, C.byref(self.snap), 0, *out)

    def end(self):
        getattr(self.lib, 'bfgx_%s_pairs_end' % self.family)(self.h)
        self.h = C.c_void_p()

    def entries_on(self, h):
        """the status of each radii / apply / finish entry of this family when it is given the handle h, with every other argument valid"""
        buf = np.zeros(1 << 16)
        src, dst = np.ones(self.size), [np.zeros(self.size) for _ in range(3)]
        st = self._lib.bfgx_stats()
        p, L = buf.ctypes.data, self.lib
        if self.which == 'shell':
            return [L.bfgx_shell_pairs_radii(h, p), L.bfgx_shell_pairs_apply(h, p, src.ctypes.data, dst[0].ctypes.data, 0, C.byref(st))]
        if self.family == 'grid':
            return [L.bfgx_grid_pairs_radii(h, 0, 0, p), L.bfgx_grid_pairs_apply(h, 0, 0, p),
                    L.bfgx_grid_pairs_finish(h, src.ctypes.data, dst[0].ctypes.data, 0, C.byref(st))]
        return [L.bfgx_snapshot_pairs_radii(h, 0, 0, p), L.bfgx_snapshot_pairs_apply(h, 0, 0, p),
                L.bfgx_snapshot_pairs_finish(h, dst[0].ctypes.data, dst[1].ctypes.data, dst[2].ctypes.data, C.byref(st))]

    def run(self, map_in=None, check_mass=1):
        """radii -> values (a smooth function of the radii) -> apply -> finish on the handle begin made; every call must return BFGX_OK.
        Returns (the map, or the positions as an array (3, np); n_pairs)."""
        check, L, h = self._lib.check, self.lib, self.h
        total = int(self.counts[:self.n].sum())
        r = np.zeros(max(total, 1))
        st = self._lib.bfgx_stats()
        src = None if map_in is None else map_in.ctypes.data
        if self.which == 'shell':
            check(L.bfgx_shell_pairs_radii(h, r.ctypes.data))
            vals = 0.01 / (1.0 + r)
            out = np.full(self.size, np.nan)
            check(L.bfgx_shell_pairs_apply(h, vals.ctypes.data, src, out.ctypes.data, check_mass, C.byref(st)))
        elif self.family == 'grid':
            check(L.bfgx_grid_pairs_radii(h, 0, self.n, r.ctypes.data))
            vals = 0.01 / (1.0 + r)
            check(L.bfgx_grid_pairs_apply(h, 0, self.n, vals.ctypes.data))
            out = np.full(self.size, np.nan)
            check(L.bfgx_grid_pairs_finish(h, src, out.ctypes.data, check_mass, C.byref(st)))
        else:
            check(L.bfgx_snapshot_pairs_radii(h, 0, self.n, r.ctypes.data))
            vals = -0.05 * r
            check(L.bfgx_snapshot_pairs_apply(h, 0, self.n, vals.ctypes.data))
            out = np.full((3, self.size), np.nan)
            check(L.bfgx_snapshot_pairs_finish(h, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, C.byref(st)))
        assert st.n_pairs == total
        return out, total


@pytest.mark.gpu
def test_families_do_not_mix(gpu):
    from baryonification_amd import _lib
    fams = [_Family(w) for w in FAMILIES]
    try:
        for f in fams:
            _lib.check(f.begin())
            assert f.h.value and f.counts.sum() > 0
        for f in fams:
            for g in fams:
                if g.family != f.family:
                    assert g.entries_on(f.h) == [_lib.ERR_INVALID] * (2 if g.which == 'shell' else 3), (f.which, g.which)
                    assert b'not a handle of bfgx_%s_pairs_begin' % g.family.encode() in f.lib.bfgx_last_error()
        results = [f.run() for f in fams]
    finally:
        for f in fams:
            f.end()
    for w, (out, total) in zip(FAMILIES, results):
        fresh = _Family(w)
        try:
            _lib.check(fresh.begin())
            ref, total_ref = fresh.run()
        finally:
            fresh.end()
        assert total == total_ref and np.isfinite(out).all()
        assert np.array_equal(out, ref), w                                  # bit for bit
        if w == 'snapshot':
            assert np.abs(out - fresh.P).max() > 0                          # (particles moved: the sequence did its work)
        else:
            assert np.abs(out).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize('which', FAMILIES)
def test_everything_is_released(gpu, which):
    from baryonification_amd import _lib
    live = _lib.load().bfgx_debug_live_allocs
    # a completed sequence
    f = _Family(which)
    before = live()
    _lib.check(f.begin())
    assert live() > before
    f.run()
    f.end()
    assert live() == before
    # end directly after begin
    f = _Family(which)
    _lib.check(f.begin())
    assert live() > before
    f.end()
    assert live() == before
    # a begin that is refused after the handle exists (snapshot: one particle at x = 1.5 L, found after the uploads)
    f = _Family(which, refuse=True)
    assert f.begin() == _lib.ERR_INVALID and not f.h.value
    assert live() == before
    f.end()                                                                 # (NULL: a no-op)
    assert live() == before


@pytest.mark.gpu
@pytest.mark.parametrize('which,paint', [('shell', 1), ('shell', 0), ('grid2', 1), ('grid2', 0), ('grid3', 1), ('grid3', 0), ('snapshot', 0)])
def test_empty_catalog(gpu, which, paint):
    from baryonification_amd import _lib
    f = _Family(which, n=0, paint=paint)
    map_in = None
    if f.family != 'snapshot' and not paint:
        map_in = np.random.default_rng(3).poisson(4.0, f.size).astype(np.float64)
    try:
        _lib.check(f.begin())
        out, total = f.run(map_in=map_in, check_mass=1)                     # (check raises unless every call returns BFGX_OK)
    finally:
        f.end()
    assert total == 0
    if f.family == 'snapshot':
        assert np.abs(out - f.P).max() <= 1e-15 * L_BOX
    elif paint:
        assert np.array_equal(out, np.zeros(f.size))
    else:
        assert np.isfinite(out).all() and out.sum() > 0                     # check_mass = 1 passed: no exception above


HALOS = dict(x=[6.0, 16.0, 24.0], y=[6.0, 24.0, 10.0], z=[7.0, 25.0, 16.0], M=[1e14, 1e14, 6e14])     # the last one outweighs the other two together


def _grid_runner(ndim, kind, model):
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    npix = 32 if ndim == 2 else 16
    bins = (np.arange(npix) + 0.5) * (L_BOX / npix)
    HCat = bfg.utils.HaloNDCatalog(x=HALOS['x'], y=HALOS['y'], z=HALOS['z'] if ndim == 3 else None, M=HALOS['M'], redshift=0.2, cosmo=syn.COSMO)
    m = np.random.default_rng(5).poisson(4.0, (npix,) * ndim).astype(np.float64) if kind == 'baryonify' else np.zeros((npix,) * ndim)
    GMap = bfg.utils.GriddedMap(map=m, redshift=0.2, bins=bins, cosmo=syn.COSMO)
    cls = bfg.Runners.BaryonifyGrid if kind == 'baryonify' else bfg.Runners.PaintProfilesGrid
    return cls(HCat, GMap, EPS['grid'], model, verbose=False)


def _snap_runner(model):
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    P = _particles()
    HCat = bfg.utils.HaloNDCatalog(redshift=0.0, cosmo=syn.COSMO, **HALOS)
    Snap = bfg.utils.ParticleSnapshot(x=P[0], y=P[1], z=P[2], M=np.ones(P.shape[1]), L=L_BOX, redshift=0.0, cosmo=syn.COSMO)
    return bfg.Runners.BaryonifySnapshot(HCat, Snap, EPS['snapshot'], model, verbose=False)


def _one_batch_then_straddling(monkeypatch, process):
    """process() with the default budget (one batch), then with EXACT_BATCH_PAIRS one below the largest halo's pair count: the two light
    halos share a batch, the heavy one is a batch of its own.  Returns the two results."""
    from baryonification_amd.Runners import _model as RM
    seen, real = [], RM._halo_batches

    def spy(off, budget):
        for b in real(off, budget):
            seen.append((b, np.diff(off)))
            yield b
    monkeypatch.setattr(RM, '_halo_batches', spy)
    one = process()
    assert [b for b, _ in seen] == [(0, 3)]
    counts = seen[0][1]
    print('pair counts per halo:', counts.tolist())
    del seen[:]
    monkeypatch.setattr(RM, 'EXACT_BATCH_PAIRS', int(counts.max()) - 1)
    many = process()
    assert [b for b, _ in seen] == [(0, 2), (2, 3)] and counts[0] > 0 and counts[1] > 0
    return one, many


@pytest.mark.gpu
@pytest.mark.parametrize('ndim,kind', [(2, 'baryonify'), (2, 'paint'), (3, 'baryonify'), (3, 'paint')])
def test_grid_batches_straddle_halos(gpu, ndim, kind, monkeypatch):
    models = []

    def process():
        models.append(CM.CallableDisplacement() if kind == 'baryonify' else CM.CallableProfile())
        return _grid_runner(ndim, kind, models[-1]).process()
    one, many = _one_batch_then_straddling(monkeypatch, process)
    assert models[0].calls == models[1].calls == 3
    assert np.abs(one).max() > 0
    assert np.abs(many - one).max() <= 1e-13 * np.abs(one).max()            # (fp64 atomics: the order of the sums may differ)


@pytest.mark.gpu
def test_snapshot_batches_straddle_halos(gpu, monkeypatch):
    models = []

    def process():
        models.append(CM.CallableDisplacement())
        cat = _snap_runner(models[-1]).process()
        return np.stack([cat[k] for k in 'xyz'])
    one, many = _one_batch_then_straddling(monkeypatch, process)
    assert models[0].calls == models[1].calls == 3
    assert np.abs(one - _particles()).max() > 0
    assert np.abs(many - one).max() <= 1e-13 * L_BOX
