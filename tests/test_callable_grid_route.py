"""
CPU tests of the grid runners' per-halo route for plain-callable models (bfgx_grid_pairs_*, Runners/_model.py): the ABI is declared,
exported and bound and refuses bad arguments before any device call; the route is chosen only on request (model.bfgx_exact = True).
"""
import ctypes as C
import os
import re

import numpy as np

from baryonification_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ['bfgx_grid_pairs_begin', 'bfgx_grid_pairs_radii', 'bfgx_grid_pairs_apply', 'bfgx_grid_pairs_finish', 'bfgx_grid_pairs_end',
           'bfgx_snapshot_pairs_begin', 'bfgx_snapshot_pairs_radii', 'bfgx_snapshot_pairs_apply', 'bfgx_snapshot_pairs_finish',
           'bfgx_snapshot_pairs_end']


def test_grid_pairs_entries_are_declared_exported_and_bound():
    with open(os.path.join(REPO, 'include', 'bfgx.h')) as f:
        header = f.read()
    L = _lib.load()
    for name in ENTRIES:
        assert re.search(r'\b%s\(' % name, header), name
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name          # bound with a signature, not called through a bare pointer
    assert L.bfgx_abi_version() == 4                               # additive: the ABI version is unchanged


def test_grid_pairs_entries_refuse_bad_arguments_before_any_device_call():
    L = _lib.load()
    h = C.c_void_p()
    assert L.bfgx_grid_pairs_begin(None, None, None, 0, 0, C.byref(h), None) == _lib.ERR_INVALID and not h.value
    assert b'NULL' in L.bfgx_last_error()
    cat = _lib.bfgx_grid_catalog()
    cat.n = 3                                                       # halos but no columns and no counts array
    m = _lib.bfgx_model()
    bins = np.arange(8) + 0.5
    grid, keep = _lib.make_grid(bins, 2, 0.0)
    counts = np.zeros(3, dtype=np.int64)
    assert L.bfgx_grid_pairs_begin(C.byref(cat), C.byref(m), C.byref(grid), 0, 0, C.byref(h), None) == _lib.ERR_INVALID
    assert L.bfgx_grid_pairs_begin(C.byref(cat), C.byref(m), C.byref(grid), 0, 0, C.byref(h), counts.ctypes.data) == _lib.ERR_INVALID
    cat.n = -1
    assert L.bfgx_grid_pairs_begin(C.byref(cat), C.byref(m), C.byref(grid), 0, 0, C.byref(h), counts.ctypes.data) == _lib.ERR_INVALID
    assert not h.value
    assert L.bfgx_grid_pairs_radii(None, 0, 0, None) == _lib.ERR_INVALID
    assert L.bfgx_grid_pairs_apply(None, 0, 0, None) == _lib.ERR_INVALID
    assert L.bfgx_grid_pairs_finish(None, None, None, 1, None) == _lib.ERR_INVALID
    L.bfgx_grid_pairs_end(None)                                                   # (a no-op)
    del keep


def test_snapshot_pairs_entries_refuse_bad_arguments_before_any_device_call():
    L = _lib.load()
    h = C.c_void_p()
    assert L.bfgx_snapshot_pairs_begin(None, None, None, 0, C.byref(h), None) == _lib.ERR_INVALID and not h.value
    cat = _lib.bfgx_grid_catalog()
    cat.n = 2
    m = _lib.bfgx_model()
    s = _lib.bfgx_snapshot(3, 0, 0, None, None, None, 10.0, 0.0)
    counts = np.zeros(2, dtype=np.int64)
    assert L.bfgx_snapshot_pairs_begin(C.byref(cat), C.byref(m), C.byref(s), 0, C.byref(h), None) == _lib.ERR_INVALID
    assert L.bfgx_snapshot_pairs_begin(C.byref(cat), C.byref(m), C.byref(s), 0, C.byref(h), counts.ctypes.data) == _lib.ERR_INVALID   # no columns
    cat.n = 0
    s.ndim = 4
    assert L.bfgx_snapshot_pairs_begin(C.byref(cat), C.byref(m), C.byref(s), 0, C.byref(h), counts.ctypes.data) == _lib.ERR_INVALID
    s.ndim, s.L = 3, -1.0
    assert L.bfgx_snapshot_pairs_begin(C.byref(cat), C.byref(m), C.byref(s), 0, C.byref(h), counts.ctypes.data) == _lib.ERR_INVALID
    assert not h.value
    assert L.bfgx_snapshot_pairs_radii(None, 0, 0, None) == _lib.ERR_INVALID
    assert L.bfgx_snapshot_pairs_apply(None, 0, 0, None) == _lib.ERR_INVALID
    assert L.bfgx_snapshot_pairs_finish(None, None, None, None, None) == _lib.ERR_INVALID
    L.bfgx_snapshot_pairs_end(None)


class _Plain(object):
    def displacement(self, r, M, a):
        return 0 * r

    def projected(self, cosmo, r, M, a):
        return 0 * r

    def real(self, cosmo, r, M, a):
        return 0 * r


def _grid_runners(model, ndim):
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    rng = np.random.default_rng(0)
    N, L = 16, 20.0
    bins = (np.arange(N) + 0.5) * (L / N)
    x, y, z = rng.uniform(0, L, (3, 10))
    HCat = bfg.utils.HaloNDCatalog(x=x, y=y, z=z if ndim == 3 else None, M=np.full(10, 1e14), redshift=0.2, cosmo=syn.COSMO)
    GMap = bfg.utils.GriddedMap(map=np.ones((N,) * ndim), redshift=0.2, bins=bins, cosmo=syn.COSMO)
    return (bfg.Runners.BaryonifyGrid(HCat, GMap, 4.0, model, verbose=False),
            bfg.Runners.PaintProfilesGrid(HCat, GMap, 4.0, model, verbose=False))


def test_grid_runners_take_the_per_halo_route_only_when_asked():
    from baryonification_amd.Runners import _model as RM
    for ndim in (2, 3):
        m = _Plain()
        bary, paint = _grid_runners(m, ndim)
        kind = 'projected' if ndim == 2 else 'real'
        assert not RM.wants_exact(bary, 'displacement') and not RM.wants_exact(paint, kind)      # unset: tabulated (the default)
        m.bfgx_exact = False
        assert not RM.wants_exact(bary, 'displacement') and not RM.wants_exact(paint, kind)
        m.bfgx_exact = 1                                                                      # only True itself asks for it
        assert not RM.wants_exact(bary, 'displacement')
        m.bfgx_exact = True
        assert RM.wants_exact(bary, 'displacement') and RM.wants_exact(paint, kind)
    # snapshot runners: the same rule
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    m = _Plain()
    rng = np.random.default_rng(1)
    H = bfg.utils.HaloNDCatalog(x=rng.uniform(0, 10, 4), y=rng.uniform(0, 10, 4), z=rng.uniform(0, 10, 4), M=np.full(4, 1e14), redshift=0.0,
                                cosmo=syn.COSMO)
    P = rng.uniform(0, 10, (3, 50))
    S = bfg.utils.ParticleSnapshot(x=P[0], y=P[1], z=P[2], M=np.ones(50), L=10.0, redshift=0.0, cosmo=syn.COSMO)
    snap = bfg.Runners.BaryonifySnapshot(H, S, 4.0, m, verbose=False)
    assert not RM.wants_exact(snap, 'displacement')
    m.bfgx_exact = True
    assert RM.wants_exact(snap, 'displacement')
    # table models ignore the flag
    t = bfg.utils.TabulatedProfile(None, bfg.utils.Cosmology.from_dict(syn.COSMO))
    t.bfgx_exact = True
    assert not RM.wants_exact(_grid_runners(t, 2)[1], 'projected')


def test_the_shell_answers_are_unchanged():
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    from baryonification_amd.Runners import _model as RM
    cat = syn.make_catalog(50)
    Catalog = bfg.utils.HaloLightConeCatalog(ra=cat['ra'], dec=cat['dec'], M=cat['M'], z=cat['z'], cosmo=syn.COSMO)
    Shell = bfg.utils.LightconeShell(map=np.ones(12 * 16 * 16), cosmo=syn.COSMO)
    m = _Plain()
    r = bfg.Runners.BaryonifyShell(Catalog, Shell, 5.0, m, verbose=False)
    assert RM.wants_exact(r, 'displacement') is True                  # by size
    m.bfgx_exact = False
    assert RM.wants_exact(r, 'displacement') is False
    m.bfgx_exact = 1                                                  # (shells: any truthy flag, as before)
    assert RM.wants_exact(r, 'displacement') is True


def test_halo_batches_cover_the_catalog_and_respect_the_budget():
    from baryonification_amd.Runners import _model as RM
    counts = np.array([5, 0, 3, 12, 0, 1, 1, 4], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    for budget in (1, 4, 6, 100):
        b = list(RM._halo_batches(off, budget))
        assert b[0][0] == 0 and b[-1][1] == counts.size and all(b[i][1] == b[i + 1][0] for i in range(len(b) - 1))
        for j0, j1 in b:
            assert j1 > j0 and (off[j1] - off[j0] <= budget or j1 == j0 + 1)
    assert list(RM._halo_batches(np.zeros(1, dtype=np.int64), 10)) == []
