"""CPU checks of the halo-centred profile measurement on gridded maps: the argument rules of bfg.Runners.MeasureProfilesGrid and of the two C
entries (all refused before any device call), radii() against the numpy restatement (gridprofiles_oracle.py), the restatement against a
literal all-pixels loop, and the arithmetic of GridProfiles on hand-made arrays."""
import ctypes as C

import numpy as np
import pytest

import gridprofiles_oracle as K
import baryonification_amd as bfg
from baryonification_amd import _lib
from baryonification_amd import synthetic as syn
from baryonification_amd.Runners import Map2DRunner as MR
from baryonification_amd.Runners._model import _placeholder_model
from oracle import grid as G


def _objects(ndim=3, n=5, N=16, L=64.0, seed=3):
    rng = np.random.default_rng(seed)
    h = rng.uniform(0, L, (n, 3))
    bins = (np.arange(N) + 0.5) * L / N
    HCat = bfg.utils.HaloNDCatalog(x=h[:, 0], y=h[:, 1], z=h[:, 2] if ndim == 3 else None, M=np.full(n, 1e14), redshift=0.2, cosmo=syn.COSMO)
    Map = bfg.utils.GriddedMap(map=rng.uniform(0.5, 2.0, (N,) * ndim), redshift=0.2, bins=bins, cosmo=syn.COSMO)
    return HCat, Map


def _runner(ndim=3, **kw):
    HCat, Map = _objects(ndim)
    kw.setdefault('r_edges', [0.0, 1.0, 2.0])
    return bfg.Runners.MeasureProfilesGrid(HCat, Map, 5.0, verbose=False, **kw)


def test_runner_argument_errors():
    assert 'MeasureProfilesGrid' in MR.__all__ and 'GridProfiles' in MR.__all__
    assert issubclass(bfg.Runners.MeasureProfilesGrid, bfg.Runners.DefaultRunnerGrid)
    r = _runner()
    assert r.model is None and r.epsilon_max == 5.0 and r.scaled is False and r.r_edges.dtype == np.float64 and r.shear is None
    with pytest.raises(TypeError, match='takes model=None: it measures the map, there is nothing to tabulate'):
        _runner(model=object())
    with pytest.raises(NotImplementedError, match='ellipticity'):
        _runner(use_ellipticity=True)
    with pytest.raises(TypeError):
        bfg.Runners.MeasureProfilesGrid(r.HaloNDCatalog, r.GriddedMap, 5.0)                      # r_edges is required
    for bad in ([1.0, 1.0, 2.0], [2.0, 1.0], [-1.0, 1.0], [0.0, np.inf], [0.0, np.nan, 1.0]):
        with pytest.raises(ValueError, match='ascending'):
            _runner(r_edges=bad)
    with pytest.raises(ValueError, match='at least 2'):
        _runner(r_edges=[1.0])                                        # nb = 0
    with pytest.raises(ValueError, match='at least 2'):
        _runner(r_edges=[[0.0, 1.0], [2.0, 3.0]])                     # not 1-D
    with pytest.raises(ValueError, match='64'):
        _runner(r_edges=np.arange(66.0))                              # nb = 65
    assert _runner(r_edges=np.arange(65.0)).r_edges.size == 65        # nb = 64 is accepted
    # the shear pair: 2D maps only, the map's shape, a pair
    g = np.zeros((16, 16))
    assert len(_runner(ndim=2, shear=(g, g)).shear) == 2
    with pytest.raises(ValueError, match='3D'):
        _runner(ndim=3, shear=(np.zeros((16, 16, 16)), np.zeros((16, 16, 16))))
    with pytest.raises(ValueError, match='shape'):
        _runner(ndim=2, shear=(g, np.zeros((16, 15))))
    with pytest.raises(ValueError, match='shape'):
        _runner(ndim=2, shear=(np.zeros(256), np.zeros(256)))
    with pytest.raises(ValueError, match='pair'):
        _runner(ndim=2, shear=(g, g, g))
    with pytest.raises(ValueError, match='shape'):
        _runner(ndim=2).process(shear=(g, np.zeros((8, 8))))
    with pytest.raises(ValueError, match='shape'):
        _runner(ndim=2).process(map=np.zeros((8, 8)))
    # the bins: one centre per pixel, uniformly spaced
    HCat, Map = _objects(2)
    for bins in (Map.bins[:-1], np.concatenate([Map.bins[:-1], [Map.bins[-1] * (1 + 1e-6)]]), Map.bins ** 2, Map.bins[::-1]):
        bad_map = bfg.utils.GriddedMap(map=Map.map, redshift=0.2, bins=bins, cosmo=syn.COSMO)
        with pytest.raises(ValueError, match='bins'):
            bfg.Runners.MeasureProfilesGrid(HCat, bad_map, 5.0, verbose=False, r_edges=[0.0, 1.0])


def test_radii_follow_the_grid_runners_ball():
    for ndim in (2, 3):
        HCat, Map = _objects(ndim)
        HCat.cat['M'][1], HCat.cat['M'][2], HCat.cat['x'][3] = -1e13, np.inf, np.nan
        r = bfg.Runners.MeasureProfilesGrid(HCat, Map, 5.0, verbose=False, r_edges=[0.0, 1.0])
        R, R_q = r.radii()
        cat = {k: np.asarray(HCat.cat[k], dtype=np.float64) for k in ('M', 'x', 'y', 'z')}
        a, R_o, Rq_o, bad, pos = K.halo_scalars(cat, ndim, Map.bins, 0.2, 5.0, G.grid_background(syn.COSMO))
        assert list(bad) == [False, True, True, True, False]
        assert np.array_equal(np.isnan(R), bad) and np.all(R_q[bad] == 0)
        assert np.allclose(R[~bad], R_o[~bad], rtol=1e-13) and np.allclose(R_q[~bad], Rq_o[~bad], rtol=1e-13)
        big = bfg.Runners.MeasureProfilesGrid(HCat, Map, 500.0, verbose=False, r_edges=[0.0, 1.0]).radii()[1]
        assert np.all(big[~bad] == np.max(Map.bins) / 2)              # the clipped ball: BaryonifyGrid's max(bins) / 2, not L / 2
    # a z column that is not finite does not matter to a 2D map
    HCat, Map = _objects(2)
    HCat.cat['z'][0] = np.nan
    assert np.all(np.isfinite(bfg.Runners.MeasureProfilesGrid(HCat, Map, 5.0, verbose=False, r_edges=[0.0, 1.0]).radii()[0]))


@pytest.mark.parametrize('ndim', [2, 3])
def test_oracle_equals_a_literal_loop_over_every_pixel(ndim):
    """the restatement's pruned outer product against the definition written out: every pixel of the grid, one halo at a time"""
    rng = np.random.default_rng(40 + ndim)
    N, L, nh, zr, eps = 12, 30.0, 8, 0.2, 5.0
    bins = (np.arange(N) + 0.5) * L / N
    M = (10 ** rng.uniform(13.5, 15.5, nh)).astype(np.float32).astype(np.float64)
    h = rng.uniform(0, L, (nh, 3)).astype(np.float32).astype(np.float64)
    h[0] = 0.0
    M[1], M[2] = -1.0, np.float64(np.float32(1e16))                  # not a halo; a ball clipped to max(bins) / 2
    cat = {'M': M, 'x': h[:, 0], 'y': h[:, 1], 'z': h[:, 2]}
    m = rng.uniform(0.5, 2.0, (N,) * ndim)
    m.flat[5] = np.nan
    edges = np.array([0.0, 2.0, 5.0, 9.0, 20.0])
    bg = G.grid_background(syn.COSMO)
    p = K.pairs(bins, ndim, cat, zr, eps, bg)
    o = K.measure(p, edges, m)
    assert np.any(p['R_q'] == np.max(bins) / 2) and o['npix'].sum() > 100 and not o['npix'][1].any()
    a, R_com, R_q, bad, pos = K.halo_scalars(cat, ndim, bins, zr, eps, bg)
    coords = np.stack(np.meshgrid(*[bins] * ndim, indexing='ij'), axis=-1).reshape(-1, ndim)
    for j in range(nh):
        want_n, want_s = np.zeros(4, dtype=np.int64), np.zeros(4)
        if not bad[j]:
            D = K.min_image(coords - pos[j], L)
            d = np.sqrt((D * D).sum(1))
            for b in range(4):
                sel = (d * d <= R_q[j] ** 2 * (1 + 1e-12)) & (d >= edges[b]) & (d < edges[b + 1]) & np.isfinite(m.reshape(-1))
                want_n[b], want_s[b] = np.count_nonzero(sel), m.reshape(-1)[sel].sum()
        assert np.all(np.abs(o['npix'][j] - want_n) <= o['amb_n'][j]), j
        assert np.allclose(o['sum'][j], want_s, rtol=1e-12, atol=3.0 * o['amb_n'][j].max()), j
    assert o['amb_n'].sum() <= 6


def test_c_entries_refuse_bad_arguments_before_any_device_call():
    L = _lib.load()
    r3, r2 = _runner(3), _runner(2)
    model, keep = _placeholder_model(r3, r3._runner_cosmo())
    hc = r3.HaloNDCatalog.cat
    cat, ckeep = _lib.make_grid_catalog_host(hc['M'], hc['x'], hc['y'], hc['z'])
    cat_noz, nkeep = _lib.make_grid_catalog_host(hc['M'], hc['x'], hc['y'])
    bins = np.ascontiguousarray(r3.GriddedMap.bins, dtype=np.float64)
    m3, m2 = np.ascontiguousarray(r3.GriddedMap.map), np.ascontiguousarray(r2.GriddedMap.map)
    g = np.zeros((16, 16))
    P = lambda v: v.ctypes.data                                       # noqa: E731
    n = hc.size
    edges = np.arange(70.0)
    oi, od, oi2, od2, od3 = (np.zeros((n, 64), dtype=dt) for dt in (np.int64, np.float64, np.int64, np.float64, np.float64))

    def grid(ndim=3, npix=16, bins_=P(bins), zr=0.2):
        return _lib.bfgx_grid(ndim, npix, bins_, zr)

    def args(cat_=C.byref(cat), model_=C.byref(model), map_=None, g1=None, g2=None, nb=2, e=P(edges), npix_=P(oi), s=P(od), ns=None, st=None,
             sx=None, null_grid=False, **kw):
        gr = grid(**kw)
        if map_ is None:
            map_ = P(m3) if gr.ndim == 3 else P(m2)
        return gr, cat_, model_, None if null_grid else C.byref(gr), map_, g1, g2, nb, e, npix_, s, ns, st, sx

    def host(**kw):
        gr, cat_, model_, grp, map_, g1, g2, nb, e, npix_, s, ns, st, sx = args(**kw)
        return L.bfgx_grid_profiles(cat_, model_, grp, map_, g1, g2, nb, e, 0, 0, npix_, s, ns, st, sx)

    def dev(**kw):
        gr, cat_, model_, grp, map_, g1, g2, nb, e, npix_, s, ns, st, sx = args(**kw)
        return L.bfgx_grid_profiles_device(0, None, cat_, model_, grp, map_, g1, g2, nb, e, 0, npix_, s, ns, st, sx)

    shear_out = dict(ns=P(oi2), st=P(od2), sx=P(od3))
    for f in (host, dev):
        for kw in ({'cat_': None}, {'model_': None}, {'null_grid': True}, {'map_': 0}, {'e': None}, {'npix_': None}, {'s': None}, {'bins_': None},
                   {'cat_': C.byref(cat_noz)},                                                      # a 3D grid needs the z column
                   dict(ndim=2, g1=P(g), **shear_out), dict(ndim=2, g2=P(g), **shear_out),          # exactly one of g1 and g2
                   dict(ndim=2, g1=P(g), g2=P(g)), dict(ndim=2, g1=P(g), g2=P(g), ns=P(oi2), st=P(od2)),   # shear maps without their outputs
                   dict(ndim=2, g1=P(g), g2=P(g), st=P(od2), sx=P(od3))):
            assert f(**kw) == _lib.ERR_INVALID, kw
            assert b'NULL' in L.bfgx_last_error(), (kw, L.bfgx_last_error())
        for kw in (dict(ndim=2, ns=P(oi2)), dict(ndim=2, st=P(od2)), dict(ndim=2, **shear_out)):    # shear outputs without shear maps
            assert f(**kw) == _lib.ERR_INVALID, kw
            assert b'shear pair' in L.bfgx_last_error(), (kw, L.bfgx_last_error())
        assert f(ndim=3, g1=P(m3), g2=P(m3), **shear_out) == _lib.ERR_INVALID                       # a shear pair on a 3D grid
        assert b'2D grids only' in L.bfgx_last_error()
        for nb in (0, 65, -3):
            assert f(nb=nb) == _lib.ERR_INVALID
            assert b'64' in L.bfgx_last_error()
        for bad in ([0.0, 2.0, 1.0], [1.0, 1.0, 3.0]):
            arr = np.array(bad)
            assert f(e=P(arr)) == _lib.ERR_INVALID
            assert b'ascending' in L.bfgx_last_error()
        for bad in ([-1.0, 0.0, 1.0], [0.0, 1.0, np.inf], [0.0, np.nan, 1.0]):
            arr = np.array(bad)
            assert f(e=P(arr)) == _lib.ERR_INVALID
            assert b'finite' in L.bfgx_last_error()
        uneven = bins.copy()
        uneven[7] += 1e-6
        for kw, word in (({'ndim': 4}, b'ndim'), ({'ndim': 1}, b'ndim'), ({'npix': 4}, b'npix'), ({'zr': -1.0}, b'redshift'),
                         ({'bins_': P(uneven)}, b'uniformly'), ({'bins_': P(bins[::-1].copy())}, b'ascending')):
            assert f(**kw) == _lib.ERR_INVALID, kw
            assert word in L.bfgx_last_error(), (kw, L.bfgx_last_error())
        # everything in order: the only thing missing on a machine without a GPU is the device
        if L.bfgx_device_count() <= 0:
            assert f() == _lib.ERR_NO_DEVICE
            assert f(ndim=2, cat_=C.byref(cat_noz)) == _lib.ERR_NO_DEVICE                           # a 2D grid has no z
            assert f(ndim=2, g1=P(g), g2=P(g), **shear_out) == _lib.ERR_NO_DEVICE
    del keep, ckeep, nkeep


def test_process_without_a_gpu_fails_loudly():
    if _lib.load().bfgx_device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(_lib.BfgxError, match="no HIP device"):
        _runner().process()
    g = np.zeros((16, 16))
    with pytest.raises(_lib.BfgxError, match="no HIP device"):
        _runner(ndim=2, scaled=True, shear=(g, g)).process()


def test_grid_profiles_arithmetic():
    edges = np.array([0.0, 1.0, 2.0, 4.0])
    npix = np.array([[2, 0, 1], [4, 2, 3], [0, 0, 0]], dtype=np.int64)
    s = np.array([[4.0, 0.0, 1.0], [2.0, 6.0, 9.0], [0.0, 0.0, 0.0]])
    R, R_q = np.array([1.0, 0.5, np.nan]), np.array([3.0, 0.9, 0.0])
    p = MR.GridProfiles(edges, npix, s, scaled=False, ndim=3, res=0.5, R=R, R_q=R_q)
    assert p.ndim == 3 and p.res == 0.5 and p.scaled is False and p.npix_shear is None and p.mean_t is None and p.mean_x is None
    mean = p.mean
    assert np.array_equal(np.isnan(mean), npix == 0) and mean[0, 0] == 2.0 and mean[1, 2] == 3.0
    dens = p.density
    assert np.array_equal(np.isnan(dens), npix == 0) and dens[0, 0] == 4.0 / (2 * 0.125) and dens[1, 1] == 6.0 / (2 * 0.125)
    assert np.array_equal(p.enclosed, np.cumsum(s, axis=1))
    st = p.stack()
    assert set(st) == {'mean', 'density'}
    assert np.allclose(st['mean'], [6.0 / 6, 6.0 / 2, 10.0 / 4]) and np.allclose(st['density'], st['mean'] / 0.125)
    st = p.stack(select=[0, 1], weights=[3.0, 1.0])
    assert st['mean'][0] == (3 * 4.0 + 2.0) / (3 * 2 + 4) and st['mean'][1] == 6.0 / 2 and st['density'][2] == (3 * 1.0 + 9.0) / (3 * 1 + 3) / 0.125
    st = p.stack(select=np.array([False, False, True]))
    assert np.all(np.isnan(st['mean'])) and np.all(np.isnan(st['density']))
    # 2-D with shear: res^2, and the shear means go by npix_shear
    ns = np.array([[1, 0, 1], [4, 2, 2], [0, 0, 0]], dtype=np.int64)
    t = np.array([[0.5, 0.0, -1.0], [2.0, 1.0, 3.0], [0.0, 0.0, 0.0]])
    q = MR.GridProfiles(edges, npix, s, ns, t, -t, scaled=True, ndim=2, res=0.5, R=R, R_q=R_q)
    assert q.density[0, 0] == 4.0 / (2 * 0.25) and q.scaled is True
    assert np.array_equal(np.isnan(q.mean_t), ns == 0) and q.mean_t[0, 0] == 0.5 and q.mean_t[1, 2] == 1.5 and q.mean_x[1, 2] == -1.5
    st = q.stack()
    assert set(st) == {'mean', 'density', 'mean_t', 'mean_x'}
    assert np.allclose(st['mean_t'], [2.5 / 5, 1.0 / 2, 2.0 / 3]) and np.allclose(st['mean_x'], -st['mean_t'])
    st = q.stack(select=slice(0, 2), weights=np.array([2.0, 1.0]))
    assert st['mean_t'][2] == (2 * -1.0 + 3.0) / (2 * 1 + 2)
