"""CPU checks of the halo-centred profile measurement on particle snapshots: the numpy restatement (snapprofiles_oracle.py) against
scipy's periodic KD-tree (the reference's own tool), the argument rules of bfg.Runners.MeasureProfilesSnapshot and of the two C entries
(all refused before any device call), and the arithmetic of SnapshotProfiles on hand-made arrays."""
import ctypes as C

import numpy as np
import pytest

import snapprofiles_oracle as K
import baryonification_amd as bfg
from baryonification_amd import _lib
from baryonification_amd import synthetic as syn
from baryonification_amd.Runners import SnapshotRunner as SR
from baryonification_amd.Runners._model import _placeholder_model
from oracle import grid as G


def _objects(ndim=3, n=5, npart=40, L=64.0, seed=3):
    rng = np.random.default_rng(seed)
    h = rng.uniform(0, L, (n, 3))
    p = rng.uniform(0, L, (npart, 3))
    HCat = bfg.utils.HaloNDCatalog(x=h[:, 0], y=h[:, 1], z=h[:, 2] if ndim == 3 else None, M=np.full(n, 1e14), redshift=0.2, cosmo=syn.COSMO)
    Snap = bfg.utils.ParticleSnapshot(x=p[:, 0], y=p[:, 1], z=p[:, 2] if ndim == 3 else None, M=np.ones(npart), L=L, redshift=0.2, cosmo=syn.COSMO)
    return HCat, Snap


def _runner(ndim=3, **kw):
    HCat, Snap = _objects(ndim)
    kw.setdefault('r_edges', [0.0, 1.0, 2.0])
    return bfg.Runners.MeasureProfilesSnapshot(HCat, Snap, 5.0, verbose=False, **kw)


def test_runner_argument_errors():
    assert 'MeasureProfilesSnapshot' in SR.__all__ and issubclass(bfg.Runners.MeasureProfilesSnapshot, bfg.Runners.DefaultRunnerSnapshot)
    r = _runner()
    assert r.model is None and r.epsilon_max == 5.0 and r.scaled is False and r.r_edges.dtype == np.float64 and r.tree is None
    with pytest.raises(TypeError, match='model'):
        _runner(model=object())
    with pytest.raises(TypeError):
        bfg.Runners.MeasureProfilesSnapshot(r.HaloNDCatalog, r.ParticleSnapshot, 5.0)             # r_edges is required
    for bad in ([1.0, 1.0, 2.0], [2.0, 1.0], [-1.0, 1.0], [0.0, np.inf], [0.0, np.nan, 1.0]):
        with pytest.raises(ValueError, match='ascending'):
            _runner(r_edges=bad)
    with pytest.raises(ValueError, match='at least 2'):
        _runner(r_edges=[1.0])                                        # nb = 0
    with pytest.raises(ValueError, match='64'):
        _runner(r_edges=np.arange(66.0))                              # nb = 65
    assert _runner(r_edges=np.arange(65.0)).r_edges.size == 65        # nb = 64 is accepted
    with pytest.raises(ValueError, match='one weight per particle'):
        r.process(weights=np.ones(3))


def test_radii_follow_the_reference_ball():
    HCat, Snap = _objects(3)
    HCat.cat['M'][1], HCat.cat['M'][2], HCat.cat['x'][3] = -1e13, np.inf, np.nan
    r = bfg.Runners.MeasureProfilesSnapshot(HCat, Snap, 5.0, verbose=False, r_edges=[0.0, 1.0])
    R, R_q = r.radii()
    cat = {k: np.asarray(HCat.cat[k], dtype=np.float64) for k in ('M', 'x', 'y', 'z')}
    a, R_o, Rq_o, bad, pos = K.halo_scalars(cat, 3, Snap.L, 0.2, 5.0, G.grid_background(syn.COSMO))
    assert list(bad) == [False, True, True, True, False]
    assert np.array_equal(np.isnan(R), bad) and np.all(R_q[bad] == 0)
    assert np.allclose(R[~bad], R_o[~bad], rtol=1e-13) and np.allclose(R_q[~bad], Rq_o[~bad], rtol=1e-13)
    big = bfg.Runners.MeasureProfilesSnapshot(HCat, Snap, 500.0, verbose=False, r_edges=[0.0, 1.0]).radii()[1]
    assert np.all(big[~bad] == Snap.L / 2)                            # the clipped ball


def test_c_entries_refuse_bad_arguments_before_any_device_call():
    L = _lib.load()
    r = _runner()
    model, keep = _placeholder_model(r, syn.COSMO)
    hc = r.HaloNDCatalog.cat
    cat, ckeep = _lib.make_grid_catalog_host(hc['M'], hc['x'], hc['y'], hc['z'])
    pc = r.ParticleSnapshot.cat
    x, y, z, w = (np.ascontiguousarray(pc[k]) for k in ('x', 'y', 'z', 'M'))
    P = lambda v: v.ctypes.data                                       # noqa: E731
    n, npart = hc.size, x.size
    edges = np.arange(70.0)
    oi, od = np.zeros((n, 64), dtype=np.int64), np.zeros((n, 64))

    def snap(ndim=3, L_=64.0, zr=0.2, np_=npart, x_=P(x), z_=P(z)):
        return _lib.bfgx_snapshot(ndim, 0, np_, x_, P(y), z_, L_, zr)

    def host(cat_=C.byref(cat), model_=C.byref(model), w_=P(w), nb=2, e=P(edges), npart_=P(oi), s=P(od), null_snap=False, **kw):
        sn = snap(**kw)
        return L.bfgx_snapshot_profiles(cat_, model_, None if null_snap else C.byref(sn), w_, nb, e, 0, 0, npart_, s)

    def dev(cat_=C.byref(cat), model_=C.byref(model), w_=P(w), nb=2, e=P(edges), npart_=P(oi), s=P(od), ndim=3, L_=64.0, zr=0.2, np_=npart,
            x_=P(x), z_=P(z)):
        return L.bfgx_snapshot_profiles_device(0, None, cat_, model_, ndim, L_, zr, np_, x_, P(y), z_, w_, nb, e, 0, npart_, s)

    assert host(null_snap=True) == _lib.ERR_INVALID and b'NULL' in L.bfgx_last_error()
    for f in (host, dev):
        for kw in ({'cat_': None}, {'model_': None}, {'e': None}, {'npart_': None}, {'s': None}, {'w_': None}, {'x_': None}, {'z_': None}):
            assert f(**kw) == _lib.ERR_INVALID, kw
            assert b'NULL' in L.bfgx_last_error(), kw
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
        for kw, word in (({'ndim': 4}, b'ndim'), ({'ndim': 1}, b'ndim'), ({'L_': 0.0}, b'L must'), ({'L_': np.nan}, b'L must'), ({'zr': -1.0}, b'redshift'),
                         ({'np_': -1}, b'size'), ({'np_': 2 ** 32}, b'2^32')):
            assert f(**kw) == _lib.ERR_INVALID, kw
            assert word in L.bfgx_last_error(), (kw, L.bfgx_last_error())
        # everything in order: the only thing missing on a machine without a GPU is the device
        if L.bfgx_device_count() <= 0:
            assert f() == _lib.ERR_NO_DEVICE
            assert f(w_=None, s=None) == _lib.ERR_NO_DEVICE           # counts only
            assert f(ndim=2, z_=None) == _lib.ERR_NO_DEVICE           # a 2-D snapshot has no z
    del keep, ckeep


def test_process_without_a_gpu_fails_loudly():
    if _lib.load().bfgx_device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(_lib.BfgxError, match="no HIP device"):
        _runner().process()
    with pytest.raises(_lib.BfgxError, match="no HIP device"):
        _runner(ndim=2, scaled=True).process(weights=False)


@pytest.mark.parametrize('ndim', [2, 3])
def test_oracle_totals_match_scipys_periodic_kdtree(ndim):
    """2 000 particles, 50 halos, L = 64: per halo the oracle's particles inside the ball are those of cKDTree(boxsize=L).query_ball_point,
    the reference's own tool (SnapshotRunner.py:225), for every halo without a particle on the rim; all of them fall into one bin [0, L)"""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(11 + ndim)
    L, nh, npart, eps, zr = 64.0, 50, 2000, 5.0, 0.2
    M = (10 ** rng.uniform(13.0, 15.0, nh)).astype(np.float32).astype(np.float64)
    h = rng.uniform(0, L, (nh, ndim)).astype(np.float32).astype(np.float64)
    part = rng.uniform(0, L, (npart, ndim))
    part[:500] = (h[rng.integers(0, nh, 500)] + rng.normal(scale=1.0, size=(500, ndim))) % L
    M[3] = -1e14
    cat = {'M': M, 'x': h[:, 0], 'y': h[:, 1], 'z': h[:, 2] if ndim == 3 else np.zeros(nh)}
    p = K.pairs(part, L, cat, zr, eps, G.grid_background(syn.COSMO))
    o = K.measure(p, [0.0, L], rng.uniform(0.5, 2, npart))
    tree = cKDTree(part, boxsize=L)
    rim = np.bincount(p['halo'][p['rim']], minlength=nh) > 0
    assert np.count_nonzero(~rim) >= nh - 2 and o['npart'].sum() > 500
    for j in np.nonzero(~rim)[0]:
        want = 0 if p['bad'][j] else len(tree.query_ball_point(h[j] % L, p['R_q'][j]))
        assert o['npart'][j, 0] == want, j
    assert not o['npart'][3].any() and np.all(o['sum'] <= 2 * o['npart']) and np.all(o['sum'] >= 0.5 * o['npart'])


def test_snapshot_profiles_arithmetic():
    edges = np.array([0.0, 1.0, 2.0, 4.0])
    npart = np.array([[2, 0, 1], [4, 2, 3], [0, 0, 0]], dtype=np.int64)
    s = np.array([[4.0, 0.0, 1.0], [2.0, 6.0, 9.0], [0.0, 0.0, 0.0]])
    R, R_q = np.array([1.0, 0.5, np.nan]), np.array([3.0, 0.9, 0.0])  # halo 0: the last bin is cut by the ball; halo 1: two bins lie outside it
    p = SR.SnapshotProfiles(edges, npart, s, scaled=False, ndim=3, R=R, R_q=R_q)
    V = lambda r: 4 * np.pi * r ** 3 / 3                              # noqa: E731
    vol = p.volume
    assert vol.shape == (3, 3)
    assert np.allclose(vol[0], [V(1.0), V(2.0) - V(1.0), V(3.0) - V(2.0)], rtol=1e-15)
    assert np.allclose(vol[1], [V(0.9), 0.0, 0.0], rtol=1e-15) and vol[1, 1] == 0 and np.all(vol[2] == 0)
    mean = p.mean
    assert np.array_equal(np.isnan(mean), npart == 0) and mean[0, 0] == 2.0 and mean[1, 2] == 3.0
    dens = p.density
    assert np.allclose(dens[0], s[0] / vol[0]) and dens[1, 0] == 2.0 / V(0.9) and np.isnan(dens[1, 1]) and np.isnan(dens[1, 2]) and np.all(np.isnan(dens[2]))
    assert np.array_equal(p.enclosed, np.cumsum(s, axis=1))
    st = p.stack()
    assert np.allclose(st['mean'], [6.0 / 6, 6.0 / 2, 10.0 / 4]) and np.allclose(st['density'], s.sum(0) / vol.sum(0))
    st = p.stack(select=[0, 1], weights=[3.0, 1.0])
    assert st['mean'][0] == (3 * 4.0 + 2.0) / (3 * 2 + 4) and np.isclose(st['density'][2], (3 * 1.0 + 9.0) / (3 * vol[0, 2]))
    st = p.stack(select=np.array([False, False, True]))
    assert np.all(np.isnan(st['mean'])) and np.all(np.isnan(st['density']))
    # scaled: the edges are in units of R_com; 2-D: annuli
    q = SR.SnapshotProfiles(edges, npart, s, scaled=True, ndim=2, R=R, R_q=R_q)
    A = lambda r: np.pi * r ** 2                                      # noqa: E731
    assert np.allclose(q.volume[0], [A(1.0), A(2.0) - A(1.0), A(3.0) - A(2.0)], rtol=1e-15)
    assert np.allclose(q.volume[1], [A(0.5), A(0.9) - A(0.5), 0.0], rtol=1e-15) and np.all(np.isnan(q.volume[2]))
    # counts only: no sum, no mean; density and enclosed work on the counts
    c = SR.SnapshotProfiles(edges, npart, None, ndim=3, R=R, R_q=R_q)
    assert c.sum is None and c.mean is None and set(c.stack()) == {'density'}
    assert np.allclose(c.density[0], npart[0] / vol[0]) and np.array_equal(c.enclosed, np.cumsum(npart, axis=1))
