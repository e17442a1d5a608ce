"""CPU checks of the halo-centred profile measurement: the numpy restatement (stack_oracle.py) against a brute-force evaluation over
all pixels, the sign and angle conventions of the tangential shear on a Kaiser-Squires shear field, and the argument rules of
bfg.Runners.MeasureProfilesShell and of the two C entries (all refused before any device call)."""
import ctypes as C

import numpy as np
import pytest

import sht_oracle as SO
import sht_spin_oracle as SP
import stack_oracle as K
import baryonification_amd as bfg
from baryonification_amd import _lib
from baryonification_amd import synthetic as syn
from baryonification_amd.Runners import HealpixRunner as HR
from baryonification_amd.Runners._model import _placeholder_model
from oracle import oracle as O

EPS = 2.2e-16


@pytest.mark.parametrize('nside,eps,edges', [(16, 1000.0, np.geomspace(40.0, 4000.0, 7)), (64, 250.0, np.geomspace(10.0, 800.0, 9))])
@pytest.mark.parametrize('scaled', [False, True])
def test_oracle_matches_brute_force(nside, eps, edges, scaled):
    """every pixel of the sphere, the angle by arccos and no query_disc, against the oracle's discs; cells with an ambiguous pixel (an
    edge or the rim of the disc within rounding) are compared within those pixels"""
    n = 40 if nside == 16 else 60
    cat = syn.make_catalog(n, seed=4242 + nside)
    cat['dec'][:2] = [89.9, -89.95]                                   # a pole inside the disc
    cat['M'][2] = -1.0                                                # invalid halos: all-zero rows
    cat['z'][3] = -1.5
    bg = O.Background.from_dict(syn.COSMO)
    rng = np.random.default_rng(7)
    npx = 12 * nside * nside
    m, g1, g2 = rng.poisson(8.0, npx).astype(float), rng.normal(size=npx), rng.normal(size=npx)
    m[rng.integers(0, npx, 40)] = K.UNSEEN
    g1[rng.integers(0, npx, 40)] = np.nan
    g2[rng.integers(0, npx, 40)] = K.UNSEEN
    if scaled:
        edges = np.geomspace(0.03 * eps, 1.01 * eps, edges.size)      # r / R_j instead of comoving Mpc
    o = K.measure(K.discs(nside, cat, eps, bg), edges, m, (g1, g2), scaled)
    b = K.brute_force(nside, cat, eps, bg, edges, m, (g1, g2), scaled)
    assert o['npix'].sum() > 20 * n and np.count_nonzero(o['npix']) > 2 * n
    assert not o['npix'][2].any() and not o['npix'][3].any() and not o['npix_shear'][2].any() and not o['sum_t'][3].any()
    clean = o['amb_n'] == 0
    assert clean.mean() > 0.99
    assert np.array_equal(o['npix'][clean], b['npix'][clean]) and np.array_equal(o['npix_shear'][clean], b['npix_shear'][clean])
    assert np.all(np.abs(o['npix'] - b['npix']) <= o['amb_n']) and np.all(np.abs(o['npix_shear'] - b['npix_shear']) <= o['amb_n'])
    assert np.all(np.abs(o['sum'] - b['sum']) <= 2 * o['npix'] * EPS * o['S'] + o['amb_abs'])
    with np.errstate(divide='ignore'):
        bound = (2 * o['npix_shear'] * EPS + 8 * EPS / o['theta_min']) * o['S_g'] + o['amb_abs_g']
    assert np.all(np.abs(o['sum_t'] - b['sum_t']) <= bound) and np.all(np.abs(o['sum_x'] - b['sum_x']) <= bound)


def test_tangential_shear_sign_and_angle_on_a_kaiser_squires_field():
    """A Gaussian convergence bump (sigma 0.12 rad) at (ra, dec) = (40.3, 25.7) deg, NSIDE 32, lmax 64, its shear by the Kaiser-Squires
    recipe of utils/sphtfunc.py through the numpy transforms: in eight rings between 0.02 and 0.5 rad the oracle's mean_t over the flat-sky
    value kappa_bar(< theta) - kappa(theta) = (1 - e^-u) / u - e^-u, u = theta^2 / (2 sigma^2), averaged over the same pixels, lies in
    [0.90, 1.05] (the wrong sign gives -1, a wrong factor of two in the angle about 0) and |mean_x| <= 1e-10 (a pure E field)."""
    nside, lmax, sigma, ra, dec = 32, 64, 0.12, 40.3, 25.7
    npx = 12 * nside * nside
    vec = K.hp.ang2vec(ra, dec, lonlat=True)
    v = np.stack(K.hp.pix2vec(nside, np.arange(npx)), axis=1)
    theta = 2 * np.arcsin(0.5 * np.sqrt(np.sum((v - vec) ** 2, axis=1)))
    u = theta ** 2 / (2 * sigma ** 2)
    kappa = np.exp(-u)
    flat = -np.expm1(-u) / u - np.exp(-u)
    klm = SO.map2alm(kappa, nside, lmax, lmax, iter=3)
    ell = np.concatenate([np.arange(m_, lmax + 1) for m_ in range(lmax + 1)]).astype(float)
    with np.errstate(divide='ignore', invalid='ignore'):
        fac = np.where(ell >= 2, np.sqrt((ell + 2) * (ell - 1) / (ell * (ell + 1))), 0.0)
    g1, g2 = SP.alm2map_spin([fac * klm, 0 * klm], nside, 2, lmax, lmax)
    # one halo whose disc reaches beyond 0.5 rad; bin edges in comoving Mpc that are the eight rings in angle
    cat = {'M': np.array([1e14]), 'z': np.array([0.25]), 'ra': np.array([ra]), 'dec': np.array([dec])}
    bg = O.Background.from_dict(syn.COSMO)
    a, R, D, radius, bad = K.halo_scalars(cat, 1.0, bg)
    eps = 0.55 / radius[0]
    edges = D[0] * 2 * np.sin(0.5 * np.linspace(0.02, 0.5, 9)) / a[0]
    d = K.discs(nside, cat, eps, bg)
    o = K.measure(d, edges, flat, (g1, g2), scaled=False)
    assert np.all(o['npix_shear'][0] >= 10) and np.array_equal(o['npix_shear'], o['npix'])
    ratio = o['mean_t'][0] / o['mean'][0]
    print('mean_t / flat-sky value per ring:', ratio, ' mean_x:', o['mean_x'][0])
    assert np.all(ratio >= 0.90) and np.all(ratio <= 1.05), ratio
    assert np.all(o['mean_t'][0] > 0)
    assert np.all(np.abs(o['mean_x'][0]) <= 1e-10), o['mean_x'][0]


def _runner(nside=8, n=5, **kw):
    cat = syn.make_catalog(n, seed=3)
    Catalog = bfg.utils.HaloLightConeCatalog(ra=cat['ra'], dec=cat['dec'], M=cat['M'], z=cat['z'], cosmo=syn.COSMO)
    Shell = bfg.utils.LightconeShell(map=np.ones(12 * nside * nside), cosmo=syn.COSMO)
    kw.setdefault('r_edges', [0.0, 1.0, 2.0])
    return bfg.Runners.MeasureProfilesShell(Catalog, Shell, 10.0, verbose=False, **kw)


def test_runner_argument_errors():
    assert 'MeasureProfilesShell' in bfg.Runners.HealpixRunner.__all__ and issubclass(bfg.Runners.MeasureProfilesShell, bfg.Runners.DefaultRunner)
    r = _runner()
    assert r.model is None and r.epsilon_max == 10.0 and r.scaled is False and r.shear is None and r.r_edges.dtype == np.float64
    import pickle
    r2 = pickle.loads(pickle.dumps(r))
    assert np.array_equal(r2.r_edges, r.r_edges) and r2.epsilon_max == r.epsilon_max
    with pytest.raises(TypeError, match='model'):
        _runner(model=object())
    with pytest.raises(TypeError):
        bfg.Runners.MeasureProfilesShell(r.HaloLightConeCatalog, r.LightconeShell, 10.0)           # r_edges is required
    for bad in ([1.0, 1.0, 2.0], [2.0, 1.0], [-1.0, 1.0], [0.0, np.inf], [0.0, np.nan, 1.0]):
        with pytest.raises(ValueError, match='ascending'):
            _runner(r_edges=bad)
    with pytest.raises(ValueError, match='at least 2'):
        _runner(r_edges=[1.0])                                        # nb = 0
    with pytest.raises(ValueError, match='64'):
        _runner(r_edges=np.arange(66.0))                              # nb = 65
    assert _runner(r_edges=np.arange(65.0)).r_edges.size == 65        # nb = 64 is accepted
    npx = 12 * 8 * 8
    with pytest.raises(ValueError, match='NSIDE'):
        _runner(shear=(np.zeros(npx), np.zeros(4 * npx)))
    with pytest.raises(ValueError, match='pair'):
        _runner(shear=(np.zeros(npx),))
    with pytest.raises(ValueError, match='NSIDE'):
        r.process(shear=(np.zeros(npx // 4), np.zeros(npx // 4)))
    with pytest.raises(NotImplementedError):
        _runner(use_ellipticity=True)


def test_c_entries_refuse_bad_arguments_before_any_device_call():
    L = _lib.load()
    r = _runner()
    model, keep = _placeholder_model(r, syn.COSMO)
    cols = [np.ascontiguousarray(r.HaloLightConeCatalog.cat[k], dtype=np.float64) for k in ('M', 'z', 'ra', 'dec')]
    cat, ckeep = _lib.make_catalog_host(*cols)
    nside, npx, n = 8, 12 * 64, cols[0].size
    m = np.ones(npx)
    edges = np.arange(70.0)
    oi, od = np.zeros((n, 64), dtype=np.int64), np.zeros((n, 64))
    P = lambda x: x.ctypes.data                                       # noqa: E731

    def host(cat_=C.byref(cat), model_=C.byref(model), nside_=nside, map_=P(m), g1=None, g2=None, nb=2, e=P(edges), npix=P(oi), s=P(od),
             ns=None, st=None, sx=None):
        return L.bfgx_shell_profiles(cat_, model_, nside_, map_, g1, g2, nb, e, 0, 0, npix, s, ns, st, sx)

    def dev(cat_=C.byref(cat), model_=C.byref(model), nside_=nside, map_=P(m), g1=None, g2=None, nb=2, e=P(edges), npix=P(oi), s=P(od),
            ns=None, st=None, sx=None):
        return L.bfgx_shell_profiles_device(0, None, cat_, model_, nside_, map_, g1, g2, nb, e, 0, npix, s, ns, st, sx)

    for f in (host, dev):
        for kw in ({'cat_': None}, {'model_': None}, {'map_': None}, {'e': None}, {'npix': None}, {'s': None}, {'g1': P(m)}, {'g2': P(m)},
                   {'g1': P(m), 'g2': P(m)}, {'g1': P(m), 'g2': P(m), 'ns': P(oi), 'st': P(od)}):
            assert f(**kw) == _lib.ERR_INVALID, kw
            assert b'NULL' in L.bfgx_last_error()
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
        for ns_ in (0, -4, 16384):
            assert f(nside_=ns_) == _lib.ERR_INVALID
            assert b'nside' in L.bfgx_last_error()
        # everything in order: the only thing missing on a machine without a GPU is the device
        if L.bfgx_device_count() <= 0:
            assert f() == _lib.ERR_NO_DEVICE
    del keep, ckeep


def test_stack_arithmetic():
    npix = np.array([[2, 0, 1], [4, 0, 3], [0, 0, 5]], dtype=np.int64)
    s = np.array([[4.0, 0.0, 1.0], [2.0, 0.0, 9.0], [0.0, 0.0, 10.0]])
    p = HR.ShellProfiles(np.arange(4.0), npix, s, npix.copy(), 2 * s, -s)
    mean = p.mean
    assert np.array_equal(np.isnan(mean), npix == 0) and mean[0, 0] == 2.0 and mean[1, 2] == 3.0 and p.mean_t[1, 0] == 1.0 and p.mean_x[2, 2] == -2.0
    st = p.stack()
    assert st['mean'][0] == 6.0 / 6 and np.isnan(st['mean'][1]) and st['mean'][2] == 20.0 / 9
    assert np.allclose(st['mean_t'][[0, 2]], 2 * st['mean'][[0, 2]]) and np.allclose(st['mean_x'][[0, 2]], -st['mean'][[0, 2]])
    st = p.stack(select=[0, 1], weights=[3.0, 1.0])
    assert st['mean'][0] == (3 * 4.0 + 2.0) / (3 * 2 + 4) and st['mean'][2] == (3 * 1.0 + 9.0) / (3 * 1 + 3)
    st = p.stack(select=np.array([False, True, True]))
    assert st['mean'][0] == 0.5 and st['mean'][2] == 19.0 / 8
    scalar_only = HR.ShellProfiles(np.arange(4.0), npix, s)
    assert scalar_only.mean_t is None and set(scalar_only.stack()) == {'mean'}
