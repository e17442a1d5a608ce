"""What the derivatives and Minkowski functionals promise without a GPU: the numpy oracle (minkowski_oracle.py) reproduces closed
forms, which pins the conventions independently of the derivation; minkowski_gaussian is exact host numpy; and every new Python
function and C entry refuses bad arguments before any device call."""
import numpy as np
import pytest

import minkowski_oracle as K
import sht_oracle as O
from baryonification_amd import _lib, utils as U
from baryonification_amd.utils import mapstats, sphtfunc


# ------------------------------------------------------------------------------------------------ (a) oracle derivatives
@pytest.mark.parametrize('nside', [4, 8])
def test_oracle_derivatives_match_closed_forms(nside):
    lmax = 6
    z, s, phi = K.pixel_angles(nside)
    alm = np.zeros(O.alm_size(lmax, lmax), dtype=np.complex128)
    alm[O.alm_index(lmax, 1, 0)] = 1.0                       # u = sqrt(3 / 4 pi) cos(theta)
    c = np.sqrt(3 / (4 * np.pi))
    ref = np.stack([c * z, -c * s, 0 * z, -c * z, 0 * z, -c * z])
    got = K.derivatives(alm, nside, lmax, lmax)
    assert np.abs(got - ref).max() <= 1e-13, np.abs(got - ref).max(axis=1)
    alm[:] = 0
    alm[O.alm_index(lmax, 2, 2)] = 1.0                       # u = c sin^2(theta) cos(2 phi), c = sqrt(15 / 2 pi) / 2
    c = 0.5 * np.sqrt(15 / (2 * np.pi))
    c2, s2 = np.cos(2 * phi), np.sin(2 * phi)
    ut = 2 * c * s * z * c2
    ref = np.stack([c * s * s * c2, ut, -2 * c * s * s2, 2 * c * (z * z - s * s) * c2, -2 * c * z * s2, -4 * c * c2 + z / s * ut])
    got = K.derivatives(alm, nside, lmax, lmax)
    assert np.abs(got - ref).max() <= 1e-13, np.abs(got - ref).max(axis=1)
    sp = K.derivatives(alm, nside, lmax, lmax, spin_form=True)
    assert np.abs(sp - K.to_spin_form(ref)).max() <= 1e-13
    # the Laplacian of Y_22 is -6 Y_22
    assert np.abs(sp[3] + 6 * ref[0]).max() <= 1e-13


# ------------------------------------------------------------------------------------------------ (b) oracle functionals
def test_oracle_minkowski_of_z():
    nside = 8
    edges, zr = K.belt_edges(nside)
    assert edges.size == 2 * nside and zr.size == 2 * nside - 1
    d = K.z_derivatives(nside)
    res = K.minkowski(d, edges)
    npix = 12 * nside * nside
    assert res['n'] == npix and (res['count'] == 4 * nside).all()
    assert np.abs(res['v1'] - np.sqrt(1 - zr * zr) / 8).max() <= 1e-13
    assert np.abs(res['v2'] - zr / (4 * np.pi)).max() <= 1e-13
    assert np.array_equal(res['v0'], np.array([(d[0] >= t).sum() for t in edges]) / npix)
    ncap = 2 * nside * (nside + 1)                            # the pixels of the rings 1 .. nside
    assert res['above'] == ncap == res['below'] and res['v0'][-1] == ncap / npix and res['v0'][0] == 1 - ncap / npix
    sp = K.minkowski(K.to_spin_form(d), edges, spin_form=True)
    assert np.array_equal(sp['sums'], res['sums']) and np.array_equal(sp['count'], res['count'])


def test_oracle_minkowski_good_pixels_and_edges():
    d = np.zeros((6, 12))
    d[0] = [0.0, 1.0, 2.0, 3.0, 0.5, 1.5, -1.0, 3.5, 1.0, 1.0, 1.0, 1.0]
    d[1] = 2.0
    d[0, 8], d[3, 9], d[5, 10] = K.M.UNSEEN, np.nan, np.inf
    res = K.minkowski(d, [0.0, 1.0, 3.0], mask=np.arange(12) != 11)
    # good: pixels 0 .. 7; 0.0 sits on edges[0] (bin 0), 1.0 on edges[1] (bin 1), 3.0 on edges[2] (above)
    assert res['n'] == 8 and res['count'].tolist() == [2, 3] and res['below'] == 1 and res['above'] == 2
    assert res['sums'][0].tolist() == [4.0, 6.0] and res['v0'].tolist() == [7 / 8, 5 / 8, 2 / 8]
    none = K.minkowski(d, [0.0, 1.0], mask=np.zeros(12))
    assert none['n'] == 0 and np.isnan(none['v0']).all() and np.isnan(none['v1']).all()


# ------------------------------------------------------------------------------------------------- (c) Gaussian fields
def test_minkowski_gaussian():
    cl = 1.0 / (1.0 + np.arange(40.0)) ** 2
    l = np.arange(40.0)
    s0 = np.sqrt(np.sum((2 * l + 1) * cl) / (4 * np.pi))
    tau = np.sum((2 * l + 1) * l * (l + 1) * cl) / (4 * np.pi) / (2 * s0 * s0)
    g = U.minkowski_gaussian(cl, 0.0)
    assert g['v0'] == 0.5 and g['v2'] == 0.0 and abs(g['v1'] - np.sqrt(tau) / 8) <= 1e-15 * np.sqrt(tau)
    assert abs(g['sigma0'] - s0) <= 1e-15 * s0
    t = np.linspace(0.1, 3.0, 9) * s0
    p, m = U.minkowski_gaussian(cl, t), U.minkowski_gaussian(cl, -t)
    assert p['v0'].shape == (9,) and np.abs(m['v0'] - (1 - p['v0'])).max() <= 1e-15
    assert np.array_equal(m['v2'], -p['v2']) and np.array_equal(m['v1'], p['v1']) and (p['v2'] > 0).all()
    nu = t / s0
    assert np.abs(p['v2'] - tau * (2 * np.pi) ** -1.5 * nu * np.exp(-nu * nu / 2)).max() <= 1e-15 * tau
    for bad in ([], [[1.0, 2.0]], [1.0, -1.0], [0.0, 0.0], [np.nan]):
        with pytest.raises(ValueError, match='cl'):
            U.minkowski_gaussian(bad, 0.0)


# ------------------------------------------------------------------------------------------------- (d) argument rules
def test_python_argument_rules():
    assert U.alm2map_der1 is sphtfunc.alm2map_der1 and U.alm2map_der2 is sphtfunc.alm2map_der2
    assert U.minkowski_functionals is mapstats.minkowski_functionals and U.minkowski_from_derivatives is mapstats.minkowski_from_derivatives
    a = np.zeros(sphtfunc.getsize(5, 3), dtype=np.complex128)
    for fn in (U.alm2map_der1, U.alm2map_der2):
        with pytest.raises(ValueError, match='integer lmax'):
            fn(np.zeros(7, dtype=np.complex128), 4)
        with pytest.raises(ValueError, match='needs'):
            fn(a, 4, lmax=5, mmax=5)
        with pytest.raises(ValueError, match='nside'):
            fn(a, 0, lmax=5, mmax=3)
        with pytest.raises(ValueError, match='2048'):
            fn(a, 4096, lmax=5, mmax=3)
        with pytest.raises(NotImplementedError, match='more than one set'):
            fn(np.zeros((3, a.size), dtype=np.complex128), 4, lmax=5, mmax=3)
        with pytest.raises(ValueError, match='1-D complex'):
            fn(np.zeros((2, 2, 2)), 4)
    d, m = np.zeros((6, 48)), np.zeros(48)
    for bad in (np.zeros(48), np.zeros((5, 48)), np.zeros((6, 0)), np.zeros((2, 6, 48))):
        with pytest.raises(ValueError, match='six maps'):
            U.minkowski_from_derivatives(bad, [0.0, 1.0])
    with pytest.raises(ValueError, match='real'):
        U.minkowski_from_derivatives(d.astype(np.complex128), [0.0, 1.0])
    with pytest.raises(ValueError, match='mask'):
        U.minkowski_from_derivatives(d, [0.0, 1.0], mask=np.ones(12))
    for call in (lambda b: U.minkowski_from_derivatives(d, b), lambda b: U.minkowski_functionals(m, b),
                 lambda b: U.shell_statistics(m, [0.1], mf_bins=b)):
        for bins in ([0.0, 1.0, 0.5], [0.0, 0.0, 1.0], [0.0, np.inf], [0.0, np.nan, 1.0]):
            with pytest.raises(ValueError, match='ascending'):
                call(bins)
        for bins in ([0.0], np.linspace(0, 1, 514), np.zeros((2, 2))):
            with pytest.raises(ValueError, match='512'):
                call(bins)
    with pytest.raises(ValueError, match='one map'):
        U.minkowski_functionals(np.zeros((2, 48)), [0.0, 1.0])
    with pytest.raises(ValueError, match='12\\*nside'):
        U.minkowski_functionals(np.zeros(50), [0.0, 1.0])
    with pytest.raises(ValueError, match='2048'):
        U.minkowski_functionals(np.broadcast_to(np.float32(0), (12 * 4096 ** 2,)), [0.0, 1.0])
    with pytest.raises(ValueError, match='iter'):
        U.minkowski_functionals(m, [0.0, 1.0], iter=-1)
    with pytest.raises(ValueError, match='lmax'):
        U.minkowski_functionals(m, [0.0, 1.0], lmax=-2)
    with pytest.raises(ValueError, match='mask'):
        U.minkowski_functionals(m, [0.0, 1.0], mask=np.ones(3))
    with pytest.raises(ValueError, match='1-D'):
        U.minkowski_functionals(m, [0.0, 1.0], beam_window=np.ones((2, 3)))


def test_cabi_refuses_before_device():
    L = _lib.load()
    z = np.zeros(6 * 48)
    cnt = np.zeros(16, dtype=np.int64)
    p = lambda a: a.ctypes.data
    ok = lambda: [0, None, 48, p(z), None, 4, p(z), p(cnt), p(z), p(z)]
    for k in (3, 6, 7, 8, 9):                                 # ders, edges, counts, sums, work
        args = ok()
        args[k] = None
        assert L.bfgx_mapstats_minkowski_device(*args) == _lib.ERR_INVALID and b'NULL' in L.bfgx_last_error()
    for nb in (0, -1, 513):
        args = ok()
        args[5] = nb
        assert L.bfgx_mapstats_minkowski_device(*args) == _lib.ERR_INVALID and b'nb must be in [1, 512]' in L.bfgx_last_error()
        assert L.bfgx_mapstats_minkowski_work_doubles(48, nb) == -1
    for npix in (0, -5, 12 * 8192 ** 2 + 1):
        args = ok()
        args[2] = npix
        assert L.bfgx_mapstats_minkowski_device(*args) == _lib.ERR_INVALID and b'npix' in L.bfgx_last_error()
        assert L.bfgx_mapstats_minkowski_work_doubles(npix, 4) == -1
    # one partial [2][nb] per workgroup of 256 pixels, at most 1024 workgroups
    assert L.bfgx_mapstats_minkowski_work_doubles(48, 4) == 8 and L.bfgx_mapstats_minkowski_work_doubles(257, 512) == 2 * 1024
    assert L.bfgx_mapstats_minkowski_work_doubles(12 * 2048 ** 2, 512) == 1024 * 1024
    assert L.bfgx_abi_version() == 4


def test_compute_fails_loudly_without_gpu():
    if _lib.load().bfgx_device_count() > 0:
        pytest.skip("GPU present")
    m = np.random.default_rng(0).random(48)
    a = np.zeros(sphtfunc.getsize(5, 5), dtype=np.complex128)
    for call in (lambda: U.alm2map_der1(a, 2), lambda: U.alm2map_der2(a, 2), lambda: U.minkowski_functionals(m, [0.0, 1.0]),
                 lambda: U.minkowski_from_derivatives(np.zeros((6, 48)), [0.0, 1.0]),
                 lambda: U.shell_statistics(m, [0.0], mf_bins=[0.0, 1.0])):
        with pytest.raises(_lib.BfgxError, match="no HIP device"):
            call()
