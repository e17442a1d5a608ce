"""CPU checks of the spherical-harmonic transforms: the numpy restatement (sht_oracle.py) against scipy and mpmath, healpy's alm
index arithmetic, and the argument rules of baryonification_amd.utils.sphtfunc (all raised before any device call)."""
import numpy as np
import pytest

import sht_oracle as O
from baryonification_amd import _lib, engine
from baryonification_amd import utils as U
from baryonification_amd.utils import sphtfunc as S


def test_oracle_lambda_matches_scipy():
    from scipy.special import sph_harm_y
    z = np.array([-0.97, -0.5, -0.1, 0.0, 0.3, 0.77, 0.999])
    th = np.arccos(z)
    for m in (0, 1, 2, 7, 50, 120, 200):
        lam = O.lambda_column(m, 200, z)
        for l in range(m, 201):
            ref = sph_harm_y(l, m, th, 0.0).real
            assert np.abs(lam[l - m] - ref).max() <= 1e-12, (l, m)


def _mp_lambda(l, m, x):
    """lambda_lm(x) = Y_lm(theta, 0) in 60-digit arithmetic (mpmath's spherharm includes the Condon-Shortley phase)"""
    import mpmath as mp
    mp.mp.dps = 60
    return mp.spherharm(l, m, mp.acos(mp.mpf(x)), 0).real


@pytest.mark.parametrize('m,theta_deg', [(1100, 30.0), (2000, 30.0), (2000, 45.0), (500, 11.2)])
def test_oracle_lambda_matches_mpmath_in_the_underflow_regime(m, theta_deg):
    """NSIDE 1024 rings where sin^m(theta) is far below the smallest double (1e-331 at m = 1100, theta = 30 deg; 1e-602 at
    m = 2000), l up to 3071: where lambda_lm has grown back above 1e-70 it matches mpmath to 1e-10 relative; below 1e-80 the
    oracle gives 0.  (2000, 30 deg) stays below 1e-80 up to l = 3071; the others come back to O(1)."""
    nside, lmax = 1024, 3071
    z = O.rings(nside)[3]
    r = int(np.argmin(np.abs(np.arccos(z) - np.radians(theta_deg))))
    zr = z[r]
    assert m * np.log10(np.sqrt((1 - zr) * (1 + zr))) < -300                  # lambda_mm underflows fp64
    lam = O.lambda_column(m, lmax, np.array([zr]))[:, 0]
    checked = 0
    for l in sorted(set(np.linspace(m, lmax, 24).astype(int)) | {lmax}):
        ref = float(_mp_lambda(l, m, zr))
        if abs(ref) >= 1e-70:
            assert abs(lam[l - m] - ref) <= 1e-10 * abs(ref), (l, m, lam[l - m], ref)
            checked += 1
        elif abs(ref) < 1e-80:
            assert lam[l - m] == 0.0 or abs(lam[l - m]) < 1e-76
    assert checked >= (0 if (m, theta_deg) == (2000, 30.0) else 5)


def test_oracle_map2alm_recovers_band_limited_alm():
    nside, lmax = 16, 32
    rng = np.random.default_rng(1)
    alm = np.zeros(O.alm_size(lmax, lmax), dtype=np.complex128)
    for l, m in [(0, 0), (1, 1), (3, 2), (5, 0), (8, 4), (8, 8)]:
        alm[O.alm_index(lmax, l, m)] = rng.normal() + (1j * rng.normal() if m else 0)
    mp = O.alm2map(alm, nside, lmax, lmax)
    err = [np.abs(O.map2alm(mp, nside, lmax, lmax, it) - alm).max() for it in (0, 3)]
    assert err[1] < 1e-5 * np.abs(alm).max() and err[1] < 0.01 * err[0], err


def test_alm_index_arithmetic():
    for lmax in (0, 1, 5, 47):
        for mmax in range(lmax + 1):
            n = S.getsize(lmax, mmax)
            assert n == engine.sht_alm_size(lmax, mmax) == O.alm_size(lmax, mmax)
            idx = [S.getidx(lmax, l, m) for m in range(mmax + 1) for l in range(m, lmax + 1)]
            assert idx == list(range(n))
        assert S.getlmax(S.getsize(lmax)) == lmax
    assert S.getlmax(S.getsize(20, 7), 7) == 20
    assert S.getlmax(7) == -1


def test_argument_errors():
    nside = 4
    m = np.zeros(12 * nside * nside)
    for kw in ({'use_weights': True}, {'use_pixel_weights': True}, {'datapath': '/x'}, {'gal_cut': 10}):
        name = list(kw)[0]
        with pytest.raises(NotImplementedError, match=name):
            U.map2alm(m, **kw)
        with pytest.raises(NotImplementedError, match=name):
            U.anafast(m, **kw)
    with pytest.raises(NotImplementedError, match='polarisation'):
        U.map2alm(np.zeros((3, m.size)))
    with pytest.raises(ValueError, match='mmax'):
        U.map2alm(m, lmax=5, mmax=6)
    with pytest.raises(ValueError):
        U.map2alm(np.zeros(13))
    with pytest.raises(ValueError):
        U.map2alm(np.zeros(m.size, dtype=np.int64))
    with pytest.raises(ValueError):
        U.map2alm(np.zeros(m.size, dtype=np.complex128))
    with pytest.raises(ValueError, match='2048'):
        U.map2alm(np.broadcast_to(np.float32(0), (12 * 4096 * 4096,)))
    alm = np.zeros(S.getsize(10), dtype=np.complex128)
    for kw in ({'pixwin': True}, {'fwhm': 0.1}, {'sigma': 0.01}):
        with pytest.raises(NotImplementedError, match=list(kw)[0]):
            U.alm2map(alm, nside, **kw)
    with pytest.raises(ValueError, match='integer lmax'):
        U.alm2map(np.zeros(7, dtype=np.complex128), nside)
    with pytest.raises(ValueError, match='integer lmax'):
        U.alm2cl(np.zeros(7, dtype=np.complex128))
    with pytest.raises(ValueError):
        U.alm2map(alm, nside, lmax=10, mmax=11)
    with pytest.raises(ValueError):
        U.alm2map(alm, nside, lmax=9)
    with pytest.raises(NotImplementedError, match='polarisation'):
        U.alm2map(np.zeros((3, alm.size), dtype=np.complex128), nside)


def test_c_entries_refuse_bad_arguments_before_any_device_call():
    L = _lib.load()
    assert L.bfgx_sht_work_doubles(0, 10, 10) == -1
    assert L.bfgx_sht_work_doubles(4096, 10, 10) == -1 and b'2048' in L.bfgx_last_error()
    assert L.bfgx_sht_work_doubles(4, 10, 11) == -1
    assert L.bfgx_sht_work_doubles(4, 11, 11) > 0
    assert L.bfgx_sht_map2alm_device(0, None, 4, 11, 11, 0, None, None, None) == _lib.ERR_INVALID
    assert b'NULL' in L.bfgx_last_error()
    assert L.bfgx_sht_alm2cl(0, 5, 6, 5, None, None, None) == _lib.ERR_INVALID
    assert L.bfgx_sht_anafast(0, 4, 11, 11, -1, None, None, None, None, None) == _lib.ERR_INVALID


def test_transforms_fail_loudly_without_gpu():
    if _lib.load().bfgx_device_count() > 0:
        pytest.skip("GPU present")
    m = np.zeros(12 * 4 * 4)
    with pytest.raises(_lib.BfgxError, match="no HIP device"):
        U.anafast(m)
    with pytest.raises(_lib.BfgxError, match="no HIP device"):
        engine.ShtPlan(4, 11, 11)
    with pytest.raises(_lib.BfgxError, match="no HIP device"):
        engine.sht_map2alm_host(m, 4, 11, 11, 0)
