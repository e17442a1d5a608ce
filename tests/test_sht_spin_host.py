"""CPU checks of the spin-weighted transforms: the numpy restatement (sht_spin_oracle.py) against the edth definition of sY_lm
(sympy), against Wigner d in 60-digit arithmetic (mpmath) where the start values underflow fp64, and against edth^s of a
band-limited scalar field at HEALPix pixel centres; the argument rules of map2alm_spin / alm2map_spin and of the C entries (all
raised before any device call)."""
import functools

import numpy as np
import pytest

import sht_oracle as O
import sht_spin_oracle as SO
from baryonification_amd import _lib, engine
from baryonification_amd import utils as U


@functools.lru_cache(maxsize=None)
def _edth_Ylm(l, m, s, module='numpy'):
    """edth^s Y_lm(theta, phi) as a function (edth eta = -(sin theta)^k (d_theta + i / sin theta d_phi)[(sin theta)^-k eta] for
    spin k): 'numpy' (called on long double arrays) or 'mpmath' (scalars)"""
    import sympy as sp
    th, ph = sp.symbols('theta phi', real=True)
    e = sp.Ynm(l, m, th, ph).expand(func=True)
    for k in range(s):
        g = sp.sin(th) ** (-k) * e
        e = -sp.sin(th) ** k * (sp.diff(g, th) + sp.I / sp.sin(th) * sp.diff(g, ph))
    return sp.lambdify((th, ph), e, module)


def _factorial_ratio(l, s):
    """(l + s)! / (l - s)!"""
    return float(np.prod(np.arange(l - s + 1, l + s + 1, dtype=np.float64)))


@pytest.mark.parametrize('s', [1, 2, 3])
def test_oracle_columns_match_edth_definition(s):
    """sY_lm = sqrt((l - s)! / (l + s)!) edth^s Y_lm for l <= 8, every m, at several theta (both hemispheres, near the poles)"""
    import mpmath as mp
    mp.mp.dps = 30                                                 # (the expressions cancel near the poles)
    theta = np.array([0.05, 0.4, 1.0, 1.5707963, 2.2, 3.0])
    for l in range(s, 9):
        for m in range(-l, l + 1):
            f = _edth_Ylm(l, m, s, 'mpmath')
            ref = np.array([complex(f(mp.mpf(float(t)), 0)) for t in theta]) / np.sqrt(_factorial_ratio(l, s))
            assert np.abs(ref.imag).max() <= 1e-12
            got = SO.sY(l, m, s, theta)
            assert np.abs(got - ref.real).max() <= 1e-12, (s, l, m, np.abs(got - ref.real).max())


def _mp_swigner(l, m, s, x):
    """(lam+, lam-) = (sY_lm, (-1)^m sY_{l,-m}) at theta = acos(x), 60 digits: sY_lm' = (-1)^s sqrt((2l + 1) / (4 pi)) d^l_{m',-s}
    for any m' (Wigner d in the convention of its Jacobi-polynomial formula, d from mpmath.jacobi; the sign is the one that makes
    test_mp_wigner_matches_oracle_at_low_l and test_oracle_columns_match_edth_definition agree)"""
    import mpmath as mp
    mp.mp.dps = 60
    th = mp.acos(mp.mpf(x))

    def d(j, mp_, m_):                                             # Wigner d^j_{mp_, m_}(th)
        k = min(j + m_, j - m_, j + mp_, j - mp_)
        if k == j + m_:
            a, lam = mp_ - m_, mp_ - m_
        elif k == j - m_:
            a, lam = m_ - mp_, 0
        elif k == j + mp_:
            a, lam = m_ - mp_, 0
        else:
            a, lam = mp_ - m_, mp_ - m_
        b = 2 * j - 2 * k - a
        return ((-1) ** lam * mp.sqrt(mp.binomial(2 * j - k, k + a)) / mp.sqrt(mp.binomial(k + b, b))
                * mp.sin(th / 2) ** a * mp.cos(th / 2) ** b * mp.jacobi(k, a, b, mp.cos(th)))

    n = mp.sqrt((2 * l + 1) / (4 * mp.pi))
    return (-1) ** s * n * d(l, m, -s), (-1) ** (m + s) * n * d(l, -m, -s)


def test_mp_wigner_matches_oracle_at_low_l():
    for s in (1, 2, 3):
        for l, m in [(3, 0), (3, 2), (5, 5), (7, 1)]:
            if l < s:
                continue
            for x in (-0.6, 0.1, 0.9):
                p, q = SO.spin_columns(m, s, l, np.array([x]))
                rp, rq = _mp_swigner(l, m, s, x)
                assert abs(p[l - m, 0] - float(rp)) <= 1e-13 and abs(q[l - m, 0] - float(rq)) <= 1e-13, (s, l, m, x)


@pytest.mark.parametrize('m,theta_deg', [(1100, 30.0), (2000, 30.0), (2000, 45.0), (500, 11.2)])
def test_oracle_spin_columns_match_mpmath_in_the_underflow_regime(m, theta_deg):
    """NSIDE 1024 rings where the start values cos^a(theta/2) sin^b(theta/2) are far below the smallest double, l up to 3071, spin
    2: where a column has grown back above 1e-70 it matches 60-digit Wigner d to 1e-10 relative; below 1e-80 the oracle gives 0"""
    nside, lmax, s = 1024, 3071, 2
    z = O.rings(nside)[3]
    r = int(np.argmin(np.abs(np.arccos(z) - np.radians(theta_deg))))
    zr = z[r]
    assert (m + s) * np.log10(np.sqrt((1 - zr) / 2)) < -300                   # the start value underflows fp64
    lp, lm = SO.spin_columns(m, s, lmax, np.array([zr]), O.sin2(nside)[r:r + 1])
    checked = 0
    for l in sorted(set(np.linspace(m, lmax, 24).astype(int)) | {lmax}):
        refs = _mp_swigner(l, m, s, zr)
        for got, ref in ((lp[l - m, 0], float(refs[0])), (lm[l - m, 0], float(refs[1]))):
            if abs(ref) >= 1e-70:
                assert abs(got - ref) <= 1e-10 * abs(ref), (l, m, got, ref)
                checked += 1
            elif abs(ref) < 1e-80:
                assert got == 0.0 or abs(got) < 1e-76
    assert checked >= (0 if (m, theta_deg) == (2000, 30.0) else 10)


@pytest.mark.parametrize('s', [1, 2, 3])
def test_oracle_synthesis_is_edth_of_a_scalar_field(s):
    """the whole convention, sign and phi dependence included: for a band-limited real scalar psi (l <= 8), edth^s psi at the
    NSIDE 8 pixel centres equals alm2map_spin([G, 0], 8, s, 8) with G_lm = -sqrt((l + s)! / (l - s)!) psi_lm (synthesis is exact)"""
    nside, lmax = 8, 8
    z = O.rings(nside)[3]
    ring, phi = O._pixel_rings(nside)
    theta = np.arccos(z)[ring].astype(np.longdouble)
    phi = phi.astype(np.longdouble)
    rng = np.random.default_rng(s)
    G = np.zeros(O.alm_size(lmax, lmax), dtype=np.complex128)
    field = np.zeros(theta.size, dtype=np.clongdouble)
    for l in range(0, lmax + 1):
        for m in range(0, l + 1):
            psi = rng.normal() + (1j * rng.normal() if m else 0.0)
            if l < s:
                continue                                           # edth^s Y_lm = 0
            G[O.alm_index(lmax, l, m)] = -np.sqrt(_factorial_ratio(l, s)) * psi
            field += psi * _edth_Ylm(l, m, s)(theta, phi)
            if m:
                field += (-1) ** m * np.conj(psi) * _edth_Ylm(l, -m, s)(theta, phi)
    got = SO.alm2map_spin(np.array([G, np.zeros_like(G)]), nside, s, lmax, lmax)
    scale = np.abs(field).max()
    assert np.abs(got[0] - field.real.astype(np.float64)).max() <= 1e-12 * scale
    assert np.abs(got[1] - field.imag.astype(np.float64)).max() <= 1e-12 * scale


def test_spin_functions_are_exported():
    assert U.map2alm_spin is U.sphtfunc.map2alm_spin and U.alm2map_spin is U.sphtfunc.alm2map_spin
    assert {'map2alm_spin', 'alm2map_spin'} <= set(U.sphtfunc.__all__)


def test_spin_argument_errors():
    nside = 4
    npix = 12 * nside * nside
    maps = np.zeros((2, npix))
    with pytest.raises(ValueError, match='map2alm'):
        U.map2alm_spin(maps, 0)
    with pytest.raises(ValueError, match='spin'):
        U.map2alm_spin(maps, -1)
    with pytest.raises(ValueError, match='spin'):
        U.map2alm_spin(maps, 6, lmax=5)
    with pytest.raises(ValueError, match='2 maps'):
        U.map2alm_spin(np.zeros((3, npix)), 2)
    with pytest.raises(ValueError, match='2 maps'):
        U.map2alm_spin([np.zeros(npix)], 2)
    with pytest.raises(ValueError, match='different sizes'):
        U.map2alm_spin([np.zeros(npix), np.zeros(12)], 2)
    with pytest.raises(ValueError, match='mmax'):
        U.map2alm_spin(maps, 2, lmax=5, mmax=6)
    with pytest.raises(ValueError, match='2048'):
        big = np.broadcast_to(np.float32(0), (12 * 4096 * 4096,))
        U.map2alm_spin([big, big], 2)
    alms = np.zeros((2, U.sphtfunc.getsize(10)), dtype=np.complex128)
    with pytest.raises(ValueError, match='map2alm'):
        U.alm2map_spin(alms, nside, 0, 10)
    with pytest.raises(ValueError, match='spin'):
        U.alm2map_spin(alms, nside, 11, 10)
    with pytest.raises(ValueError, match='2 sets'):
        U.alm2map_spin(np.zeros((3, alms.shape[1]), dtype=np.complex128), nside, 2, 10)
    with pytest.raises(ValueError, match='different sizes'):
        U.alm2map_spin([alms[0], alms[1][:-1]], nside, 2, 10)
    with pytest.raises(ValueError, match='integer lmax'):
        U.alm2map_spin(np.zeros((2, 7), dtype=np.complex128), nside, 2, None)
    with pytest.raises(ValueError, match='needs'):
        U.alm2map_spin(alms, nside, 2, 9)
    with pytest.raises(ValueError, match='2048'):
        U.alm2map_spin(alms, 4096, 2, 10)


def test_spin_c_entries_refuse_bad_arguments_before_any_device_call():
    L = _lib.load()
    assert L.bfgx_sht_spin_work_doubles(0, 10, 10) == -1
    assert L.bfgx_sht_spin_work_doubles(4096, 10, 10) == -1 and b'2048' in L.bfgx_last_error()
    assert L.bfgx_sht_spin_work_doubles(4, 10, 11) == -1
    assert L.bfgx_sht_spin_work_doubles(4, 11, 11) == 2 * 12 * 15
    assert engine.sht_spin_work_doubles(4, 11, 11) == 2 * 12 * 15
    x = np.zeros(64)
    p = x.ctypes.data
    for fn in (L.bfgx_sht_map2alm_spin_device, L.bfgx_sht_alm2map_spin_device):
        assert fn(0, None, 4, 11, 11, 2, None, p, p, p) == _lib.ERR_INVALID and b'NULL' in L.bfgx_last_error()
        assert fn(0, None, 4, 11, 11, 2, p, p, p, None) == _lib.ERR_INVALID and b'NULL' in L.bfgx_last_error()
        assert fn(0, None, 4, 11, 11, 2, p, p, None, p) == _lib.ERR_INVALID and b'NULL' in L.bfgx_last_error()
        assert fn(0, None, 4, 11, 11, 0, p, p, p, p) == _lib.ERR_INVALID and b'spin' in L.bfgx_last_error()
        assert fn(0, None, 4, 11, 11, 12, p, p, p, p) == _lib.ERR_INVALID and b'spin' in L.bfgx_last_error()
        assert fn(0, None, 4, 11, 12, 2, p, p, p, p) == _lib.ERR_INVALID and b'mmax' in L.bfgx_last_error()
        assert fn(0, None, 4096, 11, 11, 2, p, p, p, p) == _lib.ERR_INVALID and b'2048' in L.bfgx_last_error()
        assert fn(0, None, 4, 11, 11, 2, p, p, p, p + 8) == _lib.ERR_INVALID and b'aligned' in L.bfgx_last_error()
    for fn in (L.bfgx_sht_map2alm_spin, L.bfgx_sht_alm2map_spin):
        assert fn(0, 4, 11, 11, 2, None, p) == _lib.ERR_INVALID and b'NULL' in L.bfgx_last_error()
        assert fn(0, 4, 11, 11, 0, p, p) == _lib.ERR_INVALID and b'spin' in L.bfgx_last_error()
        assert fn(0, 4, 11, 11, 12, p, p) == _lib.ERR_INVALID and b'spin' in L.bfgx_last_error()
        assert fn(0, 0, 11, 11, 2, p, p) == _lib.ERR_INVALID


def test_spin_transforms_fail_loudly_without_gpu():
    if _lib.load().bfgx_device_count() > 0:
        pytest.skip("GPU present")
    nside = 4
    maps = np.zeros((2, 12 * nside * nside))
    with pytest.raises(_lib.BfgxError, match="no HIP device"):
        U.map2alm_spin(maps, 2)
    with pytest.raises(_lib.BfgxError, match="no HIP device"):
        U.alm2map_spin(np.zeros((2, U.sphtfunc.getsize(11)), dtype=np.complex128), nside, 2, 11)
    with pytest.raises(_lib.BfgxError, match="no HIP device"):
        engine.sht_map2alm_spin_host(maps, nside, 11, 11, 2)
    with pytest.raises(_lib.BfgxError, match="no HIP device"):
        engine.sht_alm2map_spin_host(np.zeros((2, U.sphtfunc.getsize(11)), dtype=np.complex128), nside, 11, 11, 2)
