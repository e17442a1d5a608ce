"""What the map statistics promise without a GPU: the oracle's neighbour rule and peak count reproduce known facts, the harmonic
windows are exact host numpy, and every new Python function and C entry refuses bad arguments before any device call."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mapstats_oracle as M
from baryonification_amd import _lib, utils as U
from baryonification_amd.utils import mapstats, sphtfunc

ARCMIN = np.pi / 180 / 60


# ------------------------------------------------------------------------------------------------------------- the oracle
def test_oracle_neighbours_of_healpy_docstring():
    assert M.neighbours(1, 4).tolist() == [11, 7, 3, -1, 0, 5, 8, -1]


@pytest.mark.parametrize('nside', [1, 2, 4, 8, 16])
def test_oracle_neighbour_relation(nside):
    npix = 12 * nside * nside
    nb = M.neighbours(nside, np.arange(npix))
    assert nb.shape == (8, npix) and (nb == -1).sum() == 24 and nb.min() == -1 and nb.max() < npix
    sets = []
    for p in range(npix):
        have = nb[:, p][nb[:, p] >= 0]
        assert p not in have and np.unique(have).size == have.size
        sets.append(set(have.tolist()))
    for p in range(npix):
        for q in sets[p]:
            assert p in sets[q]
    if nside > 1:
        assert np.array_equal(M.neighbours(nside, M.H.ring2nest(nside, np.arange(npix)), nest=True),
                              np.where(nb >= 0, M.H.ring2nest(nside, np.where(nb >= 0, nb, 0)), -1))


def test_oracle_white_noise_maxima():
    m = np.random.default_rng(1).normal(size=12288)
    counts, flags = M.peaks(m, [-1e300, 1e300])
    assert counts['maxima'].sum() == 1390 == (flags == 1).sum()
    assert abs(1390 / m.size - 1 / 9) < 0.01


def test_oracle_moments_of_a_known_sample():
    x = np.array([1.0, 2.0, 3.0, 6.0, np.nan, M.UNSEEN])
    n, mean, central, scale = M.moments(x)
    assert n == 4 and mean[0] == 3.0
    assert central[(2,)] == 3.5 and central[(3,)] == 4.5 and central[(4,)] == (16 + 1 + 0 + 81) / 4
    n, mean, central, _ = M.moments([x, 2 * x], order=3, mask=[1, 1, 1, 0, 1, 1])
    assert n == 3 and mean.tolist() == [2.0, 4.0] and central[(1, 1)] == 2 * central[(2, 0)] and len(central) == 7


# ---------------------------------------------------------------------------------------------------------------- windows
def test_gauss_beam_formula():
    for fwhm, lmax in ((0.0, 10), (np.radians(1.0), 512), (20 * ARCMIN, 95)):
        sigma = fwhm / np.sqrt(8 * np.log(2))
        l = np.arange(lmax + 1)
        # the exponent reaches -7.2 here; a few roundings of it in another order move exp by |x| 4 eps + eps < 1e-14 relative
        assert np.allclose(U.gauss_beam(fwhm, lmax), np.exp(-l * (l + 1) * sigma ** 2 / 2), rtol=1e-14, atol=0)
    assert U.gauss_beam(0.01).shape == (513,) and U.gauss_beam(0.0, 7).tolist() == [1.0] * 8
    with pytest.raises(NotImplementedError):
        U.gauss_beam(0.01, 10, pol=True)
    with pytest.raises(ValueError):
        U.gauss_beam(0.01, -1)


@pytest.mark.parametrize('radius', [1 * ARCMIN, 10 * ARCMIN, np.radians(2.0)])
def test_tophat_beam_against_mpmath(radius):
    w = U.tophat_beam(radius, 300)
    ref = M.tophat_window(radius, 300)
    assert w.shape == (301,) and w[0] == 1.0
    err = np.abs(w - ref).max()
    assert err <= 1e-13, err


def test_tophat_beam_limits():
    assert U.tophat_beam(0.0, 300).tolist() == [1.0] * 301
    assert U.tophat_beam(0.3, 0).tolist() == [1.0]
    assert abs(U.tophat_beam(np.pi / 2, 2)[1] - 0.5) < 1e-15            # (1 + 0) P'_1 / 2
    for bad in (-0.1, 3.2, np.nan):
        with pytest.raises(ValueError, match='radius'):
            U.tophat_beam(bad, 10)
    with pytest.raises(ValueError, match='lmax'):
        U.tophat_beam(0.1, -1)


def test_moment_exponents_order():
    assert mapstats.moment_exponents(1) == [(2,), (3,), (4,)]
    assert mapstats.moment_exponents(2, 3) == [(2, 0), (1, 1), (0, 2), (3, 0), (2, 1), (1, 2), (0, 3)]
    e3 = mapstats.moment_exponents(3)
    assert len(e3) == 31 and e3[:6] == [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2)]
    L = _lib.load()
    for K in (1, 2, 3):
        for order in (2, 3, 4):
            ex = mapstats.moment_exponents(K, order)
            assert sorted(ex) == sorted(M.exponents(K, order)) and L.bfgx_mapstats_moment_terms(K, order) == len(ex)
    assert L.bfgx_mapstats_moment_terms(4, 4) == -1 and L.bfgx_mapstats_moment_terms(1, 5) == -1 and L.bfgx_mapstats_moment_terms(0, 1) == -1


# ------------------------------------------------------------------------------------------- argument rules, Python level
def test_python_argument_rules():
    m = np.zeros(48)
    with pytest.raises(NotImplementedError, match='phi'):
        U.get_all_neighbours(4, 0.3, 0.2)
    for nside in (0, 8193, 1.5):
        with pytest.raises(ValueError, match=r'\[1, 8192\]|integer'):
            U.get_all_neighbours(nside, 0)
    with pytest.raises(ValueError, match='power of two'):
        U.get_all_neighbours(3, 0, nest=True)
    with pytest.raises(ValueError, match=r'\[0, 192\)'):
        U.get_all_neighbours(4, np.array([0, 192]))
    with pytest.raises(ValueError, match=r'\[0, 192\)'):
        U.get_all_neighbours(4, -1)
    with pytest.raises(ValueError, match='integer'):
        U.get_all_neighbours(4, np.array([0.5]))
    with pytest.raises(NotImplementedError, match='nest'):
        U.smoothing(m, fwhm=0.1, nest=True)
    for kw in ({'use_weights': True}, {'use_pixel_weights': True}, {'datapath': '/x'}):
        with pytest.raises(NotImplementedError):
            U.smoothing(m, fwhm=0.1, **kw)
    with pytest.raises(NotImplementedError, match='more than one map'):
        U.smoothing(np.zeros((3, 48)), fwhm=0.1)
    with pytest.raises(ValueError, match='2048'):
        U.smoothing(np.broadcast_to(np.float32(0), (12 * 4096 ** 2,)), fwhm=0.1)             # (a view: nothing that large is allocated)
    with pytest.raises(ValueError, match='iter'):
        U.smoothing(m, fwhm=0.1, iter=-1)
    with pytest.raises(ValueError, match='12\\*nside'):
        U.smoothing(np.zeros(50), fwhm=0.1)
    with pytest.raises(ValueError, match='1-D'):
        U.smoothing(m, beam_window=np.ones((2, 3)))
    a = np.zeros(sphtfunc.getsize(5, 3), dtype=np.complex128)
    with pytest.raises(ValueError, match='integer lmax'):
        U.almxfl(np.zeros(7, dtype=np.complex128), np.ones(3))
    with pytest.raises(ValueError, match='real'):
        U.almxfl(a, np.ones(3, dtype=np.complex128), mmax=3)
    with pytest.raises(ValueError, match='real'):
        U.almxfl(a, np.ones((2, 3)), mmax=3)
    with pytest.raises(ValueError, match='inplace'):
        U.almxfl(a.astype(np.complex64), np.ones(3), mmax=3, inplace=True)
    with pytest.raises(ValueError, match='inplace'):
        U.smoothalm(list(a), fwhm=0.1, mmax=3)
    for order in (1, 5, 2.5):
        with pytest.raises(ValueError, match='order'):
            U.map_moments(m, order=order)
    with pytest.raises(ValueError, match='1 to 3 maps'):
        U.map_moments(np.zeros((4, 48)))
    with pytest.raises(ValueError, match='1 to 3 maps'):
        U.map_moments([])
    with pytest.raises(ValueError, match='different sizes'):
        U.map_moments([m, np.zeros(12)])
    with pytest.raises(ValueError, match='mask'):
        U.map_moments(m, mask=np.ones(12))
    with pytest.raises(ValueError, match='real'):
        U.map_moments(m.astype(np.complex128))
    for bins in ([0.0, 1.0, 0.5], [0.0, 0.0, 1.0], [0.0, np.inf], [0.0, np.nan, 1.0]):
        with pytest.raises(ValueError, match='ascending'):
            U.peak_counts(m, bins)
    for bins in ([0.0], np.linspace(0, 1, 4098), np.zeros((2, 2))):
        with pytest.raises(ValueError, match='4096'):
            U.peak_counts(m, bins)
    with pytest.raises(ValueError, match='12\\*nside'):
        U.peak_counts(np.zeros(50), [0.0, 1.0])
    with pytest.raises(ValueError, match='power of two'):
        U.peak_counts(np.zeros(12 * 9), [0.0, 1.0], nest=True)
    with pytest.raises(ValueError, match='one map'):
        U.peak_counts(np.zeros((2, 48)), [0.0, 1.0])
    with pytest.raises(ValueError, match='mask'):
        U.peak_counts(m, [0.0, 1.0], mask=np.ones(3))
    with pytest.raises(ValueError, match='window'):
        U.shell_statistics(m, [0.1], window='boxcar')
    for scales in ([], [-0.1], [np.nan], [[0.1, 0.2]]):
        with pytest.raises(ValueError, match='scales'):
            U.shell_statistics(m, scales)
    with pytest.raises(ValueError, match='order'):
        U.shell_statistics(m, [0.1], order=7)
    with pytest.raises(ValueError, match='1 to 3 maps'):
        U.shell_statistics(np.zeros((4, 48)), [0.1])
    with pytest.raises(ValueError, match='ascending'):
        U.shell_statistics(m, [0.1], peak_bins=[1.0, 0.0])
    with pytest.raises(ValueError, match='lmax'):
        U.shell_statistics(m, [0.1], lmax=-2)
    with pytest.raises(ValueError, match='iter'):
        U.shell_statistics(m, [0.1], iter=-1)


# ------------------------------------------------------------------------------------------------ argument rules, C level
def test_cabi_refuses_before_device():
    L = _lib.load()
    z = np.zeros(64)
    ip = np.array([0, 5], dtype=np.int64)
    out = np.zeros(16, dtype=np.int64)
    p = lambda a: a.ctypes.data
    # neighbours
    assert L.bfgx_hpx_neighbours(0, 4, 0, 2, None, p(out)) == _lib.ERR_INVALID and b'NULL' in L.bfgx_last_error()
    assert L.bfgx_hpx_neighbours_device(0, None, 4, 0, 2, p(ip), None) == _lib.ERR_INVALID and b'NULL' in L.bfgx_last_error()
    assert L.bfgx_hpx_neighbours(0, 3, 1, 2, p(ip), p(out)) == _lib.ERR_INVALID and b'power of two' in L.bfgx_last_error()
    assert L.bfgx_hpx_neighbours_device(0, None, 16384, 0, 2, p(ip), p(out)) == _lib.ERR_INVALID and b'8192' in L.bfgx_last_error()
    assert L.bfgx_hpx_neighbours(0, 0, 0, 2, p(ip), p(out)) == _lib.ERR_INVALID
    assert L.bfgx_hpx_neighbours(0, 4, 0, -1, p(ip), p(out)) == _lib.ERR_INVALID and b'n must' in L.bfgx_last_error()
    bad = np.array([0, 192], dtype=np.int64)
    assert L.bfgx_hpx_neighbours(0, 4, 0, 2, p(bad), p(out)) == _lib.ERR_INVALID and b'[0, 192)' in L.bfgx_last_error()
    # almxfl
    assert L.bfgx_sht_almxfl(0, 5, 3, 4, None, p(z), p(z)) == _lib.ERR_INVALID and b'NULL' in L.bfgx_last_error()
    assert L.bfgx_sht_almxfl_device(0, None, 5, 3, 4, p(z), None, p(z)) == _lib.ERR_INVALID
    assert L.bfgx_sht_almxfl_device(0, None, 5, 3, 4, p(z), p(z), None) == _lib.ERR_INVALID
    assert L.bfgx_sht_almxfl(0, 3, 5, 4, p(z), p(z), p(z)) == _lib.ERR_INVALID and b'mmax' in L.bfgx_last_error()
    assert L.bfgx_sht_almxfl(0, -1, 0, 4, p(z), p(z), p(z)) == _lib.ERR_INVALID
    assert L.bfgx_sht_almxfl(0, 40000, 0, 4, p(z), p(z), p(z)) == _lib.ERR_INVALID
    assert L.bfgx_sht_almxfl_device(0, None, 5, 3, -1, p(z), p(z), p(z)) == _lib.ERR_INVALID and b'nfl' in L.bfgx_last_error()
    # moments
    n = np.zeros(1, dtype=np.int64)
    assert L.bfgx_mapstats_moments_device(0, None, 48, 1, 4, None, None, p(n), p(z), p(z)) == _lib.ERR_INVALID and b'NULL' in L.bfgx_last_error()
    assert L.bfgx_mapstats_moments_device(0, None, 48, 1, 4, p(z), None, None, p(z), p(z)) == _lib.ERR_INVALID
    assert L.bfgx_mapstats_moments_device(0, None, 48, 1, 4, p(z), None, p(n), None, p(z)) == _lib.ERR_INVALID
    assert L.bfgx_mapstats_moments_device(0, None, 48, 1, 4, p(z), None, p(n), p(z), None) == _lib.ERR_INVALID
    for K in (0, 4):
        assert L.bfgx_mapstats_moments_device(0, None, 48, K, 4, p(z), None, p(n), p(z), p(z)) == _lib.ERR_INVALID
        assert b'nmaps must be in [1, 3]' in L.bfgx_last_error()
    for order in (1, 5):
        assert L.bfgx_mapstats_moments_device(0, None, 48, 1, order, p(z), None, p(n), p(z), p(z)) == _lib.ERR_INVALID
        assert b'order must be in [2, 4]' in L.bfgx_last_error()
    for npix in (0, -5, 12 * 8192 ** 2 + 1):
        assert L.bfgx_mapstats_moments_device(0, None, npix, 1, 4, p(z), None, p(n), p(z), p(z)) == _lib.ERR_INVALID
        assert b'npix' in L.bfgx_last_error()
    # peaks
    assert L.bfgx_mapstats_peaks_device(0, None, 2, 0, None, None, 4, p(z), p(out), None) == _lib.ERR_INVALID and b'NULL' in L.bfgx_last_error()
    assert L.bfgx_mapstats_peaks_device(0, None, 2, 0, p(z), None, 4, None, p(out), None) == _lib.ERR_INVALID
    assert L.bfgx_mapstats_peaks_device(0, None, 2, 0, p(z), None, 4, p(z), None, None) == _lib.ERR_INVALID
    for nside, nest in ((0, 0), (8193, 0), (3, 1)):
        assert L.bfgx_mapstats_peaks_device(0, None, nside, nest, p(z), None, 4, p(z), p(out), None) == _lib.ERR_INVALID
        assert b'nside' in L.bfgx_last_error()
    for nb in (0, 4097):
        assert L.bfgx_mapstats_peaks_device(0, None, 2, 0, p(z), None, nb, p(z), p(out), None) == _lib.ERR_INVALID
        assert b'nb must be in [1, 4096]' in L.bfgx_last_error()
    assert _lib.MAPSTATS_WORK_DOUBLES == 32768
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'bfgx.h')).read()
    assert '#define BFGX_MAPSTATS_WORK_DOUBLES 32768' in hdr


def test_compute_fails_loudly_without_gpu():
    if _lib.load().bfgx_device_count() > 0:
        pytest.skip("GPU present")
    m = np.random.default_rng(0).random(48)
    a = np.zeros(sphtfunc.getsize(5, 5), dtype=np.complex128)
    for call in (lambda: U.get_all_neighbours(2, 3), lambda: U.almxfl(a, np.ones(6)), lambda: U.smoothing(m, fwhm=0.1),
                 lambda: U.map_moments(m), lambda: U.peak_counts(m, [0.0, 1.0]), lambda: U.shell_statistics(m, [0.0, 0.1])):
        with pytest.raises(_lib.BfgxError, match="no HIP device"):
            call()


def test_importing_opens_no_device():
    """importing the package and its utils neither loads libbfgx nor torch: no device can have been opened"""
    code = ("import sys; import baryonification_amd.utils as U; from baryonification_amd import _lib; "
            "assert U.shell_statistics and U.get_all_neighbours and U.smoothing; "
            "assert _lib._lib is None and 'torch' not in sys.modules")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-c', code], cwd=repo, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
