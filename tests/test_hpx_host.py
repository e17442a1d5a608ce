"""CPU checks of the HEALPix pixel functions: the numpy helper (hpx_oracle.py) against healpy's docstring answers and the
tessellation, and the argument rules of utils.pixelfunc / Runners.regrid_pixels_hpix, all raised before any device call."""
import subprocess
import sys

import numpy as np
import pytest

import hpx_oracle as H
from baryonification_amd import _lib
from baryonification_amd import utils as U
from baryonification_amd.Runners import regrid_pixels_hpix


def test_helper_reproduces_healpy_docstrings():
    assert H.ring2nest(2, np.arange(10)).tolist() == [3, 7, 11, 15, 2, 1, 6, 5, 10, 9]
    assert H.nest2ring(2, np.arange(10)).tolist() == [13, 5, 4, 0, 15, 7, 6, 1, 17, 9]
    assert int(H.ring2nest(16, 1504)) == 1130
    assert H.ring2nest([1, 2, 4, 8], 11).tolist() == [11, 13, 61, 253]
    assert H.nest2ring([1, 2, 4, 8], 11).tolist() == [11, 2, 12, 211]


@pytest.mark.parametrize('nside', [1, 2, 4, 16, 128])
def test_helper_orderings_are_inverse_and_nested(nside):
    p = np.arange(12 * nside * nside)
    r2n = H.ring2nest(nside, p)
    assert np.array_equal(np.sort(r2n), p) and np.array_equal(H.nest2ring(nside, r2n), p)
    # the 4 NEST children of a pixel surround its centre (independent RING geometry: oracle/refshim pix2vec)
    parent = np.stack(H.hp.pix2vec(nside, H.nest2ring(nside, p)), axis=1)
    kids = np.stack(H.hp.pix2vec(2 * nside, H.nest2ring(2 * nside, 4 * p[:, None] + np.arange(4))), axis=-1)
    mean = kids.mean(axis=1)
    mean /= np.linalg.norm(mean, axis=1)[:, None]
    assert np.abs(mean - parent).max() < 0.35 / nside


@pytest.mark.parametrize('r', [2, 4, 8])
def test_children_lie_on_ring_runs(r):
    """the kernels' child order: 2 r - 1 RING rows, each a run of consecutive ring pixels (up to the wrap at phi = 0)"""
    nside_out = 4
    nside_in = nside_out * r
    ch = H.children(nside_in, nside_out, np.arange(12 * nside_out ** 2))
    rp = H.nest2ring(nside_in, ch)
    u, v = H.child_order(r)
    npr = 4 * nside_in
    for t in range(2 * r - 1):
        sel = np.nonzero(u + v == t)[0]
        d = np.diff(rp[:, sel], axis=1)
        assert np.all((d == 1) | (d == 1 - npr)), t


def test_ud_grade_oracle_arithmetic():
    m = np.arange(48, dtype=np.float64)
    m[5] = H.UNSEEN
    m[6] = np.nan
    out = H.ud_grade(m, 1, order_in='NEST')
    assert out[0] == (0 + 1 + 2 + 3) / 4 and out[1] == (4 + 7) / 2
    assert H.ud_grade(m, 1, order_in='NEST', pess=True)[1] == H.UNSEEN
    m2 = np.arange(48, dtype=np.float64)
    assert np.array_equal(H.ud_grade(H.ud_grade(m2, 4, order_in='NEST'), 2, order_in='NEST', power=-2), m2 * 4)
    assert np.array_equal(H.ud_grade(H.ud_grade(m2, 4, order_in='RING'), 2, order_in='RING'), m2)


def test_import_opens_no_device():
    code = ("import baryonification_amd, baryonification_amd.utils, baryonification_amd.Runners, sys;"
            "from baryonification_amd import _lib;"
            "print(_lib._lib is None)")
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=H.REPO, check=True).stdout
    assert out.strip() == 'True'


def test_names_exported():
    import baryonification_amd.Runners as R
    from baryonification_amd.Runners import HealpixRunner
    assert 'regrid_pixels_hpix' in HealpixRunner.__all__ and R.regrid_pixels_hpix is regrid_pixels_hpix
    for name in ('ud_grade', 'get_interp_weights', 'get_interp_val'):
        assert callable(getattr(U, name))
    from baryonification_amd.utils import sphtfunc
    assert U.UNSEEN == sphtfunc.UNSEEN == -1.6375e30


# ------------------------------------------------------------------------------------------------------------------ argument rules
@pytest.mark.parametrize('nside_out', [0, 3, 6, 16384, 2.5, -4])
def test_ud_grade_bad_nside_out(nside_out):
    with pytest.raises(ValueError, match=r'\[1, 8192\]|integer'):
        U.ud_grade(np.zeros(12 * 16), nside_out)


def test_ud_grade_bad_arguments():
    with pytest.raises(ValueError, match=r'power of two'):
        U.ud_grade(np.zeros(12 * 9), 1)                          # nside_in = 3
    with pytest.raises(ValueError, match='12\\*nside'):
        U.ud_grade(np.zeros(50), 1)
    with pytest.raises(ValueError, match='RING'):
        U.ud_grade(np.zeros(48), 1, order_in='GALACTIC')
    with pytest.raises(ValueError, match='RING'):
        U.ud_grade(np.zeros(48), 1, order_out='nestt')
    with pytest.raises(ValueError, match='float32 or float64'):
        U.ud_grade(np.zeros(48), 1, dtype=np.int32)
    with pytest.raises(ValueError, match='one map'):
        U.ud_grade(np.zeros((2, 2, 48)), 1)


def test_interp_bad_arguments():
    for nside in (0, 8193, 1.5):
        with pytest.raises(ValueError, match=r'\[1, 8192\]|integer'):
            U.get_interp_weights(nside, 0.5, 0.5)
    with pytest.raises(ValueError, match='power of two'):
        U.get_interp_weights(3, 0.5, 0.5, nest=True)
    for th in (-1e-3, np.pi + 1e-9, np.nan):
        with pytest.raises(ValueError, match='THETA'):
            U.get_interp_weights(4, [0.1, th], [0.0, 0.0])
        with pytest.raises(ValueError, match='THETA'):
            U.get_interp_val(np.zeros(192), th, 0.0)
    with pytest.raises(ValueError, match='THETA'):
        U.get_interp_weights(4, 0.0, 91.0, lonlat=True)
    with pytest.raises(ValueError, match='finite'):
        U.get_interp_weights(4, 0.5, np.inf)
    with pytest.raises(ValueError, match=r'\[0, 192\)'):
        U.get_interp_weights(4, np.array([0, 192]))
    with pytest.raises(ValueError, match='integer'):
        U.get_interp_weights(4, np.array([0.5]))
    with pytest.raises(ValueError, match='12\\*nside'):
        U.get_interp_val(np.zeros(100), 0.5, 0.5)
    with pytest.raises(ValueError, match='power of two'):
        U.get_interp_val(np.zeros(12 * 9), 0.5, 0.5, nest=True)
    with pytest.raises(ValueError):
        U.get_interp_val(np.zeros(192), [0.1, 0.2], [0.1, 0.2, 0.3])         # shapes do not broadcast


def test_regrid_pixels_hpix_bad_arguments():
    h = np.zeros(48)
    vals, pix, w = np.ones(5), np.zeros((5, 4), dtype=np.int32), np.full((5, 4), 0.25)
    with pytest.raises(ValueError, match='float64'):
        regrid_pixels_hpix(np.zeros(48, dtype=np.float32), vals, pix, w)
    with pytest.raises(ValueError, match='float64'):
        regrid_pixels_hpix(np.zeros((48, 2))[:, 0], vals, pix, w)            # not contiguous
    with pytest.raises(ValueError, match='float64'):
        regrid_pixels_hpix(list(h), vals, pix, w)
    with pytest.raises(ValueError, match='transpose'):
        regrid_pixels_hpix(h, vals, pix.T, w)
    with pytest.raises(ValueError, match='transpose'):
        regrid_pixels_hpix(h, vals, pix, w.T)
    with pytest.raises(ValueError, match=r'\(N, 4\)'):
        regrid_pixels_hpix(h, np.ones(6), pix, w)
    with pytest.raises(ValueError, match='integers'):
        regrid_pixels_hpix(h, vals, pix.astype(np.float64), w)
    for bad in (48, -49, 10 ** 12):
        p = pix.copy().astype(np.int64)
        p[3, 2] = bad
        with pytest.raises(IndexError):
            regrid_pixels_hpix(h, vals, p, w)
    assert not h.any()


def test_cabi_refuses_before_device():
    L = _lib.load()
    z = np.zeros(64)
    assert L.bfgx_hpx_ud_grade(0, 3, 1, 1, 0, 0, 0, 1.0, 1, 1, z.ctypes.data, z.ctypes.data) == _lib.ERR_INVALID
    assert b'power of two' in L.bfgx_last_error()
    assert L.bfgx_hpx_ud_grade_device(0, None, 16384, 1, 1, 0, 0, 0, 1.0, 1, 1, z.ctypes.data, z.ctypes.data) == _lib.ERR_INVALID
    assert b'8192' in L.bfgx_last_error()
    assert L.bfgx_hpx_ud_grade(0, 4, 2, 1, 0, 0, 0, 1.0, 2, 1, z.ctypes.data, z.ctypes.data) == _lib.ERR_INVALID
    assert L.bfgx_hpx_interp_weights(0, 3, 1, 1, z.ctypes.data, z.ctypes.data, None, z.ctypes.data, z.ctypes.data) == _lib.ERR_INVALID
    t = np.array([4.0])
    assert L.bfgx_hpx_interp_weights(0, 4, 0, 1, t.ctypes.data, z.ctypes.data, None, z.ctypes.data, z.ctypes.data) == _lib.ERR_INVALID
    assert b'[0, pi]' in L.bfgx_last_error()
    assert L.bfgx_hpx_interp_val_device(0, None, 9000, 0, 1, 1, z.ctypes.data, 1, z.ctypes.data, z.ctypes.data, z.ctypes.data) == _lib.ERR_INVALID
    ip = np.array([0, 0, 0, 50], dtype=np.int64)
    assert L.bfgx_hpx_scatter_add(0, 48, z.ctypes.data, 1, z.ctypes.data, ip.ctypes.data, z.ctypes.data) == _lib.ERR_INVALID
    assert b'outside' in L.bfgx_last_error()
    assert L.bfgx_hpx_scatter_add_device(0, None, 48, None, 1, z.ctypes.data, ip.ctypes.data, z.ctypes.data) == _lib.ERR_INVALID


def test_compute_fails_loudly_without_gpu():
    if _lib.load().bfgx_device_count() > 0:
        pytest.skip("GPU present")
    m = np.random.default_rng(0).random(12 * 16)
    with pytest.raises(_lib.BfgxError, match="no HIP device"):
        U.ud_grade(m, 2)
    with pytest.raises(_lib.BfgxError, match="no HIP device"):
        U.get_interp_weights(4, [0.3], [1.0])
    with pytest.raises(_lib.BfgxError, match="no HIP device"):
        U.get_interp_weights(4, np.array([3]))
    with pytest.raises(_lib.BfgxError, match="no HIP device"):
        U.get_interp_val(m, 0.3, 1.0)
    with pytest.raises(_lib.BfgxError, match="no HIP device"):
        regrid_pixels_hpix(np.zeros(192), np.ones(2), np.zeros((2, 4), dtype=np.int64), np.ones((2, 4)))
