"""What the masked-sky power spectra promise without a GPU: the oracle checks itself (exact 3j symbols against sympy, the sum rule and the
symmetry of the exact matrices, the float64 recursions against the exact matrices), the C entries and the Python functions refuse bad
arguments before any device call, ClBins is exact host arithmetic, and without a device every compute call fails loudly."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pcl_oracle as P
from baryonification_amd import _lib, utils as U
from baryonification_amd.utils import pseudocl


# ------------------------------------------------------------------------------------------------------------- the oracle
def test_oracle_3j_against_sympy():
    from sympy.physics.wigner import wigner_3j
    rng = np.random.default_rng(0)
    triples = [(2, 2, 0), (2, 2, 4), (3, 2, 2), (5, 5, 1), (9, 8, 16), (10, 7, 6), (12, 12, 0), (30, 28, 17)]
    triples += [(int(a), int(b), int(rng.integers(abs(a - b), a + b + 1))) for a, b in rng.integers(2, 40, size=(12, 2))]
    for l1, l2, l3 in triples:
        for m in ((0, 0, 0), (2, -2, 0)):
            assert P.w3j(l1, l2, l3, *m) == pytest.approx(float(wigner_3j(l1, l2, l3, *m)), rel=1e-14, abs=1e-300), (l1, l2, l3, m)
    assert P.w3j(3, 2, 2, 2, -2, 0) < 0 < P.w3j(2, 2, 0, 2, -2, 0)              # the signs are the standard convention's
    assert P.w3j(1, 2, 2, 2, -2, 0) == 0.0 and P.w3j(2, 2, 5, 0, 0, 0) == 0.0


def test_oracle_row_sums_and_symmetry():
    lmax, lw = 10, 4
    wl = np.random.default_rng(3).standard_normal(lw + 1)
    ex = P.exact_matrices(wl, lmax, ncols=lmax + lw + 1)                          # columns to lmax + lw: every l' a row couples to
    S = np.sum((2 * np.arange(lw + 1) + 1) * wl) / (4 * np.pi)
    assert np.abs(ex['00'][0].sum(axis=1) - S).max() <= 1e-14 * max(1.0, abs(S))
    assert np.abs((ex['++'][0] + ex['--'][0])[2:].sum(axis=1) - S).max() <= 1e-14 * max(1.0, abs(S))
    assert np.all(ex['++'][0][:2] == 0) and np.all(ex['--'][0][:, :2] == 0) and np.all(ex['0+'][0][:2] == 0)
    g = 2.0 * np.arange(lmax + 1) + 1.0
    for k in ('00', '0+', '++', '--'):
        a = g[:, None] * ex[k][0][:, :lmax + 1]
        assert np.abs(a - a.T).max() <= 1e-14 * np.abs(a).max(), k


def test_recursions_in_float64_against_exact_matrices():
    """the measurement behind the tolerance of tests/test_gpu_pcl.py: it must not exceed what pcl_oracle.RECURSION_ERROR records"""
    worst = {0: 0.0, 1: 0.0, 2: 0.0}
    for lmax, lw in P.SHAPES:
        wl, rows = P.shape_wl(lmax, lw), P.shape_rows(lmax)
        ex = P.exact_matrices(wl, lmax, rows=rows)
        for kind, keys in ((0, ('00',)), (1, ('0+',)), (2, ('++', '--'))):
            got = P.recursion_matrices(wl, lmax, kind, rows=rows)
            for key, m in zip(keys, got if kind == 2 else (got,)):
                ref, scale = ex[key]
                assert np.all(m[scale == 0] == 0.0)
                worst[kind] = max(worst[kind], (np.abs(m - ref) / np.where(scale > 0, scale, 1.0)).max())
    print("float64 recursions against exact: %r" % worst)
    assert worst[0] <= 1e-14
    assert 0.5 * P.RECURSION_ERROR[1] <= worst[1] <= P.RECURSION_ERROR[1]
    assert 0.5 * P.RECURSION_ERROR[2] <= worst[2] <= P.RECURSION_ERROR[2]


def test_oracle_workspace_restatement():
    lmax, edges = 11, [2, 5, 8, 12]
    rng = np.random.default_rng(1)
    mats = {k: (rng.random((lmax + 1, lmax + 1)) + (3 * np.eye(lmax + 1) if k != '--' else 0), None) for k in ('00', '0+', '++', '--')}
    for spins, ns in (((0, 0), 1), ((0, 2), 2), ((2, 2), 4)):
        w = P.workspace(mats, spins, edges, lmax)
        assert w['M'].shape == (ns * (lmax + 1),) * 2 and w['ell'].tolist() == [3.0, 6.0, 9.5]
        cb = rng.random((ns, 3))
        cl = np.stack([P.unbin_matrix(edges, lmax) @ c for c in cb])
        assert np.abs(w['decouple'](w['couple'](cl)) - cb).max() <= 1e-12
        assert np.abs(np.einsum('abcl,cl->ab', w['windows'], cl) - cb).max() <= 1e-12
    ee = np.zeros((4, lmax + 1))
    ee[0] = 1.0
    out = P.workspace(mats, (2, 2), edges, lmax)['couple'](ee)
    assert np.allclose(out[0], mats['++'][0].sum(axis=1)) and np.allclose(out[3], mats['--'][0].sum(axis=1)) and not out[1].any()


# ------------------------------------------------------------------------------------------------------------- the C entries
def _both(lmax, lw, kind, wl, m0, m1):
    """(rc, message) of the host entry and of the _device entry for the same arguments (host arrays stand in for device arrays: the
    call is refused before any of them is used)"""
    L = _lib.load()
    p = lambda a: None if a is None else a.ctypes.data
    h = (L.bfgx_pcl_coupling(0, lmax, lw, kind, p(wl), p(m0), p(m1)), L.bfgx_last_error())
    d = (L.bfgx_pcl_coupling_device(0, None, lmax, lw, kind, p(wl), p(m0), p(m1)), L.bfgx_last_error())
    return h, d


@pytest.mark.parametrize('lmax,lw,kind,null,text', [
    (-1, 2, 0, (), b'lmax must be in [0, 8191]'),
    (8192, 2, 0, (), b'lmax must be in [0, 8191]'),
    (4, -1, 0, (), b'lw must be in [0, 16383]'),
    (4, 16384, 0, (), b'lw must be in [0, 16383]'),
    (4, 2, -1, (), b'kind must be 0 (M00), 1 (M0+) or 2 (M++ and M--)'),
    (4, 2, 3, (), b'kind must be 0 (M00), 1 (M0+) or 2 (M++ and M--)'),
    (4, 2, 0, ('wl',), b'NULL'),
    (4, 2, 1, ('m0',), b'NULL'),
    (4, 2, 2, ('m1',), b'NULL argument: kind 2 writes M-- to m1'),
])
def test_c_entries_refuse_alike(lmax, lw, kind, null, text):
    a = {'wl': np.ones(3), 'm0': np.full((5, 5), -7.5), 'm1': np.full((5, 5), -7.5)}
    for k in null:
        a[k] = None
    h, d = _both(lmax, lw, kind, a['wl'], a['m0'], a['m1'])
    assert h[0] == d[0] == _lib.ERR_INVALID and h[1] == d[1] and text in h[1], (h, d)
    for k in ('m0', 'm1'):
        assert a[k] is None or np.all(a[k] == -7.5)


def test_abi_version_stays():
    assert _lib.load().bfgx_abi_version() == 4
    assert 'bfgx_pcl_coupling' in _lib.SYMBOLS and 'bfgx_pcl_coupling_device' in _lib.SYMBOLS


# ------------------------------------------------------------------------------------------------------------- Python arguments
def test_mode_coupling_matrix_arguments():
    wl = np.ones(5)
    for s in ((1, 0), (0, 1), (2, 4), (-2, 0)):
        with pytest.raises(NotImplementedError, match="spin"):
            U.mode_coupling_matrix(wl, 8, *s)
    for lmax in (-1, 8192, 2.5, 'x'):
        with pytest.raises(ValueError, match="lmax"):
            U.mode_coupling_matrix(wl, lmax)
    for bad in (np.ones((2, 3)), np.array([]), np.ones(3, dtype=complex)):
        with pytest.raises(ValueError, match="wl"):
            U.mode_coupling_matrix(bad, 8)


def test_field_and_mask_arguments():
    m8, m4 = np.ones(12 * 64), np.ones(12 * 16)
    bins = U.ClBins.linear(2, 23, 4)
    with pytest.raises(ValueError, match="nside"):
        U.pseudo_cl(m8, mask1=m4)
    with pytest.raises(ValueError, match="nside"):
        U.pseudo_cl(m8, m4)
    with pytest.raises(ValueError, match="nside"):
        U.pseudo_cl((m8, m4))
    with pytest.raises(ValueError):
        U.pseudo_cl(np.ones(100))                                       # no 12 nside^2
    with pytest.raises(ValueError, match="pair"):
        U.pseudo_cl([m8, m8, m8])
    with pytest.raises(ValueError, match="lmax"):
        U.pseudo_cl(m8, lmax=-2)
    with pytest.raises(ValueError, match="iter"):
        U.pseudo_cl(m8, iter=-1)
    with pytest.raises(ValueError, match="beyond lmax"):
        U.PseudoClWorkspace(m8, bins=bins, lmax=20)
    with pytest.raises(ValueError, match="ClBins"):
        U.PseudoClWorkspace(m8, bins=[2, 4, 8])
    with pytest.raises(ValueError, match="nside"):
        U.PseudoClWorkspace(m8, m4, bins=bins)
    with pytest.raises(NotImplementedError, match="spin"):
        U.PseudoClWorkspace(m8, spin1=1, bins=bins)
    with pytest.raises(ValueError, match="mask1"):
        U.decoupled_cl(m8, bins=bins)
    with pytest.raises(ValueError, match="nside"):
        U.decoupled_cl(m8, mask1=m4, bins=bins)
    for call in (lambda: U.pseudo_cl(m8, nest=True), lambda: U.mask_spectrum(m8, nest=True),
                 lambda: U.PseudoClWorkspace(m8, bins=bins, nest=True), lambda: U.decoupled_cl(m8, mask1=m8, bins=bins, nest=True)):
        with pytest.raises(NotImplementedError, match="NEST"):
            call()


# ------------------------------------------------------------------------------------------------------------- ClBins
def test_clbins_arithmetic():
    b = U.ClBins([2, 5, 6, 10])
    assert b.nbins == 3 and b.lmin == 2 and b.lmax == 9 and b.ell.tolist() == [3.0, 5.0, 7.5] and b.width.tolist() == [3.0, 1.0, 4.0]
    B = b.matrix(11)
    assert B.shape == (3, 12) and np.all(B.sum(axis=1) == 1.0) and B[0, 2:5].tolist() == [1 / 3] * 3 and not B[:, :2].any() and not B[:, 10:].any()
    assert np.array_equal(B @ np.arange(12.0), b.ell)
    assert b.bin_index(11).tolist() == [-1, -1, 0, 0, 0, 1, 2, 2, 2, 2, -1, -1]
    cl = np.arange(12.0) ** 2
    assert np.allclose(b.bin_cell(cl), [(4 + 9 + 16) / 3, 25.0, (36 + 49 + 64 + 81) / 4], rtol=1e-15)
    assert b.bin_cell(np.stack([cl, 2 * cl])).shape == (2, 3)
    u = b.unbin_cell([1.0, 2.0, 3.0], 11)
    assert u.tolist() == [0, 0, 1, 1, 1, 2, 3, 3, 3, 3, 0, 0] and b.unbin_cell([1.0, 2.0, 3.0]).shape == (10,)
    assert np.array_equal(b.bin_cell(u), [1.0, 2.0, 3.0])
    lin = U.ClBins.linear(2, 23, 4)
    assert lin.edges.tolist() == [2, 6, 10, 14, 18, 22] and lin.lmax == 21 and lin.ell.tolist() == [3.5, 7.5, 11.5, 15.5, 19.5]
    assert U.ClBins.linear(0, 7, 4).edges.tolist() == [0, 4, 8]
    for bad in ([3], [2, 2, 4], [4, 2], [-1, 3], [2.5, 4], [[2, 4]], [2, np.inf]):
        with pytest.raises(ValueError, match="edges"):
            U.ClBins(bad)
    for bad in ((2, 4, 4), (2, 10, 0), (-1, 10, 2)):
        with pytest.raises(ValueError, match="nlb"):
            U.ClBins.linear(*bad)
    with pytest.raises(ValueError, match="beyond lmax"):
        b.matrix(8)
    with pytest.raises(ValueError, match="beyond lmax"):
        b.bin_cell(np.ones(9))
    with pytest.raises(ValueError, match="bins"):
        b.unbin_cell([1.0, 2.0])


# ------------------------------------------------------------------------------------------------------------- no device
def test_without_a_device_every_compute_call_fails_loudly():
    if _lib.load().bfgx_device_count() > 0:
        pytest.skip("GPU present")
    wl = np.ones(3)
    m0, m1 = np.full((5, 5), -7.5), np.full((5, 5), -7.5)
    for kind in (0, 1, 2):
        rc = _lib.load().bfgx_pcl_coupling(0, 4, 2, kind, wl.ctypes.data, m0.ctypes.data, m1.ctypes.data)
        assert rc == _lib.ERR_NO_DEVICE and b'no HIP device' in _lib.load().bfgx_last_error()
        rc = _lib.load().bfgx_pcl_coupling_device(0, None, 4, 2, kind, wl.ctypes.data, m0.ctypes.data, m1.ctypes.data)
        assert rc == _lib.ERR_NO_DEVICE and b'no HIP device' in _lib.load().bfgx_last_error()
    assert np.all(m0 == -7.5) and np.all(m1 == -7.5)
    m = np.ones(12 * 16)
    bins = U.ClBins.linear(2, 11, 2)
    for call in (lambda: U.mode_coupling_matrix(wl, 4), lambda: U.mode_coupling_matrix(wl, 4, 2, 2), lambda: U.mask_spectrum(m),
                 lambda: U.pseudo_cl(m, mask1=m), lambda: U.pseudo_cl((m, m), mask1=m), lambda: U.PseudoClWorkspace(m, bins=bins),
                 lambda: U.decoupled_cl(m, mask1=m, bins=bins)):
        with pytest.raises(_lib.BfgxError, match="no HIP device"):
            call()


def test_importing_opens_no_device():
    """importing the package and its utils neither loads libbfgx nor torch: no device can have been opened"""
    code = ("import sys; import baryonification_amd.utils as U; from baryonification_amd import _lib; "
            "assert U.mode_coupling_matrix and U.PseudoClWorkspace and U.decoupled_cl and U.ClBins.linear(2, 9, 2).nbins == 4; "
            "assert _lib._lib is None and 'torch' not in sys.modules")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-c', code], cwd=repo, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
