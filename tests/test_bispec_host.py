"""The bispectrum without a GPU: the numpy oracle against the brute-force triple sum and a closed form, the triangle lists of
engine.bispectrum_triangles, and what every new entry refuses before any device call."""
import numpy as np
import pytest

import bispec_oracle as B
from baryonification_amd import _lib, engine
from bispec_oracle import KF, L_BOX, half_integer_edges, noise_map, references, three_wave_case

SENTINEL = -7.5


# ------------------------------------------------------------------------------------------------- the oracle itself
@pytest.mark.parametrize('N', [8, 16])
def test_estimator_equals_brute_force(N):
    edges, tris, est, bru = references(N)
    assert len(tris) >= 10 and np.abs(bru['b_sum']).max() > 0
    err = np.abs(est['b_sum'] - bru['b_sum']) / est['abs_sum']
    print("N = %d: %d triangles, max |estimator - brute| / abs_sum = %.2e" % (N, len(tris), err.max()))
    assert err.max() <= 4 * np.log2(N ** 3) * 2.0 ** -53
    assert np.array_equal(np.rint(est['n_tri']).astype(np.int64), bru['n_tri'])
    assert np.abs(est['n_tri'] - bru['n_tri']).max() <= 1e-9 * max(1, bru['n_tri'].max())
    assert (bru['n_tri'] > 0).all()                                   # (closable bins of this width do hold triangles)
    assert np.array_equal(np.rint(est['n_modes']).astype(np.int64), bru['n_modes'])
    assert np.abs(est['pk_sum'] / bru['pk_sum'] - 1).max() <= 1e-13


@pytest.mark.parametrize('N', [8, 16])
def test_filtered_fields_are_real(N):
    """the filter depends on |k| alone, so a bin holds -k with k, Nyquist planes included: Im <= 1e-14 of Re"""
    edges = half_integer_edges(N)
    nyq = np.array([N // 2 - 0.5, N // 2 + 0.5]) * KF                  # the last bin alone: it holds Nyquist-plane modes
    for e in (edges, nyq, np.array([0.0, 0.5 * KF])):
        for unit in (0, 1):
            f = B.fields(noise_map(N), L_BOX, e, unit)
            for fi in f:
                assert np.abs(fi.imag).max() <= 1e-14 * np.abs(fi.real).max()


def test_three_wave_closed_form():
    edges, x, tri, closed = three_wave_case()
    assert len(set(tri)) == 3 and min(tri) >= 0
    tris = np.array(B.closable(edges), dtype=np.int32)
    at = [tuple(t) for t in tris].index(tri)
    est = B.estimator(x, L_BOX, edges, tris)
    scale = est['abs_sum'][at]
    bound = 4 * np.log2(16 ** 3) * 2.0 ** -53 * scale
    assert abs(closed) > 0.1 * scale
    assert abs(est['b_sum'][at] - closed) <= bound
    others = np.delete(est['b_sum'], at)
    assert np.abs(others).max() <= bound


# ------------------------------------------------------------------------------------------------- triangle lists
def test_triangle_lists():
    edges = np.array([0.0, 1.0, 2.5, 3.0, 7.0, 7.5, 20.0])             # uneven: (0, 0, l) closes for l <= 1 only, (3, 3, 5) closes, (0, 1, 4) does not
    all_ = engine.bispectrum_triangles(edges)
    assert all_.dtype == np.int32 and all_.shape[1] == 3
    assert [tuple(t) for t in all_] == B.closable(edges)
    assert (0, 0, 1) in B.closable(edges) and (0, 0, 2) not in B.closable(edges) and (0, 1, 4) not in B.closable(edges)
    eq = engine.bispectrum_triangles(edges, 'equilateral')
    iso = engine.bispectrum_triangles(edges, 'isosceles')
    assert [tuple(t) for t in eq] == [(i, i, i) for i in range(6)]
    assert all(t[0] == t[1] <= t[2] for t in iso) and len(eq) < len(iso) < len(all_)
    s_all = {tuple(t) for t in all_}
    assert {tuple(t) for t in eq} <= {tuple(t) for t in iso} <= s_all
    assert {tuple(t) for t in iso} == {t for t in s_all if t[0] == t[1]}
    with pytest.raises(ValueError):
        engine.bispectrum_triangles(edges, 'squeezed')


# ------------------------------------------------------------------------------------------------- refusals
def _aligned16(n, off=0):
    """n float64 starting 16-byte aligned (off = 1: 8 bytes past such a boundary)"""
    a = np.zeros(n + 3)
    return a[((a.ctypes.data // 8) % 2 + off):][:n]


def _p(a):
    return a.ctypes.data if isinstance(a, np.ndarray) else a


def _args():
    """name -> valid small arguments after `device` (host arrays stand in for device arrays: every call is refused before they are used)"""
    e2 = np.array([0.5, 1.5, 2.5]) * KF
    tri = np.array([[0, 0, 1]], dtype=np.int32)
    w = _aligned16(64)
    return {
        'bfgx_fft_slab_axis0_device': [None, 8, 1, w, 1],
        'bfgx_ifft_slab_planes_device': [None, 8, 1, w, np.zeros(64)],
        'bfgx_bispectrum_shell_fields_device': [None, 8, L_BOX, 2, e2, w, 0, _aligned16(64), np.zeros(8)],
        'bfgx_bispectrum_device': [None, 8, np.zeros(512), L_BOX, 2, e2, 1, tri, w, np.zeros(1), np.zeros(1), np.zeros(2), np.zeros(2)],
        'bfgx_bispectrum': [8, np.zeros(512), L_BOX, 2, e2, 1, tri, np.zeros(1), np.zeros(1), np.zeros(2), np.zeros(2)],
    }


# position of n_grid / nbins / the edges / the triangles / the complex work arrays among those arguments
WHERE = {
    'bfgx_fft_slab_axis0_device': dict(n=1, work=[3]),
    'bfgx_ifft_slab_planes_device': dict(n=1, work=[3]),
    'bfgx_bispectrum_shell_fields_device': dict(n=1, nb=3, edges=4, work=[5, 7]),
    'bfgx_bispectrum_device': dict(n=1, nb=4, edges=5, ntri=6, tri=7, work=[8]),
    'bfgx_bispectrum': dict(n=0, nb=3, edges=4, ntri=5, tri=6, work=[]),
}
NAMES = sorted(WHERE)


def _call(name, args):
    L = _lib.load()
    rc = getattr(L, name)(0, *[_p(a) for a in args])
    return rc, L.bfgx_last_error()


@pytest.mark.parametrize('name', NAMES)
def test_null_pointers_are_refused_first(name):
    args = _args()[name]
    for i, a in enumerate(args):
        if isinstance(a, np.ndarray):
            bad = list(args)
            bad[i] = None
            bad[WHERE[name]['n']] = 12                                  # (also a bad n_grid: NULL is answered first)
            rc, msg = _call(name, bad)
            assert rc == _lib.ERR_INVALID and b'NULL' in msg, (name, i, rc, msg)


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('n', [0, 4, 12, 24, 2048, -8])
def test_bad_n_grid_is_unsupported(name, n):
    bad = list(_args()[name])
    bad[WHERE[name]['n']] = n
    rc, msg = _call(name, bad)
    assert rc == _lib.ERR_UNSUPPORTED and b'power of two' in msg, (rc, msg)


@pytest.mark.parametrize('name', [n for n in NAMES if 'nb' in WHERE[n]])
def test_bad_bins_are_refused(name):
    w = WHERE[name]
    for nb in (0, 33):
        bad = list(_args()[name])
        bad[w['nb']] = nb
        bad[w['edges']] = (np.arange(34) + 0.5) * KF
        rc, msg = _call(name, bad)
        assert rc == _lib.ERR_INVALID and b'nbins <= 32' in msg, (rc, msg)
    for edges, word in ((np.array([2.5, 1.5, 0.5]) * KF, b'ascending'), (np.array([0.5, 0.5, 1.5]) * KF, b'ascending'),
                        (np.array([-0.5, 0.5, 1.5]) * KF, b'non-negative'), (np.array([0.5, np.nan, 1.5]) * KF, b'finite'),
                        (np.array([0.5, 1.5, np.inf]) * KF, b'finite')):
        bad = list(_args()[name])
        bad[w['edges']] = edges
        rc, msg = _call(name, bad)
        assert rc == _lib.ERR_INVALID and word in msg, (edges, rc, msg)
    bad = list(_args()[name])
    bad[w['edges'] - 2] = 0.0                                          # L sits two places before the edges in all three
    rc, msg = _call(name, bad)
    assert rc == _lib.ERR_INVALID and b'L > 0' in msg, (rc, msg)


@pytest.mark.parametrize('name', [n for n in NAMES if 'tri' in WHERE[n]])
def test_bad_triangles_are_refused(name):
    w = WHERE[name]
    for t in ([[0, 0, 2]], [[-1, 0, 1]], [[0, 1, 1], [0, 5, 1]]):
        bad = list(_args()[name])
        bad[w['tri']] = np.array(t, dtype=np.int32)
        bad[w['ntri']] = len(t)
        rc, msg = _call(name, bad)
        assert rc == _lib.ERR_INVALID and b'outside [0, 2)' in msg, (rc, msg)
    for ntri in (0, 8193):
        bad = list(_args()[name])
        bad[w['tri']] = np.zeros((8193, 3), dtype=np.int32)
        bad[w['ntri']] = ntri
        rc, msg = _call(name, bad)
        assert rc == _lib.ERR_INVALID and b'ntri <= 8192' in msg, (rc, msg)


@pytest.mark.parametrize('name', [n for n in NAMES if WHERE[n]['work']])
def test_misaligned_complex_arrays_are_refused(name):
    for pos in WHERE[name]['work']:
        bad = list(_args()[name])
        bad[pos] = _aligned16(64, off=1)
        rc, msg = _call(name, bad)
        assert rc == _lib.ERR_INVALID and b'16-byte aligned' in msg, (pos, rc, msg)


def test_slab_extents_are_refused():
    w = _aligned16(64)
    for planes in (0, 9):
        rc, msg = _call('bfgx_ifft_slab_planes_device', [None, 8, planes, w, np.zeros(64)])
        assert rc == _lib.ERR_INVALID and b'planes' in msg
        rc, msg = _call('bfgx_fft_slab_axis0_device', [None, 8, planes, w, 0])
        assert rc == _lib.ERR_INVALID and b'ncols' in msg


def test_work_size_is_host_arithmetic():
    for n in (8, 64, 512, 1024):
        for nb in (1, 16, 32):
            half = 2 * n * n * engine.fft_pitch(n)
            assert engine.bispectrum_work_doubles(n, nb) >= 2 * half + nb * n ** 3
            assert engine.bispectrum_work_doubles(n, nb) % 2 == 0
    assert engine.bispectrum_work_doubles(12, 4) == 0 and engine.bispectrum_work_doubles(64, 33) == 0 and engine.bispectrum_work_doubles(64, 0) == 0


def test_without_a_device_the_host_entry_is_refused_and_the_results_stay():
    if _lib.load().bfgx_device_count() > 0:
        pytest.skip("GPU present")
    args = _args()['bfgx_bispectrum']
    for a in args[-4:]:
        a[:] = SENTINEL
    rc, msg = _call('bfgx_bispectrum', args)
    assert rc == _lib.ERR_NO_DEVICE and b'no HIP device' in msg, (rc, msg)
    for a in args[-4:]:
        assert (a == SENTINEL).all()


def test_python_entry_refuses_shapes_and_sizes_before_any_device_call():
    edges = half_integer_edges(16)
    with pytest.raises(ValueError, match="cubic"):
        engine.bispectrum(np.zeros((16, 16, 8)), L_BOX, edges)
    with pytest.raises(ValueError, match="cubic"):
        engine.bispectrum(np.zeros((16, 16)), L_BOX, edges)
    with pytest.raises(ValueError, match="nbins <= 32"):
        engine.bispectrum(np.zeros((16, 16, 16)), L_BOX, (np.arange(34) + 0.5) * KF)
    with pytest.raises(ValueError, match="ntri <= 8192"):
        engine.bispectrum(np.zeros((16, 16, 16)), L_BOX, edges, triangles=np.zeros((8193, 3), dtype=np.int32))
    with pytest.raises(ValueError, match="triangles"):
        engine.bispectrum(np.zeros((16, 16, 16)), L_BOX, edges, triangles=np.zeros((4, 2), dtype=np.int32))
