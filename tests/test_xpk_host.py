"""Cross power spectrum, the parts that need no GPU: work-size arithmetic, the argument checks of the three C entries (stated once in
csrc/bfgx_xpk_api.inc, so the host and the _device entries must give the same message, and before any device call), the Python entry's
ValueErrors, the host entry without a device, and tests/xpk_oracle.py itself against a direct long-double DFT at N = 8."""
import ctypes as C

import numpy as np
import pytest

import fft_oracle as O
import xpk_oracle as X
from baryonification_amd import _lib, engine

SENTINEL = -12345.0
N0, NK0, L0 = 8, 4, 100.0


def _aligned16(n_doubles, off=0):
    """a float64 view whose address is 16-byte aligned, plus `off` doubles"""
    raw = np.zeros(n_doubles + 4)
    start = (-(raw.ctypes.data // 8) % 2) + off
    return raw[start:start + n_doubles]


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _outs(nk=NK0):
    return [np.full(nk, SENTINEL) for _ in range(4)] + [np.full(nk, -7, dtype=np.int64)]


def _host(n=N0, L=L0, nk=NK0, p=0, a='map', b='map', outs=None):
    """bfgx_cross_power_spectrum on host arrays -> (rc, message, outputs)"""
    m = np.ones(max(n, 1) ** 3 if 0 < n <= 64 else 8)
    outs = _outs(max(nk, 1) if nk <= 4096 else 4) if outs is None else outs
    rc = _lib.load().bfgx_cross_power_spectrum(0, n, _ptr(m if a == 'map' else a), _ptr(m if b == 'map' else b), float(L), nk, p, *[_ptr(o) for o in outs])
    return rc, _lib.load().bfgx_last_error(), outs


def _device(n=N0, L=L0, nk=NK0, p=0, work='ok', a='map'):
    """bfgx_cross_power_spectrum_device with host pointers in the device slots: the checks come before any device call and look at no content"""
    m = np.ones(8)
    w = _aligned16(64) if isinstance(work, str) else work
    outs = _outs()
    rc = _lib.load().bfgx_cross_power_spectrum_device(0, None, n, _ptr(m if a == 'map' else a), _ptr(m), float(L), nk, p, _ptr(w), *[_ptr(o) for o in outs])
    return rc, _lib.load().bfgx_last_error()


def _slab(n=N0, L=L0, nk=NK0, p=0, ncols=1, col0=0, spec='ok', work='ok'):
    s = _aligned16(4096) if isinstance(spec, str) else spec
    w = _aligned16(4096) if isinstance(work, str) else work
    outs = _outs()
    rc = _lib.load().bfgx_fft_slab_axis0_xpk_device(0, None, n, ncols, col0, _ptr(s), _ptr(w), float(L), nk, p, *[_ptr(o) for o in outs])
    return rc, _lib.load().bfgx_last_error()


def test_work_size_is_host_arithmetic():
    for n in (8, 16, 64, 128, 512, 1024):
        assert engine.cross_power_spectrum_work_doubles(n) == 2 * engine.power_spectrum_work_doubles(n) == 4 * n * n * engine.fft_pitch(n)


@pytest.mark.parametrize('kw,code,word', [
    (dict(n=7), 'ERR_UNSUPPORTED', b'8 <= n_grid <= 1024'), (dict(n=12), 'ERR_UNSUPPORTED', b'8 <= n_grid <= 1024'),
    (dict(n=4), 'ERR_UNSUPPORTED', b'8 <= n_grid <= 1024'), (dict(n=2048), 'ERR_UNSUPPORTED', b'8 <= n_grid <= 1024'),
    (dict(n=0), 'ERR_UNSUPPORTED', b'8 <= n_grid <= 1024'), (dict(n=-8), 'ERR_UNSUPPORTED', b'8 <= n_grid <= 1024'),
    (dict(nk=0), 'ERR_INVALID', b'1 <= nk <= 2048'), (dict(nk=2049), 'ERR_INVALID', b'1 <= nk <= 2048'), (dict(nk=-1), 'ERR_INVALID', b'1 <= nk <= 2048'),
    (dict(L=0.0), 'ERR_INVALID', b'L > 0'), (dict(L=-1.0), 'ERR_INVALID', b'L > 0'), (dict(L=float('nan')), 'ERR_INVALID', b'L > 0'),
    (dict(p=-1), 'ERR_INVALID', b'window_order'), (dict(p=4), 'ERR_INVALID', b'window_order'),
])
def test_shape_refusals_are_the_same_from_all_three_entries(kw, code, word):
    got = [f(**kw)[:2] for f in (_host, _device, _slab)]
    for rc, msg in got:
        assert rc == getattr(_lib, code) and word in msg, (kw, rc, msg)
    assert got[0][1] == got[1][1] == got[2][1]


def test_null_pointers_are_refused():
    m = np.ones(N0 ** 3)
    for pos in range(7):
        args = [m, m] + _outs()
        args[pos] = None
        rc = _lib.load().bfgx_cross_power_spectrum(0, N0, _ptr(args[0]), _ptr(args[1]), L0, NK0, 0, *[_ptr(o) for o in args[2:]])
        host_msg = _lib.load().bfgx_last_error()
        assert rc == _lib.ERR_INVALID and b'NULL' in host_msg
        assert all((o == SENTINEL).all() for o in args[2:6] if o is not None)
    w = _aligned16(64)
    for pos in range(8):
        args = [m, m, w] + _outs()
        args[pos] = None
        rc = _lib.load().bfgx_cross_power_spectrum_device(0, None, N0, _ptr(args[0]), _ptr(args[1]), L0, NK0, 0, *[_ptr(o) for o in args[2:]])
        assert rc == _lib.ERR_INVALID and _lib.load().bfgx_last_error() == host_msg
    for pos in range(7):
        args = [w, _aligned16(64)] + _outs()
        args[pos] = None
        rc = _lib.load().bfgx_fft_slab_axis0_xpk_device(0, None, N0, 1, 0, _ptr(args[0]), _ptr(args[1]), L0, NK0, 0, *[_ptr(o) for o in args[2:]])
        assert rc == _lib.ERR_INVALID and _lib.load().bfgx_last_error() == host_msg


def test_misaligned_complex_arrays_are_refused():
    rc, msg = _device(work=_aligned16(64, off=1))
    assert rc == _lib.ERR_INVALID and b'work_dev must be 16-byte aligned' in msg
    rc, msg = _slab(spec=_aligned16(4096, off=1))
    assert rc == _lib.ERR_INVALID and b'spec_a_dev must be 16-byte aligned' in msg
    rc, msg2 = _slab(work=_aligned16(4096, off=1))
    assert rc == _lib.ERR_INVALID and b'work_b_dev must be 16-byte aligned' in msg2
    assert msg.replace(b'spec_a_dev', b'X') == msg2.replace(b'work_b_dev', b'X')


def test_columns_outside_the_grid_and_overlapping_ranges_are_refused():
    for ncols, col0 in ((0, 0), (-1, 3), (1, -1), (1, 8), (3, 6), (9, 0), (2 ** 31 - 1, 2)):
        rc, msg = _slab(ncols=ncols, col0=col0)
        assert rc == _lib.ERR_INVALID and b'outside the grid' in msg, (ncols, col0, rc, msg)
    # one column of N = 8: 8 rows of pitch 8 complex values = 128 doubles; overlap by one value, from either side, and identity
    buf = _aligned16(4096)
    for spec, work in ((buf[:128], buf[126:254]), (buf[126:254], buf[:128]), (buf[:128], buf[:128])):
        rc, msg = _slab(spec=spec, work=work)
        assert rc == _lib.ERR_INVALID and b'overlap' in msg, (rc, msg)
    if _lib.load().bfgx_device_count() == 0:
        rc, msg = _slab(spec=buf[:128], work=buf[128:256])                 # adjacent ranges pass the checks: the next stop is the device
        assert rc == _lib.ERR_NO_DEVICE, (rc, msg)


def test_without_a_device_the_host_entry_is_refused_and_the_results_stay():
    if _lib.load().bfgx_device_count() > 0:
        pytest.skip("GPU present")
    rc, msg, outs = _host()
    assert rc == _lib.ERR_NO_DEVICE and b'no HIP device' in msg, (rc, msg)
    assert all((o == SENTINEL).all() for o in outs[:4]) and (outs[4] == -7).all()
    with pytest.raises(_lib.BfgxError, match="no HIP device"):
        engine.cross_power_spectrum(np.ones((8, 8, 8)), np.ones((8, 8, 8)), L0, NK0)


def test_python_entry_refuses_bad_inputs_before_any_device_call():
    import torch
    cube = np.zeros((16, 16, 16))
    with pytest.raises(ValueError, match="cubic"):
        engine.cross_power_spectrum(np.zeros((16, 16, 8)), np.zeros((16, 16, 8)), L0)
    with pytest.raises(ValueError, match="cubic"):
        engine.cross_power_spectrum(np.zeros((16, 16)), np.zeros((16, 16)), L0)
    with pytest.raises(ValueError, match="one shape"):
        engine.cross_power_spectrum(cube, np.zeros((8, 8, 8)), L0)
    with pytest.raises(ValueError, match="one of each"):
        engine.cross_power_spectrum(cube, torch.zeros((16, 16, 16), dtype=torch.float64), L0)
    with pytest.raises(ValueError, match="one of each"):
        engine.cross_power_spectrum(torch.zeros((16, 16, 16), dtype=torch.float64), cube, L0)
    for t in (torch.zeros((16, 16, 16), dtype=torch.float64), torch.zeros((16, 16, 16), dtype=torch.float32)):
        with pytest.raises(ValueError, match="CUDA float64"):                   # a host tensor, and the wrong dtype
            engine.cross_power_spectrum(t, t, L0)
        with pytest.raises(ValueError, match="CUDA float64"):
            engine.power_spectrum_tensor(t, L0)
    for w in (-1, 4, 1.5, 'tophat', 'CIC2', None, True):
        with pytest.raises(ValueError, match="window"):
            engine.cross_power_spectrum(cube, cube, L0, window=w)
    assert engine.WINDOW_ORDERS == {'none': 0, 'ngp': 1, 'cic': 2, 'tsc': 3}
    # what passes Python's checks is refused by the library with its own words
    with pytest.raises(NotImplementedError, match="8 <= n_grid <= 1024"):
        engine.cross_power_spectrum(np.zeros((12, 12, 12)), np.zeros((12, 12, 12)), L0)
    with pytest.raises(ValueError, match="1 <= nk <= 2048"):
        engine.cross_power_spectrum(cube, cube, L0, Nk=0)
    with pytest.raises(ValueError, match="L > 0"):
        engine.cross_power_spectrum(cube, cube, 0.0)


# ------------------------------------------------------------------------------------------------- the oracle itself
def test_window_weight_values():
    for N in (8, 16, 64, 1024):
        assert X.window_weight(N, 0).dtype == np.longdouble and (X.window_weight(N, 0) == 1).all()          # p = 0: exactly 1
        for p in (1, 2, 3):
            t = X.window_weight(N, p)
            assert t[0] == 1 and (t[1:] > 1).all()
            assert np.array_equal(t[1:N // 2], t[:N // 2:-1])                                                # s(n) is even
            assert abs(float(t[N // 2]) / (np.pi / 2) ** (2 * p) - 1) < 1e-15                                # s(N/2) = 2 / pi
            assert np.abs(t / X.window_weight(N, 1) ** p - 1).max() < 1e-17


def _cube_dft_ld(A):
    return O.dft_ld(O.dft_ld(O.dft_ld(A, axis=2), axis=1), axis=0)


@pytest.mark.parametrize('p', [0, 1, 2, 3])
@pytest.mark.parametrize('nk', [1, 3, 7])
def test_oracle_against_a_direct_long_double_dft(nk, p):
    """N = 8: cross_power_spectrum_ref (np.fft.fftn) against the same binning of a long-double DFT; B = A gives pab = paa; B = A rolled by
    d = (1, 2, 3) has F_B = F_A exp(-i k.d), so pab = <w |F_A|^2 cos(k.d)> per bin, of both signs"""
    N, L = 8, 305.0
    rng = np.random.default_rng(8 + nk)
    A = rng.poisson(4.0, (N, N, N)).astype(np.float64)
    A[3, 5, 7] += 50.0
    B = np.roll(A, (1, 2, 3), axis=(0, 1, 2))
    ref = X.cross_power_spectrum_ref(A, B, L, nk, p)
    FA = _cube_dft_ld(A)
    exact = X.binned_cube(FA, _cube_dft_ld(B), L, nk, p)
    good = ref['counts'] > 0
    assert good.any() and np.array_equal(ref['counts'], exact['counts'])
    for key in ('k', 'paa', 'pbb'):
        assert np.array_equal(np.isnan(ref[key]), ~good)
        assert np.abs(ref[key][good] / exact[key][good] - 1).max() < 1e-13, key
    scale = np.sqrt(exact['paa'] * exact['pbb'])[good]
    assert np.abs(ref['pab'][good] - exact['pab'][good]).max() / scale.max() < 1e-13
    assert np.abs(ref['pbb'][good] / ref['paa'][good] - 1).max() < 1e-13                       # a shift keeps |F|
    # the analytic form of the shifted pair
    i = np.arange(N)
    n = np.rint(np.fft.fftfreq(N) * N).astype(np.int64)
    ang = 8 * np.arctan(np.longdouble(1)) * ((n[:, None, None] * 1 + n[None, :, None] * 2 + n[None, None, :] * 3) % N).astype(np.longdouble) / N
    P = FA.real ** 2 + FA.imag ** 2
    t = X.window_weight(N, p)
    w = t[i[:, None, None]] * t[i[None, :, None]] * t[i[None, None, :]]
    _, kinds = O.mode_k_and_bin(N, L, nk, i[:, None, None], i[None, :, None], i[None, None, :])
    ok = (kinds >= 0) & (kinds < nk)
    want = np.array([(w * P * np.cos(ang))[ok & (kinds == b)].sum() for b in range(nk)], dtype=np.longdouble)[good] / ref['counts'][good]
    assert np.abs(ref['pab'][good] - want.astype(np.float64)).max() / scale.max() < 1e-13
    same = X.cross_power_spectrum_ref(A, A, L, nk, p)
    assert np.array_equal(same['pab'][good], same['paa'][good]) and np.abs(same['r'][good] - 1).max() < 1e-15
    if p == 0:
        from oracle import grid as G
        k_cen, Pk, k_c = G.power_spectrum(A, L, nk)
        assert np.array_equal(k_c, ref['counts'])
        assert np.abs(ref['paa'][good] / Pk[good] - 1).max() < 1e-13 and np.abs(ref['k'][good] / k_cen[good] - 1).max() < 1e-13


def test_axis0_reference_adds_up_to_the_cube():
    """axis0_xpk_ref over all columns of the half spectrum = the full-cube reference (the mirror weight stands for the other half)"""
    N, L, nk, p = 8, 305.0, 5, 2
    rng = np.random.default_rng(3)
    A, B = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))
    nz = N // 2 + 1
    spec_a = np.fft.fftn(A)[:, :, :nz]
    work_b = np.fft.fft(np.fft.rfft(B, axis=2), axis=1)
    paa, pbb, pab, ks, cnt = X.axis0_xpk_ref(spec_a, work_b, N, 0, L, nk, p)
    parts = [X.axis0_xpk_ref(spec_a[:, c0:c0 + nc], work_b[:, c0:c0 + nc], N, c0, L, nk, p) for c0, nc in ((0, 3), (3, 1), (4, 4))]
    assert np.array_equal(sum(q[4] for q in parts), cnt)
    ref = X.cross_power_spectrum_ref(A, B, L, nk, p)
    assert np.array_equal(cnt, ref['counts'])
    good = cnt > 0
    for got, key in ((paa, 'paa'), (pbb, 'pbb'), (ks, 'k')):
        assert np.abs(got[good] / cnt[good] / ref[key][good] - 1).max() < 1e-13
        assert np.abs(sum(q[{'paa': 0, 'pbb': 1, 'k': 3}[key]] for q in parts)[good] / got[good] - 1).max() < 1e-13
    assert np.abs(pab[good] / cnt[good] - ref['pab'][good]).max() / np.sqrt(ref['paa'] * ref['pbb'])[good].max() < 1e-13
