"""No GPU: the references of tests/flatstats_oracle.py on analytic cases, the tolerance test_gpu_flatstats.py uses (measured here, recorded
in the oracle file), and the argument checks of utils/flatstats.py and of the three C entries, which all come before any device call.

Found here: numpy's derivative chain against the long-double chain, relative to S_a = max|m_a b| max|x|, 2.26e-16, 2.79e-16, 4.45e-16
and 5.57e-16 at N = 8, 16, 64, 256."""
import numpy as np
import pytest

import fft2d_oracle as F
import flatstats_oracle as D


# ------------------------------------------------------------------------------------------------- the oracle on analytic cases
@pytest.mark.parametrize('N', [16, 64])
def test_plane_waves_have_their_analytic_derivatives(N):
    """u = cos(2 pi (m0 i + m1 j) / N + phi): u_x = -k0 sin, u_xy = -k0 k1 u, ...: the signs, the axes and the factor 2 pi / L"""
    L = 7.5
    for (m0, m1), phi in zip(D.waves(N), (0.0, 0.3, -1.1, 0.7)):
        assert abs(m0) < N // 2 and abs(m1) < N // 2
        x = D.wave(N, m0, m1, phi)
        ref = D.wave_derivatives(N, L, m0, m1, phi)
        got, S = D.derivatives(x, L), D.scales(x, L)
        for a in range(6):
            assert np.abs(got[a] - ref[a]).max() <= 1e-13 * S[a], (m0, m1, D.NAMES[a])
        spin = D.derivatives(x, L, spin_form=True)
        assert np.abs(spin[3] - (ref[3] + ref[5])).max() <= 2e-13 * S[3].clip(S[5])
        assert np.abs(spin[4] - (ref[3] - ref[5])).max() <= 2e-13 * S[3].clip(S[5])
        assert np.abs(spin[5] - 2 * ref[4]).max() <= 2e-13 * S[3].clip(S[5])
    # the axes are not interchangeable: a wave along x has no y derivative
    got = D.derivatives(D.wave(N, 3, 0), L)
    assert np.abs(got[2]).max() <= 1e-13 and np.abs(got[1]).max() > 1.0


@pytest.mark.parametrize('N', [8, 16, 64])
def test_nyquist_rule_keeps_every_map_real(N):
    """with the odd factors zeroed at the Nyquist index of their axis every output of a real map is real to rounding; without the rule
    u_x of a map with power at the Nyquist row is not"""
    L = 3.0
    x = F.noise(N) + D.wave(N, N // 2, 1) + D.wave(N, 2, N // 2) + D.wave(N, N // 2, N // 2)
    for spin in (False, True):
        z, S = D.derivatives_complex(x, L, spin_form=spin), D.scales(x, L, spin_form=spin)
        for a in range(6):
            assert np.abs(z[a].imag).max() <= 1e-14 * S[a], (spin, a)
    m = D.multipliers(N, L)
    h = N // 2
    assert not m[1][h].any() and not m[2][:, h].any() and not m[4][h].any() and not m[4][:, h].any()
    assert m[3][h, 0] == -(2 * np.pi / L * h) ** 2 and m[5][0, h] == -(2 * np.pi / L * h) ** 2 and m[1][1, 0] == 1j * 2 * np.pi / L
    for a in range(6):                                                     # Hermitian: m(-k) = conj(m(k))
        assert np.array_equal(m[a], np.conj(np.roll(m[a][::-1, ::-1], 1, (0, 1))))
    n = F.wave_numbers(N).astype(np.float64)
    naive = np.fft.ifft2(np.fft.fft2(x) * (1j * 2 * np.pi / L * n)[:, None])
    assert np.abs(naive.imag).max() > 1e-3


@pytest.mark.parametrize('N', [8, 64])
def test_half_plane_route_is_the_full_plane(N):
    """what N = 4096 is compared with: numpy's rfft2 / irfft2 with the same multipliers, against the full plane (and the full plane
    taken one map at a time, N = 2048's reference, against itself)"""
    L = 10.0
    x = F.noise(N) + D.wave(N, N // 2, 1) + D.wave(N, 2, N // 2)
    beam = D.beam_plane(N, L, 'gauss', 0.3)
    for spin in (False, True):
        full, S = D.derivatives(x, L, beam, spin), D.scales(x, L, beam, spin)
        half, Sh = D.derivatives_large(x, L, beam[:, :N // 2 + 1], spin, half=True)
        same, Ss = D.derivatives_large(x, L, beam, spin)
        assert np.allclose(S, Sh, rtol=1e-15, atol=0) and np.allclose(S, Ss, rtol=1e-15, atol=0)
        for a in range(6):
            assert np.abs(full[a] - half[a]).max() <= 2 * D.NUMPY_DER_ERR[N] * S[a], (spin, a)
            assert np.abs(full[a] - same[a]).max() <= 2 * D.NUMPY_DER_ERR[N] * S[a], (spin, a)


def test_peaks_on_integer_maps():
    n = 8
    m = D.plateau(n)
    edges = np.array([-10.0, 0.0, 8.0, 9.0, 10.0])
    for periodic in (True, False):
        cnt, flags = D.peaks(m, edges, periodic=periodic)
        assert flags[5, 5] == 1 and flags[5, 2] == -1 and np.abs(flags).sum() == 2         # the plateau holds no extremum, nor the flat background
        assert list(cnt['maxima']) == [0, 0, 1, 0] and list(cnt['minima']) == [1, 0, 0, 0]  # 8 sits on an edge: it belongs to [8, 9)
    # one bad neighbour removes a peak: by the mask, by NaN, by UNSEEN
    for bad in ('mask', np.nan, D.M.UNSEEN, np.inf):
        mm, mask = m.copy(), None
        if bad == 'mask':
            mask = np.ones((n, n), dtype=np.uint8)
            mask[4, 6] = 0
        else:
            mm[4, 6] = bad
        _, flags = D.peaks(mm, edges, mask=mask)
        assert flags[5, 5] == 0 and flags[5, 2] == -1 and np.abs(flags).sum() == 1
    # border pixels: extrema of the periodic patch, never of the open one
    b = np.ones((n, n))
    b[0, 3], b[n - 1, n - 1], b[4, 0] = 5.0, -2.0, 7.0
    _, fp = D.peaks(b, edges, periodic=True)
    _, fo = D.peaks(b, edges, periodic=False)
    assert fp[0, 3] == 1 and fp[n - 1, n - 1] == -1 and fp[4, 0] == 1 and np.abs(fp).sum() == 3 and not fo.any()
    # n = 3: every other pixel is a neighbour, each once
    t = np.arange(9.0).reshape(3, 3)
    _, f3 = D.peaks(t, edges)
    assert f3[2, 2] == 1 and f3[0, 0] == -1 and np.abs(f3).sum() == 2
    _, f3 = D.peaks(t, edges, periodic=False)
    assert not f3.any()


def test_minkowski_gaussian_2d_is_the_closed_form_of_the_sphere():
    from baryonification_amd import utils as U
    cl = 1.0 / (1.0 + np.arange(40.0)) ** 2
    t = np.linspace(-1.0, 1.5, 9)
    ref = U.minkowski_gaussian(cl, t)
    got = U.minkowski_gaussian_2d(ref['sigma0'], ref['sigma1'], t)
    for key in ('v0', 'v1', 'v2'):
        assert np.allclose(got[key], ref[key], rtol=1e-14, atol=0)
    assert got['sigma0'] == ref['sigma0'] and got['sigma1'] == ref['sigma1']
    for s0, s1 in ((0.0, 1.0), (-1.0, 1.0), (1.0, -1.0), (float('nan'), 1.0), (1.0, float('inf'))):
        with pytest.raises(ValueError, match='sigma0'):
            U.minkowski_gaussian_2d(s0, s1, t)


# ------------------------------------------------------------------------------------------------- the tolerance
@pytest.mark.parametrize('N', [8, 16, 64, 256])
def test_numpy_derivative_error_is_the_recorded_one(N):
    err = D.numpy_der_error(N)
    print("numpy's derivative chain against long double, N = %d: %.2e of S_a (recorded %.2e, bound %.2e)" % (N, err, D.NUMPY_DER_ERR[N], D.der_bound(N)))
    assert err <= D.NUMPY_DER_ERR[N] <= 1.5 * err


def test_der_bound_by_size():
    assert D.der_bound(8) == 16 * D.NUMPY_DER_ERR[8] and D.der_bound(64) == 16 * D.NUMPY_DER_ERR[64] and D.der_bound(32) == D.der_bound(64)
    assert D.der_bound(1024) == 16 * D.NUMPY_DER_ERR[256] * 10 / 8 and D.der_bound(4096) == 16 * D.NUMPY_DER_ERR[256] * 12 / 8


def test_relative_to_the_output_the_wave_is_much_worse():
    """why the errors are stated in S_a: u_yy of the wave (N/2 - 1, 2) is small against max|m b| max|x|"""
    N, L = 64, 10.0
    x = D.wave(N, N // 2 - 1, 2)
    got, ref, S = D.derivatives(x, L), D.derivatives_ld(x, L, which=[5]), D.scales(x, L)
    err = float(np.abs(got[5] - ref[0]).max())
    assert err / S[5] <= D.NUMPY_DER_ERR[64] and err / float(np.abs(ref[0]).max()) > 20 * err / S[5]


# ------------------------------------------------------------------------------------------------- argument checks, Python
def test_public_functions_refuse_bad_arguments():
    import torch
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    U = bfg.utils
    ok, bins = np.zeros((16, 16)), np.linspace(-1.0, 1.0, 5)
    cpu = torch.zeros((16, 16), dtype=torch.float64)
    spectral = [lambda m, **kw: U.derivatives_2d(m, 1.0, **kw), lambda m, **kw: U.minkowski_functionals_2d(m, 1.0, bins, **kw),
                lambda m, **kw: U.patch_statistics(m, 1.0, [0.0, 0.1], **kw)]
    for f in spectral:
        for bad in (np.zeros(16), np.zeros((16, 8)), np.zeros((12, 12)), np.zeros((4, 4)), np.zeros((2, 2, 16, 16))):
            with pytest.raises(ValueError):
                f(bad)
        with pytest.raises(ValueError, match='CUDA float64'):
            f(cpu)
    for f in spectral[:2]:
        for kw in (dict(fwhm=1.0, sigma=1.0), dict(tophat=1.0, beam=([0.0, 1.0], [1.0, 0.5])), dict(fwhm=1.0, sigma=1.0, tophat=1.0)):
            with pytest.raises(ValueError, match='at most one'):
                f(ok, **kw)
        for kw in (dict(fwhm=-1.0), dict(sigma=float('nan')), dict(tophat=-0.5), dict(beam=([1.0, 0.5], [1.0, 1.0])), dict(beam=([0.0, 1.0], [1.0]))):
            with pytest.raises(ValueError):
                f(ok, **kw)
    for L in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='L > 0'):
            U.derivatives_2d(ok, L)
        with pytest.raises(ValueError, match='L > 0'):
            U.minkowski_functionals_2d(ok, L, bins)
        with pytest.raises(ValueError, match='L > 0'):
            U.patch_statistics(ok, L, [0.1])
    # peak counts: any side in [3, 16384]
    for bad in (np.zeros(16), np.zeros((16, 8)), np.zeros((2, 2)), np.zeros((3, 3, 3))):
        with pytest.raises(ValueError):
            U.peak_counts_2d(bad, bins)
    with pytest.raises(ValueError, match='CUDA float64'):
        U.peak_counts_2d(cpu, bins)
    # bins, masks
    for badbins in ([0.0], [1.0, 0.0], [0.0, np.nan], np.zeros((2, 2)), np.arange(4098.0)):
        with pytest.raises(ValueError, match='bins'):
            U.peak_counts_2d(np.zeros((5, 5)), badbins)
    for badbins in ([0.0], [1.0, 0.0], np.arange(514.0)):
        with pytest.raises(ValueError, match='bins'):
            U.minkowski_functionals_2d(ok, 1.0, badbins)
        with pytest.raises(ValueError, match='bins'):
            U.patch_statistics(ok, 1.0, [0.1], mf_bins=badbins)
    with pytest.raises(ValueError, match='bins'):
        U.patch_statistics(ok, 1.0, [0.1], peak_bins=[2.0, 1.0])
    for f in (lambda mask: U.peak_counts_2d(ok, bins, mask=mask), lambda mask: U.minkowski_functionals_2d(ok, 1.0, bins, mask=mask),
              lambda mask: U.patch_statistics(ok, 1.0, [0.1], mask=mask)):
        with pytest.raises(ValueError, match='mask'):
            f(np.ones((16, 8)))
        with pytest.raises(ValueError, match='mask'):
            f(np.ones(256))
        with pytest.raises(ValueError, match='not one of each'):
            f(torch.ones((16, 16)))
    # patch_statistics
    with pytest.raises(ValueError, match='1 to 3 maps'):
        U.patch_statistics(np.zeros((4, 16, 16)), 1.0, [0.1])
    with pytest.raises(ValueError, match='one shape'):
        U.patch_statistics([ok, np.zeros((8, 8))], 1.0, [0.1])
    with pytest.raises(ValueError, match='not one of each'):
        U.patch_statistics([ok, cpu], 1.0, [0.1])
    for order in (1, 5, 2.5):
        with pytest.raises(ValueError, match='order'):
            U.patch_statistics(ok, 1.0, [0.1], order=order)
    with pytest.raises(ValueError, match='window'):
        U.patch_statistics(ok, 1.0, [0.1], window='box')
    for scales in ([], [-1.0], [np.nan], np.zeros((2, 2))):
        with pytest.raises(ValueError, match='scales'):
            U.patch_statistics(ok, 1.0, scales)
    # GriddedMap.statistics: its own side, 2-D maps only
    Map = bfg.utils.GriddedMap(map=np.zeros((12, 12)), redshift=0.2, bins=(np.arange(12) + 0.5) * 2.0, cosmo=dict(syn.COSMO))
    with pytest.raises(ValueError, match='power of two'):
        Map.statistics([1.0])
    Map = bfg.utils.GriddedMap(map=np.zeros((16, 16)), redshift=0.2, bins=(np.arange(16) + 0.5) * 2.0, cosmo=dict(syn.COSMO))
    with pytest.raises(ValueError, match='scales'):
        Map.statistics([-1.0])


# ------------------------------------------------------------------------------------------------- argument checks, C entries
def _ptr(a):
    return None if a is None else a.ctypes.data


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """host pointers stand in for device pointers: every check comes before the device is selected, so the answers are the same with and
    without a GPU"""
    from baryonification_amd import _lib, engine
    L = _lib.load()
    pitch = engine.fft_pitch(16)
    assert engine.derivatives_2d_work_doubles(16, 6) == 2 * 16 * pitch * 7 and engine.derivatives_2d_work_doubles(16, 1) == 2 * 16 * pitch * 2
    assert engine.derivatives_2d_work_doubles(4096, 6) == 2 * 4096 * 2056 * 7
    assert [engine.derivatives_2d_work_doubles(n, 6) for n in (4, 12, 8192, 0, -8)] == [0] * 5
    assert [engine.derivatives_2d_work_doubles(16, k) for k in (0, 2, 3, 5, 7, -1)] == [0] * 6
    w = np.zeros(engine.derivatives_2d_work_doubles(16, 6) + 2)
    sp = np.zeros(2 * 16 * pitch + 2)
    wa, sa = w[(-w.ctypes.data // 8) % 2:], sp[(-sp.ctypes.data // 8) % 2:]                # 16-byte aligned
    wu, su = wa[1:], sa[1:]                                                                # and not
    assert wa.ctypes.data % 16 == 0 and wu.ctypes.data % 16 == 8 and sa.ctypes.data % 16 == 0 and su.ctypes.data % 16 == 8
    o = np.zeros((6, 16, 16))
    der = lambda n=16, s=sa, Lb=1.0, kind=0, par=1.0, tk=None, tb=None, nder=6, spin=0, wk=wa, out=o: L.bfgx_derivatives_2d_device(   # noqa: E731
        0, None, n, _ptr(s), Lb, kind, par, _ptr(tk), _ptr(tb), 0 if tk is None else tk.size, nder, spin, _ptr(wk), _ptr(out))
    m, e = np.zeros((16, 16)), np.linspace(0.0, 1.0, 5)
    cnt, fl = np.zeros((2, 4), dtype=np.int64), np.zeros((16, 16), dtype=np.int8)
    pk = lambda n=16, per=1, a=m, mask=None, nb=4, ed=e, c=cnt, f=fl: L.bfgx_mapstats_peaks_2d_device(                               # noqa: E731
        0, None, n, per, _ptr(a), _ptr(mask), nb, _ptr(ed), _ptr(c), _ptr(f))
    up, down = np.array([0.0, 1.0, 2.0]), np.array([0.0, 2.0, 1.0])
    cases = [
        (lambda: der(s=None), _lib.ERR_INVALID, b'NULL'), (lambda: der(wk=None), _lib.ERR_INVALID, b'NULL'),
        (lambda: der(out=None), _lib.ERR_INVALID, b'NULL'),
        (lambda: der(n=12), _lib.ERR_UNSUPPORTED, b'8 <= n <= 4096'), (lambda: der(n=4), _lib.ERR_UNSUPPORTED, b'8 <= n <= 4096'),
        (lambda: der(n=8192), _lib.ERR_UNSUPPORTED, b'8 <= n <= 4096'),
        (lambda: der(Lb=0.0), _lib.ERR_INVALID, b'L > 0'), (lambda: der(Lb=float('nan')), _lib.ERR_INVALID, b'L > 0'),
        (lambda: der(kind=3, Lb=-1.0), _lib.ERR_INVALID, b'L > 0'),
        (lambda: der(par=-1.0), _lib.ERR_INVALID, b'width >= 0'), (lambda: der(kind=1, par=float('inf')), _lib.ERR_INVALID, b'width >= 0'),
        (lambda: der(kind=4), _lib.ERR_INVALID, b'kind'), (lambda: der(kind=-1), _lib.ERR_INVALID, b'kind'),
        (lambda: der(kind=2), _lib.ERR_INVALID, b'NULL'),
        (lambda: der(kind=2, tk=down, tb=up), _lib.ERR_INVALID, b'ascending'),
        (lambda: der(nder=2), _lib.ERR_INVALID, b'nder'), (lambda: der(nder=0), _lib.ERR_INVALID, b'nder'),
        (lambda: der(nder=7), _lib.ERR_INVALID, b'nder'),
        (lambda: der(wk=wu), _lib.ERR_INVALID, b'16-byte'), (lambda: der(s=su), _lib.ERR_INVALID, b'16-byte'),
        (lambda: pk(a=None), _lib.ERR_INVALID, b'NULL'), (lambda: pk(ed=None), _lib.ERR_INVALID, b'NULL'),
        (lambda: pk(c=None), _lib.ERR_INVALID, b'NULL'),
        (lambda: pk(n=2), _lib.ERR_INVALID, b'[3, 16384]'), (lambda: pk(n=0), _lib.ERR_INVALID, b'[3, 16384]'),
        (lambda: pk(n=-5), _lib.ERR_INVALID, b'[3, 16384]'), (lambda: pk(n=16385), _lib.ERR_INVALID, b'[3, 16384]'),
        (lambda: pk(n=1 << 33), _lib.ERR_INVALID, b'[3, 16384]'),
        (lambda: pk(nb=0), _lib.ERR_INVALID, b'[1, 4096]'), (lambda: pk(nb=4097), _lib.ERR_INVALID, b'[1, 4096]'),
        (lambda: pk(nb=-1), _lib.ERR_INVALID, b'[1, 4096]'),
    ]
    for i, (call, rc, word) in enumerate(cases):
        assert call() == rc, i
        assert word in L.bfgx_last_error(), (i, L.bfgx_last_error())
