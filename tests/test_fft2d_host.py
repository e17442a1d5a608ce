"""No GPU: the references of tests/fft2d_oracle.py on analytic cases, the tolerances test_gpu_fft2d.py uses (measured here, recorded in
the oracle file), and the argument checks of utils/flatsky.py and of the C entries, which all come before any device call.

Found here: numpy's sampled single-transform error 3.99e-16 (N = 2048) and 2.94e-16 (4096); numpy's chain error 2.26e-16, 2.79e-16,
3.48e-16, 3.44e-16 at N = 8, 16, 64, 256.  Gaussian bump (sigma = 3 pixels on 128^2, rings from 1 to 12 pixels): mean_t of the oracle's
Kaiser-Squires shear against the ring means of kappa_bar(<r) - kappa(r) to 1.07e-5 of the largest mean_t, 0.294 (the periodic images,
whose e^(-4 i phi) field the pixels of a ring do not average out exactly), |mean_x| <= 6.1e-18 (the halo sits on a pixel centre: the
pixels of a ring come in mirror pairs)."""
import numpy as np
import pytest

import fft_oracle as O
import fft2d_oracle as F
import gridprofiles_oracle as K


# ------------------------------------------------------------------------------------------------- the oracle on analytic cases
@pytest.mark.parametrize('N', [8, 16, 64])
def test_plane_wave_lands_in_its_two_modes(N):
    for p, q in [(0, 0), (1, 0), (0, 1), (N // 2, 0), (0, N // 2), (N // 2, N // 2), (N - 1, 3), (37 % N, N // 2 - 1)]:
        x = O.plane_wave(N, p, q)
        full = np.zeros((N, N))
        full[p % N, q % N] += 0.5 * N * N
        full[-p % N, -q % N] += 0.5 * N * N
        assert np.abs(np.fft.fft2(x) - full).max() <= 1e-13 * N * N
        for a, c in [(p % N, q % N), (-p % N, -q % N), (1, 2), (0, 0)]:
            assert abs(complex(F.coeff_ld(x, a, c)) - full[a, c]) <= 1e-15 * N * N
        # the binning sees the two modes (one of them through the mirror weight) and nothing else
        L, nk = 305.0, 7
        ref = F.cross_power_spectrum_ref(x, x, L, nk)
        k, kinds = F.mode_k_and_bin(N, L, nk)
        lit = {(p % N, q % N), (-p % N, -q % N)}
        expect = np.zeros(nk)
        for a, c in lit:
            if 0 <= kinds[a, c] < nk:
                expect[kinds[a, c]] += full[a, c] ** 2
        got = np.nan_to_num(ref['paa'] * ref['counts'])
        assert np.allclose(got, expect, rtol=1e-12, atol=1e-12 * N ** 4)


def test_coeff_ld_against_whole_planes():
    x = F.noise(64)
    ref = F.fft2_ld(x)
    for a, c in F.sampled_modes(64):
        assert abs(F.coeff_ld(x, a, c) - ref[a, c]) <= 1e-17 * np.abs(ref).max()


def _bump_profiles(shear):
    from baryonification_amd import synthetic as syn
    from oracle import grid as G
    b = F.BUMP
    bins, kappa, gt = F.bump_maps()
    pairs = K.pairs(bins, 2, F.bump_catalog(bins), b['redshift'], b['eps'], G.grid_background(syn.COSMO))
    assert pairs['R_q'][0] > b['edges'][-1]
    return K.measure(pairs, b['edges'], gt, shear=shear)


def test_gaussian_bump_has_the_analytic_tangential_shear():
    """gamma_t = kappa_bar(<r) - kappa(r) > 0 around a mass peak in MeasureProfilesGrid's convention, gamma_x = 0: the ring means of the
    oracle's shear against the ring means of the analytic profile over the same pixels"""
    bins, kappa, gt = F.bump_maps()
    b = F.BUMP
    assert np.exp(-0.5 * (np.pi * b['sigma'] * b['N'] / b['L']) ** 2) < 1e-16           # nothing at the Nyquist frequency: no aliasing
    g1, g2 = F.kappa_to_shear(kappa)
    o = _bump_profiles((g1, g2))
    n = o['npix_shear'][0]
    assert np.all(n[1:] > 0) and np.array_equal(n[1:], o['npix'][0][1:])
    mean_t, mean_x, analytic = o['sum_t'][0][1:] / n[1:], o['sum_x'][0][1:] / n[1:], o['sum'][0][1:] / n[1:]
    assert np.all(mean_t > 0)
    res_t = float(np.abs(mean_t - analytic).max() / np.abs(mean_t).max())
    res_x = float(np.abs(mean_x).max())
    print("Gaussian bump: residual of mean_t %.2e of max|mean_t| = %.3f, max|mean_x| %.2e" % (res_t, np.abs(mean_t).max(), res_x))
    assert res_t <= 4 * F.BUMP_RESIDUAL_T
    assert res_x <= 4 * F.BUMP_RESIDUAL_X


def test_shear_to_kappa_inverts_kappa_to_shear():
    """... for a kappa without power at a Nyquist index, up to the mean"""
    for N in (8, 64):
        spec = np.fft.fft2(F.noise(N, 1))
        spec[N // 2, :] = 0
        spec[:, N // 2] = 0
        kappa = np.fft.ifft2(spec).real
        ke, kb = F.shear_to_kappa(*F.kappa_to_shear(kappa))
        scale = np.abs(kappa).max()
        assert np.abs(ke - (kappa - kappa.mean())).max() <= 1e-13 * scale
        assert np.abs(kb).max() <= 1e-13 * scale
    c2, s2 = F.ks_factors(16)
    assert c2[0, 0] == 0 and s2[0, 0] == 0 and not s2[8].any() and not s2[:, 8].any() and c2[8, 0] == 1 and c2[0, 8] == -1 and c2[8, 8] == 0
    assert np.array_equal(s2, np.roll(s2[::-1, ::-1], 1, (0, 1))) and np.array_equal(c2, np.roll(c2[::-1, ::-1], 1, (0, 1)))   # real fields stay real


def test_filters_of_the_oracle():
    k = F.k_plane(16, 10.0)
    assert k[0, 0] == 0 and np.isclose(k[8, 8], 2 * np.pi / 10.0 * 8 * np.sqrt(2))
    assert F.beam_gauss(k, 0.0).min() == 1.0 and F.beam_tophat(k, 0.0).min() == 1.0 and F.beam_tophat(k, 1.0)[0, 0] == 1.0
    assert np.isclose(F.beam_tophat(np.array([1e-4]), 1.0)[0], 1 - 1e-8 / 8, rtol=0, atol=1e-15)
    x = F.noise(16)
    assert np.abs(F.smoothing_ref(x, 10.0, lambda kk: F.beam_gauss(kk, 0.0)) - x).max() <= 1e-15 * np.abs(x).max()
    tk, tb = np.array([0.5, 1.0, 2.0]), np.array([1.0, 0.5, 0.25])
    assert np.array_equal(F.beam_table(np.array([0.0, 0.75, 3.0]), tk, tb), [1.0, 0.75, 0.25])


# ------------------------------------------------------------------------------------------------- the tolerances
@pytest.mark.parametrize('N', [2048, 4096])
def test_numpy_sampled_error_is_the_recorded_one(N):
    modes = F.sampled_modes(N)
    for axis in (0, 1):
        assert {0, 1, N // 2 - 1, N // 2} <= {m[axis] for m in modes}
    assert len(modes) == 8
    err = F.numpy_error_sampled(N)
    print("numpy against long double on 8 modes, N = %d: %.2e (recorded %.2e, bound %.2e)" % (N, err, F.NUMPY_ERR_SAMPLED[N], F.bound(N)))
    assert err <= F.NUMPY_ERR_SAMPLED[N] <= 1.5 * err


@pytest.mark.parametrize('N', [8, 16, 64, 256])
def test_numpy_chain_error_is_the_recorded_one(N):
    err = F.numpy_chain_error(N)
    print("numpy's chain against long double, N = %d: %.2e (recorded %.2e, bound %.2e)" % (N, err, F.NUMPY_CHAIN_ERR[N], F.chain_bound(N)))
    assert err <= F.NUMPY_CHAIN_ERR[N] <= 1.5 * err


def test_bounds_by_size():
    assert F.bound(1024) == O.bound(1024) and F.bound(8) == O.bound(8)
    assert F.bound(2048) == 16 * F.NUMPY_ERR_SAMPLED[2048] and F.bound(4096) == 16 * F.NUMPY_ERR_SAMPLED[4096]
    assert F.chain_bound(8) == 16 * F.NUMPY_CHAIN_ERR[8] and F.chain_bound(64) == 16 * F.NUMPY_CHAIN_ERR[64]
    assert F.chain_bound(1024) == 16 * F.NUMPY_CHAIN_ERR[256] * 10 / 8 and F.chain_bound(4096) == 16 * F.NUMPY_CHAIN_ERR[256] * 12 / 8


# the shapes test_gpu_fft2d.py bins at: (N, Nk, L)
BIN_SHAPES = [(32, 15, 305.0), (64, 31, 1.0), (64, 62, 1000.0 / 3.0), (128, 63, 2 * np.pi), (16, 1, 305.0), (16, 2, 305.0), (64, 2048, 305.0),
              (2048, 180, 305.0)]


def test_bin_shapes_put_modes_on_edges():
    """at least three of the shapes have modes whose bin the reciprocal floor gets wrong, or modes exactly on a bin edge"""
    hard = []
    for N, nk, L in BIN_SHAPES:
        differ, on_edge = F.edge_disagreements(N, L, nk)
        print("N = %4d nk = %4d L = %-8.6g: the two floors differ at %d modes, %d modes on an edge" % (N, nk, L, differ, on_edge))
        if differ or on_edge:
            hard.append((N, nk, L))
    assert len(hard) >= 3


# ------------------------------------------------------------------------------------------------- argument checks, Python
def test_public_functions_refuse_bad_arguments():
    import torch
    from baryonification_amd import utils as U
    ok = np.zeros((16, 16))
    one = [U.rfft2, U.kappa_to_shear_2d, lambda m: U.power_spectrum_2d(m, 1.0), lambda m: U.smoothing_2d(m, 1.0, fwhm=0.1),
           lambda m: U.cross_power_spectrum_2d(m, m, 1.0), lambda m: U.shear_to_kappa_2d(m, m)]
    for f in one:
        for bad in (np.zeros(16), np.zeros((16, 8)), np.zeros((16, 16, 16)), np.zeros((12, 12)), np.zeros((4, 4)), np.zeros((8192, 1))):
            with pytest.raises(ValueError):
                f(bad)
        with pytest.raises(ValueError, match='CUDA float64'):
            f(torch.zeros((16, 16), dtype=torch.float64))                 # a CPU tensor
    with pytest.raises(ValueError, match='power of two'):
        U.irfft2(np.zeros((12, 7), dtype=complex), 12)
    with pytest.raises(ValueError, match='shape'):
        U.irfft2(np.zeros((16, 8), dtype=complex), 16)
    two = [lambda a, b: U.cross_power_spectrum_2d(a, b, 1.0), U.shear_to_kappa_2d]
    for f in two:
        with pytest.raises(ValueError, match='one shape'):
            f(ok, np.zeros((8, 8)))
        with pytest.raises(ValueError, match='not one of each'):
            f(ok, torch.zeros((16, 16), dtype=torch.float64))
        with pytest.raises(ValueError, match='not one of each'):
            f(torch.zeros((16, 16), dtype=torch.float64), ok)
    for w in ('pcs', 4, -1, True, None):
        with pytest.raises(ValueError, match='window'):
            U.power_spectrum_2d(ok, 1.0, window=w)
    for nk in (0, 2049, -3, 1.5):
        with pytest.raises(ValueError, match='Nk'):
            U.power_spectrum_2d(ok, 1.0, Nk=nk)
        with pytest.raises(ValueError, match='Nk'):
            U.cross_power_spectrum_2d(ok, ok, 1.0, Nk=nk)
    for L in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='L > 0'):
            U.power_spectrum_2d(ok, L)
        with pytest.raises(ValueError, match='L > 0'):
            U.smoothing_2d(ok, L, fwhm=1.0)
    for kw in ({}, dict(fwhm=1.0, sigma=1.0), dict(tophat=1.0, beam=([0.0, 1.0], [1.0, 0.5])), dict(fwhm=1.0, sigma=1.0, tophat=1.0)):
        with pytest.raises(ValueError, match='exactly one'):
            U.smoothing_2d(ok, 1.0, **kw)
    for kw in (dict(fwhm=-1.0), dict(sigma=float('nan')), dict(tophat=-0.5), dict(beam=([1.0, 0.5], [1.0, 1.0])), dict(beam=([0.0, 1.0], [1.0]))):
        with pytest.raises(ValueError):
            U.smoothing_2d(ok, 1.0, **kw)


def test_gridded_map_power_spectrum_checks_2d_maps_on_the_host():
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    bins = (np.arange(12) + 0.5) * 2.0
    Map = bfg.utils.GriddedMap(map=np.zeros((12, 12)), redshift=0.2, bins=bins, cosmo=dict(syn.COSMO))
    with pytest.raises(ValueError, match='power of two'):
        Map.power_spectrum()
    Map = bfg.utils.GriddedMap(map=np.zeros((16, 16)), redshift=0.2, bins=(np.arange(16) + 0.5) * 2.0, cosmo=dict(syn.COSMO))
    with pytest.raises(ValueError, match='Nk'):
        Map.power_spectrum(Nk=0)


# ------------------------------------------------------------------------------------------------- argument checks, C entries
def _ptr(a):
    return None if a is None else a.ctypes.data


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """host pointers stand in for device pointers: every check comes before the device is selected, so the answers are the same with and
    without a GPU"""
    from baryonification_amd import _lib, engine
    L = _lib.load()
    m, w, o = np.zeros((16, 16)), np.zeros(engine.fft2_work_doubles(16) + 2), np.zeros((4, 16 * 16))
    cnt = np.zeros(8, dtype=np.uint64)
    assert engine.fft2_work_doubles(16) == 6 * 16 * engine.fft_pitch(16) and engine.fft2_work_doubles(4096) == 6 * 4096 * 2056
    assert [engine.fft2_work_doubles(n) for n in (4, 12, 8192, 0, -8)] == [0] * 5
    wa = w[(-w.ctypes.data // 8) % 2:]                                     # 16-byte aligned
    wu = wa[1:]                                                            # and not
    assert wa.ctypes.data % 16 == 0 and wu.ctypes.data % 16 == 8
    pk = lambda n=16, a=m, b=m, Lb=1.0, nk=8, p=0, wk=wa, out=o[0]: L.bfgx_power_spectrum_2d_device(                       # noqa: E731
        0, None, n, _ptr(a), _ptr(b), Lb, nk, p, _ptr(wk), _ptr(out), _ptr(o[1]), _ptr(o[2]), _ptr(o[3]), _ptr(cnt))
    flt = lambda n=16, a=m, Lb=1.0, kind=0, par=1.0, tk=None, tb=None, wk=wa, out=o[0]: L.bfgx_filter_map_2d_device(       # noqa: E731
        0, None, n, _ptr(a), Lb, kind, par, _ptr(tk), _ptr(tb), 0 if tk is None else tk.size, _ptr(wk), _ptr(out))
    up, down = np.array([0.0, 1.0, 2.0]), np.array([0.0, 2.0, 1.0])
    cases = [
        (lambda: L.bfgx_rfft2_device(0, None, 16, None, _ptr(wa), _ptr(o[0])), _lib.ERR_INVALID, b'NULL'),
        (lambda: L.bfgx_rfft2_device(0, None, 16, _ptr(m), None, _ptr(o[0])), _lib.ERR_INVALID, b'NULL'),
        (lambda: L.bfgx_rfft2_device(0, None, 16, _ptr(m), _ptr(wa), None), _lib.ERR_INVALID, b'NULL'),
        (lambda: L.bfgx_rfft2_device(0, None, 12, _ptr(m), _ptr(wa), _ptr(o[0])), _lib.ERR_UNSUPPORTED, b'8 <= n <= 4096'),
        (lambda: L.bfgx_rfft2_device(0, None, 4, _ptr(m), _ptr(wa), _ptr(o[0])), _lib.ERR_UNSUPPORTED, b'8 <= n <= 4096'),
        (lambda: L.bfgx_rfft2_device(0, None, 8192, _ptr(m), _ptr(wa), _ptr(o[0])), _lib.ERR_UNSUPPORTED, b'8 <= n <= 4096'),
        (lambda: L.bfgx_rfft2_device(0, None, 16, _ptr(m), _ptr(wu), _ptr(o[0])), _lib.ERR_INVALID, b'16-byte'),
        (lambda: L.bfgx_irfft2_device(0, None, 16, None, 1.0, _ptr(wa), _ptr(o[0])), _lib.ERR_INVALID, b'NULL'),
        (lambda: L.bfgx_irfft2_device(0, None, 24, _ptr(wa), 1.0, _ptr(wa), _ptr(o[0])), _lib.ERR_UNSUPPORTED, b'8 <= n <= 4096'),
        (lambda: L.bfgx_irfft2_device(0, None, 16, _ptr(wa), 1.0, _ptr(wu), _ptr(o[0])), _lib.ERR_INVALID, b'16-byte'),
        (lambda: L.bfgx_irfft2_device(0, None, 16, _ptr(wu), 1.0, _ptr(wa), _ptr(o[0])), _lib.ERR_INVALID, b'16-byte'),
        (lambda: pk(a=None), _lib.ERR_INVALID, b'NULL'), (lambda: pk(b=None), _lib.ERR_INVALID, b'NULL'),
        (lambda: pk(wk=None), _lib.ERR_INVALID, b'NULL'), (lambda: pk(out=None), _lib.ERR_INVALID, b'NULL'),
        (lambda: pk(n=48), _lib.ERR_UNSUPPORTED, b'8 <= n <= 4096'),
        (lambda: pk(nk=0), _lib.ERR_INVALID, b'1 <= nk <= 2048'), (lambda: pk(nk=2049), _lib.ERR_INVALID, b'1 <= nk <= 2048'),
        (lambda: pk(Lb=0.0), _lib.ERR_INVALID, b'L > 0'), (lambda: pk(Lb=float('nan')), _lib.ERR_INVALID, b'L > 0'),
        (lambda: pk(p=4), _lib.ERR_INVALID, b'window_order'), (lambda: pk(p=-1), _lib.ERR_INVALID, b'window_order'),
        (lambda: pk(wk=wu), _lib.ERR_INVALID, b'16-byte'),
        (lambda: flt(a=None), _lib.ERR_INVALID, b'NULL'), (lambda: flt(out=None), _lib.ERR_INVALID, b'NULL'),
        (lambda: flt(n=17), _lib.ERR_UNSUPPORTED, b'8 <= n <= 4096'),
        (lambda: flt(Lb=-1.0), _lib.ERR_INVALID, b'L > 0'),
        (lambda: flt(par=-1.0), _lib.ERR_INVALID, b'width >= 0'), (lambda: flt(kind=1, par=-0.1), _lib.ERR_INVALID, b'width >= 0'),
        (lambda: flt(kind=3), _lib.ERR_INVALID, b'kind'),
        (lambda: flt(kind=2), _lib.ERR_INVALID, b'NULL'),
        (lambda: flt(kind=2, tk=down, tb=up), _lib.ERR_INVALID, b'ascending'),
        (lambda: flt(kind=2, tk=np.array([0.0, 0.0]), tb=np.array([1.0, 1.0])), _lib.ERR_INVALID, b'ascending'),
        (lambda: flt(wk=wu), _lib.ERR_INVALID, b'16-byte'),
        (lambda: L.bfgx_kappa_to_shear_2d_device(0, None, 16, None, _ptr(wa), _ptr(o[0]), _ptr(o[1])), _lib.ERR_INVALID, b'NULL'),
        (lambda: L.bfgx_kappa_to_shear_2d_device(0, None, 16, _ptr(m), _ptr(wa), _ptr(o[0]), None), _lib.ERR_INVALID, b'NULL'),
        (lambda: L.bfgx_kappa_to_shear_2d_device(0, None, 6, _ptr(m), _ptr(wa), _ptr(o[0]), _ptr(o[1])), _lib.ERR_UNSUPPORTED, b'8 <= n <= 4096'),
        (lambda: L.bfgx_kappa_to_shear_2d_device(0, None, 16, _ptr(m), _ptr(wu), _ptr(o[0]), _ptr(o[1])), _lib.ERR_INVALID, b'16-byte'),
        (lambda: L.bfgx_shear_to_kappa_2d_device(0, None, 16, _ptr(m), None, _ptr(wa), _ptr(o[0]), _ptr(o[1])), _lib.ERR_INVALID, b'NULL'),
        (lambda: L.bfgx_shear_to_kappa_2d_device(0, None, 2048 + 1024, _ptr(m), _ptr(m), _ptr(wa), _ptr(o[0]), _ptr(o[1])), _lib.ERR_UNSUPPORTED, b'8 <= n'),
        (lambda: L.bfgx_shear_to_kappa_2d_device(0, None, 16, _ptr(m), _ptr(m), _ptr(wu), _ptr(o[0]), _ptr(o[1])), _lib.ERR_INVALID, b'16-byte'),
        # the host entries: the same checks, before the device is asked for
        (lambda: L.bfgx_power_spectrum_2d(0, 16, None, _ptr(m), 1.0, 8, 0, _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), _ptr(o[3]), _ptr(cnt)), _lib.ERR_INVALID, b'NULL'),
        (lambda: L.bfgx_power_spectrum_2d(0, 20, _ptr(m), _ptr(m), 1.0, 8, 0, _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), _ptr(o[3]), _ptr(cnt)), _lib.ERR_UNSUPPORTED, b'8 <= n'),
        (lambda: L.bfgx_power_spectrum_2d(0, 16, _ptr(m), _ptr(m), 1.0, 0, 0, _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), _ptr(o[3]), _ptr(cnt)), _lib.ERR_INVALID, b'nk'),
        (lambda: L.bfgx_filter_map_2d(0, 16, _ptr(m), 1.0, 0, -1.0, None, None, 0, _ptr(o[0])), _lib.ERR_INVALID, b'width >= 0'),
        (lambda: L.bfgx_filter_map_2d(0, 16, _ptr(m), 1.0, 2, 0.0, _ptr(down), _ptr(up), 3, _ptr(o[0])), _lib.ERR_INVALID, b'ascending'),
        (lambda: L.bfgx_kappa_to_shear_2d(0, 10, _ptr(m), _ptr(o[0]), _ptr(o[1])), _lib.ERR_UNSUPPORTED, b'8 <= n'),
        (lambda: L.bfgx_shear_to_kappa_2d(0, 16, _ptr(m), None, _ptr(o[0]), _ptr(o[1])), _lib.ERR_INVALID, b'NULL'),
    ]
    for i, (call, rc, word) in enumerate(cases):
        assert call() == rc, i
        assert word in L.bfgx_last_error(), (i, L.bfgx_last_error())
