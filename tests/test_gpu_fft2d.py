"""The 2-D FFT kernels of csrc/bfgx_fft2d.hpp and the functions of utils/flatsky.py against tests/fft2d_oracle.py (plain numpy on the full
plane) at N = 8, 16, 64, 1024 (the last size of the strided column pass), 2048 (the first of the split one, 64 x 32) and 4096 (64 x 64).

  1. rfft2: noise, impulses, plane waves; work and output start as NaN
  2. irfft2: round trips, single modes -> cosine planes; the output starts as NaN
  3. binning: the shapes whose modes sit on bin edges (test_fft2d_host.py), one-hot spectra, a map with itself, windows
  4. filters: Gaussian, top hat, table
  5. Kaiser-Squires: both directions, the Nyquist rows and columns, the Gaussian bump through MeasureProfilesGrid
  6. cached setups in the orders large, small, large; residency of the results

Bounds (fft2d_oracle.bound / chain_bound): max|got - ref| / max|ref| <= 16 x numpy's own error against long double, see the oracle file.

Measured on the MI355X, max|got - ref| / max|ref| (worst over the cases of a test):
  N                          8        16       64       1024     2048     4096
  bound                      1.8e-15  4.2e-15  4.5e-15  5.3e-15  6.4e-15  4.8e-15
  rfft2 noise                1.5e-16  2.2e-16  2.9e-16  4.9e-16  5.6e-16  5.1e-16
  rfft2 impulses             2.3e-16  2.7e-16  3.4e-16  7.8e-16  7.1e-16  8.2e-16
  rfft2 plane waves          1.1e-16  1.1e-16  1.1e-16  5.6e-17  7.9e-17  8.8e-17
  chain bound                3.7e-15  4.5e-15  5.6e-15  7.0e-15  7.7e-15  8.4e-15
  irfft2(rfft2)              1.7e-16  3.4e-16  2.8e-16  5.1e-16  5.1e-16  5.6e-16
  irfft2 single modes        1.1e-16  2.2e-16  4.4e-16  7.8e-16  1.0e-15  1.1e-15
  Kaiser-Squires, forward    2.0e-16           4.6e-16           5.7e-16  7.3e-16
  Kaiser-Squires, to E / B   2.8e-16           3.9e-16           5.4e-16  6.3e-16
  filters (worst of 8)                3.7e-16           1.4e-15  1.7e-15           (the worst is the top hat of N/8 pixels)
The bump through MeasureProfilesGrid on the device: mean_t within 1.7e-16 and mean_x within 1.3e-17 of the CPU chain (allowed 2.9e-12).
Binned sums, one-hot spectra and the bitwise repeats pass as asserted.  The file takes 33 s, 12 of them the first call's start-up of the
runtime; the slowest case after that is Kaiser-Squires at 4096 (4.5 s, nearly all of it the oracle's four full-plane numpy transforms).
"""
import functools

import numpy as np
import pytest

import fft_oracle as O
import fft2d_oracle as F
import gridprofiles_oracle as K

pytestmark = pytest.mark.gpu

SIZES = (8, 16, 64, 1024, 2048, 4096)


@pytest.fixture(scope='module', autouse=True)
def _release_the_setups():
    """the twiddles and window tables of this file are handed back when it is done"""
    yield
    import torch
    from baryonification_amd import _lib
    torch.cuda.synchronize()
    _lib.load().bfgx_cache_clear()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


def _rel(got, ref):
    """max|got - ref| / max|ref| (long double up to N = 256, double above: the differences of close doubles are exact enough)"""
    if np.asarray(ref).size <= 256 * 256:
        return O.rel_err(got, ref)
    return float(np.abs(np.asarray(got) - np.asarray(ref)).max() / np.abs(ref).max())


@functools.lru_cache(maxsize=None)
def _circle(N):
    """cos and sin of 2 pi m / N, m < N, from long double"""
    ang = 8 * np.arctan(np.longdouble(1)) * np.arange(N).astype(np.longdouble) / N
    return np.cos(ang).astype(np.float64), np.sin(ang).astype(np.float64)


def _wave(N, p, q):
    """fft_oracle.plane_wave by table look-up (the same values: the argument is reduced as an integer first)"""
    i = np.arange(N, dtype=np.int64)
    return _circle(N)[0][(p * i[:, None] + q * i[None, :]) % N]


def _impulse_ref(N, i0, j0):
    """fft_oracle.impulse_ref by table look-up"""
    m = (i0 * np.arange(N, dtype=np.int64)[:, None] + j0 * np.arange(N // 2 + 1, dtype=np.int64)[None, :]) % N
    c, s = _circle(N)
    return c[m] - 1j * s[m]


def test_the_fast_references_are_the_oracles(gpu):
    for N in (8, 64):
        assert np.array_equal(_wave(N, N - 1, 3), O.plane_wave(N, N - 1, 3))
        assert np.array_equal(_impulse_ref(N, N - 1, 37 % N), O.impulse_ref(N, N - 1, 37 % N).astype(np.complex128))


def _rfft2(x, fill=float('nan')):
    """engine.rfft2_device on a real plane -> complex [N][pitch]; work and output pre-filled with `fill`"""
    import torch
    from baryonification_amd import engine
    N = x.shape[0]
    pitch = engine.fft_pitch(N)
    d = _dev(x)
    work = torch.full((engine.fft2_work_doubles(N),), fill, dtype=torch.float64, device='cuda:0')
    out = torch.full((N, pitch, 2), fill, dtype=torch.float64, device='cuda:0')
    engine.rfft2_device(d.data_ptr(), N, work.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.complex128)[..., 0]


def _irfft2(spec, scale, fill=float('nan'), pad=float('nan')):
    """engine.irfft2_device on complex [N][N/2 + 1] -> real [N][N]; pad columns hold `pad`, work and output start as `fill`"""
    import torch
    from baryonification_amd import engine
    N = spec.shape[0]
    pitch = engine.fft_pitch(N)
    padded = np.full((N, pitch), complex(pad, pad), dtype=np.complex128)
    padded[:, :N // 2 + 1] = spec
    d = _dev(padded.view(np.float64))
    work = torch.full((engine.fft2_work_doubles(N),), fill, dtype=torch.float64, device='cuda:0')
    out = torch.full((N, N), fill, dtype=torch.float64, device='cuda:0')
    engine.irfft2_device(d.data_ptr(), N, scale, work.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _half_ref(x):
    N = x.shape[0]
    if N <= 64:
        return F.fft2_ld(x)[:, :N // 2 + 1]
    return np.fft.fft(np.fft.rfft(x, axis=1), axis=0)


WAVES = lambda N: [(0, 0), (1, 0), (0, 1), (N // 2, 0), (0, N // 2), (N // 2, N // 2), (N - 1, 3), (37 % N, N // 2 - 1)]      # noqa: E731


# ------------------------------------------------------------------------------------------------- 1. rfft2
@pytest.mark.parametrize('N', SIZES)
def test_rfft2_noise(gpu, N):
    x = F.noise(N)
    got = _rfft2(x)[:, :N // 2 + 1]
    assert np.isfinite(got.view(np.float64)).all()
    err = _rel(got, _half_ref(x))
    print("rfft2 noise N = %4d: %.2e (bound %.2e)" % (N, err, F.bound(N)))
    assert err <= F.bound(N)
    # bitwise what a zero-filled work and output give: nothing of the pad columns reaches a coefficient
    again = _rfft2(x, 0.0)[:, :N // 2 + 1]
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(again).view(np.uint64))


@pytest.mark.parametrize('N', SIZES)
def test_rfft2_impulses(gpu, N):
    worst = 0.0
    for i0, j0 in [(0, 0), (1, 0), (0, 1), (N // 2, N // 2), (N - 1, 37 % N)]:
        x = np.zeros((N, N))
        x[i0, j0] = 1.0
        got = _rfft2(x)[:, :N // 2 + 1]
        assert np.isfinite(got.view(np.float64)).all()
        worst = max(worst, _rel(got, O.impulse_ref(N, i0, j0) if N <= 64 else _impulse_ref(N, i0, j0)))
    print("rfft2 impulses N = %4d: %.2e (bound %.2e)" % (N, worst, F.bound(N)))
    assert worst <= F.bound(N)


@pytest.mark.parametrize('N', SIZES)
def test_rfft2_plane_waves(gpu, N):
    worst = 0.0
    for p, q in WAVES(N):
        got = _rfft2(_wave(N, p, q))[:, :N // 2 + 1]
        assert np.isfinite(got.view(np.float64)).all()
        worst = max(worst, _rel(got, O.plane_wave_ref(N, p, q)))
    print("rfft2 plane waves N = %4d: %.2e (bound %.2e)" % (N, worst, F.bound(N)))
    assert worst <= F.bound(N)


# ------------------------------------------------------------------------------------------------- 2. irfft2
@pytest.mark.parametrize('N', SIZES)
def test_irfft2_inverts_rfft2(gpu, N):
    x = F.noise(N, 2)
    spec = _rfft2(x)[:, :N // 2 + 1]
    back = _irfft2(spec, 1.0 / (float(N) * N))
    assert np.isfinite(back).all()
    err = _rel(back, x)
    print("irfft2(rfft2) N = %4d: %.2e (bound %.2e)" % (N, err, F.chain_bound(N)))
    assert err <= F.chain_bound(N)
    # the public pair, numpy in and out
    from baryonification_amd import utils as U
    if N <= 1024:
        s = U.rfft2(x)
        assert isinstance(s, np.ndarray) and s.shape == (N, N // 2 + 1) and s.dtype == np.complex128
        assert np.array_equal(s, spec)
        assert np.array_equal(U.irfft2(s, N), _irfft2(spec, 1.0 / (float(N) * N), 0.0, 0.0))


@pytest.mark.parametrize('N', SIZES)
def test_irfft2_single_modes_are_cosine_planes(gpu, N):
    """the half spectrum of a plane wave (one mode, and its mirror in the self-conjugate columns) -> the wave"""
    worst = 0.0
    for p, q in WAVES(N):
        back = _irfft2(O.plane_wave_ref(N, p, q).astype(np.complex128), 1.0 / (float(N) * N))
        assert np.isfinite(back).all()
        worst = max(worst, _rel(back, _wave(N, p, q)))
    print("irfft2 single modes N = %4d: %.2e (bound %.2e)" % (N, worst, F.chain_bound(N)))
    assert worst <= F.chain_bound(N)


def test_irfft2_ignores_what_breaks_hermitian_symmetry(gpu):
    """imaginary parts in the columns 0 and N/2 that a real field cannot have do not reach the map"""
    N = 16
    x = F.noise(N, 3)
    spec = np.fft.fft(np.fft.rfft(x, axis=1), axis=0)
    ref = _irfft2(spec, 1.0 / (N * N))
    dirty = spec.copy()
    dirty[0, 0] += 5j
    dirty[N // 2, N // 2] -= 3j
    dirty[3, 0] += 2j
    dirty[N - 3, 0] += 2j                                              # (a Hermitian pair would have -2j here)
    assert _rel(_irfft2(dirty, 1.0 / (N * N)), ref) <= F.chain_bound(N)


# ------------------------------------------------------------------------------------------------- 3. binning
def _poisson_map(N, seed):
    rng = np.random.default_rng(seed)
    m = rng.poisson(3.0, (N, N)).astype(np.float64)
    m[rng.integers(N), rng.integers(N)] += 1000.0                      # one bright pixel: power in every mode
    return m


def _check_spectra(got, ref, keys):
    assert got['counts'].dtype == np.int64 and np.array_equal(got['counts'], ref['counts'])
    good = ref['counts'] > 0
    assert good.any()
    assert np.all(np.abs(got['k'][good] - ref['k'][good]) <= 1e-12 * ref['k'][good])
    for key in keys:
        assert np.all(np.isnan(got[key][~good])) and np.all(np.isfinite(got[key][good])), key
        scale = np.maximum(np.abs(ref[key][good]), 1e-10 * np.abs(ref[key][good]).max() if key in ('pab', 'r') else 0.0)
        assert np.all(np.abs(got[key][good] - ref[key][good]) <= 1e-10 * scale), key
    assert np.all(np.isnan(got['k'][~good]))
    return good


@pytest.mark.parametrize('N,Nk,L', [(32, 15, 305.0), (64, 31, 1.0), (64, 62, 1000.0 / 3.0), (128, 63, 2 * np.pi), (16, 1, 305.0), (16, 2, 305.0),
                                    (64, 2048, 305.0), (2048, 180, 305.0)])
def test_power_spectrum_bin_edges(gpu, N, Nk, L):
    from baryonification_amd import utils as U
    m = _poisson_map(N, 50 + N + Nk)
    ref = F.cross_power_spectrum_ref(m, m, L, Nk)
    got = U.power_spectrum_2d(m, L, Nk)
    assert set(got) == {'k', 'pk', 'counts'}
    _check_spectra(dict(got, paa=got['pk']), ref, ('paa',))
    if N <= 64:
        norm = U.power_spectrum_2d(m, L, Nk, normalize=True)
        good = ref['counts'] > 0
        assert np.allclose(norm['pk'][good], got['pk'][good] * (L * L / float(N) ** 4), rtol=1e-15, atol=0)


@pytest.mark.parametrize('N', [8, 64, 2048])
def test_one_hot_spectra_land_in_their_bin(gpu, N):
    """a spectrum that is 1 at one mode (a, c) of the half plane goes through irfft2_device (scale 1) and the map through
    power_spectrum_2d_device: for 0 < c < N/2 the map is 2 cos and the forward transform has N^2 at (a, c); in the columns 0 and N/2 the
    inverse keeps the Hermitian part, N^2 / 2 at (a, c) and at (-a, c), which share |k|, the window weight and so the bin"""
    import torch
    from baryonification_amd import engine
    L, nk = O.ONE_HOT_L, 31
    pitch, h = engine.fft_pitch(N), N // 2
    modes = sorted({(a, c) for a, _, c in O.one_hot_modes(N)})
    work = torch.empty(engine.fft2_work_doubles(N), dtype=torch.float64, device='cuda:0')
    spec = torch.zeros((N, pitch, 2), dtype=torch.float64, device='cuda:0')
    m = torch.full((N, N), float('nan'), dtype=torch.float64, device='cuda:0')
    sums = torch.empty((4, nk), dtype=torch.float64, device='cuda:0')
    cnt = torch.empty(nk, dtype=torch.int64, device='cuda:0')
    all_counts = F.cross_power_spectrum_ref(np.ones((N, N)), np.ones((N, N)), L, nk)['counts']
    for p in (0, 2):
        for a, c in modes:
            spec.zero_()
            spec[a, c, 0] = 1.0
            engine.irfft2_device(spec.data_ptr(), N, 1.0, work.data_ptr(), m.data_ptr())
            engine.power_spectrum_2d_device(m.data_ptr(), m.data_ptr(), N, L, nk, p, work.data_ptr(), sums[0].data_ptr(), sums[1].data_ptr(),
                                            sums[2].data_ptr(), sums[3].data_ptr(), cnt.data_ptr())
            s, n = sums.cpu().numpy(), cnt.cpu().numpy()
            assert np.array_equal(n, all_counts)
            b, w, _, mult = F.one_hot_ref(N, L, nk, a, c, p)
            self_conj = c in (0, h) and a in (0, h)
            power = float(N) ** 4 * (w if (0 < c < h or self_conj) else 0.5 * w)          # (w carries the mirror weight)
            rest = np.ones(nk, dtype=bool)
            if b is not None:
                rest[b] = False
                for row in s[:3]:
                    assert abs(row[b] - power) <= 1e-12 * power, (N, a, c, p)
            assert np.all(np.abs(s[:3][:, rest]) <= 1e-24 * float(N) ** 4), (N, a, c, p)


@pytest.mark.parametrize('N,Nk,L', [(64, 31, 305.0), (1024, 180, 700.0)])
def test_cross_spectrum_of_a_map_with_itself(gpu, N, Nk, L):
    from baryonification_amd import utils as U
    m = _poisson_map(N, 60 + N)
    x = U.cross_power_spectrum_2d(m, m, L, Nk)
    assert set(x) == {'k', 'paa', 'pbb', 'pab', 'r', 'counts'}
    good = _check_spectra(x, F.cross_power_spectrum_ref(m, m, L, Nk), ('paa', 'pbb', 'pab', 'r'))
    assert np.all(np.abs(x['pab'][good] - x['paa'][good]) <= 1e-14 * x['paa'][good])
    assert np.all(np.abs(x['r'][good] - 1) <= 1e-12)
    # two copies of the map at different addresses take the two-spectra path
    y = U.cross_power_spectrum_2d(m, m.copy(), L, Nk)
    assert np.all(np.abs(y['pab'][good] - y['paa'][good]) <= 1e-14 * y['paa'][good]) and np.all(np.abs(y['r'][good] - 1) <= 1e-12)


@pytest.mark.parametrize('window,p', [('cic', 2), ('tsc', 3)])
@pytest.mark.parametrize('N,Nk,L', [(16, 7, 305.0), (64, 31, 1000.0 / 3.0), (2048, 180, 305.0)])
def test_cross_spectrum_of_two_maps_with_a_window(gpu, N, Nk, L, window, p):
    from baryonification_amd import utils as U
    A, B = _poisson_map(N, 70 + N), _poisson_map(N, 71 + N) + 0.5 * _poisson_map(N, 70 + N)
    ref = F.cross_power_spectrum_ref(A, B, L, Nk, p)
    got = U.cross_power_spectrum_2d(A, B, L, Nk, window=window)
    good = _check_spectra(got, ref, ('paa', 'pbb', 'pab', 'r'))
    plain = U.cross_power_spectrum_2d(A, B, L, Nk)
    assert np.all(got['paa'][good] >= plain['paa'][good])             # every weight is >= 1
    assert np.array_equal(U.cross_power_spectrum_2d(A, B, L, Nk, window=p)['counts'], got['counts'])
    if N == 64:
        on_dev = U.cross_power_spectrum_2d(_dev(A), _dev(B), L, Nk, window=window, normalize=True)
        _check_spectra(on_dev, F.cross_power_spectrum_ref(A, B, L, Nk, p, normalize=True), ('paa', 'pbb', 'pab', 'r'))


# ------------------------------------------------------------------------------------------------- 4. filters
@pytest.mark.parametrize('N', [16, 1024, 2048])
def test_filters(gpu, N):
    from baryonification_amd import utils as U
    L = 0.7 * N
    res = L / N
    x = F.noise(N, 4)
    kmax = F.k_plane(N, L).max()
    worst = 0.0
    for width in (1.5 * res, N / 8 * res):
        tk = np.linspace(0.0, 0.8 * kmax, 33)                          # (the corner modes lie beyond the table: held at its end value)
        tb = 1.0 / (1.0 + (tk * width) ** 2)
        cases = [(dict(sigma=width), lambda k: F.beam_gauss(k, width)),
                 (dict(fwhm=width * np.sqrt(8 * np.log(2))), lambda k: F.beam_gauss(k, width)),
                 (dict(tophat=width), lambda k: F.beam_tophat(k, width)),
                 (dict(beam=(tk, tb)), lambda k: F.beam_table(k, tk, tb))]
        for kw, beam in cases:
            ref = F.smoothing_ref(x, L, beam)
            got = U.smoothing_2d(x, L, **kw)
            assert isinstance(got, np.ndarray) and got.shape == (N, N)
            err = _rel(got, ref)
            print("filter N = %4d width %.3g %s: %.2e (bound %.2e)" % (N, width / res, sorted(kw)[0], err, F.chain_bound(N)))
            worst = max(worst, err)
    assert worst <= F.chain_bound(N)
    same = U.smoothing_2d(x, L, fwhm=0)
    assert _rel(same, x) <= F.chain_bound(N)
    t = U.smoothing_2d(_dev(x), L, tophat=1.5 * res)
    assert t.is_cuda and _rel(t.cpu().numpy(), F.smoothing_ref(x, L, lambda k: F.beam_tophat(k, 1.5 * res))) <= F.chain_bound(N)


# ------------------------------------------------------------------------------------------------- 5. Kaiser-Squires
@pytest.mark.parametrize('N', [8, 64, 2048, 4096])
def test_kaiser_squires_both_directions(gpu, N):
    from baryonification_amd import utils as U
    kappa, g2in = F.noise(N, 5), F.noise(N, 6)
    tk, t2 = _dev(kappa), _dev(g2in)
    g1, g2 = U.kappa_to_shear_2d(tk)
    assert g1.is_cuda and g2.is_cuda and g1.shape == (N, N)
    r1, r2 = F.kappa_to_shear(kappa)
    scale = max(np.abs(r1).max(), np.abs(r2).max())
    e_fwd = max(np.abs(g1.cpu().numpy() - r1).max(), np.abs(g2.cpu().numpy() - r2).max()) / scale
    ke, kb = U.shear_to_kappa_2d(tk, t2)
    re, rb = F.shear_to_kappa(kappa, g2in)
    scale = max(np.abs(re).max(), np.abs(rb).max())
    e_back = max(np.abs(ke.cpu().numpy() - re).max(), np.abs(kb.cpu().numpy() - rb).max()) / scale
    print("Kaiser-Squires N = %4d: kappa -> shear %.2e, shear -> E/B %.2e (bound %.2e)" % (N, e_fwd, e_back, F.chain_bound(N)))
    assert e_fwd <= F.chain_bound(N) and e_back <= F.chain_bound(N)
    if N <= 64:                                                         # numpy in, numpy out, the same numbers
        h1, h2 = U.kappa_to_shear_2d(kappa)
        assert isinstance(h1, np.ndarray) and np.array_equal(h1, g1.cpu().numpy()) and np.array_equal(h2, g2.cpu().numpy())
        he, hb = U.shear_to_kappa_2d(kappa, g2in)
        assert np.array_equal(he, ke.cpu().numpy()) and np.array_equal(hb, kb.cpu().numpy())


@pytest.mark.parametrize('N', [8, 64, 2048])
def test_kaiser_squires_nyquist_rows_and_columns(gpu, N):
    """a map that is one plane wave with a Nyquist index: s2 = 0 there, c2 from the squares alone"""
    from baryonification_amd import utils as U
    h = N // 2
    for p, q in [(h, 0), (0, h), (h, h), (h, 3), (3, h), (h, h - 1)]:
        kappa = _wave(N, p, q)
        n0 = p if p < h else p - N
        c2 = (n0 * n0 - q * q) / float(n0 * n0 + q * q)
        g1, g2 = U.kappa_to_shear_2d(kappa)
        assert np.abs(g1 - c2 * kappa).max() <= F.chain_bound(N), (p, q)
        assert np.abs(g2).max() <= F.chain_bound(N), (p, q)
        ke, kb = U.shear_to_kappa_2d(kappa, kappa)                       # kE = c2 kappa, kB = c2 kappa where s2 = 0
        assert np.abs(ke - c2 * kappa).max() <= F.chain_bound(N) and np.abs(kb - c2 * kappa).max() <= F.chain_bound(N), (p, q)


def test_gaussian_bump_through_measure_profiles_grid(gpu):
    """the chain of the README on the device: kappa -> (g1, g2) -> gamma_t, against the same chain on the CPU (the oracle's Kaiser-Squires
    and gridprofiles_oracle); gamma_t > 0 around the peak"""
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    from oracle import grid as G
    b = F.BUMP
    bins, kappa, _ = F.bump_maps()
    cat = F.bump_catalog(bins)
    HCat = bfg.utils.HaloNDCatalog(x=cat['x'], y=cat['y'], z=None, M=cat['M'], redshift=b['redshift'], cosmo=dict(syn.COSMO))
    Map = bfg.utils.GriddedMap(map=kappa, redshift=b['redshift'], bins=bins, cosmo=dict(syn.COSMO))
    used = {k: np.array(HCat.cat[k], dtype=np.float64) for k in ('M', 'x', 'y', 'z')}
    assert used['x'][0] == cat['x'][0] and used['y'][0] == cat['y'][0]
    pairs = K.pairs(bins, 2, used, b['redshift'], b['eps'], G.grid_background(syn.COSMO))
    o = K.measure(pairs, b['edges'], kappa, shear=F.kappa_to_shear(kappa))
    tk = _dev(kappa)
    g1, g2 = bfg.utils.kappa_to_shear_2d(tk)
    res = bfg.Runners.MeasureProfilesGrid(HCat, Map, b['eps'], verbose=False, r_edges=b['edges']).process(map=tk, shear=(g1, g2))
    n = o['npix_shear'][0]
    assert np.array_equal(res.npix_shear.cpu().numpy()[0], n) and np.all(n[1:] > 0)
    ref_t, ref_x = o['sum_t'][0][1:] / n[1:], o['sum_x'][0][1:] / n[1:]
    st = res.stack()
    mean_t, mean_x = st['mean_t'].cpu().numpy()[1:], st['mean_x'].cpu().numpy()[1:]
    tol = 1e-11 * np.abs(ref_t).max()
    print("bump on the device: max|mean_t - cpu| %.2e, max|mean_x - cpu| %.2e (allowed %.2e)" % (np.abs(mean_t - ref_t).max(), np.abs(mean_x - ref_x).max(), tol))
    assert np.all(mean_t > 0)
    assert np.abs(mean_t - ref_t).max() <= tol and np.abs(mean_x - ref_x).max() <= tol


# ------------------------------------------------------------------------------------------------- 6. cache and residency
@pytest.mark.parametrize('order', [(4096, 8, 4096), (2048, 1024, 2048)])
def test_cached_setups_large_small_large(gpu, order):
    """every instantiation has the dynamic LDS of its largest N: a cached large setup launches after a small one ran; the transforms use no
    atomics, so every call repeats bitwise"""
    import torch
    from baryonification_amd import utils as U
    first = {}
    for N in order:
        x = _dev(F.noise(N, 7))
        for _ in range(2):
            spec = U.rfft2(x)
            back = U.irfft2(spec, N)
            g1, g2 = U.kappa_to_shear_2d(x)
            torch.cuda.synchronize()
            assert spec.is_cuda and spec.device == x.device and back.device == x.device and g1.device == x.device
            from baryonification_amd import engine
            got = (spec[:, :N // 2 + 1].cpu().numpy(), back.cpu().numpy(), g1.cpu().numpy(), g2.cpu().numpy())
            assert spec.shape == (N, engine.fft_pitch(N), 2)
            if N not in first:
                first[N] = got
                assert _rel(got[1], x.cpu().numpy()) <= F.chain_bound(N)
            for a, b in zip(got, first[N]):
                assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), N


def test_residency(gpu):
    import torch
    from baryonification_amd import utils as U
    x = F.noise(64, 8)
    t = _dev(x)
    assert isinstance(U.rfft2(x), np.ndarray) and isinstance(U.irfft2(U.rfft2(x), 64), np.ndarray)
    assert isinstance(U.smoothing_2d(x, 10.0, sigma=1.0), np.ndarray) and isinstance(U.shear_to_kappa_2d(x, x)[1], np.ndarray)
    for out in (U.rfft2(t), U.irfft2(U.rfft2(t), 64), U.smoothing_2d(t, 10.0, sigma=1.0), *U.kappa_to_shear_2d(t), *U.shear_to_kappa_2d(t, t)):
        assert isinstance(out, torch.Tensor) and out.device == t.device and out.dtype == torch.float64
    p = U.power_spectrum_2d(t, 10.0, 20)
    assert all(isinstance(v, np.ndarray) for v in p.values())
    assert np.array_equal(p['counts'], U.power_spectrum_2d(x, 10.0, 20)['counts'])
    # a non-contiguous view is made contiguous; the spectrum of the transpose is the transposed spectrum's
    assert _rel(U.irfft2(U.rfft2(t.t()), 64).cpu().numpy(), x.T) <= F.chain_bound(64)
    # GriddedMap.power_spectrum: L = Npix res
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    Map = bfg.utils.GriddedMap(map=x, redshift=0.2, bins=(np.arange(64) + 0.5) * 0.25, cosmo=dict(syn.COSMO))
    a, b = Map.power_spectrum(Nk=20), U.power_spectrum_2d(x, 16.0, 20)
    assert np.array_equal(a['counts'], b['counts']) and np.allclose(a['pk'], b['pk'], rtol=1e-12, equal_nan=True)
    cube = np.random.default_rng(9).standard_normal((16, 16, 16))
    Map3 = bfg.utils.GriddedMap(map=cube, redshift=0.2, bins=(np.arange(16) + 0.5) * 2.0, cosmo=dict(syn.COSMO))
    from baryonification_amd import engine
    c3 = Map3.power_spectrum(Nk=6)
    kc, pk, cnt = engine.power_spectrum(cube, 32.0, 6)
    assert set(c3) == {'k', 'pk', 'counts'} and np.array_equal(c3['counts'], cnt) and np.allclose(c3['pk'], pk, rtol=1e-12, equal_nan=True)


def test_two_threads_filter_one_resident_map_with_their_own_tables(gpu):
    """the beam table of a call is uploaded from a copy of the call's own: two threads on one cached N = 64 setup, each four calls with
    a table of its own (16 and 33 nodes), get bit for bit what the same call gives alone"""
    import threading
    from baryonification_amd import utils as U
    N, L = 64, 45.0
    x = _dev(F.noise(N, 9))
    kmax = F.k_plane(N, L).max()
    beams = []
    for nodes, width in ((16, 1.1), (33, 3.7)):
        tk = np.linspace(0.0, 0.8 * kmax, nodes)
        beams.append((tk, 1.0 / (1.0 + (tk * width) ** 2)))
    alone = [U.smoothing_2d(x, L, beam=b).cpu().numpy() for b in beams]
    assert not np.array_equal(alone[0], alone[1])
    gate, got = threading.Barrier(2), [[], []]

    def calls(t):
        gate.wait()
        for _ in range(4):
            got[t].append(U.smoothing_2d(x, L, beam=beams[t]).cpu().numpy())

    threads = [threading.Thread(target=calls, args=(t,)) for t in range(2)]
    for th in threads: th.start()
    for th in threads: th.join()
    for t in range(2):
        assert len(got[t]) == 4
        for g in got[t]:
            assert np.array_equal(g.view(np.uint64), alone[t].view(np.uint64))
