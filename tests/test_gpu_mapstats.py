"""GPU harmonic filters, pixel neighbours, map moments, peak counts and shell_statistics (bfgx_sht_almxfl*, bfgx_hpx_neighbours*,
bfgx_mapstats_*; baryonification_amd.utils) against the numpy restatements of mapstats_oracle.py and sht_oracle.py.

Bounds.  Neighbours, almxfl, peak counts and flags, and the pixel count n of the moments: exact.  smoothing: 3e-11 of max|map|
(two transforms at the 1e-11 test_gpu_sht.py holds each to, plus the multiply).  Moments: 1e-11 x the mean absolute value of the
summed term: the fp64 sum tree gives about 3e-15 of it and the rounding of the mean, propagated at |mean| / std = 100, about 4e-13
on the odd moments; the bound is about 25x over that.  Measured on an MI355X: smoothing 7.3e-15 at the worst of these shapes;
central moments 2.7e-14 and means 1.4e-16 of the mean absolute term at |mean| / std = 100 (nside 16, 64 and 512, K = 3)."""
import numpy as np
import pytest

import hpx_oracle as H
import mapstats_oracle as M
import sht_oracle as O

pytestmark = pytest.mark.gpu

ARCMIN = np.pi / 180 / 60
UNSEEN = M.UNSEEN


# -------------------------------------------------------------------------------------------------------------- neighbours
@pytest.mark.parametrize('nside', [1, 2, 4, 8])
@pytest.mark.parametrize('nest', [False, True])
def test_neighbours_of_every_pixel(gpu, nside, nest):
    import torch
    from baryonification_amd import utils as U
    pix = np.arange(12 * nside * nside)
    ref = M.neighbours(nside, pix, nest)
    got = U.get_all_neighbours(nside, pix, nest=nest)
    assert got.dtype == np.int64 and got.shape == (8, pix.size) and np.array_equal(got, ref)
    dev = U.get_all_neighbours(nside, torch.from_numpy(pix).cuda(), nest=nest)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), ref)                   # the device entry agrees with the host entry
    one = U.get_all_neighbours(nside, 4, nest=nest)
    assert one.shape == (8,) and np.array_equal(one, ref[:, 4])
    if nside == 1 and not nest:
        assert one.tolist() == [11, 7, 3, -1, 0, 5, 8, -1]


def _sample(nside, rng):
    """pixels 0 and npix - 1, the two rings on both sides of each cap / belt boundary (nside 64), 10^4 random pixels"""
    npix, ncap = 12 * nside * nside, 2 * nside * (nside - 1)
    pix = [np.array([0, npix - 1]), rng.integers(0, npix, 10 ** 4)]
    if nside <= 64:
        north = np.arange(ncap - 4 * (nside - 1), ncap + 4 * nside)                # rings nside - 1 (cap) and nside (belt)
        pix += [north, npix - 1 - north]
    return np.unique(np.concatenate(pix))


@pytest.mark.parametrize('nside,nest', [(64, False), (64, True), (8192, False), (8192, True), (12, False)])
def test_neighbours_at_boundaries_and_random_pixels(gpu, nside, nest):
    import ctypes as C
    import torch
    from baryonification_amd import _lib, utils as U
    pix = _sample(nside, np.random.default_rng(nside))
    if nest:
        pix = np.unique(H.ring2nest(nside, pix))
    ref = M.neighbours(nside, pix, nest)
    assert np.array_equal(U.get_all_neighbours(nside, pix, nest=nest), ref)
    # the device entry: the same, and -1 for indices outside [0, npix)
    npix = 12 * nside * nside
    ip = torch.from_numpy(np.concatenate([pix, [-1, npix, npix + 7, -2 ** 40]])).cuda()
    out = torch.empty((8, ip.numel()), dtype=torch.int64, device='cuda')
    _lib.check(_lib.load().bfgx_hpx_neighbours_device(0, None, nside, int(nest), ip.numel(), C.c_void_p(ip.data_ptr()), C.c_void_p(out.data_ptr())))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert np.array_equal(out[:, :pix.size], ref) and (out[:, pix.size:] == -1).all()


# ------------------------------------------------------------------------------------------------------------------ almxfl
def _ell(lmax, mmax):
    return np.concatenate([np.arange(m, lmax + 1) for m in range(mmax + 1)])


@pytest.mark.parametrize('lmax,mmax', [(0, 0), (5, 3), (47, 47), (100, 80)])
def test_almxfl_equals_numpy_exactly(gpu, lmax, mmax):
    import torch
    from baryonification_amd import utils as U
    rng = np.random.default_rng(lmax)
    n = O.alm_size(lmax, mmax)
    alm = rng.normal(size=n) + 1j * rng.normal(size=n)
    ell = _ell(lmax, mmax)
    for nfl in sorted({1, lmax // 2 + 1, lmax + 1, lmax + 9}):
        fl = rng.normal(size=nfl)
        ref = alm * np.concatenate([fl, np.zeros(lmax + 9)])[ell]
        got = U.almxfl(alm, fl, mmax=mmax)
        assert got is not alm and got.dtype == np.complex128 and np.array_equal(got, ref), (lmax, mmax, nfl)
        a = alm.copy()
        assert U.almxfl(a, fl, mmax=mmax, inplace=True) is a and np.array_equal(a, ref)
        t = torch.from_numpy(alm).cuda()
        out = U.almxfl(t, fl, mmax=mmax)
        assert out.is_cuda and out.data_ptr() != t.data_ptr() and np.array_equal(out.cpu().numpy(), ref) and np.array_equal(t.cpu().numpy(), alm)
        assert U.almxfl(t, torch.from_numpy(fl).cuda(), mmax=mmax, inplace=True) is t and np.array_equal(t.cpu().numpy(), ref)
    assert np.array_equal(U.smoothalm(alm.copy(), beam_window=np.ones(lmax + 1), mmax=mmax), alm)
    if lmax == mmax:
        assert np.array_equal(U.smoothalm(alm.copy(), fwhm=0.3), alm * U.gauss_beam(0.3, lmax)[ell])


# --------------------------------------------------------------------------------------------------------------- smoothing
@pytest.mark.parametrize('nside', [8, 16])
def test_smoothing_matches_oracle(gpu, nside):
    import torch
    from baryonification_amd import utils as U
    rng = np.random.default_rng(nside)
    npix = 12 * nside * nside
    m = rng.normal(size=npix)
    bad = rng.random(npix) < 0.1
    m[bad] = UNSEEN
    fwhm, radius = 3.0 * np.sqrt(4 * np.pi / npix), 2.5 * np.sqrt(4 * np.pi / npix)
    sig = fwhm / np.sqrt(8 * np.log(2))
    for lmax in (nside, 3 * nside - 1):
        ell = _ell(lmax, lmax)
        for it in (0, 3):
            alm = O.map2alm(m, nside, lmax, lmax, it)                              # one analysis shared by the three filters
            for kw, fl in (({'fwhm': fwhm}, U.gauss_beam(fwhm, lmax)), ({'sigma': sig, 'fwhm': 9.9}, U.gauss_beam(fwhm, lmax)),
                           ({'beam_window': U.tophat_beam(radius, lmax), 'sigma': 9.9}, U.tophat_beam(radius, lmax))):
                ref = O.alm2map(alm * fl[ell], nside, lmax, lmax)
                got = U.smoothing(m, iter=it, lmax=lmax, **kw)
                assert got.dtype == np.float64 and (got[bad] == UNSEEN).all()
                err = np.abs(got - ref)[~bad].max() / np.abs(ref).max()
                assert err <= 3e-11, (nside, lmax, it, sorted(kw), err)
    t = torch.from_numpy(m).cuda()
    out = U.smoothing(t, fwhm=fwhm, iter=3)
    assert out.is_cuda and np.array_equal(out.cpu().numpy(), U.smoothing(m, fwhm=fwhm, iter=3)) and np.array_equal(t.cpu().numpy(), m)


# ----------------------------------------------------------------------------------------------------------------- moments
def _check_moments(got, maps, order, mask):
    n, mean, central, scale = M.moments(maps, order, mask)
    assert got['n'] == n and isinstance(got['n'], int)
    K = np.atleast_2d(maps).shape[0]
    assert got['mean'].shape == (K,) and sorted(got['central']) == sorted(central)
    if n == 0:
        assert np.isnan(got['mean']).all() and all(np.isnan(v) for v in got['central'].values())
        return
    assert (np.abs(got['mean'] - mean) <= 1e-11 * scale['mean']).all(), (got['mean'], mean)
    for e, v in central.items():
        assert abs(got['central'][e] - v) <= 1e-11 * scale[e], (e, got['central'][e], v, scale[e])


@pytest.mark.parametrize('nside', [1, 16, 64])
@pytest.mark.parametrize('K', [1, 2, 3])
def test_map_moments_match_oracle(gpu, nside, K):
    import torch
    from baryonification_amd import utils as U
    rng = np.random.default_rng(100 * nside + K)
    npix = 12 * nside * nside
    base = rng.normal(size=npix)
    maps = np.stack([0.6 * base + rng.normal(size=npix) ** (1 + a % 2) + a for a in range(K)])   # correlated, one skewed
    mask = rng.random(npix) < 0.7
    dirty = maps.copy()
    for a, v in zip(range(K), (UNSEEN, np.nan, np.inf)):
        dirty[a, rng.integers(0, npix, max(1, npix // 50))] = v
    dirty[0, rng.integers(0, npix, 2)] = -np.inf
    dirty[K - 1, rng.integers(0, npix, 2)] = UNSEEN * (1 + 1e-7)
    arg = lambda x: x[0] if K == 1 else x
    for mp, mk in ((maps, None), (maps, mask), (dirty, None), (dirty, mask)):
        got = U.map_moments(arg(mp), mask=mk)
        _check_moments(got, mp, 4, mk)
        again = U.map_moments(list(mp) if K > 1 else mp[0], mask=mk)                # a sequence of maps, and the same bits
        assert again['n'] == got['n'] and again['mean'].tobytes() == got['mean'].tobytes()
        assert np.array([again['central'][e] for e in got['central']]).tobytes() == np.array(list(got['central'].values())).tobytes()
    _check_moments(U.map_moments(arg(dirty), order=2, mask=mask), dirty, 2, mask)
    _check_moments(U.map_moments(torch.from_numpy(dirty).cuda() if K > 1 else torch.from_numpy(dirty[0]).cuda(), order=3,
                                 mask=torch.from_numpy(mask).cuda()), dirty, 3, mask)
    _check_moments(U.map_moments(arg(maps), mask=np.zeros(npix)), maps, 4, np.zeros(npix))       # nothing left: n = 0, NaN


def test_map_moments_far_from_zero(gpu):
    """|mean| / std = 100: the two passes keep the odd moments"""
    from baryonification_amd import utils as U
    rng = np.random.default_rng(9)
    x = 100.0 + rng.normal(size=12 * 64 * 64)
    y = -100.0 + 0.5 * (x - 100.0) + rng.normal(size=x.size) ** 2
    _check_moments(U.map_moments(x), x, 4, None)
    _check_moments(U.map_moments([x, y]), np.stack([x, y]), 4, None)


# ------------------------------------------------------------------------------------------------------------------- peaks
def _check_peaks(U, m, edges, mask=None, nest=False):
    ref, rflags = M.peaks(m, edges, mask, nest)
    got, flags = U.peak_counts(m, edges, mask=mask, nest=nest, return_flags=True)
    assert flags.dtype == np.int8 and np.array_equal(flags, rflags)
    for k in ('maxima', 'minima'):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    only = U.peak_counts(m, edges, mask=mask, nest=nest)
    assert np.array_equal(only['maxima'], ref['maxima']) and np.array_equal(only['minima'], ref['minima'])
    return ref


@pytest.mark.parametrize('nside', [1, 2, 16])
def test_peak_counts_match_oracle(gpu, nside):
    import torch
    from baryonification_amd import utils as U
    rng = np.random.default_rng(nside)
    npix = 12 * nside * nside
    noise = rng.normal(size=npix)
    edges = np.linspace(-2.0, 2.0, 9)                                               # values beyond +-2 are dropped
    ref = _check_peaks(U, noise, edges)
    if nside == 16:
        assert ref['maxima'].sum() > 200 and ref['minima'].sum() > 200
    levels = np.floor(rng.random(npix) * 5.0)                                       # 5 integer levels: ties everywhere
    ledges = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 4.5])                               # values sit exactly on the edges; 4.0 is in the last bin
    ref = _check_peaks(U, levels, ledges)
    _check_peaks(U, levels, np.array([1.0, 2.0, 4.0]))                              # 0 below the first edge, 4 on the last one: dropped
    const, cflags = U.peak_counts(np.full(npix, 3.0), ledges, return_flags=True)
    assert not const['maxima'].any() and not const['minima'].any() and not cflags.any()
    dirty = noise.copy()
    for v in (UNSEEN, np.nan, np.inf, -np.inf):
        dirty[rng.integers(0, npix, max(1, npix // 40))] = v
    mask = rng.random(npix) < 0.8
    _check_peaks(U, dirty, edges)
    ref, rflags = M.peaks(dirty, edges, mask)
    _check_peaks(U, dirty, edges, mask)
    nb = M.neighbours(nside, np.arange(npix))
    gone = ~M.good(dirty, mask)
    assert not rflags[nb[:, gone][nb[:, gone] >= 0]].any() and not rflags[gone].any()   # next to a bad pixel: never an extremum
    if nside > 1:
        r2n = H.ring2nest(nside, np.arange(npix))
        nest_map, nest_mask = np.empty(npix), np.empty(npix, dtype=bool)
        nest_map[r2n], nest_mask[r2n] = dirty, mask
        got, flags = U.peak_counts(nest_map, edges, mask=nest_mask, nest=True, return_flags=True)
        assert np.array_equal(got['maxima'], ref['maxima']) and np.array_equal(got['minima'], ref['minima'])
        assert np.array_equal(flags[r2n], rflags)
        _check_peaks(U, nest_map, edges, nest_mask, nest=True)
    dev, dflags = U.peak_counts(torch.from_numpy(dirty).cuda(), edges, mask=torch.from_numpy(mask).cuda(), return_flags=True)
    assert dev['maxima'].is_cuda and dflags.is_cuda and np.array_equal(dev['maxima'].cpu().numpy(), ref['maxima'])
    assert np.array_equal(dev['minima'].cpu().numpy(), ref['minima']) and np.array_equal(dflags.cpu().numpy(), rflags)


def test_peak_counts_of_seeded_white_noise(gpu):
    from baryonification_amd import utils as U
    m = np.random.default_rng(1).normal(size=12288)
    got = U.peak_counts(m, np.linspace(-8.0, 8.0, 4097))
    assert got['maxima'].shape == (4096,) and got['maxima'].sum() == 1390
    ref, _ = M.peaks(m, np.linspace(-8.0, 8.0, 4097))
    assert np.array_equal(got['maxima'], ref['maxima']) and np.array_equal(got['minima'], ref['minima'])


# -------------------------------------------------------------------------------------------------------- shell_statistics
SCALES = [0.0, 20 * ARCMIN, np.radians(1.0)]


def _shell_inputs():
    nside = 32
    rng = np.random.default_rng(32)
    npix = 12 * nside * nside
    kappa = rng.normal(size=npix) ** 2
    y = 0.5 * kappa + rng.normal(size=npix)
    y[rng.integers(0, npix, 20)] = UNSEEN
    mask = rng.random(npix) < 0.8
    return nside, np.stack([kappa, y]), mask


@pytest.mark.parametrize('window', ['gauss', 'tophat'])
def test_shell_statistics_equals_the_calls_one_by_one(gpu, window, monkeypatch):
    import torch
    from baryonification_amd import engine, utils as U
    nside, maps, mask = _shell_inputs()
    lmax, it, bins = 2 * nside, 1, np.linspace(-3.0, 6.0, 19)
    calls = []
    real = engine.ShtPlan.map2alm_device
    monkeypatch.setattr(engine.ShtPlan, 'map2alm_device', lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    res = U.shell_statistics(maps, SCALES, window=window, lmax=lmax, iter=it, order=4, peak_bins=bins, mask=mask)
    assert len(calls) == 2                                                          # K analyses, not K x n_scales
    monkeypatch.undo()
    exps = res['exponents']
    assert exps == U.moment_exponents(2, 4) and res['n'].shape == (3,) and res['n'].dtype == np.int64
    assert res['mean'].shape == (3, 2) and res['central'].shape == (3, 12) and res['maxima'].shape == res['minima'].shape == (3, 2, 18)
    zeroed = np.where(mask, maps, 0.0)
    for s, scale in enumerate(SCALES):
        w = U.gauss_beam(scale, lmax) if window == 'gauss' else U.tophat_beam(scale, lmax)
        sm = [U.smoothing(zeroed[k], beam_window=w, lmax=lmax, iter=it) for k in range(2)]
        mom = U.map_moments(sm, order=4, mask=mask)
        assert res['n'][s] == mom['n'] and res['mean'][s].tobytes() == mom['mean'].tobytes()
        assert res['central'][s].tobytes() == np.array([mom['central'][e] for e in exps]).tobytes()
        for k in range(2):
            pk = U.peak_counts(sm[k], bins, mask=mask)
            assert np.array_equal(res['maxima'][s, k], pk['maxima']) and np.array_equal(res['minima'][s, k], pk['minima'])
    assert res['n'][0] == (mask & M.good(maps)).sum() and res['maxima'].sum() > 0
    dev = U.shell_statistics(torch.from_numpy(maps).cuda(), SCALES, window=window, lmax=lmax, iter=it, peak_bins=bins,
                             mask=torch.from_numpy(mask).cuda())
    for k in ('n', 'mean', 'central', 'maxima', 'minima'):
        assert dev[k].is_cuda and dev[k].cpu().numpy().tobytes() == np.ascontiguousarray(res[k]).tobytes(), k
    one = U.shell_statistics(maps[0], SCALES[1], lmax=lmax, iter=it, order=3)       # one map, one scale, no peaks
    assert one['central'].shape == (1, 2) and 'maxima' not in one and one['exponents'] == [(2,), (3,)]


def test_shell_statistics_allocates_no_new_device_memory(gpu):
    import torch
    from baryonification_amd import utils as U
    nside, maps, mask = _shell_inputs()
    kw = dict(lmax=2 * nside, iter=1, peak_bins=np.linspace(-3.0, 6.0, 19), mask=mask)
    U.shell_statistics(maps, SCALES, **kw)
    torch.cuda.synchronize()
    before = torch.cuda.memory_reserved()
    for _ in range(2):
        U.shell_statistics(maps, SCALES, **kw)
    torch.cuda.synchronize()
    assert torch.cuda.memory_reserved() == before
