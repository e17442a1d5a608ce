"""MI355X: fft2_der_kernel, mapstats_peaks_grid_kernel and utils/flatstats.py against tests/flatstats_oracle.py.

Bounds.  Derivative maps: der_bound(N) x S_a, S_a = max|m_a b| max|x| (the oracle file says why and where the figure comes from).  Peak
counts and flags: exact (inputs without equal neighbours; the peaks of a smoothed map are taken on the device's own smoothed map).  The
Minkowski reduction on the device's own six maps: counts, n and v0 exact, the sums 1e-11 x the sum of the absolute terms of the bin
(test_gpu_minkowski.py's bound); end to end against the oracle pipeline: the propagation stands next to the assertion.
patch_statistics: the single calls, bit for bit."""
import numpy as np
import pytest

import fft2d_oracle as F
import flatstats_oracle as D

pytestmark = pytest.mark.gpu

L0 = 10.0
KINDS = ('unit', 'gauss', 'tophat', 'table')


def _filter(kind, N, L):
    """(engine arguments (kind, param, tk, tb), the oracle's beam on the full plane)"""
    if kind == 'unit':
        return ('unit', 0.0, None, None), None
    if kind == 'gauss':
        return ('gauss', 1.5 * L / N, None, None), D.beam_plane(N, L, 'gauss', 1.5 * L / N)
    if kind == 'tophat':
        return ('tophat', 2.5 * L / N, None, None), D.beam_plane(N, L, 'tophat', 2.5 * L / N)
    tk = np.linspace(0.0, 2 * np.pi / L * N / 2, 12)
    tb = 1.0 / (1.0 + (tk / tk[4]) ** 2)
    return ('table', 0.0, tk, tb), D.beam_plane(N, L, 'table', table=(tk, tb))


class _Der(object):
    """bfgx_derivatives_2d_device on the spectrum of one map, through engine: the work array and the outputs are filled with NaN first"""

    def __init__(self, x):
        import torch
        from baryonification_amd import utils as U
        self.N = x.shape[0]
        self.x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        self.spec = U.rfft2(self.x)
        self.spec0 = self.spec.clone()

    def __call__(self, L, flt, nder, spin):
        import torch
        from baryonification_amd import engine
        N = self.N
        work = torch.full((engine.derivatives_2d_work_doubles(N, nder),), float('nan'), dtype=torch.float64, device='cuda')
        out = torch.full((nder, N, N), float('nan'), dtype=torch.float64, device='cuda')
        engine.derivatives_2d_device(self.spec.data_ptr(), N, L, flt[0], flt[1], flt[2], flt[3], nder, spin, work.data_ptr(), out.data_ptr(),
                                     device=0, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(self.spec.view(torch.int64), self.spec0.view(torch.int64)), "the input spectrum changed"
        return out.cpu().numpy()


def _inputs(N):
    xs = [('noise', F.noise(N))] + [('wave %d %d' % w, D.wave(N, w[0], w[1], 0.4)) for w in D.waves(N)]
    return xs + [('impulse', D.impulse(N, N // 3, N - 2))]


@pytest.mark.parametrize('N', [8, 16, 64])
def test_derivatives_match_oracle(gpu, N):
    L = L0
    worst = 0.0
    for name, x in _inputs(N):
        run = _Der(x)
        for kind in KINDS:
            flt, beam = _filter(kind, N, L)
            first = None
            for spin in (False, True):
                ref, S = D.derivatives(x, L, beam, spin), D.scales(x, L, beam, spin)
                got = run(L, flt, 6, spin)
                assert np.isfinite(got).all(), (name, kind, spin)
                for a in range(6):
                    err = float(np.abs(got[a] - ref[a]).max() / S[a])
                    worst = max(worst, err)
                    assert err <= D.der_bound(N), (name, kind, spin, a, err)
                assert got.tobytes() == run(L, flt, 6, spin).tobytes(), "a repeated call differs"
                one = run(L, flt, 1, spin)
                assert one.shape == (1, N, N) and one[0].tobytes() == got[0].tobytes(), "nder = 1 is not the first of nder = 6"
                first = got if first is None else first
            assert first[:3].tobytes() == got[:3].tobytes()              # the two forms share u, u_x, u_y
    print("N = %d: worst derivative error %.2e of S_a (bound %.2e)" % (N, worst, D.der_bound(N)))


def _nyquist_noise(N):
    """noise plus a wave at the Nyquist index of each axis (with a phase, so that neither lies in the kernel of the odd factors)"""
    i = np.arange(N)
    sign = 1.0 - 2.0 * (i % 2)
    return F.noise(N) + sign[:, None] * np.cos(2 * np.pi * i / N + 0.3)[None, :] + np.cos(4 * np.pi * i / N + 0.3)[:, None] * sign[None, :]


# per size: the filter and the form of the first visit.  The reference is the full plane up to 2048; at 4096 the full plane takes 8 s
# on the host, so numpy's own half-plane pair stands in (flatstats_oracle.derivatives_large).  np.fft.irfft2 drops the imaginary part
# of the column c = N/2, and so does the library's fft_c2r_lines_kernel at every size: a real map's column N/2 is real after the
# transform along axis 0, a factor i g1 that is constant along that axis makes it imaginary, and it is dropped whether or not the kernel
# zeroed it.  So no reference, full plane or not, sees the rule on axis 1 through the maps; the rule on axis 0 (row N/2, which both
# routes keep) is what the Nyquist waves of the input test, at every size.
LARGE = {4096: ('gauss', True), 2048: ('tophat', False), 1024: ('table', False), 8: ('gauss', True)}


@pytest.mark.parametrize('sizes', [(4096, 8, 4096), (2048, 1024, 2048)])
def test_derivatives_large_sizes_in_the_order_of_the_cached_setups(gpu, sizes):
    """both column routes (in place up to 1024, four steps above) and the largest work array, nder = 6 and 1; a setup of another size
    in between changes nothing: the second visit gives the first one's bits"""
    seen = {}
    for N in sizes:
        L = 0.7 * N
        kind, spin = LARGE[N]
        x = _nyquist_noise(N)
        flt, beam = _filter(kind, N, L)
        run = _Der(x)
        got = run(L, flt, 6, spin)
        assert np.isfinite(got).all()
        if N in seen:
            assert got.tobytes() == seen[N]
            continue
        seen[N] = got.tobytes()
        one = run(L, flt, 1, spin)
        assert one.shape == (1, N, N) and one[0].tobytes() == got[0].tobytes(), "nder = 1 is not the first of nder = 6"
        if N > 1024:
            ref, S = D.derivatives_large(x, L, beam[:, :N // 2 + 1] if N > 2048 else beam, spin, half=N > 2048)
        else:
            ref, S = D.derivatives(x, L, beam, spin), D.scales(x, L, beam, spin)
        for a in range(6):
            err = float(np.abs(got[a] - ref[a]).max() / S[a])
            print("N = %d %s %s: %.2e of S_a (bound %.2e)" % (N, kind, (D.SPIN_NAMES if spin else D.NAMES)[a], err, D.der_bound(N)))
            assert err <= D.der_bound(N), (N, a, err)


def test_derivatives_2d_public(gpu):
    """numpy in, numpy out; a CUDA tensor stays on the device; no filter argument: the unfiltered derivatives; the waves' analytic values"""
    import torch
    from baryonification_amd import utils as U
    N, L = 64, 7.5
    for (m0, m1) in D.waves(N):
        x = D.wave(N, m0, m1, 0.3)
        got, ref, S = U.derivatives_2d(x, L), D.wave_derivatives(N, L, m0, m1, 0.3), D.scales(x, L)
        assert got.shape == (6, N, N) and got.dtype == np.float64
        for a in range(6):
            assert np.abs(got[a] - ref[a]).max() <= (D.der_bound(N) + 1e-13) * S[a], (m0, m1, a)     # (1e-13: the oracle against the closed forms)
    x = F.noise(N)
    sig = 2.0 * L / N
    a = U.derivatives_2d(x, L, sigma=sig)
    b = U.derivatives_2d(torch.from_numpy(x).cuda(), L, sigma=sig)
    c = U.derivatives_2d(x, L, fwhm=sig * np.sqrt(8 * np.log(2)), spin_form=True)
    assert b.is_cuda and b.cpu().numpy().tobytes() == a.tobytes()
    assert np.abs(c[:3] - a[:3]).max() <= 1e-14 * np.abs(a[:3]).max()
    ref = D.derivatives(x, L, D.beam_plane(N, L, 'gauss', sig), True)
    for k in range(6):
        assert np.abs(c[k] - ref[k]).max() <= D.der_bound(N) * D.scales(x, L, D.beam_plane(N, L, 'gauss', sig), True)[k]
    assert U.derivatives_2d(x, L, sigma=0.0).tobytes() == U.derivatives_2d(x, L).tobytes()      # b = exp(-0) = 1


# ------------------------------------------------------------------------------------------------- extrema
def _noise_grid(n, seed=0):
    m = np.random.default_rng(500 + 3 * n + seed).standard_normal((n, n))
    assert D.min_neighbour_gap(m) > 0 and np.unique(m).size == m.size    # no two neighbours (no two pixels at all) are equal
    return m


def _check_peaks(m, edges, mask, periodic):
    from baryonification_amd import utils as U
    ref, rflags = D.peaks(m, edges, mask, periodic)
    got, flags = U.peak_counts_2d(m, edges, mask=mask, periodic=periodic, return_flags=True)
    assert flags.dtype == np.int8 and flags.shape == m.shape and np.array_equal(flags, rflags), (m.shape, periodic)
    for key in ('maxima', 'minima'):
        assert got[key].dtype == np.int64 and np.array_equal(got[key], ref[key]), (key, m.shape, periodic)
    plain = U.peak_counts_2d(m, edges, mask=mask, periodic=periodic)
    assert np.array_equal(plain['maxima'], ref['maxima']) and np.array_equal(plain['minima'], ref['minima'])
    return ref, rflags


@pytest.mark.parametrize('periodic', [True, False])
@pytest.mark.parametrize('n', [3, 4, 5, 16, 17, 67, 130, 1024])
def test_peak_counts_match_oracle(gpu, n, periodic):
    m = _noise_grid(n)
    edges = np.linspace(-3.0, 3.0, 13)
    ref, flags = _check_peaks(m, edges, None, periodic)
    if n >= 16:
        assert ref['maxima'].sum() > 0 and ref['minima'].sum() > 0
        border = np.abs(flags[0]).sum() + np.abs(flags[-1]).sum() + np.abs(flags[:, 0]).sum() + np.abs(flags[:, -1]).sum()
        assert (border > 0) == periodic                                    # extrema on the seams of the periodic patch, none on an open border
    # with a mask, with NaN, infinite and UNSEEN pixels (at the seams too)
    rng = np.random.default_rng(n)
    dirty = m.copy()
    k = max(1, n * n // 40)
    for val in (np.nan, D.M.UNSEEN, np.inf):
        dirty[rng.integers(0, n, k), rng.integers(0, n, k)] = val
    dirty[0, n - 1] = np.nan
    mask = (rng.random((n, n)) < 0.9).astype(np.uint8)
    _check_peaks(dirty, edges, None, periodic)
    _check_peaks(dirty, edges, mask, periodic)
    _check_peaks(m, edges, mask.astype(bool), periodic)
    # nb = 1 and nb = 4096
    _check_peaks(m, np.array([-0.5, 10.0]), None, periodic)
    _check_peaks(m, np.linspace(-4.0, 4.0, 4097), mask, periodic)
    # values on an edge exactly: the edges are pixel values, extrema among them
    vals = np.sort(np.concatenate([m[flags == 1].ravel()[:3], m[flags == -1].ravel()[:3], m.ravel()[:2]]))
    vals = np.unique(vals)
    if vals.size >= 2:
        _check_peaks(m, vals, None, periodic)


def test_peak_counts_plateau_and_cuda_input(gpu):
    import torch
    from baryonification_amd import utils as U
    m = D.plateau(8)
    edges = np.array([-10.0, 0.0, 8.0, 9.0, 10.0])
    for periodic in (True, False):
        ref, flags = _check_peaks(m, edges, None, periodic)
        assert flags[5, 5] == 1 and flags[5, 2] == -1 and np.abs(flags).sum() == 2
        assert list(ref['maxima']) == [0, 0, 1, 0] and list(ref['minima']) == [1, 0, 0, 0]
    b = np.ones((8, 8))
    b[0, 3], b[7, 7], b[4, 0] = 5.0, -2.0, 7.0
    _, fp = _check_peaks(b, edges, None, True)
    _, fo = _check_peaks(b, edges, None, False)
    assert np.abs(fp).sum() == 3 and not fo.any()
    x = _noise_grid(67)
    mask = np.random.default_rng(1).random((67, 67)) < 0.9
    e = np.linspace(-3.0, 3.0, 9)
    host, hflags = U.peak_counts_2d(x, e, mask=mask, return_flags=True)
    dev, dflags = U.peak_counts_2d(torch.from_numpy(x).cuda(), e, mask=torch.from_numpy(mask).cuda(), return_flags=True)
    assert dev['maxima'].is_cuda and dflags.is_cuda and np.array_equal(dflags.cpu().numpy(), hflags)
    assert np.array_equal(dev['maxima'].cpu().numpy(), host['maxima']) and np.array_equal(dev['minima'].cpu().numpy(), host['minima'])


def test_peaks_of_a_smoothed_map(gpu):
    """on the device's own smoothed map, copied back: neighbours closer than the transform's rounding could change sides otherwise"""
    from baryonification_amd import utils as U
    N, L = 64, 10.0
    x = np.random.default_rng(5).standard_normal((N, N))
    u = U.derivatives_2d(x, L, sigma=3 * L / N)[0]
    assert D.min_neighbour_gap(u) > 0
    edges = u.mean() + u.std() * np.linspace(-2.5, 2.5, 11)
    for periodic in (True, False):
        ref, _ = _check_peaks(u, edges, None, periodic)
        assert 0 < ref['maxima'].sum() < 60                                # a smooth field: a few tens of peaks, not a ninth of the pixels
    ou = D.derivatives(x, L, D.beam_plane(N, L, 'gauss', 3 * L / N))[0]
    print("smallest neighbour gap of the oracle's smoothed map: %.2e of max|u|" % (D.min_neighbour_gap(ou) / np.abs(ou).max()))


# ------------------------------------------------------------------------------------------------- Minkowski functionals
MF_N, MF_L = 64, 10.0


def _mf_input():
    x = np.random.default_rng(5).standard_normal((MF_N, MF_N))
    return x, 3 * MF_L / MF_N


def _check_reduction(got, ref, edges):
    nb = edges.size - 1
    assert isinstance(got['n'], int) and got['n'] == ref['n']
    assert got['count'].dtype == np.int64 and np.array_equal(got['count'], ref['count'])
    assert got['v0'].shape == (nb + 1,) and np.array_equal(got['v0'], ref['v0'])
    for k, a, f in (('v1', 0, 4.0), ('v2', 1, 2.0 * np.pi)):
        norm = f * ref['n'] * np.diff(edges)
        err = np.abs(got[k] * norm - ref['sums'][a])
        assert (err <= 1e-11 * ref['scale'][a]).all(), (k, err.max())


@pytest.mark.parametrize('nb', [6, 8, 12])
def test_minkowski_reduction_on_the_devices_own_maps(gpu, nb):
    from baryonification_amd import utils as U
    x, sig = _mf_input()
    ders = U.derivatives_2d(x, MF_L, sigma=sig, spin_form=True)
    edges = ders[0].mean() + ders[0].std() * np.linspace(-2.5, 2.5, nb + 1)
    mask = np.random.default_rng(7).random((MF_N, MF_N)) < 0.85
    for mk in (None, mask):
        ref = D.minkowski(ders, edges, mk)
        got = U.minkowski_from_derivatives(ders.reshape(6, -1), edges, mask=None if mk is None else mk.ravel(), spin_form=True)
        _check_reduction(got, ref, edges)
    # minkowski_functionals_2d is that chain: the same bits
    full = U.minkowski_functionals_2d(x, MF_L, edges, sigma=sig)
    one = U.minkowski_from_derivatives(ders.reshape(6, -1), edges, spin_form=True)
    for k in ('count', 'v0', 'v1', 'v2'):
        assert full[k].tobytes() == one[k].tobytes(), k
    assert full['n'] == one['n'] == MF_N * MF_N


@pytest.mark.parametrize('nb', [6, 8, 12])
def test_minkowski_functionals_2d_end_to_end(gpu, nb):
    from baryonification_amd import utils as U
    x, sig = _mf_input()
    N, L = MF_N, MF_L
    beam = D.beam_plane(N, L, 'gauss', sig)
    od = D.derivatives(x, L, beam, spin_form=True)
    u = od[0]
    edges = u.mean() + u.std() * np.linspace(-2.5, 2.5, nb + 1)
    # the oracle's own u decides the bins: no pixel may be within the transform's rounding of an edge
    gap = float(np.abs(u.ravel()[:, None] - edges[None, :]).min() / np.abs(u).max())
    print("nb = %d: min|u - edge| = %.2e of max|u|" % (nb, gap))
    assert gap >= 1e-6
    ora = D.minkowski(od, edges)
    got = U.minkowski_functionals_2d(x, L, edges, sigma=sig)
    assert got['n'] == N * N and np.array_equal(got['count'], ora['count']) and np.array_equal(got['v0'], ora['v0'])
    # Propagation.  Each of the device's six maps is within eps_a = der_bound(64) S_a of the oracle's (test_derivatives_match_oracle).
    # With (c, s) = (u_x, u_y) / |grad u| the two summed terms of a pixel are
    #     t1 = |grad u|                                      dt1 = c du_x + s du_y
    #     t2 = q_cross c s - lap / 2 + q_plus (c^2 - s^2) / 2,
    #     dt2 = -dlap / 2 + (c^2 - s^2) dq_plus / 2 + c s dq_cross + (q_cross (c^2 - s^2) - 2 q_plus c s) (c du_y - s du_x) / |grad u|
    # to first order (the second order is smaller by |d grad u| / |grad u|, asserted below to be under 1e-3), so
    #     |dt| <= sum_a |dt / da| eps_a <= 6 der_bound(64) max_a (|dt / da| S_a)
    # and a bin's sum is off by at most 6 der_bound(64) S, S = the sum over the bin's pixels of that maximum.  The reduction's own
    # rounding (a few eps of the bin's sum of absolute terms, which is below S) is far inside that and gets no allowance of its own.
    S = D.scales(x, L, beam, spin_form=True)
    g = np.hypot(od[1], od[2])
    assert g.min() >= 1e3 * D.der_bound(N) * (S[1] + S[2])
    c, s = od[1] / g, od[2] / g
    rot = np.abs(od[5] * (c * c - s * s) - 2 * od[4] * c * s) / g
    w1 = np.maximum(np.abs(c) * S[1], np.abs(s) * S[2])
    w2 = np.max([0.5 * S[3] * np.ones_like(g), 0.5 * np.abs(c * c - s * s) * S[4], np.abs(c * s) * S[5], rot * np.abs(s) * S[1], rot * np.abs(c) * S[2]], axis=0)
    b = np.searchsorted(edges, u.ravel(), side='right') - 1
    inside = (b >= 0) & (b < nb)
    for k, a, f, w in (('v1', 0, 4.0, w1), ('v2', 1, 2.0 * np.pi, w2)):
        Sb = np.bincount(b[inside], weights=w.ravel()[inside], minlength=nb)
        err = np.abs(got[k] * (f * ora['n'] * np.diff(edges)) - ora['sums'][a])
        tol = 6 * D.der_bound(N) * Sb
        print("nb = %d %s: worst error / tolerance %.2e" % (nb, k, float((err / tol).max())))
        assert (err <= tol).all(), (k, err, tol)


# ------------------------------------------------------------------------------------------------- patch_statistics
PS_N, PS_L = 32, 4.0
PS_SCALES = [0.0, 0.3, 0.5, 0.9]


def _patch_inputs():
    rng = np.random.default_rng(32)
    kappa = rng.standard_normal((PS_N, PS_N)) ** 2
    y = 0.5 * kappa + rng.standard_normal((PS_N, PS_N))
    t = rng.standard_normal((PS_N, PS_N))
    return np.stack([kappa, y, t]), rng.random((PS_N, PS_N)) < 0.8


def _single_calls(maps, mask, scale, window, order, pbins, mbins, periodic):
    """what patch_statistics promises, one call at a time: (n, mean, central in moment_exponents' order, maxima, minima, v0, v1, v2)"""
    from baryonification_amd import utils as U
    K = maps.shape[0]
    kw = {} if scale == 0 else {'fwhm': scale} if window == 'gauss' else {'tophat': scale}
    zeroed = maps if mask is None else np.where(mask, maps, 0.0)
    sm = np.stack([U.derivatives_2d(zeroed[k], PS_L, **kw)[0] for k in range(K)])
    mom = U.map_moments(sm.reshape(K, -1), order=order, mask=None if mask is None else mask.ravel())
    central = np.array([mom['central'][e] for e in U.moment_exponents(K, order)])
    out = {'n': mom['n'], 'mean': mom['mean'], 'central': central}
    if pbins is not None:
        pk = [U.peak_counts_2d(sm[k], pbins, mask=mask, periodic=periodic) for k in range(K)]
        out['maxima'], out['minima'] = np.stack([p['maxima'] for p in pk]), np.stack([p['minima'] for p in pk])
    if mbins is not None:
        mf = [U.minkowski_functionals_2d(zeroed[k], PS_L, mbins, mask=mask, **kw) for k in range(K)]
        for key in ('v0', 'v1', 'v2'):
            out[key] = np.stack([f[key] for f in mf])
    return out


@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('window', ['gauss', 'tophat'])
def test_patch_statistics_equals_the_single_calls(gpu, K, window):
    import torch
    from baryonification_amd import utils as U
    maps, mask = _patch_inputs()
    maps = maps[:K]
    pbins, mbins = np.linspace(-3.0, 6.0, 19), np.linspace(-1.0, 3.0, 12)
    for use_mask, use_p, use_m, periodic, order in ((False, False, False, True, 4), (True, True, True, True, 3), (False, True, True, False, 4),
                                                    (True, False, True, True, 2)):
        mk = mask if use_mask else None
        kw = dict(window=window, order=order, peak_bins=pbins if use_p else None, mf_bins=mbins if use_m else None, mask=mk, periodic=periodic)
        res = U.patch_statistics(maps if K > 1 else maps[0], PS_L, PS_SCALES, **kw)
        keys = ['central', 'exponents', 'mean', 'n'] + (['maxima', 'minima'] if use_p else []) + (['v0', 'v1', 'v2'] if use_m else [])
        assert sorted(res) == sorted(keys)
        S, nt = len(PS_SCALES), len(U.moment_exponents(K, order))
        assert res['exponents'] == U.moment_exponents(K, order)
        assert res['n'].shape == (S,) and res['n'].dtype == np.int64 and res['mean'].shape == (S, K) and res['central'].shape == (S, nt)
        if use_p:
            assert res['maxima'].shape == res['minima'].shape == (S, K, 18) and res['maxima'].dtype == np.int64
        if use_m:
            assert res['v0'].shape == (S, K, 12) and res['v1'].shape == res['v2'].shape == (S, K, 11)
        for s, scale in enumerate(PS_SCALES):
            one = _single_calls(maps, mk, scale, window, order, kw['peak_bins'], kw['mf_bins'], periodic)
            assert int(res['n'][s]) == one['n'] == (PS_N * PS_N if mk is None else int(mk.sum()))
            for key in keys:
                if key not in ('n', 'exponents'):
                    assert np.ascontiguousarray(res[key][s]).tobytes() == np.ascontiguousarray(one[key]).tobytes(), (key, s, use_mask)
        # CUDA input: the same bits, CUDA results
        tm = torch.from_numpy(maps if K > 1 else maps[0]).cuda()
        dev = U.patch_statistics(tm, PS_L, PS_SCALES, **dict(kw, mask=None if mk is None else torch.from_numpy(mk).cuda()))
        for key in keys:
            if key != 'exponents':
                assert dev[key].is_cuda and dev[key].cpu().numpy().tobytes() == np.ascontiguousarray(res[key]).tobytes(), key


def test_patch_statistics_smooths_and_sees_unseen_pixels(gpu):
    """the variance falls with the scale; an UNSEEN pixel counts as 0 on the way in and is left out after"""
    from baryonification_amd import utils as U
    maps, _ = _patch_inputs()
    res = U.patch_statistics(maps[0], PS_L, PS_SCALES)
    var = res['central'][:, 0]
    assert (np.diff(var) < 0).all() and np.isclose(var[0], maps[0].var(), rtol=1e-12) and np.isclose(res['mean'][0, 0], maps[0].mean(), rtol=1e-12)
    holed = maps[0].copy()
    holed[3, 4] = holed[20, 0] = D.M.UNSEEN
    mask = np.ones((PS_N, PS_N), bool)
    mask[3, 4] = mask[20, 0] = False
    a = U.patch_statistics(holed, PS_L, PS_SCALES, mf_bins=np.linspace(-1.0, 3.0, 12))
    b = U.patch_statistics(maps[0], PS_L, PS_SCALES, mf_bins=np.linspace(-1.0, 3.0, 12), mask=mask)
    assert (a['n'] == PS_N * PS_N - 2).all()
    for key in ('n', 'mean', 'central', 'v0', 'v1', 'v2'):
        assert a[key].tobytes() == b[key].tobytes(), key


def test_patch_statistics_allocates_no_new_device_memory(gpu):
    import torch
    from baryonification_amd import utils as U
    maps, mask = _patch_inputs()
    tm, tk = torch.from_numpy(maps).cuda(), torch.from_numpy(mask).cuda()
    kw = dict(peak_bins=np.linspace(-3.0, 6.0, 19), mf_bins=np.linspace(-1.0, 3.0, 12), mask=tk)
    U.patch_statistics(tm, PS_L, PS_SCALES, **kw)
    torch.cuda.synchronize()
    before, reserved = torch.cuda.memory_allocated(), torch.cuda.memory_reserved()
    U.patch_statistics(tm, PS_L, PS_SCALES, **kw)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() <= before and torch.cuda.memory_reserved() == reserved


def test_gridded_map_statistics_takes_its_side_from_the_map(gpu):
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    maps, mask = _patch_inputs()
    res_pix = 0.25
    Map = bfg.utils.GriddedMap(map=maps[0], redshift=0.2, bins=(np.arange(PS_N) + 0.5) * res_pix, cosmo=dict(syn.COSMO))
    kw = dict(window='tophat', order=3, peak_bins=np.linspace(-3.0, 6.0, 10), mf_bins=np.linspace(-1.0, 3.0, 8), mask=mask, periodic=False)
    got = Map.statistics([0.0, 0.7], **kw)
    ref = bfg.utils.patch_statistics(maps[0], PS_N * res_pix, [0.0, 0.7], **kw)
    other = bfg.utils.patch_statistics(maps[0], 2 * PS_N * res_pix, [0.0, 0.7], **kw)
    assert sorted(got) == sorted(ref)
    for key in ref:
        assert key == 'exponents' or got[key].tobytes() == ref[key].tobytes(), key
    assert got['v1'].tobytes() != other['v1'].tobytes()
