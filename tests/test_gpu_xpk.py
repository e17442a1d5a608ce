"""The cross power spectrum of two gridded 3-D maps on the GPU: the cross modes of the last strided FFT pass (BIN 3 and 4 of
fft_c2c_strided_kernel in csrc/bfgx_fft.hpp) through engine.fft_slab_axis0_xpk_device, and the public entry engine.cross_power_spectrum,
against tests/xpk_oracle.py (plain numpy, sums in long double).

  1. the cross pass on synthetic spectra (moduli in [1, 2], random phases, NaN pad columns), a subset of test_gpu_fft.AXIS0_CASES
  2. one mode at a time: f_a must be read at exactly the (row, line, column) f_b leaves from
  3. the public entry against the oracle: B = A, B = -A, B = A shifted, B independent; numpy inputs and CUDA tensors
  4. the window weights p = 1, 2, 3
  5. cached setups called in the order large, small, large

Bound of 1, 2 and 5 (fft_oracle.bound, what the auto pass is held to): per filled bin |paa - ref| / ref, |pbb - ref| / ref and
|pab - ref| / sqrt(paa_ref pbb_ref) <= 16 x numpy's own FFT error against the long-double DFT at the same N, about 5e-15.  Moduli
within a factor 2 make an error relative to max|F| one relative to each product; Cauchy-Schwarz makes sqrt(paa pbb) the scale of pab,
which may itself cancel to nothing.  3 and 4 are held to 1e-10 (pab relative to sqrt(paa pbb)), the tolerance
test_gpu_fft.test_power_spectrum_bin_edges uses for the same route.

Measured on the MI355X, check 1 and 5, worst bin of the worst case per N (the bound is 1.8e-15 at N = 8, 4.1e-15 to 5.3e-15 above):
  N      8        16       64       256      512      1024
  paa    2.6e-16  2.5e-16  7.2e-16  5.1e-16  8.2e-16  1.6e-15
  pbb    3.0e-16  3.4e-16  5.8e-16  6.8e-16  9.0e-16  1.4e-15
  pab    1.1e-16  2.0e-16  3.0e-16  2.2e-16  2.6e-16  2.8e-16    (relative to sqrt(paa pbb))
paa is a sum of the given spectrum's squares alone (no transform), so its figure is that of the atomic sums against the long-double
ones.  The file takes 16 s, 12 of them the first call's start-up of the runtime."""
import numpy as np
import pytest

import fft_oracle as O
import xpk_oracle as X

pytestmark = pytest.mark.gpu

TWO_PI = 2 * np.pi


@pytest.fixture(scope='module', autouse=True)
def _release_the_tables():
    """the setups of this file hold 0.5 GB bin tables (N = 1024): hand them back when the file is done"""
    yield
    import torch
    from baryonification_amd import _lib
    torch.cuda.synchronize()
    _lib.load().bfgx_cache_clear()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


def _padded(work, pitch):
    """[N][ncols][nz] -> device [N][ncols][pitch][2], the pad columns c > N/2 NaN"""
    out = np.full(work.shape[:2] + (pitch,), np.nan + 1j * np.nan)
    out[:, :, :work.shape[2]] = work
    return _dev(out.view(np.float64).reshape(out.shape + (2,)))


def _run_xpk(spec_dev, work_dev, N, ncols, col0, L, nk, p):
    """fft_slab_axis0_xpk_device on device tensors [N][ncols][pitch][2] -> (paa, pbb, pab, k_sum, counts); the outputs start as garbage"""
    import torch
    from baryonification_amd import engine
    sums = torch.full((4, nk), float('nan'), dtype=torch.float64, device='cuda:0')
    cnt = torch.full((nk,), -1, dtype=torch.int64, device='cuda:0')
    engine.fft_slab_axis0_xpk_device(spec_dev.data_ptr(), work_dev.data_ptr(), N, ncols, col0, L, nk, p, sums[0].data_ptr(), sums[1].data_ptr(),
                                     sums[2].data_ptr(), sums[3].data_ptr(), cnt.data_ptr())
    torch.cuda.synchronize()
    s = sums.cpu().numpy()
    return s[0], s[1], s[2], s[3], cnt.cpu().numpy()


def _synthetic_pair(N, ncols, seed):
    """(spec_a, work_b): two spectra [N][ncols][N/2 + 1] with moduli in [1, 2] and random phases, the second one given before its transform
    along axis 0"""
    rng = np.random.default_rng(seed)
    shape = (N, ncols, N // 2 + 1)
    FA = rng.uniform(1.0, 2.0, shape) * np.exp(2j * np.pi * rng.uniform(0, 1, shape))
    FB = rng.uniform(1.0, 2.0, shape) * np.exp(2j * np.pi * rng.uniform(0, 1, shape))
    return FA, np.fft.ifft(FB, axis=0)


def _check_xpk(got, ref, N):
    """the assertions of check 1 -> (err_aa, err_bb, err_ab)"""
    (paa, pbb, pab, ks, cnt), (raa, rbb, rab, rks, rcnt) = got, ref
    for a in (paa, pbb, pab, ks):
        assert np.isfinite(a).all()                                        # (a NaN pad column that was binned would show here)
    assert np.array_equal(cnt, rcnt)
    full = rcnt > 0
    for a in (paa, pbb, pab, ks):
        assert (a[~full] == 0).all()
    if not full.any():
        return 0.0, 0.0, 0.0
    assert np.abs(ks[full] / rks[full] - 1).max() <= 1e-12
    eaa = np.abs(paa[full] - raa[full]) / raa[full]
    ebb = np.abs(pbb[full] - rbb[full]) / rbb[full]
    eab = np.abs(pab[full] - rab[full]) / np.sqrt(raa[full] * rbb[full])
    print("   N = %4d: paa %.2e  pbb %.2e  pab %.2e  (bound %.2e)" % (N, eaa.max(), ebb.max(), eab.max(), O.bound(N)))
    assert eaa.max() <= O.bound(N), ('paa', int(np.argmax(eaa)), eaa.max())
    assert ebb.max() <= O.bound(N), ('pbb', int(np.argmax(ebb)), ebb.max())
    assert eab.max() <= O.bound(N), ('pab', int(np.argmax(eab)), eab.max())
    return float(eaa.max()), float(ebb.max()), float(eab.max())


# ------------------------------------------------------------------------------------------------- 1. synthetic spectra
# (N, nk, L, ncols, col0) out of test_gpu_fft.AXIS0_CASES, with the window order: N = 8 .. 1024, nk = 1, 7, 254 (table), 255, 2048 (per mode), 1 to 3 columns,
# col0 = 0, 1, N/2, N - ncols; p = 0 and 2
XPK_CASES = [
    ((8, 1, 305.0, 1, 0), 0), ((8, 7, TWO_PI, 3, 5), 2), ((8, 254, 305.0, 1, 4), 2), ((8, 255, 1.0, 2, 0), 0), ((8, 2048, TWO_PI, 3, 1), 2),
    ((16, 7, 305.0, 3, 0), 0), ((16, 2, 1.0, 2, 8), 2), ((16, 255, TWO_PI, 1, 1), 2), ((16, 2048, 305.0, 3, 13), 0),
    ((64, 1, TWO_PI, 2, 0), 2), ((64, 254, 1.0, 3, 1), 0), ((64, 255, 305.0, 2, 32), 2), ((64, 2048, 1.0, 1, 0), 0), ((64, 7, 305.0, 1, 63), 2),
    ((256, 7, 1.0, 3, 0), 2), ((256, 254, TWO_PI, 2, 1), 0), ((256, 255, 305.0, 3, 253), 0), ((256, 2048, 305.0, 1, 128), 2), ((256, 1, 305.0, 2, 254), 0),
    ((512, 7, 305.0, 2, 1), 0), ((512, 254, 305.0, 3, 0), 2), ((512, 255, 1.0, 1, 511), 2), ((512, 2048, TWO_PI, 3, 0), 0), ((512, 2, TWO_PI, 2, 256), 2),
    ((1024, 1, 305.0, 3, 0), 2), ((1024, 254, 305.0, 2, 1), 0), ((1024, 255, 1.0, 3, 1021), 0), ((1024, 2048, 305.0, 1, 0), 2),
    ((1024, 254, 305.0, 3, 512), 2),
]


@pytest.mark.parametrize('case,p', XPK_CASES)
def test_xpk_synthetic_spectra(gpu, case, p):
    from baryonification_amd import engine
    N, nk, L, ncols, col0 = case
    spec_a, work_b = _synthetic_pair(N, ncols, 11 * N + nk + ncols + p)
    ref = X.axis0_xpk_ref(spec_a, work_b, N, col0, L, nk, p)
    pitch = engine.fft_pitch(N)
    da, db = _padded(spec_a, pitch), _padded(work_b, pitch)
    print("xpk N = %4d nk = %4d L = %-6.4g cols %d @ %4d p = %d: %d of %d bins filled" % (N, nk, L, ncols, col0, p, (ref[4] > 0).sum(), nk))
    got = _run_xpk(da, db, N, ncols, col0, L, nk, p)
    _check_xpk(got, ref, N)
    if nk <= 254:
        # bins, counts and |k| sums now come from the cached table: bitwise the same; the three power sums are added by atomics in another order
        again = _run_xpk(da, db, N, ncols, col0, L, nk, p)
        assert np.array_equal(again[4], got[4]) and np.array_equal(again[3].view(np.uint64), got[3].view(np.uint64))
        _check_xpk(again, ref, N)
    # neither input is changed by the pass
    assert np.array_equal(db.cpu().numpy().view(np.uint64), _padded(work_b, pitch).cpu().numpy().view(np.uint64))


# ------------------------------------------------------------------------------------------------- 2. one mode at a time
ALPHA, BETA = 1 + 2j, 3 - 1j                 # Re(alpha conj beta) = 1


@pytest.mark.parametrize('nk', [254, 2048])
@pytest.mark.parametrize('N', [8, 64, 512, 1024])
def test_xpk_one_hot(gpu, N, nk):
    """A and B carry ONE mode (a0, b, c), amplitudes alpha N and beta N: pab must hold m N^2 Re(alpha conj beta) = m N^2 in the reference's
    bin of that mode (nowhere if it lies outside the bins), paa and pbb m N^2 |alpha|^2 and m N^2 |beta|^2, every other bin less than the
    bound times N^2 |alpha| |beta|.  With A's mode moved to the next row, then to the next line, pab must vanish to the same bound while
    paa and pbb keep their entries (in the bins of where their modes now are)."""
    import torch
    from baryonification_amd import engine
    L = O.ONE_HOT_L
    pitch, nz = engine.fft_pitch(N), N // 2 + 1
    j = np.arange(N, dtype=np.int64)
    tol = O.bound(N) * N * N * abs(ALPHA) * abs(BETA)
    work = torch.empty((N, 1, pitch, 2), dtype=torch.float64, device='cuda:0')
    spec = torch.empty((N, 1, pitch, 2), dtype=torch.float64, device='cuda:0')

    def mult(c):
        return 2.0 if 0 < c < N // 2 else 1.0

    def expect(a, b, c, amp2):
        e = np.zeros(nk)
        _, bin_ = O.mode_k_and_bin(N, L, nk, a, b, c)
        if 0 <= bin_ < nk:
            e[bin_] = mult(c) * N * N * amp2
        return e

    n_runs = n_hits = 0
    for (a0, b, c) in O.one_hot_modes(N):
        ang = 2 * np.pi * ((a0 * j) % N) / N
        col = BETA * (np.cos(ang) + 1j * np.sin(ang))                      # its transform along axis 0: beta N at row a0
        work.fill_(float('nan'))
        work[:, 0, :nz, :] = 0.0
        work[:, 0, c, :] = _dev(np.stack([col.real, col.imag], axis=1))
        a_row, c_line = (a0 + 1) % N, (c + 1 if c + 1 < nz else c - 1)
        for (ar, cl, together) in ((a0, c, True), (a_row, c, False), (a0, c_line, False)):
            spec.fill_(float('nan'))
            spec[:, 0, :nz, :] = 0.0
            spec[ar, 0, cl, 0] = ALPHA.real * N
            spec[ar, 0, cl, 1] = ALPHA.imag * N
            paa, pbb, pab, ks, cnt = _run_xpk(spec, work, N, 1, b, L, nk, 0)
            assert np.isfinite(paa).all() and np.isfinite(pbb).all() and np.isfinite(pab).all()
            where = (a0, b, c, ar, cl)
            assert np.abs(pbb - expect(a0, b, c, abs(BETA) ** 2)).max() <= tol, where
            assert np.abs(paa - expect(ar, b, cl, abs(ALPHA) ** 2)).max() <= tol, where
            want_ab = expect(a0, b, c, (ALPHA * np.conj(BETA)).real) if together else np.zeros(nk)
            assert np.abs(pab - want_ab).max() <= tol, (where, np.flatnonzero(np.abs(pab) > 0.5)[:4], np.abs(pab).max())
            n_runs += 1
            n_hits += int(together and want_ab.any())
    print("one-hot N = %4d nk = %4d: %d runs, %d modes inside the bins" % (N, nk, n_runs, n_hits))
    assert n_runs == 3 * len(O.one_hot_modes(N)) and n_hits >= 8


# ------------------------------------------------------------------------------------------------- 3. the public entry
def _poisson_with_spike(N, seed):
    rng = np.random.default_rng(seed)
    M = rng.poisson(4.0, (N, N, N)).astype(np.float64)
    M[3, 5, 7] += 500.0
    return M


def _check_public(got, ref, tol=1e-10):
    assert set(got) == {'k', 'paa', 'pbb', 'pab', 'r', 'counts'}
    assert np.array_equal(got['counts'], ref['counts'])
    good = ref['counts'] > 0
    assert good.any()
    for key in ('k', 'paa', 'pbb', 'pab', 'r'):
        assert np.array_equal(np.isnan(got[key]), ~good), key
    assert np.abs(got['k'][good] / ref['k'][good] - 1).max() <= 1e-12
    assert np.abs(got['paa'][good] / ref['paa'][good] - 1).max() <= tol
    assert np.abs(got['pbb'][good] / ref['pbb'][good] - 1).max() <= tol
    scale = np.sqrt(ref['paa'][good] * ref['pbb'][good])
    assert (np.abs(got['pab'][good] - ref['pab'][good]) / scale).max() <= tol
    assert np.abs(got['r'][good] - ref['r'][good]).max() <= 2 * tol
    return good


PUBLIC_CASES = [(16, 1, 305.0), (16, 15, 1.0), (32, 15, 305.0), (32, 31, TWO_PI), (64, 31, 305.0), (64, 254, 305.0), (64, 255, 305.0), (32, 254, 1.0),
                (16, 255, TWO_PI)]


@pytest.mark.parametrize('N,Nk,L', PUBLIC_CASES)
def test_cross_power_spectrum_against_the_oracle(gpu, N, Nk, L):
    import torch
    from baryonification_amd import engine
    A = _poisson_with_spike(N, N)
    rolled = np.roll(A, (1, 2, 3), axis=(0, 1, 2))
    other = _poisson_with_spike(N, N + 1000)
    # B = A
    same = engine.cross_power_spectrum(A, A, L, Nk)
    good = _check_public(same, X.cross_power_spectrum_ref(A, A, L, Nk))
    assert np.abs(same['pab'][good] / same['paa'][good] - 1).max() <= 1e-13 and np.abs(same['pbb'][good] / same['paa'][good] - 1).max() <= 1e-13
    assert np.abs(same['r'][good] - 1).max() <= 1e-13
    k_cen, Pk, k_c = engine.power_spectrum(A, L, Nk)
    assert np.array_equal(k_c, same['counts'])
    assert np.abs(same['paa'][good] / Pk[good] - 1).max() <= 1e-12 and np.abs(same['k'][good] / k_cen[good] - 1).max() <= 1e-12
    # B = -A
    neg = engine.cross_power_spectrum(A, -A, L, Nk)
    _check_public(neg, X.cross_power_spectrum_ref(A, -A, L, Nk))
    assert np.abs(neg['r'][good] + 1).max() <= 1e-13
    # B = A shifted by (1, 2, 3): the same |F|, phases that turn pab to both signs
    ref = X.cross_power_spectrum_ref(A, rolled, L, Nk)
    shifted = engine.cross_power_spectrum(A, rolled, L, Nk)
    _check_public(shifted, ref)
    if good.sum() >= 8:
        assert (shifted['pab'][good] > 0).any() and (shifted['pab'][good] < 0).any()
    # B independent
    indep = engine.cross_power_spectrum(A, other, L, Nk)
    _check_public(indep, X.cross_power_spectrum_ref(A, other, L, Nk))
    # CUDA tensors are analysed where they lie and give the same
    dA, dB = torch.from_numpy(A).to('cuda:0'), torch.from_numpy(other).to('cuda:0')
    on_dev = engine.cross_power_spectrum(dA, dB, L, Nk)
    assert np.array_equal(on_dev['counts'], indep['counts'])
    for key in ('k', 'paa', 'pbb'):
        assert np.abs(on_dev[key][good] / indep[key][good] - 1).max() <= 1e-12, key
    assert (np.abs(on_dev['pab'][good] - indep['pab'][good]) / np.sqrt(indep['paa'][good] * indep['pbb'][good])).max() <= 1e-12
    assert np.array_equal(np.isnan(on_dev['r']), ~good)
    assert np.array_equal(dA.cpu().numpy(), A) and np.array_equal(dB.cpu().numpy(), other)
    tk, tP, tc = engine.power_spectrum_tensor(dA, L, Nk)
    assert np.array_equal(tc, k_c) and np.array_equal(np.isnan(tP), ~good) and np.array_equal(np.isnan(tk), ~good)
    assert np.abs(tP[good] / Pk[good] - 1).max() <= 1e-12 and np.abs(tk[good] / k_cen[good] - 1).max() <= 1e-12


# ------------------------------------------------------------------------------------------------- 4. window
@pytest.mark.parametrize('p,name', [(1, 'ngp'), (2, 'cic'), (3, 'tsc')])
@pytest.mark.parametrize('N,Nk', [(16, 15), (64, 31), (64, 255)])
def test_cross_power_spectrum_window(gpu, N, Nk, p, name):
    from baryonification_amd import engine
    L = 305.0
    A, B = _poisson_with_spike(N, N + p), _poisson_with_spike(N, N + 50 + p)
    got = engine.cross_power_spectrum(A, B, L, Nk, window=p)
    good = _check_public(got, X.cross_power_spectrum_ref(A, B, L, Nk, p))
    plain = engine.cross_power_spectrum(A, B, L, Nk)
    assert np.array_equal(plain['counts'], got['counts']) and np.abs(plain['k'][good] / got['k'][good] - 1).max() <= 1e-12      # not weighted
    assert (got['paa'][good] >= plain['paa'][good] * (1 - 1e-12)).all()               # every weight is >= 1
    assert (got['paa'][good][-1:] > plain['paa'][good][-1:] * 1.5).all()              # ... and large near the Nyquist frequency
    named = engine.cross_power_spectrum(A, B, L, Nk, window=name)
    for key in ('paa', 'pbb'):
        assert np.abs(named[key][good] / got[key][good] - 1).max() <= 1e-13
    assert (np.abs(named['pab'][good] - got['pab'][good]) / np.sqrt(got['paa'][good] * got['pbb'][good])).max() <= 1e-13
    assert np.array_equal(engine.cross_power_spectrum(A, B, L, Nk, window=name.upper())['counts'], got['counts'])


# ------------------------------------------------------------------------------------------------- 5. large, small, large
@pytest.mark.parametrize('big,small', [((1024, 2048), (1024, 255)), ((512, 100), (256, 100))])
def test_cached_xpk_setups_large_small_large(gpu, big, small):
    """per-mode binning at N = 1024 with nk = 2048, then nk = 255 (less LDS, the same instantiation), then 2048 again; table binning at
    N = 512, then N = 256, then 512 again: the dynamic-LDS attribute is per instantiation, the setups per shape.  L is this test's own,
    so that all three setups are built here."""
    from baryonification_amd import engine
    L = 79.0
    res = []
    for (N, nk) in (big, small, big):
        spec_a, work_b = _synthetic_pair(N, 1, N + nk)
        pitch = engine.fft_pitch(N)
        got = _run_xpk(_padded(spec_a, pitch), _padded(work_b, pitch), N, 1, 1, L, nk, 2)
        _check_xpk(got, X.axis0_xpk_ref(spec_a, work_b, N, 1, L, nk, 2), N)
        res.append(got)
    assert np.array_equal(res[0][4], res[2][4])
    if big[1] <= 254:
        assert np.array_equal(res[0][3].view(np.uint64), res[2][3].view(np.uint64))
