"""The LDS FFT and P(k) kernels of csrc/bfgx_fft.hpp, one Fourier coefficient at a time, N = 8 .. 1024, against tests/fft_oracle.py
(plain numpy, long double where it is affordable).  Everything goes through the Python entries of engine/fourier.py.

  1. plane passes (fft_r2c_lines_kernel + fft_c2c_strided_kernel<0>): noise, impulses, plane waves, NaN-filled pad columns
  2. axis-0 pass with binning (fft_c2c_strided_kernel<1 | 2>, pk_table_build_kernel, pk_table_sums_kernel) on synthetic spectra,
     one-hot spectra that pin every mode to its (a, b, c), a repeated call on a cached table
  3. bin edges through engine.power_spectrum at shapes where the reciprocal floor and the division floor differ
     (test_fft_oracle_host.py shows that they do)
  4. cached setups called in the order large, small, large (the dynamic-LDS attribute is per instantiation, the setups per shape)
  5. the shared Fourier host code: one owner of the attributes across the 2-D and 3-D families, the lazy bin table built once by two
     threads, one release of all five caches

Bound (fft_oracle.bound): max|got - ref| / max|ref| <= 16 x numpy's own error against the long-double DFT at the same N, i.e. about
5e-15.  Both are O(eps log N) fp64 recursions with other radices and twiddle sources; 16 is the margin the mode-coupling tests give a
second fp64 implementation.

Measured on the MI355X, max|got - ref| / max|ref| of the plane passes, worst of planes = 1, 2, 3 (the bound is 1.8e-15 at N = 8, 3e-15 to
5.3e-15 above):
  N          8        16       32       64       128      256      512      1024
  noise      2.9e-16  2.6e-16  2.6e-16  2.6e-16  3.3e-16  4.7e-16  4.7e-16  5.4e-16
  impulse    2.3e-16  2.7e-16  2.7e-16  3.6e-16  5.4e-16  6.9e-16  7.2e-16  8.7e-16
  wave       1.1e-16  1.1e-16  7.5e-17  7.9e-17  1.1e-16  1.1e-16  1.1e-16  5.8e-17
binned axis-0 pass, |F|^2 sums per bin against long-double sums: at most 1.4e-15 (N = 1024, nk = 255), mostly 3e-16 to 1e-15.
Large, small, large: every instantiation has its dynamic-LDS attribute set once per device to the most any shape asks of it; all
calls return and repeat their results.  The file takes 21 s, 12 of them the first call's start-up of the runtime.

Not covered: a full 1024^3 power_spectrum (17 GB of scratch): the slab entries run the same kernels at
N = 1024 on a few planes or columns."""
import numpy as np
import pytest

import fft_oracle as O

pytestmark = pytest.mark.gpu

SIZES = (8, 16, 32, 64, 128, 256, 512, 1024)
PLANES = (1, 2, 3)


@pytest.fixture(scope='module', autouse=True)
def _release_the_bin_tables():
    """the setups of this file hold two 0.5 GB bin tables (N = 1024): hand them back when the file is done"""
    yield
    import torch
    from baryonification_amd import _lib
    torch.cuda.synchronize()
    _lib.load().bfgx_cache_clear()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


def _run_planes(slab, fill=float('nan')):
    """fft_slab_planes_device on real planes [planes][N][N] -> complex [planes][N][pitch]; work pre-filled with `fill`"""
    import torch
    from baryonification_amd import engine
    planes, N = slab.shape[0], slab.shape[1]
    pitch = engine.fft_pitch(N)
    assert pitch % 8 == 0 and N // 2 + 1 <= pitch < N // 2 + 1 + 8
    d = _dev(slab)
    work = torch.full((planes, N, pitch, 2), fill, dtype=torch.float64, device='cuda:0')
    engine.fft_slab_planes_device(d.data_ptr(), N, planes, work.data_ptr())
    torch.cuda.synchronize()
    return work.cpu().numpy().view(np.complex128)[..., 0]


def _noise(N, planes):
    return np.random.default_rng(100 * N + planes).standard_normal((planes, N, N))


# ------------------------------------------------------------------------------------------------- 1. plane passes
@pytest.mark.parametrize('planes', PLANES)
@pytest.mark.parametrize('N', SIZES)
def test_planes_noise(gpu, N, planes):
    """(a) every coefficient of Gaussian-noise planes; planes = 1 and 3 pair lines of the r2c pass across a plane boundary (N <= 512)"""
    x = _noise(N, planes)
    got = _run_planes(x)[:, :, :N // 2 + 1]
    ref = O.planes_ref(x)
    err = O.rel_err(got, ref)
    print("planes noise N = %4d planes = %d: %.2e (bound %.2e, numpy itself %.2e)" % (N, planes, err, O.bound(N), O.bound(N) / O.MARGIN))
    assert np.isfinite(got.view(np.float64)).all()
    assert err <= O.bound(N)


@pytest.mark.parametrize('planes', PLANES)
@pytest.mark.parametrize('N', SIZES)
def test_planes_pad_columns_never_leak(gpu, N, planes):
    """(d) work pre-filled with NaN: the columns c <= N/2 are finite and bitwise what a zero-filled work gives (no atomics in these passes).
    The last tile of a row holds pad lines (N = 1024: 4-line tiles inside an 8-padded pitch)."""
    x = _noise(N, planes)
    nz = N // 2 + 1
    a = _run_planes(x, float('nan'))[:, :, :nz]
    b = _run_planes(x, 0.0)[:, :, :nz]
    assert np.isfinite(a.view(np.float64)).all()
    assert np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _impulse_positions(N):
    return [(0, 0), (1, 0), (0, 1), (N - 1, N - 1), (N // 2, 3)]


@pytest.mark.parametrize('planes', PLANES)
@pytest.mark.parametrize('N', SIZES)
def test_planes_impulse(gpu, N, planes):
    """(b) one voxel set: the answer is a pure phase of modulus 1 at every (k1, c), so a permuted, dropped or leaked coefficient shows at
    full scale.  Every position is run in every plane slot; the planes of one call carry different positions."""
    pos = _impulse_positions(N)
    refs = [O.impulse_ref(N, i0, j0) for (i0, j0) in pos]
    worst = 0.0
    for s in range(len(pos)):
        x = np.zeros((planes, N, N))
        idx = [(s + p) % len(pos) for p in range(planes)]
        for p, i in enumerate(idx):
            x[p, pos[i][0], pos[i][1]] = 1.0
        got = _run_planes(x)[:, :, :N // 2 + 1]
        for p, i in enumerate(idx):
            err = O.rel_err(got[p], refs[i])
            worst = max(worst, err)
            assert err <= O.bound(N), (pos[i], p, err)
    print("planes impulse N = %4d planes = %d: %.2e" % (N, planes, worst))


def _waves(N):
    return [(0, 0), (1, 0), (0, 1), (N // 2, N // 2), (N - 1, 1), (3, N // 2 - 1), (5 % N, N // 2)]


@pytest.mark.parametrize('planes', PLANES)
@pytest.mark.parametrize('N', SIZES)
def test_planes_plane_wave(gpu, N, planes):
    """(c) cos(2 pi (p i + q j) / N): one or two coefficients are N^2 / 2 (or N^2), every other one is below the bound times the peak.
    This pins the index of each coefficient, which no binned test sees."""
    waves = _waves(N)
    worst = 0.0
    for s in range(len(waves)):
        idx = [(s + p) % len(waves) for p in range(planes)]
        x = np.stack([O.plane_wave(N, *waves[i]) for i in idx])
        got = _run_planes(x)[:, :, :N // 2 + 1]
        for p, i in enumerate(idx):
            ref = O.plane_wave_ref(N, *waves[i])
            assert ref.max() in (0.5 * N * N, 1.0 * N * N)
            err = O.rel_err(got[p], ref)
            worst = max(worst, err)
            assert err <= O.bound(N), (waves[i], p, err)
    print("planes wave    N = %4d planes = %d: %.2e" % (N, planes, worst))


# ------------------------------------------------------------------------------------------------- 2. axis-0 pass with binning
def _run_axis0(work_dev, N, ncols, col0, L, nk):
    """fft_slab_axis0_pk_device on a device tensor [N][ncols][pitch][2] -> (pk_sum, k_sum, counts); the outputs start as garbage"""
    import torch
    from baryonification_amd import engine
    sums = torch.full((2, nk), float('nan'), dtype=torch.float64, device='cuda:0')
    cnt = torch.full((nk,), -1, dtype=torch.int64, device='cuda:0')
    engine.fft_slab_axis0_pk_device(work_dev.data_ptr(), N, ncols, col0, L, nk, sums[0].data_ptr(), sums[1].data_ptr(), cnt.data_ptr())
    torch.cuda.synchronize()
    s = sums.cpu().numpy()
    return s[0], s[1], cnt.cpu().numpy()


def _synthetic_work(N, ncols, seed):
    """complex work [N][ncols][N/2 + 1] whose transform along axis 0 has moduli in [1, 2] and random phases: with every |F| within a
    factor 2 of the largest, an error bounded relative to max|F| is bounded relative to each |F|^2 as well, also in a bin of one mode"""
    rng = np.random.default_rng(seed)
    nz = N // 2 + 1
    F = rng.uniform(1.0, 2.0, (N, ncols, nz)) * np.exp(2j * np.pi * rng.uniform(0, 1, (N, ncols, nz)))
    return np.fft.ifft(F, axis=0)


def _padded(work, pitch):
    """[N][ncols][nz] -> device [N][ncols][pitch][2], the pad columns c > N/2 NaN"""
    out = np.full(work.shape[:2] + (pitch,), np.nan + 1j * np.nan)
    out[:, :, :work.shape[2]] = work
    return _dev(out.view(np.float64).reshape(out.shape + (2,)))


TWO_PI = 2 * np.pi
# (N, nk, L, ncols, col0): every N with the table (nk <= 254) and with per-mode binning, nk = 1 (its own branch in the setup), the
# switch 254 / 255, the maximum 2048; col0 = 0, 1, N/2, N - ncols; N = 1024 with nk = 1, 254, 255, 2048
AXIS0_CASES = [
    (8, 1, 305.0, 1, 0), (8, 2, 1.0, 2, 1), (8, 7, TWO_PI, 3, 5), (8, 254, 305.0, 1, 4), (8, 255, 1.0, 2, 0), (8, 2048, TWO_PI, 3, 1),
    (16, 7, 305.0, 3, 0), (16, 2, 1.0, 2, 8), (16, 255, TWO_PI, 1, 1), (16, 2048, 305.0, 3, 13),
    (64, 1, TWO_PI, 2, 0), (64, 2, 305.0, 3, 61), (64, 254, 1.0, 3, 1), (64, 255, 305.0, 2, 32), (64, 2048, 1.0, 1, 0), (64, 7, 305.0, 1, 63),
    (256, 7, 1.0, 3, 0), (256, 254, TWO_PI, 2, 1), (256, 255, 305.0, 3, 253), (256, 2048, 305.0, 1, 128), (256, 1, 305.0, 2, 254),
    (512, 7, 305.0, 2, 1), (512, 254, 305.0, 3, 0), (512, 255, 1.0, 1, 511), (512, 2048, TWO_PI, 3, 0), (512, 2, TWO_PI, 2, 256),
    (1024, 1, 305.0, 3, 0), (1024, 254, 305.0, 2, 1), (1024, 255, 1.0, 3, 1021), (1024, 2048, 305.0, 1, 0), (1024, 2048, TWO_PI, 3, 1),
    (1024, 254, 305.0, 3, 512),
]


def _check_axis0(got, ref, N):
    (pk, ks, cnt), (rpk, rks, rcnt) = got, ref
    assert np.isfinite(pk).all() and np.isfinite(ks).all()                 # (a NaN pad column that was binned would show here)
    assert np.array_equal(cnt, rcnt)
    full = rcnt > 0
    assert (pk[~full] == 0).all() and (ks[~full] == 0).all()
    if full.any():
        assert np.abs(ks[full] / rks[full] - 1).max() <= 1e-12
        e = np.abs(pk[full] - rpk[full]) / rpk[full]
        assert e.max() <= O.bound(N), (int(np.argmax(e)), e.max())
        return float(e.max())
    return 0.0


@pytest.mark.parametrize('N,nk,L,ncols,col0', AXIS0_CASES)
def test_axis0_pk_synthetic_spectra(gpu, N, nk, L, ncols, col0):
    from baryonification_amd import engine
    work = _synthetic_work(N, ncols, 7 * N + nk + ncols)
    ref = O.axis0_pk_ref(work, N, col0, L, nk)
    d = _padded(work, engine.fft_pitch(N))
    got = _run_axis0(d, N, ncols, col0, L, nk)
    e = _check_axis0(got, ref, N)
    print("axis0 N = %4d nk = %4d L = %-6.4g cols %d @ %4d: %d of %d bins filled, %d modes, pk %.2e" % (N, nk, L, ncols, col0, (ref[2] > 0).sum(), nk, ref[2].sum(), e))
    if nk <= 254:
        # the bins, counts and |k| sums now come from the cached table: bitwise the same; |F|^2 is added by atomics in another order
        again = _run_axis0(d, N, ncols, col0, L, nk)
        assert np.array_equal(again[2], got[2]) and np.array_equal(again[1].view(np.uint64), got[1].view(np.uint64))
        _check_axis0(again, ref, N)


@pytest.mark.parametrize('nk', [254, 2048])
@pytest.mark.parametrize('N', [8, 16, 64, 256, 512, 1024])
def test_axis0_pk_one_hot(gpu, N, nk):
    """work[:, b, c] = exp(2 pi i a0 j / N) for ONE (a0, b, c): that mode carries N^2, every other one nothing.  pk_sum must hold
    weight * N^2 in the reference's bin of (a0, b, c) -- nowhere if the mode lies outside the bins, as most modes with a Nyquist
    index do -- and less than the bound times N^2 in every other bin.  test_fft_oracle_host.py holds the list to enough modes inside
    the bins, among them the axis mode (0, 0, N/2), which rounding puts into the LAST bin at some N and whose weight is 1.  A row misplaced by the permutation of the binned last
    pass, a wrong weight or a table byte read from another [row][line] moves or rescales the one entry."""
    import torch
    from baryonification_amd import engine
    L = O.ONE_HOT_L
    pitch, nz = engine.fft_pitch(N), N // 2 + 1
    j = np.arange(N, dtype=np.int64)
    work = torch.empty((N, 1, pitch, 2), dtype=torch.float64, device='cuda:0')
    for (a0, b, c) in O.one_hot_modes(N):
        ang = 2 * np.pi * ((a0 * j) % N) / N
        work.fill_(float('nan'))
        work[:, 0, :nz, :] = 0.0
        work[:, 0, c, :] = _dev(np.stack([np.cos(ang), np.sin(ang)], axis=1))
        pk, ks, cnt = _run_axis0(work, N, 1, b, L, nk)
        _, bin_ = O.mode_k_and_bin(N, L, nk, a0, b, c)
        exp = np.zeros(nk)
        if 0 <= bin_ < nk:
            exp[bin_] = (2.0 if 0 < c < N // 2 else 1.0) * N * N
        assert np.isfinite(pk).all()
        assert np.abs(pk - exp).max() <= O.bound(N) * N * N, (a0, b, c, int(bin_), np.flatnonzero(pk > 0.5)[:4], pk.max())


# ------------------------------------------------------------------------------------------------- 3. bin edges, public entry
@pytest.mark.parametrize('N,Nk,L', [(32, 15, 305.0), (64, 31, 305.0), (64, 31, 1.0), (64, 62, 1000 / 3), (32, 5, 305.0), (128, 63, TWO_PI),
                                    (16, 1, 305.0), (16, 2, 305.0), (64, 254, 305.0), (64, 255, 305.0)])
def test_power_spectrum_bin_edges(gpu, N, Nk, L):
    """engine.power_spectrum against the oracle where modes sit on bin edges and the floor of (k - k0) * (1 / dk) is not the floor of
    (k - k0) / dk (pk_bin_of's fallback decides), at nk = 1, 2 and on both sides of the table / per-mode switch"""
    from baryonification_amd.engine import power_spectrum
    from oracle import grid as G
    rng = np.random.default_rng(N)
    Map = rng.poisson(4.0, (N, N, N)).astype(np.float64)
    Map[3, 5, 7] += 500.0
    k_cen, Pk, k_c = power_spectrum(Map, L, Nk)
    ok_cen, oPk, ok_c = G.power_spectrum(Map, L, Nk)
    assert np.array_equal(k_c, ok_c)
    good = ok_c > 0
    assert good.any()
    assert np.array_equal(np.isnan(Pk), ~good)
    assert np.abs(Pk[good] / oPk[good] - 1).max() <= 1e-10
    assert np.abs(k_cen[good] / ok_cen[good] - 1).max() <= 1e-12


# ------------------------------------------------------------------------------------------------- 4. large, small, large
def test_cached_plane_setups_large_small_large(gpu):
    """N = 512 and N = 256 share one instantiation of the strided kernel, whose dynamic-LDS attribute the setups set when they are built:
    the cached N = 512 setup must still launch, and give the same bits, after an N = 256 setup was built"""
    import torch
    from baryonification_amd import _lib
    torch.cuda.synchronize()
    _lib.load().bfgx_cache_clear()                      # (both setups are built below, in this order)
    x512, x256 = _noise(512, 2), _noise(256, 2)
    first = _run_planes(x512, 0.0)
    small = _run_planes(x256, 0.0)
    third = _run_planes(x512, 0.0)
    assert np.array_equal(first.view(np.uint64), third.view(np.uint64))
    assert O.rel_err(small[:, :, :129], O.planes_ref(x256)) <= O.bound(256)
    assert O.rel_err(first[:, :, :257], O.planes_ref(x512)) <= O.bound(512)


@pytest.mark.parametrize('big,small', [((1024, 2048), (1024, 255)), ((512, 100), (256, 100))])
def test_cached_binned_setups_large_small_large(gpu, big, small):
    """the same for the binned pass: per-mode binning at N = 1024 with nk = 2048, then nk = 255 (less LDS, same kernel), then 2048 again;
    table binning at N = 512, then N = 256, then 512 again.  L is this test's own, so that all three setups are built here."""
    from baryonification_amd import engine
    L = 77.0
    res = []
    for (N, nk) in (big, small, big):
        work = _synthetic_work(N, 1, N + nk)
        got = _run_axis0(_padded(work, engine.fft_pitch(N)), N, 1, 1, L, nk)
        _check_axis0(got, O.axis0_pk_ref(work, N, 1, L, nk), N)
        res.append(got)
    assert np.array_equal(res[0][2], res[2][2])
    if big[1] <= 254:
        assert np.array_equal(res[0][1].view(np.uint64), res[2][1].view(np.uint64))


# ------------------------------------------------------------------------------------------------- 5. one owner of the attributes, one cache
def _run_rfft2(x):
    """engine.rfft2_device on a real plane [N][N] -> complex [N][N/2 + 1]"""
    import torch
    from baryonification_amd import engine
    N = x.shape[0]
    work = torch.zeros((engine.fft2_work_doubles(N),), dtype=torch.float64, device='cuda:0')
    out = torch.zeros((N, engine.fft_pitch(N), 2), dtype=torch.float64, device='cuda:0')
    engine.rfft2_device(_dev(x).data_ptr(), N, work.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.complex128)[..., 0][:, :N // 2 + 1]


def _clear_caches():
    import torch
    from baryonification_amd import _lib
    torch.cuda.synchronize()
    _lib.load().bfgx_cache_clear()
    return _lib.load().bfgx_debug_live_allocs()


def test_one_attribute_owner_across_families(gpu):
    """The 2-D and the 3-D transforms launch the same instantiations of the strided kernel, and the binned passes ask the most LDS of
    theirs at (1024, nk 2048): in an order that mixes the families and the sizes every call launches, meets its oracle, and repeats its
    bits."""
    from baryonification_amd import engine
    _clear_caches()
    L = 91.0
    m512, m128, p256, p512 = _noise(512, 1)[0], _noise(128, 1)[0], _noise(256, 2), _noise(512, 2)

    def first_three():
        return [_run_rfft2(m512), _run_planes(p256, 0.0)[:, :, :129], _run_planes(p512, 0.0)[:, :, :257]]

    first = first_three()
    for (N, nk) in ((1024, 2048), (1024, 8)):
        work = _synthetic_work(N, 1, N + nk)
        got = _run_axis0(_padded(work, engine.fft_pitch(N)), N, 1, 1, L, nk)
        _check_axis0(got, O.axis0_pk_ref(work, N, 1, L, nk), N)
    small = _run_rfft2(m128)
    again = first_three()
    for a, b in zip(first, again):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))
    assert O.rel_err(first[0], O.planes_ref(m512[None])[0]) <= O.bound(512)
    assert O.rel_err(first[1], O.planes_ref(p256)) <= O.bound(256)
    assert O.rel_err(first[2], O.planes_ref(p512)) <= O.bound(512)
    assert O.rel_err(small, O.planes_ref(m128[None])[0]) <= O.bound(128)


def test_lazy_bin_table_is_built_once_by_two_threads(gpu):
    """two threads make the first binned call of a fresh (64, L, 20) setup at the same time: both meet the oracle, and the library owns
    exactly one setup afterwards -- its twiddles, its k axis and the three buffers of one bin table"""
    import threading
    from baryonification_amd import _lib, engine
    N, L, nk = 64, 123.25, 20
    before = _clear_caches()
    works = [_synthetic_work(N, 2, 900 + t) for t in range(2)]
    devs = [_padded(w, engine.fft_pitch(N)) for w in works]
    gate, got = threading.Barrier(2), [None, None]

    def call(t):
        gate.wait()
        got[t] = _run_axis0(devs[t], N, 2, 3, L, nk)

    threads = [threading.Thread(target=call, args=(t,)) for t in range(2)]
    for th in threads: th.start()
    for th in threads: th.join()
    for t in range(2):
        _check_axis0(got[t], O.axis0_pk_ref(works[t], N, 3, L, nk), N)
    assert _lib.load().bfgx_debug_live_allocs() == before + 5
    assert _clear_caches() == before


def test_one_release_for_all_fourier_caches(gpu):
    """one small call of every family, then bfgx_cache_clear: no device allocation of theirs is left"""
    from baryonification_amd import engine, utils as U
    before = _clear_caches()
    rng = np.random.default_rng(16)
    A, B = rng.standard_normal((16, 16, 16)), rng.standard_normal((16, 16, 16))
    engine.power_spectrum(A, 100.0, 6)
    engine.cross_power_spectrum(A, B, 100.0, 6, window='cic')
    engine.interlaced_power_spectrum(A, B, 100.0, 6)
    engine.bispectrum(A, 100.0, 2 * np.pi / 100.0 * np.array([0.5, 2.5, 4.5, 6.5]))
    U.rfft2(rng.standard_normal((8, 8)))
    U.rfft2(rng.standard_normal((2048, 2048)))
    from baryonification_amd import _lib
    assert _lib.load().bfgx_debug_live_allocs() > before
    assert _clear_caches() == before
