"""The bispectrum kernels of csrc/bfgx_bispec.hpp and the inverse slab transforms under them, against tests/bispec_oracle.py and numpy.
Everything goes through the Python entries of engine/fourier.py.

  1. slab inverses (fft_conj_kernel, fft_c2c_strided_kernel<0>, fft_c2r_lines_kernel): noise, one-hot spectra, NaN pad columns, round trips;
     N = 8 .. 1024 on 1 to 3 planes or columns
  2. filtered fields (bispec_select_kernel + the inverse) at N = 8, 16, 64, with a bin of k = 0 alone and one of Nyquist-plane modes alone
  3. the estimator (bispec_triangle_kernel, bispec_finish_kernel) at N = 8, 16 against the brute-force triple sum, at N = 32 against the
     numpy estimator
  4. three plane waves at N = 16: the closed form in one triangle, nothing in the others
  5. bitwise repeats, permuted triangle lists, tensor input, cached setups in the order small, large, small
  6. normalize=True

Bounds.  Transforms: fft_oracle.bound(N) relative to max|ref| (the inverse is the forward recursion on conjugated data).  Sums:
4 log2(N^3) 2^-53 abs_sum, abs_sum = sum_x |I_i I_j I_l| / N^3 from the oracle: three transforms of log2(N^3) butterfly stages and a tree sum.

Measured on the MI355X, max|got - ref| / max|ref|, worst of 1, 2, 3 planes or columns (the bound is 1.8e-15 at N = 8, 4.2e-15 to 5.3e-15 above):
  N                        8        16       64       256      512      1024
  inverse planes, noise    2.2e-16  2.2e-16  3.2e-16  4.7e-16  5.2e-16  5.2e-16
  inverse planes, one-hot  1.7e-16  2.2e-16  4.5e-16  7.8e-16  1.0e-15  1.2e-15
  axis 0 inverse, noise    1.1e-16  2.8e-16  2.5e-16  3.2e-16  3.4e-16  3.7e-16
  axis 0 forward, noise    1.1e-16  2.0e-16  3.4e-16  3.0e-16  4.0e-16  4.0e-16
  planes round trip        3.4e-16  3.7e-16  3.9e-16  4.5e-16  5.3e-16  6.2e-16   (twice the bound allowed)
filtered fields, N = 8, 16, 64: at most 2.6e-16, 3.3e-16, 7.0e-16.
estimator, |b_sum - ref| / abs_sum (and |pk_sum - ref| / pk_sum), worst triangle (bin):
  N = 8   1.3e-16 (2.2e-16), bound 4.0e-15;  N = 16  1.0e-16 (4.2e-16), bound 5.3e-15;  N = 32  5.4e-17 (2.9e-16), bound 6.7e-15;
  N = 64  4.3e-17, bound 8.0e-15.  n_tri differs from the brute-force count by at most 3.6e-12 (N = 8) and 5.8e-11 (N = 16).
three waves: the closed form is met to 4.5e-16 of the triangle's abs_sum, every other triangle holds less than 2.3e-17 of it.
The file takes 17 s, 12 of them the first call's start-up of the runtime."""
import numpy as np
import pytest

import bispec_oracle as B
import fft_oracle as O
from bispec_oracle import KF, L_BOX, half_integer_edges, noise_map, references, three_wave_case

pytestmark = pytest.mark.gpu

SIZES = (8, 16, 64, 256, 512, 1024)
PLANES = (1, 2, 3)


@pytest.fixture(scope='module', autouse=True)
def _release_the_tables():
    yield
    import torch
    from baryonification_amd import _lib
    torch.cuda.synchronize()
    _lib.load().bfgx_cache_clear()


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order='C', copy=True)).to('cuda:0')            # (a copy: the cached maps are read-only)


def _padded(work, pitch, fill=np.nan):
    """complex [..][nz] -> device [..][pitch][2], the pad columns c > N/2 filled with `fill`"""
    out = np.full(work.shape[:-1] + (pitch,), fill + 1j * fill)
    out[..., :work.shape[-1]] = work
    return _dev(out.view(np.float64).reshape(out.shape + (2,)))


def _complex(t):
    return t.cpu().numpy().view(np.complex128)[..., 0]


def _spectrum_noise(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _bound_sum(N):
    return 4 * np.log2(float(N) ** 3) * 2.0 ** -53


# ------------------------------------------------------------------------------------------------- 1. slab inverses
def _run_iplanes(work, N, fill=np.nan):
    """ifft_slab_planes_device on complex [planes][N][N/2 + 1] -> real [planes][N][N]; pad columns `fill`, the output starts as NaN"""
    import torch
    from baryonification_amd import engine
    d = _padded(work, engine.fft_pitch(N), fill)
    out = torch.full((work.shape[0], N, N), float('nan'), dtype=torch.float64, device='cuda:0')
    engine.ifft_slab_planes_device(d.data_ptr(), N, work.shape[0], out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _iplanes_ref(work, N):
    """numpy: unnormalised inverse along the middle axis, then irfft along the last (which ignores Im of the columns 0 and N/2)"""
    return np.fft.irfft(np.fft.ifft(work, axis=1) * N, n=N, axis=2) * N


@pytest.mark.parametrize('planes', PLANES)
@pytest.mark.parametrize('N', SIZES)
def test_inverse_planes_noise_and_nan_pads(gpu, N, planes):
    """every value of the inverse of a noise spectrum (its columns 0 and N/2 complex: their imaginary parts are to be ignored); the pad
    columns hold NaN and must not leak: finite, and bitwise what zero pads give"""
    w = _spectrum_noise((planes, N, N // 2 + 1), 31 * N + planes)
    got = _run_iplanes(w, N)
    ref = _iplanes_ref(w, N)
    err = O.rel_err(got, ref)
    print("inverse planes noise N = %4d planes = %d: %.2e (bound %.2e)" % (N, planes, err, O.bound(N)))
    assert np.isfinite(got).all()
    assert err <= O.bound(N)
    assert np.array_equal(got.view(np.uint64), _run_iplanes(w, N, 0.0).view(np.uint64))


@pytest.mark.parametrize('N', SIZES)
def test_inverse_planes_one_hot(gpu, N):
    """one coefficient (b, c) lit per plane: the plane is a plane wave of amplitude 1 or 2, so a misplaced row or column, a wrong mirror
    image or a wrong sign of the exponent shows at full scale"""
    h = N // 2
    modes = [(0, 0), (1, 0), (0, 1), (N - 1, 1), (h, h), (3, h - 1), (5 % N, h), (h + 1, 2), (N - 2, h - 1)]
    vals = [1.0, 0.6 - 0.8j, 1j]                 # (the modes of the columns 0 and N/2 get a real part: their imaginary part is ignored)
    worst = 0.0
    for s in range(0, len(modes), 3):
        w = np.zeros((3, N, h + 1), dtype=np.complex128)
        for p in range(3):
            b, c = modes[s + p]
            w[p, b, c] = vals[(s + p) % 3]
        got = _run_iplanes(w, N)
        ref = _iplanes_ref(w, N)
        for p in range(3):
            assert np.abs(ref[p]).max() >= 0.5
            err = O.rel_err(got[p], ref[p])
            worst = max(worst, err)
            assert err <= O.bound(N), (modes[s + p], err)
    print("inverse planes one-hot N = %4d: %.2e" % (N, worst))


def _run_axis0(work, N, inverse, fill=np.nan):
    import torch
    from baryonification_amd import engine
    d = _padded(work, engine.fft_pitch(N), fill)
    engine.fft_slab_axis0_device(d.data_ptr(), N, work.shape[1], inverse)
    torch.cuda.synchronize()
    return _complex(d)[:, :, :N // 2 + 1]


@pytest.mark.parametrize('ncols', PLANES)
@pytest.mark.parametrize('N', SIZES)
def test_axis0_forward_and_inverse_noise(gpu, N, ncols):
    w = _spectrum_noise((N, ncols, N // 2 + 1), 17 * N + ncols)
    for inverse, ref in ((1, np.fft.ifft(w, axis=0) * N), (0, np.fft.fft(w, axis=0))):
        got = _run_axis0(w, N, inverse)
        err = O.rel_err(got, ref)
        print("axis 0 %s N = %4d cols = %d: %.2e (bound %.2e)" % ('inverse' if inverse else 'forward', N, ncols, err, O.bound(N)))
        assert np.isfinite(got.view(np.float64)).all()
        assert err <= O.bound(N)
    inv = _run_axis0(w, N, 1)
    assert np.array_equal(np.ascontiguousarray(inv).view(np.uint64), np.ascontiguousarray(_run_axis0(w, N, 1, 0.0)).view(np.uint64))


@pytest.mark.parametrize('N', SIZES)
def test_axis0_inverse_one_hot(gpu, N):
    """row a0 of one column lit: exp(+2 pi i a0 j / N) along the first axis, exactly the conjugate of what the forward pass gives"""
    h = N // 2
    j = np.arange(N, dtype=np.int64)
    for a0, c in ((0, 0), (1, h), (h, 1), (N - 1, 2), (37 % N, h - 1), (h + 1, 0)):
        w = np.zeros((N, 2, h + 1), dtype=np.complex128)
        w[a0, 1, c] = 1.0
        got = _run_axis0(w, N, 1)
        ang = 2 * np.pi * ((a0 * j) % N) / N
        ref = np.zeros_like(w)
        ref[:, 1, c] = np.cos(ang) + 1j * np.sin(ang)
        assert O.rel_err(got, ref) <= O.bound(N), (a0, c)


@pytest.mark.parametrize('planes', PLANES)
@pytest.mark.parametrize('N', SIZES)
def test_planes_round_trip(gpu, N, planes):
    """fft_slab_planes_device then ifft_slab_planes_device: N^2 times the planes (both unnormalised, two axes of length N), within twice
    the bound of one direction"""
    import torch
    from baryonification_amd import engine
    x = np.random.default_rng(5 * N + planes).standard_normal((planes, N, N))
    d = _dev(x)
    work = torch.full((planes, N, engine.fft_pitch(N), 2), float('nan'), dtype=torch.float64, device='cuda:0')
    back = torch.full((planes, N, N), float('nan'), dtype=torch.float64, device='cuda:0')
    engine.fft_slab_planes_device(d.data_ptr(), N, planes, work.data_ptr())
    engine.ifft_slab_planes_device(work.data_ptr(), N, planes, back.data_ptr())
    torch.cuda.synchronize()
    err = O.rel_err(back.cpu().numpy(), x * float(N) ** 2)
    print("round trip N = %4d planes = %d: %.2e (bound %.2e)" % (N, planes, err, 2 * O.bound(N)))
    assert err <= 2 * O.bound(N)


@pytest.mark.parametrize('N', [8, 16, 64])
def test_full_round_trip(gpu, N):
    """all three axes of a whole box, forward and back: N^3 times the map (N^2 per plane pass times the N planes of the first axis)"""
    import torch
    from baryonification_amd import engine
    x = np.random.default_rng(N).standard_normal((N, N, N))
    d = _dev(x)
    work = torch.full((N, N, engine.fft_pitch(N), 2), float('nan'), dtype=torch.float64, device='cuda:0')
    back = torch.empty((N, N, N), dtype=torch.float64, device='cuda:0')
    engine.fft_slab_planes_device(d.data_ptr(), N, N, work.data_ptr())
    engine.fft_slab_axis0_device(work.data_ptr(), N, N, 0)
    spec = _complex(work)[:, :, :N // 2 + 1]
    assert O.rel_err(spec, np.fft.rfftn(x)) <= O.bound(N)
    engine.fft_slab_axis0_device(work.data_ptr(), N, N, 1)
    engine.ifft_slab_planes_device(work.data_ptr(), N, N, back.data_ptr())
    torch.cuda.synchronize()
    assert O.rel_err(back.cpu().numpy(), x * float(N) ** 3) <= 2 * O.bound(N)


# ------------------------------------------------------------------------------------------------- 2. filtered fields
def field_edges(N):
    """six bins: k = 0 alone; two thin ones; up to the Nyquist frequency; the corner modes below ny; and [ny, ny + 1) kf, which holds modes
    with a Nyquist component alone (every mode beyond sqrt(3) (N/2 - 1) kf has one)"""
    ny = np.ceil(np.sqrt(3.0) * (N // 2 - 1)) + 0.5
    return np.array([0.0, 0.5, 1.5, 2.5, N // 2 + 0.5, ny, ny + 1.0]) * KF


@pytest.mark.parametrize('unit', [0, 1])
@pytest.mark.parametrize('N', [8, 16, 64])
def test_shell_fields(gpu, N, unit):
    import torch
    from baryonification_amd import engine
    x = np.random.default_rng(3 * N).standard_normal((N, N, N)) + 0.25
    edges = field_edges(N)
    nb = edges.size - 1
    bins = B.bins_of(N, L_BOX, edges)
    h = N // 2
    n = B.wavenumbers(N)
    nyq = (np.abs(n)[:, None, None] == h) | (np.abs(n)[None, :, None] == h) | (np.abs(n)[None, None, :] == h)
    assert (bins == 0).sum() == 1 and bins[0, 0, 0] == 0                                       # k = 0 alone
    assert (bins == nb - 1).sum() >= 1 and nyq[bins == nb - 1].all()                            # Nyquist-plane modes alone
    pitch = engine.fft_pitch(N)
    spec = _padded(np.fft.rfftn(x), pitch)
    keep = spec.clone()
    scratch = torch.full((N, N, pitch, 2), float('nan'), dtype=torch.float64, device='cuda:0')
    out = torch.full((nb, N, N, N), float('nan'), dtype=torch.float64, device='cuda:0')
    engine.bispectrum_shell_fields_device(spec.data_ptr(), N, L_BOX, edges, unit, scratch.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    ref = B.fields(x, L_BOX, edges, unit).real
    assert np.isfinite(got).all()
    assert np.array_equal(spec.cpu().numpy().view(np.uint64), keep.cpu().numpy().view(np.uint64))      # the spectrum is kept, NaN pads and all
    errs = [O.rel_err(got[i], ref[i]) for i in range(nb)]
    print("shell fields N = %3d unit = %d: %s (bound %.2e)" % (N, unit, ' '.join('%.1e' % e for e in errs), O.bound(N)))
    assert max(errs) <= O.bound(N)


# ------------------------------------------------------------------------------------------------- 3. the estimator
def _raw(Map, edges, tris, N):
    """bispectrum_device on a host map: (b_sum, n_tri, pk_sum, n_modes); outputs and work start as NaN"""
    import torch
    from baryonification_amd import engine
    nb, ntri = len(edges) - 1, len(tris)
    d = _dev(Map)
    work = torch.full((engine.bispectrum_work_doubles(N, nb),), float('nan'), dtype=torch.float64, device='cuda:0')
    res = [torch.full((n,), float('nan'), dtype=torch.float64, device='cuda:0') for n in (ntri, ntri, nb, nb)]
    engine.bispectrum_device(d.data_ptr(), N, L_BOX, edges, tris, work.data_ptr(), *[r.data_ptr() for r in res])
    torch.cuda.synchronize()
    return [r.cpu().numpy() for r in res]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize('N', [8, 16])
def test_estimator_against_brute_force(gpu, N):
    edges, tris, est, bru = references(N)
    b_sum, n_tri, pk_sum, n_modes = _raw(noise_map(N), edges, tris, N)
    err = np.abs(b_sum - bru['b_sum']) / est['abs_sum']
    epk = np.abs(pk_sum - bru['pk_sum']) / bru['pk_sum']
    print("estimator N = %2d: %d triangles, b_sum %.2e, pk_sum %.2e of the scale (bound %.2e); n_tri off by %.1e at most"
          % (N, len(tris), err.max(), epk.max(), _bound_sum(N), np.abs(n_tri - bru['n_tri']).max()))
    assert err.max() <= _bound_sum(N)
    assert epk.max() <= _bound_sum(N)
    assert np.array_equal(np.rint(n_tri).astype(np.int64), bru['n_tri'])
    assert np.array_equal(np.rint(n_modes).astype(np.int64), bru['n_modes'])


def test_estimator_against_numpy_at_32(gpu):
    N = 32
    edges = half_integer_edges(N)
    tris = np.array(B.closable(edges), dtype=np.int32)
    est = B.estimator(noise_map(N), L_BOX, edges, tris)
    b_sum, n_tri, pk_sum, n_modes = _raw(noise_map(N), edges, tris, N)
    err = np.abs(b_sum - est['b_sum']) / est['abs_sum']
    epk = np.abs(pk_sum - est['pk_sum']) / est['pk_sum']
    print("estimator N = 32: %d triangles, b_sum %.2e, pk_sum %.2e of the scale (bound %.2e)" % (len(tris), err.max(), epk.max(), _bound_sum(N)))
    assert err.max() <= _bound_sum(N)
    assert epk.max() <= _bound_sum(N)
    counts = np.bincount(B.bins_of(N, L_BOX, edges).ravel() + 1, minlength=len(edges))[1:]
    assert np.array_equal(np.rint(n_modes).astype(np.int64), counts)
    assert np.array_equal(np.rint(n_tri).astype(np.int64), np.rint(est['n_tri']).astype(np.int64))
    assert np.abs(n_tri - np.rint(n_tri)).max() <= 1e-6 * n_tri.max()


# terms = ntri + 5 diagonal sums.  Up to 256 terms a thread of bispec_triangle_kernel<1> owns one over a share of the points (1, 3, 59:
# groups of 8, 8 and 64 threads; 251: all 256 threads); beyond, the instantiations <2> .. <33> own that many terms per thread: both sides
# of every switch, and the longest list there is
TERMS_PER_THREAD = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 28)
LIST_LENGTHS = (1, 3, 59) + tuple(256 * t - 5 + d for t in TERMS_PER_THREAD for d in (0, 1)) + (8192,)


@pytest.mark.parametrize('ntri', LIST_LENGTHS)
def test_triangle_list_lengths(gpu, ntri):
    """lists of every length at which the triangle kernel changes its instantiation or its thread groups, at N = 8: the closable triangles
    repeated, with their three indices in rotating order (the product is symmetric, its rounding is not)"""
    N = 8
    edges, tris, est, bru = references(N)
    pick = np.arange(ntri) % len(tris)
    order = np.array([(0, 1, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0), (0, 2, 1), (1, 0, 2)])[(np.arange(ntri) // len(tris)) % 6]
    long_list = np.take_along_axis(tris[pick], order, axis=1).astype(np.int32)
    b_sum, n_tri, pk_sum, n_modes = _raw(noise_map(N), edges, long_list, N)
    err = np.abs(b_sum - bru['b_sum'][pick]) / est['abs_sum'][pick]
    assert err.max() <= _bound_sum(N), (int(np.argmax(err)), err.max())
    assert np.array_equal(np.rint(n_tri).astype(np.int64), bru['n_tri'][pick])
    assert np.array_equal(np.rint(n_modes).astype(np.int64), bru['n_modes'])
    assert (np.abs(pk_sum - bru['pk_sum']) / bru['pk_sum']).max() <= _bound_sum(N)


# ------------------------------------------------------------------------------------------------- 4. three plane waves
def test_three_waves(gpu):
    N = 16
    edges, x, tri, closed = three_wave_case(N)
    tris = np.array(B.closable(edges), dtype=np.int32)
    at = [tuple(t) for t in tris].index(tri)
    scale = B.estimator(x, L_BOX, edges, tris)['abs_sum'][at]
    b_sum = _raw(x, edges, tris, N)[0]
    bound = _bound_sum(N) * scale
    print("three waves: |b_sum - closed form| = %.2e, others at most %.2e of the triangle's scale (bound %.2e)"
          % (abs(b_sum[at] - closed) / scale, np.abs(np.delete(b_sum, at)).max() / scale, _bound_sum(N)))
    assert abs(b_sum[at] - closed) <= bound
    assert np.abs(np.delete(b_sum, at)).max() <= bound


# ------------------------------------------------------------------------------------------------- 5. reproducibility and layout
def test_repeats_permutations_and_tensor_input(gpu):
    from baryonification_amd import engine
    N = 16
    edges, tris, est, _ = references(N)
    first = _raw(noise_map(N), edges, tris, N)
    again = _raw(noise_map(N), edges, tris, N)
    for a, b in zip(first, again):
        assert np.array_equal(_bits(a), _bits(b))
    perm = np.random.default_rng(2).permutation(len(tris))
    mixed = _raw(noise_map(N), edges, tris[perm], N)
    assert np.abs(mixed[0] - first[0][perm]).max() <= (_bound_sum(N) * est['abs_sum'][perm]).max()
    assert (np.abs(mixed[0] - first[0][perm]) <= _bound_sum(N) * est['abs_sum'][perm]).all()
    assert np.array_equal(np.rint(mixed[1]), np.rint(first[1][perm]))
    # the public entry: a numpy map goes through the host entry, a tensor is analysed where it lies; same kernels, same bits
    host = engine.bispectrum(noise_map(N), L_BOX, edges)
    dev = engine.bispectrum(_dev(noise_map(N)), L_BOX, edges)
    assert np.array_equal(host['triangles'], tris) and np.array_equal(host['k'], 0.5 * (edges[:-1] + edges[1:]))
    for key in ('B', 'n_tri', 'pk', 'n_modes'):
        assert isinstance(dev[key], np.ndarray)
        assert np.array_equal(_bits(host[key]), _bits(dev[key])), key
    assert np.array_equal(_bits(host['B']), _bits(first[0] / first[1]))
    assert np.array_equal(_bits(host['pk']), _bits(first[2] / first[3]))


def test_cached_setups_small_large_small(gpu):
    """N = 16, N = 64, N = 16 on setups that stay cached: the second N = 16 call gives the bits of the first (the dynamic-LDS attribute of the
    strided kernel was set again by the N = 64 setup in between; those of this file's kernels are set once, to their maximum)"""
    import torch
    from baryonification_amd import _lib
    torch.cuda.synchronize()
    _lib.load().bfgx_cache_clear()
    edges16, tris16, _, _ = references(16)
    first = _raw(noise_map(16), edges16, tris16, 16)
    edges64 = half_integer_edges(64)
    tris64 = np.array(B.closable(edges64), dtype=np.int32)
    big = _raw(noise_map(64), edges64, tris64, 64)
    # (N = 64: 2048 chunks of points on at most 512 workgroups, so each strides over several)
    est64 = B.estimator(noise_map(64), L_BOX, edges64, tris64)
    err = np.abs(big[0] - est64['b_sum']) / est64['abs_sum']
    print("estimator N = 64: %d triangles, b_sum %.2e of the scale (bound %.2e)" % (len(tris64), err.max(), _bound_sum(64)))
    assert err.max() <= _bound_sum(64)
    assert (np.rint(big[3]) == np.bincount(B.bins_of(64, L_BOX, edges64).ravel() + 1, minlength=6)[1:]).all()
    assert np.array_equal(np.rint(big[1]), np.rint(est64['n_tri']))
    third = _raw(noise_map(16), edges16, tris16, 16)
    for a, b in zip(first, third):
        assert np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------- 6. normalize
def test_normalize(gpu):
    from baryonification_amd import engine
    N = 16
    edges = half_integer_edges(N)
    raw = engine.bispectrum(noise_map(N), L_BOX, edges, triangles='isosceles')
    nrm = engine.bispectrum(noise_map(N), L_BOX, edges, triangles='isosceles', normalize=True)
    assert np.array_equal(raw['triangles'], engine.bispectrum_triangles(edges, 'isosceles'))
    assert np.array_equal(nrm['B'], raw['B'] * (L_BOX ** 6 / float(N) ** 9))
    assert np.array_equal(nrm['pk'], raw['pk'] * (L_BOX ** 3 / float(N) ** 6))
    assert np.array_equal(_bits(nrm['n_tri']), _bits(raw['n_tri']))


def test_two_threads_with_their_own_triangle_lists(gpu):
    """the packed terms of a call are uploaded from a copy of the call's own: two threads on one cached N = 16 setup, each four calls
    with a list of its own (one triangle; all triangles of the first 3 bins), meet the brute-force sums of their list.  The sums are
    atomic, so they are held to test_estimator_against_brute_force's tolerance, not to the bit."""
    import threading
    N = 16
    edges, tris, est, bru = references(N)
    tris = np.asarray(tris)
    lists = [np.array([len(tris) // 2]), np.flatnonzero((tris < 3).all(axis=1))]
    assert len(lists[0]) == 1 and len(lists[1]) > 1
    Map = noise_map(N)
    gate, got = threading.Barrier(2), [[], []]

    def calls(t):
        gate.wait()
        for _ in range(4):
            got[t].append(_raw(Map, edges, tris[lists[t]], N))

    threads = [threading.Thread(target=calls, args=(t,)) for t in range(2)]
    for th in threads: th.start()
    for th in threads: th.join()
    for t in range(2):
        sel = lists[t]
        assert len(got[t]) == 4
        for b_sum, n_tri, pk_sum, n_modes in got[t]:
            assert (np.abs(b_sum - bru['b_sum'][sel]) / est['abs_sum'][sel]).max() <= _bound_sum(N)
            assert (np.abs(pk_sum - bru['pk_sum']) / bru['pk_sum']).max() <= _bound_sum(N)
            assert np.array_equal(np.rint(n_tri).astype(np.int64), bru['n_tri'][sel])
            assert np.array_equal(np.rint(n_modes).astype(np.int64), bru['n_modes'])
