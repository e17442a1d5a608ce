"""Plain-numpy references for csrc/bfgx_fft.hpp, one Fourier coefficient at a time (no GPU, nothing of the library).

  dft_ld         direct DFT in long double (eps 1.08e-19 on x86): the yardstick numpy's FFT and the kernels are both measured with
  planes_ref     what the plane passes (r2c along the last axis, c2c along the middle one) must deliver
  axis0_pk_ref   what the binned axis-0 pass must deliver for a block of columns: sums of |F|^2 and |k| and counts per linear k-bin,
                 bins exactly as oracle/grid.py:power_spectrum computes them
  numpy_error    numpy's own error against dft_ld, the figure the GPU bound is built on (bound = MARGIN * that)

Everything here is O(N^2) per line on purpose: the references share no recursion, radix or twiddle table with what they check."""
import functools

import numpy as np

MARGIN = 16                       # a second fp64 implementation of the same O(eps log N) recursion, other radices and twiddles
NUMPY_ERR_RECORDED = 3.3e-16      # numpy's 2-D error at N = 1024 (test_fft_oracle_host.py measures it again and holds it below 5e-16)
LD_WHOLE_PLANES_MAX_N = 256       # a whole plane in long double: 0.02 s at 64, 0.3 s at 256, of the order of a minute at 1024


@functools.lru_cache(maxsize=None)
def _dft_matrix(N, sign=-1):
    """W[j, k] = exp(sign 2 pi i ((j k) mod N) / N) in long double; the integer product is reduced before cos / sin see it"""
    jk = (np.arange(N, dtype=np.int64)[:, None] * np.arange(N, dtype=np.int64)[None, :]) % N
    ang = 8 * np.arctan(np.longdouble(1)) * jk.astype(np.longdouble) / np.longdouble(N)                   # 2 pi ((j k) mod N) / N
    W = np.empty((N, N), dtype=np.clongdouble)
    W.real = np.cos(ang)
    W.imag = sign * np.sin(ang)
    W.setflags(write=False)
    return W


def dft_ld(x, axis=-1):
    """F[k] = sum_j x[j] exp(-2 pi i j k / N) along `axis`, in np.clongdouble"""
    x = np.moveaxis(np.asarray(x).astype(np.clongdouble), axis, -1)
    F = x @ _dft_matrix(x.shape[-1])
    return np.moveaxis(F, -1, axis)


def planes_ref(slab, exact=None):
    """The half spectrum [planes][N][N/2 + 1] of real planes [planes][N][N]: transformed along the last axis (kept for c <= N/2), then
    along the middle one.  exact: long double throughout (default where a whole plane is affordable), else numpy's FFT."""
    slab = np.asarray(slab, dtype=np.float64)
    N = slab.shape[-1]
    if exact is None:
        exact = N <= 128
    if not exact:
        return np.fft.fft(np.fft.rfft(slab, axis=2), axis=1)
    assert N <= LD_WHOLE_PLANES_MAX_N
    return dft_ld(dft_ld(slab, axis=2)[:, :, :N // 2 + 1], axis=1)


def rel_err(got, ref):
    """max|got - ref| / max|ref|, in long double"""
    ref = np.asarray(ref).astype(np.clongdouble)
    return float(np.abs(np.asarray(got).astype(np.clongdouble) - ref).max() / np.abs(ref).max())


@functools.lru_cache(maxsize=None)
def numpy_error(N, ndim=2):
    """numpy's own error against dft_ld on seeded Gaussian noise, relative to max|F|.  ndim = 1: 16 lines; ndim = 2: one plane through
    planes_ref's numpy route, whole up to N = 256, above that on 8 sampled columns c of the half spectrum (a column of the 2-D
    transform is one matrix-vector product per axis)."""
    rng = np.random.default_rng(1000 + N)
    if ndim == 1:
        x = rng.standard_normal((16, N)) + 1j * rng.standard_normal((16, N))
        return rel_err(np.fft.fft(x, axis=1), dft_ld(x, axis=1))
    x = rng.standard_normal((1, N, N))
    got = planes_ref(x, exact=False)
    if N <= LD_WHOLE_PLANES_MAX_N:
        return rel_err(got, planes_ref(x, exact=True))
    cols = np.unique(np.concatenate([[0, 1, N // 2 - 1, N // 2], rng.integers(2, N // 2 - 1, 4)]))
    W = _dft_matrix(N)
    ref = W @ (x[0].astype(np.clongdouble) @ W[:, cols])               # [k1][sampled c]
    return float(np.abs(got[0][:, cols].astype(np.clongdouble) - ref).max() / np.abs(ref).max())


def bound(N):
    """What a kernel's max|got - ref| / max|ref| is held to at grid size N: MARGIN x numpy's own error against long double, measured
    up to N = 256 and taken from the record above that"""
    return MARGIN * (numpy_error(N) if N <= LD_WHOLE_PLANES_MAX_N else NUMPY_ERR_RECORDED)


# ------------------------------------------------------------------------------------------------- analytic plane spectra
def _two_pi_ld():
    return 8 * np.arctan(np.longdouble(1))


def impulse_ref(N, i0, j0):
    """Half spectrum [N][N/2 + 1] of the plane that is 1 at (i0, j0) and 0 elsewhere: exp(-2 pi i (i0 k1 + j0 c) / N), modulus 1 everywhere"""
    k1 = np.arange(N, dtype=np.int64)[:, None]
    c = np.arange(N // 2 + 1, dtype=np.int64)[None, :]
    ang = _two_pi_ld() * ((i0 * k1 + j0 * c) % N).astype(np.longdouble) / N
    return np.cos(ang) - 1j * np.sin(ang)


@functools.lru_cache(maxsize=None)
def plane_wave(N, p, q):
    """cos(2 pi (p i + q j) / N) on the plane [i][j], the argument reduced as an integer first (cached, read-only)"""
    i = np.arange(N, dtype=np.int64)[:, None]
    j = np.arange(N, dtype=np.int64)[None, :]
    x = np.cos(_two_pi_ld() * ((p * i + q * j) % N).astype(np.longdouble) / N).astype(np.float64)
    x.setflags(write=False)
    return x


def plane_wave_ref(N, p, q):
    """Its half spectrum, exact: N^2 / 2 at (p, q) and at (-p, -q) mod N (N^2 where the two coincide), kept where c <= N/2"""
    F = np.zeros((N, N), dtype=np.float64)
    F[p % N, q % N] += 0.5 * N * N
    F[-p % N, -q % N] += 0.5 * N * N
    return F[:, :N // 2 + 1]


# ------------------------------------------------------------------------------------------------- k-bins, the oracle's rule
def k_axes(N, L, nk):
    """(kbins, klin) as oracle/grid.py:power_spectrum builds them"""
    kbins = np.linspace(2 * np.pi / L, 2 * np.pi / L * N / 2, nk + 1)
    klin = np.fft.fftfreq(N, 1 / (2 * np.pi / (L)) / N)
    return kbins, klin


def mode_k_and_bin(N, L, nk, a, b, c):
    """|k| and k-bin of the modes (a, b, c) (arrays broadcast): the oracle's summation order ka^2 + kc^2 + kb^2 and floor of the TRUE
    quotient.  Bins outside [0, nk) are returned as they come; the caller masks."""
    kbins, klin = k_axes(N, L, nk)
    k = np.sqrt(klin[a] ** 2 + klin[c] ** 2 + klin[b] ** 2)
    return k, np.floor((k - kbins[0]) / (kbins[1] - kbins[0])).astype(np.int64)


def axis0_pk_ref(work, N, col0, L, nk):
    """work[N][ncols][nz] complex, nz = N/2 + 1 (the columns b = col0 .. col0 + ncols - 1 of the middle axis after the plane passes):
    transform along axis 0, then per linear k-bin (pk_sum, k_sum, counts) over exactly these columns.  Only the half c <= N/2 of
    the spectrum is there; a mode with 0 < c < N/2 stands for itself and for its mirror image (-a, -b, -c), which has the same |k|
    to the bit and, for a real map, the same |F|^2, so it counts twice -- summed over all column blocks this is the full cube."""
    work = np.asarray(work)
    ncols, nz = work.shape[1], work.shape[2]
    assert work.shape[0] == N and nz == N // 2 + 1 and 0 <= col0 and col0 + ncols <= N
    F = np.fft.fft(work, axis=0)
    P = F.real ** 2 + F.imag ** 2
    a = np.arange(N)[:, None, None]
    b = (col0 + np.arange(ncols))[None, :, None]
    c = np.arange(nz)[None, None, :]
    k, kinds = mode_k_and_bin(N, L, nk, a, b, c)
    w = np.broadcast_to(np.where((c > 0) & (c < N // 2), 2, 1), k.shape)
    m = (kinds >= 0) & (kinds < nk)
    order = np.argsort(kinds[m], kind='stable')
    sel = kinds[m][order]
    counts = np.bincount(sel, weights=w[m][order], minlength=nk).astype(np.int64)
    return _bin_sums(sel, (w * P)[m][order], nk), _bin_sums(sel, (w * k)[m][order], nk), counts


def _bin_sums(sorted_bins, values, nk):
    """sum of `values` per bin, added up in long double (the sums of 10^6 terms are then good to 1e-16, not to 1e-13)"""
    out = np.zeros(nk)
    if sorted_bins.size:
        starts = np.flatnonzero(np.r_[True, sorted_bins[1:] != sorted_bins[:-1]])
        out[sorted_bins[starts]] = np.add.reduceat(values.astype(np.longdouble), starts).astype(np.float64)
    return out


ONE_HOT_L = 305.0


def one_hot_modes(N):
    """The (a0, b, c) at which test_gpu_fft.py lights one mode: rows 0, 1, N/2, N - 1, 37, two more odd / even ones, against the
    lines 0, 1, 2, N/4, N/2 - 1, N/2 (N = 1024: also 508 .. 512, the last two 4-line tiles), the column cycling through
    0, 1, N - 1, 3, N/2; then the modes on the three axes at index 1 and at the Nyquist index"""
    a0s = [0, 1, N // 2, N - 1, 37 % N, N // 4 + 1, N - 2]
    cs = [0, 1, N // 2 - 1, N // 2, 2, N // 4] + ([508, 509, 510, 511, 512] if N == 1024 else [])
    bs = [0, 1, N - 1, 3, N // 2]
    modes = [(a0, bs[n % len(bs)], c) for n, (a0, c) in enumerate((a0, c) for a0 in a0s for c in cs)]
    return modes + [(0, 0, N // 2), (N // 2, 0, 0), (0, N // 2, 0), (0, 0, 1), (1, 0, 0), (0, 1, 0)]


def edge_disagreements(N, L, nk):
    """Over the half spectrum: (modes whose floor through the reciprocal of the bin width differs from the floor of the true quotient,
    modes that sit exactly on a bin edge).  A shape with the first figure > 0 is one where pk_bin_of's fallback decides a bin."""
    kbins, _ = k_axes(N, L, nk)
    a = np.arange(N)[:, None, None]
    b = np.arange(N)[None, :, None]
    c = np.arange(N // 2 + 1)[None, None, :]
    k, kinds = mode_k_and_bin(N, L, nk, a, b, c)
    dk = kbins[1] - kbins[0]
    inv = 1.0 / dk
    recip = np.floor((k - kbins[0]) * inv).astype(np.int64)
    q = (k - kbins[0]) / dk
    return int((recip != kinds).sum()), int((q == np.rint(q)).sum())


def counts_by_rule(N, L, nk, reciprocal):
    """Modes per bin over the full cube, binned by the floor of the true quotient or by the floor through the reciprocal alone"""
    kbins, _ = k_axes(N, L, nk)
    i = np.arange(N)
    k, kinds = mode_k_and_bin(N, L, nk, i[:, None, None], i[None, :, None], i[None, None, :])
    if reciprocal:
        kinds = np.floor((k - kbins[0]) * (1.0 / (kbins[1] - kbins[0]))).astype(np.int64)
    m = (kinds >= 0) & (kinds < nk)
    return np.bincount(kinds[m], minlength=nk)
