"""Plain-numpy references for fft2_der_kernel / mapstats_peaks_grid_kernel and utils/flatstats.py (no GPU, nothing of the library),
everything on the FULL plane of np.fft.fft2 so that the half-spectrum bookkeeping of the kernels is not shared:

  multipliers        the six complex factors of [u, u_x, u_y, u_xx, u_xy, u_yy] (or of the spin form) with the Nyquist rule
  derivatives        real(ifft2(fft2(x) m b)) in double precision; derivatives_complex keeps the imaginary parts (the Nyquist rule's test)
  derivatives_large  the same one map at a time for the sizes above 1024: the full plane at 2048, numpy's own rfft2 / irfft2 at 4096
  derivatives_ld     the same chain in long double (fft2d_oracle.fft2_ld / ifft2_ld), complex multipliers
  scales             S_a = max|m_a b| max|x|: what an error of map a is stated in
  wave, wave_derivatives   u = cos(2 pi (m0 i + m1 j) / N + phi) and its analytic derivatives
  peaks              extrema of a square grid by np.roll (periodic) or slicing (not periodic); plateau: the integer-valued map
  minkowski          the sums through minkowski_oracle.minkowski(..., spin_form=True)

Tolerances of tests/test_gpu_flatstats.py.  A high-k multiplier amplifies the rounding of the forward transform into maps whose true
values may be small (u_yy of the wave (N/2 - 1, 2) is off by 2e-12 of its own maximum in numpy, by 8e-15 of S_a), so errors are relative
to S_a, not to the output's own maximum.  NUMPY_DER_ERR[N] is numpy's double-precision chain against derivatives_ld, the worst of the six
multipliers on fft2d_oracle.noise(N) and on the wave (N/2 - 1, 2), measured by tests/test_flatstats_host.py and recorded here;
der_bound(N) = fft_oracle.MARGIN (16: a second fp64 implementation of the same recursion) times that figure, above 256 the 256 figure
times log2(N) / 8 (fft2d_oracle.chain_bound's rule)."""
import functools

import numpy as np

import fft_oracle as O
import fft2d_oracle as F
import mapstats_oracle as M
import minkowski_oracle as K

MARGIN = O.MARGIN
NAMES = ('u', 'u_x', 'u_y', 'u_xx', 'u_xy', 'u_yy')
SPIN_NAMES = ('u', 'u_x', 'u_y', 'lap', 'q_plus', 'q_cross')

# numpy's chain error per N, relative to S_a (test_flatstats_host.py measures them again and holds them within 1.5x)
NUMPY_DER_ERR = {8: 2.3e-16, 16: 2.8e-16, 64: 4.5e-16, 256: 5.6e-16}


def waves(N):
    """the four plane waves of the tests: (m0, m1) fixes the signs, the axes and the factor 2 pi / L"""
    return [(3, 5), (0, 7), (-4, 0), (N // 2 - 1, 2)]


def der_bound(N):
    if N <= 256:
        return MARGIN * NUMPY_DER_ERR[min(n for n in NUMPY_DER_ERR if n >= N)]
    return MARGIN * NUMPY_DER_ERR[256] * np.log2(N) / 8.0


# ------------------------------------------------------------------------------------------------- multipliers
def _factors(N, L, ncols):
    """g0 [N][1], g1 [1][ncols] = 2 pi / L times fftfreq's integer wave numbers (the first ncols of axis 1), and the same with the
    Nyquist index zeroed (o0, o1): what the factors that are odd in an index are built from"""
    n = F.wave_numbers(N).astype(np.float64)
    kv = 2 * np.pi / L
    g0, g1 = (kv * n)[:, None], (kv * n)[None, :ncols]
    h = N // 2
    o0, o1 = g0.copy(), g1.copy()
    o0[h, :] = 0.0
    if ncols > h:
        o1[:, h] = 0.0
    return g0, g1, o0, o1


def _multiplier(a, fac, spin_form):
    g0, g1, o0, o1 = fac
    one = np.ones((g0.shape[0], g1.shape[1]))
    if a == 0:
        return one + 0j
    if a == 1:
        return 1j * o0 * one
    if a == 2:
        return 1j * o1 * one
    if spin_form:
        return (-(g0 * g0 + g1 * g1), -(g0 * g0 - g1 * g1), -2.0 * o0 * o1)[a - 3] + 0j
    return (-(g0 * g0) * one, -(o0 * o1), -(g1 * g1) * one)[a - 3] + 0j


def multipliers(N, L, spin_form=False):
    """complex [6][N][N]: with n0 (axis 0, x) and n1 (axis 1, y) fftfreq's integer wave numbers, kv = 2 pi / L and h = N / 2,
    1, i kv n0 (0 where a == h), i kv n1 (0 where c == h), -kv^2 n0^2, -kv^2 n0 n1 (0 where a == h or c == h), -kv^2 n1^2;
    spin_form: the last three are -kv^2 (n0^2 + n1^2), -kv^2 (n0^2 - n1^2), -2 kv^2 n0 n1 (the last with u_xy's zero rule)"""
    fac = _factors(N, L, N)
    return np.stack([_multiplier(a, fac, spin_form) for a in range(6)])


def beam_plane(N, L, kind='unit', param=0.0, table=None):
    k = F.k_plane(N, L)
    if kind == 'unit':
        return np.ones((N, N))
    if kind == 'gauss':
        return F.beam_gauss(k, param)
    if kind == 'tophat':
        return F.beam_tophat(k, param)
    return F.beam_table(k, *table)


def derivatives_complex(x, L, beam=None, spin_form=False):
    N = x.shape[0]
    b = np.ones((N, N)) if beam is None else beam
    return np.fft.ifft2(np.fft.fft2(x)[None] * (multipliers(N, L, spin_form) * b[None]), axes=(1, 2))


def derivatives(x, L, beam=None, spin_form=False):
    """float64 [6][N][N]"""
    return np.ascontiguousarray(derivatives_complex(x, L, beam, spin_form).real)


def derivatives_large(x, L, beam=None, spin_form=False, half=False):
    """(maps [6][N][N], S_a [6]) for the sizes above 1024, one map at a time to bound the memory.  half=False: the full plane of
    np.fft.fft2, as derivatives (N = 2048; beam [N][N]).  half=True: numpy's own half-plane pair rfft2 / irfft2, a quarter of the work
    (N = 4096, where the full plane takes 8 s; beam [N][N/2 + 1]; test_flatstats_host.py holds this route to the full plane at the
    small sizes)"""
    N = x.shape[0]
    fac = _factors(N, L, N // 2 + 1 if half else N)
    Fx = np.fft.rfft2(x) if half else np.fft.fft2(x)
    if beam is not None:
        Fx = Fx * beam
    out, S = np.empty((6, N, N)), np.empty(6)
    for a in range(6):
        m = _multiplier(a, fac, spin_form)
        S[a] = np.abs(m if beam is None else m * beam).max() * np.abs(x).max()
        out[a] = np.fft.irfft2(Fx * m, s=(N, N)) if half else np.fft.ifft2(Fx * m).real
    return out, S


def derivatives_ld(x, L, beam=None, spin_form=False, which=range(6)):
    """the same in long double; the multipliers are the double-precision ones, so the two chains differ in the transforms' arithmetic alone"""
    N = x.shape[0]
    assert N <= O.LD_WHOLE_PLANES_MAX_N
    b = np.ones((N, N)) if beam is None else beam
    m = multipliers(N, L, spin_form) * b[None]
    Fx = F.fft2_ld(x)
    return np.stack([F.ifft2_ld(Fx * m[a].astype(np.clongdouble)).real for a in which])


def scales(x, L, beam=None, spin_form=False):
    """S_a = max|m_a b| max|x|, a < 6"""
    N = x.shape[0]
    b = np.ones((N, N)) if beam is None else beam
    return np.abs(multipliers(N, L, spin_form) * b[None]).reshape(6, -1).max(1) * np.abs(x).max()


@functools.lru_cache(maxsize=None)
def numpy_der_error(N, L=10.0):
    """the worst over the six multipliers, on noise(N) and on the wave (N/2 - 1, 2), of numpy's chain against the long-double chain,
    relative to S_a"""
    worst = 0.0
    for x in (F.noise(N), wave(N, N // 2 - 1, 2)):
        got, ref, S = derivatives(x, L), derivatives_ld(x, L), scales(x, L)
        for a in range(6):
            worst = max(worst, float(np.abs(got[a].astype(np.longdouble) - ref[a]).max() / S[a]))
    return worst


# ------------------------------------------------------------------------------------------------- plane waves
def _phase(N, m0, m1, phi):
    i = np.arange(N, dtype=np.int64)[:, None]
    j = np.arange(N, dtype=np.int64)[None, :]
    return (O._two_pi_ld() * ((m0 * i + m1 * j) % N).astype(np.longdouble) / N + np.longdouble(phi))


def wave(N, m0, m1, phi=0.0):
    """cos(2 pi (m0 i + m1 j) / N + phi), the integer part of the argument reduced first"""
    return np.cos(_phase(N, m0, m1, phi)).astype(np.float64)


def wave_derivatives(N, L, m0, m1, phi=0.0):
    """[u, u_x, u_y, u_xx, u_xy, u_yy] of that wave on a patch of side L (x = i L / N, y = j L / N): k = 2 pi m / L"""
    th = _phase(N, m0, m1, phi)
    k0, k1 = 2 * np.pi * m0 / L, 2 * np.pi * m1 / L
    u, s = np.cos(th), np.sin(th)
    return np.stack([u, -k0 * s, -k1 * s, -k0 * k0 * u, -k0 * k1 * u, -k1 * k1 * u]).astype(np.float64)


def impulse(N, i0, j0):
    x = np.zeros((N, N))
    x[i0, j0] = 1.0
    return x


# ------------------------------------------------------------------------------------------------- extrema of a grid
OFFSETS = [(di, dj) for di in (-1, 0, 1) for dj in (-1, 0, 1) if (di, dj) != (0, 0)]


def good_2d(m, mask=None):
    m = np.asarray(m, dtype=np.float64)
    return M.good(m.ravel(), None if mask is None else np.asarray(mask).ravel()).reshape(m.shape)


def peaks(m, edges, mask=None, periodic=True):
    """({'maxima': int64 [nb], 'minima': int64 [nb]}, flags int8 [n][n]): strictly above / below all 8 neighbours, all 9 pixels good;
    periodic: neighbours by np.roll; not periodic: interior pixels by slicing, border pixels never"""
    m = np.asarray(m, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    n = m.shape[0]
    g = good_2d(m, mask)
    with np.errstate(invalid='ignore'):
        if periodic:
            elig, gt, lt = g.copy(), np.ones((n, n), bool), np.ones((n, n), bool)
            for di, dj in OFFSETS:
                w, gw = np.roll(m, (-di, -dj), (0, 1)), np.roll(g, (-di, -dj), (0, 1))       # w[i, j] = m[i + di, j + dj]
                elig &= gw
                gt &= m > w
                lt &= m < w
        else:
            elig, gt, lt = np.zeros((n, n), bool), np.zeros((n, n), bool), np.zeros((n, n), bool)
            c = (slice(1, n - 1), slice(1, n - 1))
            elig[c], gt[c], lt[c] = g[c], True, True
            for di, dj in OFFSETS:
                s = (slice(1 + di, n - 1 + di), slice(1 + dj, n - 1 + dj))
                elig[c] &= g[s]
                gt[c] &= m[c] > m[s]
                lt[c] &= m[c] < m[s]
    flags = np.where(elig & gt, 1, np.where(elig & lt, -1, 0)).astype(np.int8)
    out = {}
    for name, sign in (('maxima', 1), ('minima', -1)):
        v = m[flags == sign]
        b = np.searchsorted(edges, v, side='right') - 1                  # edges[b] <= v < edges[b + 1]
        b = b[(b >= 0) & (b < edges.size - 1)]
        out[name] = np.bincount(b, minlength=edges.size - 1).astype(np.int64)
    return out, flags


def plateau(n=8):
    """integer values on a flat background of 1s: a 2 x 2 plateau of 9s (no extremum: strictness), a single 8 at (5, 5) (a maximum), a
    single -5 at (5, 2) (a minimum); n >= 8"""
    m = np.ones((n, n))
    m[1:3, 1:3] = 9.0
    m[5, 5] = 8.0
    m[5, 2] = -5.0
    return m


def min_neighbour_gap(m):
    """the smallest |m[p] - m[q]| over all pairs of (periodic) neighbours"""
    return min(float(np.abs(m - np.roll(m, (-di, -dj), (0, 1))).min()) for di, dj in OFFSETS)


# ------------------------------------------------------------------------------------------------- Minkowski sums
def minkowski(ders, edges, mask=None):
    """minkowski_oracle.minkowski of six maps [6][N][N] in spin form"""
    d = np.asarray(ders, dtype=np.float64)
    return K.minkowski(d.reshape(6, -1), edges, None if mask is None else np.asarray(mask).ravel(), spin_form=True)
