"""Plain-numpy references for the bispectrum of gridded maps (csrc/bfgx_bispec.hpp): no GPU, nothing of the library.

  bins_of       the k-bin of every mode of the full cube, by the rule of include/bfgx.h ("bispectrum")
  fields        the filtered fields I_i (unit: U_i) through np.fft.fftn / ifftn
  estimator     the FFT estimator's sums from those fields, and abs_sum, the scale every tolerance is stated against
  brute         the direct sum over pairs of modes, the third fixed by closure, in long double: shares no transform with the estimator
  three_waves   a map of three plane waves whose wavevectors close, and the closed form of its one triangle

Units: F = np.fft.fftn(map), unnormalised; all sums are divided by N^3 once."""
import functools

import numpy as np


def wavenumbers(N):
    """integer wavevector components fftfreq(N) N per axis: 0, 1, .., N/2 - 1, -N/2, .., -1"""
    i = np.arange(N, dtype=np.int64)
    return np.where(i < N // 2, i, i - N)


def n2_cube(N):
    n = wavenumbers(N)
    return n[:, None, None] ** 2 + n[None, :, None] ** 2 + n[None, None, :] ** 2


def bins_of(N, L, edges):
    """bin of every mode [N][N][N], -1 outside: edges[i] <= 2 pi / L sqrt(n^2) < edges[i + 1]"""
    edges = np.asarray(edges, dtype=np.float64)
    k = 2 * np.pi / L * np.sqrt(n2_cube(N).astype(np.float64))
    b = np.searchsorted(edges, k, side='right') - 1
    b[(b < 0) | (b >= edges.size - 1)] = -1
    return b


def fields(x, L, edges, unit):
    """complex [nbins][N][N][N]: I_i = ifftn(F [k in i]) N^3, or U_i from a spectrum of ones; real up to rounding"""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    b = bins_of(N, L, edges)
    F = np.ones(x.shape, dtype=np.complex128) if unit else np.fft.fftn(x)
    return np.stack([np.fft.ifftn(np.where(b == i, F, 0.0)) * float(N) ** 3 for i in range(len(edges) - 1)])


def _sum_ld(a):
    return float(np.sum(a.astype(np.longdouble)))


def estimator(x, L, edges, tris):
    """dict of b_sum[ntri], n_tri[ntri], abs_sum[ntri], pk_sum[nbins], n_modes[nbins] from the filtered fields (products in fp64, sums
    in long double)"""
    N = np.asarray(x).shape[0]
    I = fields(x, L, edges, 0).real
    U = fields(x, L, edges, 1).real
    n3 = float(N) ** 3
    tris = np.asarray(tris).reshape(-1, 3)
    out = {'b_sum': np.array([_sum_ld(I[i] * I[j] * I[l]) / n3 for i, j, l in tris]),
           'abs_sum': np.array([_sum_ld(np.abs(I[i] * I[j] * I[l])) / n3 for i, j, l in tris]),
           'n_tri': np.array([_sum_ld(U[i] * U[j] * U[l]) / n3 for i, j, l in tris]),
           'pk_sum': np.array([_sum_ld(I[i] * I[i]) / n3 for i in range(len(I))]),
           'n_modes': np.array([_sum_ld(U[i] * U[i]) / n3 for i in range(len(U))])}
    return out


def brute(x, L, edges, tris):
    """dict of b_sum[ntri] (long double sums of F(k1) F(k2) F(k3), k3 = -k1 - k2 mod N, k1 in i, k2 in j, k3 in l), n_tri[ntri] (the number of
    such triples, int64), pk_sum[nbins], n_modes[nbins] (int64).  O(modes^2) per pair of bins: affordable to N = 16."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    assert N <= 16
    tris = np.asarray(tris).reshape(-1, 3)
    b = bins_of(N, L, edges).ravel()
    F = np.fft.fftn(x).ravel().astype(np.clongdouble)
    a_, b_, c_ = [v.ravel() for v in np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing='ij')]
    nb = len(edges) - 1
    members = [np.flatnonzero(b == i) for i in range(nb)]
    bsum = np.zeros(len(tris), dtype=np.longdouble)
    cnt = np.zeros(len(tris), dtype=np.int64)
    pairs = {}
    for t, (i, j, l) in enumerate(tris):
        pairs.setdefault((int(i), int(j)), []).append((t, int(l)))
    for (i, j), wanted in pairs.items():
        m2 = members[j]
        for k1 in members[i]:
            k3 = ((-a_[k1] - a_[m2]) % N * N + (-b_[k1] - b_[m2]) % N) * N + (-c_[k1] - c_[m2]) % N
            term = (F[k1] * F[m2] * F[k3]).real
            b3 = b[k3]
            for t, l in wanted:
                hit = b3 == l
                bsum[t] += term[hit].sum()
                cnt[t] += int(hit.sum())
    P = (F.real ** 2 + F.imag ** 2)
    return {'b_sum': bsum.astype(np.float64), 'n_tri': cnt,
            'pk_sum': np.array([float(P[m].sum()) for m in members]), 'n_modes': np.array([m.size for m in members], dtype=np.int64)}


def three_waves(N, n1, n2, A, phi):
    """delta(x) = sum_m A_m cos(2 pi n_m . x / N + phi_m), n_3 = -n_1 - n_2 (the phase reduced as an integer first), and the closed form of
    b_sum of the triangle of the three waves' bins when these differ: 2 (N^3 / 2)^3 A_1 A_2 A_3 cos(phi_1 + phi_2 + phi_3)"""
    n1, n2 = np.asarray(n1, dtype=np.int64), np.asarray(n2, dtype=np.int64)
    ns = [n1, n2, -n1 - n2]
    g = np.arange(N, dtype=np.int64)
    two_pi = 8 * np.arctan(np.longdouble(1))
    x = np.zeros((N, N, N), dtype=np.longdouble)
    for n, a, p in zip(ns, A, phi):
        ph = (n[0] * g[:, None, None] + n[1] * g[None, :, None] + n[2] * g[None, None, :]) % N
        x += a * np.cos(two_pi * ph.astype(np.longdouble) / N + np.longdouble(p))
    closed = 2 * (float(N) ** 3 / 2) ** 3 * A[0] * A[1] * A[2] * np.cos(phi[0] + phi[1] + phi[2])
    return x.astype(np.float64), ns, float(closed)


def bin_of_vector(n, L, edges):
    """the bin of one integer wavevector (-1 outside)"""
    k = 2 * np.pi / L * np.sqrt(np.float64(int(n[0]) ** 2 + int(n[1]) ** 2 + int(n[2]) ** 2))
    i = int(np.searchsorted(np.asarray(edges, dtype=np.float64), k, side='right')) - 1
    return i if 0 <= i < len(edges) - 1 else -1


def closable(edges):
    """every i <= j <= l whose bins can hold a closed triangle, by brute force over the triples: edges[l] < edges[i + 1] + edges[j + 1]"""
    nb = len(edges) - 1
    return [(i, j, l) for i in range(nb) for j in range(nb) for l in range(nb) if i <= j <= l and edges[l] < edges[i + 1] + edges[j + 1]]


# ------------------------------------------------------------------------------------------------- the cases the tests share
L_BOX = 100.0
KF = 2 * np.pi / L_BOX


def half_integer_edges(N, nb=5):
    """nb bins between 0.5 kf and the Nyquist frequency + 0.5 kf (N = 8: 5.5 kf, among the corner modes): edges are (m + 1/2) kf, which no
    mode sits on ((m + 1/2)^2 is no integer)"""
    hi = max(N // 2, nb)
    m = np.unique(np.round(np.linspace(0, hi, nb + 1)).astype(int))
    assert m.size == nb + 1
    return (m + 0.5) * KF


@functools.lru_cache(maxsize=None)
def noise_map(N):
    """x + 0.3 x^2 of Gaussian noise: skewed, so that B != 0"""
    x = np.random.default_rng(7 + N).standard_normal((N, N, N))
    m = x + 0.3 * x * x
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def references(N):
    edges = half_integer_edges(N)
    tris = np.array(closable(edges), dtype=np.int32)
    return edges, tris, estimator(noise_map(N), L_BOX, edges, tris), brute(noise_map(N), L_BOX, edges, tris)


def three_wave_case(N=16):
    edges = half_integer_edges(N)
    n1, n2 = (1, 0, 0), (-3, 2, 1)
    x, ns, closed = three_waves(N, n1, n2, (1.0, 0.7, 1.3), (0.3, -1.1, 0.45))
    bins = sorted(bin_of_vector(n, L_BOX, edges) for n in ns)
    return edges, x, tuple(bins), closed
