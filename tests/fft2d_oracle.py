"""Plain-numpy references for csrc/bfgx_fft2d.hpp and utils/flatsky.py (no GPU, nothing of the library): everything on the FULL plane of
np.fft.fft2, so the half-spectrum bookkeeping of the kernels (mirror weights, pad columns, conjugation trick) is not shared.

  coeff_ld                  one coefficient F[a, c] of a real plane in long double, two matrix-vector products, any N
  cross_power_spectrum_ref  the k-bins, mirror weights and windows of the 3-D rule with the third index at 0, sums in long double
  beam_*, smoothing_ref     the three isotropic filters
  ks_factors, kappa_to_shear, shear_to_kappa   the Kaiser-Squires pair with the Nyquist rule
  chain_ld                  forward, product, inverse in long double on a whole plane: what the chain tolerances are measured against

Tolerances of tests/test_gpu_fft2d.py (max|got - ref| / max|ref|), measured by tests/test_fft2d_host.py and recorded here:
  bound(N)        one transform: fft_oracle.bound(N) up to 1024; above, MARGIN x numpy's own error against coeff_ld on 8 sampled modes
  chain_bound(N)  forward, product, inverse: MARGIN x numpy's double-precision chain against chain_ld on whole planes, measured at
                  N = 8, 16, 64, 256; above 256 the 256 figure times log2(N) / 8 (both sides are O(eps log N) recursions)"""
import functools

import numpy as np

import fft_oracle as O

MARGIN = O.MARGIN

# numpy's rfft2-route error against coeff_ld on sampled_modes(N) of seeded noise, relative to the largest sampled |F|
# (test_fft2d_host.py measures them again and holds them within 1.5x)
NUMPY_ERR_SAMPLED = {2048: 4.0e-16, 4096: 3.0e-16}
# numpy's chain error (the worst of the identity and the two Kaiser-Squires products) against chain_ld, relative to max|ref|
NUMPY_CHAIN_ERR = {8: 2.3e-16, 16: 2.8e-16, 64: 3.5e-16, 256: 3.5e-16}


def bound(N):
    if N <= 1024:
        return O.bound(N)
    return MARGIN * NUMPY_ERR_SAMPLED[N]


def chain_bound(N):
    if N <= 256:
        return MARGIN * NUMPY_CHAIN_ERR[min(n for n in NUMPY_CHAIN_ERR if n >= N)]
    return MARGIN * NUMPY_CHAIN_ERR[256] * np.log2(N) / 8.0


# ------------------------------------------------------------------------------------------------- single coefficients, long double
def _w(N, k):
    """exp(-2 pi i j k / N), j < N, in long double; the integer product is reduced before cos / sin see it"""
    ang = 8 * np.arctan(np.longdouble(1)) * ((np.arange(N, dtype=np.int64) * int(k)) % N).astype(np.longdouble) / np.longdouble(N)
    return np.cos(ang), -np.sin(ang)


def coeff_ld(x, a, c):
    """F[a, c] = sum_ij x[i, j] exp(-2 pi i (a i + c j) / N) = (w_a @ x) @ w_c of a real plane, as a complex long double"""
    x = np.asarray(x, dtype=np.longdouble)
    N = x.shape[0]
    ar, ai = _w(N, a)
    cr, ci = _w(N, c)
    ur, ui = ar @ x, ai @ x
    return np.clongdouble(ur @ cr - ui @ ci) + 1j * np.clongdouble(ur @ ci + ui @ cr)


def sampled_modes(N):
    """8 modes with the indices 0, 1, N/2 - 1 and N/2 on each axis, and two seeded ones"""
    h = N // 2
    rng = np.random.default_rng(2000 + N)
    extra = [(int(rng.integers(2, N)), int(rng.integers(2, h - 1))) for _ in range(2)]
    return [(0, 0), (1, 1), (h - 1, h), (h, h - 1), (0, h), (h, 0)] + extra


def noise(N, seed=0):
    return np.random.default_rng(3000 + 7 * N + seed).standard_normal((N, N))


@functools.lru_cache(maxsize=None)
def numpy_error_sampled(N):
    """numpy's own error on sampled_modes(N) of noise(N), relative to the largest sampled |F|"""
    x = noise(N)
    got = np.fft.fft(np.fft.rfft(x, axis=1), axis=0)
    ref = np.array([coeff_ld(x, a, c) for a, c in sampled_modes(N)])
    g = np.array([got[a, c] for a, c in sampled_modes(N)]).astype(np.clongdouble)
    return float(np.abs(g - ref).max() / np.abs(ref).max())


# ------------------------------------------------------------------------------------------------- whole planes, long double
def fft2_ld(x):
    return O.dft_ld(O.dft_ld(np.asarray(x), axis=1), axis=0)


def ifft2_ld(F):
    N = F.shape[0]
    Wp = O._dft_matrix(N, +1)
    return (Wp @ (F @ Wp)) / np.longdouble(N * N)


def chain_ld(x, mult):
    """real(ifft2(fft2(x) * mult)) in long double, mult a real full-plane factor"""
    assert x.shape[0] <= O.LD_WHOLE_PLANES_MAX_N
    return ifft2_ld(fft2_ld(x) * np.asarray(mult).astype(np.longdouble)).real


def chain_np(x, mult):
    return np.fft.ifft2(np.fft.fft2(x) * mult).real


@functools.lru_cache(maxsize=None)
def numpy_chain_error(N):
    """the worst of numpy's chain errors against chain_ld over the identity and the two Kaiser-Squires factors, on noise(N)"""
    x = noise(N)
    c2, s2 = ks_factors(N)
    worst = 0.0
    for mult in (np.ones((N, N)), c2, s2):
        worst = max(worst, O.rel_err(chain_np(x, mult), chain_ld(x, mult)))
    return worst


# ------------------------------------------------------------------------------------------------- k-bins on the full plane
def wave_numbers(N):
    """fftfreq's integer wave numbers; the Nyquist index is -N/2"""
    return np.fft.fftfreq(N, 1.0 / N).astype(np.int64)


def window_table(N, p):
    """t[i] = s(n_i)^(-2p), s(n) = sin(pi n / N) / (pi n / N), in long double, rounded once"""
    n = wave_numbers(N).astype(np.longdouble)
    x = 4 * np.arctan(np.longdouble(1)) * n / np.longdouble(N)
    with np.errstate(invalid='ignore', divide='ignore'):
        s = np.where(n == 0, np.longdouble(1), np.sin(x) / np.where(n == 0, 1, x))
    return (1 / s ** (2 * p)).astype(np.float64)


def mode_k_and_bin(N, L, nk, reciprocal=False):
    """|k| and bin of every mode of the full plane [a][c]: k = sqrt(klin[a]^2 + klin[c]^2), floor of the TRUE quotient (or, for the
    comparison of the two rules, of the product with the reciprocal of the bin width)"""
    kbins, klin = O.k_axes(N, L, nk)
    k = np.sqrt(klin[:, None] ** 2 + klin[None, :] ** 2)
    dk = kbins[1] - kbins[0]
    q = (k - kbins[0]) * (1.0 / dk) if reciprocal else (k - kbins[0]) / dk
    return k, np.floor(q).astype(np.int64)


def edge_disagreements(N, L, nk):
    """(modes of the plane whose two floors differ, modes that sit exactly on a bin edge)"""
    kbins, _ = O.k_axes(N, L, nk)
    k, true = mode_k_and_bin(N, L, nk)
    _, recip = mode_k_and_bin(N, L, nk, reciprocal=True)
    q = (k - kbins[0]) / (kbins[1] - kbins[0])
    return int((true != recip).sum()), int((q == np.rint(q)).sum())


def binned(FA, FB, L, nk, p=0):
    """per-bin means of w |F_A|^2, w |F_B|^2, w Re(F_A conj F_B) and k, and the counts, over the full plane of two spectra [N][N]"""
    N = FA.shape[0]
    k, kinds = mode_k_and_bin(N, L, nk)
    win = window_table(N, p)
    w = win[:, None] * win[None, :]
    m = (kinds >= 0) & (kinds < nk)
    order = np.argsort(kinds[m], kind='stable')
    sel = kinds[m][order]
    counts = np.bincount(sel, minlength=nk).astype(np.int64)
    sums = [O._bin_sums(sel, v[m][order], nk) for v in (w * (FA.real ** 2 + FA.imag ** 2), w * (FB.real ** 2 + FB.imag ** 2),
                                                        w * (FA.real * FB.real + FA.imag * FB.imag), k)]
    with np.errstate(divide='ignore', invalid='ignore'):
        paa, pbb, pab, kc = (s / counts for s in sums)
        r = pab / np.sqrt(paa * pbb)
    return {'k': kc, 'paa': paa, 'pbb': pbb, 'pab': pab, 'r': r, 'counts': counts}


def cross_power_spectrum_ref(A, B, L, nk, p=0, normalize=False):
    N = A.shape[0]
    out = binned(np.fft.fft2(A), np.fft.fft2(B), L, nk, p)
    if normalize:
        for key in ('paa', 'pbb', 'pab'):
            out[key] = out[key] * (L * L / float(N) ** 4)
    return out


def one_hot_ref(N, L, nk, a, c, p=0):
    """what the binning gives for the half spectrum that is 1 at (a, c), c <= N/2, and 0 elsewhere: (bin or None, the sum of w m |F|^2,
    the sum of m k, the count m)"""
    k, kinds = mode_k_and_bin(N, L, nk)
    win = window_table(N, p)
    b = int(kinds[a, c])
    mult = 2 if 0 < c < N // 2 else 1
    return (b if 0 <= b < nk else None), mult * win[a] * win[c], mult * k[a, c], mult


# ------------------------------------------------------------------------------------------------- filters
def k_plane(N, L):
    n = wave_numbers(N).astype(np.float64)
    return 2 * np.pi / L * np.sqrt(n[:, None] ** 2 + n[None, :] ** 2)


def beam_gauss(k, sigma):
    return np.exp(-0.5 * (k * sigma) ** 2)


def beam_tophat(k, R):
    from scipy.special import j1
    x = k * R
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(x > 0, 2 * j1(x) / np.where(x > 0, x, 1.0), 1.0)


def beam_table(k, tk, tb):
    return np.interp(k, tk, tb)


def smoothing_ref(x, L, beam):
    """real(ifft2(fft2(x) beam(k)))"""
    return chain_np(x, beam(k_plane(x.shape[0], L)))


# ------------------------------------------------------------------------------------------------- Kaiser-Squires
def ks_factors(N):
    """(c2, s2) on the full plane: (n0^2 - n1^2, 2 n0 n1) / (n0^2 + n1^2), 0 at the zero mode, s2 = 0 in the Nyquist row and column"""
    n = wave_numbers(N).astype(np.float64)
    n0, n1 = n[:, None], n[None, :]
    d = n0 * n0 + n1 * n1
    with np.errstate(invalid='ignore', divide='ignore'):
        c2 = np.where(d > 0, (n0 * n0 - n1 * n1) / np.where(d > 0, d, 1.0), 0.0)
        s2 = np.where(d > 0, 2 * n0 * n1 / np.where(d > 0, d, 1.0), 0.0)
    s2[N // 2, :] = 0.0
    s2[:, N // 2] = 0.0
    return c2, s2


def kappa_to_shear(kappa):
    c2, s2 = ks_factors(kappa.shape[0])
    F = np.fft.fft2(kappa)
    return np.fft.ifft2(c2 * F).real, np.fft.ifft2(s2 * F).real


def shear_to_kappa(g1, g2):
    c2, s2 = ks_factors(g1.shape[0])
    F1, F2 = np.fft.fft2(g1), np.fft.fft2(g2)
    return np.fft.ifft2(c2 * F1 + s2 * F2).real, np.fft.ifft2(-s2 * F1 + c2 * F2).real


# ------------------------------------------------------------------------------------------------- the Gaussian bump
BUMP = dict(N=128, L=128.0, sigma=3.0, centre=(40, 77), M=2e15, eps=5.0, redshift=0.2, edges=np.concatenate([[0.0], np.geomspace(1.0, 12.0, 10)]))
# test_fft2d_host.py: the largest |mean_t - <kappa_bar(<r) - kappa(r)>| over the rings, relative to the largest |mean_t| (periodic images
# and the sampling of the rings), and the largest |mean_x|, as found there
BUMP_RESIDUAL_T = 1.1e-5
BUMP_RESIDUAL_X = 6.1e-18


def bump_maps():
    """(bins, kappa, gamma_t_analytic): a periodic Gaussian convergence bump centred on a pixel centre, and the analytic tangential shear
    kappa_bar(<d) - kappa(d) of the isolated bump at every pixel's (minimum-image) distance"""
    b = BUMP
    N, L, s = b['N'], b['L'], b['sigma']
    bins = (np.arange(N) + 0.5) * L / N
    dx = bins - bins[b['centre'][0]]
    dy = bins - bins[b['centre'][1]]
    dx = np.where(dx > L / 2, dx - L, np.where(dx < -L / 2, dx + L, dx))
    dy = np.where(dy > L / 2, dy - L, np.where(dy < -L / 2, dy + L, dy))
    d2 = dx[:, None] ** 2 + dy[None, :] ** 2
    kappa = np.exp(-d2 / (2 * s * s))
    with np.errstate(invalid='ignore', divide='ignore'):
        kbar = np.where(d2 > 0, 2 * s * s / np.where(d2 > 0, d2, 1.0) * -np.expm1(-d2 / (2 * s * s)), 1.0)
    return bins, kappa, kbar - kappa


def bump_catalog(bins):
    b = BUMP
    return {'M': np.array([b['M']]), 'x': np.array([bins[b['centre'][0]]]), 'y': np.array([bins[b['centre'][1]]]), 'z': np.zeros(1)}
