"""High-precision references for the FFTLog path (csrc/bfgx_fftlog.hpp, bfgx_fftlog_api.inc), pinned on the CPU by
tests/test_fftlog_host.py and used on the GPU by tests/test_gpu_fftlog_kernels.py.

  u, ln(k r)   Hamilton 2000 eqs. B18 and B22 (the statement of oracle/fftlog.py) with mpmath.loggamma at 40 digits
  transform    b = reverse(irfft(rfft(f pre) u)) post in long double (eps 1.08e-19; numpy >= 2 keeps longdouble through
               np.fft), 2 pi from a 40-digit string, pre / post / k as long-double powers
  PCHIP        Fritsch-Butland as scipy.interpolate.PchipInterpolator states it, in fractions.Fraction: every sign
               decision and every value is exact
"""
import math
from fractions import Fraction

import mpmath
import numpy as np

LD = np.longdouble
CLD = np.clongdouble
EPS = 2.0 ** -52
TWO_PI = LD('6.283185307179586476925286766559005768394')
MP_DPS = 40
# what the code under test is given over an independent double implementation's worst error: four times it, and at least 8.
# Measured in tests/test_fftlog_host.py: scipy.special.loggamma's route 7.96 (ln|u|); scipy's PchipInterpolator 2.19
K_U = 32.0
K_PCHIP = 8.8

# (dim, mu, plaw) of the issue's grid; q = dim / 2 + plaw, mu_b = mu + 1/2 in 3-D.  (3, 0, -0.5) and (2, 0, -0.5) have q > mu_b:
# the denominator Gamma is evaluated at Re z = 1/4, through the reflection formula
TRIPLES = [(3, 0, -1.5), (3, 0, -2.0), (3, 0, -1.0), (3, 0, -0.5), (2, 0, -1.0), (2, 0, -0.5), (2, 1, -1.0), (3, 2, -1.5)]


def require_longdouble():
    import pytest
    if not np.finfo(LD).eps < 1e-18:
        pytest.skip("np.longdouble is no wider than double here (eps %.3g): no high-precision transform reference" % np.finfo(LD).eps)


def bias(dim, mu, plaw):
    """q, mu_b: the bias exponent and the order of the Bessel function of the underlying Hankel transform"""
    return dim / 2.0 + plaw, (mu + 0.5 if dim == 3 else float(mu))


def dln_of(r):
    """the grid step as the library takes it from r: libm's log, one division"""
    return math.log(r[-1] / r[0]) / (len(r) - 1.0)


def log_grid(n, per_decade, r0=1.0):
    """n points, `per_decade` to the decade, from r0"""
    return r0 * 10.0 ** (np.arange(n) / float(per_decade))


# ---------------------------------------------------------------------------------------------------- u and ln(k r), mpmath
def mp_u(n, dln, mub, q):
    """(lnkr, ln|u_m|, arg u_m, S_m, u_0 is zero, S_lnkr, frac) with lists over m = 0 .. n/2, all mpf.  The Nyquist coefficient of an
    even n is made real (ln|u| and a phase of 0 or pi); u_0 = 0 where the denominator Gamma has a pole.  S_m and S_lnkr are the
    scales of the rounding errors of ln u_m and lnkr (tests/test_fftlog_host.py); frac in (-1/2, 1/2] is lnkr / dln"""
    with mpmath.workdps(MP_DPS):
        dln, mub, q = mpmath.mpf(dln), mpmath.mpf(mub), mpmath.mpf(q)
        xp, xm = (mub + 1 + q) / 2, (mub + 1 - q) / 2
        ln2, pi = mpmath.log(2), mpmath.pi
        y = pi / (2 * dln)
        gp, gm = mpmath.loggamma(mpmath.mpc(xp, y)), mpmath.loggamma(mpmath.mpc(xm, y))
        arg = ln2 / dln + (gp.imag + gm.imag) / pi
        frac = arg - mpmath.nint(arg)
        lnkr = frac * dln
        s_lnkr = dln * (1 + ln2 / dln + (abs(gp) + abs(gm)) / pi)
        lnmod, phase, S = [], [], []
        zero0 = xm <= 0 and xm == mpmath.nint(xm)
        for m in range(n // 2 + 1):
            ym = pi * m / (n * dln)
            if m == 0 and zero0:
                lnmod.append(mpmath.ninf); phase.append(mpmath.mpf(0)); S.append(mpmath.mpf(1))
                continue
            gp, gm = mpmath.loggamma(mpmath.mpc(xp, ym)), mpmath.loggamma(mpmath.mpc(xm, ym))
            lm = q * ln2 + gp.real - gm.real
            ph = 2 * ym * (ln2 - lnkr) + gp.imag + gm.imag
            if n % 2 == 0 and m == n // 2:                    # made real: u = |u| cos(phase)
                c = mpmath.cos(ph)
                lm, ph = lm + mpmath.log(abs(c)), (mpmath.mpf(0) if c > 0 else pi)
            lnmod.append(lm); phase.append(ph)
            S.append(1 + abs(q) * ln2 + abs(gp) + abs(gm) + abs(2 * ym * (ln2 - lnkr)))
        return lnkr, lnmod, phase, S, zero0, s_lnkr, frac


def u_errors(u, lnkr, ref):
    """worst |ln|u| - ref| / (2^-52 S_m), worst |arg u - ref mod 2 pi| / (2^-52 S_m), |lnkr - ref| / (2^-52 S_lnkr) of complex double
    coefficients u[n/2 + 1] and a double lnkr against ref = mp_u(...)"""
    lnkr_ref, lnmod, phase, S, zero0, s_lnkr, _ = ref
    worst_mod = worst_ph = 0.0
    with mpmath.workdps(MP_DPS):
        for m in range(len(lnmod)):
            um = complex(u[m])
            if m == 0 and zero0:
                assert um == 0, "u_0 must be 0 on a pole of the denominator Gamma"
                continue
            if not (np.isfinite(um.real) and np.isfinite(um.imag)) or um == 0:
                return np.inf, np.inf, np.inf
            z = mpmath.mpc(um.real, um.imag)
            e_mod = abs(mpmath.log(abs(z)) - lnmod[m])
            d = (mpmath.arg(z) - phase[m]) / (2 * mpmath.pi)
            e_ph = abs(d - mpmath.nint(d)) * 2 * mpmath.pi
            worst_mod = max(worst_mod, float(e_mod / (EPS * S[m])))
            worst_ph = max(worst_ph, float(e_ph / (EPS * S[m])))
        e_k = float(abs(mpmath.mpf(lnkr) - lnkr_ref) / (EPS * s_lnkr)) if np.isfinite(lnkr) else np.inf
    return worst_mod, worst_ph, e_k


# ---------------------------------------------------------------------------------------------------- the discrete transform
def stage_factors(r, dim, mu, plaw, lnkr):
    """pre, post, k of one _fftlog_transform in long double, for a given ln(k r)"""
    q, _ = bias(dim, mu, plaw)
    r = np.asarray(r, dtype=np.float64).astype(LD)
    k = np.exp(LD(lnkr)) / r[::-1]
    if dim == 3:
        pre = r ** LD(1.5 - q)
        post = (TWO_PI * k) ** LD(-1.5) * k ** LD(-q)
    else:
        pre = r ** LD(1.0 - q)
        post = k ** LD(-(1.0 + q)) / TWO_PI
    return pre, post, k


MUTATIONS = ('nyquist dropped', 'nyquist sign flipped', 'mtop one short', 'not reversed')


def ld_fht(a, u, mutation=None):
    """reverse(irfft(rfft(a) u)) of the rows of a, in long double; u complex [n/2 + 1].  `mutation` states one of the mistakes a
    kernel of this shape can make (the two Nyquist ones exist for even n only)"""
    a = np.atleast_2d(np.asarray(a, dtype=LD))
    n = a.shape[-1]
    B = np.fft.rfft(a, axis=-1)
    assert B.dtype == CLD, "np.fft does not keep long double here"
    B = B * np.asarray(u, dtype=CLD)
    nh = n // 2
    if mutation in ('nyquist dropped', 'nyquist sign flipped'):
        assert n % 2 == 0
        B[:, nh] = 0 if mutation == 'nyquist dropped' else -B[:, nh]
    elif mutation == 'mtop one short':
        B[:, nh - 1 if n % 2 == 0 else nh] = 0
    c = np.fft.irfft(B, n, axis=-1)
    assert c.dtype == LD
    return c if mutation == 'not reversed' else c[:, ::-1]


def ld_fht_direct(a, u):
    """the same by direct sums (rows of a short): the statement the kernel implements, for pinning ld_fht"""
    a = np.atleast_2d(np.asarray(a, dtype=LD))
    n = a.shape[-1]
    nh = n // 2
    j = np.arange(n)
    ang = TWO_PI * ((np.outer(np.arange(nh + 1), j) % n).astype(LD) / LD(n))
    E = np.cos(ang) - 1j * np.sin(ang)                                           # [m][j]
    B = (a.astype(CLD) @ E.T) * np.asarray(u, dtype=CLD)
    w = np.full(nh + 1, 2, dtype=LD)
    w[0] = 1
    B = B.copy()
    if n % 2 == 0:
        w[nh] = 1
        B[:, nh] = B[:, nh].real
    B[:, 0] = B[:, 0].real
    c = ((B * w) @ np.conj(E)).real / LD(n)                                      # sum_m w_m Re(B_m e^{+i ang})
    return c[:, ::-1]


def fht_bound(f, pre, u, post, ref, extra_A=0.0):
    """the forward-error bound of fht_rows_kernel per element (see tests/test_gpu_fftlog_kernels.py):
    (2 n + 32) 2^-52 A U |post_p| + 8 2^-52 |ref_p|,  A = sum_j |f_j pre_j| (+ extra_A), U = (1/n) sum_m w_m |u_m|"""
    f = np.atleast_2d(np.asarray(f, dtype=LD))
    n = f.shape[-1]
    w = np.full(n // 2 + 1, 2, dtype=LD)
    w[0] = 1
    if n % 2 == 0:
        w[-1] = 1
    U = (w * np.abs(np.asarray(u, dtype=CLD))).sum() / LD(n)
    A = np.abs(f * pre).sum(axis=-1) + extra_A
    core = LD(2 * n + 32) * LD(EPS) * A[:, None] * U * np.abs(post)[None, :]
    return core + LD(8 * EPS) * np.abs(ref), core


def ld_transform(r, f, dim, mu, plaw, u, lnkr, mutation=None):
    """k, F, bound, bound before the 8 ulp of `post`: one _fftlog_transform of the rows f with the coefficients (u, lnkr) given"""
    pre, post, k = stage_factors(r, dim, mu, plaw, lnkr)
    f = np.atleast_2d(np.asarray(f, dtype=np.float64)).astype(LD)
    F = ld_fht(f * pre, u, mutation) * post
    bound, core = fht_bound(f, pre, u, post, F)
    return k, F, bound, core


# ---------------------------------------------------------------------------------------------------- PCHIP, exact
def _frac(v):
    """a double or long double as the rational it is"""
    if isinstance(v, Fraction):
        return v
    hi = float(v)
    return Fraction(hi) + Fraction(float(v - LD(hi))) if isinstance(v, LD) else Fraction(hi)


def _sign(v):
    return (v > 0) - (v < 0)


def _edge(h0, h1, m0, m1, hits):
    d = ((2 * h0 + h1) * m0 - h0 * m1) / (h0 + h1)
    if _sign(d) != _sign(m0):
        hits.add('edge zero')
        return Fraction(0)
    if _sign(m0) != _sign(m1) and abs(d) > 3 * abs(m0):
        hits.add('edge clamp')
        return 3 * m0
    hits.add('edge plain')
    return d


def pchip_derivatives(x, y, hits=None):
    """the derivatives scipy's PchipInterpolator._find_derivatives gives, as Fractions; `hits` collects the branches taken"""
    hits = set() if hits is None else hits
    x, y = [_frac(v) for v in x], [_frac(v) for v in y]
    n = len(x)
    h = [x[i + 1] - x[i] for i in range(n - 1)]
    m = [(y[i + 1] - y[i]) / h[i] for i in range(n - 1)]
    if n == 2:
        hits.add('n == 2')
        return x, y, [m[0], m[0]]
    d = [Fraction(0)] * n
    for k in range(1, n - 1):
        if _sign(m[k - 1]) != _sign(m[k]) or m[k - 1] == 0 or m[k] == 0:
            hits.add('flat secant' if (m[k - 1] == 0 or m[k] == 0) else 'sign change')
            continue
        w1, w2 = 2 * h[k] + h[k - 1], h[k] + 2 * h[k - 1]
        d[k] = (w1 + w2) / (w1 / m[k - 1] + w2 / m[k])
        hits.add('harmonic mean')
    d[0] = _edge(h[0], h[1], m[0], m[1], hits)
    d[-1] = _edge(h[-1], h[-2], m[-1], m[-2], hits)
    return x, y, d


class ExactPchip(object):
    """PchipInterpolator(x, y, extrapolate=False) in exact rational arithmetic.  __call__(q) -> (value or None outside, scale),
    scale = |y_lo| + |y_lo+1| + dx (|d_lo| + |d_lo+1|), the size of the terms the cubic is summed from"""

    def __init__(self, x, y, hits=None):
        self.xf = np.asarray(x, dtype=np.float64)
        self.x, self.y, self.d = pchip_derivatives(self.xf, y, hits)

    def interval(self, q):
        n = len(self.x)
        if not (q >= self.xf[0]) or not (q <= self.xf[-1]):
            return None
        return min(int(np.searchsorted(self.xf, q, side='right')) - 1, n - 2)

    def __call__(self, q):
        lo = self.interval(q)
        if lo is None:
            return None, Fraction(0)
        x, y, d = self.x, self.y, self.d
        dx = x[lo + 1] - x[lo]
        slope = (y[lo + 1] - y[lo]) / dx
        t = (d[lo] + d[lo + 1] - 2 * slope) / dx
        s = Fraction(float(q)) - x[lo]
        val = y[lo] + s * (d[lo] + s * ((slope - d[lo]) / dx - t + s * t / dx))
        return val, abs(y[lo]) + abs(y[lo + 1]) + dx * (abs(d[lo]) + abs(d[lo + 1]))


def _ld(v):
    """a Fraction rounded to long double (twice to double: 106 bits before the last rounding)"""
    hi = float(v)
    return LD(hi) + LD(float(v - Fraction(hi)))


def pchip_reference(x, y, qs):
    """the interpolant of one row at many queries: the derivatives and every sign decision exact (ExactPchip), the cubic itself summed
    in long double from the exact coefficients, which leaves an error below 1e-18 `scale`, a thousandth of what is asserted.
    Returns val [nq] (long double, NaN outside), scale [nq] = |y_lo| + |y_lo+1| + dx (|d_lo| + |d_lo+1|), inside [nq] (bool)"""
    E = ExactPchip(x, y)
    qs = np.asarray(qs, dtype=np.float64)
    n = len(E.x)
    with np.errstate(invalid='ignore'):
        inside = (qs >= E.xf[0]) & (qs <= E.xf[-1])
    lo = np.clip(np.searchsorted(E.xf, np.where(inside, qs, E.xf[0]), side='right') - 1, 0, n - 2)
    c0, c1, sc = [], [], []
    for k in range(n - 1):
        dx = E.x[k + 1] - E.x[k]
        slope = (E.y[k + 1] - E.y[k]) / dx
        t = (E.d[k] + E.d[k + 1] - 2 * slope) / dx
        c0.append(_ld(t / dx)); c1.append(_ld((slope - E.d[k]) / dx - t))
        sc.append(_ld(abs(E.y[k]) + abs(E.y[k + 1]) + dx * (abs(E.d[k]) + abs(E.d[k + 1]))))
    c0, c1, sc = (np.array(v, dtype=LD)[lo] for v in (c0, c1, sc))
    c2, c3 = np.array([_ld(v) for v in E.d], dtype=LD)[lo], np.array([_ld(v) for v in E.y], dtype=LD)[lo]
    s_ = np.where(inside, qs, E.xf[0]).astype(LD) - E.xf.astype(LD)[lo]
    val = c3 + s_ * (c2 + s_ * (c1 + s_ * c0))
    return np.where(inside, val, LD('nan')), sc, inside


def pchip_ratios(got, val, scale):
    """|got - val| / (2^-52 scale) per element; 0 / 0 counts as 0, anything else over 0 as inf"""
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - val)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(err == 0, LD(0), err / (LD(EPS) * scale)).astype(np.float64)


# the PCHIP test inputs: dyadic rationals below 2^20 throughout, so slopes and sign tests are exact in double as well
PCHIP_N = (2, 3, 4, 17, 300)
PCHIP_ROWS = ('monotone', 'alternating', 'plateau', 'edge zero', 'edge clamp', 'constant', 'scattered')


def pchip_knots(n, spacing):
    if spacing == 'uniform':
        return -2.0 + 0.25 * np.arange(n)
    e = np.array([0, -6, -3, 3, -2, -6, 0, -5, 1, -4])[np.arange(n - 1) % 10]           # neighbours differ by up to 2^6
    return np.concatenate([[-3.5], -3.5 + np.cumsum(2.0 ** e)])


def pchip_rows(n):
    """one row per behaviour, [7][n]"""
    i = np.arange(n)
    mono = np.cumsum((i % 5 + 1) / 4.0)
    mono -= mono[min(2, n - 1)]                                                           # crosses zero, with a knot on it
    alt = (-1.0) ** i * (1 + i % 3) / 2
    plat = (i // 2).astype(float)
    if n >= 4:
        plat[-1] = plat[-2]
    dist = np.minimum(i, n - 1 - i).astype(float)
    zero = np.minimum(dist, 6.0) ** 3                                                                      # convex towards both ends: the 3-point derivative has the wrong sign
    clamp = np.zeros(n)
    clamp[1] = 1
    if n > 2:
        clamp[2] = -8
    if n >= 6:
        clamp[n - 2], clamp[n - 3] = 1, -8
    const = np.full(n, 2.5)
    scat = ((i * 37) % 64 - 32) / 8.0
    return np.stack([mono, alt, plat, zero, clamp, const, scat])


def pchip_queries(x):
    """every knot, both ends, midpoints, 2^-40 inside each knot, just outside both ends, +-inf, NaN"""
    x = np.asarray(x, dtype=np.float64)
    t = 2.0 ** -40
    inside = np.concatenate([x[:-1] + t, x[1:] - t])
    outside = [np.nextafter(x[0], -np.inf), np.nextafter(x[-1], np.inf), x[0] - t, x[-1] + t, np.inf, -np.inf, np.nan]
    return np.concatenate([x, 0.5 * (x[:-1] + x[1:]), inside, outside])


# ---------------------------------------------------------------------------------------------------- the chain
def pchip_margin(E, b, lo):
    """how far, in units of what errors of size b[k] in y[k] can do to it, every quantity whose sign PCHIP tests on the way to the cubic
    of interval lo is from zero: the secants of intervals lo - 1 .. lo + 1 and, at an end node, the three-point derivative and its
    distance from the clamp.  The smallest such ratio"""
    x, y, n = E.x, E.y, len(E.x)
    b = [_frac(v) for v in b]
    h = lambda k: x[k + 1] - x[k]
    m = lambda k: (y[k + 1] - y[k]) / h(k)
    dm = lambda k: (b[k] + b[k + 1]) / h(k)
    ratios = []

    def far(value, err):
        ratios.append(float('inf') if err == 0 else float(abs(value) / err))
    for k in range(max(lo - 1, 0), min(lo + 1, n - 2) + 1):
        far(m(k), dm(k))
    if n > 2:
        for node, (k0, k1) in ((0, (0, 1)), (n - 1, (n - 2, n - 3))):
            if node in (lo, lo + 1):
                h0, h1 = h(k0), h(k1)
                d = ((2 * h0 + h1) * m(k0) - h0 * m(k1)) / (h0 + h1)
                dd = ((2 * h0 + h1) * dm(k0) + h0 * dm(k1)) / (h0 + h1)
                far(d, dd)
                if _sign(m(k0)) != _sign(m(k1)) and _sign(d) == _sign(m(k0)):
                    far(abs(d) - 3 * abs(m(k0)), dd + 3 * dm(k0))
    return min(ratios)


def ld_chain(r_fft, prof, dim, mu, plaw_fwd, plaw_back, window, k1, x, lnq, coeff1, coeff2):
    """bfgx_fftlog_convolve in long double and exact PCHIP: two transforms with the coefficients given, coeffN = (u, lnkr) of stage N;
    k1[n] the doubles the second stage takes for its grid, x[n] the doubles ln(r_out r_scale), lnq[nq] the doubles ln r_eval.
    Returns ref [nrows][nq] (long double, times (2 pi)^dim), tol [nrows][nq], margin (the smallest pchip_margin over the queries)"""
    f = np.atleast_2d(np.asarray(prof, dtype=np.float64)).astype(LD)
    pre1, post1, _ = stage_factors(r_fft, dim, mu, plaw_fwd, coeff1[1])
    pre2, post2, _ = stage_factors(k1, dim, mu, plaw_back, coeff2[1])
    mid = post1 * np.asarray(window, dtype=np.float64).astype(LD) * pre2
    g1 = ld_fht(f * pre1, coeff1[0]) * mid
    b1, _ = fht_bound(f, pre1, coeff1[0], mid, g1)
    g2 = ld_fht(g1, coeff2[0]) * post2
    b2, _ = fht_bound(g1, LD(1), coeff2[0], post2, g2, extra_A=b1.sum(axis=-1))
    scale = TWO_PI ** dim
    ref, tol = np.zeros((f.shape[0], len(lnq)), dtype=LD), np.zeros((f.shape[0], len(lnq)), dtype=LD)
    margin = float('inf')
    n = len(x)
    for row in range(f.shape[0]):
        E = ExactPchip(x, list(g2[row]))
        for i, q in enumerate(lnq):
            lo = E.interval(q)
            if lo is None:
                continue
            val, S = E(q)
            margin = min(margin, pchip_margin(E, b2[row], lo))
            ks = range(max(lo - 1, 0), min(lo + 2, n - 1) + 1)
            bmax = max(b2[row][k] for k in ks)
            dx = E.x[lo + 1] - E.x[lo]
            hmin = min(E.x[k + 1] - E.x[k] for k in ks if k + 1 < n)
            lip = 1 + 3 * float(dx / hmin)                                     # see tests/test_gpu_fftlog_kernels.py
            slope = (E.y[lo + 1] - E.y[lo]) / dx
            deriv = float(abs(E.d[lo]) + abs(E.d[lo + 1]) + Fraction(3, 2) * abs(slope))
            xerr = EPS * (abs(x[lo]) + abs(x[lo + 1]) + abs(q))
            v = LD(float(val)) + LD(float(val - Fraction(float(val))))
            ref[row, i] = v * scale
            tol[row, i] = scale * (lip * bmax + LD(K_PCHIP * EPS * float(S)) + LD(deriv * xerr)) + LD(4 * EPS) * abs(ref[row, i])
    return ref, tol, margin
