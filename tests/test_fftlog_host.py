"""The host side of the FFTLog path -- clngamma, fftlog_good_lnkr, fftlog_u, fftlog_stage of csrc/bfgx_fftlog_api.inc, reached alone
through bfgx_fftlog_u / bfgx_fftlog_kgrid -- against mpmath, and the references of tests/fftlog_oracle.py against independent
implementations.  No GPU.

Tolerance of the coefficients: K 2^-52 S_m on ln|u_m| and on arg u_m mod 2 pi, with
    S_m = 1 + |q| ln 2 + |lnGamma(x+ + i y_m)| + |lnGamma(x- + i y_m)| + |2 y_m (ln 2 - ln kr)|,
the sizes of the terms ln u_m is summed from (complex moduli from mpmath); and K 2^-52 dln (1 + ln 2 / dln + (|lnGamma+| + |lnGamma-|) / pi)
on ln(k r), the same statement for eq. B22.  K is not guessed: scipy.special.loggamma through oracle.fftlog.u_coefficients / good_lnkr,
an independent double implementation of the same formulas, is measured against mpmath over the same grid, and the library is given four
times its worst ratio, and at least 8 (two different libms).  Measured on the grid below (8 parameter triples x n in 4, 5, 64, 1100, 4096
x 100, 331, 332, 400, 1000 points per decade), worst ratios over the grid of ln|u|, arg u, ln kr:
    scipy's route  7.96 (at (3, 0, -1); 7.88 at (3, 0, -2), 5.19 at (2, 0, -0.5)), 4.82 (at (2, 1, -1)), 1.45      ->  K = 32
    the library    0.19, 0.14, 0.002
The library works the coefficients out in long double and rounds once.  Before that (double throughout) it measured 18.2, 6.31, 1.54: the
recurrence and Stirling's series sum terms of size 30 to an ln Gamma of order 1.  And before the fix of the reflection it returned u = inf /
NaN wherever q > mu_b ((3, 0, -0.5) and (2, 0, -0.5) here) at 332 points per decade and above: std::sin(pi z) overflows from Im z = 226,
and Im z reaches pi / (2 dln).

PCHIP: K_p is measured in the same way, scipy's double PchipInterpolator against the exact rational restatement on the inputs of
fftlog_oracle.pchip_rows: worst ratio 2.19 of 2^-52 (|y_lo| + |y_lo+1| + dx (|d_lo| + |d_lo+1|)); K_p = 8.8.
"""
from fractions import Fraction

import numpy as np
import pytest
from scipy import interpolate

import fftlog_oracle as O
from baryonification_amd import _lib
from baryonification_amd.utils.Pixel import _kgrid, fftlog_u
from oracle import fftlog as F

K_U, K_PCHIP = O.K_U, O.K_PCHIP

GRID_N = (4, 5, 64, 1100, 4096)
GRID_PER_DECADE = (100, 331, 332, 400, 1000)


def _scipy_route(n, dln, mub, q):
    with np.errstate(all='ignore'):
        lnkr = F.good_lnkr(dln, mub, q)
        return F.u_coefficients(n, dln, mub, q, lnkr), lnkr


@pytest.mark.parametrize('dim,mu,plaw', O.TRIPLES)
def test_u_and_kgrid_against_mpmath(dim, mu, plaw):
    q, mub = O.bias(dim, mu, plaw)
    worst_lib, worst_sci = np.zeros(3), np.zeros(3)
    for per_decade in GRID_PER_DECADE:
        for n in GRID_N:
            r = O.log_grid(n, per_decade, 1e-3)
            dln = O.dln_of(r)
            ref = O.mp_u(n, dln, mub, q)
            assert abs(ref[6]) < 0.5 - 1e-6, "ln(k r) sits on a rounding boundary of eq. B22: move the grid"
            sci = np.array(O.u_errors(*_scipy_route(n, dln, mub, q), ref))
            u, lnkr = fftlog_u(r, dim, mu, plaw)
            lib = np.array(O.u_errors(u, lnkr, ref))
            worst_lib, worst_sci = np.maximum(worst_lib, lib), np.maximum(worst_sci, sci)
            assert (lib <= K_U).all(), "n = %d, %d per decade: |ln|u||, arg u, ln kr off by %s x 2^-52 S (K = %g)" % (n, per_decade, lib, K_U)
            if n % 2 == 0:
                assert u[-1].imag == 0
            k = _kgrid(r, dim, mu, plaw)
            k_ref = np.exp(O.LD(float(ref[0]))) / r[::-1].astype(O.LD)
            tol = K_U * O.EPS * float(ref[5]) + 4 * O.EPS                      # ln kr, then exp and the division
            assert np.abs(k / k_ref - 1).max() <= tol
            assert np.abs(k * r[::-1] / np.exp(lnkr) - 1).max() <= 2 * O.EPS     # the k grid is the returned ln kr
    print("(%d, %g, %g): worst ratio to 2^-52 S of ln|u|, arg u, ln kr: library %.2f %.2f %.2f; scipy's loggamma route %.2f %.2f %.2f"
          % ((dim, mu, plaw) + tuple(worst_lib) + tuple(worst_sci)))


@pytest.mark.parametrize('plaw', [0.0, 2.0])
def test_pole_of_the_denominator_gamma_gives_u0_zero(plaw):
    """dim 2, mu 0: x- = (1 - q) / 2 = 0 for plaw = 0 and -1 for plaw = 2, so 1 / Gamma(x-) = 0 at m = 0.  The coefficients beside the
    pole (small y_m on a wide grid) go through the reflection next to a zero of sin(pi z), where the phase used to be wrong"""
    q, mub = O.bias(2, 0, plaw)
    for n, per_decade in ((4, 0.02), (5, 0.02), (64, 100), (257, 1000)):
        r = O.log_grid(n, per_decade, 1e-3 if per_decade > 1 else 1e-100)
        ref = O.mp_u(n, O.dln_of(r), mub, q)
        assert ref[4] and abs(ref[6]) < 0.5 - 1e-6
        u, lnkr = fftlog_u(r, 2, 0, plaw)
        assert u[0] == 0 and np.isfinite(u.view(np.float64)).all() and (u[1:] != 0).all()
        lib = np.array(O.u_errors(u, lnkr, ref))
        print("plaw %g n %d: ratios %s" % (plaw, n, lib))
        assert (lib <= K_U).all(), (n, per_decade, lib)


def test_pole_of_the_numerator_gamma_is_refused():
    """x+ = (mu_b + 1 + q) / 2 a non-positive integer: Gamma(x+) is infinite in u_0.  dim 2, mu 0: plaw -2 (x+ = 0), -4 (x+ = -1)"""
    L = _lib.load()
    r = np.geomspace(1e-2, 1e2, 8)
    k, u, lnkr = np.full(8, -7.5), np.full(10, -7.5), np.full(1, -7.5)
    for plaw in (-2.0, -4.0):
        assert L.bfgx_fftlog_kgrid(8, r.ctypes.data, 2, 0.0, plaw, k.ctypes.data) == _lib.ERR_INVALID
        assert b'pole' in L.bfgx_last_error()
        assert L.bfgx_fftlog_u(8, r.ctypes.data, 2, 0.0, plaw, u.ctypes.data, lnkr.ctypes.data) == _lib.ERR_INVALID
        assert L.bfgx_fftlog_transform(0, 1, 8, r.ctypes.data, r.ctypes.data, 2, 0.0, plaw, k.ctypes.data, k.ctypes.data) == _lib.ERR_INVALID
        assert L.bfgx_fftlog_convolve(0, 1, 8, r.ctypes.data, r.ctypes.data, 2, 0.0, -1.0, plaw, r.ctypes.data, 8, r.ctypes.data, 1.0,
                                      k.ctypes.data) == _lib.ERR_INVALID
        assert (k == -7.5).all() and (u == -7.5).all() and (lnkr == -7.5).all()
        with pytest.raises(ValueError, match="pole"):
            fftlog_u(r, 2, 0, plaw)
    assert L.bfgx_fftlog_kgrid(8, r.ctypes.data, 3, 0.0, -3.0, k.ctypes.data) == _lib.ERR_INVALID     # 3-D: x+ = (1.5 + q) / 2 = 0 at q = -1.5


def test_grid_length_limits_and_null_arguments():
    L = _lib.load()
    for n, ok in ((4096, True), (4, True), (4097, False), (3, False)):
        r = O.log_grid(n, 1000, 1e-2)
        k, u, lnkr = np.empty(n), np.empty(2 * (n // 2 + 1)), np.empty(1)
        rc = L.bfgx_fftlog_kgrid(n, r.ctypes.data, 3, 0.0, -1.5, k.ctypes.data)
        rc_u = L.bfgx_fftlog_u(n, r.ctypes.data, 3, 0.0, -1.5, u.ctypes.data, lnkr.ctypes.data)
        assert rc == rc_u == (_lib.OK if ok else _lib.ERR_INVALID), (n, rc, rc_u)
        if not ok:
            assert b'[4, 4096]' in L.bfgx_last_error()
    r, u, lnkr = np.geomspace(1.0, 8.0, 4), np.empty(6), np.empty(1)
    for args in ((None, u.ctypes.data, lnkr.ctypes.data), (r.ctypes.data, None, lnkr.ctypes.data), (r.ctypes.data, u.ctypes.data, None)):
        assert L.bfgx_fftlog_u(4, args[0], 3, 0.0, -1.5, args[1], args[2]) == _lib.ERR_INVALID and b'NULL' in L.bfgx_last_error()


def test_pchip_rows_refuses_bad_arguments_before_any_device_call():
    L = _lib.load()
    x, y, q, out = np.array([1.0, 2.0, 4.0]), np.ones(3), np.ones(1), np.full(1, -7.5)

    def call(nrows=1, n=3, nq=1, xx=x):
        return L.bfgx_pchip_rows(0, nrows, n, xx.ctypes.data, y.ctypes.data, nq, q.ctypes.data, out.ctypes.data)
    for kw in (dict(nrows=0), dict(nrows=65536), dict(n=1), dict(nq=0)):
        assert call(**kw) == _lib.ERR_INVALID and b'pchip' in L.bfgx_last_error(), kw
    for bad in ([1.0, 1.0, 4.0], [1.0, 4.0, 2.0], [1.0, np.nan, 4.0]):
        assert call(xx=np.array(bad)) == _lib.ERR_INVALID and b'ascending' in L.bfgx_last_error(), bad
    assert out[0] == -7.5


# ---------------------------------------------------------------------------------------------------- the references themselves
def _smooth_rows(r):
    return np.stack([np.exp(-(r / s) ** 1.3) / (1 + (r / 0.05) ** p) for s, p in ((0.3, 0.7), (1.0, 1.2), (7.0, 0.9))])


@pytest.mark.parametrize('n', [4, 5, 63, 64, 257, 1100])
def test_long_double_transform_against_the_numpy_oracle_and_direct_sums(n):
    O.require_longdouble()
    r = np.geomspace(1e-2, 1e2, n) if n <= 64 else O.log_grid(n, 100, 1e-6)
    rows = _smooth_rows(r)
    for dim, mu, plaw in O.TRIPLES:
        q, mub = O.bias(dim, mu, plaw)
        u, lnkr = _scipy_route(n, O.dln_of(r), mub, q)
        k, T, bound, _ = O.ld_transform(r, rows, dim, mu, plaw, u, lnkr)
        ko, To = F.fftlog_transform(r, rows, dim, mu, plaw)                        # numpy's double FFT: inside the kernel's bound
        assert np.abs(ko / k - 1).max() <= 8 * O.EPS
        assert (np.abs(To - T) <= bound).all(), float((np.abs(To - T) / bound).max())
        if n <= 257:
            pre, post, _ = O.stage_factors(r, dim, mu, plaw, lnkr)
            a = rows.astype(O.LD) * pre
            d = np.abs(O.ld_fht_direct(a, u) - O.ld_fht(a, u))
            U = np.abs(u).sum() * 2 / n
            assert (d <= 64 * n * np.finfo(O.LD).eps * np.abs(a).sum(axis=-1)[:, None] * U).all()


def test_mutated_references_differ():
    O.require_longdouble()
    for n in (8, 9):
        r = np.geomspace(1e-2, 1e2, n)
        u, lnkr = _scipy_route(n, O.dln_of(r), 0.5, 0.0)
        a = np.eye(n)
        ref = O.ld_fht(a, u)
        for mut in O.MUTATIONS:
            if n % 2 and mut.startswith('nyquist'):
                continue
            assert np.abs(O.ld_fht(a, u, mut) - ref).max() > 1e-3, (n, mut)


def test_exact_pchip_against_scipy():
    """the rational restatement against scipy's PchipInterpolator on the inputs the GPU test uses; the worst ratio is K_p's source"""
    worst, hits = 0.0, set()
    for n in O.PCHIP_N:
        for spacing in ('uniform', 'varying'):
            x, Y = O.pchip_knots(n, spacing), O.pchip_rows(n)
            assert np.abs(x).max() < 2 ** 20 and np.abs(Y).max() < 2 ** 20 and (np.diff(x) > 0).all()
            if spacing == 'varying' and n > 2:
                ratio = np.diff(x)[1:] / np.diff(x)[:-1]
                assert max(ratio.max(), 1 / ratio.min()) == 64 or n < 4
            qs = O.pchip_queries(x)
            for row, y in zip(O.PCHIP_ROWS, Y):
                E = O.ExactPchip(x, y, hits)
                val, scale, inside = O.pchip_reference(x, y, qs)
                with np.errstate(invalid='ignore'):
                    got = interpolate.PchipInterpolator(x, y, extrapolate=False)(qs)
                assert np.array_equal(np.isnan(got), ~inside), (n, spacing, row)
                worst = max(worst, O.pchip_ratios(got[inside], val[inside], scale[inside]).max())
                for i in list(range(0, len(qs), 7)) + [n - 1]:                     # the long-double cubic against the all-rational one
                    exact, sc = E(qs[i])
                    assert (exact is None) == (not inside[i])
                    if exact is not None:
                        assert abs(O._frac(val[i]) - exact) <= Fraction(1e-18) * sc and abs(O._frac(scale[i]) - sc) <= Fraction(1e-18) * sc
                for xx, yy in zip(x, y):                                           # knots are reproduced exactly by the restatement
                    assert E(xx)[0] == yy
    print("scipy PchipInterpolator against the exact restatement: worst ratio %.3f; branches taken: %s" % (worst, sorted(hits)))
    assert hits == {'n == 2', 'harmonic mean', 'sign change', 'flat secant', 'edge zero', 'edge clamp', 'edge plain'}
    assert worst <= K_PCHIP
