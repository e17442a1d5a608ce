"""The fp64 device functions of csrc/bfgx_math.hpp, one by one, against mpmath (60 digits, rounded once to double): every pair
kernel, the regrid, K0 and the FFTLog twiddles take their logarithms, exponentials, reciprocals, square roots and angles from
these sequences, and the end-to-end tests (budgets 1e-10 to 1e-6) would not notice a function that is wrong by 1e-13.

Each test runs one function through engine.math_probe (bfgx_math_probe: one thread per element, every argument loaded from
memory) over the seeded set of tests/math_oracle.py, prints the worst error and the argument where it occurs (against the
once-rounded reference, which is what is asserted, and against the unrounded one), and asserts the bound:

  4e-16 relative          fast_rcp, fast_rsq, fast_sqrt, fast_log, atan_small, asin_small, both outputs of sincos_small, both
                          outputs of sincos_bounded for |x| <= 7, fast_exp where the result is normal (the header's own claim)
  4e-16 |ref| + 2^-1074   fast_exp where the result is subnormal (the two-step ldexp rounds once more)
  4e-16 absolute          sincos_bounded for 7 < |x| <= 1e3
  sincos_dphi             no fold: as the branch taken (4e-16 relative); fold: 4e-16 + |2 pi - fl(2 pi)| = 6.5e-16 absolute (the
                          fold subtracts the double 2 pi, so no relative bound applies)
  1e-15 relative          atan2_generic: three half-angle steps, each with an rcp, an rsq and a product, reach 6.6e-16 in an
                          exactly rounded emulation of the sequence; x 1.5 for the real seeds and the contraction of 1 + t t
  E(NSIDE) + 1e-15 theta  ring_theta_nolibm against the colatitude of the ring's exact rational z.  ring_z_sth rounds z first, so
                          the bound is not atan2's alone: E is the worst error, per NSIDE, of the float64 restatement of
                          healpix_cxx get_ring_info2 (oracle/refshim/healpy.py::_ring_theta) against the same mpmath values,
                          measured on the CPU when the test runs.  Measured: NSIDE 1: 3.10e-16, 2: 3.10e-16, 3: 4.24e-16,
                          4: 3.10e-16, 64: 4.51e-16, 1024: 4.87e-16, 8192: 5.31e-16 rad.  theta must also increase strictly with
                          the ring (the regrid's window search walks on that)
  bit for bit             the KReg forms of fast_log and sincos_small against the literal forms; add_nc(mul_nc(a, b), c) against
                          numpy's a * b + c

Measured on an MI355X, worst error against the once-rounded reference (against the unrounded one): fast_rcp 2.22e-16 (1.11e-16),
fast_rsq 2.22e-16 (1.35e-16), fast_sqrt 2.22e-16 (2.05e-16), fast_log 3.43e-16 (2.89e-16) at 1.0843, fast_exp 2.14e-16 (1.57e-16),
sincos_small 2.18e-16 / 1.27e-16, sincos_bounded 2.22e-16 relative and 1.11e-16 absolute, sincos_dphi 2.22e-16 unfolded and 3.33e-16
absolute folded, atan_small 2.09e-16, asin_small 1.88e-16, atan2_generic 5.41e-16 (5.23e-16) at (y, x) = (-0.32617, 1.02529),
ring_theta_nolibm at most 0.45 of its bound (NSIDE 8192, ring 1604).

fast_log missed its bound when these tests were written: (m - 1) * fast_rcp(m + 1) carried three roundings into s, and the result
was 4.19e-16 from the rounded reference (3.2e-16 from the unrounded one) at x = 1.3030997316033976.  s is now a corrected quotient.

What the probe cannot see: it checks the sequences as compiled into the probe kernel.  Instruction scheduling and fp contraction
inside K1 / K2 and the other product kernels may differ, and the end-to-end parity tests stay responsible for that.
"""
import numpy as np
import pytest

import math_oracle as O
from baryonification_amd import engine

pytestmark = pytest.mark.gpu

REL = 4e-16
FOLD_ABS = 4e-16 + 2.4492935982947064e-16                                     # |2 pi - fl(2 pi)|: 6.45e-16


def _report(label, got, ref, args, bound, relative=True, sel=None, floor=0.0):
    """print the worst error of `got` over `sel` and where it occurs, then assert err <= bound (+ floor, an absolute allowance)"""
    e_round, e_exact = O.errors(got, ref, relative)
    if floor:                                                                  # |err| <= bound |ref| + floor, stated as a relative error
        with np.errstate(divide='ignore', invalid='ignore'):
            e_round = np.where(ref[0] != 0, np.maximum(0.0, e_round - floor / np.abs(ref[0])), e_round)
    idx = np.arange(got.size) if sel is None else np.flatnonzero(sel)
    assert idx.size > 0, label
    i, j = idx[np.argmax(e_round[idx])], idx[np.argmax(e_exact[idx])]
    at = lambda k: ", ".join("%.17g" % a[k] for a in args)
    print("%-34s n = %5d  worst %s error %.3e at (%s); against the unrounded reference %.3e at (%s); bound %.2e"
          % (label, idx.size, "rel" if relative else "abs", e_round[i], at(i), e_exact[j], at(j), bound))
    assert e_round[i] <= bound, "%s: error %.3e at (%s) exceeds %.2e" % (label, e_round[i], at(i), bound)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize('name', ['rcp', 'rsq', 'sqrt', 'log', 'atan_small', 'asin_small'])
def test_one_result_functions(gpu, name):
    x, = O.inputs(name)
    got = engine.math_probe(name, x)
    _report("fast_" + name if name in ('rcp', 'rsq', 'sqrt', 'log') else name, got, O.reference(name), (x,), REL)
    if name in ('log', 'atan_small', 'asin_small'):                           # log 1 = atan 0 = asin 0 = 0, exactly
        zero = x == (1.0 if name == 'log' else 0.0)
        assert zero.any() and (got[zero] == 0).all()


def test_fast_sqrt_of_zero_and_negative_arguments_is_zero(gpu):
    got = engine.math_probe('sqrt', np.array([0.0, -0.0, -1.0, 4.0]))
    assert list(_bits(got)) == list(_bits([0.0, 0.0, 0.0, 2.0]))


def test_fast_log_kreg_is_bit_identical_to_the_literal_form(gpu):
    x, = O.inputs('log')
    assert np.array_equal(_bits(engine.math_probe('log_kreg', x)), _bits(engine.math_probe('log', x)))


def test_fast_exp(gpu):
    x, = O.inputs('exp')
    ref = O.reference('exp')
    got = engine.math_probe('exp', x)
    normal, sub = np.isfinite(ref[0]) & (ref[0] >= O.MIN_NORMAL), (ref[0] > 0) & (ref[0] < O.MIN_NORMAL)
    _report("fast_exp, normal results", got, ref, (x,), REL, sel=normal)
    _report("fast_exp, subnormal results", got, ref, (x,), REL, sel=sub, floor=2.0 ** -1074)
    rest = ~(normal | sub)                                                     # overflow
    assert rest.any() and np.isinf(ref[0][rest]).all() and np.array_equal(got[rest], ref[0][rest])
    sp = engine.math_probe('exp', np.array([0.0, np.inf, -np.inf, 710.0, -746.0, np.nan]))
    assert list(_bits(sp[:5])) == list(_bits([1.0, np.inf, 0.0, np.inf, 0.0])) and np.isnan(sp[5])


def test_sincos_small(gpu):
    x, = O.inputs('sincos_small')
    rs, rc = O.reference('sincos_small')
    s, c = engine.math_probe('sincos_small', x)
    _report("sincos_small sin", s, rs, (x,), REL)
    _report("sincos_small cos", c, rc, (x,), REL)
    assert (s[x == 0] == 0).all() and (c[x == 0] == 1).all()
    sk, ck = engine.math_probe('sincos_small_kreg', x)
    assert np.array_equal(_bits(sk), _bits(s)) and np.array_equal(_bits(ck), _bits(c))


def test_sincos_bounded(gpu):
    x, = O.inputs('sincos_bounded')
    rs, rc = O.reference('sincos_bounded')
    s, c = engine.math_probe('sincos_bounded', x)
    near = np.abs(x) <= 7
    _report("sincos_bounded sin, |x| <= 7", s, rs, (x,), REL, sel=near)
    _report("sincos_bounded cos, |x| <= 7", c, rc, (x,), REL, sel=near)
    _report("sincos_bounded sin, |x| <= 1e3", s, rs, (x,), 4e-16, relative=False)
    _report("sincos_bounded cos, |x| <= 1e3", c, rc, (x,), 4e-16, relative=False)


def test_sincos_dphi(gpu):
    x, = O.inputs('sincos_dphi')
    rs, rc = O.reference('sincos_dphi')
    s, c = engine.math_probe('sincos_dphi', x)
    xf, fold = O.dphi_fold(x)
    small = np.abs(xf) <= 0.5
    for label, sel in (("small branch", small), ("Cody-Waite branch", ~small)):
        _report("sincos_dphi sin, no fold, " + label, s, rs, (x,), REL, sel=(fold == 0) & sel)
        _report("sincos_dphi cos, no fold, " + label, c, rc, (x,), REL, sel=(fold == 0) & sel)
        _report("sincos_dphi sin, folded, " + label, s, rs, (x,), FOLD_ABS, relative=False, sel=(fold != 0) & sel)
        _report("sincos_dphi cos, folded, " + label, c, rc, (x,), FOLD_ABS, relative=False, sel=(fold != 0) & sel)


def test_atan2_generic(gpu):
    y, x = O.inputs('atan2')
    ref = O.reference('atan2')
    got = engine.math_probe('atan2', y, x)
    _report("atan2_generic", got, ref, (y, x), 1e-15)
    swap, steps, _ = O.atan2_path(y, x)
    for n in range(4):
        _report("atan2_generic, %d half-angle steps" % n, got, ref, (y, x), 1e-15, sel=steps == n)
    # the axes: (0, x > 0) -> exactly 0, (0, x < 0) -> pi, (y != 0, 0) -> +- pi / 2
    mag = np.array([1.0, 3.0e-300, 7.0e300, 0.1])
    ax = engine.math_probe('atan2', np.concatenate([0 * mag, 0 * mag, mag, -mag]), np.concatenate([mag, -mag, 0 * mag, 0 * mag]))
    assert (_bits(ax[:4]) == 0).all()
    want = np.repeat([np.pi, np.pi / 2, -np.pi / 2], 4)
    assert (np.abs(ax[4:] - want) <= 1e-15 * np.abs(want)).all(), ax[4:]


def test_ring_theta_nolibm(gpu):
    ns, ring = O.inputs('ring_theta')
    hi, lo = O.reference('ring_theta')
    got = engine.math_probe('ring_theta', ns, ring)
    for n in O.RING_NSIDES:
        sel = ns == n
        E = np.abs((O.ring_theta_float64(n, ring[sel]) - hi[sel]) - lo[sel]).max()     # the float64 get_ring_info2 against mpmath
        err = np.abs((got[sel] - hi[sel]) - lo[sel])
        over = err / (E + 1e-15 * hi[sel])
        i = np.argmax(over)
        print("ring_theta_nolibm NSIDE %5d  E = %.3e  worst error %.3e rad at ring %d (theta %.17g), %.2f of its bound"
              % (n, E, err[i], ring[sel][i], hi[sel][i], over[i]))
        assert over[i] <= 1.0
        assert (np.diff(got[sel]) > 0).all(), "NSIDE %d: theta does not increase strictly with the ring" % n


def test_mul_nc_add_nc_round_twice_like_numpy(gpu):
    a, b, c = O.inputs('mul_add_nc')
    assert np.array_equal(_bits(engine.math_probe('mul_add_nc', a, b, c)), _bits(a * b + c))


def test_probe_runs_more_than_one_block_and_a_ragged_tail(gpu):
    for n in (1, 255, 257, 1000):
        x = np.linspace(1.0, 2.0, n)
        assert np.array_equal(_bits(engine.math_probe('rcp', x)), _bits(engine.math_probe('rcp', np.concatenate([x, x]))[:n]))
    assert engine.math_probe('rcp', np.empty(0)).size == 0
