"""CPU checks of tests/math_oracle.py: every input set stays inside the domain csrc/bfgx_math.hpp states for its function and reaches
the branches, thresholds and ranges it is there for.  A set that fails here has to be moved, not the assertion."""
import mpmath
import numpy as np
import pytest

import math_oracle as O

SETS = ('rcp', 'rsq', 'sqrt', 'log', 'exp', 'sincos_small', 'sincos_bounded', 'sincos_dphi', 'atan_small', 'asin_small', 'atan2',
        'mul_add_nc', 'ring_theta')


@pytest.mark.parametrize('name', SETS)
def test_sets_are_seeded_finite_and_of_bounded_size(name):
    arg = O.inputs(name)
    assert all(a.size == arg[0].size and np.isfinite(a).all() and not a.flags.writeable for a in arg)
    # (the ring set holds every ring of the seven NSIDEs, 4 * sum(nside) - 7 of them; every other set stays at 2e4 points or fewer)
    assert 0 < arg[0].size <= (4 * sum(O.RING_NSIDES) - 7 if name == 'ring_theta' else 20000)
    O.inputs.cache_clear()
    again = O.inputs(name)
    assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(arg, again))


def test_domains():
    normal = lambda a: (np.abs(a) >= O.MIN_NORMAL).all()
    x, = O.inputs('rcp')
    assert normal(x) and (x > 0).any() and (x < 0).any() and np.abs(x).min() <= 2.0 ** -999 and np.abs(x).max() >= 2.0 ** 999
    for name in ('rsq', 'sqrt', 'log'):
        x, = O.inputs(name)
        assert normal(x) and (x > 0).all()
    for name in ('rcp', 'rsq', 'sqrt'):
        x, = O.inputs(name)
        assert all(v in x for v in O.nearby(1.0, 32)) and all(2.0 ** e in x for e in (-1000, -1, 0, 1, 1000))
    x, = O.inputs('exp')
    assert (x <= 745.14).all() and (x >= -745.14).all() and (x > 709.79).any()          # the ties of rint run past the overflow threshold
    for name, lim in (('sincos_small', 0.5), ('atan_small', 0.1), ('asin_small', 0.05)):
        x, = O.inputs(name)
        assert np.abs(x).max() == lim and (x == lim).any() and (x == -lim).any() and (x == 0).any()
        assert 0 < np.abs(x[x != 0]).min() < 2.0 ** -55
    x, = O.inputs('sincos_bounded')
    assert np.abs(x).max() <= 1e3 and (np.abs(x) > 900).any() and (np.abs(x) <= 7).sum() > 9000
    x, = O.inputs('sincos_dphi')
    assert np.abs(x).max() < 2 * np.pi and (x == np.nextafter(2 * np.pi, 0)).any() and (x == -np.nextafter(2 * np.pi, 0)).any()
    y, x = O.inputs('atan2')
    assert normal(y) and normal(x) and np.abs(x).max() > 2.0 ** 480 and np.abs(x).min() < 2.0 ** -480
    assert (np.abs(y) == np.abs(x)).sum() >= 1000


def test_log_set_sits_on_both_sides_of_the_mantissa_switch():
    x, = O.inputs('log')
    low = O.log_low_mantissa(x)
    assert low.sum() > 4000 and (~low).sum() > 4000
    near = O.nearby(O.SQRT_HALF, 64)
    assert all(v in x for v in near) and O.log_low_mantissa(near).sum() == 64          # the constant itself is not below itself
    assert all(v in x for v in O.nearby(1.0, 64)) and all(v in x for v in O.nearby(2.0, 64))
    assert (x == 1.0).any() and (x == 2.0 ** -1022).any() and (x == 2.0 ** 1023).any()


def test_sincos_bounded_set_reaches_every_quadrant_and_the_zeros():
    x, = O.inputs('sincos_bounded')
    for sel in (np.abs(x) <= 7, np.abs(x) > 7):
        assert sorted(set(O.sincos_bounded_q(x[sel]))) == [0, 1, 2, 3]
    with mpmath.workdps(O.DPS):
        for k in range(-8, 9):
            assert all(v in x for v in (O.nearby(float(k * mpmath.pi / 2), 4) if k else [0.0]))


def test_sincos_dphi_set_takes_both_branches_under_every_fold():
    x, = O.inputs('sincos_dphi')
    xf, fold = O.dphi_fold(x)
    assert np.abs(xf).max() <= O.PI
    for f in (0, 1, -1):
        small = np.abs(xf[fold == f]) <= 0.5
        assert small.sum() >= 50 and (~small).sum() >= 50, f
    for c in (O.PI, -O.PI, 0.5, -0.5):                                          # the doubles on both sides of each threshold
        assert all(v in x for v in O.nearby(c, 8))


def test_atan2_set_reaches_every_step_count_swap_and_quadrant():
    y, x = O.inputs('atan2')
    swap, steps, quad = O.atan2_path(y, x)
    assert steps.max() == 3
    for s in (False, True):
        for n in range(4):
            for q in range(4):
                assert ((swap == s) & (steps == n) & (quad == q)).sum() >= 20, (s, n, q)
    # ratios a few ulp on either side of 0.1 at the start, and after one and after two half-angle steps
    t = np.minimum(np.abs(y), np.abs(x)) / np.maximum(np.abs(y), np.abs(x))
    for j, t0 in enumerate(O._atan_step_thresholds()):
        near = np.abs(t / t0 - 1) < 1e-14
        assert near.sum() >= 100 and sorted(set(steps[near])) == [j, j + 1], (j, sorted(set(steps[near])))


def test_exp_set_reaches_the_subnormal_range_and_the_rint_ties():
    x, = O.inputs('exp')
    hi, _ = O.reference('exp')
    sub = (hi > 0) & (hi < O.MIN_NORMAL)
    assert sub.sum() >= 100 and np.isinf(hi).any() and (x[sub] < -708.39).all()
    assert np.allclose(hi[sub], np.exp(x[sub]), rtol=0, atol=2.0 ** -1073)     # the subnormal rounding done in math_oracle._split
    kx = x * 1.44269504088896338700
    assert (np.abs(kx - np.floor(kx) - 0.5) < 1e-12).sum() >= 5 * 2149


def test_no_contraction_set_tells_an_fma_from_two_roundings():
    """fl(fl(a b) + c) differs from the exactly rounded fma(a, b, c) on 23.5 % of uniform (-2, 2) triples: a contracted multiply-add
    cannot pass a bit-for-bit comparison on this set"""
    a, b, c = O.inputs('mul_add_nc')
    fma, _ = O.reference('mul_add_nc')
    frac = np.mean((a * b + c).view(np.uint64) != fma.view(np.uint64))
    print("a * b + c differs from fma(a, b, c) on %.1f %% of the points" % (100 * frac))
    assert frac >= 0.15


def test_references_round_once_and_keep_the_remainder():
    for name in ('log', 'atan2', 'sincos_small'):
        ref = O.reference(name)
        hi, lo = ref[0] if name == 'sincos_small' else ref
        ok = np.isfinite(hi) & (np.abs(hi) >= O.MIN_NORMAL)
        assert (np.abs(lo[ok]) <= 0.5 * np.spacing(np.abs(hi[ok]))).all() and (lo[ok] != 0).mean() > 0.9
    x, = O.inputs('log')
    hi, _ = O.reference('log')
    assert (hi[x == 1.0] == 0.0).all() and np.abs(hi[x != 1.0] / np.log(x[x != 1.0]) - 1).max() < 5e-16
    got = np.array([1.0, 0.0, 2.0, 0.0])
    e_round, e_exact = O.errors(got, (np.array([1.0, 0.0, 1.0, 1.0]), np.array([2.0 ** -54, 0.0, 0.0, 0.0])))
    assert list(e_round) == [0.0, 0.0, 1.0, 1.0] and list(e_exact) == [2.0 ** -54, 0.0, 1.0, 1.0]
    assert list(O.errors(np.array([1e-300]), (np.array([0.0]), np.array([0.0])))[0]) == [np.inf]


def test_ring_reference_is_monotonic_and_the_float64_restatement_is_close():
    ns, ring = O.inputs('ring_theta')
    hi, lo = O.reference('ring_theta')
    for n in O.RING_NSIDES:
        sel = ns == n
        assert sel.sum() == 4 * n - 1 and (np.diff(hi[sel]) > 0).all()
        assert np.abs(hi[sel] + hi[sel][::-1] - np.pi).max() < 1e-15            # north / south symmetry
        E = np.abs((O.ring_theta_float64(n, ring[sel]) - hi[sel]) - lo[sel]).max()
        print("NSIDE %5d  worst error of the float64 get_ring_info2 restatement: %.3e rad" % (n, E))
        assert E < 1e-15
