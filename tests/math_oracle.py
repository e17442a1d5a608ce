"""References and seeded input sets for the device functions of csrc/bfgx_math.hpp (tests/test_gpu_math.py runs them on the GPU
through engine.math_probe, tests/test_math_oracle_host.py checks on the CPU that every set reaches what it is there for).

reference(name) evaluates the function with mpmath at 60 digits and rounds ONCE to double: that double is what the bounds
are asserted against.  The part the rounding drops is returned with it (ref = hi + lo to about 1e-32 relative), so that a test
can also print the error against the unrounded value.  Results in the subnormal range are rounded to a multiple of 2^-1074 here,
since mpmath's own conversion would round them twice.

inputs(name) and reference(name) are computed once per process and returned read-only.

The predicates at the end restate, in numpy, the DECISIONS the device code takes (which side of a threshold, which quadrant,
how many half-angle steps), not its arithmetic.
"""
import functools
import importlib.util
import os

import mpmath
import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('_math_refshim_healpy', os.path.join(REPO, 'oracle', 'refshim', 'healpy.py'))
hp = importlib.util.module_from_spec(_spec)                        # the refshim, loaded under a private name (as hpx_oracle.py does)
_spec.loader.exec_module(hp)

DPS = 60
SQRT_HALF = 0.70710678118654752440          # the switch of fast_log, as the header spells it
PI, TWO_PI = 3.141592653589793238462643383279502884197, 2.0 * 3.141592653589793238462643383279502884197
RING_NSIDES = (1, 2, 3, 4, 64, 1024, 8192)
MIN_NORMAL = 2.0 ** -1022


def _frozen(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    a.setflags(write=False)
    return a


def nearby(x, k):
    """the 2k + 1 doubles x - k ulp .. x + k ulp (x normal, not zero), ascending"""
    bits = np.array([x], dtype=np.float64).view(np.int64)[0]
    steps = np.arange(-k, k + 1, dtype=np.int64)
    return (bits + (steps if x > 0 else -steps)).view(np.float64)


def _log_uniform(rng, n, e_lo, e_hi):
    """2^e_lo <= x < 2^e_hi, uniform in the exponent and in the mantissa"""
    return np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(e_lo, e_hi, n).astype(np.int32))


def _both_signs(rng, x):
    return x * rng.choice([-1.0, 1.0], x.size)


# ------------------------------------------------------------------------------------------------ input sets
def _rcp_like(seed, signed):
    rng = np.random.default_rng(seed)
    x = np.concatenate([_log_uniform(rng, 12000, -1000, 1000), np.ldexp(1.0, np.arange(-1000, 1001, dtype=np.int32)), nearby(1.0, 32)])
    return np.concatenate([x, -x[::3]]) if signed else x


def _small_arg(seed, lim):
    """uniform [-lim, lim], log-uniform 2^-60 .. lim with both signs, the endpoints and 0"""
    rng = np.random.default_rng(seed)
    tiny = np.exp(rng.uniform(np.log(2.0 ** -60), np.log(lim), 6000))
    return np.concatenate([rng.uniform(-lim, lim, 12000), _both_signs(rng, tiny), [lim, -lim, 0.0]])


def _atan_step_thresholds():
    """the ratios t0 that arrive at 0.1 after 0, 1 and 2 half-angle steps (a third step cannot start above 0.1: tan(8 atan 0.1) > 1)"""
    with mpmath.workdps(DPS):
        return [float(mpmath.tan(2 ** j * mpmath.atan(mpmath.mpf('0.1')))) for j in range(3)]


def _atan2_inputs():
    rng = np.random.default_rng(1212)
    y, x = [rng.standard_normal(9000)], [rng.standard_normal(9000)]
    m = np.exp(rng.uniform(-3, 3, 250))                                       # |y| = |x|
    for sy in (1, -1):
        for sx in (1, -1):
            y.append(sy * m); x.append(sx * m)
    for t0 in _atan_step_thresholds():                                        # ratios within a few ulp of a step's threshold
        for den in (1.0, 1.5, 0.7, 3.0e5):
            num = np.array([fl for u in nearby(t0, 6) for fl in nearby(u * den, 1)])
            for sy in (1, -1):
                for sx in (1, -1):
                    y.append(sy * num); x.append(sx * np.full(num.size, den))      # swap off
                    y.append(sy * np.full(num.size, den)); x.append(sx * num)      # swap on
    e = rng.integers(-500, 501, 4000).astype(np.int32)                        # common scales 2^-500 .. 2^500
    y.append(np.ldexp(rng.standard_normal(4000), e)); x.append(np.ldexp(rng.standard_normal(4000), e))
    return np.concatenate(y), np.concatenate(x)


def _ring_inputs():
    ns = np.concatenate([np.full(4 * n - 1, n, dtype=np.int64) for n in RING_NSIDES])
    ring = np.concatenate([np.arange(1, 4 * n, dtype=np.int64) for n in RING_NSIDES])
    return ns, ring


@functools.lru_cache(maxsize=None)
def inputs(name):
    """tuple of read-only argument arrays of the set `name`"""
    if name == 'rcp':
        out = (_rcp_like(101, True),)
    elif name == 'rsq':
        out = (_rcp_like(202, False),)
    elif name == 'sqrt':
        out = (_rcp_like(303, False),)
    elif name == 'log':
        rng = np.random.default_rng(404)
        out = (np.concatenate([_log_uniform(rng, 8000, -1022, 1024), rng.uniform(0.5, 2.0, 8000), nearby(SQRT_HALF, 64), nearby(1.0, 64),
                               nearby(2.0, 64), np.ldexp(1.0, np.arange(-1022, 1024, dtype=np.int32))]),)
    elif name == 'exp':
        rng = np.random.default_rng(505)
        with mpmath.workdps(DPS):
            ties = [float((k + mpmath.mpf('0.5')) * mpmath.ln2) for k in range(-1074, 1075)]          # where rint(x / ln 2) ties
        out = (np.concatenate([rng.uniform(-745.13, 709.78, 5000), rng.uniform(-1.0, 1.0, 3000)] + [nearby(t, 2) for t in ties]),)
    elif name == 'sincos_small':
        out = (_small_arg(606, 0.5),)
    elif name == 'sincos_bounded':
        rng = np.random.default_rng(707)
        with mpmath.workdps(DPS):
            zeros = [nearby(float(k * mpmath.pi / 2), 4) for k in range(-8, 9) if k]
        out = (np.concatenate([rng.uniform(-7.0, 7.0, 9000), rng.uniform(-1e3, 1e3, 9000), [0.0]] + zeros),)
    elif name == 'sincos_dphi':
        rng = np.random.default_rng(808)
        edge = [s * (TWO_PI - 2.0 ** -k) for k in range(0, 51) for s in (1, -1)]                       # up to the last double inside (-2 pi, 2 pi)
        x = np.concatenate([rng.uniform(-TWO_PI, TWO_PI, 12000), nearby(PI, 8), nearby(-PI, 8), nearby(0.5, 8), nearby(-0.5, 8), edge])
        out = (x[np.abs(x) < 2 * np.pi],)
    elif name == 'atan_small':
        out = (_small_arg(909, 0.1),)
    elif name == 'asin_small':
        out = (_small_arg(1010, 0.05),)
    elif name == 'atan2':
        out = _atan2_inputs()
    elif name == 'mul_add_nc':
        rng = np.random.default_rng(1313)
        out = tuple(rng.uniform(-2.0, 2.0, 20000) for _ in range(3))
    elif name == 'ring_theta':
        out = _ring_inputs()
    else:
        raise KeyError(name)
    return tuple(_frozen(a) for a in out)


# ------------------------------------------------------------------------------------------------ references
def _split(v):
    """mpf -> (the double nearest to it, what that rounding dropped)"""
    if v != 0 and abs(v) < MIN_NORMAL:
        hi = float(np.ldexp(float(int(mpmath.nint(mpmath.ldexp(v, 1074)))), -1074))
    else:
        hi = float(v)
    return hi, (float(v - mpmath.mpf(hi)) if np.isfinite(hi) else 0.0)


def _map(fn, *args):
    with mpmath.workdps(DPS):
        res = [_split(fn(*[mpmath.mpf(float(a)) for a in p])) for p in zip(*args)]
    return _frozen([r[0] for r in res]), _frozen([r[1] for r in res])


def ring_z_exact(nside, ring):
    """cos(colatitude) of a ring centre as an exact rational (mpmath.mpf at the working precision)"""
    nside, ring = int(nside), int(ring)
    north = min(ring, 4 * nside - ring)
    z = 1 - mpmath.mpf(north * north) / (3 * nside * nside) if north < nside else mpmath.mpf(2 * (2 * nside - north)) / (3 * nside)
    return z if north == ring else -z


@functools.lru_cache(maxsize=None)
def reference(name):
    """(hi, lo) of the result over inputs(name); for the sincos sets ((sin hi, sin lo), (cos hi, cos lo))"""
    arg = inputs(name)
    if name in ('sincos_small', 'sincos_bounded', 'sincos_dphi'):
        return _map(mpmath.sin, *arg), _map(mpmath.cos, *arg)
    if name == 'ring_theta':
        with mpmath.workdps(DPS):
            res = [_split(mpmath.acos(ring_z_exact(n, r))) for n, r in zip(*arg)]
        return _frozen([r[0] for r in res]), _frozen([r[1] for r in res])
    fn = {'rcp': lambda x: 1 / x, 'rsq': lambda x: 1 / mpmath.sqrt(x), 'sqrt': mpmath.sqrt, 'log': mpmath.log, 'exp': mpmath.exp,
          'atan_small': mpmath.atan, 'asin_small': mpmath.asin, 'atan2': mpmath.atan2, 'mul_add_nc': lambda a, b, c: a * b + c}[name]
    return _map(fn, *arg)


def errors(got, ref, relative=True):
    """(error against the once-rounded reference, error against the unrounded one), elementwise.  Relative errors are taken over
    |ref|; where the reference is 0 the relative error is 0 for an exact 0 and inf otherwise."""
    hi, lo = ref
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        d = got - hi
        e_round, e_exact = np.abs(d), np.abs(d - lo)
        same = (got == hi) | (np.isnan(got) & np.isnan(hi))                    # (inf - inf)
        e_round, e_exact = np.where(same, 0.0, e_round), np.where(same & (lo == 0), 0.0, e_exact)
        if relative:
            den = np.abs(hi)
            e_round = np.where(den > 0, e_round / den, np.where(e_round == 0, 0.0, np.inf))
            e_exact = np.where(den > 0, e_exact / den, np.where(got == 0, 0.0, np.inf))
    return e_round, e_exact


# ------------------------------------------------------------------------------------------------ what the device code decides
def log_low_mantissa(x):
    """fast_log's `m < sqrt(1/2)` on the frexp mantissa"""
    return np.frexp(x)[0] < SQRT_HALF


def sincos_bounded_q(x):
    return np.rint(x * 0.63661977236758134308).astype(np.int64) & 3


def dphi_fold(x):
    """(folded argument, +1 / -1 / 0 for the fold taken), with the double 2 pi as the device subtracts it"""
    up, dn = x > PI, x < -PI
    return np.where(up, x - TWO_PI, np.where(dn, x + TWO_PI, x)), up.astype(int) - dn.astype(int)


def atan2_path(y, x):
    """(swap, half-angle steps, quadrant 0..3 counter-clockwise from +x +y) of atan2_generic"""
    ay, ax = np.abs(y), np.abs(x)
    swap = ay > ax
    num, den = np.where(swap, ax, ay), np.where(swap, ay, ax)
    t = np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)
    steps = np.zeros(t.size, dtype=np.int64)
    for _ in range(4):
        go = t > 0.1
        steps += go
        t = np.where(go, t / (1.0 + np.sqrt(1.0 + t * t)), t)
    quad = np.where(x >= 0, np.where(y >= 0, 0, 3), np.where(y >= 0, 1, 2))
    return swap, steps, quad


def ring_theta_float64(nside, ring):
    """the float64 restatement of healpix_cxx get_ring_info2 (oracle/refshim/healpy.py), whose own error against mpmath the
    device's ring colatitudes are measured by"""
    return hp._ring_theta(int(nside), np.asarray(ring, dtype=np.int64))
