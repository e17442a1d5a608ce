"""fht_rows_kernel and pchip_rows_kernel (csrc/bfgx_fftlog.hpp) element by element against the references of tests/fftlog_oracle.py,
and bfgx_fftlog_convolve, the chain of the two, against the same references chained.  No masking anywhere: every element of every row
is compared.

fht_rows_kernel, through bfgx_fftlog_transform.  The reference takes the very coefficients the library hands the kernel (bfgx_fftlog_u,
checked on their own in tests/test_fftlog_host.py), so the kernel is judged alone.  The bound is the forward error of what it does -- one
FMA per term, twiddles with an absolute error of tau = 4e-16 (sincos_bounded, tests/test_gpu_math.py) + 4 pi 2^-53 (the argument) --:
    before `post`  |c_p - ref_p| <= (2 n + 32) 2^-52 A U,   A = sum_j |f_j pre_j|,  U = (1 / n) sum_m w_m |u_m|,  w = 1 at m = 0 and at the
                   Nyquist term, 2 elsewhere
    after          that times |post_p|, plus 8 x 2^-52 |ref_p| for the two powers of `post`
Unit rows f = e_j read the transform's matrix out element by element: all n of them for n up to 257 (257 rows are also more rows than
compute units), five of them (j = 0, 1, n/2 - 1, n/2, n - 1), two rows of random signs and a smooth profile from n = 511 to 4096 =
kFhtMaxN.  Four mutated references -- the Nyquist term dropped, its sign flipped, the last m of the inverse sum left out, the output not
reversed -- must each miss the true one by 100 bounds somewhere at every n (the two Nyquist ones exist for even n only).

Measured on an MI355X, worst observed / bound over the parameter triples: n = 4: 0.038, 5: 0.029, 7: 0.025, 8: 0.031, 63: 0.010, 64: 0.011,
255: 0.0028, 256: 0.0030, 257: 0.0037, 511: 0.0013, 512: 0.0015, 1100: 0.0008, 4095: 0.0005, 4096: 0.0005 (the bound is a worst case over
signs; the sums behave like sqrt n).  Every mutated reference was rejected at every n.

pchip_rows_kernel, through bfgx_pchip_rows: dyadic inputs (slopes and sign tests exact on both sides) against the exact rational PCHIP;
K_p 2^-52 (|y_lo| + |y_lo+1| + dx (|d_lo| + |d_lo+1|)) per query with K_p = 8.8, four times the 2.19 that scipy's double
PchipInterpolator needs on these inputs; knots and ends bit for bit, 0.0 outside, for inf and for NaN.  When this test was written the
last knot came out of the last interval's cubic at s = dx, which only rounds to y[n - 1] (scipy's does the same: 10.500000000000002 for
10.5); pchip_rows_kernel now returns y[n - 1] there.  Measured on an MI355X, worst observed / (2^-52 scale): 0.00 at n = 2, 0.09 / 0.50
(uniform / varying spacing) at n = 3, 0.07 / 0.45 at 4, 0.28 / 1.35 at 17 and at 300.

bfgx_fftlog_convolve: the first stage's bound b1 enters the second stage's A as sum_p b1_p, the second stage's bound b2 reaches the
query through the interpolant's Lipschitz factor: a cubic Hermite value is h00 y_lo + h01 y_lo+1 + dx (h10 d_lo + h11 d_lo+1) with
|h00| + |h01| = 1 and |h10| + |h11| <= 1/4; a Fritsch-Butland derivative moves by at most 3 per unit of either secant (its weights
are at least a third of their sum), a secant by 2 b / h, so d by 12 b / h_min and the value by (1 + 3 dx / h_min) b -- as long as no
sign decision flips, which the test first checks on the reference: every tested quantity is 1e6 of its possible error from zero.  On top:
the cubic's own rounding (K_p as above), one ulp in each logarithm of the abscissae times the largest derivative, 4 ulp of the result.
(The error the first stage leaves in the second stage's input also travels through the second transform itself, as at most
sum_p b1_p U |post|; the bound as stated does not add that term, and the kernels do not need it.)  Measured on an MI355X, worst observed /
bound: 0.031 to 0.059 at n = 4, 0.0001 to 0.0006 at n = 64, at most 0.0001 at n = 257; the smallest sign margin is 1.37e6 (n = 257,
nq = 300, dim 3, no window), found on the CPU.
"""
import math

import numpy as np
import pytest

import fftlog_oracle as O
from baryonification_amd.utils.Pixel import _convolve, _kgrid, fftlog_transform, fftlog_u, pchip_rows

pytestmark = pytest.mark.gpu

MAIN = [(3, 0, -1.5), (2, 0, -0.5)]                       # the second takes clngamma's reflection
OTHERS = [t for t in O.TRIPLES if t not in MAIN]


def _grid(n):
    return np.geomspace(1e-2, 1e2, n) if n <= 64 else O.log_grid(n, 100, 10.0 ** (-0.5 * (n - 1) / 100.0))


def _smooth(r):
    return np.exp(-(r / 0.3) ** 1.3) / (1 + (r / 0.05) ** 0.7)


def _check_transform(r, rows, dim, mu, plaw, mutations=True):
    """one bfgx_fftlog_transform call against the long-double transform; returns the worst observed / bound and the result.
    `mutations`: the rows must also tell every mutated reference from the true one (a smooth row alone does not: the reason for unit rows)"""
    n = r.size
    u, lnkr = fftlog_u(r, dim, mu, plaw)
    k, T = fftlog_transform(r, rows, dim, mu, plaw)
    T = np.atleast_2d(T)
    k_ref, ref, bound, _ = O.ld_transform(r, rows, dim, mu, plaw, u, lnkr)
    assert np.abs(k.astype(O.LD) / k_ref - 1).max() <= 4 * O.EPS
    assert np.isfinite(T).all() and (bound > 0).all()
    ratio = np.abs(T.astype(O.LD) - ref) / bound
    worst = float(ratio.max())
    where = np.unravel_index(np.argmax(ratio), ratio.shape)
    # the mutated references are told from the true one by the same bound
    for mut in (O.MUTATIONS if mutations else ()):
        if n % 2 and mut.startswith('nyquist'):
            continue
        miss = float((np.abs(O.ld_transform(r, rows, dim, mu, plaw, u, lnkr, mut)[1] - ref) / bound).max())
        assert miss >= 100, "n = %d (%d, %g, %g): the reference with %s is only %.3g bounds away" % (n, dim, mu, plaw, mut, miss)
    assert worst <= 1, "n = %d (%d, %g, %g): row %d element %d is %.3g bounds from the reference" % ((n, dim, mu, plaw) + where + (worst,))
    return worst, T


@pytest.mark.parametrize('n', [4, 5, 7, 8, 63, 64, 255, 256, 257])
def test_fht_every_matrix_element(gpu, n):
    O.require_longdouble()
    r = _grid(n)
    worst = {}
    for dim, mu, plaw in MAIN + (OTHERS if n in (64, 257) else []):
        worst[(dim, mu, plaw)], _ = _check_transform(r, np.eye(n), dim, mu, plaw)
    print("fht_rows_kernel n = %4d, %d unit rows: worst observed / bound %.4f  (%s)"
          % (n, n, max(worst.values()), ", ".join("%s: %.4f" % kv for kv in worst.items())))


@pytest.mark.parametrize('n', [511, 512, 1100, 4095, 4096])
def test_fht_large_n(gpu, n):
    O.require_longdouble()
    r = _grid(n)
    rng = np.random.default_rng(n)
    rows = np.zeros((8, n))
    for i, j in enumerate((0, 1, n // 2 - 1, n // 2, n - 1)):
        rows[i, j] = 1.0
    rows[5:7] = rng.choice([-1.0, 1.0], size=(2, n))
    rows[7] = _smooth(r)
    worst = {}
    for dim, mu, plaw in MAIN:
        worst[(dim, mu, plaw)], T = _check_transform(r, rows, dim, mu, plaw)
        w1, T1 = _check_transform(r, rows[7:], dim, mu, plaw, mutations=False)                  # one row, one workgroup
        assert np.array_equal(T1[0], T[7])
        worst[(dim, mu, plaw)] = max(worst[(dim, mu, plaw)], w1)
    print("fht_rows_kernel n = %4d, 8 + 1 rows: worst observed / bound %.4f  (%s)"
          % (n, max(worst.values()), ", ".join("%s: %.4f" % kv for kv in worst.items())))


# ---------------------------------------------------------------------------------------------------- pchip_rows_kernel
NQ = (1, 255, 256, 257, 1000)


@pytest.mark.parametrize('spacing', ['uniform', 'varying'])
@pytest.mark.parametrize('n', O.PCHIP_N)
def test_pchip_rows(gpu, n, spacing):
    x, Y = O.pchip_knots(n, spacing), O.pchip_rows(n)
    pool = O.pchip_queries(x)
    refs = [O.pchip_reference(x, y, pool) for y in Y]                          # once per input, shared by the calls below
    at_knot = np.isin(pool, x)
    y_at = np.searchsorted(x, np.where(at_knot, pool, x[0]))
    worst, start, seen = 0.0, 0, set()
    for nq in NQ:
        idx = (start + np.arange(nq)) % pool.size
        start += nq
        seen.update(idx.tolist())
        got = pchip_rows(x, Y, pool[idx])
        assert got.shape == (len(Y), nq)
        for row, (val, scale, inside) in enumerate(refs):
            label = (n, spacing, O.PCHIP_ROWS[row], nq)
            g, ins, kn = got[row], inside[idx], at_knot[idx]
            assert (g[~ins] == 0.0).all(), label                                # outside, +-inf, NaN: exactly 0
            assert np.array_equal(g[kn], Y[row][y_at[idx][kn]]), label           # knots and both ends: bit for bit
            ratio = O.pchip_ratios(g[ins], val[idx][ins], scale[idx][ins])
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= O.K_PCHIP, label + (pool[idx][ins][np.argmax(ratio)], float(ratio.max()))
        one = pchip_rows(x, Y[0], pool[idx])                                   # nrows = 1
        assert np.array_equal(one, got[0])
    assert len(seen) == pool.size                                              # every query of the pool went through the kernel
    print("pchip_rows_kernel n = %3d %-7s: %d queries x 7 rows, worst observed / (2^-52 scale) %.3f (K_p = %.1f)" % (n, spacing, pool.size, worst, O.K_PCHIP))


# ---------------------------------------------------------------------------------------------------- the chain
def chain_case(n, nq, dim, window):
    """inputs of one bfgx_fftlog_convolve call: a Gaussian profile on the FFTLog grid, a Gaussian window or none, and r_eval: points in
    range, two r_out knots (one exact, one through exp(log), so to rounding), two points out of range"""
    r = _grid(n)
    plaw_fwd, plaw_back = (-1.5, -0.5) if dim == 3 else (-0.5, -0.5)             # ConvolvedProfile.real / .projected, pyccl's defaults
    prof = np.stack([np.exp(-r ** 2 / (2 * s ** 2)) for s in (1.0, 0.5)])
    k1 = _kgrid(r, dim, 0, plaw_fwd)
    r_out = _kgrid(k1, dim, 0, plaw_back)
    win = np.exp(-k1 ** 2 * 0.3 ** 2 / 2) if window == 'gauss' else np.ones(n)
    lo, hi = (r_out[0], r_out[-1]) if n == 4 else (0.25, 1.5)
    inside = np.geomspace(lo * 1.0001, hi, max(nq - 4, 1))
    if nq == 1:
        r_eval = inside
    else:
        ka, kb = np.searchsorted(r_out, [0.4, 1.1]) if n > 4 else (1, 2)
        r_eval = np.concatenate([inside, [r_out[ka], math.exp(math.log(r_out[kb])), r_out[0] * 0.999, r_out[-1] * 1.001]])
    return r, prof, dim, plaw_fwd, plaw_back, win, k1, r_out, r_eval


def chain_reference(case):
    r, prof, dim, plaw_fwd, plaw_back, win, k1, r_out, r_eval = case
    x = [math.log(v) for v in r_out]
    lnq = [math.log(v) for v in r_eval]
    return O.ld_chain(r, prof, dim, 0, plaw_fwd, plaw_back, win, k1, x, lnq, fftlog_u(r, dim, 0, plaw_fwd), fftlog_u(k1, dim, 0, plaw_back))


@pytest.mark.parametrize('window', ['gauss', 'ones'])
@pytest.mark.parametrize('dim', [2, 3])
@pytest.mark.parametrize('nq', [1, 300])
@pytest.mark.parametrize('n', [4, 64, 257])
def test_convolve_chain(gpu, n, nq, dim, window):
    O.require_longdouble()
    case = chain_case(n, nq, dim, window)
    r, prof, dim, plaw_fwd, plaw_back, win, k1, r_out, r_eval = case
    ref, tol, margin = chain_reference(case)
    assert margin >= 1e6, "a sign decision of the interpolant is only %.3g possible errors from flipping: not a case for this test" % margin
    got = _convolve(r, prof, dim, plaw_fwd, plaw_back, win, r_eval, 1.0)
    assert got.shape == ref.shape == (2, nq)
    outside = (r_eval < r_out[0]) | (r_eval > r_out[-1])
    assert outside.sum() == (2 if nq > 1 else 0) and (got[:, outside] == 0.0).all()
    ins = ~outside
    assert (tol[:, ins] > 0).all()
    ratio = np.abs(got.astype(O.LD) - ref)[:, ins] / tol[:, ins]
    print("bfgx_fftlog_convolve n = %3d nq = %3d dim %d %-5s: worst observed / bound %.4f, sign margin %.3g" % (n, nq, dim, window, float(ratio.max()), margin))
    assert ratio.max() <= 1
