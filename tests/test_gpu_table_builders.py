"""The four table-builder kernels of csrc/bfgx_tables.hpp away from the golden shapes: every case runs a
`baryonification_amd.tables` front-end and oracle/tables.py (numpy + scipy) on the same synthetic, seeded input.

What the shapes are for
  displacement_rows   N_R on both sides of the 256-thread block (chunks of one and of several nodes, the carry of the last
                      kept node from chunk to chunk, up to ten laps of the `i += 256` loops), statuses 0, 1 and 2, and the
                      admitted maximum tables.MAX_N_R, whose row fills the workgroup's LDS
  enclosed mass       rows shorter than the block, at multiples of it and at the 50 000 the builders use; two to four
                      usable samples (PCHIP's n == 2 form, both end-slope stencils); holes, negative patches, inf; queries
                      on a node and outside the table; a second lap of the output loop
  pressure_profile    ln P with local extrema and with each of scipy's end-slope rules (plain, set to zero, capped at 3 m0)
  project_profile     nl = 2 and the maximum 2048, a second block in x, a column where every node takes the clamp

Every case builder asserts ON THE ORACLE SIDE that the branch it is there for is reached, and that the oracle's statuses,
NaN patterns and zeros do not move when the sampled profile is multiplied by (1 + 1e-15 N(0, 1)): a case that fails this
has to be moved, not the assertion.  Only the sampled values are perturbed, never the radial grids: a query "exactly on a
node" has to stay on it, and both sides take the grid's logarithms from identical bits.

scipy refuses a non-finite y and fewer than two points, so rows with fewer than two usable samples and pressure rows
whose running sum changes sign (ln of a negative number) are left out: what the kernels do there has no reference.

Bounds are the ones tests/test_tables.py holds these kernels to (projection 1e-12, enclosed mass 1e-10, pressure 1e-10
relative; displacement 1e-9 max|d|), or ten times the oracle's own sensitivity to that 1e-15 perturbation where that is
larger (the device's log / exp differ from libm by an ulp or two and the sums run in another order).  Each test prints
the worst error, the sensitivity and the bound in force.

Measured on an MI355X (worst over all cases; oracle sensitivity in brackets): displacement 4.2e-15 max|d| (2e-14),
enclosed mass 7.1e-15 (5.4e-15), pressure 1.4e-14 (1.4e-14), projection 5.2e-15 (2.6e-15).  No case needs the
sensitivity bound: the bounds of tests/test_tables.py are in force everywhere.

The n_int = 50 000 row with an inf found a defect: block_excl_scan_sum returned (inclusive sum - own value), which is
inf - inf = NaN for the thread whose 49 samples hold the inf, so the usable samples before the inf in that thread's chunk
were dropped and the table ended up to 48 nodes early.
"""
import functools

import numpy as np
import pytest
from scipy import interpolate

from oracle import tables as OT

pytestmark = pytest.mark.gpu

PERT = 1e-15


def _perturbed(a, seed):
    """a (1 + 1e-15 N(0, 1)): zeros, infinities, NaNs and signs stay what they are"""
    return a * (1.0 + PERT * np.random.default_rng(seed).standard_normal(a.shape))


def _rel(a, ref):
    """largest |a / ref - 1| over the finite, non-zero entries of ref (0 if there are none)"""
    ok = np.isfinite(ref) & (ref != 0)
    return float(np.abs(a[ok] / ref[ok] - 1).max()) if ok.any() else 0.0


def _bound(base, sens):
    return max(base, 10.0 * sens)


# ------------------------------------------------------------------------------------------------- displacement
DISP_SIZES = (6, 255, 256, 257, 300, 1000, 'max')


def _disp_nr(size):
    from baryonification_amd import tables as T
    return T.MAX_N_R if size == 'max' else size


@functools.lru_cache(maxsize=None)
def _displacement_case(n):
    r = np.geomspace(1e-3, 3e2, n)
    base = 1e14 * r ** 1.5 / (1 + (r / 2.0) ** 1.5)
    M_dmo = base
    smooth = base * (1 + 0.05 * np.tanh(np.log(r)))
    per = -(-n // 256)                                   # nodes per thread chunk in displacement_kernel
    if n == 6:
        nan = smooth.copy()
        nan[3] = np.nan                                  # 5 nodes left: not "> 5"
        half = smooth.copy()
        half[:3] = M_dmo[:3]
        rows, expect = [smooth, nan, half], [0, 2, 2]
    else:
        k = n // 3
        spike40 = smooth.copy()
        spike40[k] = 1.0001 * smooth[k + 40]             # one node peeled per iteration: more than 30
        spike20 = smooth.copy()
        spike20[k] = 1.0001 * smooth[k + 20]
        flat = smooth.copy()
        a = per * 37 - 5
        flat[a:a + 10] = flat[a - 1]                     # 10 flat nodes across the boundary between chunks 36 and 37
        flat[per * 45 - 1] = np.nan                      # last node of chunk 44
        assert a // per < (a + 9) // per and a + 10 < per * 45 - 1 < n
        half = smooth.copy()
        half[:n // 2] = M_dmo[:n // 2]
        rows, expect = [smooth, spike40, spike20, flat, half], [0, 1, 0, 0, 0]
        assert (per >= 2) == (n > 256)
    M_dmb = np.stack(rows)
    M_dmo = np.broadcast_to(M_dmo, M_dmb.shape).copy()
    d, st = OT.displacement_rows(r, M_dmo, M_dmb)
    assert st.tolist() == expect, (n, st)
    assert np.all(d[st != 0] == 0) and all(np.abs(d[i]).max() > 0 for i in np.flatnonzero(st == 0))
    dp, stp = OT.displacement_rows(r, _perturbed(M_dmo, 10 * n), _perturbed(M_dmb, 10 * n + 1))
    assert np.array_equal(st, stp) and np.array_equal(d == 0, dp == 0), "case is not robust: move the input"
    sens = np.array([np.abs(dp[i] - d[i]).max() / max(np.abs(d[i]).max(), 1e-300) for i in range(len(rows))])
    return dict(r=r, M_dmo=M_dmo, M_dmb=M_dmb, d=d, st=st, sens=sens)


@pytest.mark.parametrize('size', DISP_SIZES)
def test_displacement_rows_chunks_laps_and_statuses(gpu, size):
    """Smooth, 40-node spike (status 1), 20-node spike, flat stretch + NaN across a chunk boundary, half the row equal
    to the DMO mass; at N_R = 6 rows of status 0, 2, 2.  Statuses equal the oracle's, d is exactly 0 where the status
    is not 0, and each row is within 1e-9 of its own max|d| (or ten times the oracle's sensitivity)."""
    from baryonification_amd import tables as T
    c = _displacement_case(_disp_nr(size))
    d, st = T.displacement_rows(c['r'], c['M_dmo'], c['M_dmb'])
    assert np.array_equal(st, c['st']), (st, c['st'])
    assert np.all(d[c['st'] != 0] == 0)
    assert np.array_equal(d == 0, c['d'] == 0)
    for i in range(d.shape[0]):
        scale = max(np.abs(c['d'][i]).max(), 1e-300)
        err = np.abs(d[i] - c['d'][i]).max() / scale
        bound = _bound(1e-9, c['sens'][i])
        print('N_R %4d row %d status %d: max|d - oracle| / max|d| = %.3e  (oracle sensitivity %.3e, bound %.3e)'
              % (c['r'].size, i, st[i], err, c['sens'][i], bound))
        assert err <= bound


# ------------------------------------------------------------------------------------------------- enclosed mass
ENC_SIZES = (3, 5, 1023, 1024, 1025, 2049, 50_000)
ENC_ORACLE = {2: OT.enclosed_mass_from_sigma, 3: OT.enclosed_mass_3d}


def _enc_rows(n, r_int):
    """(name, sampled profile, index of the first usable node); rows with fewer than two usable samples are left out"""
    plain = 1.0 / (r_int * (1 + r_int) ** 2)
    rows = [('plain', plain)]
    w = max(1, n // 10)
    s = plain.copy(); s[n // 2:n // 2 + w] = 0.0
    rows.append(('zero hole', s))
    s = plain.copy(); s[n // 3:n // 3 + w] *= -1e-3
    rows.append(('negative patch', s))
    s = plain.copy(); s[:max(1, n // 4)] = 0.0
    rows.append(('first quarter zero', s))
    s = plain.copy(); s[(3 * n) // 4] = np.inf
    rows.append(('inf at three quarters', s))
    for k in (2, 3, 4):
        pad = n // 4 if n >= 16 else 0                              # (short rows need every node to reach k samples)
        idx = np.unique(np.round(np.linspace(pad, n - 1 - pad, k)).astype(int))
        if idx.size == k:
            s = np.zeros(n); s[idx] = plain[idx]
            rows.append(('%d positive samples' % k, s))
    out = []
    for name, s in rows:
        sc = np.where(s < 0, 0, s)
        usable = np.flatnonzero((sc > 0) & np.isfinite(np.cumsum(sc)))
        if usable.size >= 2:
            out.append((name, s, usable))
    return out


@functools.lru_cache(maxsize=None)
def _enclosed_case(n, n_out):
    r_int = np.geomspace(1e-3, 1e2, n)
    rows = _enc_rows(n, r_int)
    names = [x[0] for x in rows]
    S = np.stack([x[1] for x in rows])
    firsts = sorted({int(x[2][0]) for x in rows})
    lasts = sorted({int(x[2][-1]) for x in rows})
    nodes = r_int[firsts + lasts]                                   # queries exactly on first / last usable nodes
    r = np.concatenate([np.geomspace(3e-4, 3e2, n_out - nodes.size), nodes])
    assert r.size == n_out and (r < r_int[0]).sum() >= 1 and (r > r_int[-1]).sum() >= 1
    ref, sens = {}, {}
    for dim, fn in ENC_ORACLE.items():
        m = fn(r_int, S, r)
        mp = fn(r_int, _perturbed(S, 7 * n + dim), r)
        assert np.array_equal(np.isnan(m), np.isnan(mp)), "case is not robust: move the input"
        outside = (r < r_int[0]) | (r > r_int[-1])
        assert np.all(np.isnan(m[:, outside]))                      # NaN outside the table
        for i, (_, _, usable) in enumerate(rows):                   # a query on the first usable node, NaN just below it
            j = int(np.flatnonzero(r == r_int[usable[0]])[0])
            assert np.isfinite(m[i, j]) and np.all(np.isnan(m[i, r < r_int[usable[0]]]))
            assert np.isfinite(m[i, np.flatnonzero(r == r_int[usable[-1]])[0]])
        ref[dim] = m
        sens[dim] = np.array([_rel(mp[i], m[i]) for i in range(len(rows))])
    counts = {x[0]: x[2].size for x in rows}
    if n >= 5:
        assert counts['2 positive samples'] == 2 and counts['3 positive samples'] == 3 and counts['4 positive samples'] == 4
        assert rows[names.index('first quarter zero')][2][0] == max(1, n // 4)
        assert rows[names.index('inf at three quarters')][2][-1] == (3 * n) // 4 - 1
    else:
        assert counts['2 positive samples'] == 2 and counts['plain'] == 3
    return dict(r_int=r_int, S=S, r=r, names=names, ref=ref, sens=sens)


@pytest.mark.parametrize('dim', (2, 3))
@pytest.mark.parametrize('n_int,n_out', [(n, 17) for n in ENC_SIZES] + [(1025, 1500), (50_000, 1500)])
def test_enclosed_mass_row_lengths_masks_and_node_queries(gpu, n_int, n_out, dim):
    """Plain row, zero hole, negative patch, first quarter zero, inf at three quarters, exactly 2 / 3 / 4 positive
    samples; queries outside the table (NaN), on the first and on the last usable node of every row.  The NaN pattern
    equals the oracle's, the finite entries agree to 1e-10 relative (or ten times the oracle's sensitivity)."""
    from baryonification_amd import tables as T
    c = _enclosed_case(n_int, n_out)
    fn = T.enclosed_mass_from_sigma if dim == 2 else T.enclosed_mass_3d
    m = fn(c['r_int'], c['S'], c['r'])
    ref = c['ref'][dim]
    bad = np.argwhere(np.isnan(m) != np.isnan(ref))
    assert bad.size == 0, 'NaN pattern differs at (row, r, hip, oracle): %s' % [(c['names'][i], c['r'][j], m[i, j], ref[i, j]) for i, j in bad[:8]]
    worst = []
    for i, name in enumerate(c['names']):
        err, sens = _rel(m[i], ref[i]), c['sens'][dim][i]
        worst.append((err, sens, name))
        assert err <= _bound(1e-10, sens), (name, err, sens)
    err, sens, name = max(worst)
    print('dim %d n_int %5d n_out %4d: worst |M / oracle - 1| = %.3e in row "%s" (oracle sensitivity %.3e, bound %.3e; %d rows)'
          % (dim, n_int, n_out, err, name, sens, _bound(1e-10, sens), len(worst)))


# ------------------------------------------------------------------------------------------------- PCHIP rules (pressure)
def _edge_rule(h0, h1, m0, m1):
    """which of scipy's end-slope rules (PchipInterpolator._edge_case) applies, and the slope it gives"""
    d = ((2 * h0 + h1) * m0 - h0 * m1) / (h0 + h1)
    if np.sign(d) != np.sign(m0):
        return 'zero', 0.0
    if np.sign(m0) != np.sign(m1) and abs(d) > 3 * abs(m0):
        return 'capped', 3 * m0
    return 'plain', d


@functools.lru_cache(maxsize=None)
def _pressure_case():
    r = np.geomspace(1e-6, 1000, 500)
    rho_tot = np.tile(1e14 / (r * (1 + r) ** 2), (3, 1))
    rho_gas = 0.1 * rho_tot
    rho_gas[:, 200:215] *= -1.0                       # ln P rises again towards small r: two interior extrema
    rho_gas[0, 330:335] *= -1.0                       # a second, shorter patch
    rho_gas[0, 498] *= -0.1                           # outer end: slopes of opposite sign, |m1| > 3 |m0| -> 3 m0
    rho_gas[1, 498] *= 0.01                           # outer end: same sign, m1 > 3 m0 -> 0
    rho_gas[1, 420:423] *= -1.0
    rho_gas[2, 498] *= -0.5                           # outer end: opposite sign, not capped
    rho_gas[2] *= 1.7
    # ln P on the nodes, as oracle/tables.py::pressure_profile forms it
    dlnr = np.log(r[1]) - np.log(r[0])
    M_total = 4 * np.pi * np.cumsum(r ** 3 * rho_tot * dlnr, axis=-1)
    dP_dr = -OT.G_MPC * M_total * rho_gas / r ** 2
    prof = -np.cumsum((dP_dr * r)[:, ::-1] * dlnr, axis=-1)[:, ::-1]
    assert np.all(prof > 0), "the running sum changes sign: scipy has no answer for such a row"
    x, y = np.log(r), np.log(prof + OT.PRESSURE_AT_INFINITY)
    rules = set()
    for i in range(3):
        m = np.diff(y[i]) / np.diff(x)
        assert (np.sign(m[1:]) * np.sign(m[:-1]) < 0).sum() >= 2                        # interior local extrema
        der = interpolate.PchipInterpolator(x, y[i]).derivative()
        for (h0, h1, m0, m1, xe) in ((x[1] - x[0], x[2] - x[1], m[0], m[1], x[0]),
                                    (x[-1] - x[-2], x[-2] - x[-3], m[-1], m[-2], x[-1])):
            rule, d = _edge_rule(h0, h1, m0, m1)
            assert abs(der(xe) - d) <= 1e-9 * max(abs(d), abs(m0))                       # scipy does take that rule
            rules.add(rule)
    assert rules == {'plain', 'zero', 'capped'}, rules
    assert any(np.sign(np.diff(y[i])[-1]) != np.sign(np.diff(y[i])[-2]) for i in range(3))   # sign change next to an end interval
    mid = lambda a, b: np.sqrt(r[a] * r[b])
    r_use = np.concatenate([np.geomspace(1e-3, 50, 300), [1e-6, 1e3],
                            [mid(0, 1), mid(1, 2), mid(497, 498), mid(498, 499)],       # inside the end intervals
                            [0.5e-6, 1.5e3]])                                           # beyond both ends: 0
    ref, sens = {}, {}
    for cutoff in (np.inf, 20.0):
        P = OT.pressure_profile(rho_tot, rho_gas, r_use, cutoff=cutoff)
        Pp = OT.pressure_profile(_perturbed(rho_tot, 11), _perturbed(rho_gas, 12), r_use, cutoff=cutoff)
        assert np.all(np.isfinite(P)) and np.all(P[:, -2:] == 0) and np.all(P[:, :300] > 0)
        assert np.array_equal(P == 0, Pp == 0), "case is not robust: move the input"
        if np.isfinite(cutoff):
            assert (r_use - cutoff > 30).any() and np.all(P[:, r_use - cutoff > 30] == 0)
        ref[cutoff] = P
        sens[cutoff] = np.array([_rel(Pp[i], P[i]) for i in range(3)])
    return dict(rho_tot=rho_tot, rho_gas=rho_gas, r_use=r_use, ref=ref, sens=sens)


@pytest.mark.parametrize('cutoff', (np.inf, 20.0))
def test_pressure_profile_extrema_and_end_slope_rules(gpu, cutoff):
    """ln P with interior extrema (gas density flipped over nodes 200-214 and shorter patches) and an outer end that
    takes, row by row, the capped, the zeroed and the plain end slope; radii inside the end intervals, on the end nodes
    and beyond them (exactly 0).  1e-10 relative, or ten times the oracle's sensitivity."""
    from baryonification_amd import tables as T
    c = _pressure_case()
    P = T.pressure_profile(c['rho_tot'], c['rho_gas'], c['r_use'], cutoff=cutoff)
    ref = c['ref'][cutoff]
    assert np.all(np.isfinite(P)) and np.array_equal(P == 0, ref == 0)
    for i in range(3):
        err, sens = _rel(P[i], ref[i]), c['sens'][cutoff][i]
        ends = _rel(P[i, 300:306], ref[i, 300:306])
        print('cutoff %4s row %d: max|P / oracle - 1| = %.3e (end nodes and end intervals %.3e; oracle sensitivity %.3e, bound %.3e)'
              % (cutoff, i, err, ends, sens, _bound(1e-10, sens)))
        assert err <= _bound(1e-10, sens)


# ------------------------------------------------------------------------------------------------- projection
PROJ_SHAPES = ((2, 1), (60, 255), (60, 256), (60, 257), (2048, 513))
PROJ_SCALE = 0.37


@functools.lru_cache(maxsize=None)
def _projection_case(nl, nr):
    rng = np.random.default_rng(1000 * nl + nr)
    steps = rng.uniform(0.2, 1.8, nl - 1)                                # uneven steps in ln l: not a geomspace
    l = 1e-3 * np.exp(np.concatenate([[0.0], np.cumsum(steps) * np.log(5e4) / steps.sum()]))
    assert np.all(np.diff(l) > 0) and (nl == 2 or np.ptp(np.diff(np.log(l))) > 0.1 * np.log(5e4) / nl)
    rho = np.stack([1.0 / ((l / rs) * (1 + l / rs) ** 2) * (1 + b * np.exp(-np.log(l / 0.7) ** 2)) for rs, b in ((0.3, 0.0), (1.5, 0.0), (0.5, 4.0))])
    if nr == 1:
        r = np.array([2.0 * l[-1]])                                      # the one column clamps
    else:
        r = np.concatenate([[0.5 * l[0]], np.geomspace(2 * l[0], 0.9 * l[-1], nr - 2), [1.5 * l[-1]]])
    ref = OT.project_realspace(l, rho, r) * PROJ_SCALE
    clamp = 2.0 * rho[:, -1] * (l[-1] - l[0]) * PROJ_SCALE               # every node beyond l[-1]: 2 trapz(rho[-1], l)
    assert r[-1] > l[-1] and np.abs(ref[:, -1] / clamp - 1).max() < 1e-12
    assert nr == 1 or r[0] < l[0]
    sens = _rel(OT.project_realspace(l, _perturbed(rho, nl + nr), r) * PROJ_SCALE, ref)
    return dict(l=l, rho=rho, r=r, ref=ref, sens=sens)


@pytest.mark.parametrize('nl,nr', PROJ_SHAPES)
def test_project_profile_blocks_node_counts_and_clamp_column(gpu, nl, nr):
    """Three rows on an uneven l, scale 0.37, one r below l[0] and one beyond l[-1] (every node clamps to rho[-1]);
    nl = 2 and the maximum 2048, nr on both sides of one 256-thread block.  1e-12 relative."""
    from baryonification_amd import tables as T
    c = _projection_case(nl, nr)
    s = T.project_profile(c['l'], c['rho'], c['r'], scale=PROJ_SCALE)
    assert s.shape == c['ref'].shape and np.all(np.isfinite(s))
    err = _rel(s, c['ref'])
    print('nl %4d nr %3d: max|Sigma / oracle - 1| = %.3e (clamp column %.3e; oracle sensitivity %.3e, bound %.3e)'
          % (nl, nr, err, _rel(s[:, -1], c['ref'][:, -1]), c['sens'], _bound(1e-12, c['sens'])))
    assert err <= _bound(1e-12, c['sens'])
