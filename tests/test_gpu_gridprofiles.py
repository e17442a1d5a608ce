"""GPU checks of bfg.Runners.MeasureProfilesGrid (csrc/bfgx_grid_stack.hpp): parity with the brute-force numpy oracle
(gridprofiles_oracle.py) in 2-D and 3-D, scaled and unscaled; the smallest shapes at which the kernel can go wrong (an axis covered
completely, a ball that wraps on every axis at once, 1 and 64 bins, no halo, invalid halos only, a constant map); the flat-sky shear about
an analytic tangential field and about random fields; host entry == device entry; and BaryonifyGrid measured before and after.

Bounds (derived, not measured).  eps = 2.2e-16.  Per (halo, bin) cell without an ambiguous pixel: npix and npix_shear equal, and
    |sum - sum_o| <= 2 npix eps S,                     S = sum |v| over the cell  (two fp64 summations of npix terms in any order);
    |sum_t - sum_t_o|, |sum_x - sum_x_o| <= (2 npix_shear + 16) eps S,   S = sum (|g1| + |g2|) over the cell.
The 16: per pixel both sides form c2 and s2 from the same Deltas (|c2|, |s2| <= 1).  With u = eps / 2 per rounding, d2 carries 2 u,
1 / d2 one more; the kernel's c2 = (Dx - Dy)(Dx + Dy) / d2 has 7 u, its s2 5 u; numpy's (Dx Dx - Dy Dy) / d2 has 5 u, its s2 4 u; the two
products and the sum of g1 c2 + g2 s2 add 2 u (|g1| + |g2|) on each side: at most 16 u (|g1| + |g2|) = 8 eps (|g1| + |g2|) per pixel.
A pixel is ambiguous when |d - R_q| <= 1e-9 R_q or |x - e| <= 1e-9 e for some edge e > 0 (x = 0 at an edge 0 is exact on both sides: that
cell keeps the plain bounds); it is charged to its own bin and both neighbours.
Cells with ambiguous pixels get the same bounds with npix and S widened by those pixels' count and sum |v|, plus that sum |v|; their
share of all cells is a condition on the inputs, asserted <= 1e-3."""
import ctypes as C
import functools

import numpy as np
import pytest

import gridprofiles_oracle as K

pytestmark = pytest.mark.gpu

EPS = 2.2e-16
ZR = 0.2


def _objects(cat, m, bins, ndim, zr=ZR):
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    HCat = bfg.utils.HaloNDCatalog(x=cat['x'], y=cat['y'], z=cat['z'] if ndim == 3 else None, M=cat['M'], redshift=zr, cosmo=dict(syn.COSMO))
    Map = bfg.utils.GriddedMap(map=m, redshift=zr, bins=bins, cosmo=dict(syn.COSMO))
    return HCat, Map


def _used(HCat):
    return {k: np.array(HCat.cat[k], dtype=np.float64) for k in ('M', 'x', 'y', 'z')}


def _background():
    from baryonification_amd import synthetic as syn
    from oracle import grid as G
    return G.grid_background(syn.COSMO)


def _bins(N, L):
    return (np.arange(N) + 0.5) * L / N


def _mass_for_ball(R_q, eps, zr=ZR):
    """the mass whose ball epsilon_max R_com is R_q (R_com goes as M^(1/3))"""
    a = 1.0 / (1.0 + zr)
    R0 = _background().get_radius(1e14, a) / a
    return 1e14 * (R_q / (eps * R0)) ** 3


def _get(v):
    return v.cpu().numpy() if hasattr(v, 'cpu') else np.asarray(v)


def _compare(res, o, label, max_share=1e-3):
    """asserts the bounds of the module docstring; prints and returns the ambiguous share and the largest error / bound ratios"""
    amb = o['amb_n'] > 0
    share = float(amb.mean()) if amb.size else 0.0
    stats = {'ambiguous_cell_share': share, 'cells': int(amb.size), 'pairs': o['pairs'], 'ambiguous_pixels': o['amb_pixels']}
    checks = [('npix', 'sum', 'S', 'amb_abs', 0)]
    if 'sum_t' in o:
        checks += [('npix_shear', 'sum_t', 'S_shear', 'amb_abs_shear', 16), ('npix_shear', 'sum_x', 'S_shear', 'amb_abs_shear', 16)]
        assert res.npix_shear is not None and res.sum_t is not None and res.sum_x is not None, label
    else:
        assert res.npix_shear is None and res.sum_t is None and res.sum_x is None, label
    verdict = []
    for cnt, tot, S, amb_abs, extra in checks:
        n, s = _get(getattr(res, cnt)), _get(getattr(res, tot))
        assert n.dtype == np.int64 and n.shape == o[cnt].shape and s.dtype == np.float64 and s.shape == o[tot].shape, (label, cnt, tot)
        bound = (2 * (o[cnt] + o['amb_n']) + extra) * EPS * (o[S] + o[amb_abs]) + o[amb_abs]
        err = np.abs(s - o[tot])
        with np.errstate(divide='ignore', invalid='ignore'):
            stats[tot] = float(np.max(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)), initial=0.0))
        verdict.append((cnt, tot, np.array_equal(n[~amb], o[cnt][~amb]) and bool(np.all(np.abs(n - o[cnt]) <= o['amb_n'])), bool(np.all(err <= bound))))
    print('%s: %s' % (label, stats))
    assert share <= max_share, (label, stats)
    for cnt, tot, counts_ok, sums_ok in verdict:
        assert counts_ok, (label, cnt, stats)
        assert sums_ok, (label, tot, stats)
    return stats


PARITY_EDGES = {False: np.concatenate([[0.0], np.geomspace(0.3, 14.0, 16)]), True: np.geomspace(0.02, 5.0, 17)}
PARITY_ROWS = {'negative': 7, 'zero': 8, 'tiny': 9, 'origin': 10, 'corner': 11, 'huge': 12, 'centred': 13}
PARITY_BOX = {2: (128, 200.0), 3: (48, 75.0)}


@functools.lru_cache(maxsize=None)
def _parity_case(ndim):
    """the inputs of the parity test and the oracle's pairs, once per ndim"""
    rng = np.random.default_rng(70 + ndim)
    (N, L), nh, eps = PARITY_BOX[ndim], 300, 5.0
    bins = _bins(N, L)
    M = (10 ** rng.uniform(12.8, 15.0, nh)).astype(np.float32).astype(np.float64)
    hpos = rng.uniform(0, L, (nh, 3)).astype(np.float32).astype(np.float64)
    R = PARITY_ROWS
    M[R['negative']], M[R['zero']], M[R['tiny']] = -3e13, 0.0, 1e8                        # not halos; a ball with no pixel in it
    M[R['origin']] = M[R['corner']] = np.float64(np.float32(1e15))                         # (balls that reach through every face of the box)
    hpos[R['origin']] = 0.0
    hpos[R['corner']] = np.float32(L)
    M[R['huge']] = np.float64(np.float32(3e17))                                            # clipped to max(bins) / 2 where the box is smaller than its ball
    hpos[R['centred']] = np.float32(bins[5])                                               # effectively on a pixel centre
    m = rng.uniform(0.5, 2.0, (N,) * ndim)
    bad = rng.choice(m.size, 22, replace=False)
    m.flat[bad[:20]] = np.nan
    m.flat[bad[20:]] = np.inf
    cat = {'M': M, 'x': hpos[:, 0], 'y': hpos[:, 1], 'z': hpos[:, 2]}
    HCat, Map = _objects(cat, m, bins, ndim)
    pairs = K.pairs(bins, ndim, _used(HCat), ZR, eps, _background())
    return HCat, Map, eps, pairs, bad


@pytest.mark.parametrize('scaled', [False, True])
@pytest.mark.parametrize('ndim', [2, 3])
def test_parity_with_the_oracle(gpu, ndim, scaled):
    import baryonification_amd as bfg
    HCat, Map, eps, pairs, bad = _parity_case(ndim)
    edges = PARITY_EDGES[scaled]
    o = K.measure(pairs, edges, Map.map, scaled)
    R = PARITY_ROWS
    for row in ('origin', 'corner', 'huge', 'centred'):
        assert o['npix'][R[row]].sum() > 0, row
    for row in ('negative', 'zero', 'tiny'):
        assert not o['npix'][R[row]].any(), row
    # the 3e17 halo: epsilon_max R_com = 79.5 is clipped to max(bins) / 2 = 37.1 in the 3-D box of 75; the 2-D box of 200 holds it unclipped
    assert pairs['R_q'][R['huge']] == (np.max(Map.bins) / 2 if ndim == 3 else eps * pairs['R'][R['huge']]) and o['npix'].sum() > 0.5 * o['pairs']
    # pixels that are not finite lie inside balls and bins, and the oracle does not count them
    inside_bad = np.isin(pairs['pix'][pairs['inside']], bad)
    assert np.count_nonzero(inside_bad) >= 10
    runner = bfg.Runners.MeasureProfilesGrid(HCat, Map, eps, verbose=False, r_edges=edges, scaled=scaled)
    res = runner.process()
    assert isinstance(res.npix, np.ndarray) and res.npix.shape == (300, 16) and res.ndim == ndim and res.scaled == scaled
    assert res.res == Map.bins[1] - Map.bins[0]
    _compare(res, o, 'parity %d-D scaled %s' % (ndim, scaled))
    assert np.all(np.isfinite(res.sum))                               # no NaN and no inf pixel was added
    every = K.measure(pairs, edges, np.ones_like(Map.map), scaled)['npix']           # ... and none was counted
    assert (every - o['npix']).sum() >= 10 and np.all(res.npix <= every)
    for row in ('negative', 'zero', 'tiny'):
        assert not res.npix[R[row]].any() and not res.sum[R[row]].any()
    assert np.array_equal(np.isnan(res.mean), res.npix == 0)
    ok = ~pairs['bad']
    assert np.allclose(res.R_q, pairs['R_q'], rtol=1e-13) and np.allclose(res.R[ok], pairs['R'][ok], rtol=1e-13) and np.all(np.isnan(res.R[~ok]))
    again = runner.process(map=Map.map.copy())                        # the counts are exact and reproducible
    assert np.array_equal(again.npix, res.npix)
    st = res.stack()
    has = res.npix.sum(0) > 0                                         # (no pixel centre lies within 0.02 R_com of a halo)
    assert np.count_nonzero(has) >= 12 and np.all(st['density'][has] > 0) and np.all(np.isnan(st['density'][~has]))
    assert np.allclose(st['density'][has], st['mean'][has] / res.res ** ndim)


def _small_case(ndim, N, L, M, hpos, eps, seed, edges, scaled=False, m=None, label=''):
    import baryonification_amd as bfg
    rng = np.random.default_rng(seed)
    bins = _bins(N, L)
    hpos = np.atleast_2d(np.asarray(hpos, dtype=np.float64))
    cat = {'M': np.asarray(M, dtype=np.float64), 'x': hpos[:, 0], 'y': hpos[:, 1], 'z': hpos[:, 2]}
    if m is None:
        m = rng.uniform(0.5, 2.0, (N,) * ndim)
    HCat, Map = _objects(cat, m, bins, ndim)
    pairs = K.pairs(bins, ndim, _used(HCat), ZR, eps, _background())
    o = K.measure(pairs, edges, m, scaled)
    res = bfg.Runners.MeasureProfilesGrid(HCat, Map, eps, verbose=False, r_edges=edges, scaled=scaled).process()
    _compare(res, o, label, max_share=0.0)
    return res, o, pairs


@pytest.mark.parametrize('N', [8, 9, 10])
@pytest.mark.parametrize('ndim', [2, 3])
def test_an_axis_covered_completely_is_visited_exactly_once(gpu, ndim, N):
    """a clipped ball (R_q = max(bins) / 2) and a ball of 3.2 pixels in a box of 8, 9 and 10: 2 w + 1 is 9, so the visited range is the
    whole axis for N = 8 and 9 and a window that wraps for N = 10; a pixel visited twice would be counted twice"""
    rng = np.random.default_rng(800 + 10 * ndim + N)
    L, eps = 2.5 * N, 5.0
    hpos = rng.uniform(0, L, (4, 3))
    hpos[2] = [0.1, L - 0.2, 0.3]
    M = [3e17, _mass_for_ball(3.2 * 2.5, eps), 3e17, _mass_for_ball(3.2 * 2.5, eps)]
    edges = np.array([0.0, 2.0, 4.5, 7.0, 9.5, 20.0])
    res, o, pairs = _small_case(ndim, N, L, M, hpos, eps, 810 + N, edges, label='whole axis %d-D N = %d' % (ndim, N))
    assert pairs['R_q'][0] == pairs['R_q'][2] == np.max(_bins(N, L)) / 2 and 3.1 * 2.5 < pairs['R_q'][1] < 3.3 * 2.5
    inside = np.bincount(pairs['halo'][pairs['inside']], minlength=4)
    assert np.array_equal(res.npix.sum(1), inside) and np.array_equal(res.npix.sum(1), o['npix'].sum(1))
    assert inside[0] > 0.5 * N ** ndim * (np.pi / 6 if ndim == 3 else np.pi / 4) and np.all(inside <= N ** ndim)


@pytest.mark.parametrize('ndim', [2, 3])
def test_a_one_pixel_ball_in_the_corner_pixel_wraps_on_every_axis(gpu, ndim):
    N, L, eps = 16, 40.0, 5.0
    res_ = L / N
    hpos = np.array([[0.31 * res_, 0.43 * res_, 0.17 * res_], [L - 0.29 * res_, L - 0.13 * res_, L - 0.41 * res_]])
    M = [_mass_for_ball(1.3 * res_, eps)] * 2
    edges = np.array([0.0, 0.5 * res_, 1.0 * res_, 2.0 * res_])
    res, o, pairs = _small_case(ndim, N, L, M, hpos, eps, 820 + ndim, edges, label='corner pixel %d-D' % ndim)
    for j in (0, 1):                                                  # the ball holds pixels 0 and N - 1 of every axis
        pix = pairs['pix'][pairs['inside'] & (pairs['halo'] == j)]
        idx = np.stack(np.unravel_index(pix, (N,) * ndim), axis=1)
        assert all(0 in idx[:, k] and N - 1 in idx[:, k] for k in range(ndim)), j
        assert res.npix[j].sum() == pix.size >= 2 * ndim + 1


@pytest.mark.parametrize('nb', [1, 64])
def test_one_bin_and_sixty_four_bins(gpu, nb):
    rng = np.random.default_rng(830 + nb)
    N, L, eps, nh = 32, 64.0, 5.0, 20
    M = 10 ** rng.uniform(13.0, 15.0, nh)
    hpos = rng.uniform(0, L, (nh, 3))
    edges = np.array([0.0, 40.0]) if nb == 1 else np.linspace(0.05, 12.0, 65)
    for ndim in (2, 3):
        res, o, pairs = _small_case(ndim, N, L, M, hpos, eps, 840, edges, label='%d bins %d-D' % (nb, ndim))
        assert res.npix.shape == (nh, nb) and res.npix.sum() > 100
        if nb == 1:
            assert np.array_equal(res.npix[:, 0], np.bincount(pairs['halo'][pairs['inside']], minlength=nh))


def test_no_halo_and_invalid_halos_only(gpu):
    import baryonification_amd as bfg
    rng = np.random.default_rng(850)
    N, L = 16, 40.0
    for ndim in (2, 3):
        m = rng.uniform(0.5, 2.0, (N,) * ndim)
        none = {k: np.zeros(0) for k in ('M', 'x', 'y', 'z')}
        HCat, Map = _objects(none, m, _bins(N, L), ndim)
        res = bfg.Runners.MeasureProfilesGrid(HCat, Map, 5.0, verbose=False, r_edges=[0.0, 1.0, 2.0, 5.0]).process()
        assert res.npix.shape == (0, 3) and res.sum.shape == (0, 3) and res.npix.dtype == np.int64 and res.R.shape == (0,)
        assert res.mean.shape == (0, 3) and np.all(np.isnan(res.stack()['mean']))
        inv = {'M': np.array([-1e14, 0.0, np.nan, np.inf, 1e14, 1e14]), 'x': np.array([1.0, 2.0, 3.0, 4.0, np.nan, 5.0]),
               'y': np.array([1.0, 2.0, 3.0, 4.0, 5.0, np.inf]), 'z': np.full(6, 7.0)}
        HCat, Map = _objects(inv, m, _bins(N, L), ndim)
        res = bfg.Runners.MeasureProfilesGrid(HCat, Map, 5.0, verbose=False, r_edges=[0.0, 1.0, 2.0, 5.0]).process()
        assert res.npix.shape == (6, 3) and not res.npix.any() and np.all(res.sum == 0.0)
        assert np.all(np.isnan(res.R)) and np.all(res.R_q == 0) and np.all(np.isnan(res.mean))


@pytest.mark.parametrize('ndim', [2, 3])
def test_constant_map(gpu, ndim):
    rng = np.random.default_rng(860 + ndim)
    N, L, eps, nh, value = 40, 60.0, 5.0, 30, 3.7
    M = 10 ** rng.uniform(13.0, 15.3, nh)
    hpos = rng.uniform(0, L, (nh, 3))
    edges = np.concatenate([[0.0], np.geomspace(0.4, 15.0, 12)])
    res, o, pairs = _small_case(ndim, N, L, M, hpos, eps, 0, edges, m=np.full((N,) * ndim, value), label='constant map %d-D' % ndim)
    assert res.npix.sum() > 1000
    assert np.all(np.abs(res.sum - value * res.npix) <= 2 * res.npix * EPS * value * res.npix)
    assert np.allclose(res.mean[res.npix > 0], value, rtol=1e-13)


def _tangential_field(bins, h, profile):
    """(g1, g2) of a purely tangential field gamma(d) about h: g1 + i g2 = -gamma e^{2 i phi}"""
    L = bins.size * (bins[1] - bins[0])
    Dx, Dy = np.meshgrid(K.min_image(bins - h[0], L), K.min_image(bins - h[1], L), indexing='ij')
    d2 = Dx * Dx + Dy * Dy
    gam = profile(np.sqrt(d2))
    with np.errstate(divide='ignore', invalid='ignore'):
        c2, s2 = np.where(d2 > 0, (Dx * Dx - Dy * Dy) / d2, 0.0), np.where(d2 > 0, 2 * Dx * Dy / d2, 0.0)
    return -gam * c2, -gam * s2


def test_shear_of_an_analytic_tangential_field(gpu):
    """gamma(d) = 1 / (1 + d) about the halo, tangential: mean_x is 0 to the bound, mean_t is the oracle's and lies between the profile's
    values at the bin's edges; the halo sits where its ball wraps around both axes"""
    import baryonification_amd as bfg
    N, L, eps = 64, 96.0, 5.0
    bins = _bins(N, L)
    cat = {'M': np.array([1e15]), 'x': np.array([2.2]), 'y': np.array([L - 3.1]), 'z': np.zeros(1)}
    rng = np.random.default_rng(870)
    m = rng.uniform(0.5, 2.0, (N, N))
    HCat, Map = _objects(cat, m, bins, 2)
    h = np.array([HCat.cat['x'][0], HCat.cat['y'][0]], dtype=np.float64)
    g1, g2 = _tangential_field(bins, h, lambda d: 1.0 / (1.0 + d))
    edges = np.concatenate([[0.0], np.geomspace(0.8, 11.0, 12)])
    pairs = K.pairs(bins, 2, _used(HCat), ZR, eps, _background())
    assert pairs['R_q'][0] > edges[-1]
    o = K.measure(pairs, edges, m, shear=(g1, g2))
    runner = bfg.Runners.MeasureProfilesGrid(HCat, Map, eps, verbose=False, r_edges=edges, shear=(g1, g2))
    res = runner.process()
    _compare(res, o, 'tangential field', max_share=0.0)
    assert np.count_nonzero(res.npix_shear[0]) >= 9 and np.array_equal(res.npix_shear, res.npix)
    assert np.all(np.abs(res.sum_x) <= (2 * o['npix_shear'] + 16) * EPS * o['S_shear'])          # within the bound of 0
    lo, hi = 1.0 / (1.0 + edges[1:]), 1.0 / (1.0 + edges[:-1])
    has = res.npix_shear[0] > 0
    assert np.all(res.mean_t[0][has] > lo[has] * (1 - 1e-12)) and np.all(res.mean_t[0][has] <= hi[has] * (1 + 1e-12))
    flipped = runner.process(shear=(-g1, -g2))                        # a radial field: gamma_t < 0
    assert np.all(flipped.mean_t[0][has] < 0) and np.array_equal(flipped.npix_shear, res.npix_shear)


def test_shear_of_random_fields(gpu):
    """50 halos, random g1 and g2 with NaN pixels; halo 3 sits exactly on a pixel centre (res = 2: the bins are odd integers, exact in
    float32), so the d = 0 pixel is alone in bin [0, 0.3): it counts for the map and has no position angle"""
    import baryonification_amd as bfg
    rng = np.random.default_rng(880)
    N, L, eps, nh = 96, 192.0, 5.0, 50
    bins = _bins(N, L)
    M = (10 ** rng.uniform(13.0, 15.2, nh)).astype(np.float32).astype(np.float64)
    hpos = rng.uniform(0, L, (nh, 3)).astype(np.float32).astype(np.float64)
    hpos[3, :2] = [bins[10], bins[N - 1]]
    M[3] = np.float64(np.float32(5e14))
    M[6] = -1.0
    m, g1, g2 = rng.uniform(0.5, 2.0, (N, N)), rng.normal(size=(N, N)), rng.normal(size=(N, N))
    for k, f in enumerate((m, g1, g2)):
        f.flat[rng.choice(N * N, 40, replace=False)] = np.nan
    m[10, N - 1], g1[10, N - 1], g2[10, N - 1] = 1.5, 0.25, -0.5        # the centred halo's own pixel is finite
    cat = {'M': M, 'x': hpos[:, 0], 'y': hpos[:, 1], 'z': hpos[:, 2]}
    HCat, Map = _objects(cat, m, bins, 2)
    assert HCat.cat['x'][3] == bins[10] and HCat.cat['y'][3] == bins[N - 1]
    edges = np.concatenate([[0.0], np.geomspace(0.3, 14.0, 24)])
    pairs = K.pairs(bins, 2, _used(HCat), ZR, eps, _background())
    o = K.measure(pairs, edges, m, shear=(g1, g2))
    assert o['npix'][3, 0] == 1 and o['npix_shear'][3, 0] == 0 and np.any(o['npix_shear'] < o['npix']) and np.any(o['npix_shear'] > o['npix'])
    for scaled, e in ((False, edges), (True, np.geomspace(0.02, 5.0, 25))):
        oo = o if not scaled else K.measure(pairs, e, m, True, shear=(g1, g2))
        res = bfg.Runners.MeasureProfilesGrid(HCat, Map, eps, verbose=False, r_edges=e, scaled=scaled).process(shear=(g1, g2))
        _compare(res, oo, 'random shear scaled %s' % scaled)
        assert not res.npix_shear[6].any() and not res.sum_t[6].any() and np.all(np.isfinite(res.sum_t)) and np.all(np.isfinite(res.sum_x))
        assert np.array_equal(np.isnan(res.mean_t), res.npix_shear == 0)
        if not scaled:
            assert res.npix[3, 0] == 1 and res.sum[3, 0] == 1.5 and res.npix_shear[3, 0] == 0 and res.sum_t[3, 0] == 0.0 and res.sum_x[3, 0] == 0.0
    st = res.stack()
    assert set(st) == {'mean', 'density', 'mean_t', 'mean_x'} and np.array_equal(np.isnan(st['mean_t']), res.npix_shear.sum(0) == 0)


def test_device_entry(gpu):
    import torch
    import baryonification_amd as bfg
    from baryonification_amd import _lib
    from baryonification_amd.Runners._model import _placeholder_model
    dev = torch.device('cuda', 0)
    T = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)                       # noqa: E731
    for ndim in (3, 2):
        rng = np.random.default_rng(890 + ndim)
        N, L, eps, nh, nb = (40, 60.0, 5.0, 120, 12) if ndim == 3 else (96, 150.0, 5.0, 120, 12)
        bins = _bins(N, L)
        M = (10 ** rng.uniform(13.0, 15.0, nh)).astype(np.float32).astype(np.float64)
        hpos = rng.uniform(0, L, (nh, 3)).astype(np.float32).astype(np.float64)
        M[4] = -1.0
        m = rng.uniform(0.5, 2.0, (N,) * ndim)
        pair = (rng.uniform(0.1, 1.0, (N, N)), rng.uniform(0.1, 1.0, (N, N))) if ndim == 2 else None
        cat = {'M': M, 'x': hpos[:, 0], 'y': hpos[:, 1], 'z': hpos[:, 2]}
        HCat, Map = _objects(cat, m, bins, ndim)
        edges = np.concatenate([[0.0], np.geomspace(0.5, 12.0, nb)])
        runner = bfg.Runners.MeasureProfilesGrid(HCat, Map, eps, verbose=False, r_edges=edges, shear=pair)
        host = runner.process()
        assert host.npix.sum() > 5_000 and not host.npix[4].any()
        tm, tpair = T(m), None if pair is None else (T(pair[0]), T(pair[1]))
        ondev = runner.process(map=tm, shear=tpair)
        names = ('npix', 'sum', 'mean', 'density', 'enclosed') + (('npix_shear', 'sum_t', 'sum_x', 'mean_t', 'mean_x') if pair else ())
        for name in names:
            assert getattr(ondev, name).is_cuda and getattr(ondev, name).shape == (nh, nb), name
        # the same pixels in the same cells; the sums within two fp64 summations in any order (every value > 0: S = sum)
        assert np.array_equal(_get(ondev.npix), host.npix)
        assert np.all(np.abs(_get(ondev.sum) - host.sum) <= 2 * host.npix * EPS * host.sum)
        if pair:
            assert np.array_equal(_get(ondev.npix_shear), host.npix_shear)
            S = 2.0 * host.npix_shear                                                     # |g1| + |g2| <= 2 per pixel
            assert np.all(np.abs(_get(ondev.sum_t) - host.sum_t) <= (2 * host.npix_shear + 16) * EPS * S)
            assert np.all(np.abs(_get(ondev.sum_x) - host.sum_x) <= (2 * host.npix_shear + 16) * EPS * S)
        st = ondev.stack(select=torch.arange(100, device=dev))
        assert st['mean'].is_cuda and np.allclose(_get(st['mean']), host.stack(select=np.arange(100))['mean'], rtol=1e-12, equal_nan=True)
        # numpy and tensors do not mix; a tensor must be C-contiguous, float64 and of the map's shape
        if pair:
            with pytest.raises(ValueError, match='all be numpy arrays or all CUDA tensors'):
                runner.process(map=tm)                                                    # (the constructor's pair is numpy)
            with pytest.raises(ValueError, match='all be numpy arrays or all CUDA tensors'):
                runner.process(map=m, shear=tpair)
        plain = bfg.Runners.MeasureProfilesGrid(HCat, Map, eps, verbose=False, r_edges=edges)
        for bad in (tm.float(), tm.transpose(0, 1), tm.reshape(-1)):
            with pytest.raises(ValueError, match='C-contiguous float64'):
                plain.process(map=bad)
        # at C level: outputs pre-filled with -1 / NaN are overwritten in every cell, also in the invalid halo's row; without halos nothing is written
        lib = _lib.load()
        model, keep = _placeholder_model(runner, runner._runner_cosmo())
        hc = HCat.cat
        c, ckeep = _lib.make_grid_catalog_host(hc['M'], hc['x'], hc['y'], hc['z'])
        grid, gkeep = _lib.make_grid(bins, ndim, ZR)
        P = lambda t: None if t is None else C.c_void_p(t.data_ptr())                   # noqa: E731
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream or None)
        outs = [torch.full((nh, nb), -1, dtype=torch.int64, device=dev), torch.full((nh, nb), float('nan'), dtype=torch.float64, device=dev)]
        if pair:
            outs += [torch.full((nh, nb), -1, dtype=torch.int64, device=dev)] + [torch.full((nh, nb), float('nan'), dtype=torch.float64, device=dev) for _ in (0, 1)]
        optr = [P(t) for t in outs] + [None] * (5 - len(outs))

        def call(cat_):
            _lib.check(lib.bfgx_grid_profiles_device(0, stream, C.byref(cat_), C.byref(model), C.byref(grid), P(tm), P(tpair[0]) if pair else None,
                                                     P(tpair[1]) if pair else None, nb, edges.ctypes.data, 0, *optr))
            torch.cuda.synchronize()

        call(c)
        assert np.array_equal(_get(outs[0]), host.npix) and all(bool(torch.isfinite(t).all()) for t in outs[1::2] + outs[4:])
        assert bool((outs[0][4] == 0).all()) and bool((outs[1][4] == 0).all())
        for t in outs:
            t.fill_(-1 if t.dtype == torch.int64 else float('nan'))
        none, nkeep = _lib.make_grid_catalog_host(np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0))
        call(none)                                                    # n_halo = 0: there is no cell
        assert bool((outs[0] == -1).all()) and bool(torch.isnan(outs[1]).all())
        del keep, ckeep, gkeep, nkeep


def test_baryonify_grid_before_and_after(gpu):
    """BaryonifyGrid on a 64^3 synthetic mass map with a closed-form table: one runner measures the map and the displaced map, both equal
    the oracle on their map; the stacked density ratio is printed, not asserted"""
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    rng = np.random.default_rng(900)
    N, L, eps, nh = 64, 128.0, 5.0, 60
    bins = _bins(N, L)
    M = (10 ** rng.uniform(13.3, 15.0, nh)).astype(np.float32).astype(np.float64)
    hpos = rng.uniform(0, L, (nh, 3)).astype(np.float32).astype(np.float64)
    before = rng.poisson(4.0, (N, N, N)).astype(np.float64)
    cat = {'M': M, 'x': hpos[:, 0], 'y': hpos[:, 1], 'z': hpos[:, 2]}
    HCat, Map = _objects(cat, before, bins, 3)
    z, Mt, r = np.linspace(ZR - 0.05, ZR + 0.05, 3), np.geomspace(10 ** 13.2, 10 ** 15.1, 6), np.geomspace(1e-3, 2e2, 200)
    model = bfg.Profiles.Baryonification2D(None, None, bfg.utils.Cosmology.from_dict(syn.COSMO), epsilon_max=eps)
    model.set_table(z, Mt, r, syn.displacement_table(z, Mt, r))
    after = bfg.Runners.BaryonifyGrid(HCat, Map, eps, model, verbose=False).process()
    assert after.shape == before.shape and np.any(after != before) and np.isclose(after.sum(), before.sum(), rtol=1e-9)
    edges = np.concatenate([[0.0], np.geomspace(1.0, 12.0, 10)])
    m = bfg.Runners.MeasureProfilesGrid(HCat, Map, eps, verbose=False, r_edges=edges)
    pairs = K.pairs(bins, 3, _used(HCat), ZR, eps, _background())
    p0, p1 = m.process(), m.process(map=after)
    _compare(p0, K.measure(pairs, edges, before), 'before BaryonifyGrid')
    _compare(p1, K.measure(pairs, edges, after), 'after BaryonifyGrid')
    assert np.array_equal(p0.npix, p1.npix) and np.any(p0.sum != p1.sum)
    print('stacked density after / before:', p1.stack()['density'] / p0.stack()['density'])
