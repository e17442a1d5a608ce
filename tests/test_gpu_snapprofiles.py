"""GPU checks of bfg.Runners.MeasureProfilesSnapshot (csrc/bfgx_snapshot_stack.hpp): parity with the brute-force numpy oracle
(snapprofiles_oracle.py), exact bin edges and the periodic wrap, the clipped ball of a small box, one dense halo, the per-halo counts of the
reference-pinned pair entry, host entry == device entry, and the definition of baryonification measured end to end.

Bounds (derived, not measured).  Per (halo, bin) cell without an ambiguous particle: npart equal;
    |sum - sum_o| <= 2 npart eps S,  S = sum |w| over the cell, eps = 2.2e-16  (two fp64 summations of npart terms in any order).
Cells with ambiguous particles (within 1e-9 R_q of the rim of the ball; in scaled mode within 1e-9 edge of a bin edge) get the same bounds
widened by those particles' count and sum |w|; their share of all cells is asserted <= 1e-3."""
import ctypes as C
import functools

import numpy as np
import pytest

import snapprofiles_oracle as K

pytestmark = pytest.mark.gpu

EPS = 2.2e-16


def _objects(cat, part, L, zr, ndim, mass=None):
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    HCat = bfg.utils.HaloNDCatalog(x=cat['x'], y=cat['y'], z=cat['z'] if ndim == 3 else None, M=cat['M'], redshift=zr, cosmo=dict(syn.COSMO))
    Snap = bfg.utils.ParticleSnapshot(x=part[:, 0], y=part[:, 1], z=part[:, 2] if ndim == 3 else None,
                                      M=np.ones(part.shape[0]) if mass is None else mass, L=L, redshift=zr, cosmo=dict(syn.COSMO))
    return HCat, Snap


def _used(HCat):
    return {k: np.array(HCat.cat[k], dtype=np.float64) for k in ('M', 'x', 'y', 'z')}


def _background():
    from baryonification_amd import synthetic as syn
    from oracle import grid as G
    return G.grid_background(syn.COSMO)


def _compare(res, o, label):
    """asserts the bounds of the module docstring; returns and prints the ambiguous share and the largest error / bound ratio"""
    get = lambda v: v.cpu().numpy() if hasattr(v, 'cpu') else np.asarray(v)               # noqa: E731
    amb = o['amb_n'] > 0
    share = float(amb.mean()) if amb.size else 0.0
    npart = get(res.npart)
    assert npart.dtype == np.int64 and npart.shape == o['npart'].shape, label
    stats = {'ambiguous_cell_share': share, 'cells': int(amb.size), 'pairs': o['pairs'], 'ambiguous_particles': o['amb_particles'],
             'halos_without_a_particle': int(np.count_nonzero(o['npart'].sum(1) == 0))}
    if res.sum is not None:
        s = get(res.sum)
        assert s.dtype == np.float64 and s.shape == o['sum'].shape, label
        bound = 2 * o['npart'] * EPS * o['S'] + o['amb_abs']
        err = np.abs(s - o['sum'])
        with np.errstate(divide='ignore', invalid='ignore'):
            stats['sum'] = float(np.max(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)), initial=0.0))
    print('%s: %s' % (label, stats))
    assert share <= 1e-3, stats
    assert np.array_equal(npart[~amb], o['npart'][~amb]) and np.all(np.abs(npart - o['npart']) <= o['amb_n']), (label, stats)
    if res.sum is not None:
        assert np.all(err <= bound), (label, stats)
    return stats


PARITY_EDGES = {False: np.concatenate([[0.0], np.geomspace(0.05, 12.0, 16)]), True: np.geomspace(0.02, 5.0, 17)}
PARITY_ROWS = {'negative': 7, 'zero': 8, 'tiny': 9, 'origin': 10, 'corner': 11}


@functools.lru_cache(maxsize=None)
def _parity_case(ndim):
    """the inputs of the parity test and the oracle's pairs, once per ndim (the 3-D case also serves the pair-entry test)"""
    rng = np.random.default_rng(70 + ndim)
    L, nh, npart, zr, eps = 300.0, 600, 200_000, 0.2, 5.0
    M = (10 ** rng.uniform(12.8, 15.0, nh)).astype(np.float32).astype(np.float64)
    hpos = rng.uniform(0, L, (nh, 3)).astype(np.float32).astype(np.float64)
    part = rng.uniform(0, L, (npart, 3))
    part[:40_000] = (hpos[rng.integers(0, nh, 40_000)] + rng.normal(scale=1.0, size=(40_000, 3))) % L    # clustered around halos
    w = rng.uniform(0.5, 2.0, npart)
    w[rng.choice(npart, 10, replace=False)] = np.nan
    R = PARITY_ROWS
    M[R['negative']], M[R['zero']], M[R['tiny']] = -3e13, 0.0, 1e8                        # not halos; a ball with no particle in it
    M[R['origin']] = M[R['corner']] = np.float64(np.float32(1e15))                         # (balls that reach through every face of the box)
    hpos[R['origin']] = 0.0
    hpos[R['corner']] = np.float32(L)                                                       # the float32 value nearest (L, L, L)
    cat = {'M': M, 'x': hpos[:, 0], 'y': hpos[:, 1], 'z': hpos[:, 2]}
    HCat, Snap = _objects(cat, part[:, :ndim], L, zr, ndim, mass=w)
    pairs = K.pairs(part[:, :ndim], L, _used(HCat), zr, eps, _background())
    return HCat, Snap, w, eps, pairs


@pytest.mark.parametrize('scaled', [False, True])
@pytest.mark.parametrize('ndim', [2, 3])
def test_parity_with_the_oracle(gpu, ndim, scaled):
    import baryonification_amd as bfg
    HCat, Snap, w, eps, pairs = _parity_case(ndim)
    edges = PARITY_EDGES[scaled]
    o = K.measure(pairs, edges, w, scaled)
    R = PARITY_ROWS
    assert o['npart'][R['origin']].sum() > 0 and o['npart'][R['corner']].sum() > 0 and o['npart'].sum() > 0.5 * o['pairs']
    for row in (R['negative'], R['zero'], R['tiny']):
        assert not o['npart'][row].any()
    runner = bfg.Runners.MeasureProfilesSnapshot(HCat, Snap, eps, verbose=False, r_edges=edges, scaled=scaled)
    res = runner.process()                                            # the snapshot's own particles, weights = its 'M' column
    assert isinstance(res.npart, np.ndarray) and res.npart.shape == (600, 16) and res.ndim == ndim and res.scaled == scaled
    _compare(res, o, 'parity %d-D scaled %s' % (ndim, scaled))
    for row in (R['negative'], R['zero'], R['tiny']):
        assert not res.npart[row].any() and not res.sum[row].any()
    assert np.array_equal(np.isnan(res.mean), res.npart == 0) and np.all(np.isfinite(res.sum))
    assert np.allclose(res.R_q, pairs['R_q'], rtol=1e-13) and np.allclose(res.R[~pairs['bad']], pairs['R'][~pairs['bad']], rtol=1e-13)
    # the same particles handed over as a catalog, explicit weights, and counts only: the counts are exact and reproducible
    again = runner.process(cat=Snap.cat, weights=w)
    assert np.array_equal(again.npart, res.npart)
    assert np.all(np.abs(again.sum - res.sum) <= 2 * res.npart * EPS * 2.0 * res.npart)    # (|w| <= 2)
    counts = runner.process(weights=False)
    assert counts.sum is None and np.array_equal(counts.npart, res.npart)
    st = res.stack()
    assert np.all(np.isfinite(st['density'])) and np.all(st['density'] >= 0) and np.count_nonzero(st['density']) >= 12


@pytest.mark.parametrize('ndim', [2, 3])
def test_exact_edges_and_the_periodic_wrap(gpu, ndim):
    """L = 256: every difference and +-L is exact, so are d = 0, 5, 5 (through the wrap) and 10; a particle ON an edge belongs to the bin
    that starts there, and one on the last edge to no bin although it is inside the ball"""
    import baryonification_amd as bfg
    L = 256.0
    cat = {'M': np.array([1e15]), 'x': np.array([1.0]), 'y': np.array([1.0]), 'z': np.array([1.0])}
    part = np.array([[1.0, 1.0, 1.0], [4.0, 5.0, 1.0], [L - 2.0, L - 3.0, 1.0], [7.0, 9.0, 1.0]])
    wts = np.array([1.0, 2.0, 4.0, 8.0])
    HCat, Snap = _objects(cat, part[:, :ndim], L, 0.0, ndim, mass=wts)
    runner = bfg.Runners.MeasureProfilesSnapshot(HCat, Snap, 8.0, verbose=False, r_edges=[0.0, 5.0, 10.0])
    R, R_q = runner.radii()
    assert 10.0 < R_q[0] < L / 2
    res = runner.process()
    assert res.npart.tolist() == [[1, 2]] and res.sum.tolist() == [[1.0, 6.0]]
    wide = bfg.Runners.MeasureProfilesSnapshot(HCat, Snap, 8.0, verbose=False, r_edges=[0.0, 5.0, 10.0, 11.0]).process()
    assert wide.npart.tolist() == [[1, 2, 1]] and wide.sum.tolist() == [[1.0, 6.0, 8.0]]


@pytest.mark.parametrize('ndim', [2, 3])
def test_clipped_ball_in_a_small_box(gpu, ndim):
    """L = 20 and epsilon_max R_com > L / 2 for every halo: R_q = L / 2 and the cube of cells is the whole axis"""
    import baryonification_amd as bfg
    rng = np.random.default_rng(300 + ndim)
    L, nh, npart, zr, eps = 20.0, 50, 20_000, 0.2, 20.0
    M = (10 ** rng.uniform(14.0, 15.0, nh)).astype(np.float32).astype(np.float64)
    hpos = rng.uniform(0, L, (nh, 3)).astype(np.float32).astype(np.float64)
    part = rng.uniform(0, L, (npart, 3))
    w = rng.uniform(0.5, 2.0, npart)
    cat = {'M': M, 'x': hpos[:, 0], 'y': hpos[:, 1], 'z': hpos[:, 2]}
    HCat, Snap = _objects(cat, part[:, :ndim], L, zr, ndim, mass=w)
    pairs = K.pairs(part[:, :ndim], L, _used(HCat), zr, eps, _background())
    assert np.all(pairs['R_q'] == L / 2) and np.all(eps * pairs['R'] > L / 2)
    for scaled, edges in ((False, np.concatenate([[0.0], np.geomspace(0.1, 10.5, 13)])), (True, np.geomspace(0.05, 12.0, 14))):
        runner = bfg.Runners.MeasureProfilesSnapshot(HCat, Snap, eps, verbose=False, r_edges=edges, scaled=scaled)
        assert np.all(runner.radii()[1] == L / 2)
        o = K.measure(pairs, edges, w, scaled)
        assert o['pairs'] > 0.4 * nh * npart * (np.pi / 6 if ndim == 3 else np.pi / 4)
        _compare(runner.process(), o, 'clipped ball %d-D scaled %s' % (ndim, scaled))


def test_dense_halo(gpu):
    """one halo with ~2e5 particles in its ball and ~1e5 in one bin: long runs, many rounds, every lane adding to the same LDS bin"""
    import baryonification_amd as bfg
    rng = np.random.default_rng(404)
    L, zr, eps = 300.0, 0.2, 5.0
    h = np.array([0.5, 0.5, L - 0.5])
    part = np.concatenate([(h + rng.normal(scale=2.0, size=(150_000, 3))) % L, rng.uniform(0, L, (50_000, 3))])
    w = rng.uniform(0.5, 2.0, part.shape[0])
    cat = {'M': np.array([1e15]), 'x': h[:1], 'y': h[1:2], 'z': h[2:]}
    HCat, Snap = _objects(cat, part, L, zr, 3, mass=w)
    edges = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 6.0, 7.0, 8.0, 10.0])
    pairs = K.pairs(part, L, _used(HCat), zr, eps, _background())
    assert pairs['R_q'][0] > 8.0
    o = K.measure(pairs, edges, w)
    assert o['npart'].max() > 100_000 and o['pairs'] > 140_000
    res = bfg.Runners.MeasureProfilesSnapshot(HCat, Snap, eps, verbose=False, r_edges=edges).process()
    _compare(res, o, 'dense halo')
    o = K.measure(pairs, edges / 2.0, w, scaled=True)
    _compare(bfg.Runners.MeasureProfilesSnapshot(HCat, Snap, eps, verbose=False, r_edges=edges / 2.0, scaled=True).process(), o, 'dense halo, scaled')


class _CountingModel(object):
    """a plain callable on the exact per-halo route: records how many particles each halo is called with, moves none"""
    bfgx_exact = True

    def __init__(self):
        self.counts = []

    def displacement(self, r, M, a):
        self.counts.append(len(r))
        return np.zeros(len(r))


def test_counts_equal_the_reference_pinned_pair_entry(gpu):
    import baryonification_amd as bfg
    HCat, Snap, w, eps, pairs = _parity_case(3)
    model = _CountingModel()
    bfg.Runners.BaryonifySnapshot(HCat, Snap, eps, model, verbose=False).process()
    counts = np.array(model.counts, dtype=np.int64)
    assert counts.size == 600 and counts.sum() > 10_000
    res = bfg.Runners.MeasureProfilesSnapshot(HCat, Snap, eps, verbose=False, r_edges=[0.0, Snap.L]).process(weights=False)
    assert res.npart.shape == (600, 1) and np.array_equal(res.npart[:, 0], counts)


def test_device_entry(gpu):
    import torch
    import baryonification_amd as bfg
    from baryonification_amd import _lib
    from baryonification_amd.Runners._model import _placeholder_model
    rng = np.random.default_rng(606)
    L, nh, npart, zr, eps, nb = 100.0, 300, 50_000, 0.2, 5.0, 12
    M = (10 ** rng.uniform(13.0, 15.0, nh)).astype(np.float32).astype(np.float64)
    hpos = rng.uniform(0, L, (nh, 3)).astype(np.float32).astype(np.float64)
    part = rng.uniform(0, L, (npart, 3))
    w = rng.uniform(0.5, 2.0, npart)
    M[4] = -1.0
    cat = {'M': M, 'x': hpos[:, 0], 'y': hpos[:, 1], 'z': hpos[:, 2]}
    HCat, Snap = _objects(cat, part, L, zr, 3, mass=w)
    edges = np.concatenate([[0.0], np.geomspace(0.1, 12.0, nb)])
    runner = bfg.Runners.MeasureProfilesSnapshot(HCat, Snap, eps, verbose=False, r_edges=edges)
    host = runner.process()
    assert host.npart.sum() > 10_000 and not host.npart[4].any()
    dev = torch.device('cuda', 0)
    tx, ty, tz, tw = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (part[:, 0], part[:, 1], part[:, 2], w))
    ondev = runner.process(cat=(tx, ty, tz), weights=tw)
    for name in ('npart', 'sum', 'mean', 'density', 'enclosed', 'volume'):
        assert getattr(ondev, name).is_cuda and getattr(ondev, name).shape == (nh, nb), name
    # the same particles in the same cells; the sums within two fp64 summations in any order (w > 0: S = sum)
    assert np.array_equal(ondev.npart.cpu().numpy(), host.npart)
    assert np.all(np.abs(ondev.sum.cpu().numpy() - host.sum) <= 2 * host.npart * EPS * host.sum)
    counts = runner.process(cat=(tx, ty, tz))                         # device tensors without weights: counts only
    assert counts.sum is None and counts.npart.is_cuda and np.array_equal(counts.npart.cpu().numpy(), host.npart)
    st = ondev.stack(select=torch.arange(100, device=dev))
    assert st['mean'].is_cuda and np.allclose(st['mean'].cpu().numpy(), host.stack(select=np.arange(100))['mean'], rtol=1e-12, equal_nan=True)
    assert np.allclose(st['density'].cpu().numpy(), host.stack(select=np.arange(100))['density'], rtol=1e-12, equal_nan=True)
    # at C level: outputs pre-filled with -1 / NaN are overwritten in every cell, also without particles; without halos nothing is written
    lib = _lib.load()
    model, keep = _placeholder_model(runner, runner._cosmo_dict())
    hc = HCat.cat
    c, ckeep = _lib.make_grid_catalog_host(hc['M'], hc['x'], hc['y'], hc['z'])
    P = lambda t: C.c_void_p(t.data_ptr())                            # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream or None)

    def call(cat_, n_part, out_n, out_s):
        _lib.check(lib.bfgx_snapshot_profiles_device(0, stream, C.byref(cat_), C.byref(model), 3, L, zr, n_part, P(tx), P(ty), P(tz), P(tw), nb,
                                                     edges.ctypes.data, 0, P(out_n), P(out_s)))
        torch.cuda.synchronize()

    out_n = torch.full((nh, nb), -1, dtype=torch.int64, device=dev)
    out_s = torch.full((nh, nb), float('nan'), dtype=torch.float64, device=dev)
    call(c, npart, out_n, out_s)
    assert np.array_equal(out_n.cpu().numpy(), host.npart) and bool(torch.isfinite(out_s).all())
    assert np.all(np.abs(out_s.cpu().numpy() - host.sum) <= 2 * host.npart * EPS * host.sum)
    out_n.fill_(-1); out_s.fill_(float('nan'))
    call(c, 0, out_n, out_s)                                          # n_part = 0
    assert bool((out_n == 0).all()) and bool((out_s == 0).all())
    out_n.fill_(-1); out_s.fill_(float('nan'))
    none, nkeep = _lib.make_grid_catalog_host(np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0))
    call(none, npart, out_n, out_s)                                   # n_halo = 0: there is no cell
    assert bool((out_n == -1).all()) and bool(torch.isnan(out_s).all())
    # particles outside [0, L] are refused, as by the pair entry
    tx[17] = -1.0
    with pytest.raises(ValueError, match=r'\[0, L\]'):
        runner.process(cat=(tx, ty, tz))
    bad = Snap.cat.copy()
    bad['y'][3] = np.nan
    with pytest.raises(ValueError, match=r'\[0, L\]'):
        runner.process(cat=bad)
    del keep, ckeep, nkeep


def test_baryonification_moves_enclosed_mass_as_defined(gpu):
    """The enclosed mass of the dark-matter-only halo at r is the enclosed mass at r + d(r) afterwards: the cumulative counts inside
    r_k before BaryonifySnapshot equal those inside r_k + a displacement(r_k) after it (the runner's offset is displacement * a)."""
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    rng = np.random.default_rng(707)
    L, zr, eps = 200.0, 0.2, 5.0
    h = np.array([100.0, 90.0, 110.0])
    part = (h + rng.normal(scale=1.5, size=(60_000, 3))) % L
    cat = {'M': np.array([1e14]), 'x': h[:1], 'y': h[1:2], 'z': h[2:]}
    HCat, Snap = _objects(cat, part, L, zr, 3)
    z, Mt, r = np.linspace(0.15, 0.25, 3), np.geomspace(5e13, 2e14, 5), np.geomspace(1e-3, 2e2, 400)
    model = bfg.Profiles.Baryonification3D(None, None, bfg.utils.Cosmology.from_dict(syn.COSMO), epsilon_max=eps)
    model.set_table(z, Mt, r, syn.displacement_table(z, Mt, r))
    a = 1.0 / (1.0 + zr)
    r_k = np.geomspace(0.1, 4.0, 17)
    r_after = r_k + a * np.asarray(model.displacement(r_k, HCat.cat['M'][0], a), dtype=np.float64).reshape(-1)
    assert np.all(np.diff(r_after) > 0) and r_after[0] > 0 and np.any(np.abs(r_after - r_k) > 1e-3)
    before = bfg.Runners.MeasureProfilesSnapshot(HCat, Snap, eps, verbose=False, r_edges=np.concatenate([[0.0], r_k]))
    after = bfg.Runners.MeasureProfilesSnapshot(HCat, Snap, eps, verbose=False, r_edges=np.concatenate([[0.0], r_after]))
    assert before.radii()[1][0] > max(r_k[-1], r_after[-1])           # every edge lies inside the ball
    moved = bfg.Runners.BaryonifySnapshot(HCat, Snap, eps, model, verbose=False).process()
    n_before = np.cumsum(before.process(weights=False).npart[0])       # N(< r_k)
    n_after = np.cumsum(after.process(cat=moved, weights=False).npart[0])
    d = K.separations(part, np.array([HCat.cat[k][0] for k in ('x', 'y', 'z')], dtype=np.float64), L)[1]
    slack = np.array([np.count_nonzero(np.abs(d - rk) <= 1e-8 * rk) for rk in r_k])
    print('N(< r_k) before:', n_before, ' after - before:', n_after - n_before, ' slack:', slack)
    assert n_before[-1] > 40_000 and np.all(np.diff(n_before) > 0)
    assert np.all(np.abs(n_after - n_before) <= slack)
    # and the displacement is visible where it is defined: measured with the edges of `before`, the displaced counts differ
    assert np.any(np.cumsum(before.process(cat=moved, weights=False).npart[0]) != n_before)
