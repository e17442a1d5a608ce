"""CPU checks of the inputs of test_gpu_snapshot_regimes.py (snapshot_regimes.py): for every regime the brute-force oracle runs alone and
the preconditions that make the GPU comparison discriminating are asserted -- conditions on the inputs, held by the builder's fixed seeds.
Printed per regime (pytest -s): pairs per particle, face crossings, halos with a clamped query radius."""
import numpy as np
import pytest

import snapshot_regimes as SR

CASES = [(name, ndim) for name in SR.REGIMES for ndim in (2, 3)]
DEPOSIT_GRID = {3: 33, 2: 100}


def _setup(name, ndim):
    c = SR.case(name, ndim)
    ora, pairs = SR.oracle(name, ndim)
    d, inball = SR.separations(c)
    return c, ora, pairs, d, inball


@pytest.mark.parametrize('name,ndim', CASES)
def test_oracle_census_and_table_range(name, ndim):
    """the numpy restatement of the ball query counts the oracle's pairs; every halo lies inside the table's z and M range and every
    nonzero in-ball separation strictly inside its r range, so that no in-ball pair reads NaN (offset 0) but d = 0"""
    c, ora, pairs, d, inball = _setup(name, ndim)
    assert pairs == np.count_nonzero(inball) > 0
    lnM = np.log(c['M'].astype(np.float32)).astype(np.float64)
    assert np.log(c['tab_M'][0]) < lnM.min() and lnM.max() < np.log(c['tab_M'][-1])
    assert c['tab_z'][0] < c['redshift'] < c['tab_z'][-1]
    sep = d[inball & (d > 0)]
    assert c['tab_r'][0] < sep.min() and sep.max() < c['tab_r'][-1]
    on_centre = np.count_nonzero(inball & (d == 0))
    assert on_centre == np.count_nonzero(c['kind'] == SR.CENTRE)
    assert np.array_equal(np.isnan(ora).any(axis=1), (inball & (d == 0)).any(axis=1)) and np.array_equal(np.isnan(ora).any(axis=1), np.isnan(ora).all(axis=1))
    clamped = np.count_nonzero(c['R_q'] == c['L'] / 2)
    up, down = SR.crossings(c, ora)
    print('%s %dD: %d particles, %d halos (%d with R_q clamped to L / 2), %d pairs = %.2f per particle, crossings up %s down %s'
          % (name, ndim, c['part'].shape[0], c['M'].size, clamped, pairs, pairs / c['part'].shape[0], up.sum(axis=0), down.sum(axis=0)))
    if name == 'half_box_balls':
        assert clamped == c['M'].size
    if name == 'cluster_core':
        assert pairs / c['part'].shape[0] > 3                        # the hit queue holds 3 per particle: it overflows every round
    if name == 'rcut_bites':                                         # the strict d < rcut decides pairs: some in-ball pairs lie at or beyond the cut
        rcut = c['eps_model'] * SR.query_radii(c['M'], np.inf, 1.0)
        assert np.count_nonzero(inball & (d >= rcut[None, :])) > 100 and np.count_nonzero(inball & (d < rcut[None, :])) > 100


@pytest.mark.parametrize('name,ndim', CASES)
def test_surface_shells(name, ndim):
    """the particles at R_q (1 -+ 1e-9) are inside / outside their halo's ball in the oracle's own arithmetic; an inner one is displaced
    by more than 1e-6 of the largest displacement (so a dropped surface hit shows in the positions -- in half_box_balls and rcut_bites the
    pair count tells instead); an outer one that lies in no other ball does not move at all"""
    c, ora, pairs, d, inball = _setup(name, ndim)
    rows = np.arange(c['part'].shape[0])
    inner, outer = c['kind'] == SR.INNER, c['kind'] == SR.OUTER
    if name.startswith('tails_') and int(name[6:]) < 255:
        assert inner.sum() + outer.sum() <= 1
        return
    assert inner.sum() > 0 and outer.sum() > 0
    assert np.all(inball[rows[inner], c['owner'][inner]]) and not np.any(inball[rows[outer], c['owner'][outer]])
    off = SR.offsets(c, ora)
    scale = np.nanmax(np.abs(off))
    if name not in ('half_box_balls', 'rcut_bites'):
        assert np.abs(off[inner]).max(axis=1).min() > 1e-6 * scale
    alone = outer & ~inball.any(axis=1)
    assert np.array_equal(ora[alone], c['part'][alone])
    if name == 'gpc_box':
        assert alone.sum() > 0.8 * outer.sum()                       # (isolated balls: most outer particles are in no ball at all)


@pytest.mark.parametrize('name', ['small_box', 'cluster_core'])
@pytest.mark.parametrize('ndim', [2, 3])
def test_face_crossings(name, ndim):
    """at least 5 particles are displaced through a face in each direction on some axis: the re-wrap runs both ways"""
    c, ora, pairs, d, inball = _setup(name, ndim)
    up, down = SR.crossings(c, ora)
    assert up.sum(axis=0).max() >= 5 and down.sum(axis=0).max() >= 5
    assert np.nanmin(ora) >= 0.0 and np.nanmax(ora) <= c['L']


@pytest.mark.parametrize('name', ['small_box', 'tails_4097'])
@pytest.mark.parametrize('ndim', [2, 3])
def test_no_displaced_particle_on_a_grid_edge(name, ndim):
    """the fused deposit is compared cell for cell: no displaced coordinate of the oracle lies within 1e-9 L of an edge of the map's grid,
    so that no rounding decides a cell (allowed share of such particles: 0)"""
    c, ora, pairs, d, inball = _setup(name, ndim)
    edges = np.linspace(0, c['L'], DEPOSIT_GRID[ndim] + 1)
    v = ora[~np.isnan(ora)]
    assert np.abs(v[:, None] - edges[None, :]).min() > 1e-9 * c['L']
    assert np.isnan(ora).any() or name != 'small_box'                # (the particles on a halo centre: NaN, in no cell)


def test_tails_are_prefixes_of_small_box():
    for ndim in (2, 3):
        full = SR.case('small_box', ndim)
        for n in SR.TAIL_SIZES:
            c = SR.case('tails_%d' % n, ndim)
            assert c['part'].shape == (n, ndim) and np.array_equal(c['part'], full['part'][:n]) and np.array_equal(c['hpos'], full['hpos'])
            assert np.array_equal(SR.oracle('tails_%d' % n, ndim)[0], SR.oracle('small_box', ndim)[0][:n], equal_nan=True)
