"""deposit_cloud_oracle.py (the CIC / TSC oracle of test_gpu_deposit_cloud.py) against hand-computed cases, and the parts of the feature
that need no GPU: make_map's argument check, the three C entries' export, signatures and order check."""
import ctypes as C

import numpy as np
import pytest

import deposit_cloud_oracle as CO
import deposit_oracle as DO


def _one(v, N, L, order):
    keep, cells, w = CO.weights(np.array([v], dtype=np.float64), N, L, order)
    return bool(keep[0]), cells[0].tolist(), w[0].tolist()


@pytest.mark.parametrize('order', [2, 3])
@pytest.mark.parametrize('N,L', [(1, 1.0), (2, 2.0), (7, 7.0), (33, 250.0 / 3.0), (130, 0.37)])
def test_weights_are_nonnegative_and_sum_to_one(N, L, order):
    rng = np.random.default_rng(N)
    edges = np.linspace(0.0, L, N + 1)
    centres = 0.5 * (edges[1:] + edges[:-1])
    v = np.concatenate([rng.uniform(0, L, 20000), edges, centres, np.nextafter(edges, np.inf)[:-1], np.nextafter(edges, -np.inf)[1:],
                        np.nextafter(centres, np.inf), np.nextafter(centres, -np.inf), [-0.0]])
    keep, cells, w = CO.weights(v, N, L, order)
    assert keep.all() and (w >= 0).all() and (w <= 1).all()
    assert np.abs(w.sum(axis=1) - 1).max() <= 4 * 2.0 ** -53 * (1 + N * (order == 3))          # (TSC: d carries the rounding of v s, |t| <= N)
    assert cells.min() >= 0 and cells.max() <= N - 1
    assert np.array_equal(cells[:, 1], (cells[:, 0] + 1) % N)
    assert np.array_equal(cells[:, order - 2], CO.base_cell(v, N, L, order))


def test_particle_on_a_cell_centre():
    # centre of cell 3 of 8 on [0, 8]
    assert _one(3.5, 8, 8.0, 2) == (True, [3, 4], [1.0, 0.0])
    assert _one(3.5, 8, 8.0, 3) == (True, [2, 3, 4], [0.125, 0.75, 0.125])
    # the same with s = 4: L = 2, centre of cell 3 at 0.875
    assert _one(0.875, 8, 2.0, 2) == (True, [3, 4], [1.0, 0.0])
    assert _one(0.875, 8, 2.0, 3) == (True, [2, 3, 4], [0.125, 0.75, 0.125])


def test_particle_on_a_cell_edge():
    # the edge between cells 2 and 3: CIC halves; TSC sits at d = -0.5 of cell 3: 0.5, 0.5, 0
    assert _one(3.0, 8, 8.0, 2) == (True, [2, 3], [0.5, 0.5])
    assert _one(3.0, 8, 8.0, 3) == (True, [2, 3, 4], [0.5, 0.5, 0.0])
    # a quarter of a cell past the edge
    assert _one(3.25, 8, 8.0, 2) == (True, [2, 3], [0.25, 0.75])
    assert _one(3.25, 8, 8.0, 3) == (True, [2, 3, 4], [0.5 * 0.75 ** 2, 0.75 - 0.0625, 0.5 * 0.25 ** 2])


def test_the_wrap():
    # v = 0: CIC u = -0.5, i = -1: cells 7 and 0, halves; TSC i = 0, d = -0.5: cells 7, 0, 1
    assert _one(0.0, 8, 8.0, 2) == (True, [7, 0], [0.5, 0.5])
    assert _one(-0.0, 8, 8.0, 2) == (True, [7, 0], [0.5, 0.5])
    assert _one(0.0, 8, 8.0, 3) == (True, [7, 0, 1], [0.5, 0.5, 0.0])
    # v = L: CIC i = 7, f = 0.5: cells 7 and 0; TSC i = min(8, 7), d = 0.5: cells 6, 7, 0 with 0, 0.5, 0.5
    assert _one(8.0, 8, 8.0, 2) == (True, [7, 0], [0.5, 0.5])
    assert _one(8.0, 8, 8.0, 3) == (True, [6, 7, 0], [0.0, 0.5, 0.5])
    # u in [-0.5, 0): v = 0.25, u = -0.25, i = -1, f = 0.75
    assert _one(0.25, 8, 8.0, 2) == (True, [7, 0], [0.25, 0.75])
    assert _one(0.25, 8, 8.0, 3) == (True, [7, 0, 1], [0.5 * 0.75 ** 2, 0.75 - 0.0625, 0.5 * 0.25 ** 2])
    # the last cell's upper half
    assert _one(7.75, 8, 8.0, 2) == (True, [7, 0], [0.75, 0.25])
    assert _one(7.75, 8, 8.0, 3) == (True, [6, 7, 0], [0.5 * 0.25 ** 2, 0.75 - 0.0625, 0.5 * 0.75 ** 2])


@pytest.mark.parametrize('order', [2, 3])
def test_one_and_two_cells_add_the_coincident_cells(order):
    m = np.array([3.0, 5.0])
    # N = 1: everything lands in the one cell, whatever the position
    for ndim in (2, 3):
        got = CO.deposit([np.array([0.25, 1.0])] * ndim, m, 1, 1.0, order)
        assert got.shape == (1,) * ndim and got.ravel()[0] == 8.0
    # N = 2 on [0, 2], one axis at a time (the other at a cell centre of cell 0, where CIC is one cell)
    keep, cells, w = CO.weights(np.array([0.25]), 2, 2.0, order)
    if order == 2:                                               # u = -0.25: cells 1 and 0 with 0.25, 0.75
        assert cells[0].tolist() == [1, 0] and w[0].tolist() == [0.25, 0.75]
        assert CO.deposit([np.array([0.25]), np.array([0.5])], None, 2, 2.0, 2).tolist() == [[0.75, 0.0], [0.25, 0.0]]
    else:                                                        # i = 0, d = -0.25: cells 1, 0, 1: cell 1 gets the two outer weights
        assert cells[0].tolist() == [1, 0, 1]
        got = CO.deposit([np.array([0.25]), np.array([0.5])], None, 2, 2.0, 3)
        wy = np.array([0.75, 0.25])                              # y = 0.5: d = 0: 1/8 + 1/8 to cell 1, 3/4 to cell 0
        wx = np.array([0.75 - 0.0625, 0.5 * 0.75 ** 2 + 0.5 * 0.25 ** 2])
        assert np.array_equal(got, np.outer(wx, wy)) and got.sum() == 1.0


@pytest.mark.parametrize('order', [2, 3])
def test_particles_outside_and_nan_are_dropped_whole(order):
    L, N = 8.0, 8
    bad = [np.nan, np.inf, -np.inf, -0.125, 8.125, np.nextafter(8.0, np.inf), -5e-324]
    for ndim in (2, 3):
        for axis in range(ndim):
            cols = [np.full(len(bad) + 2, 3.5) for _ in range(ndim)]
            cols[axis][:len(bad)] = bad
            cols[axis][-2:] = [8.0, -0.0]                        # inside
            assert CO.kept(cols, L).tolist() == [False] * len(bad) + [True, True]
            got = CO.deposit(cols, np.full(len(bad) + 2, 2.0), N, L, order)
            assert got.sum() == 4.0 and np.isfinite(got).all()
            # np.histogramdd keeps the same particles
            ref = np.histogramdd(np.stack(cols, axis=1)[~np.isnan(cols[axis])], bins=[np.linspace(0, L, N + 1)] * ndim)[0]
            assert ref.sum() == 2.0


@pytest.mark.parametrize('order', [2, 3])
@pytest.mark.parametrize('ndim,N', [(3, 1), (3, 2), (3, 3), (3, 33), (2, 1), (2, 2), (2, 130)])
def test_mass_is_conserved_exactly_on_the_lattice(ndim, N, order):
    """L == N, coordinates multiples of 1/8, masses k / 1024: every weight, product and sum is exact in fp64"""
    rng = np.random.default_rng(10 * N + order)
    n = 20000
    p = rng.integers(-4, 8 * N + 5, (n, ndim)) / 8.0             # some outside
    mass = DO.dyadic_masses(rng, n)
    cols = [p[:, a] for a in range(ndim)]
    keep = CO.kept(cols, float(N))
    assert 0 < np.count_nonzero(~keep) < n
    got = CO.deposit(cols, mass, N, float(N), order)
    total = float(np.sum((mass[keep] * 1024).astype(np.int64))) / 1024.0
    assert got.sum() == total
    # in any order of the particles, and particle by particle
    perm = rng.permutation(n)
    assert np.array_equal(got, CO.deposit([c[perm] for c in cols], mass[perm], N, float(N), order))
    few = slice(0, 50)
    one_by_one = sum(CO.deposit([c[i:i + 1] for c in cols], mass[i:i + 1], N, float(N), order) for i in range(50))
    assert np.array_equal(one_by_one, CO.deposit([c[few] for c in cols], mass[few], N, float(N), order))


def test_make_map_refuses_an_unknown_assignment_without_a_gpu():
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    snap = bfg.utils.ParticleSnapshot(x=np.array([0.5, 1.5]), y=np.array([0.5, 1.5]), z=np.array([0.5, 1.5]), M=np.ones(2), L=8.0, redshift=0.0,
                                      cosmo=dict(syn.COSMO))
    for bad in ('nope', 'none', '', 2, None):
        with pytest.raises(ValueError, match="assignment must be 'ngp', 'cic' or 'tsc'"):
            snap.make_map(8, assignment=bad)


def test_the_three_entries_are_exported_with_signatures_and_check_the_order():
    from baryonification_amd import _lib
    names = ('bfgx_deposit_cloud_device', 'bfgx_deposit_cloud', 'bfgx_deposit_cloud_records')
    L = _lib.load()
    for name, nargs in zip(names, (12, 11, 13)):
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(_lib.SYMBOLS[name][1])
    # order is checked before any device is touched: NGP and anything else are sent to bfgx_deposit_particles
    x = np.array([0.5])
    out = np.full(8, -7.0)
    for order in (0, 1, 4, -2):
        rc = L.bfgx_deposit_cloud(0, 3, 1, x.ctypes.data, x.ctypes.data, x.ctypes.data, None, 2, 2.0, order, out.ctypes.data)
        assert rc == _lib.ERR_INVALID and b'bfgx_deposit_particles' in L.bfgx_last_error()
        rc = L.bfgx_deposit_cloud_device(0, None, 3, 1, x.ctypes.data, x.ctypes.data, x.ctypes.data, None, 2, 2.0, order, out.ctypes.data)
        assert rc == _lib.ERR_INVALID and b'bfgx_deposit_particles' in L.bfgx_last_error()
        rec = np.zeros(1, dtype=[('M', np.float64), ('x', np.float64), ('y', np.float64), ('z', np.float64)])
        rc = L.bfgx_deposit_cloud_records(0, 3, 1, rec.ctypes.data, 32, 8, 16, 24, 0, 2, 2.0, order, out.ctypes.data)
        assert rc == _lib.ERR_INVALID and b'bfgx_deposit_particles' in L.bfgx_last_error()
    assert (out == -7.0).all()
    from baryonification_amd import engine
    assert callable(engine.deposit_cloud_device)
