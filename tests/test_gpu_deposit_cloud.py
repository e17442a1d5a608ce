"""The CIC / TSC particle deposit (csrc/bfgx_deposit_cloud.hpp: the tile-owned form with its halo scratch and fold, the atomic form)
case by case against deposit_cloud_oracle.py (plain numpy, checked against hand-computed cases in test_deposit_cloud_oracle_host.py).

Exact cases use L == N (s == 1.0), coordinates that are multiples of 1/8 and masses k / 1024: every weight (multiples of 1/128), product
(2^-21 in 3-D) and sum is exact in fp64 whatever the order of addition, so the maps are compared with np.array_equal -- a cloud placed one
cell off, a halo cell folded twice or not at all cannot hide under a tolerance.  The output is filled with NaN before every call: the
tiled form stores every cell, it does not zero the map.  Two cases keep a box length that fp64 does not hold and a derived per-cell bound.
Every "reaches the branch" statement is an assertion on the INPUTS through the oracle and deposit_oracle.geometry, made before the GPU call."""
import numpy as np
import pytest

import deposit_cloud_oracle as CO
import deposit_oracle as DO

pytestmark = pytest.mark.gpu

L_ODD = 250.0 / 3.0                                   # not representable in fp64
FORMS = ['tiled', 'atomic']
ORDERS = [2, 3]
PARTIAL = [(3, 33), (3, 40), (2, 130), (2, 200)]      # grids that are no multiple of the tile side: the wrap cell lies inside the LDS box


def _deposit(monkeypatch, form, coords, mass, N, L, order):
    """the map of engine.deposit_cloud_device for host columns, the output pre-filled with NaN"""
    import torch
    from baryonification_amd import engine
    monkeypatch.setenv('BFGX_DEPOSIT', form)
    dev = torch.device('cuda:0')
    ndim, n = len(coords), coords[0].size
    cols = [torch.from_numpy(np.ascontiguousarray(c, dtype=np.float64)).to(dev) for c in coords]
    m = None if mass is None else torch.from_numpy(np.ascontiguousarray(mass, dtype=np.float64)).to(dev)
    out = torch.full((N,) * ndim, float('nan'), dtype=torch.float64, device=dev)
    ptr = [c.data_ptr() if n else 0 for c in cols] + [0] * (3 - ndim)
    engine.deposit_cloud_device(ptr[0], ptr[1], ptr[2], m.data_ptr() if (m is not None and n) else 0, n, N, L, order, out.data_ptr(), ndim)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same(got, ref):
    assert got.shape == ref.shape
    bad = got != ref                                                  # (a cell left NaN differs too)
    assert not bad.any(), '%d of %d cells differ, sum %r against %r, first at %s' % (
        bad.sum(), bad.size, np.nansum(got), ref.sum(), np.argwhere(bad)[:5].tolist())
    assert np.array_equal(got, ref)


def _check(monkeypatch, form, p, mass, N, order):
    """exact comparison on the lattice: L == N"""
    coords = [p[:, a] for a in range(p.shape[1])]
    ref = CO.deposit(coords, mass, N, float(N), order)
    _same(_deposit(monkeypatch, form, coords, mass, N, float(N), order), ref)
    return ref


def _lattice(rng, n, ndim, N):
    """multiples of 1/8 in [0, N], both ends included"""
    return rng.integers(0, 8 * N + 1, (n, ndim)) / 8.0


def _tiles_touched(g, p, N, order):
    """number of distinct tiles that the cloud of every particle feeds (a product set: distinct tiles per axis, multiplied)"""
    count = np.ones(p.shape[0], dtype=np.int64)
    for a in range(g.ndim):
        _, cells, w = CO.weights(p[:, a], N, float(N), order)
        t = np.where(w > 0, cells // g.shape[a], -1)                  # (a cell of weight zero feeds nothing)
        t.sort(axis=1)
        distinct = (t[:, 1:] != t[:, :-1]).sum(axis=1) + 1 - (t[:, 0] < 0)
        count *= distinct
    return count


def _seam_particles(rng, g, N, k):
    """k particles in the LAST cell of a tile on all axes at once, in its upper half (CIC reaches the next tile on every axis), and k in
    the FIRST cell of a tile on all axes, in its lower half (CIC and TSC reach the tile below on every axis)"""
    last = [np.minimum((np.arange(nt) + 1) * s, N) - 1 for nt, s in zip(g.ntiles, g.shape)]
    first = [np.arange(nt) * s for nt, s in zip(g.ntiles, g.shape)]
    up = np.stack([rng.choice(c, k) for c in last], axis=1) + 0.5 + rng.integers(1, 4, (k, g.ndim)) / 8.0
    down = np.stack([rng.choice(c, k) for c in first], axis=1) + rng.integers(0, 4, (k, g.ndim)) / 8.0
    return up, down


# --------------------------------------------------------------------------------------------- partial tiles and seams
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('ndim,N', PARTIAL)
def test_partial_tiles_and_seams(gpu, monkeypatch, ndim, N, order, form):
    """clouds that straddle tile seams on all axes at once, on grids whose last tile is partial (N = 33: one cell wide), plus random
    lattice particles"""
    rng = np.random.default_rng(100 * N + order)
    g = DO.geometry(ndim, N)
    assert all(N % s for s in g.shape) and g.T > 1
    up, down = _seam_particles(rng, g, N, 300)
    assert np.count_nonzero(_tiles_touched(g, up, N, order) >= 2 ** ndim) >= 50
    # the lower corner neighbour: the first cloud cell lies in another tile than the base cell on EVERY axis
    corner = np.ones(300, dtype=bool)
    for a in range(ndim):
        _, cells, w = CO.weights(down[:, a], N, float(N), order)          # (cells[:, 1] is the tile's first cell for both orders)
        corner &= (cells[:, 0] // g.shape[a] != cells[:, 1] // g.shape[a]) & (w[:, 0] > 0)
        assert np.array_equal(cells[:, 1] % g.shape[a], np.zeros(300, dtype=np.int64))
    assert np.count_nonzero(corner) >= 50
    p = np.concatenate([up, down, _lattice(rng, 3000, ndim, N)])
    ref = _check(monkeypatch, form, p, DO.dyadic_masses(rng, p.shape[0]), N, order)
    assert ref.sum() > 0


# --------------------------------------------------------------------------------------------- the wrap
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('ndim,N', PARTIAL)
def test_the_wrap_and_dropped_particles(gpu, monkeypatch, ndim, N, order, form):
    """particles within one cell of every face, edge and corner of the box (v = 0, L, -0.0 and CIC's base -1 among them); beside them NaN,
    +-inf and values just outside on each axis in turn, which drop the particle whole"""
    rng = np.random.default_rng(200 * N + order)
    Lb = float(N)
    low = np.array([0.0, -0.0, 0.125, 0.375, 0.5, 0.875])
    high = Lb - np.array([0.0, 0.125, 0.5, 0.625, 0.875])
    n = 3000
    kind = rng.integers(0, 3, (n, ndim))                               # per axis: near 0, near L, anywhere
    p = np.choose(kind, [rng.choice(low, (n, ndim)), rng.choice(high, (n, ndim)), _lattice(rng, n, ndim, N)])
    near = (kind < 2).sum(axis=1)
    assert all(np.count_nonzero(near == k) >= 50 for k in range(1, ndim + 1))        # faces, edges (and corners in 3-D)
    for combo in range(2 ** ndim):                                     # every corner (edge of a 2-D box), by its low / high pattern
        want = [(combo >> a) & 1 for a in range(ndim)]
        assert np.count_nonzero((kind == want).all(axis=1)) >= 5
    assert np.count_nonzero(p == 0.0) > 50 and np.count_nonzero(np.signbit(p) & (p == 0.0)) > 10 and np.count_nonzero(p == Lb) > 50
    if order == 2:
        assert np.count_nonzero(np.floor(p - 0.5) == -1) > 100         # CIC base -1
    bad = np.array([np.nan, np.inf, -np.inf, -0.125, Lb + 0.125, np.nextafter(Lb, np.inf), -5e-324])
    rows = []
    for a in range(ndim):
        q = _lattice(rng, bad.size, ndim, N)
        q[:, a] = bad
        rows.append(q)
    dropped = np.concatenate(rows)
    assert not CO.kept([dropped[:, a] for a in range(ndim)], Lb).any() and CO.kept([p[:, a] for a in range(ndim)], Lb).all()
    allp = rng.permutation(np.concatenate([p, dropped]))
    mass = DO.dyadic_masses(rng, allp.shape[0])
    ref = _check(monkeypatch, form, allp, mass, N, order)
    keep = CO.kept([allp[:, a] for a in range(ndim)], Lb)
    assert ref.sum() == float(np.sum((mass[keep] * 1024).astype(np.int64))) / 1024.0


# --------------------------------------------------------------------------------------------- a tile that is its own neighbour
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('with_mass', [True, False])
@pytest.mark.parametrize('ndim,N', [(3, 1), (3, 2), (3, 3), (3, 16), (2, 1), (2, 2), (2, 64)])
def test_a_tile_that_is_its_own_neighbour(gpu, monkeypatch, ndim, N, with_mass, order, form):
    """one tile per axis: every halo cell of the tile folds back into the tile itself; N = 1 and 2: several cloud cells are one cell"""
    rng = np.random.default_rng(300 * N + 10 * ndim + order)
    g = DO.geometry(ndim, N)
    assert g.T == 1
    p = _lattice(rng, 2000, ndim, N)
    p[:4] = [[0.0] * ndim, [float(N)] * ndim, [-0.0] * ndim, [0.5] * ndim]
    ref = _check(monkeypatch, form, p, DO.dyadic_masses(rng, 2000) if with_mass else None, N, order)
    if not with_mass:
        assert ref.sum() == 2000.0


# --------------------------------------------------------------------------------------------- particle counts
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('n', [0, 1, 255, 4095, 4096, 4097, 8193])
def test_particle_counts_around_the_chunk(gpu, monkeypatch, n, order, form):
    rng = np.random.default_rng(n)
    N = 40
    p = _lattice(rng, n, 3, N) if n != 1 else np.array([[27.625, 40.0, 0.0]])
    ref = _check(monkeypatch, form, p, DO.dyadic_masses(rng, n), N, order)
    assert (ref.sum() > 0) == (n > 0)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('where', ['above', 'nan'])
def test_no_particle_inside(gpu, monkeypatch, where, order, form):
    """5000 particles, none inside the box: an all-zero map, no NaN left"""
    rng = np.random.default_rng(5)
    N, n = 40, 5000
    p = _lattice(rng, n, 3, N)
    p[np.arange(n), np.arange(n) % 3] = np.nan if where == 'nan' else N + 0.125 + rng.integers(0, 80, n) / 8.0
    assert not CO.kept([p[:, a] for a in range(3)], float(N)).any()
    for mass in (DO.dyadic_masses(rng, n), None):
        ref = _check(monkeypatch, form, p, mass, N, order)
        assert not ref.any()


# --------------------------------------------------------------------------------------------- more tiles than a sort pass ranks in LDS
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('order', ORDERS)
def test_tiles_beyond_the_level2_table(gpu, monkeypatch, order, form):
    """N = 257, 3-D: 2601 tiles, one chunk of 3000 sparse lattice particles that starts in bucket 0: tiles 2048 and up are counted with
    global atomics and placed key by key with their index payload; the halo scratch spans more than 2048 tiles"""
    rng = np.random.default_rng(257 + order)
    N = 257
    g = DO.geometry(3, N)
    p = _lattice(rng, 3000, 3, N)
    base = np.stack([CO.base_cell(p[:, a], N, float(N), order) for a in range(3)], axis=1)
    tile = DO.tile_of(g, base)
    assert g.T > DO.TABLE and p.shape[0] <= DO.CHUNK
    assert (tile // g.B2).min() == 0 and np.count_nonzero(tile >= DO.TABLE) > 50
    ref = _check(monkeypatch, form, p, DO.dyadic_masses(rng, 3000), N, order)
    assert np.count_nonzero(ref) > 3000


# --------------------------------------------------------------------------------------------- crowded cells in curve order
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('ndim,N', [(3, 80), (2, 300)])
def test_crowded_cells_in_curve_order(gpu, monkeypatch, ndim, N, order, form):
    """120 000 clustered lattice particles and 3000 in each of two single cells, sorted along a Z-curve of their base cells: whole waves add
    to the same few LDS cells.  Still exact: at most a few thousand particles reach a cell, far from 2^53 of the 2^-31 granularity"""
    rng = np.random.default_rng(N + order)
    n = 120_000
    centres = rng.uniform(0, N, (40, ndim))
    p = np.round(np.mod(centres[rng.integers(0, 40, n)] + rng.normal(0, 0.06 * N, (n, ndim)), N) * 8.0) / 8.0
    crowd = np.concatenate([c + rng.integers(0, 8, (3000, ndim)) / 8.0 for c in (np.full(ndim, 17.0), np.full(ndim, float(N - 1)))])
    p = np.concatenate([p, crowd])
    base = np.stack([CO.base_cell(p[:, a], N, float(N), order) for a in range(ndim)], axis=1)
    p = p[DO.morton_order(base)]
    coords = [p[:, a] for a in range(ndim)]
    touch = CO.deposit(coords, None, N, float(N), order, unit_weights=True)
    assert 3000 <= touch.max() <= 20000
    mass = DO.dyadic_masses(rng, p.shape[0]) * np.where(rng.uniform(size=p.shape[0]) < 0.3, -1.0, 1.0)
    ref = _check(monkeypatch, form, p, mass, N, order)
    assert np.count_nonzero(ref) > 0.2 * ref.size


# --------------------------------------------------------------------------------------------- generic input: the bound
def _bound(coords, mass, N, L, order):
    """per cell: see test_generic_input_within_the_derived_bound"""
    k = CO.deposit(coords, None, N, L, order, unit_weights=True, widen=1)
    s_abs = CO.deposit(coords, np.abs(mass), N, L, order)
    m_abs = CO.deposit(coords, np.abs(mass), N, L, order, unit_weights=True, widen=1)
    eps_w = (6.0 * N + 12.0) * 2.0 ** -53
    return 2.0 * k * 2.0 ** -53 * (s_abs + eps_w * m_abs) + eps_w * m_abs, k


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('order', ORDERS)
def test_generic_input_within_the_derived_bound(gpu, monkeypatch, order, form):
    """L = 250/3, N = 33, 400 000 uniform particles plus a clump, real masses of both signs.  Per cell, with S = sum |m w| over the
    oracle's contributions to it, and k, M = the number and the sum of |m| of the particles whose cloud, taken one cell wider on every
    side, holds the cell (a particle whose base cell comes out one off on one side reaches such a cell, with a weight within dw of 0):
      weights     t = v s is rounded once (|t| <= N: within N 2^-53 of v s) where numpy rounds the product and a compiler may contract it
                  into the subtraction that follows: the two sides' t differ by at most N 2^-52.  Every weight is a function of t of
                  slope <= 1 (CIC: 1; TSC: |0.5 -+ d| <= 1, |2 d| <= 1), continuous across a change of base cell, and is evaluated with at
                  most 3 roundings of numbers <= 1: |dw| <= N 2^-52 + 3 2^-53.  The product of up to three weights <= 1 and the mass
                  adds 3 more roundings: |d(m w)| <= |m| eps, eps = 3 N 2^-52 + 12 2^-53 = (6 N + 12) 2^-53: eps M per cell;
      summation   both sides add at most k terms in some order, of absolute sum at most S + eps M, each sum within (k - 1) 2^-53 of
                  that of the exact one: 2 k 2^-53 (S + eps M).
    bound = 2 k 2^-53 (S + eps M) + eps M."""
    rng = np.random.default_rng(11)
    N, n = 33, 400_000
    p = rng.uniform(-0.01 * L_ODD, 1.01 * L_ODD, (n, 3))
    p[:40000] = 0.3 * L_ODD + rng.normal(0, 0.01 * L_ODD, (40000, 3))   # cells with thousands of particles
    mass = rng.uniform(0.5, 2.0, n) * np.where(rng.uniform(size=n) < 0.3, -1.0, 1.0)
    coords = [p[:, a] for a in range(3)]
    ref = CO.deposit(coords, mass, N, L_ODD, order)
    bound, k = _bound(coords, mass, N, L_ODD, order)
    assert k.max() > 1000 and k.min() > 0 and 0 < np.count_nonzero(~CO.kept(coords, L_ODD)) < 0.1 * n
    got = _deposit(monkeypatch, form, coords, mass, N, L_ODD, order)
    err = np.abs(got - ref)
    print('max err / bound = %.3g, largest k = %d' % (np.nanmax(err / bound), k.max()))
    assert np.isfinite(got).all() and (err <= bound).all()


# --------------------------------------------------------------------------------------------- base-cell switches
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('ndim,N', [(3, 33), (2, 130)])
def test_base_cell_switches_move_nothing(gpu, monkeypatch, ndim, N, order, form):
    """L = 250/3: coordinates one ulp either side of (and on) every cell centre, where CIC changes its base cell, and every cell edge,
    where TSC does, on every axis in turn.  The assignment is continuous across the switch, so a particle whose base cell comes out
    differently on the GPU changes a cell by no more than the bound of test_generic_input_within_the_derived_bound; a cloud placed one
    cell off is an error of order m"""
    rng = np.random.default_rng(400 * N + order)
    edges = np.linspace(0.0, L_ODD, N + 1)
    centres = (np.arange(N) + 0.5) * (L_ODD / N)
    sw = np.concatenate([centres, edges])
    special = np.concatenate([sw, np.nextafter(sw, -np.inf)[sw > 0], np.nextafter(sw, np.inf)[sw < L_ODD]])
    rows = []
    for a in range(ndim):
        q = rng.uniform(0.0, L_ODD, (special.size, ndim))
        q[:, a] = special
        rows.append(q)
    p = np.concatenate(rows + [rng.uniform(0.0, L_ODD, (2000, ndim))])
    mass = rng.uniform(0.5, 2.0, p.shape[0])
    coords = [p[:, a] for a in range(ndim)]
    assert CO.kept(coords, L_ODD).all()
    # the input does switch: the doubles either side of a nominal switch point have different base cells (not at every point: the rounding
    # of v s moves the switch by an ulp or two)
    nominal = centres if order == 2 else edges[1:-1]
    below, above = (CO.base_cell(np.nextafter(nominal, d), N, L_ODD, order) for d in (-np.inf, np.inf))
    assert np.count_nonzero(below != above) >= N // 8
    ref = CO.deposit(coords, mass, N, L_ODD, order)
    bound, k = _bound(coords, mass, N, L_ODD, order)
    got = _deposit(monkeypatch, form, coords, mass, N, L_ODD, order)
    err = np.abs(got - ref)
    print('max err / bound = %.3g' % np.nanmax(err[k > 0] / bound[k > 0]))
    assert np.isfinite(got).all() and (err <= bound).all() and mass.min() > 1e6 * bound.max()


# --------------------------------------------------------------------------------------------- records
def _snapshot(ndim, rec, Lbox):
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    snap = bfg.utils.ParticleSnapshot(x=np.zeros(1), y=np.zeros(1), z=None if ndim == 2 else np.zeros(1), M=np.ones(1), L=Lbox, redshift=0.0,
                                      cosmo=dict(syn.COSMO))
    snap.cat = rec
    return snap


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('assignment', ['cic', 'TSC'])
@pytest.mark.parametrize('ndim,N', [(3, 40), (2, 130)])
def test_make_map_on_records_and_on_columns(gpu, monkeypatch, ndim, N, assignment, form):
    """a `cat` with extra fields between the coordinates goes to the device as it is (the kernels read at a stride of 7 doubles); a
    non-contiguous view of it takes the column entry; both equal the oracle.  A NaN mass raises the reference's AssertionError"""
    monkeypatch.setenv('BFGX_DEPOSIT', form)
    order = CO.ORDERS[assignment.lower()]
    rng = np.random.default_rng(N + order)
    n = 9000
    rec = np.zeros(2 * n, dtype=[('M', np.float64), ('z', np.float64), ('vx', np.float64), ('x', np.float64), ('id', np.int64), ('vy', np.float64),
                                 ('y', np.float64)])
    assert rec.dtype.itemsize == 56
    p = rng.integers(-2, 8 * N + 3, (2 * n, 3)) / 8.0                  # a few outside
    rec['x'], rec['y'], rec['z'], rec['M'] = p[:, 0], p[:, 1], p[:, 2], DO.dyadic_masses(rng, 2 * n)
    rec['vx'] = rec['vy'] = np.nan
    if ndim == 2:
        rec['z'] = np.nan                                              # (not read)
    coords = [p[:, a] for a in range(ndim)]
    assert 0 < np.count_nonzero(~CO.kept(coords, float(N))) < 0.1 * n
    got = _snapshot(ndim, rec, float(N)).make_map(N, assignment)
    _same(np.array(got), CO.deposit(coords, rec['M'], N, float(N), order))
    half = rec[::2]
    assert not half.flags.c_contiguous
    got = _snapshot(ndim, half, float(N)).make_map(N, assignment=assignment)
    _same(got, CO.deposit([c[::2] for c in coords], rec['M'][::2], N, float(N), order))
    rec['M'][77] = np.nan
    with pytest.raises(AssertionError, match="If you want to make a map, provide a value for the particle mass"):
        _snapshot(ndim, rec, float(N)).make_map(N, assignment)
    with pytest.raises(AssertionError, match="If you want to make a map, provide a value for the particle mass"):
        _snapshot(ndim, rec[1::2], float(N)).make_map(N, assignment)


# --------------------------------------------------------------------------------------------- the runner
def test_process_make_map_with_an_assignment(gpu, monkeypatch):
    """BaryonifySnapshot.process_make_map(N, assignment='tsc') == make_map(N, 'tsc') of process()'s catalog, cell for cell.  process() is
    called once and its catalog handed to both routes (its displacement sums run in an order that may differ from call to call): the
    same particles and the same weights bit for bit (the kernels evaluate them without contraction), added by global atomics in an
    order that differs from run to run -- so a cell's k terms of absolute sum S agree within 2 (k - 1) 2^-53 S, the summation bound of
    test_generic_masses_within_the_fp64_summation_bound, and equal the oracle within the same bound.  process_make_map(N) is what it was"""
    import helpers as H
    g = H.load_snapshot_golden('snap3d_rdelta')
    N = 32
    runner = H.snapshot_product_runner(g)
    ngp = runner.process_make_map(N)
    assert np.array_equal(ngp, runner.process_make_map(N, assignment='ngp')) and ngp.sum() > 0
    new = runner.process()
    assert np.abs(np.array(new['x']) - g['part'][:, 0]).max() > 0      # (particles did move)
    monkeypatch.setattr(runner, 'process', lambda: new)
    coords = [np.array(new[k]) for k in ('x', 'y', 'z')]
    for assignment in ('tsc', 'CIC'):
        order = CO.ORDERS[assignment.lower()]
        got = runner.process_make_map(N, assignment=assignment)
        two = runner._map_of(runner.process(), N, assignment)
        ref = CO.deposit(coords, new['M'], N, g['L'], order)
        k = CO.deposit(coords, None, N, g['L'], order, unit_weights=True)
        bound = 2.0 * np.maximum(k - 1, 0) * 2.0 ** -53 * CO.deposit(coords, np.abs(new['M']), N, g['L'], order)
        print('%s: max |fused - two calls| / bound = %.3g, against the oracle %.3g' % (
            assignment, np.max(np.abs(got - two)[k > 1] / bound[k > 1]), np.max(np.abs(got - ref)[k > 1] / bound[k > 1])))
        assert (np.abs(got - two) <= bound).all() and (np.abs(got - ref) <= bound).all() and np.abs(got - ngp).max() > 0.1
    with pytest.raises(ValueError, match="assignment"):
        runner.process_make_map(N, assignment='nope')
