"""The particle deposit's sort and routing kernels (csrc/bfgx_deposit.hpp, particle_deposit_kernel and nan_scan_strided_kernel of
bfgx_grid.hpp, the exclusive scan of bfgx_scan.hpp) case by case against deposit_oracle.py (searchsorted + bincount, checked against
np.histogramdd in test_deposit_oracle_host.py): grids with more tiles than a sort pass ranks in LDS, edges read from global memory, a
particle on every edge and one ulp either side of it with uniform and non-uniform edges, particles in space-filling-curve order,
particle counts around the chunk size and inputs with no particle inside, slabs that are no multiple of the tile side, records at a
stride, the second copy and tile totals of the fused entry, routing to up to 255 ranks.

Masses are dyadic (k / 1024): every order of addition gives the same fp64 sum, so every map is compared with np.array_equal -- a
misplaced, doubled or dropped particle cannot hide under a tolerance.  The output is filled with NaN before every call (the tiled form
stores every cell, it does not zero the map).  One case keeps generic masses and a derived per-cell bound.  Every "reaches the branch"
statement is an assertion on the INPUTS through deposit_oracle.geometry, made before the GPU call; no assertion on a kernel's output
goes through it."""
import numpy as np
import pytest

import deposit_oracle as DO

pytestmark = pytest.mark.gpu

L = 250.0 / 3.0                                       # not representable in fp64
FORMS = ['tiled', 'atomic']


def _deposit(monkeypatch, form, coords, mass, edges, plane_lo=0, plane_n=None):
    """the map of engine.deposit_particles_device / _slab_device for host columns, the output pre-filled with NaN"""
    import torch
    from baryonification_amd import engine
    monkeypatch.setenv('BFGX_DEPOSIT', form)
    dev = torch.device('cuda:0')
    ndim, N, n = len(coords), edges.size - 1, coords[0].size
    cols = [torch.from_numpy(np.ascontiguousarray(c, dtype=np.float64)).to(dev) for c in coords]
    m = None if mass is None else torch.from_numpy(np.ascontiguousarray(mass, dtype=np.float64)).to(dev)
    e = torch.from_numpy(edges).to(dev)
    out = torch.full((N if plane_n is None else plane_n,) + (N,) * (ndim - 1), float('nan'), dtype=torch.float64, device=dev)
    ptr = [c.data_ptr() if n else 0 for c in cols] + [0] * (3 - ndim)
    mp = m.data_ptr() if (m is not None and n) else 0
    if plane_n is None:
        engine.deposit_particles_device(ptr[0], ptr[1], ptr[2], mp, n, N, e.data_ptr(), out.data_ptr(), ndim)
    else:
        engine.deposit_particles_slab_device(ptr[0], ptr[1], ptr[2], mp, n, N, e.data_ptr(), plane_lo, plane_n, out.data_ptr(), ndim)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same(got, ref):
    assert got.shape == ref.shape
    bad = got != ref                                                  # (a cell left NaN differs too)
    assert not bad.any(), '%d of %d cells differ, sum %r against %r, first at %s' % (
        bad.sum(), bad.size, np.nansum(got), ref.sum(), np.argwhere(bad)[:5].tolist())
    assert np.array_equal(got, ref)


def _check(monkeypatch, form, p, mass, edges, plane_lo=0, plane_n=None):
    coords = [p[:, a] for a in range(p.shape[1])]
    ref = DO.histogramdd(coords, mass, edges, plane_lo, plane_n)
    _same(_deposit(monkeypatch, form, coords, mass, edges, plane_lo, plane_n), ref)
    return ref


def _buckets(g, p, edges, plane_lo=0):
    return DO.buckets_of(g, [p[:, a] for a in range(p.shape[1])], edges, plane_lo)


# --------------------------------------------------------------------------------------------- level 2 beyond its LDS table
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('with_mass', [True, False])
@pytest.mark.parametrize('ndim,N', [(3, 257), (2, 4160)])
def test_tiles_beyond_the_level2_table(gpu, monkeypatch, ndim, N, with_mass, form):
    """more than 2048 tiles and ONE chunk of sparse particles that starts in bucket 0: tiles 2048 and up are counted with global atomics
    (deposit_count_kernel) and placed key by key with their masses (deposit_split_kernel<2>, rank -2).  N = 4160: the edges are also
    read from global memory"""
    rng = np.random.default_rng(N)
    g = DO.geometry(ndim, N)
    edges = np.linspace(0.0, L, N + 1)
    p = rng.uniform(-0.005 * L, 1.005 * L, (3000, ndim))
    bucket, tile = _buckets(g, p, edges)
    assert g.T > DO.TABLE and p.shape[0] <= DO.CHUNK
    assert bucket[bucket >= 0].min() == 0 and np.count_nonzero(tile >= DO.TABLE) > 50 and 0 < np.count_nonzero(bucket < 0) < 200
    assert (edges.size > DO.EDGES_LDS) == (N == 4160)
    ref = _check(monkeypatch, form, p, DO.dyadic_masses(rng, 3000) if with_mass else None, edges)
    assert np.count_nonzero(ref) > 2500


@pytest.mark.parametrize('form', FORMS)
def test_one_tile_fed_by_ranges_and_key_by_key(gpu, monkeypatch, form):
    """N = 257, 3-D: ~1000 particles in tiles below bucket 33, ~6000 inside the 64 tiles of bucket 33.  Sorted by bucket, chunk 0 starts in
    bucket 0 and ends inside bucket 33 (those keys lie >= 2048 tiles past its first bucket: one returning atomic each), chunk 1 starts in
    bucket 33 (its keys go by ranges): both kinds of cursor updates meet in the same tiles"""
    rng = np.random.default_rng(33)
    N, B = 257, 33
    g = DO.geometry(3, N)
    edges = np.linspace(0.0, L, N + 1)
    tiles = rng.permutation(np.concatenate([rng.integers(0, B * g.B2, 1000), rng.integers(B * g.B2, (B + 1) * g.B2, 6000)]))
    cells = np.array([[rng.integers(lo, hi) for lo, hi in DO.tile_box(g, t)] for t in tiles])
    p = edges[cells] + rng.uniform(0.25, 0.75, cells.shape) * (edges[cells + 1] - edges[cells])
    bucket, tile = _buckets(g, p, edges)
    assert np.array_equal(tile, tiles) and (B + 1) * g.B2 <= g.T
    cum = np.cumsum(np.bincount(bucket, minlength=g.B1))              # bucket b holds the sorted positions [cum[b - 1], cum[b])
    assert cum[0] > 0 and B * g.B2 >= DO.TABLE
    assert cum[B - 1] < DO.CHUNK - 100 and cum[B] > DO.CHUNK + 100 and cum[B] == cum[-1] == 7000 < 2 * DO.CHUNK
    ref = _check(monkeypatch, form, p, DO.dyadic_masses(rng, 7000), edges)
    assert ref.sum() > 3500


@pytest.mark.parametrize('with_mass', [True, False])
def test_level1_histograms_longer_than_one_scan_block(gpu, monkeypatch, with_mass):
    """N = 257, 3-D, 450 000 particles: 41 buckets x 110 chunks of per-workgroup histograms, more than the 4096 counts one block of
    exclusive_scan takes -- the block sums and the add-back pass decide every level-1 range"""
    rng = np.random.default_rng(450)
    N, n = 257, 450_000
    g = DO.geometry(3, N)
    assert g.B1 * -(-n // DO.CHUNK) + 1 > DO.SCAN_BLOCK and g.T > DO.TABLE
    edges = np.linspace(0.0, L, N + 1)
    p = rng.uniform(-0.005 * L, 1.005 * L, (n, 3))
    ref = _check(monkeypatch, 'tiled', p, DO.dyadic_masses(rng, n) if with_mass else None, edges)
    assert ref.sum() > 0.9 * n


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('with_mass', [True, False])
def test_edges_in_global_memory(gpu, monkeypatch, with_mass, form):
    """2-D, N = 2100: 2101 edges do not fit the LDS copy, few enough tiles for the LDS table; 200 000 particles, ~5 % outside"""
    rng = np.random.default_rng(2100)
    N, n = 2100, 200_000
    g = DO.geometry(2, N)
    edges = np.linspace(0.0, L, N + 1)
    assert edges.size > DO.EDGES_LDS and g.T <= DO.TABLE
    p = rng.uniform(-0.0125 * L, 1.0125 * L, (n, 2))
    p[:4] = [[0.0, L], [L, 0.0], [np.nextafter(L, np.inf), 1.0], [1.0, -1e-300]]
    ref = _check(monkeypatch, form, p, DO.dyadic_masses(rng, n) if with_mass else None, edges)
    assert 0.93 * n < np.count_nonzero(_buckets(g, p, edges)[0] >= 0) < 0.97 * n and ref[0, -1] > 0 and ref[-1, 0] > 0


# --------------------------------------------------------------------------------------------- histogram_bin on and around every edge
EDGE_CASES = [(ndim, N, kind) for ndim, Ns in ((3, (33, 100, 300)), (2, (300, 2100))) for N in Ns for kind in ('linspace', 'jitter')]
EDGE_CASES += [(3, 64, 'geomspace'), (2, 64, 'geomspace')]


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('ndim,N,kind', EDGE_CASES)
def test_every_edge_and_one_ulp_either_side(gpu, monkeypatch, ndim, N, kind, form):
    """a particle on every edge, on the doubles just below and above it, NaN, +-inf and -0.0, on every axis, plus 2000 random particles:
    uniform edges of a box length that fp64 does not hold, a jittered linspace, and geometric edges where the seed of the bin search is
    off by dozens of bins"""
    rng = np.random.default_rng(1000 * ndim + N)
    edges = DO.make_edges(kind, N, L, rng)
    p = DO.every_edge_particles(ndim, edges, rng, 2000)
    if kind == 'geomspace':                                           # the linear seed against the true bin
        v = p[-2000:, 0]
        v = v[(v > 0) & (v < L)]
        assert np.abs((v / L * N).astype(int) - DO.bins_of(v, edges)).max() > 20
    ref = _check(monkeypatch, form, p, DO.dyadic_masses(rng, p.shape[0]), edges)
    assert ref.sum() > 0


# --------------------------------------------------------------------------------------------- particle counts
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('n', [1, 255, 4095, 4096, 4097, 8192, 8193])
def test_particle_counts_around_the_chunk(gpu, monkeypatch, n, form):
    """one particle, less than a workgroup, one chunk of 4096 less one / exactly / plus one, two chunks and one more; masses, so that the
    1024-mass rounds of deposit_split end partway"""
    rng = np.random.default_rng(n)
    N = 48
    edges = np.linspace(0.0, L, N + 1)
    p = rng.uniform(-0.01 * L, 1.01 * L, (n, 3)) if n > 1 else np.array([[0.7 * L, L, 0.0]])
    ref = _check(monkeypatch, form, p, DO.dyadic_masses(rng, n), edges)
    assert ref.sum() > 0


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('where', ['above', 'nan'])
def test_no_particle_inside(gpu, monkeypatch, where, form):
    """5000 particles, none inside the edges: every level-2 workgroup returns at once and every cell is stored as zero"""
    rng = np.random.default_rng(5)
    N, n = 48, 5000
    edges = np.linspace(0.0, L, N + 1)
    if where == 'above':
        p = L * (1.0 + rng.uniform(1e-9, 0.5, (n, 3)))
        p[0] = np.nextafter(L, np.inf)
    else:
        p = rng.uniform(0.0, L, (n, 3))
        p[np.arange(n), np.arange(n) % 3] = np.nan
    for mass in (DO.dyadic_masses(rng, n), None):
        ref = _check(monkeypatch, form, p, mass, edges)
        assert not ref.any()


# --------------------------------------------------------------------------------------------- space-filling-curve order
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('with_mass', [True, False])
@pytest.mark.parametrize('ndim,N', [(3, 80), (2, 300)])
def test_curve_ordered_particles(gpu, monkeypatch, ndim, N, with_mass, form):
    """300 000 clustered particles sorted along a Z-curve of their cells, ~8 % of them then thrown outside the box where they stand:
    lds_hist_rank merges runs of equal bucket that start and end inside a wave, are cut by dropped particles and reach lane 63.
    Masses of both signs (dyadic: the sums stay exact)"""
    rng = np.random.default_rng(N)
    n = 300_000
    g = DO.geometry(ndim, N)
    edges = np.linspace(0.0, L, N + 1)
    centres = rng.uniform(0, L, (60, ndim))
    p = np.mod(centres[rng.integers(0, 60, n)] + rng.normal(0, 0.04 * L, (n, ndim)), L)
    p = p[DO.morton_order(np.stack([DO.bins_of(p[:, a], edges) for a in range(ndim)], axis=1))]
    out = np.nonzero(rng.uniform(size=n) < 0.08)[0]
    p[out, rng.integers(0, ndim, out.size)] = np.choose(rng.integers(0, 3, out.size), [L * (1 + rng.uniform(0.001, 1, out.size)),
                                                                                         -L * rng.uniform(0.001, 1, out.size), np.nan])
    bucket, tile = _buckets(g, p, edges)
    assert np.array_equal(np.nonzero(bucket < 0)[0], out) and len(np.unique(bucket)) == g.B1 + 1 > 4
    start, length, heads = DO.wave_runs(bucket)
    merged = (heads <= DO.RUN_HEADS_MAX) & (length >= 2) & (length < DO.WAVE)           # runs that take the merging branch, no whole waves
    assert len(np.unique(length[merged])) >= 40
    assert np.count_nonzero(merged & (start > 0) & (start + length == DO.WAVE)) > 100   # begin inside the wave, reach lane 63
    assert np.count_nonzero(merged & (start > 0) & (start + length < DO.WAVE)) > 100    # begin and end inside the wave
    assert np.count_nonzero(heads > DO.RUN_HEADS_MAX) < 0.01 * heads.size
    mass = None
    if with_mass:
        mass = DO.dyadic_masses(rng, n) * np.where(rng.uniform(size=n) < 0.3, -1.0, 1.0)
    ref = _check(monkeypatch, form, p, mass, edges)
    assert np.count_nonzero(ref) > 0.2 * ref.size


# --------------------------------------------------------------------------------------------- slabs
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('ndim,N,plane_lo,plane_n', [(3, 100, 37, 23), (3, 100, 99, 1), (3, 100, 0, 17), (2, 300, 64, 65)])
def test_slabs_that_are_no_multiple_of_the_tile(gpu, monkeypatch, ndim, N, plane_lo, plane_n, form):
    """planes [plane_lo, plane_lo + plane_n) with particles exactly on the slab's first edge (inside) and on its last edge (the next
    plane's, but the box face is inclusive), one ulp either side of both"""
    rng = np.random.default_rng(plane_lo + plane_n)
    n = 60_000
    edges = np.linspace(0.0, L, N + 1)
    lo, hi = edges[plane_lo], edges[plane_lo + plane_n]
    p = rng.uniform(-0.01 * L, 1.01 * L, (n, ndim))
    p[:1200, 0] = np.repeat([lo, np.nextafter(lo, -np.inf), np.nextafter(lo, np.inf), hi, np.nextafter(hi, -np.inf), np.nextafter(hi, np.inf)], 200)
    p[1200:1500, 0] = rng.uniform(lo, hi, 300)                         # (a thin slab still holds particles)
    mass = DO.dyadic_masses(rng, n)
    b0 = DO.bins_of(p[:1200:200, 0], edges)
    last = plane_lo + plane_n == N
    assert ((b0 >= plane_lo) & (b0 < plane_lo + plane_n)).tolist() == [True, False, True, last, True, False]
    ref = _check(monkeypatch, form, p, mass, edges, plane_lo, plane_n)
    assert ref.shape[0] == plane_n and ref[0].sum() > 0 and ref[-1].sum() > 0
    # the same slab cut out of the whole-grid oracle
    assert np.array_equal(ref, DO.histogramdd([p[:, a] for a in range(ndim)], mass, edges)[plane_lo:plane_lo + plane_n])


# --------------------------------------------------------------------------------------------- records at a stride
@pytest.mark.parametrize('with_mass', [True, False])
@pytest.mark.parametrize('ndim,N', [(3, 50), (2, 200)])
def test_strided_records_in_the_tiled_form(gpu, monkeypatch, ndim, N, with_mass):
    """bfgx_deposit_particles_records on 48-byte records with the fields in the order (mass, z, pad, x, pad, y), forced into the tiled
    form: deposit_keys and deposit_split<1> read at a stride of 6 doubles.  == the oracle, == the column entry bit for bit"""
    from baryonification_amd import _lib
    rng = np.random.default_rng(48 + ndim)
    n = 10_000
    edges = np.linspace(0.0, L, N + 1)
    rec = np.zeros(n, dtype=[('M', np.float64), ('z', np.float64), ('pad0', np.float64), ('x', np.float64), ('pad1', np.float64), ('y', np.float64)])
    assert rec.dtype.itemsize == 48 and [rec.dtype.fields[k][1] for k in ('M', 'z', 'x', 'y')] == [0, 8, 24, 40]
    p = rng.uniform(-0.01 * L, 1.01 * L, (n, 3))
    rec['x'], rec['y'], rec['z'], rec['M'] = p[:, 0], p[:, 1], p[:, 2], DO.dyadic_masses(rng, n)
    rec['pad0'] = rec['pad1'] = np.nan
    if ndim == 2:
        rec['z'] = np.nan                                              # (not read)
    if not with_mass:
        rec['M'] = np.nan                                              # (not read, not scanned for NaN either)
    monkeypatch.setenv('BFGX_DEPOSIT', 'tiled')
    out = np.full((N,) * ndim, np.nan)
    _lib.check(_lib.load().bfgx_deposit_particles_records(0, ndim, n, rec.ctypes.data, 48, 24, 40, 8 if ndim == 3 else 0, 0 if with_mass else -1, N,
                                                          edges.ctypes.data, out.ctypes.data))
    coords = [p[:, a].copy() for a in range(ndim)]
    mass = rec['M'].copy() if with_mass else None
    _same(out, DO.histogramdd(coords, mass, edges))
    cols = _deposit(monkeypatch, 'tiled', coords, mass, edges)
    assert out.tobytes() == cols.tobytes()


# --------------------------------------------------------------------------------------------- second copy and tile totals
@pytest.mark.parametrize('ndim,N', [(3, 61), (2, 250)])
def test_fused_entry_second_copy_and_tile_totals(gpu, monkeypatch, ndim, N):
    """grid_plan.deposit_baryonify with an empty catalogue, tiled form: deposit_tiles_kernel stores every cell to map_in and to map_out
    and leaves the tiles' totals, no halo moves anything: map_in == the oracle, map_out == map_in bit for bit, both sums == the exact
    total of the masses inside"""
    import torch
    from baryonification_amd import _lib, engine, synthetic as syn
    monkeypatch.setenv('BFGX_DEPOSIT', 'tiled')
    rng = np.random.default_rng(N)
    n = 150_000
    dev = torch.device('cuda:0')
    stream = torch.cuda.current_stream().cuda_stream
    z, Mt, r = np.array([0.25, 0.3, 0.35]), np.geomspace(10 ** 12.4, 10 ** 15.1, 8), np.geomspace(1e-3, 2e2, 200)
    model, keep = engine.model_from_tables([np.log(1 + z), np.log(Mt), np.log(r)], syn.displacement_table(z, Mt, r), dict(syn.COSMO, w0=-1.0), 6.0, 8.0)
    edges = np.linspace(0.0, L, N + 1)
    plan = engine.GridPlan(model, keep, 0.5 * (edges[1:] + edges[:-1]), ndim, 0.3, 1, 0, stream)
    try:
        empty = torch.empty(0, dtype=torch.float64, device=dev)
        dcat = _lib.make_grid_catalog_dev(0, empty.data_ptr(), empty.data_ptr(), empty.data_ptr(), empty.data_ptr() if ndim == 3 else 0, empty.data_ptr())
        p = rng.uniform(-0.01 * L, 1.01 * L, (n, 3))
        p[:3] = [[0.0] * 3, [L] * 3, [edges[7]] * 3]
        mass = DO.dyadic_masses(rng, n)
        cols, m, e = torch.from_numpy(np.ascontiguousarray(p.T)).to(dev), torch.from_numpy(mass).to(dev), torch.from_numpy(edges).to(dev)
        m_in, m_out = (torch.full((N,) * ndim, float('nan'), dtype=torch.float64, device=dev) for _ in range(2))
        sums = torch.zeros(2, dtype=torch.float64, device=dev)
        pairs = plan.deposit_baryonify(dcat, n, cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr() if ndim == 3 else 0, m.data_ptr(),
                                       e.data_ptr(), m_in.data_ptr(), m_out.data_ptr(), sums.data_ptr())
        torch.cuda.synchronize()
        ref = DO.histogramdd([p[:, a] for a in range(ndim)], mass, edges)
        a, b = m_in.cpu().numpy(), m_out.cpu().numpy()
        _same(a, ref)
        assert pairs == 0 and a.tobytes() == b.tobytes()
        inside = ((p[:, :ndim] >= 0) & (p[:, :ndim] <= L)).all(axis=1)
        total = float(np.sum((mass[inside] * 1024).astype(np.int64))) / 1024.0
        assert sums.cpu().numpy().tolist() == [total, total] and total == ref.sum()
    finally:
        plan.close()


# --------------------------------------------------------------------------------------------- generic masses
@pytest.mark.parametrize('form', FORMS)
def test_generic_masses_within_the_fp64_summation_bound(gpu, monkeypatch, form):
    """real masses of both signs: the cell's k particles are summed in some order on both sides, each sum within (k - 1) 2^-53 sum|m_i| of
    the exact one, so |got - ref| <= 2 (k - 1) 2^-53 sum|m_i| per cell; a cell with one particle is exact"""
    rng = np.random.default_rng(11)
    N, n = 33, 400_000
    edges = np.linspace(0.0, L, N + 1)
    p = rng.uniform(-0.01 * L, 1.01 * L, (n, 3))
    p[:40000] = 0.3 * L + rng.normal(0, 0.01 * L, (40000, 3))          # cells with thousands of particles
    mass = rng.uniform(0.5, 2.0, n) * np.where(rng.uniform(size=n) < 0.3, -1.0, 1.0)
    coords = [p[:, a] for a in range(3)]
    ref, k, s = DO.histogramdd(coords, mass, edges), DO.histogramdd(coords, None, edges), DO.histogramdd(coords, np.abs(mass), edges)
    bound = 2.0 * np.maximum(k - 1, 0) * 2.0 ** -53 * s
    got = _deposit(monkeypatch, form, coords, mass, edges)
    err = np.abs(got - ref)
    print('max err / bound = %.3g, largest k = %d' % (np.nanmax(err[k > 1] / bound[k > 1]), k.max()))
    assert k.max() > 1000 and np.isfinite(got).all() and (err <= bound).all()


# --------------------------------------------------------------------------------------------- routing
def _check_route(cols, edges, world):
    """route_particles_count_device, then -- only once owners and counts are the oracle's: the fill pass trusts them for its ranges --
    route_particles_fill_device; returns the counts"""
    import torch
    from baryonification_amd import engine
    dev = torch.device('cuda:0')
    ncols, n = cols.shape
    N = edges.size - 1
    want = DO.owners(cols[0], edges, world)
    want_counts = np.bincount(want[want != DO.ROUTE_DROPPED], minlength=world)
    d_cols = torch.from_numpy(np.ascontiguousarray(cols)).to(dev)
    d_edges = torch.from_numpy(edges).to(dev)
    owner = torch.full((max(n, 1),), 77, dtype=torch.uint8, device=dev)
    counts = torch.full((world,), -5, dtype=torch.int32, device=dev)
    engine.route_particles_count_device(d_cols[0].data_ptr() if n else 0, n, N, d_edges.data_ptr(), world, owner.data_ptr() if n else 0, counts.data_ptr())
    assert np.array_equal(owner.cpu().numpy()[:n], want)
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    total = int(want_counts.sum())
    start = np.concatenate([[0], np.cumsum(want_counts)[:-1]])
    packed = torch.full((ncols, max(total, 1)), float('nan'), dtype=torch.float64, device=dev)
    cursor = torch.full((world,), -5, dtype=torch.int32, device=dev)
    engine.route_particles_fill_device([d_cols[i].data_ptr() if n else 0 for i in range(ncols)], n, owner.data_ptr() if n else 0, world, start, total,
                                       cursor.data_ptr(), packed.data_ptr() if total else 0)
    torch.cuda.synchronize()
    got = packed.cpu().numpy()[:, :total]
    assert not np.isnan(got).any()
    assert np.array_equal(cursor.cpu().numpy(), want_counts)          # every destination's range filled to its end
    for d in range(world):
        sel = cols[:, want == d]
        blk = got[:, start[d]:start[d] + want_counts[d]]
        assert np.array_equal(blk[:, np.lexsort(blk[::-1])], sel[:, np.lexsort(sel[::-1])])          # the same particles, column by column
    return want_counts


@pytest.mark.parametrize('kind', ['linspace', 'jitter'])
@pytest.mark.parametrize('n', [1, 200, 100_000])
@pytest.mark.parametrize('world,N', [(255, 255), (255, 2295), (3, 96), (7, 49)])
def test_routing_many_and_odd_rank_counts(gpu, world, N, n, kind):
    """owners and counts == the oracle exactly, every destination receives exactly its particles: 255 ranks of one and of nine planes
    (2296 edges: read from global memory), 3 and 7 ranks; one particle, less than a workgroup, many; a particle on every rank boundary
    and one ulp either side, NaN, +-inf, -0.0"""
    rng = np.random.default_rng(world * N + n)
    edges = DO.make_edges(kind, N, L, rng)
    assert (edges.size > DO.EDGES_LDS) == (N == 2295)
    bnd = edges[::N // world]
    special = rng.permutation(np.concatenate([bnd, np.nextafter(bnd, -np.inf), np.nextafter(bnd, np.inf), [np.nan, np.inf, -np.inf, -0.0]]))
    cols = rng.uniform(-0.02 * L, 1.02 * L, (3, n))
    k = min(n, special.size)
    cols[0, :k] = special[:k] if n > 1 else bnd[world - 1]              # (one particle: on the last rank's first edge)
    cols[0] = rng.permutation(cols[0])
    counts = _check_route(cols, edges, world)
    assert counts.sum() > 0 and (n < 100_000 or (counts > 0).all())


@pytest.mark.parametrize('world,N', [(255, 2295), (7, 49)])
def test_routing_nothing_to_route(gpu, world, N):
    """every particle outside the edges (total = 0: the fill pass has nothing to write) and no particle at all"""
    rng = np.random.default_rng(world)
    edges = DO.make_edges('jitter', N, L, rng)
    cols = rng.uniform(0, L, (3, 5000))
    cols[0] = np.choose(np.arange(5000) % 3, [L * (1 + rng.uniform(1e-9, 1, 5000)), -L * rng.uniform(1e-300, 1, 5000), np.nan])
    cols[0, 0], cols[0, 1] = np.nextafter(L, np.inf), np.nextafter(0.0, -np.inf)
    assert not _check_route(cols, edges, world).any()
    assert not _check_route(np.zeros((3, 0)), edges, world).any()
