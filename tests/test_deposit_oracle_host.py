"""deposit_oracle.py against np.histogramdd itself and against hand-computed rows of the tile geometry; the constants it restates
against the text of csrc/bfgx_deposit.hpp (a change of tile shape, chunk or table size must be followed here, or the branch assertions of
test_gpu_deposit_kernels.py would reason about another kernel).  No GPU."""
import os
import re

import numpy as np
import pytest

import deposit_oracle as DO

L = 250.0 / 3.0                                       # not representable in fp64


@pytest.mark.parametrize('kind', ['linspace', 'jitter', 'geomspace'])
@pytest.mark.parametrize('ndim,N', [(2, 7), (2, 100), (3, 5), (3, 33)])
def test_histogramdd_is_numpys(ndim, N, kind):
    rng = np.random.default_rng(100 * ndim + N)
    edges = DO.make_edges(kind, N, L, rng)
    assert np.all(np.diff(edges) > 0) and edges[0] == 0.0 and edges[-1] == L and edges.size == N + 1
    assert (kind == 'linspace') == bool(np.allclose(np.diff(edges), L / N, rtol=1e-9))
    p = DO.every_edge_particles(ndim, edges, rng, 500)
    assert p.shape == (ndim * (3 * (N + 1) + 4) + 500, ndim)
    w = DO.dyadic_masses(rng, p.shape[0])
    fin = np.isfinite(p).all(axis=1)                                  # (np.histogramdd refuses non-finite samples: they are dropped by hand)
    assert np.count_nonzero(~fin) == 3 * ndim
    ref_w, _ = np.histogramdd(p[fin], bins=(edges,) * ndim, weights=w[fin])
    ref_c, _ = np.histogramdd(p[fin], bins=(edges,) * ndim)
    cols = [p[:, a] for a in range(ndim)]
    got_w, got_c = DO.histogramdd(cols, w, edges), DO.histogramdd(cols, None, edges)
    assert got_w.shape == (N,) * ndim and got_w.dtype == np.float64
    assert np.array_equal(got_w, ref_w) and np.array_equal(got_c, ref_c)          # dyadic weights: every order of addition gives the same sum
    assert 0 < got_c.sum() < p.shape[0]
    # -0.0 lies in bin 0, the last edge in the last bin, one ulp outside either end is dropped
    assert np.array_equal(DO.bins_of([-0.0, 0.0, L, np.nextafter(L, np.inf), np.nextafter(0.0, -np.inf), np.nan, np.inf, -np.inf], edges),
                          [0, 0, N - 1, -1, -1, -1, -1, -1])
    # slabs are slices of the full result
    for lo, n in [(0, N), (0, 1), (N - 1, 1), (N // 3, N - N // 3 - 1), (1, 2)]:
        assert np.array_equal(DO.histogramdd(cols, w, edges, lo, n), ref_w[lo:lo + n])
        assert np.array_equal(DO.histogramdd(cols, None, edges, lo, n), ref_c[lo:lo + n])


@pytest.mark.parametrize('world,N', [(1, 5), (3, 96), (7, 49), (255, 255), (255, 2295)])
def test_owners_follow_their_definition(world, N):
    rng = np.random.default_rng(world + N)
    edges = DO.make_edges('jitter', N, L, rng)
    cnt = N // world
    x = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf), [np.nan, np.inf, -np.inf, -0.0], rng.uniform(-1.0, L + 1.0, 3000)])
    own = DO.owners(x, edges, world)
    assert own.dtype == np.uint8
    with np.errstate(invalid='ignore'):
        inside = (x >= edges[0]) & (x <= edges[-1])
        b = np.minimum((edges[None, :-1] <= x[:, None]).sum(axis=1) - 1, N - 1)          # the definition: the last lower edge not above x
    assert np.array_equal(own, np.where(inside, b // cnt, 255))
    kept = own[own != 255]
    assert kept.max() == world - 1 and kept.min() == 0 and np.count_nonzero(own == 255) >= 5


@pytest.mark.parametrize('ndim,N,plane_n,ntiles,T,B1,B2', [
    (3, 257, None, (17, 17, 9), 2601, 41, 64), (2, 4160, None, (65, 33), 2145, 34, 64), (2, 2100, None, (33, 17), 561, 18, 32),
    (3, 128, None, (8, 8, 4), 256, 16, 16), (3, 100, 23, (2, 7, 4), 56, 7, 8), (3, 100, 1, (1, 7, 4), 28, 4, 8), (2, 300, 65, (2, 3), 6, 2, 4),
    (3, 48, None, (3, 3, 2), 18, 3, 8), (3, 1, None, (1, 1, 1), 1, 1, 1)])
def test_geometry_rows(ndim, N, plane_n, ntiles, T, B1, B2):
    g = DO.geometry(ndim, N, plane_n)
    assert (g.ntiles, g.T, g.B1, g.B2) == (ntiles, T, B1, B2)
    assert g.B2 * g.B2 >= g.T and (g.B2 == 1 or (g.B2 // 2) ** 2 < g.T) and g.B1 * g.B2 >= g.T > (g.B1 - 1) * g.B2
    # tile_of: row-major over the tiles, every cell of tile_box(t) names t, the boxes partition the grid
    extent = (g.plane_n,) + (g.N,) * (ndim - 1)
    corner = np.array([[e - 1 for e in extent], [0] * ndim])
    assert np.array_equal(DO.tile_of(g, corner), [T - 1, 0])
    cells = 0
    for t in sorted({0, min(1, T - 1), T // 2, T - 1}):
        box = DO.tile_box(g, t)
        assert all(0 <= lo < hi <= e for (lo, hi), e in zip(box, extent))
        grid = np.stack(np.meshgrid(*[np.arange(lo, hi) for lo, hi in box], indexing='ij'), axis=-1).reshape(-1, ndim)
        assert np.all(DO.tile_of(g, grid) == t)
    for t in range(T):
        cells += int(np.prod([hi - lo for lo, hi in DO.tile_box(g, t)]))
    assert cells == int(np.prod(extent))


def test_tile_of_hand_rows():
    g = DO.geometry(3, 257)
    assert np.array_equal(DO.tile_of(g, [[0, 0, 31], [0, 0, 32], [0, 16, 0], [16, 0, 0], [256, 256, 256], [223, 100, 77]]),
                          [0, 1, 9, 153, 2600, (13 * 17 + 6) * 9 + 2])
    g = DO.geometry(2, 4160)
    assert np.array_equal(DO.tile_of(g, [[63, 127], [63, 128], [64, 0], [4159, 4159]]), [0, 1, 33, 2144])


def test_buckets_and_morton_order():
    rng = np.random.default_rng(3)
    g = DO.geometry(3, 80)
    edges = np.linspace(0.0, L, 81)
    p = rng.uniform(-0.02 * L, 1.02 * L, (5000, 3))
    bucket, tile = DO.buckets_of(g, [p[:, 0], p[:, 1], p[:, 2]], edges)
    inside = ((p >= 0) & (p <= L)).all(axis=1)
    assert np.array_equal(bucket >= 0, inside) and np.array_equal(tile >= 0, inside)
    assert np.array_equal(bucket[inside], tile[inside] // g.B2) and tile.max() < g.T
    # Z-curve: a permutation; in 2-D the first 4^k cells of the curve fill the 2^k square
    cells = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing='ij'), axis=-1).reshape(-1, 2)
    order = DO.morton_order(cells)
    assert np.array_equal(np.sort(order), np.arange(64))
    assert np.array_equal(cells[order][:4], [[0, 0], [0, 1], [1, 0], [1, 1]])
    for k in (1, 2, 3):
        assert cells[order][:4 ** k].max() == 2 ** k - 1
    c3 = rng.integers(0, 80, (1000, 3))
    o3 = DO.morton_order(c3)
    assert np.array_equal(np.sort(o3), np.arange(1000))
    low = np.count_nonzero((c3 < 64).all(axis=1))                     # the 64^3 cube comes first on the curve, whole
    assert (c3[o3][:low] < 64).all() and (c3[o3][low:] >= 64).any(axis=1).all()


def test_wave_runs_hand_case():
    b = np.full(130, 5)
    b[3] = -1                                     # a dropped particle splits a run
    b[10:20] = 6
    b[60:70] = 7                                  # reaches lane 63 of wave 0 and goes on in wave 1
    start, length, heads = DO.wave_runs(b)
    w0 = [(0, 3), (4, 6), (10, 10), (20, 40), (60, 4)]
    w1 = [(0, 6), (6, 58)]
    w2 = [(0, 2)]
    assert list(zip(start.tolist(), length.tolist())) == w0 + w1 + w2
    assert heads.tolist() == [6] * 5 + [2] * 2 + [63] * 1          # (the 62 lanes past the end are dropped: one head each)


def test_constants_are_the_headers():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'baryonification_amd', 'csrc', 'bfgx_deposit.hpp')
    src = open(path).read()

    def const(name):
        return int(eval(re.search(r'constexpr int %s = ([0-9 <]+);' % name, src).group(1)))
    assert const('kDepLocalBits') == 13
    assert const('kDepChunk') == DO.CHUNK and const('kDepHist') == DO.TABLE and const('kDepEdgesLds') == DO.EDGES_LDS
    shapes = re.findall(r'g\.sx = (\d+); g\.sy = (\d+); g\.sz = (\d+);', src)
    assert [tuple(int(v) for v in s) for s in shapes] == [DO.TILE_SHAPE[3], DO.TILE_SHAPE[2] + (1,)]
    assert int(re.search(r'__popcll\(hm\) > (\d+)', src).group(1)) == DO.RUN_HEADS_MAX
    assert int(re.search(r'kRouteDropped = (\d+);', src).group(1)) == DO.ROUTE_DROPPED
    csrc = os.path.dirname(os.path.abspath(path))
    threads = int(re.search(r'constexpr int kTabThreads = (\d+);', open(os.path.join(csrc, 'bfgx_tables.hpp')).read()).group(1))
    per = int(re.search(r'constexpr int kScanPerBlock = (\d+) \* kTabThreads;', open(os.path.join(csrc, 'bfgx_scan.hpp')).read()).group(1))
    assert per * threads == DO.SCAN_BLOCK
    for s in DO.TILE_SHAPE.values():
        assert int(np.prod(s)) == 1 << 13
