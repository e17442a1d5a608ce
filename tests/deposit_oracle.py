"""Plain-numpy oracle of the particle deposit and the slab routing (csrc/bfgx_deposit.hpp): np.histogramdd's bin rule restated with
searchsorted + bincount, the owner of a particle's first-axis bin, and -- only to BUILD inputs and to assert that an input reaches the
branch it was built for -- a restatement of the tile geometry of the two-level counting sort.  No project code, no GPU.
test_deposit_oracle_host.py checks it against np.histogramdd itself and against hand-computed geometry rows."""
import collections

import numpy as np

# restated from csrc/bfgx_deposit.hpp (test_deposit_oracle_host.py compares them with the header's text)
TILE_SHAPE = {3: (16, 16, 32), 2: (64, 128)}          # cells per tile; the last axis runs fastest
CHUNK = 4096                                          # kDepChunk: keys per workgroup of a sort pass
TABLE = 2048                                          # kDepHist: buckets a sort pass ranks in LDS, counted from the chunk's first bucket
EDGES_LDS = 2049                                      # kDepEdgesLds: edges staged in LDS up to this many; beyond, read from global memory
SCAN_BLOCK = 4096                                     # kScanPerBlock: counts per block of exclusive_scan (bfgx_scan.hpp)
WAVE = 64
RUN_HEADS_MAX = 40                                    # lds_hist_rank merges runs when a wave holds at most this many run heads
ROUTE_DROPPED = 255


def make_edges(kind, N, L, rng):
    """N + 1 strictly ascending edges from exactly 0 to exactly L: 'linspace'; 'jitter' (inner edges moved by up to 0.3 cells); 'geomspace'
    (cell widths growing by a constant factor, 1e4 overall: a linear guess of the bin is wrong by many bins)"""
    if kind == 'linspace':
        e = np.linspace(0.0, L, N + 1)
    elif kind == 'jitter':
        e = np.linspace(0.0, L, N + 1)
        e[1:-1] += rng.uniform(-0.3, 0.3, N - 1) * (L / N)
    else:
        e = L * (np.geomspace(1.0, 1.0e4, N + 1) - 1.0) / (1.0e4 - 1.0)
    e[0], e[-1] = 0.0, L
    assert np.all(np.diff(e) > 0)
    return e


def every_edge_particles(ndim, edges, rng, extra):
    """[n, ndim]: every edge, one ulp below and above it, NaN, +-inf and -0.0 on every axis in turn (the other axes random interior values),
    then `extra` random particles, some outside"""
    L = edges[-1]
    special = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf), [np.nan, np.inf, -np.inf, -0.0]])
    rows = []
    for a in range(ndim):
        p = rng.uniform(0.01 * L, 0.99 * L, (special.size, ndim))
        p[:, a] = special
        rows.append(p)
    rows.append(rng.uniform(-0.03 * L, 1.03 * L, (extra, ndim)))
    return np.concatenate(rows, axis=0)


def dyadic_masses(rng, n):
    """k / 1024 with 512 <= k < 2048: sums of millions of them are exact in fp64, so every order of addition gives the same map"""
    return rng.integers(512, 2048, n) / 1024.0


def bins_of(v, edges):
    """np.histogramdd's bin of every value of one column: edges[b] <= v < edges[b + 1], the last edge inclusive; -1: dropped
    (below, above, NaN, +-inf)"""
    v, edges = np.asarray(v, dtype=np.float64), np.asarray(edges, dtype=np.float64)
    nb = edges.size - 1
    b = np.searchsorted(edges, v, side='right').astype(np.int64) - 1            # (NaN sorts past the end: nb)
    b[v == edges[-1]] = nb - 1
    b[(b < 0) | (b >= nb) | np.isnan(v)] = -1
    return b


def histogramdd(coords, weights, edges, plane_lo=0, plane_n=None):
    """np.histogramdd(coords, bins=(edges,) * ndim, weights=weights), the planes [plane_lo, plane_lo + plane_n) of the first axis;
    weights=None counts"""
    edges = np.asarray(edges, dtype=np.float64)
    nb, ndim = edges.size - 1, len(coords)
    plane_n = nb - plane_lo if plane_n is None else plane_n
    b = [bins_of(c, edges) for c in coords]
    keep = np.ones(b[0].shape, dtype=bool)
    for q in b:
        keep &= q >= 0
    keep &= (b[0] >= plane_lo) & (b[0] < plane_lo + plane_n)
    flat = b[0][keep] - plane_lo
    for q in b[1:]:
        flat = flat * nb + q[keep]
    shape = (plane_n,) + (nb,) * (ndim - 1)
    w = None if weights is None else np.asarray(weights, dtype=np.float64)[keep]
    return np.bincount(flat, weights=w, minlength=int(np.prod(shape))).astype(np.float64).reshape(shape)


def owners(x, edges, world):
    """rank that owns the plane of every particle's first-axis bin, N // world planes per rank; ROUTE_DROPPED outside the edges"""
    nb = np.asarray(edges).size - 1
    assert nb % world == 0
    b = bins_of(x, edges)
    return np.where(b >= 0, b // (nb // world), ROUTE_DROPPED).astype(np.uint8)


Geometry = collections.namedtuple('Geometry', 'ndim N plane_n shape ntiles T B1 B2')


def geometry(ndim, N, plane_n=None):
    """dep_geom restated: tiles per axis, T tiles, level-1 buckets of B2 consecutive tiles (B2 the smallest power of two with B2^2 >= T),
    B1 = ceil(T / B2) of them"""
    plane_n = N if plane_n is None else plane_n
    shape = TILE_SHAPE[ndim]
    extent = (plane_n,) + (N,) * (ndim - 1)
    ntiles = tuple(-(-e // s) for e, s in zip(extent, shape))
    T = int(np.prod(ntiles))
    B2 = 1
    while B2 * B2 < T:
        B2 *= 2
    return Geometry(ndim, N, plane_n, shape, ntiles, T, -(-T // B2), B2)


def tile_of(g, cells):
    """tile index of cells [n, ndim] (first axis counted from the slab's first plane): tiles in row-major order"""
    cells = np.asarray(cells, dtype=np.int64)
    t = cells[:, 0] // g.shape[0]
    for a in range(1, g.ndim):
        t = t * g.ntiles[a] + cells[:, a] // g.shape[a]
    return t


def tile_box(g, tile):
    """(lo, hi) cell ranges per axis of one tile, clipped to the grid"""
    idx = np.unravel_index(int(tile), g.ntiles)
    extent = (g.plane_n,) + (g.N,) * (g.ndim - 1)
    return [(int(i) * s, min((int(i) + 1) * s, e)) for i, s, e in zip(idx, g.shape, extent)]


def buckets_of(g, coords, edges, plane_lo=0):
    """level-1 bucket (tile // B2) and tile of every particle; -1 for a particle the deposit drops"""
    b = np.stack([bins_of(c, edges) for c in coords], axis=1)
    b[:, 0] -= plane_lo
    keep = (b >= 0).all(axis=1) & (b[:, 0] < g.plane_n)
    tile = np.where(keep, tile_of(g, np.where(keep[:, None], b, 0)), -1)
    return np.where(keep, tile // g.B2, -1), tile


def morton_order(cells):
    """permutation that sorts particles along a Z-curve of their cells [n, ndim] (stable: particles of one cell keep their order)"""
    cells = np.asarray(cells, dtype=np.uint64)
    n, ndim = cells.shape
    code = np.zeros(n, dtype=np.uint64)
    for bit in range(int(cells.max()).bit_length() if n else 0):
        for a in range(ndim):
            code |= ((cells[:, a] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(bit * ndim + (ndim - 1 - a))
    return np.argsort(code, kind='stable')


def wave_runs(bucket):
    """runs of equal level-1 bucket inside the 64-lane waves of the key pass, as lds_hist_rank sees them (a dropped particle, bucket -1, is
    a run of its own): arrays (start lane, length, heads in the run's wave) of the runs of kept particles"""
    bucket = np.asarray(bucket, dtype=np.int64)
    n = bucket.size
    pad = (-n) % WAVE
    key = np.concatenate([bucket, np.full(pad, -1, dtype=np.int64)]).reshape(-1, WAVE)
    lane = np.arange(WAVE)
    head = np.ones(key.shape, dtype=bool)
    head[:, 1:] = (key[:, 1:] != key[:, :-1]) | (key[:, 1:] < 0)
    heads = head.sum(axis=1)
    starts, lengths, nheads = [], [], []
    for w in range(key.shape[0]):
        h = lane[head[w]]
        ln = np.diff(np.concatenate([h, [WAVE]]))
        act = key[w, h] >= 0
        starts.append(h[act]); lengths.append(ln[act]); nheads.append(np.full(int(act.sum()), heads[w]))
    return np.concatenate(starts), np.concatenate(lengths), np.concatenate(nheads)
