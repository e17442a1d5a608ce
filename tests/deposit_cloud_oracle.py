"""Plain-numpy oracle of the CIC / TSC mass assignment (csrc/bfgx_deposit_cloud.hpp), following the definition literally in fp64.  No
project code, no GPU.  test_deposit_cloud_oracle_host.py checks it against hand-computed cases.

Grid of N cells per axis on [0, L], cell centres at (i + 1/2) L / N, s = N / L computed once.  Per axis, for a coordinate v:
  dropped   any coordinate not in [0, L] (below, above, NaN, +-inf) drops the particle whole, as np.histogramdd does; v == L and -0.0 are inside
  CIC (2)   u = v s - 0.5, i = floor(u), f = u - i: cell i mod N gets 1 - f, cell (i + 1) mod N gets f (i = -1 for u < 0: the cloud wraps)
  TSC (3)   i = min(floor(v s), N - 1), d = v s - i - 0.5: cells (i - 1) mod N, i, (i + 1) mod N get 0.5 (0.5 - d)^2, 0.75 - d^2, 0.5 (0.5 + d)^2
The particle adds ((wx wy) wz) m to each of its 2^dim / 3^dim cells (m = 1 without masses); coincident cells (N = 1, 2) add."""
import numpy as np

ORDERS = {'cic': 2, 'tsc': 3}


def inside(v, L):
    """which values of one column np.histogramdd keeps on [0, L]"""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return (v >= 0.0) & (v <= L)


def base_cell(v, N, L, order):
    """the cell a particle is sorted by, per value of one column: CIC i mod N, TSC i (dropped values: whatever 0.0 gives)"""
    v = np.asarray(v, dtype=np.float64)
    t = np.where(inside(v, L), v, 0.0) * (N / L)
    if order == 2:
        return np.floor(t - 0.5).astype(np.int64) % N
    return np.minimum(np.floor(t), N - 1).astype(np.int64)


def weights(v, N, L, order):
    """(keep [n], cells [n, order] wrapped into 0 .. N - 1, w [n, order]) of one column"""
    assert order in (2, 3)
    v = np.asarray(v, dtype=np.float64)
    s = N / L
    keep = inside(v, L)
    t = np.where(keep, v, 0.0) * s
    if order == 2:
        u = t - 0.5
        fl = np.floor(u)
        f = u - fl
        i = fl.astype(np.int64)
        cells = np.stack([i % N, (i + 1) % N], axis=1)
        w = np.stack([1.0 - f, f], axis=1)
    else:
        fl = np.minimum(np.floor(t), N - 1)
        d = t - fl - 0.5
        a, b = 0.5 - d, 0.5 + d
        i = fl.astype(np.int64)
        cells = np.stack([(i - 1) % N, i % N, (i + 1) % N], axis=1)
        w = np.stack([0.5 * (a * a), 0.75 - d * d, 0.5 * (b * b)], axis=1)
    return keep, cells, w


def deposit(coords, mass, N, L, order, unit_weights=False, widen=0):
    """the map [N] * ndim of the particles coords (a list of ndim columns); mass None: unit masses.  unit_weights: every cloud cell
    gets m instead of m w (counts of contributions, or sums of |m| over the particles that touch a cell); with it, widen = 1 takes the
    cloud one cell wider on both sides of every axis: the cells a particle can reach when its base cell comes out one off"""
    assert unit_weights or not widen
    ndim = len(coords)
    n = np.asarray(coords[0]).size
    per = [weights(c, N, L, order) for c in coords]
    keep = np.ones(n, dtype=bool)
    for k, _, _ in per:
        keep &= k
    m = np.ones(n) if mass is None else np.asarray(mass, dtype=np.float64)
    m = m[keep]
    out = np.zeros(N ** ndim)
    offsets = np.stack(np.meshgrid(*([np.arange(-widen, order + widen)] * ndim), indexing='ij'), axis=-1).reshape(-1, ndim)
    for off in offsets:
        flat = np.zeros(m.size, dtype=np.int64)
        w = None
        for a in range(ndim):
            if unit_weights:
                flat = flat * N + (per[a][1][keep, 0] + off[a]) % N
                continue
            flat = flat * N + per[a][1][keep, off[a]]
            wa = per[a][2][keep, off[a]]
            w = wa if w is None else w * wa
        val = m.copy() if unit_weights else w * m
        out += np.bincount(flat, weights=val, minlength=out.size)
    return out.reshape((N,) * ndim)


def kept(coords, L):
    keep = np.ones(np.asarray(coords[0]).size, dtype=bool)
    for c in coords:
        keep &= inside(c, L)
    return keep
