"""numpy restatements for the map statistics (baryonification_amd.utils.mapstats, get_all_neighbours, the harmonic windows):

  neighbours      healpix_cxx neighbors() over hpx_oracle's xyf functions: step (dx, dy) in the face, and across an edge or corner the
                  face table and the mirror / swap of (x, y); healpy's order SW, W, NW, N, NE, E, SE, S, -1 where there is none
  moments         two passes in extended precision: mean = fsum / n, central = longdouble mean of the products; also the mean absolute
                  value of every summed term, which is what the tolerance of the GPU test is stated in
  peaks           strict local maxima / minima over `neighbours`, eligible only where the pixel and all its existing neighbours are good
  tophat_window   (P_{l-1} - P_{l+1}) / ((2l + 1) (1 - cos r)) with mpmath's Legendre polynomials at 50 digits
"""
import itertools
import math

import numpy as np

import hpx_oracle as H

UNSEEN = H.UNSEEN
XOFF = np.array([-1, -1, 0, 1, 1, 1, 0, -1])
YOFF = np.array([0, 1, 1, 1, 0, -1, -1, -1])
# rows: where the step leaves the face, 4 + (x: -1 under, +1 over) + 3 (the same for y); columns: the base face
FACE = np.array([[8, 9, 10, 11, -1, -1, -1, -1, 10, 11, 8, 9],
                 [5, 6, 7, 4, 8, 9, 10, 11, 9, 10, 11, 8],
                 [-1, -1, -1, -1, 5, 6, 7, 4, -1, -1, -1, -1],
                 [4, 5, 6, 7, 11, 8, 9, 10, 11, 8, 9, 10],
                 [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11],
                 [1, 2, 3, 0, 0, 1, 2, 3, 5, 6, 7, 4],
                 [-1, -1, -1, -1, 7, 4, 5, 6, -1, -1, -1, -1],
                 [3, 0, 1, 2, 3, 0, 1, 2, 4, 5, 6, 7],
                 [2, 3, 0, 1, -1, -1, -1, -1, 0, 1, 2, 3]], dtype=np.int64)
# bit 0: mirror x, bit 1: mirror y, bit 2: swap; columns: north, equatorial, south faces
SWAP = np.array([[0, 0, 3], [0, 0, 6], [0, 0, 0], [0, 0, 5], [0, 0, 0], [5, 0, 0], [0, 0, 0], [6, 0, 0], [3, 0, 0]], dtype=np.int64)


def neighbours(nside, pix, nest=False):
    """(8,) for one index, (8, N) for N"""
    p = np.asarray(pix, dtype=np.int64)
    q = np.atleast_1d(p)
    ix, iy, f = H.nest2xyf(nside, q) if nest else H.ring2xyf(nside, q)
    out = np.empty((8, q.size), dtype=np.int64)
    for k in range(8):
        x, y = ix + XOFF[k], iy + YOFF[k]
        nb = 4 + np.where(x < 0, -1, np.where(x >= nside, 1, 0)) + 3 * np.where(y < 0, -1, np.where(y >= nside, 1, 0))
        x, y = x % nside, y % nside
        nf = FACE[nb, f]
        bits = SWAP[nb, f >> 2]
        x = np.where(bits & 1, nside - 1 - x, x)
        y = np.where(bits & 2, nside - 1 - y, y)
        x, y = np.where(bits & 4, y, x), np.where(bits & 4, x, y)
        ok = nf >= 0
        nfc = np.where(ok, nf, 0)
        r = H.xyf2nest(nside, x, y, nfc) if nest else H.xyf2ring(nside, x, y, nfc)
        out[k] = np.where(ok, r, -1)
    return out[:, 0] if p.ndim == 0 else out


def good(maps, mask=None):
    X = np.atleast_2d(np.asarray(maps, dtype=np.float64))
    g = H.good(X).all(0)
    return g if mask is None else g & (np.asarray(mask) != 0)


def exponents(K, order=4):
    """every tuple with 2 <= sum <= order (in no particular order: the results are keyed by the tuple)"""
    return [e for e in itertools.product(range(order + 1), repeat=K) if 2 <= sum(e) <= order]


def moments(maps, order=4, mask=None):
    """n, mean [K], central {tuple: value}, and scale: {'mean': [K], tuple: value} = the mean |summed term| of each"""
    X = np.atleast_2d(np.asarray(maps, dtype=np.float64))
    K = X.shape[0]
    g = good(X, mask)
    n = int(g.sum())
    exps = exponents(K, order)
    if n == 0:
        nan = float('nan')
        return 0, np.full(K, nan), {e: nan for e in exps}, {'mean': np.full(K, nan), **{e: nan for e in exps}}
    Xg = X[:, g]
    mean = np.array([np.longdouble(math.fsum(Xg[a])) / n for a in range(K)], dtype=np.longdouble)
    d = Xg.astype(np.longdouble) - mean[:, None]
    central, scale = {}, {'mean': np.abs(Xg).mean(1)}
    for e in exps:
        term = np.ones(n, dtype=np.longdouble)
        for a in range(K):
            term = term * d[a] ** e[a]
        central[e] = float(term.sum() / n)
        scale[e] = float(np.abs(term).sum() / n)
    return n, mean.astype(np.float64), central, scale


def peaks(m, edges, mask=None, nest=False):
    """({'maxima': int64 [nb], 'minima': int64 [nb]}, flags int8 [npix])"""
    m = np.asarray(m, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    nside = int(round(np.sqrt(m.size / 12)))
    nb = neighbours(nside, np.arange(m.size), nest)
    exists = nb >= 0
    idx = np.where(exists, nb, 0)
    g = good(m, mask)
    elig = g & (g[idx] | ~exists).all(0)
    with np.errstate(invalid='ignore'):
        gt = ((m[None, :] > m[idx]) | ~exists).all(0)
        lt = ((m[None, :] < m[idx]) | ~exists).all(0)
    flags = np.where(elig & gt, 1, np.where(elig & lt, -1, 0)).astype(np.int8)
    out = {}
    for name, sign in (('maxima', 1), ('minima', -1)):
        v = m[flags == sign]
        b = np.searchsorted(edges, v, side='right') - 1                  # edges[b] <= v < edges[b + 1]
        b = b[(b >= 0) & (b < edges.size - 1)]
        out[name] = np.bincount(b, minlength=edges.size - 1).astype(np.int64)
    return out, flags


def tophat_window(radius, lmax):
    import mpmath
    with mpmath.workdps(50):
        mu = mpmath.cos(mpmath.mpf(radius))
        P = [mpmath.legendre(l, mu) for l in range(lmax + 2)]
        return np.array([1.0] + [float((P[l - 1] - P[l + 1]) / ((2 * l + 1) * (1 - mu))) for l in range(1, lmax + 1)])
