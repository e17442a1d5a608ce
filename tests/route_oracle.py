"""numpy reference for the halo routing of a spatially sharded multi-GPU step (bfgx_disc_rings_device, bfgx_route_*_device):

  true_ring_ranges   the rings a halo REALLY touches: the pixels of oracle.query_disc(nside, vec, R eps / D_A) (HealpixRunner.py:306), or the four
                     pixels of get_interp_weights when the disc is empty, turned into ring numbers with the refshim ring layout
                     (oracle/refshim/healpy._pix2ring, as tests/hpx_oracle.py uses it).  Also the range of everything BaryonifyShell can touch:
                     the disc's pixels and, for discs of fewer than 4 pixels (HealpixRunner.py:309-310), the four fallback pixels.
  widen              a ring range widened by a margin and clipped to [1, 4 nside - 1]; empty ranges stay (1, 0)
  destinations       the rule of include/bfgx.h: halo -> rank j iff first <= last and bounds[j] <= last and bounds[j + 1] > first
  expected_blocks    the halo numbers every destination receives
  block_position     where a destination's block sits in a buffer that leaves one rank out
  ring_colatitudes   colatitude of every ring (for the rows a test may set aside: a disc edge on a ring)

Nothing here restates the kernels' arithmetic (ring_above and the widening): the ranges come from pixel lists.
"""
import numpy as np

from hpx_oracle import hp
from oracle import oracle as O

EMPTY = (1, 0)                      # the range of a halo that touches nothing


_CAP = float(np.degrees(np.arcsin(2.0 / 3.0)))       # latitude of the boundary between a polar cap and the equatorial belt
# hand-placed rows (M, z, ra, dec) for a runner with eps = 10 on the synthetic cosmology; what each is for:
HAND_VALID = [
    (1e14, 0.25, 10.0, 90.0), (1e14, 0.25, 10.0, -90.0),                                # on the poles exactly
    (1e14, 0.25, 200.0, 90.0 - 1e-9), (1e14, 0.25, 200.0, -90.0 + 1e-9),                # within 1e-9 deg of them
    (1e14, 0.25, 33.0, 0.0),                                                            # on the equator
    (1e16, 1e-3, 50.0, 20.0), (1e16, 1e-3, 50.0, 90.0), (1e16, 1e-3, 1.0, -90.0),       # radius >= pi: the whole sphere
    (1e15, 0.01, 120.0, 0.0), (1e15, 0.01, 120.0, _CAP), (1e15, 0.01, 10.0, -_CAP),     # ~0.45 rad across the equator / a cap boundary
    (1e15, 0.01, 0.0, 89.0), (1e15, 0.01, 0.0, -89.0),                                  # ... and over a pole
    (1e15, 0.05, 77.0, 0.001), (1e15, 0.05, 77.0, _CAP + 1e-7), (1e15, 0.05, 77.0, -_CAP - 1e-7),
    (1e12, 0.3, 5.0, 12.3), (1e12, 0.3, 5.0, 0.0),                                      # smaller than a pixel: the 4-pixel fallback
    (1e12, 0.3, 5.0, 89.9), (1e12, 0.3, 5.0, -89.9), (1e12, 0.3, 5.0, 89.9999), (1e12, 0.3, 5.0, -89.9999),      # ... beyond the last ring
]
HAND_INVALID = [
    (np.nan, 0.25, 10.0, 10.0), (0.0, 0.25, 10.0, 10.0), (-1e13, 0.25, 10.0, 10.0), (np.inf, 0.25, 10.0, 10.0),
    (1e14, -1.0, 10.0, 10.0), (1e14, -1.5, 10.0, 10.0),
    (1e14, 0.25, 10.0, 90.0001), (1e14, 0.25, 10.0, -90.0001), (1e14, 0.25, 10.0, np.nan),
]


def catalog_with_hand_rows(random_cat):
    """(catalog, is_random): the hand-placed rows, valid then invalid, in front of the rows of `random_cat`"""
    hand = np.array(HAND_VALID + HAND_INVALID, dtype=np.float64)
    cat = {k: np.concatenate([hand[:, i], np.asarray(random_cat[k], dtype=np.float64)]) for i, k in enumerate(('M', 'z', 'ra', 'dec'))}
    is_random = np.arange(cat['M'].size) >= hand.shape[0]
    return cat, is_random


def valid_rows(cat):
    """rows a runner can place on the sphere: finite M > 0, z > -1, -90 <= dec <= 90"""
    M, z, dec = (np.asarray(cat[k], dtype=np.float64) for k in ('M', 'z', 'dec'))
    with np.errstate(invalid='ignore'):
        return np.isfinite(M) & (M > 0) & np.isfinite(z) & (z > -1.0) & np.isfinite(dec) & (np.abs(dec) <= 90.0)


def disc_radii(cat, eps, bg):
    """(valid, radius [rad], colatitude [rad]) per row; radius = R eps / D_A from oracle.halo_scalars, NaN on invalid rows"""
    ok = valid_rows(cat)
    radius = np.full(ok.size, np.nan)
    sub = {k: np.asarray(cat[k], dtype=np.float64)[ok] for k in ('M', 'z')}
    if ok.any():
        with np.errstate(all='ignore'):
            a, R, D, _ = O.halo_scalars(sub, bg)
            radius[ok] = R * eps / D
    with np.errstate(invalid='ignore'):
        ok &= np.isfinite(radius) & (radius > 0)
    theta = np.pi / 2 - np.radians(np.asarray(cat['dec'], dtype=np.float64))
    return ok, radius, theta


def _rings_of(nside, pix):
    r = hp._pix2ring(nside, np.asarray(pix, dtype=np.int64))
    return int(r.min()), int(r.max())


def true_ring_ranges(nside, cat, eps, bg):
    """dict of per-row arrays: valid; first / last = ring range of the disc's pixels (of the four interpolation pixels when the disc is empty);
    tfirst / tlast = ring range of everything the halo can touch (disc + the fallback pixels of a disc with < 4 pixels); npix_disc; radius; theta.
    Invalid rows carry EMPTY."""
    ok, radius, theta = disc_radii(cat, eps, bg)
    n = ok.size
    out = {'valid': ok, 'radius': radius, 'theta': theta, 'npix_disc': np.zeros(n, dtype=np.int64)}
    for k, v in (('first', EMPTY[0]), ('last', EMPTY[1]), ('tfirst', EMPTY[0]), ('tlast', EMPTY[1])):
        out[k] = np.full(n, v, dtype=np.int64)
    ra, dec = np.asarray(cat['ra'], dtype=np.float64), np.asarray(cat['dec'], dtype=np.float64)
    for j in np.nonzero(ok)[0]:
        if radius[j] >= np.pi:                                   # the whole sphere (query_disc returns every pixel)
            lo, hi, m = 1, 4 * nside - 1, 12 * nside * nside
            flo, fhi = lo, hi
        else:
            pix = O.query_disc(nside, O.ang2vec_lonlat(ra[j], dec[j]).reshape(3), radius[j])
            m = pix.size
            if m < 4:
                flo, fhi = _rings_of(nside, O.get_interp_weights_lonlat(nside, ra[j:j + 1], dec[j:j + 1])[0].reshape(-1))
            lo, hi = _rings_of(nside, pix) if m else (flo, fhi)
            if m >= 4:
                flo, fhi = lo, hi
        out['npix_disc'][j] = m
        out['first'][j], out['last'][j] = lo, hi
        out['tfirst'][j], out['tlast'][j] = min(lo, flo), max(hi, fhi)
    return out


def widen(first, last, margin, nside):
    """[first - margin, last + margin] clipped to [1, 4 nside - 1]; empty ranges (first > last) are returned as EMPTY"""
    first, last = np.asarray(first, dtype=np.int64), np.asarray(last, dtype=np.int64)
    some = first <= last
    return (np.where(some, np.maximum(1, first - margin), EMPTY[0]), np.where(some, np.minimum(4 * nside - 1, last + margin), EMPTY[1]))


def ring_colatitudes(nside):
    """colatitude of the rings 1 .. 4 nside - 1"""
    return hp._ring_theta(nside, np.arange(1, 4 * nside, dtype=np.int64))


def edge_on_a_ring(nside, radius, theta, tol=1e-9):
    """rows whose disc edge theta -+ radius lies within `tol` rad of a ring's colatitude: whether that ring counts as inside the disc is
    decided by the last bit there"""
    th = ring_colatitudes(nside)
    near = np.zeros(np.shape(radius), dtype=bool)
    for edge in (theta - radius, theta + radius):
        i = np.clip(np.searchsorted(th, edge), 1, th.size - 1)
        with np.errstate(invalid='ignore'):
            near |= np.minimum(np.abs(edge - th[i - 1]), np.abs(edge - th[i])) <= tol
    return near


def destinations(first, last, bounds):
    """bool [n][world]: halo -> rank j iff first <= last and bounds[j] <= last and bounds[j + 1] > first"""
    first, last = np.asarray(first, dtype=np.int64)[:, None], np.asarray(last, dtype=np.int64)[:, None]
    b = np.asarray(bounds, dtype=np.int64)
    return (first <= last) & (b[None, :-1] <= last) & (b[None, 1:] > first)


def expected_blocks(first, last, bounds):
    """per destination the (ascending) numbers of the halos it receives"""
    to = destinations(first, last, bounds)
    return [np.nonzero(to[:, j])[0] for j in range(to.shape[1])]


def block_position(d, rank):
    """position of rank d's block in a buffer of world - 1 blocks in rank order that leaves `rank` out"""
    assert d != rank
    return d if d < rank else d - 1
