"""numpy restatements for the derivatives and Minkowski functionals of HEALPix maps (sphtfunc.alm2map_der1 / alm2map_der2,
mapstats.minkowski_*), over sht_oracle.py and sht_spin_oracle.py:

  derivatives   [u, u_t, u_p, u;tt, u;tp, u;pp] of a set of alm in the orthonormal basis (e_theta, e_phi): u_t = d_theta u,
                u_p = d_phi u / sin, u;tt = d_theta^2 u, u;tp = d_theta d_phi u / sin - cos d_phi u / sin^2,
                u;pp = d_phi^2 u / sin^2 + cos d_theta u / sin.  Computed as syntheses of scaled alm: spin 1 of [sqrt(l(l+1)) a, 0] is
                (u_t, u_p), spin 2 of [-sqrt((l+2)(l+1)l(l-1)) a, 0] is (u;tt - u;pp, 2 u;tp), spin 0 of -l(l+1) a is u;tt + u;pp
                (spin_form=True returns these three instead of the Hessian)
  pixel_angles  z = cos(theta), sin(theta) and phi of every RING pixel
  belt_edges, z_derivatives   the known answer u = z: one bin per equatorial-belt ring and the analytic derivatives
  minkowski     per bin of u: the pixel counts, sum sqrt(g2) and sum c / g2 (np.bincount with weights) and the sums of the absolute
                terms (what the GPU test's tolerance is stated in); v0, v1, v2 from them
"""
import numpy as np

import mapstats_oracle as M
import sht_oracle as O
import sht_spin_oracle as S


def ell(lmax, mmax):
    return np.concatenate([np.arange(m, lmax + 1) for m in range(mmax + 1)]).astype(np.float64)


def pixel_angles(nside):
    ring, phi = O._pixel_rings(nside)
    return O.rings(nside)[3][ring], np.sqrt(O.sin2(nside))[ring], phi


def belt_edges(nside):
    """(edges midway between the z of consecutive equatorial-belt rings, ascending; the z of the ring inside every bin)"""
    z = O.rings(nside)[3][nside - 1:3 * nside][::-1]          # rings nside .. 3 nside, z ascending
    return 0.5 * (z[1:] + z[:-1]), z[1:-1]


def z_derivatives(nside):
    """the derivatives of u = z = cos(theta): u_t = -sin, u;tt = u;pp = -z, the rest 0"""
    z, s, _ = pixel_angles(nside)
    return np.stack([z, -s, 0 * z, -z, 0 * z, -z])


def to_spin_form(ders):
    d = np.asarray(ders, dtype=np.float64)
    return np.stack([d[0], d[1], d[2], d[3] + d[5], d[3] - d[5], 2.0 * d[4]])


def derivatives(alm, nside, lmax, mmax, spin_form=False):
    alm = np.asarray(alm, dtype=np.complex128)
    l = ell(lmax, mmax)
    zero = np.zeros_like(alm)
    npix = 12 * nside * nside
    u = O.alm2map(alm, nside, lmax, mmax)
    g = S.alm2map_spin([np.sqrt(l * (l + 1)) * alm, zero], nside, 1, lmax, mmax) if lmax >= 1 else np.zeros((2, npix))
    lap = O.alm2map(-l * (l + 1) * alm, nside, lmax, mmax)
    q = (S.alm2map_spin([-np.sqrt((l + 2) * (l + 1) * l * np.maximum(l - 1, 0)) * alm, zero], nside, 2, lmax, mmax) if lmax >= 2
         else np.zeros((2, npix)))
    if spin_form:
        return np.stack([u, g[0], g[1], lap, q[0], q[1]])
    return np.stack([u, g[0], g[1], 0.5 * (lap + q[0]), 0.5 * q[1], 0.5 * (lap - q[0])])


def minkowski(ders, edges, mask=None, spin_form=False):
    """ders [6, npix]; a pixel is good if all six maps are finite, u is not UNSEEN (mapstats_oracle.good) and the mask, if any, is nonzero"""
    d = np.asarray(ders, dtype=np.float64)
    if not spin_form:
        with np.errstate(invalid='ignore', over='ignore'):
            d = to_spin_form(d)
    e = np.asarray(edges, dtype=np.float64)
    nb = e.size - 1
    ok = M.good(d[0], mask) & np.isfinite(d).all(0)
    u, ut, up, lap, qp, qc = d[:, ok]
    b = np.searchsorted(e, u, side='right') - 1                 # edges[b] <= u < edges[b + 1]; -1 below, nb at or above edges[nb]
    inside = (b >= 0) & (b < nb)
    g2 = ut * ut + up * up
    c = ut * up * qc - 0.5 * lap * g2 + 0.5 * qp * (ut * ut - up * up)
    t1 = np.sqrt(g2)
    t2 = np.divide(c, g2, out=np.zeros_like(c), where=g2 > 0)
    bi = b[inside]
    n = int(ok.sum())
    count = np.bincount(bi, minlength=nb).astype(np.int64)
    sums = np.stack([np.bincount(bi, weights=t[inside], minlength=nb) for t in (t1, t2)])
    scale = np.stack([np.bincount(bi, weights=np.abs(t[inside]), minlength=nb) for t in (t1, t2)])
    width = np.diff(e)
    nf = float(n) if n else np.nan
    v0 = np.array([np.count_nonzero(u >= t) for t in e]) / nf
    return {'n': n, 'count': count, 'below': int((b < 0).sum()), 'above': int((b >= nb).sum()), 'sums': sums, 'scale': scale,
            'v0': v0, 'v1': sums[0] / (4.0 * nf * width), 'v2': sums[1] / (2.0 * np.pi * nf * width)}
