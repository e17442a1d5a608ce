"""numpy restatement of MeasureProfilesShell (tests only): halo-centred radial profiles of a RING map, per halo exactly the quantities
of PaintProfilesShell.process (reference HealpixRunner.py:418-441).

Geometry from oracle/refshim/healpy.py (ang2vec, query_disc, pix2vec, pix2ang), the background (D_A spline, critical density) from
oracle.oracle.Background; bins by np.digitize, sums by np.bincount with weights.  Two steps, so that several binnings of one
catalog share the per-halo disc queries:

    d = discs(nside, cat, eps, bg)                     # per-halo loop: query_disc, then the pairs of all halos as flat arrays
    o = measure(d, r_edges, m, shear=(g1, g2), scaled=False)

`measure` also returns what a comparison of two correct fp64 evaluations needs: per (halo, bin) cell the number and the sum |value|
of AMBIGUOUS pixels -- |x / edge - 1| < 1e-6 for some edge, or an angle from the halo within 1e-9 (relative) of the disc radius, inside
or outside the disc -- and the smallest halo-pixel angle of the cell."""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location(
    '_stack_refshim_healpy', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle', 'refshim', 'healpy.py'))
hp = importlib.util.module_from_spec(_spec)                        # the refshim, loaded under a private name (as sht_oracle.py does)
_spec.loader.exec_module(hp)

UNSEEN = -1.6375e30
EDGE_TOL = 1e-6
DISC_TOL = 1e-9


def counts(v):
    """finite and not UNSEEN by healpy's mask_bad rule (np.isclose(v, UNSEEN, rtol=1e-5, atol=1e-8))"""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return np.isfinite(v) & ~(np.abs(v - UNSEEN) <= 1e-8 + 1e-5 * abs(UNSEEN))


def halo_scalars(cat, eps, bg, md=(200.0, 'critical')):
    """a_j, R_j (physical Mpc), D_j, disc radius [rad], and the `bad` rule of the halo preparation"""
    M, z = np.asarray(cat['M'], dtype=np.float64), np.asarray(cat['z'], dtype=np.float64)
    dec = np.asarray(cat['dec'], dtype=np.float64)
    with np.errstate(all='ignore'):
        a = 1.0 / (1.0 + z)
        R = bg.get_radius(M, a, *md)
        D = bg.Da_spline()(z)
        radius = R * eps / D
        theta = np.pi / 2.0 - np.radians(dec)
        bad = ~(radius > 0) | ~np.isfinite(radius) | ~(theta >= 0) | ~(theta <= np.pi) | ~(M > 0) | ~np.isfinite(M) | ~(z > -1)
    return a, R, D, radius, bad


def discs(nside, cat, eps, bg, md=(200.0, 'critical')):
    """The (halo, pixel) pairs of every halo's disc and of the rim just outside it, as flat arrays:
    halo, pix, inside (member of query_disc at the exact radius), dist = |vec_pix - vec_j|, angle, t_th, t_ph"""
    a, R, D, radius, bad = halo_scalars(cat, eps, bg, md)
    n = a.size
    ra, dec = np.asarray(cat['ra'], dtype=np.float64), np.asarray(cat['dec'], dtype=np.float64)
    hal, pixs, ins = [], [], []
    vecs = np.zeros((n, 3))
    for j in range(n):
        if bad[j]:
            continue
        vec = hp.ang2vec(ra[j], dec[j], lonlat=True)
        vecs[j] = vec
        pix = hp.query_disc(nside, vec, radius[j], inclusive=False, nest=False)
        wide = hp.query_disc(nside, vec, min(radius[j] * (1.0 + 4 * DISC_TOL) + 1e-15, np.pi), inclusive=False, nest=False)
        allp = np.union1d(pix, wide)
        hal.append(np.full(allp.size, j, dtype=np.int64))
        pixs.append(allp)
        ins.append(np.isin(allp, pix))
    cat_ = lambda l, dt: np.concatenate(l) if l else np.zeros(0, dtype=dt)               # noqa: E731
    halo, pix, inside = cat_(hal, np.int64), cat_(pixs, np.int64), cat_(ins, bool)
    vx, vy, vz = hp.pix2vec(nside, pix)
    v = np.stack([vx, vy, vz], axis=1)
    vj = vecs[halo]
    dist = np.sqrt(np.sum((v - vj) ** 2, axis=1))                                          # :435-438 without D_j
    angle = 2.0 * np.arcsin(np.minimum(0.5 * dist, 1.0))
    theta, phi = hp.pix2ang(nside, pix)
    e_th = np.stack([np.cos(theta) * np.cos(phi), np.cos(theta) * np.sin(phi), -np.sin(theta)], axis=1)
    e_ph = np.stack([-np.sin(phi), np.cos(phi), np.zeros(phi.size)], axis=1)
    t = vj - np.sum(vj * v, axis=1)[:, None] * v                                           # tangent at the pixel pointing to the halo
    return dict(nside=nside, n=n, a=a, R=R, D=D, radius=radius, bad=bad, halo=halo, pix=pix, inside=inside, dist=dist, angle=angle,
                t_th=np.sum(t * e_th, axis=1), t_ph=np.sum(t * e_ph, axis=1))


def measure(d, r_edges, m, shear=None, scaled=False):
    r_edges = np.asarray(r_edges, dtype=np.float64)
    nb, n = r_edges.size - 1, d['n']
    halo, pix = d['halo'], d['pix']
    x = d['D'][halo] * d['dist'] / (d['R'][halo] if scaled else d['a'][halo])               # r_sep / R_j, or r_sep / a_j (:441)
    b = np.digitize(x, r_edges) - 1
    inbin = (b >= 0) & (b < nb)
    cell = halo * nb + np.clip(b, 0, nb - 1)
    mv = np.asarray(m, dtype=np.float64)[pix]
    shape = (n, nb)

    def count(sel):
        return np.bincount(cell[sel], minlength=n * nb).reshape(shape).astype(np.int64)

    def total(sel, w):
        return np.bincount(cell[sel], weights=w[sel], minlength=n * nb).reshape(shape)

    ok = d['inside'] & inbin & counts(mv)
    out = dict(r_edges=r_edges, npix=count(ok), sum=total(ok, mv), S=total(ok, np.abs(mv)))
    # ambiguous pixels: next to a bin edge (they may fall into either neighbour), or on the rim of the disc (inside or outside it)
    with np.errstate(divide='ignore', invalid='ignore'):
        near_edge = np.any(np.abs(x[:, None] / r_edges[None, :] - 1.0) < EDGE_TOL, axis=1)
        rim = np.abs(d['angle'] / d['radius'][halo] - 1.0) < DISC_TOL
    amb = (near_edge & d['inside']) | rim
    absval = np.where(np.isfinite(mv), np.abs(mv), 0.0)
    if shear is not None:
        g1, g2 = (np.asarray(g, dtype=np.float64)[pix] for g in shear)
        absval_g = np.where(np.isfinite(g1), np.abs(g1), 0.0) + np.where(np.isfinite(g2), np.abs(g2), 0.0)
    amb_n = np.zeros(n * nb)
    amb_abs = np.zeros(n * nb)
    amb_abs_g = np.zeros(n * nb)
    ia = np.nonzero(amb)[0]
    for xs in (x[ia] * (1 - 2 * EDGE_TOL), x[ia] * (1 + 2 * EDGE_TOL)):
        bb = np.digitize(xs, r_edges) - 1
        s = (bb >= 0) & (bb < nb)
        c = halo[ia][s] * nb + bb[s]
        np.add.at(amb_n, c, 1.0)
        np.add.at(amb_abs, c, absval[ia][s])
        if shear is not None:
            np.add.at(amb_abs_g, c, absval_g[ia][s])
    out.update(amb_n=amb_n.reshape(shape), amb_abs=amb_abs.reshape(shape), amb_abs_g=amb_abs_g.reshape(shape),
               pairs=int(np.count_nonzero(d['inside'])), amb_pixels=int(ia.size))
    if shear is not None:
        t_th, t_ph = d['t_th'], d['t_ph']
        n2 = t_th ** 2 + t_ph ** 2
        oks = d['inside'] & inbin & counts(g1) & counts(g2) & (n2 > 0)                     # (a halo on the pixel centre has no position angle)
        with np.errstate(divide='ignore', invalid='ignore'):
            c2 = (t_th ** 2 - t_ph ** 2) / n2
            s2 = 2.0 * t_th * t_ph / n2
        gt = np.where(oks, -(g1 * c2 + g2 * s2), 0.0)                                       # gamma_t + i gamma_x = -(g1 + i g2) e^{-2 i phi}
        gx = np.where(oks, g1 * s2 - g2 * c2, 0.0)
        tmin = np.full(n * nb, np.inf)
        np.minimum.at(tmin, cell[oks], d['angle'][oks])
        out.update(npix_shear=count(oks), sum_t=total(oks, gt), sum_x=total(oks, gx), S_g=total(oks, np.abs(g1) + np.abs(g2)),
                   theta_min=tmin.reshape(shape))
    with np.errstate(divide='ignore', invalid='ignore'):
        out['mean'] = np.where(out['npix'] > 0, out['sum'] / out['npix'], np.nan)
        if shear is not None:
            out['mean_t'] = np.where(out['npix_shear'] > 0, out['sum_t'] / out['npix_shear'], np.nan)
            out['mean_x'] = np.where(out['npix_shear'] > 0, out['sum_x'] / out['npix_shear'], np.nan)
    return out


def brute_force(nside, cat, eps, bg, r_edges, m, shear=None, scaled=False, md=(200.0, 'critical')):
    """The same definition over ALL 12 nside^2 pixels: the angle from the halo by arccos, no query_disc.  Returns npix, sum and, with
    shear, npix_shear, sum_t, sum_x."""
    r_edges = np.asarray(r_edges, dtype=np.float64)
    a, R, D, radius, bad = halo_scalars(cat, eps, bg, md)
    n, nb, npx = a.size, r_edges.size - 1, 12 * nside * nside
    allpix = np.arange(npx)
    v = np.stack(hp.pix2vec(nside, allpix), axis=1)
    theta, phi = hp.pix2ang(nside, allpix)
    e_th = np.stack([np.cos(theta) * np.cos(phi), np.cos(theta) * np.sin(phi), -np.sin(theta)], axis=1)
    e_ph = np.stack([-np.sin(phi), np.cos(phi), np.zeros(npx)], axis=1)
    mv = np.asarray(m, dtype=np.float64)
    out = dict(npix=np.zeros((n, nb), dtype=np.int64), sum=np.zeros((n, nb)))
    if shear is not None:
        g1, g2 = (np.asarray(g, dtype=np.float64) for g in shear)
        out.update(npix_shear=np.zeros((n, nb), dtype=np.int64), sum_t=np.zeros((n, nb)), sum_x=np.zeros((n, nb)))
    for j in range(n):
        if bad[j]:
            continue
        vj = hp.ang2vec(cat['ra'][j], cat['dec'][j], lonlat=True)
        ang = np.arccos(np.clip(v @ vj, -1.0, 1.0))
        x = D[j] * np.sqrt(np.sum((v - vj) ** 2, axis=1)) / (R[j] if scaled else a[j])
        for bi in range(nb):
            sel = (ang <= radius[j]) & (x >= r_edges[bi]) & (x < r_edges[bi + 1])
            s = sel & counts(mv)
            out['npix'][j, bi] = np.count_nonzero(s)
            out['sum'][j, bi] = mv[s].sum()
            if shear is not None:
                t = vj[None, :] - (v @ vj)[:, None] * v
                t_th, t_ph = np.sum(t * e_th, axis=1), np.sum(t * e_ph, axis=1)
                n2 = t_th ** 2 + t_ph ** 2
                s = sel & counts(g1) & counts(g2) & (n2 > 0)
                c2, s2 = (t_th[s] ** 2 - t_ph[s] ** 2) / n2[s], 2 * t_th[s] * t_ph[s] / n2[s]
                out['npix_shear'][j, bi] = np.count_nonzero(s)
                out['sum_t'][j, bi] = -(g1[s] * c2 + g2[s] * s2).sum()
                out['sum_x'][j, bi] = (g1[s] * s2 - g2[s] * c2).sum()
    return out
