"""numpy restatement of MeasureProfilesSnapshot (tests only): halo-centred radial profiles of the particles of a periodic box, per halo
the ball and the separations of BaryonifySnapshot.process (reference SnapshotRunner.py:217-228), by brute force: every halo against every
particle, no search structure.

The separations are `enforce_periodicity`'s np.where form (:67-92) and d2 = dx*dx + dy*dy (+ dz*dz) left to right, the comoving radius
comes from oracle.oracle.Background.get_radius (oracle.grid.grid_background: w0 = -1), the bins from np.searchsorted(edges, x, 'right') - 1.
Two steps, so that several binnings of one catalog share the brute-force loop:

    p = pairs(part, L, cat, redshift, eps, bg)           # per-halo loop: the particles in and just around every ball, as flat arrays
    o = measure(p, r_edges, weights, scaled=False)

`measure` also returns what a comparison of two correct fp64 evaluations needs: per (halo, bin) cell the number `amb_n` and the sum of
|weight| `amb_abs` of AMBIGUOUS particles -- within RIM_TOL R_q of the rim of the ball (inside or outside it) or, in scaled mode only,
within EDGE_TOL edge of a bin edge.  In unscaled mode x = d is the same correctly rounded square root of the same d2 on both sides, so the
edge comparisons are exact and nothing is ambiguous at an edge."""
import numpy as np

RIM_TOL = 1e-9
EDGE_TOL = 1e-9


def enforce_periodicity(dx, L):
    dx = np.where(dx > L / 2, dx - L, dx)
    dx = np.where(dx < -L / 2, dx + L, dx)
    return dx


def separations(part, h, L):
    """d2 and d of every particle (rows of `part`) from the point h"""
    d2 = 0
    for k in range(part.shape[1]):
        dx = enforce_periodicity(part[:, k] - h[k], L)
        d2 = d2 + dx * dx
    return d2, np.sqrt(d2)


def halo_scalars(cat, ndim, L, redshift, eps, bg, md=(200.0, 'critical')):
    """a, R_com, R_q and the `bad` rule of the halo preparation"""
    M = np.asarray(cat['M'], dtype=np.float64)
    pos = np.stack([np.asarray(cat[k], dtype=np.float64) for k in ('x', 'y', 'z')[:ndim]], axis=1)
    a = 1.0 / (1.0 + redshift)
    bad = ~(M > 0) | ~np.isfinite(M) | ~np.all(np.isfinite(pos), axis=1)
    with np.errstate(all='ignore'):
        R = bg.get_radius(np.where(bad, 1.0, M), a, *md)              # :220 physical Mpc
        R_com = np.where(bad, np.nan, R / a)
        R_q = np.where(bad, 0.0, np.minimum(np.maximum(eps * R / a, 0.0), L / 2))          # :221-222
    return a, R_com, R_q, bad, pos


def pairs(part, L, cat, redshift, eps, bg, md=(200.0, 'critical')):
    """The (halo, particle) pairs of every halo's ball and of the rim just outside it, as flat arrays: halo, part, d, inside (d2 <= R_q^2,
    scipy's squared-distance comparison) and rim (|d - R_q| <= RIM_TOL R_q)."""
    part = np.asarray(part, dtype=np.float64)
    ndim = part.shape[1]
    a, R_com, R_q, bad, pos = halo_scalars(cat, ndim, L, redshift, eps, bg, md)
    hal, idx, dist, ins = [], [], [], []
    for j in range(pos.shape[0]):
        if bad[j]:
            continue
        d2, d = separations(part, pos[j], L)
        near = np.nonzero(d <= R_q[j] * (1.0 + 2 * RIM_TOL))[0]
        hal.append(np.full(near.size, j, dtype=np.int64))
        idx.append(near)
        dist.append(d[near])
        ins.append(d2[near] <= R_q[j] * R_q[j])
    cat_ = lambda l, dt: np.concatenate(l) if l else np.zeros(0, dtype=dt)               # noqa: E731
    halo, pidx, d, inside = cat_(hal, np.int64), cat_(idx, np.int64), cat_(dist, np.float64), cat_(ins, bool)
    rim = np.abs(d - R_q[halo]) <= RIM_TOL * R_q[halo]
    return dict(n=pos.shape[0], ndim=ndim, L=L, R=R_com, R_q=R_q, bad=bad, halo=halo, part=pidx, d=d, inside=inside, rim=rim)


def measure(p, r_edges, weights=None, scaled=False):
    r_edges = np.asarray(r_edges, dtype=np.float64)
    nb, n = r_edges.size - 1, p['n']
    halo = p['halo']
    x = p['d'] / p['R'][halo] if scaled else p['d']
    b = np.searchsorted(r_edges, x, 'right') - 1
    inbin = (b >= 0) & (b < nb)
    cell = halo * nb + np.clip(b, 0, nb - 1)
    shape = (n, nb)
    w = np.ones(x.size) if weights is None else np.asarray(weights, dtype=np.float64)[p['part']]
    wfin = np.where(np.isfinite(w), w, 0.0)                          # a particle with a non-finite weight is counted, not summed
    ok = p['inside'] & inbin
    out = dict(r_edges=r_edges, pairs=int(np.count_nonzero(p['inside'])),
               npart=np.bincount(cell[ok], minlength=n * nb).reshape(shape).astype(np.int64),
               sum=np.bincount(cell[ok], weights=wfin[ok], minlength=n * nb).reshape(shape),
               S=np.bincount(cell[ok], weights=np.abs(wfin[ok]), minlength=n * nb).reshape(shape))
    amb = p['rim'].copy()
    if scaled:
        with np.errstate(divide='ignore', invalid='ignore'):
            amb |= p['inside'] & np.any(np.abs(x[:, None] - r_edges[None, :]) <= EDGE_TOL * r_edges[None, :], axis=1)
    amb_n, amb_abs = np.zeros(n * nb), np.zeros(n * nb)
    ia = np.nonzero(amb)[0]
    tol = 2 * max(RIM_TOL, EDGE_TOL)
    for xs in (x[ia] * (1 - tol), x[ia] * (1 + tol)):               # the cells such a particle may fall into on the other side
        bb = np.searchsorted(r_edges, xs, 'right') - 1
        s = (bb >= 0) & (bb < nb)
        c = halo[ia][s] * nb + bb[s]
        np.add.at(amb_n, c, 1.0)
        np.add.at(amb_abs, c, np.abs(wfin[ia][s]))
    out.update(amb_n=amb_n.reshape(shape), amb_abs=amb_abs.reshape(shape), amb_particles=int(ia.size))
    return out
