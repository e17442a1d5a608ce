"""numpy restatement of MeasureProfilesGrid (tests only): halo-centred radial profiles of a periodic gridded map by brute force, one halo
at a time, no search structure.

Geometry (the runner's docstring): map[i0, i1(, i2)] is the pixel centred on (bins[i0], bins[i1](, bins[i2])); res = bins[1] - bins[0],
L = Npix res; per axis Delta = bins[i] - x_halo, minus L where Delta > L / 2, plus L where Delta < -L / 2 (np.where, in that order), over
the WHOLE axis; d2 = sum Delta^2 left to right, d = sqrt(d2); a pixel is in the ball iff d2 <= R_q^2.  The comoving radius comes from
oracle.oracle.Background.get_radius (oracle.grid.grid_background: w0 = -1), R_q = clip(eps R_com, 0, max(bins) / 2), the bins from
np.searchsorted(edges, x, 'right') - 1.  The distances of a halo are formed on the outer product of the per-axis Deltas that can reach
the ball (|Delta| <= R_q (1 + 4 RIM_TOL)): every other pixel of the grid is farther than the rim on that axis alone.

Two steps, so that several binnings and maps of one catalog share the per-halo loop:

    p = pairs(bins, ndim, cat, redshift, eps, bg)        # the pixels in and just around every ball, as flat arrays
    o = measure(p, r_edges, map, scaled=False, shear=None)

`measure` also returns what a comparison of two correct fp64 evaluations needs: per (halo, bin) cell the number `amb_n` and the sums
`amb_abs` of |v| and `amb_abs_shear` of |g1| + |g2| of its AMBIGUOUS pixels -- |d - R_q| <= RIM_TOL R_q (inside or outside the ball) or
|x - e| <= EDGE_TOL e for some edge e > 0.  (At an edge e = 0 that rule would single out x = 0, the pixel centred exactly on the halo: its
d is a sum of squares of differences of equal numbers, 0 in every evaluation, so nothing is ambiguous there and the cell is held to the
plain bounds.)  An ambiguous pixel is charged to its own bin and to both neighbouring bins."""
import numpy as np

RIM_TOL = 1e-9
EDGE_TOL = 1e-9


def min_image(dx, L):
    dx = np.where(dx > L / 2, dx - L, dx)
    dx = np.where(dx < -L / 2, dx + L, dx)
    return dx


def halo_scalars(cat, ndim, bins, redshift, eps, bg, md=(200.0, 'critical')):
    """a, R_com, R_q, the `bad` rule of the halo preparation and the positions by array axis"""
    M = np.asarray(cat['M'], dtype=np.float64)
    pos = np.stack([np.asarray(cat[k], dtype=np.float64) for k in ('x', 'y', 'z')[:ndim]], axis=1).reshape(M.size, ndim)
    a = 1.0 / (1.0 + redshift)
    bad = ~(M > 0) | ~np.isfinite(M) | ~np.all(np.isfinite(pos), axis=1)
    with np.errstate(all='ignore'):
        R_com = bg.get_radius(np.where(bad, 1.0, M), a, *md) / a
        R_q = np.where(bad, 0.0, np.minimum(np.maximum(eps * R_com, 0.0), np.max(bins) / 2))
        R_com = np.where(bad, np.nan, R_com)
    return a, R_com, R_q, bad, pos


def pairs(bins, ndim, cat, redshift, eps, bg, md=(200.0, 'critical')):
    """The (halo, pixel) pairs of every halo's ball and of the rim just outside it, as flat arrays: halo, pix (flat C-order index), d, the
    per-axis separations D (n_pairs, ndim), inside (d2 <= R_q^2) and rim (|d - R_q| <= RIM_TOL R_q)."""
    bins = np.asarray(bins, dtype=np.float64)
    N = bins.size
    res = bins[1] - bins[0]
    L = N * res
    a, R_com, R_q, bad, pos = halo_scalars(cat, ndim, bins, redshift, eps, bg, md)
    hal, pix, dist, seps, ins = [], [], [], [], []
    for j in range(pos.shape[0]):
        if bad[j]:
            continue
        D = [min_image(bins - pos[j, k], L) for k in range(ndim)]                      # the whole axis
        keep = [np.nonzero(np.abs(Dk) <= R_q[j] * (1.0 + 4 * RIM_TOL))[0] for Dk in D]
        G = np.meshgrid(*[Dk[ik] for Dk, ik in zip(D, keep)], indexing='ij')
        I = np.meshgrid(*keep, indexing='ij')
        d2 = 0
        for Gk in G:
            d2 = d2 + Gk * Gk
        d = np.sqrt(d2)
        near = d <= R_q[j] * (1.0 + 2 * RIM_TOL)
        flat = 0
        for Ik in I:
            flat = flat * N + Ik
        hal.append(np.full(np.count_nonzero(near), j, dtype=np.int64))
        pix.append(np.asarray(flat)[near].astype(np.int64))
        dist.append(d[near])
        seps.append(np.stack([Gk[near] for Gk in G], axis=1))
        ins.append((d2 <= R_q[j] * R_q[j])[near])
    cat_ = lambda l, dt, shape=(0,): np.concatenate(l) if l else np.zeros(shape, dtype=dt)               # noqa: E731
    halo, pidx, d, inside = cat_(hal, np.int64), cat_(pix, np.int64), cat_(dist, np.float64), cat_(ins, bool)
    D = cat_(seps, np.float64, (0, ndim))
    rim = np.abs(d - R_q[halo]) <= RIM_TOL * R_q[halo]
    return dict(n=pos.shape[0], ndim=ndim, N=N, res=res, L=L, R=R_com, R_q=R_q, bad=bad, halo=halo, pix=pidx, d=d, D=D, inside=inside, rim=rim)


def measure(p, r_edges, map, scaled=False, shear=None):
    r_edges = np.asarray(r_edges, dtype=np.float64)
    nb, n = r_edges.size - 1, p['n']
    halo = p['halo']
    x = p['d'] / p['R'][halo] if scaled else p['d']
    b = np.searchsorted(r_edges, x, 'right') - 1
    inbin = (b >= 0) & (b < nb)
    cell = halo * nb + np.clip(b, 0, nb - 1)
    shape = (n, nb)
    count = lambda sel, w=None: np.bincount(cell[sel], weights=None if w is None else w[sel], minlength=n * nb).reshape(shape)   # noqa: E731
    v = np.asarray(map, dtype=np.float64).reshape(-1)[p['pix']]
    fin = np.isfinite(v)
    v0 = np.where(fin, v, 0.0)
    ok = p['inside'] & inbin
    out = dict(r_edges=r_edges, pairs=int(np.count_nonzero(p['inside'])), R=p['R'], R_q=p['R_q'],
               npix=count(ok & fin).astype(np.int64), sum=count(ok & fin, v0), S=count(ok & fin, np.abs(v0)))
    with np.errstate(divide='ignore', invalid='ignore'):
        amb = p['rim'] | np.any((np.abs(x[:, None] - r_edges[None, :]) <= EDGE_TOL * r_edges[None, :]) & (r_edges[None, :] > 0), axis=1)
    g_abs = np.zeros(x.size)
    if shear is not None:
        assert p['ndim'] == 2
        ga, gb = (np.asarray(g, dtype=np.float64).reshape(-1)[p['pix']] for g in shear)
        Dx, Dy, d2 = p['D'][:, 0], p['D'][:, 1], p['d'] * p['d']
        sfin = np.isfinite(ga) & np.isfinite(gb) & (p['d'] > 0)
        ga, gb = np.where(sfin, ga, 0.0), np.where(sfin, gb, 0.0)
        with np.errstate(divide='ignore', invalid='ignore'):
            c2 = np.where(sfin, (Dx * Dx - Dy * Dy) / d2, 0.0)
            s2 = np.where(sfin, 2 * Dx * Dy / d2, 0.0)
        g_abs = np.abs(ga) + np.abs(gb)
        out.update(npix_shear=count(ok & sfin).astype(np.int64), sum_t=count(ok & sfin, -(ga * c2 + gb * s2)),
                   sum_x=count(ok & sfin, ga * s2 - gb * c2), S_shear=count(ok & sfin, g_abs))
    amb_n, amb_abs, amb_abs_shear = np.zeros(n * nb), np.zeros(n * nb), np.zeros(n * nb)
    ia = np.nonzero(amb)[0]
    for db in (-1, 0, 1):                                            # its own bin and both neighbours
        bb = b[ia] + db
        s = (bb >= 0) & (bb < nb)
        c = halo[ia][s] * nb + bb[s]
        np.add.at(amb_n, c, 1.0)
        np.add.at(amb_abs, c, np.abs(v0[ia][s]))
        np.add.at(amb_abs_shear, c, g_abs[ia][s])
    out.update(amb_n=amb_n.reshape(shape), amb_abs=amb_abs.reshape(shape), amb_abs_shear=amb_abs_shear.reshape(shape), amb_pixels=int(ia.size))
    return out
