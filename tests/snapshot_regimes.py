"""Inputs that drive the particle-snapshot kernels (csrc/bfgx_snapshot.hpp) away from the golden shapes: one deterministic case per
regime name, plus the brute-force oracle run of a case (oracle.grid.baryonify_snapshot, cached) and a numpy restatement of the
halo x particle separations that the host test states its preconditions on.  Shared by test_snapshot_regimes_host.py (CPU) and
test_gpu_snapshot_regimes.py.

Conventions of the oracle (see test_snapshot_vs_oracle_larger): halo masses and positions are float32 values held in float64, ln M is the
float32 log, the table is synthetic.displacement_table (strictly negative: no in-table offset is exactly 0) on radii
np.geomspace(1e-6, 1e3, 200), so that no in-ball separation leaves the table.  A "1e-9 inside the upper face" halo sits at the largest
float32 below L (the catalogs hold float32: L - 1e-9 would round to L itself).

A case is a dict: name, ndim, L, redshift, M, hpos [nh, 3], part [np, ndim], kind / owner [np] (what a particle was built as, and for
which halo), R_q [nh] (the oracle's query radius, clamp included), tab_z / tab_M / tab_r / tab_values, eps_runner, eps_model, cells (the
BFGX_SNAP_CELLS values to run; None = unset) and cosmo."""
import functools

import numpy as np

from baryonification_amd import synthetic as syn
from oracle import grid as G
from oracle import oracle as O

REDSHIFT = 0.2
TAB_Z = np.linspace(0.15, 0.25, 3)
TAB_R = np.geomspace(1e-6, 1e3, 200)
UNIFORM, INNER, OUTER, CENTRE, FACE, CROSS_UP, CROSS_DOWN = range(7)          # particle kinds
SHELL = 8                                                                     # particles per shell and halo
TAIL_SIZES = (1, 255, 256, 257, 4097)
REGIMES = ('small_box', 'half_box_balls', 'gpc_box', 'cluster_core', 'rcut_bites') + tuple('tails_%d' % n for n in TAIL_SIZES)


def f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def query_radii(M, L, eps_runner, redshift=REDSHIFT):
    """R_q as bfgo_snapshot_offsets computes it: eps R / a, clipped to [0, L / 2] (SnapshotRunner.py:220-222)"""
    a = 1.0 / (1.0 + redshift)
    return np.clip(eps_runner * G.grid_background(syn.COSMO).get_radius(M, a) / a, 0.0, L / 2)


def _directions(rng, n, ndim):
    v = rng.normal(size=(n, ndim))
    return v / np.linalg.norm(v, axis=1)[:, None]


def _in_balls(rng, centres, radii, ndim):
    """one point per row, uniform in the ball of that row"""
    n = centres.shape[0]
    return centres[:, :ndim] + _directions(rng, n, ndim) * (radii * rng.random(n) ** (1.0 / ndim))[:, None]


class _Particles(object):
    def __init__(self, L, ndim):
        self.L, self.ndim, self.pos, self.kind, self.owner = L, ndim, [], [], []

    def add(self, pos, kind, owner=-1, wrap=True):
        pos = np.atleast_2d(pos)[:, :self.ndim]
        self.pos.append(np.mod(pos, self.L) if wrap else pos)
        self.kind.append(np.full(pos.shape[0], kind))
        self.owner.append(np.broadcast_to(owner, pos.shape[0]).copy())

    def shells(self, rng, hpos, R_q):
        for j in range(hpos.shape[0]):
            for kind, f in ((INNER, 1.0 - 1e-9), (OUTER, 1.0 + 1e-9)):
                self.add(hpos[j, :self.ndim] + R_q[j] * f * _directions(rng, SHELL, self.ndim), kind, j)

    def centres(self, hpos, which):
        for j in which:
            self.add(hpos[j], CENTRE, j, wrap=False)

    def faces(self, rng, per_face=4):
        for ax in range(self.ndim):
            for v in (0.0, self.L):
                p = rng.uniform(0, self.L, (per_face, self.ndim))
                p[:, ax] = v
                self.add(p, FACE, wrap=False)

    def done(self, rng):
        """shuffled, so that every prefix (the `tails` regime) holds a mix of kinds"""
        pos, kind, owner = np.concatenate(self.pos), np.concatenate(self.kind), np.concatenate(self.owner)
        order = rng.permutation(pos.shape[0])
        return np.ascontiguousarray(pos[order]), kind[order], owner[order]


def _finish(name, ndim, L, logM_range, M, hpos, parts, rng, eps_runner, eps_model, cells):
    if ndim == 2:
        hpos = hpos.copy()
        hpos[:, 2] = 0.0
    part, kind, owner = parts.done(rng)
    assert part.min() >= 0.0 and part.max() <= L
    tab_M = np.geomspace(10 ** (logM_range[0] - 0.1), 10 ** (logM_range[1] + 0.1), 8)
    return dict(name=name, ndim=ndim, L=L, redshift=REDSHIFT, M=M, hpos=hpos, part=part, kind=kind, owner=owner,
                R_q=query_radii(M, L, eps_runner), tab_z=TAB_Z, tab_M=tab_M, tab_r=TAB_R, tab_values=syn.displacement_table(TAB_Z, tab_M, TAB_R),
                eps_runner=eps_runner, eps_model=eps_model, cells=list(cells), cosmo=dict(syn.COSMO))


def _small_box(ndim, name='small_box', eps_model=8.0, cells=(1, 2, 3, 4, 7, None)):
    rng = np.random.default_rng(4100 + ndim)
    L, nh, eps = 50.0, 40, 8.0
    below_L = float(np.nextafter(np.float32(L), np.float32(0)))
    M = f32(10 ** rng.uniform(12.0, 15.5, nh))
    hpos = rng.uniform(0, L, (nh, 3))
    hpos[0], hpos[1], hpos[2] = 0.0, L, L / 2                        # corner, the same corner given as (L, L, L), the centre
    for ax in range(3):                                              # 1e-9 inside each face
        hpos[3 + 2 * ax, ax], hpos[4 + 2 * ax, ax] = 1e-9, below_L
    hpos[9, 0], hpos[10, 0] = -0.3, L + 0.4                          # given outside the box
    # the two heaviest halos sit 3 Mpc inside the two x faces and pull the particles that lie just beyond the face through it: the
    # re-wrap in both directions
    M[11], M[12] = f32(10 ** 15.5), f32(10 ** 15.4)
    hpos[11], hpos[12] = (3.0, 12.0, 12.0), (L - 3.0, 37.0, 37.0)
    hpos = f32(hpos)
    R_q = query_radii(M, L, eps)
    P = _Particles(L, ndim)
    P.add(rng.uniform(0, L, (5300, ndim)), UNIFORM)
    P.shells(rng, hpos, R_q)
    P.centres(hpos, (2, 20, 30))
    P.faces(rng)
    for j, kind, x in ((11, CROSS_UP, lambda t: L - t), (12, CROSS_DOWN, lambda t: t)):
        p = hpos[j] + rng.normal(scale=0.3, size=(12, 3))
        p[:, 0] = x(np.geomspace(1e-6, 1e-3, 12))
        P.add(p, kind, j)
    return _finish(name, ndim, L, (12.0, 15.5), M, hpos, P, rng, eps, eps_model, cells)


def _half_box_balls(ndim):
    rng = np.random.default_rng(4200 + ndim)
    L, nh, eps = 6.0, 12, 8.0
    M = f32(10 ** rng.uniform(14.5, 15.3, nh))
    hpos = f32(rng.uniform(0, L, (nh, 3)))
    hpos[0], hpos[1] = 0.0, (L, L / 2, 0.0)
    R_q = query_radii(M, L, eps)
    assert np.all(R_q == L / 2)
    P = _Particles(L, ndim)
    P.add(rng.uniform(0, L, (3000, ndim)), UNIFORM)
    P.shells(rng, hpos, R_q)
    P.centres(hpos, (3, 5, 8))
    P.faces(rng)
    return _finish('half_box_balls', ndim, L, (14.5, 15.3), M, hpos, P, rng, eps, 8.0, (1, 3, 16))


def _gpc_box(ndim):
    rng = np.random.default_rng(4300 + ndim)
    L, nh, eps = 4000.0, 300, 5.0
    M = f32(10 ** rng.uniform(12.5, 14.0, nh))
    hpos = rng.uniform(0, L, (nh, 3))
    near = rng.uniform(0, 2.0, (nh // 2, 3)) * rng.choice([-1.0, 1.0], (nh // 2, 3))          # signed distance to a face, < 2 Mpc
    on = rng.random((nh // 2, 3)) < 0.5                                                        # which axes: a face, an edge or a corner
    on[~on[:, :ndim].any(axis=1), 0] = True
    hpos[:nh // 2] = np.where(on, np.mod(near, L), hpos[:nh // 2])
    hpos = f32(hpos)
    R_q = query_radii(M, L, eps)
    P = _Particles(L, ndim)
    P.add(_in_balls(rng, np.repeat(hpos, 20, axis=0), np.repeat(R_q, 20), ndim), UNIFORM, np.repeat(np.arange(nh), 20))
    P.shells(rng, hpos, R_q)
    P.centres(hpos, (7, 160, 299))
    P.faces(rng)
    return _finish('gpc_box', ndim, L, (12.5, 14.0), M, hpos, P, rng, eps, 8.0, (None,))


def _cluster_core(ndim):
    rng = np.random.default_rng(4400 + ndim)
    L, nh, eps = 200.0, 61, 8.0
    blob = np.array([0.3, 199.8, 77.0])                             # a ball of 2 Mpc across that straddles the x and the y face
    M = f32(10 ** rng.uniform(14.8, 15.3, nh))
    hpos = f32(np.mod(_in_balls(rng, np.tile(blob, (nh, 1)), np.ones(nh), 3), L))
    R_q = query_radii(M, L, eps)
    P = _Particles(L, ndim)
    P.add(_in_balls(rng, np.tile(blob, (4097, 1)), np.ones(4097), ndim), UNIFORM)
    P.shells(rng, hpos, R_q)
    P.centres(hpos, (0, 30, 60))
    P.faces(rng)
    return _finish('cluster_core', ndim, L, (14.8, 15.3), M, hpos, P, rng, eps, 8.0, (None, 2))


@functools.lru_cache(maxsize=None)
def case(name, ndim):
    if name == 'small_box':
        return _small_box(ndim)
    if name == 'half_box_balls':
        return _half_box_balls(ndim)
    if name == 'gpc_box':
        return _gpc_box(ndim)
    if name == 'cluster_core':
        return _cluster_core(ndim)
    if name == 'rcut_bites':
        return _small_box(ndim, 'rcut_bites', 0.6 * 8.0, (None,))
    if name.startswith('tails_'):
        n = int(name[6:])
        c = dict(_small_box(ndim, name, 8.0, (None,)))
        for k in ('part', 'kind', 'owner'):
            c[k] = np.ascontiguousarray(c[k][:n])
        return c
    raise KeyError(name)


def oracle_cat(c):
    return {'M': c['M'], 'x': c['hpos'][:, 0].copy(), 'y': c['hpos'][:, 1].copy(), 'z': c['hpos'][:, 2].copy()}


def oracle_table(c):
    return O.Table([np.log(1 + c['tab_z']), np.log(c['tab_M']), np.log(c['tab_r'])], c['tab_values'], False, c['eps_model'])


def run_oracle(c):
    """(displaced positions [np, ndim], in-ball pairs) of the brute-force fp64 loop"""
    ora, pairs = G.baryonify_snapshot([c['part'][:, k].copy() for k in range(c['ndim'])], c['L'], oracle_cat(c), c['redshift'], oracle_table(c),
                                      c['eps_runner'], G.grid_background(c['cosmo']), return_pairs=True)
    return np.stack(ora, axis=1), int(pairs)


@functools.lru_cache(maxsize=None)
def oracle(name, ndim):
    """the oracle's answer for case(name, ndim): computed once, shared, read-only"""
    ora, pairs = run_oracle(case(name, ndim))
    ora.setflags(write=False)
    return ora, pairs


def min_image(d, L):
    d = np.where(d > L / 2, d - L, d)
    return np.where(d < -L / 2, d + L, d)


def offsets(c, ora):
    """the displacement the oracle applied: ora - part without the re-wrap"""
    return min_image(ora - c['part'], c['L'])


def separations(c):
    """(d [np, nh], in_ball [np, nh]) as the oracle forms them: min-image per axis, d2 <= R_q^2"""
    L, nd = c['L'], c['ndim']
    d2 = np.zeros((c['part'].shape[0], c['M'].size))
    for ax in range(nd):
        d2 += min_image(c['part'][:, ax, None] - c['hpos'][None, :, ax], L) ** 2
    return np.sqrt(d2), d2 <= (c['R_q'] ** 2)[None, :]


def crossings(c, ora):
    """(up, down) [np, ndim]: where the oracle's coordinate before the re-wrap (SnapshotRunner.py:254-257) was above L / below 0.  The
    offsets are far smaller than L / 2, so a re-wrapped coordinate is one that jumped by the box size."""
    with np.errstate(invalid='ignore'):
        return ora - c['part'] < -c['L'] / 2, ora - c['part'] > c['L'] / 2
