"""Interlaced CIC / TSC grids and P(k) straight from particles on the GPU, against tests/interlace_oracle.py (plain numpy, checked by hand
in test_interlace_oracle_host.py):

  1. the shifted deposit bit for bit (L == N, coordinates on multiples of a quarter cell, masses k / 1024: every weight, product and sum
     is exact in fp64 whatever the order of addition), both forms, on an output that starts NaN-filled
  2. the shifted deposit on generic input within the per-cell bound derived in test_gpu_deposit_cloud.py
  3. shift = 0 is deposit_cloud_device
  4. the estimator on two independent random maps: per filled bin |pk - ref| <= (fft_oracle.bound(N) + 8 * 2^-53) (paa_ref + pbb_ref) / 2
     ((|F1|^2 + |F2|^2) / 2 bounds |C|^2 mode by mode and bound(N) is what the three sums of the cross pass are held to; the second
     term is the twist's complex multiplications), pk_grid1 to bound(N), relative
  5. phase, sign and index of the twist on single plane waves
  6. the public route engine.particle_power_spectrum against particle_power_spectrum_ref at 1e-10 (the tolerance test_gpu_xpk.py uses
     for public routes), numpy columns and CUDA tensors
  7. ParticleSnapshot.power_spectrum
  8. the tiled deposits end to end, 2^20 particles, no environment override
  9. one particle: the interlaced estimate misses |F|^2 = 1 by five times less than the deconvolved single grid

Measured on the MI355X, check 4, worst bin of the worst case per N, as a fraction of its bound (bound(N) is 1.8e-15 at N = 8 and 4.1e-15
to 5.3e-15 above):
  N           8      16     64     256
  pk          0.082  0.063  0.089  0.24
  pk_grid1    0.24   0.11   0.27   0.60    (0.76 in another run: the sums are added by atomics in an order that changes)
pk_grid1 at N = 256 is the sum of a few 1e5 squares per bin, added up by the cross pass as it is: 512 workgroups' partial sums meet in
one global atomic per bin, and a random walk of that many roundings is the size of its 2.4e-15 to 3.1e-15.  Check 5: pk / pk_grid1 - 1 is 0 or +-2.2e-16 with +map2 and
at most 5.6e-17 with -map2.  Check 9: 0.1098 against 1.015 (CIC), 0.01528 against 0.3162 (TSC), the oracle's figures.
The N = 256 cases of check 4 take 5 to 7 s each, nearly all of it xpk_oracle.binned_cube on the full cube; the first test of the file
pays the runtime's start-up."""
import numpy as np
import pytest

import deposit_cloud_oracle as CO
import deposit_oracle as DO
import fft_oracle as O
import interlace_oracle as IO
import xpk_oracle as X

pytestmark = pytest.mark.gpu

L_ODD = 250.0 / 3.0                                   # not representable in fp64
FORMS = ['tiled', 'atomic']
ORDERS = [2, 3]


@pytest.fixture(scope='module', autouse=True)
def _release_the_tables():
    yield
    import torch
    from baryonification_amd import _lib
    torch.cuda.synchronize()
    _lib.load().bfgx_cache_clear()


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64, order='C')).to('cuda:0')            # (a copy: the shared maps are read-only)


def _deposit(monkeypatch, form, coords, mass, N, L, order, shift=1):
    """the map of engine.deposit_cloud_device(..., shift) for host columns, the output pre-filled with NaN"""
    import torch
    from baryonification_amd import engine
    monkeypatch.setenv('BFGX_DEPOSIT', form)
    ndim, n = len(coords), coords[0].size
    cols = [_dev(c) for c in coords]
    m = None if mass is None else _dev(mass)
    out = torch.full((N,) * ndim, float('nan'), dtype=torch.float64, device='cuda:0')
    ptr = [c.data_ptr() if n else 0 for c in cols] + [0] * (3 - ndim)
    engine.deposit_cloud_device(ptr[0], ptr[1], ptr[2], m.data_ptr() if (m is not None and n) else 0, n, N, L, order, out.data_ptr(), ndim,
                                shift=shift)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same(got, ref):
    assert got.shape == ref.shape
    bad = got != ref                                                  # (a cell left NaN differs too)
    assert not bad.any(), '%d of %d cells differ, sum %r against %r, first at %s' % (
        bad.sum(), bad.size, np.nansum(got), ref.sum(), np.argwhere(bad)[:5].tolist())
    assert np.array_equal(got, ref)


def _check(monkeypatch, form, p, mass, N, order, shift=1):
    coords = [p[:, a] for a in range(p.shape[1])]
    ref = IO.deposit(coords, mass, N, float(N), order, shift=shift)
    _same(_deposit(monkeypatch, form, coords, mass, N, float(N), order, shift), ref)
    return ref


def _quarter_lattice(rng, n, ndim, N):
    """multiples of 1/4 in [0, N], both ends included"""
    return rng.integers(0, 4 * N + 1, (n, ndim)) / 4.0


def _seam_and_face_particles(rng, ndim, N, k):
    """k particles within a cell of a tile seam on every axis at once, and every combination of 0, L and L - 1/4 over the axes"""
    g = DO.geometry(ndim, N)
    seams = [np.arange(nt) * s for nt, s in zip(g.ntiles, g.shape)]
    near = np.stack([rng.choice(c, k) for c in seams], axis=1) + rng.integers(-4, 5, (k, ndim)) / 4.0
    near = np.mod(near, float(N))
    ends = np.array([0.0, float(N), N - 0.25])
    faces = np.stack(np.meshgrid(*([ends] * ndim), indexing='ij'), axis=-1).reshape(-1, ndim)
    return np.concatenate([near, faces])


def _dropped(rng, ndim, N):
    """NaN, -1 and L + 1 on each axis in turn"""
    bad = np.array([np.nan, -1.0, N + 1.0])
    rows = []
    for a in range(ndim):
        q = _quarter_lattice(rng, bad.size, ndim, N)
        q[:, a] = bad
        rows.append(q)
    return np.concatenate(rows)


# --------------------------------------------------------------------------------------------- 1. the shifted deposit, bit for bit
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('with_mass', [True, False])
@pytest.mark.parametrize('ndim,N', [(3, 1), (3, 2), (3, 17), (3, 33), (3, 70), (2, 1), (2, 2), (2, 65), (2, 130)])
def test_shifted_deposit_exact(gpu, monkeypatch, ndim, N, with_mass, order, form):
    """seams and partial tiles (3-D tiles are 16 x 16 x 32 cells, 2-D ones 64 x 128), grids of one and two cells, particles at 0, L and
    L - 1/4 in every combination over the axes, dropped particles in between"""
    rng = np.random.default_rng(1000 * N + 10 * ndim + order)
    p = np.concatenate([_seam_and_face_particles(rng, ndim, N, 400), _quarter_lattice(rng, 3000, ndim, N), _dropped(rng, ndim, N)])
    p = rng.permutation(p)
    coords = [p[:, a] for a in range(ndim)]
    keep = CO.kept(coords, float(N))
    assert np.count_nonzero(~keep) == 3 * ndim and np.count_nonzero(p == float(N)) >= ndim and np.count_nonzero(p == 0.0) >= ndim
    if N > 2:
        # the input reaches both sides of the wrap on the shifted grid: base cell 0 from v = L, and cell N - 1 feeding cell 0
        base = np.stack([IO.shifted_base_cell(c, N, float(N), order) for c in coords], axis=1)[keep]
        assert (base[(p[keep] == float(N))] == 0).all() and np.count_nonzero(base == N - 1) > 0
    mass = DO.dyadic_masses(rng, p.shape[0]) if with_mass else None
    ref = _check(monkeypatch, form, p, mass, N, order)
    assert ref.sum() == (float(np.sum((mass[keep] * 1024).astype(np.int64))) / 1024.0 if with_mass else float(keep.sum()))
    if N > 2:
        assert np.abs(ref - CO.deposit(coords, mass, N, float(N), order)).max() > 0      # (the shift does something)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('n', [0, 1, 255, 256, 257, DO.CHUNK - 1, DO.CHUNK + 1])
def test_shifted_deposit_particle_counts(gpu, monkeypatch, n, order, form):
    rng = np.random.default_rng(n)
    N = 33
    p = _quarter_lattice(rng, n, 3, N) if n != 1 else np.array([[27.75, 33.0, 0.0]])
    ref = _check(monkeypatch, form, p, DO.dyadic_masses(rng, n), N, order)
    assert (ref.sum() > 0) == (n > 0)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('ndim,N,cell', [(3, 33, 32), (3, 33, 15), (2, 130, 129), (2, 130, 0)])
def test_shifted_deposit_every_particle_in_one_cell(gpu, monkeypatch, ndim, N, cell, order, form):
    """5000 particles whose base cell on the shifted grid is one cell (the last cell of the grid, whose cloud wraps; a cell at a seam)"""
    rng = np.random.default_rng(cell + order)
    lo = cell if order == 2 else cell - 0.5                                 # base cell: floor(t) (CIC), floor(t + 1/2) (TSC)
    p = np.mod(lo + rng.integers(0, 4, (5000, ndim)) / 4.0, float(N))
    base = np.stack([IO.shifted_base_cell(p[:, a], N, float(N), order) for a in range(ndim)], axis=1)
    assert (base == cell).all()
    ref = _check(monkeypatch, form, p, DO.dyadic_masses(rng, 5000), N, order)
    assert np.count_nonzero(ref) <= order ** ndim


# --------------------------------------------------------------------------------------------- 2. generic input
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('order', ORDERS)
def test_shifted_deposit_generic_input_within_the_derived_bound(gpu, monkeypatch, order, form):
    """L = 250/3, N = 40, 20 000 particles with masses.  The bound of test_gpu_deposit_cloud.py, restated: per cell, with S = sum |m w|
    over the oracle's contributions, and k, M the number and the sum of |m| of the particles whose cloud, taken one cell wider on every
    side, holds the cell: t = v s is rounded once on either side and may differ by N 2^-52 where a compiler contracts; every weight has
    slope <= 1 in t, is continuous across a change of base cell and takes at most 3 roundings, the product with the mass 3 more:
    |d(m w)| <= |m| eps, eps = (6 N + 12) 2^-53; both sides add at most k terms in some order: bound = 2 k 2^-53 (S + eps M) + eps M"""
    rng = np.random.default_rng(12)
    N, n = 40, 20000
    p = rng.uniform(-0.01 * L_ODD, 1.01 * L_ODD, (n, 3))
    p[:2000] = 0.3 * L_ODD + rng.normal(0, 0.01 * L_ODD, (2000, 3))
    p[2000:2003] = [[0.0, L_ODD, 0.5 * L_ODD], [L_ODD, L_ODD, L_ODD], [np.nextafter(L_ODD, 0.0), 0.0, 0.0]]
    mass = rng.uniform(0.5, 2.0, n)
    coords = [p[:, a] for a in range(3)]
    ref = IO.shifted_deposit(coords, mass, N, L_ODD, order)
    k = IO.shifted_deposit(coords, None, N, L_ODD, order, unit_weights=True, widen=1)
    s_abs = IO.shifted_deposit(coords, np.abs(mass), N, L_ODD, order)
    m_abs = IO.shifted_deposit(coords, np.abs(mass), N, L_ODD, order, unit_weights=True, widen=1)
    eps_w = (6.0 * N + 12.0) * 2.0 ** -53
    bound = 2.0 * k * 2.0 ** -53 * (s_abs + eps_w * m_abs) + eps_w * m_abs
    assert k.max() > 100 and 0 < np.count_nonzero(~CO.kept(coords, L_ODD)) < 0.1 * n
    got = _deposit(monkeypatch, form, coords, mass, N, L_ODD, order)
    err = np.abs(got - ref)
    print('max err / bound = %.3g, largest k = %d' % (np.nanmax(err[k > 0] / bound[k > 0]), k.max()))
    assert np.isfinite(got).all() and (err <= bound).all() and mass.min() > 1e6 * bound.max()


# --------------------------------------------------------------------------------------------- 3. shift = 0
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('order', ORDERS)
def test_shift_zero_is_the_unshifted_deposit(gpu, monkeypatch, order, form):
    import torch
    from baryonification_amd import engine
    rng = np.random.default_rng(33 + order)
    N = 33
    p = np.concatenate([_seam_and_face_particles(rng, 3, N, 400), _quarter_lattice(rng, 3000, 3, N), _dropped(rng, 3, N)])
    mass = DO.dyadic_masses(rng, p.shape[0])
    ref = _check(monkeypatch, form, p, mass, N, order, shift=0)
    assert np.array_equal(ref, CO.deposit([p[:, a] for a in range(3)], mass, N, float(N), order))
    cols, m = [_dev(p[:, a]) for a in range(3)], _dev(mass)
    out = torch.full((N,) * 3, float('nan'), dtype=torch.float64, device='cuda:0')
    engine.deposit_cloud_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), m.data_ptr(), p.shape[0], N, float(N), order,
                                out.data_ptr())
    torch.cuda.synchronize()
    _same(out.cpu().numpy(), ref)


# --------------------------------------------------------------------------------------------- 4. the estimator on synthetic maps
_MAPS = {}


def _random_maps(N):
    """two independent maps per N, made once and left alone"""
    if N not in _MAPS:
        rng = np.random.default_rng(500 + N)
        a, b = rng.poisson(4.0, (N, N, N)).astype(np.float64), rng.poisson(4.0, (N, N, N)).astype(np.float64)
        a[3, 5, 7] += 500.0
        a.setflags(write=False)
        b.setflags(write=False)
        _MAPS[N] = (a, b, _dev(a), _dev(b))
    return _MAPS[N]


def _check_estimator(got, ref, N):
    """the assertions of check 4 -> (worst pk error, worst pk_grid1 error) as fractions of their bounds"""
    assert set(got) == {'k', 'pk', 'pk_grid1', 'counts'}
    assert np.array_equal(got['counts'], ref['counts'])
    good = ref['counts'] > 0
    assert good.any()
    for key in ('k', 'pk', 'pk_grid1'):
        assert np.array_equal(np.isnan(got[key]), ~good), key
    assert np.abs(got['k'][good] / ref['k'][good] - 1).max() <= 1e-12
    bound = O.bound(N) + 8 * 2.0 ** -53
    e = np.abs(got['pk'][good] - ref['pk'][good]) / (0.5 * (ref['paa'][good] + ref['pbb'][good]))
    e1 = np.abs(got['pk_grid1'][good] / ref['pk_grid1'][good] - 1)
    print("   N = %4d: pk %.2e (%.3f of the bound)  pk_grid1 %.2e (%.3f of the bound)" % (N, e.max(), e.max() / bound, e1.max(), e1.max() / O.bound(N)))
    assert e.max() <= bound, ('pk', int(np.argmax(e)), e.max())
    assert e1.max() <= O.bound(N), ('pk_grid1', int(np.argmax(e1)), e1.max())
    return e.max() / bound, e1.max() / O.bound(N)


ESTIMATOR_CASES = [(N, nk, p) for N in (8, 16, 64) for nk in (7, 100, 300) for p in (0, 2, 3)] + [(256, 100, 3), (256, 300, 2)]


@pytest.mark.parametrize('N,nk,p', ESTIMATOR_CASES)
def test_interlaced_estimator_on_synthetic_maps(gpu, N, nk, p):
    """nk = 7 and 100 take the tabulated bins, nk = 300 the bins computed per mode; numpy cubes and CUDA tensors give the same"""
    from baryonification_amd import engine
    L = 305.0
    a, b, da, db = _random_maps(N)
    ref = IO.interlaced_ref(a, b, L, nk, p)
    got = engine.interlaced_power_spectrum(da, db, L, nk, window=p)
    _check_estimator(got, ref, N)
    assert np.array_equal(da.cpu().numpy(), a) and np.array_equal(db.cpu().numpy(), b)
    if N <= 16:
        host = engine.interlaced_power_spectrum(a, b, L, nk, window={0: 'none', 2: 'cic', 3: 'TSC'}[p])
        _check_estimator(host, ref, N)
    # the two maps are not interchangeable, and grid 1 alone is the windowed auto spectrum
    good = ref['counts'] > 0
    x = engine.cross_power_spectrum(da, db, L, nk, window=p)
    assert np.abs(got['pk_grid1'][good] / x['paa'][good] - 1).max() <= 1e-12
    assert np.abs(got['pk'][good] / got['pk_grid1'][good] - 1).max() > 1e-3


# --------------------------------------------------------------------------------------------- 5. phase, sign and index
@pytest.mark.parametrize('nk', [8, 300])
@pytest.mark.parametrize('m', [(1, 0, 0), (0, 2, 0), (0, 0, 3), (-3, 0, 0), (5, -1, -2), (7, 7, 0)])
def test_twist_phase_sign_and_index(gpu, m, nk):
    """map1 = cos(2 pi m.x / N + 0.3) and the same wave sampled half a cell further on every axis: with +map2 the two grids add up in
    the mode's bin, pk = pk_grid1; with -map2 they cancel, |pk| <= bound pk_grid1 (the sum may round to either side of zero).  The
    conjugate phase leaves 0.69 to 0.96 of pk_grid1 on these modes, a phase applied to the wrong axis or index likewise: neither can
    pass.  (7, 7, 0) has |k| = 9.9 fundamentals, beyond the Nyquist frequency of 8 where the bins end: it must leave every bin empty
    to the same bound, which a phase read at a wrong index of the table's upper half would not"""
    from baryonification_amd import engine
    N, L = 16, 305.0
    i = np.arange(N)
    arg = 2 * np.pi * (m[0] * i[:, None, None] + m[1] * i[None, :, None] + m[2] * i[None, None, :]) / N + 0.3
    map1 = np.cos(arg)
    map2 = np.cos(arg - np.pi * sum(m) / N)
    _, bin_ = O.mode_k_and_bin(N, L, nk, m[0] % N, m[1] % N, m[2] % N)
    bound = O.bound(N) + 8 * 2.0 ** -53
    plus = engine.interlaced_power_spectrum(map1, map2, L, nk, window=0)
    minus = engine.interlaced_power_spectrum(map1, -map2, L, nk, window=0)
    ref = IO.interlaced_ref(map1, map2, L, nk, 0)
    if not 0 <= bin_ < nk:
        assert m == (7, 7, 0)
        mode_power = 0.25 * float(N) ** 6                                   # |F1|^2 of the mode
        filled = ref['counts'] > 0
        for r in (plus, minus):
            assert (np.abs(r['pk'][filled]) * ref['counts'][filled] <= bound * mode_power).all()
            assert (np.abs(r['pk_grid1'][filled]) * ref['counts'][filled] <= bound * mode_power).all()
        return
    p1 = plus['pk_grid1'][bin_]
    print('m = %s: pk / pk_grid1 = 1 %+.3g with +map2, %.3g with -map2' % (m, plus['pk'][bin_] / p1 - 1, minus['pk'][bin_] / p1))
    assert p1 > 0 and abs(p1 / ref['pk_grid1'][bin_] - 1) <= O.bound(N)
    assert abs(plus['pk'][bin_] - p1) <= bound * p1
    assert abs(plus['pk'][bin_] - ref['pk'][bin_]) <= bound * 0.5 * (ref['paa'][bin_] + ref['pbb'][bin_])
    assert abs(minus['pk'][bin_]) <= bound * p1
    conj = IO.phase_cube(N).conj()
    wrong = 0.25 * np.abs(np.fft.fftn(map1) + conj * np.fft.fftn(map2)) ** 2
    assert wrong[m[0] % N, m[1] % N, m[2] % N] < 0.97 * np.abs(np.fft.fftn(map1)[m[0] % N, m[1] % N, m[2] % N]) ** 2


# --------------------------------------------------------------------------------------------- 6. the public route
_PARTICLES = {}


def _particles():
    if not _PARTICLES:
        rng = np.random.default_rng(77)
        L = 7.3
        p = rng.uniform(-0.02 * L, 1.02 * L, (2000, 3))
        p[:300] = 0.6 * L + rng.normal(0, 0.03 * L, (300, 3))
        _PARTICLES.update(L=L, coords=[np.ascontiguousarray(p[:, a]) for a in range(3)], mass=rng.uniform(0.5, 2.0, 2000))
    return _PARTICLES['coords'], _PARTICLES['mass'], _PARTICLES['L']


def _snapshot(coords, mass, L, flat=False):
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    return bfg.utils.ParticleSnapshot(x=coords[0], y=coords[1], z=None if flat else coords[2], M=mass, L=L, redshift=0.0, cosmo=dict(syn.COSMO))


def _check_particles(got, ref, tol=1e-10):
    assert set(got) == {'k', 'pk', 'pk_grid1', 'counts', 'shot_noise', 'mass'}
    assert np.array_equal(got['counts'], ref['counts'])
    good = ref['counts'] > 0
    assert good.any()
    for key in ('k', 'pk', 'pk_grid1'):
        assert np.array_equal(np.isnan(got[key]), ~good), key
        assert np.abs(got[key][good] / ref[key][good] - 1).max() <= tol, (key, np.abs(got[key][good] / ref[key][good] - 1).max())
    assert abs(got['mass'] / ref['mass'] - 1) <= 1e-13 and abs(got['shot_noise'] / ref['shot_noise'] - 1) <= 1e-13
    return good


@pytest.mark.parametrize('assignment', ['cic', 'TSC'])
@pytest.mark.parametrize('N', [16, 32])
def test_particle_power_spectrum_against_the_oracle(gpu, N, assignment):
    from baryonification_amd import engine
    coords, mass, L = _particles()
    order = CO.ORDERS[assignment.lower()]
    nk = 12
    assert 0 < np.count_nonzero(~CO.kept(coords, L)) < 400
    ref = IO.particle_power_spectrum_ref(coords, mass, N, L, nk, order)
    got = engine.particle_power_spectrum(coords, mass, N, L, Nk=nk, assignment=assignment)
    good = _check_particles(got, ref)
    assert np.abs(got['pk'][good] / got['pk_grid1'][good] - 1).max() > 1e-3
    # CUDA tensors, analysed where they lie
    dc, dm = [_dev(c) for c in coords], _dev(mass)
    on_dev = engine.particle_power_spectrum(dc, dm, N, L, Nk=nk, assignment=assignment)
    _check_particles(on_dev, ref)
    assert all(np.array_equal(d.cpu().numpy(), c) for d, c in zip(dc, coords))
    # unit masses
    _check_particles(engine.particle_power_spectrum(dc, None, N, L, Nk=nk, assignment=assignment),
                     IO.particle_power_spectrum_ref(coords, None, N, L, nk, order))
    # one grid: the windowed auto spectrum of make_map's grid, in both keys
    single = engine.particle_power_spectrum(coords, mass, N, L, Nk=nk, assignment=assignment, interlace=False)
    _check_particles(single, IO.particle_power_spectrum_ref(coords, mass, N, L, nk, order, interlace=False))
    assert np.array_equal(single['pk'], single['pk_grid1'], equal_nan=True)
    grid = _snapshot(coords, mass, L).make_map(N, assignment)
    x = engine.cross_power_spectrum(grid, grid, L, nk, window=order)
    assert np.abs(single['pk'][good] / x['paa'][good] - 1).max() <= 1e-12
    assert np.abs(got['pk_grid1'][good] / x['paa'][good] - 1).max() <= 1e-12
    # normalize and subtract_shot_noise, by their definitions
    norm = L ** 3 / got['mass'] ** 2
    n_ = engine.particle_power_spectrum(coords, mass, N, L, Nk=nk, assignment=assignment, normalize=True)
    s_ = engine.particle_power_spectrum(coords, mass, N, L, Nk=nk, assignment=assignment, subtract_shot_noise=True)
    b_ = engine.particle_power_spectrum(dc, dm, N, L, Nk=nk, assignment=assignment, normalize=True, subtract_shot_noise=True)
    for key in ('pk', 'pk_grid1'):
        scale = ref[key][good]
        assert (np.abs(n_[key][good] - got[key][good] * norm) <= 1e-10 * scale * norm).all()
        assert (np.abs(s_[key][good] - (got[key][good] - got['shot_noise'])) <= 1e-10 * scale).all()
        assert (np.abs(b_[key][good] - (got[key][good] - got['shot_noise']) * norm) <= 1e-10 * scale * norm).all()
    assert abs(n_['shot_noise'] / (got['shot_noise'] * norm) - 1) <= 1e-13 and s_['shot_noise'] == got['shot_noise'] and n_['mass'] == got['mass']


# --------------------------------------------------------------------------------------------- 7. the snapshot
def test_snapshot_power_spectrum(gpu):
    from baryonification_amd import engine
    coords, mass, L = _particles()
    snap = _snapshot(coords, mass, L)
    for kw in (dict(), dict(assignment='cic', interlace=False), dict(Nk=9, normalize=True, subtract_shot_noise=True)):
        got = snap.power_spectrum(16, **kw)
        want = engine.particle_power_spectrum(coords, mass, 16, L, **kw)
        good = want['counts'] > 0
        assert np.array_equal(got['counts'], want['counts']) and got['mass'] == want['mass'] and got['shot_noise'] == want['shot_noise']
        for key in ('k', 'pk', 'pk_grid1'):
            assert (np.abs(got[key][good] - want[key][good]) <= 1e-12 * (np.abs(want[key][good]) + want['shot_noise'])).all(), key
    assert got['k'].size == 9 and snap.power_spectrum(16)['k'].size == 180
    with pytest.raises(ValueError, match="3-D"):
        _snapshot(coords, mass, L, flat=True).power_spectrum(16)


# --------------------------------------------------------------------------------------------- 8. the tiled form end to end
def test_a_million_particles_take_the_tiled_deposits(gpu, monkeypatch):
    """n = 2^20 at N = 64 with no environment override: both deposits take the tile-owned form"""
    from baryonification_amd import engine
    monkeypatch.delenv('BFGX_DEPOSIT', raising=False)
    rng = np.random.default_rng(20)
    L, N, nk, n = L_ODD, 64, 31, 1 << 20
    coords = [rng.uniform(0.0, L, n) for _ in range(3)]
    mass = rng.uniform(0.5, 2.0, n)
    ref = IO.particle_power_spectrum_ref(coords, mass, N, L, nk, 3)
    got = engine.particle_power_spectrum([_dev(c) for c in coords], _dev(mass), N, L, Nk=nk, assignment='tsc')
    _check_particles(got, ref)


# --------------------------------------------------------------------------------------------- 9. what the feature is for
@pytest.mark.parametrize('assignment', ['cic', 'tsc'])
def test_one_particle_is_five_times_closer_to_flat(gpu, assignment):
    """one unit particle has |F|^2 = 1 in every mode.  The oracle alone gives max |pk - 1| = 0.110 against 1.015 for the deconvolved
    single grid with CIC, 0.0153 against 0.316 with TSC: margins of 9 and 20 over the factor 5 asked for"""
    from baryonification_amd import engine
    L, N, nk = 7.3, 16, 8
    coords = [np.array([f * L]) for f in (0.2137, 0.6181, 0.9049)]
    got = engine.particle_power_spectrum(coords, None, N, L, Nk=nk, assignment=assignment)
    good = got['counts'] > 0
    e, e1 = np.abs(got['pk'][good] - 1).max(), np.abs(got['pk_grid1'][good] - 1).max()
    print('%s: max |pk - 1| = %.4g, max |pk_grid1 - 1| = %.4g' % (assignment, e, e1))
    assert good.sum() >= 7 and e <= e1 / 5
    assert got['mass'] == 1.0 and got['shot_noise'] == 1.0
