"""interlace_oracle.py (the oracle of test_gpu_interlace.py) against hand-computed cases, and the parts of the feature that need no GPU:
the shifted weights at v = 0, v = L and one ulp below L, exact mass conservation, the shifted deposit against the unshifted oracle fed
moved coordinates, the reality of the combined field, the twisted route against the binned |C|^2, the argument checks of the new C
entries (made before any device call) and the ValueErrors of the Python surface."""
import ctypes as C

import numpy as np
import pytest

import deposit_cloud_oracle as CO
import interlace_oracle as IO
import xpk_oracle as X
from baryonification_amd import _lib, engine


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _aligned16(n_doubles):
    raw = np.zeros(n_doubles + 4)
    start = -(raw.ctypes.data // 8) % 2
    return raw[start:start + n_doubles]


# ------------------------------------------------------------------------------------------------- the shifted weights, by hand
def test_shifted_cic_weights_by_hand():
    N = 8
    below = np.nextafter(8.0, 0.0)                                         # 8 - 2^-50
    v = np.array([0.0, 8.0, below, 2.25, 7.5, -0.0])
    keep, cells, w = IO.shifted_weights(v, N, 8.0, 2)
    assert keep.all()
    assert cells.tolist() == [[0, 1], [0, 1], [7, 0], [2, 3], [7, 0], [0, 1]]            # v = L: i = N wraps to cell 0
    assert w.tolist() == [[1.0, 0.0], [1.0, 0.0], [2.0 ** -50, 1.0 - 2.0 ** -50], [0.75, 0.25], [0.5, 0.5], [1.0, 0.0]]
    # the unshifted grid puts the same particles half a cell lower: v = 2.25 there is 0.25 / 0.75 on cells 1, 2
    _, c0, w0 = CO.weights(np.array([2.25]), N, 8.0, 2)
    assert c0.tolist() == [[1, 2]] and w0.tolist() == [[0.25, 0.75]]
    # L = 4 on N = 8: s = 2
    _, cells, w = IO.shifted_weights(np.array([1.125, 4.0]), N, 4.0, 2)
    assert cells.tolist() == [[2, 3], [0, 1]] and w.tolist() == [[0.75, 0.25], [1.0, 0.0]]


def test_shifted_tsc_weights_by_hand():
    N = 8
    below = np.nextafter(8.0, 0.0)                                         # t2 = 8.5 - 2^-50 is a tie and rounds to the even 8.5: as v = L
    v = np.array([0.0, 8.0, below, 2.25, 2.5, 7.75])
    keep, cells, w = IO.shifted_weights(v, N, 8.0, 3)
    assert keep.all()
    assert cells.tolist() == [[7, 0, 1], [7, 0, 1], [7, 0, 1], [1, 2, 3], [2, 3, 4], [7, 0, 1]]
    centre = [0.125, 0.75, 0.125]
    assert w.tolist() == [centre, centre, centre, [0.03125, 0.6875, 0.28125], [0.5, 0.5, 0.0], [0.28125, 0.6875, 0.03125]]
    assert (w.sum(axis=1) == 1.0).all()
    assert IO.shifted_base_cell(v, N, 8.0, 3).tolist() == [0, 0, 0, 2, 3, 0]
    assert IO.shifted_base_cell(v, N, 8.0, 2).tolist() == [0, 0, 7, 2, 2, 7]


def test_dropped_particles_are_those_of_the_unshifted_grid():
    v = np.array([np.nan, -1.0, 9.0, np.inf, -np.inf, np.nextafter(8.0, 9.0), -5e-324, 8.0, 0.0, -0.0])
    for order in (2, 3):
        keep, cells, _ = IO.shifted_weights(v, 8, 8.0, order)
        assert keep.tolist() == CO.weights(v, 8, 8.0, order)[0].tolist() == [False] * 7 + [True] * 3
        assert cells.min() >= 0 and cells.max() <= 7
    x = np.array([1.0, 2.0, 3.0])
    got = IO.shifted_deposit([x, np.array([1.0, np.nan, 3.0]), x], None, 8, 8.0, 2)
    assert got.sum() == 2.0


# ------------------------------------------------------------------------------------------------- mass
@pytest.mark.parametrize('order', [2, 3])
@pytest.mark.parametrize('ndim,N', [(3, 1), (3, 2), (3, 17), (2, 65)])
def test_mass_is_conserved_exactly_on_the_lattice(ndim, N, order):
    rng = np.random.default_rng(N + order)
    p = rng.integers(0, 8 * N + 1, (3000, ndim)) / 8.0
    mass = rng.integers(1, 2048, 3000) / 1024.0
    coords = [p[:, a] for a in range(ndim)]
    for m in (mass, None):
        got = IO.shifted_deposit(coords, m, N, float(N), order)
        assert got.shape == (N,) * ndim and got.sum() == (3000.0 if m is None else mass.sum())
    assert np.abs(IO.shifted_deposit(coords, mass, N, float(N), order) - CO.deposit(coords, mass, N, float(N), order)).max() > 0 or N == 1


# ------------------------------------------------------------------------------------------------- against moved coordinates
@pytest.mark.parametrize('order', [2, 3])
@pytest.mark.parametrize('L', [250.0 / 3.0, 7.3])
def test_shifted_deposit_is_the_unshifted_one_of_moved_particles(L, order):
    """500 particles of mass 0.5 to 2 on N = 12: the shifted deposit against deposit_cloud_oracle.deposit of v + L / (2N), wrapped.  The
    two evaluate the same continuous weights at arguments that differ by the rounding of v + h and of the two products with s (at most
    3 N 2^-53 in t, slope <= 1), with at most 3 roundings per weight and 3 more in the product: per cell eps M, eps = (3 N + 12) 2^-53,
    plus the summation of k terms of absolute sum S on either side, 2 k 2^-53 (S + eps M); k, M over the cloud taken one cell wider"""
    rng = np.random.default_rng(7)
    N, n = 12, 500
    p = rng.uniform(0.0, L, (n, 3))
    p[:3] = [[0.0, L, 0.5 * L], [L, L, L], [np.nextafter(L, 0.0), 0.0, L - L / (2 * N)]]
    mass = rng.uniform(0.5, 2.0, n)
    h = L / (2 * N)
    moved = p + h
    moved = np.where(moved > L, moved - L, moved)
    coords, mcoords = [p[:, a] for a in range(3)], [moved[:, a] for a in range(3)]
    assert CO.kept(mcoords, L).all()
    got = IO.shifted_deposit(coords, mass, N, L, order)
    ref = CO.deposit(mcoords, mass, N, L, order)
    k = IO.shifted_deposit(coords, None, N, L, order, unit_weights=True, widen=1)
    S = IO.shifted_deposit(coords, mass, N, L, order)
    M = IO.shifted_deposit(coords, mass, N, L, order, unit_weights=True, widen=1)
    eps = (3.0 * N + 12.0) * 2.0 ** -53
    bound = 2.0 * k * 2.0 ** -53 * (S + eps * M) + eps * M
    err = np.abs(got - ref)
    print('L = %.4g order %d: max err %.3g, max err / bound %.3g' % (L, order, err.max(), (err / bound).max()))
    assert (err <= bound).all() and err.max() < 1e-13 and got.sum() > 0.99 * mass.sum()


# ------------------------------------------------------------------------------------------------- the combined field
def test_phi_table():
    for N in (8, 16, 64):
        phi = IO.phi_table(N)
        n = np.rint(np.fft.fftfreq(N) * N)
        assert phi[0] == 1.0 and phi[N // 2] == 1.0 and phi[N // 4] == complex(np.sqrt(0.5), np.sqrt(0.5))
        ok = np.arange(N) != N // 2
        assert np.abs(phi[ok] - np.exp(1j * np.pi * n[ok] / N)).max() < 3e-16
        assert np.array_equal(phi[1:N // 2], np.conj(phi[:N // 2:-1]))              # phi[-i] = conj(phi[i]): the combined field is real
        assert phi[1].imag > 0                                                     # +i: grid 2 lies half a cell ABOVE grid 1


@pytest.mark.parametrize('N', [8, 16])
def test_the_combined_field_is_real(N):
    rng = np.random.default_rng(N)
    m1, m2 = rng.poisson(4.0, (N, N, N)).astype(float), rng.poisson(4.0, (N, N, N)).astype(float)
    c = np.fft.ifftn(IO.combined(m1, m2))
    print('N = %d: max |imag| / max|map| = %.3g' % (N, np.abs(c.imag).max() / m1.max()))
    assert np.abs(c.imag).max() <= 1e-12 * max(m1.max(), m2.max())
    # with phi[N/2] = i instead, it is not
    phi = IO.phi_table(N)
    phi[N // 2] = 1j
    Phi = phi[:, None, None] * phi[None, :, None] * phi[None, None, :]
    bad = np.fft.ifftn(0.5 * (np.fft.fftn(m1) + Phi * np.fft.fftn(m2)))
    assert np.abs(bad.imag).max() > 1e-3


@pytest.mark.parametrize('p', [0, 2, 3])
@pytest.mark.parametrize('N,nk', [(8, 7), (16, 15), (16, 40)])
def test_the_twisted_route_gives_the_binned_combined_power(N, nk, p):
    rng = np.random.default_rng(10 * N + p)
    m1, m2 = rng.poisson(4.0, (N, N, N)).astype(float), rng.poisson(4.0, (N, N, N)).astype(float)
    ref = IO.interlaced_ref(m1, m2, 305.0, nk, p)
    got = IO.twisted_route(m1, m2, 305.0, nk, p)
    good = ref['counts'] > 0
    assert good.any() and np.array_equal(np.isnan(got), ~good)
    err = np.abs(got[good] - ref['pk'][good]) / (0.5 * (ref['paa'][good] + ref['pbb'][good]))
    print('N = %d nk = %d p = %d: %.3g' % (N, nk, p, err.max()))
    assert err.max() <= 1e-14
    assert np.array_equal(ref['pk_grid1'][good], X.cross_power_spectrum_ref(m1, m1, 305.0, nk, p)['paa'][good])


def test_one_particle_is_what_the_feature_is_for():
    """one unit particle has |F|^2 = 1 in every mode: the deconvolved single grid misses that by the aliased images, the interlaced pair
    by five times less (the figures of the issue: CIC 0.110 against 1.015, TSC 0.0153 against 0.316)"""
    L, N, nk = 7.3, 16, 8
    coords = [np.array([f * L]) for f in (0.2137, 0.6181, 0.9049)]
    for order, want, want1 in ((2, 0.110, 1.015), (3, 0.0153, 0.316)):
        r = IO.particle_power_spectrum_ref(coords, None, N, L, nk, order)
        good = r['counts'] > 0
        e, e1 = np.abs(r['pk'][good] - 1).max(), np.abs(r['pk_grid1'][good] - 1).max()
        print('order %d: %.4g against %.4g' % (order, e, e1))
        assert abs(e / want - 1) < 0.02 and abs(e1 / want1 - 1) < 0.02 and e <= e1 / 5
        assert r['mass'] == 1.0 and r['shot_noise'] == 1.0


def test_normalize_and_shot_noise_of_the_oracle():
    rng = np.random.default_rng(3)
    L, N = 10.0, 8
    coords = [rng.uniform(-0.5, L + 0.5, 300) for _ in range(3)]
    mass = rng.uniform(0.5, 2.0, 300)
    keep = CO.kept(coords, L)
    assert 0 < (~keep).sum() < 150
    a = IO.particle_power_spectrum_ref(coords, mass, N, L, 5, 3)
    b = IO.particle_power_spectrum_ref(coords, mass, N, L, 5, 3, normalize=True, subtract_shot_noise=True)
    assert a['mass'] == mass[keep].sum() and a['shot_noise'] == (mass[keep] ** 2).sum()
    norm = L ** 3 / a['mass'] ** 2
    assert np.allclose(b['pk'], (a['pk'] - a['shot_noise']) * norm, rtol=1e-14, equal_nan=True) and b['shot_noise'] == a['shot_noise'] * norm
    c = IO.particle_power_spectrum_ref(coords, mass, N, L, 5, 3, interlace=False)
    assert np.array_equal(c['pk'], c['pk_grid1'], equal_nan=True) and np.array_equal(c['pk_grid1'], a['pk_grid1'], equal_nan=True)


# ------------------------------------------------------------------------------------------------- the C entries' refusals
def _shifted(order=2, shift=1, ndim=3, n_grid=4, L=4.0, x='ok', out='ok'):
    """bfgx_deposit_cloud_shifted_device with host pointers in the device slots: the checks come before any device call"""
    xs = np.array([0.5]) if isinstance(x, str) else x
    o = np.full(64, -7.0) if isinstance(out, str) else out
    rc = _lib.load().bfgx_deposit_cloud_shifted_device(0, None, ndim, 1, _ptr(xs), _ptr(xs), _ptr(xs), None, n_grid, float(L), order, shift, _ptr(o))
    assert o is None or (o == -7.0).all()
    return rc, _lib.load().bfgx_last_error()


def _interlaced(n=8, L=100.0, nk=4, p=3, null=None):
    m, w = np.ones(8), _aligned16(64)
    args = [m, m, w] + [np.full(4, -7.0) for _ in range(3)] + [np.full(4, -7, dtype=np.int64)]
    if null is not None:
        args[null] = None
    rc = _lib.load().bfgx_interlaced_power_spectrum_device(0, None, n, _ptr(args[0]), _ptr(args[1]), float(L), nk, p, *[_ptr(a) for a in args[2:]])
    assert all((a == -7).all() for a in args[3:] if a is not None)
    return rc, _lib.load().bfgx_last_error()


def _particles(n_grid=8, L=100.0, order=3, interlace=1, nk=4, null=None, host=False):
    x, w = np.array([0.5]), _aligned16(64)
    outs = [np.full(4, -7.0) for _ in range(3)] + [np.full(4, -7, dtype=np.int64)]
    if host:
        args = [x, x, x, None] + outs
        if null is not None:
            args[null] = None
        rc = _lib.load().bfgx_particle_power_spectrum(0, 1, *[_ptr(a) for a in args[:4]], n_grid, float(L), order, interlace, nk, *[_ptr(a) for a in args[4:]])
    else:
        args = [x, x, x, None, w] + outs
        if null is not None:
            args[null] = None
        rc = _lib.load().bfgx_particle_power_spectrum_device(0, None, 1, *[_ptr(a) for a in args[:4]], n_grid, float(L), order, interlace, nk,
                                                            *[_ptr(a) for a in args[4:]])
    assert all((a == -7).all() for a in outs)
    return rc, _lib.load().bfgx_last_error()


def test_the_new_entries_are_declared_and_bound():
    L = _lib.load()
    for name, nargs in (('bfgx_deposit_cloud_shifted_device', 13), ('bfgx_interlaced_power_spectrum_device', 13),
                        ('bfgx_particle_power_spectrum_device', 17), ('bfgx_particle_power_spectrum', 15), ('bfgx_particle_power_spectrum_work_doubles', 1)):
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs
        assert list(getattr(L, name).argtypes) == list(_lib.SYMBOLS[name][1])
    for n in (8, 16, 64, 512):
        assert engine.particle_power_spectrum_work_doubles(n) == 2 * n ** 3 + engine.cross_power_spectrum_work_doubles(n)


def test_the_shifted_deposit_refuses_bad_arguments_before_any_device_call():
    for shift in (2, -1, 3):
        rc, msg = _shifted(shift=shift)
        assert rc == _lib.ERR_INVALID and b'shift' in msg, (shift, rc, msg)
    for order in (0, 1, 4):
        rc, msg = _shifted(order=order)
        assert rc == _lib.ERR_INVALID and b'CIC' in msg and b'TSC' in msg
    for kw in (dict(ndim=1), dict(ndim=4), dict(n_grid=0), dict(L=0.0), dict(L=float('inf'))):
        rc, msg = _shifted(**kw)
        assert rc == _lib.ERR_INVALID, (kw, rc, msg)
    rc, msg = _shifted(out=None)
    assert rc == _lib.ERR_INVALID and b'NULL' in msg
    rc, msg = _shifted(x=None)
    assert rc == _lib.ERR_INVALID and b'NULL' in msg
    if _lib.load().bfgx_device_count() == 0:
        for shift in (0, 1):
            assert _shifted(shift=shift)[0] == _lib.ERR_NO_DEVICE                 # good arguments: the next stop is the device


def test_the_spectrum_entries_refuse_bad_arguments_before_any_device_call():
    for f in (_interlaced, _particles, lambda **kw: _particles(host=True, **kw)):
        rc, msg = f(nk=0)
        assert rc == _lib.ERR_INVALID and b'1 <= nk <= 2048' in msg
        rc, msg = f(L=0.0)
        assert rc == _lib.ERR_INVALID and b'L > 0' in msg
    rc, msg = _interlaced(n=12)
    assert rc == _lib.ERR_UNSUPPORTED and b'8 <= n_grid <= 1024' in msg
    assert _interlaced(p=4)[0] == _lib.ERR_INVALID and _interlaced(p=-1)[0] == _lib.ERR_INVALID
    for host in (False, True):
        rc, msg2 = _particles(n_grid=12, host=host)
        assert rc == _lib.ERR_UNSUPPORTED and msg2 == msg                           # xpk_check_shape's words
        for order in (0, 1, 4):
            rc, m = _particles(order=order, host=host)
            assert rc == _lib.ERR_INVALID and b'CIC' in m and b'TSC' in m, (order, rc, m)
        for interlace in (2, -1):
            rc, m = _particles(interlace=interlace, host=host)
            assert rc == _lib.ERR_INVALID and b'interlace' in m
    for pos in range(7):
        rc, m = _interlaced(null=pos)
        assert rc == _lib.ERR_INVALID and b'NULL' in m, pos
    for pos in (0, 1, 2, 4, 5, 6, 7, 8):
        rc, m = _particles(null=pos)
        assert rc == _lib.ERR_INVALID and b'NULL' in m, pos
    for pos in (0, 1, 2, 4, 5, 6, 7):
        rc, m = _particles(null=pos, host=True)
        assert rc == _lib.ERR_INVALID and b'NULL' in m, pos
    if _lib.load().bfgx_device_count() == 0:
        assert _interlaced()[0] == _lib.ERR_NO_DEVICE and _particles()[0] == _lib.ERR_NO_DEVICE and _particles(host=True)[0] == _lib.ERR_NO_DEVICE


# ------------------------------------------------------------------------------------------------- the Python surface
def test_value_errors_of_the_python_surface():
    import torch
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    x = np.array([0.5, 1.5])
    with pytest.raises(ValueError, match="'ngp' has no interlaced form"):
        engine.particle_power_spectrum((x, x, x), None, 8, 8.0, assignment='ngp', interlace=True)
    with pytest.raises(ValueError, match="'cic' or 'tsc'"):
        engine.particle_power_spectrum((x, x, x), None, 8, 8.0, assignment='NGP', interlace=False)
    for bad in ('nope', 'none', 3, None):
        with pytest.raises(ValueError, match="assignment must be 'cic' or 'tsc'"):
            engine.particle_power_spectrum((x, x, x), None, 8, 8.0, assignment=bad)
    with pytest.raises(ValueError, match="3-D"):
        engine.particle_power_spectrum((x, x), None, 8, 8.0)
    with pytest.raises(ValueError, match="one length"):
        engine.particle_power_spectrum((x, x, x[:1]), None, 8, 8.0)
    with pytest.raises(ValueError, match="not some of each"):
        engine.particle_power_spectrum((x, x, torch.zeros(2, dtype=torch.float64)), None, 8, 8.0)
    with pytest.raises(NotImplementedError, match="8 <= n_grid <= 1024"):
        engine.particle_power_spectrum((x, x, x), None, 12, 8.0)
    with pytest.raises(ValueError, match="1 <= nk <= 2048"):
        engine.particle_power_spectrum((x, x, x), None, 8, 8.0, Nk=0)
    cube = np.zeros((16, 16, 16))
    with pytest.raises(ValueError, match="not one of each"):
        engine.interlaced_power_spectrum(cube, torch.zeros((16, 16, 16), dtype=torch.float64), 100.0)
    with pytest.raises(ValueError, match="cubic 3-D maps"):
        engine.interlaced_power_spectrum(np.zeros((16, 16)), np.zeros((16, 16)), 100.0)
    with pytest.raises(ValueError, match="one shape"):
        engine.interlaced_power_spectrum(cube, np.zeros((8, 8, 8)), 100.0)
    for w in ('nope', 4, -1, True, None):
        with pytest.raises(ValueError, match="window must be"):
            engine.interlaced_power_spectrum(cube, cube, 100.0, window=w)
    with pytest.raises(ValueError, match="CUDA float64 tensor"):
        t = torch.zeros((16, 16, 16), dtype=torch.float64)
        engine.interlaced_power_spectrum(t, t, 100.0)
    snap = bfg.utils.ParticleSnapshot(x=x, y=x, z=None, M=np.ones(2), L=8.0, redshift=0.0, cosmo=dict(syn.COSMO))
    with pytest.raises(ValueError, match="3-D"):
        snap.power_spectrum(8)
    snap3 = bfg.utils.ParticleSnapshot(x=x, y=x, z=x, M=np.ones(2), L=8.0, redshift=0.0, cosmo=dict(syn.COSMO))
    with pytest.raises(ValueError, match="no interlaced form"):
        snap3.power_spectrum(8, assignment='ngp')
