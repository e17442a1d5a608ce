"""GPU checks of what the call scaffold of the synchronous host entries (csrc/bfgx_hostcall.hpp) can get wrong and the rest of the suite
does not pin: arguments that are read and written, in-place and empty requests, optional arguments, n = 0 and several results.  Every
result is compared exactly, with numpy or with the _device entry of the same operation; the inputs are small integers and dyadic
fractions where sums are formed, so that no order of summation rounds (the two atomic sums of the power spectrum excepted: see there)."""
import ctypes as C

import numpy as np
import pytest

from baryonification_amd import _lib, engine

pytestmark = pytest.mark.gpu

SENTINEL = -7.5


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())


def _ok(rc):
    _lib.check(rc)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sync():
    import torch
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ in and out
def test_regrid_pixels_adds_to_a_grid_that_is_not_zero(gpu):
    L = _lib.load()
    pos = np.array([[1.25, 2.5], [4.75, 0.25], [1.25, 2.5]])          # (the last cell wraps; two points share their cells)
    val = np.array([3.0, 5.0, 7.0])
    start = (np.arange(25.0) - 7.0).reshape(5, 5) / 4
    zero, grid = np.zeros((5, 5)), start.copy()
    _ok(L.bfgx_regrid_pixels(0, 2, 5, 3, _p(pos), _p(val), _p(zero)))
    _ok(L.bfgx_regrid_pixels(0, 2, 5, 3, _p(pos), _p(val), _p(grid)))
    # the unit cell displaced to s overlaps cell int(s) by int(s) + 1 - s and the next one (periodic) by the rest; positions are (x, y) =
    # (second, first) array axis
    ref = np.zeros((5, 5))
    for (x, y), v in zip(pos, val):
        for i, wy in ((int(y), int(y) + 1 - y), (int(y) + 1, y - int(y))):
            for j, wx in ((int(x), int(x) + 1 - x), (int(x) + 1, x - int(x))):
                ref[i % 5, j % 5] += wy * wx * v
    assert ref.sum() == val.sum() and np.count_nonzero(ref) == 8
    assert np.array_equal(zero, ref) and np.array_equal(grid, start + ref)


def test_scatter_add_adds_to_a_map_that_is_not_zero(gpu):
    L = _lib.load()
    start = np.arange(12.0) + 0.5
    vals = np.array([2.0, -3.0])
    pix = np.array([[0, 5, 11, -1], [5, 5, -12, 3]], dtype=np.int64)   # (negative indices count from the end; repeats add up)
    w = np.array([[0.5, 0.25, 0.125, 0.125], [0.25, 0.25, 0.25, 0.25]])
    hmap = start.copy()
    _ok(L.bfgx_hpx_scatter_add(0, 12, _p(hmap), 2, _p(vals), _p(pix), _p(w)))
    ref = start.copy()
    np.add.at(ref, pix.ravel(), (vals[:, None] * w).ravel())
    assert np.array_equal(hmap, ref) and not np.array_equal(hmap, start)


def test_math_probe_mul_add_nc_reads_its_third_argument(gpu):
    L = _lib.load()
    a, b, c = np.array([3.0, 1 + 2.0 ** -30, -2.5]), np.array([7.0, 1 - 2.0 ** -30, 4.0]), np.array([0.5, -1.0, 10.0])
    out = c.copy()
    _ok(L.bfgx_math_probe(0, _lib.MATH_FN['mul_add_nc'], 3, _p(a), _p(b), _p(out), None))
    assert np.array_equal(out, a * b + c)


# ------------------------------------------------------------------------------------------------------------------ in place and empty
def _alm(rng, lmax):
    na = engine.sht_alm_size(lmax, lmax)
    l = np.concatenate([np.arange(m, lmax + 1) for m in range(lmax + 1)])          # healpy order: m-major
    return rng.normal(size=na) + 1j * rng.normal(size=na), l


def test_almxfl_in_place_and_with_an_empty_filter(gpu):
    L = _lib.load()
    lmax = 3
    alm, l = _alm(np.random.default_rng(1), lmax)
    fl = np.array([2.0, -0.5, 3.0])                                                # (shorter than lmax + 1: fl[3] counts as 0)
    f = np.where(l < fl.size, fl[np.minimum(l, fl.size - 1)], 0.0)
    ref = (alm.view(np.float64).reshape(-1, 2) * f[:, None]).ravel().view(np.complex128)
    out = np.full(alm.size, SENTINEL + 0j)
    _ok(L.bfgx_sht_almxfl(0, lmax, lmax, fl.size, _p(fl), _p(alm), _p(out)))
    assert np.array_equal(out, ref)
    same = alm.copy()
    _ok(L.bfgx_sht_almxfl(0, lmax, lmax, fl.size, _p(fl), _p(same), _p(same)))
    assert np.array_equal(same, ref)
    _ok(L.bfgx_sht_almxfl(0, lmax, lmax, 0, _p(fl), _p(alm), _p(out)))
    assert np.array_equal(out, np.zeros(alm.size, dtype=np.complex128))


# ------------------------------------------------------------------------------------------------------------------ optional arguments
def test_interp_weights_by_pixel_and_by_angles(gpu):
    import torch
    L = _lib.load()
    nside, n = 2, 3
    theta, phi = np.array([0.3, 1.5, 2.9]), np.array([0.1, 3.0, 6.0])
    ipix = np.array([0, 17, 47], dtype=np.int64)
    for th, ph, ip in ((theta, phi, None), (None, None, ipix)):
        pix, w = np.full(4 * n, -1, dtype=np.int64), np.full(4 * n, SENTINEL)
        _ok(L.bfgx_hpx_interp_weights(0, nside, 0, n, _p(th), _p(ph), _p(ip), _p(pix), _p(w)))
        dpix, dw = torch.full((4 * n,), -1, dtype=torch.int64, device='cuda'), torch.full((4 * n,), SENTINEL, dtype=torch.float64, device='cuda')
        dth, dph, dip = (None if a is None else _dev(a) for a in (th, ph, ip))
        _ok(L.bfgx_hpx_interp_weights_device(0, None, nside, 0, n, _p(dth), _p(dph), _p(dip), _p(dpix), _p(dw)))
        _sync()
        assert np.array_equal(pix, dpix.cpu().numpy()) and np.array_equal(w, dw.cpu().numpy())
        assert pix.min() >= 0 and pix.max() < 48 and np.abs(w.reshape(4, n).sum(0) - 1).max() < 1e-13


def test_alm2cl_with_and_without_the_second_alm(gpu):
    L = _lib.load()
    lmax = 3
    rng = np.random.default_rng(2)
    a, _ = _alm(rng, lmax)
    b, _ = _alm(rng, lmax)
    for second in (None, b):
        cl = np.full(lmax + 1, SENTINEL)
        _ok(L.bfgx_sht_alm2cl(0, lmax, lmax, lmax, _p(a), _p(second), _p(cl)))
        ref = engine.alm2cl_device(_dev(a), None if second is None else _dev(second), lmax, lmax, lmax).cpu().numpy()
        assert np.array_equal(cl, ref)
    assert not np.array_equal(cl, engine.sht_alm2cl_host(a, None, lmax, lmax, lmax))


@pytest.fixture(scope='module')
def anafast_case(gpu):
    """two maps of nside 4 and, from the _device entries, their alm (lmax = mmax = 11, 3 iterations) and spectra"""
    nside, lmax = 4, 11
    rng = np.random.default_rng(3)
    m1, m2 = rng.normal(size=12 * nside * nside), rng.normal(size=12 * nside * nside)
    plan = engine.sht_plan(nside, lmax, lmax)
    a1, a2 = plan.map2alm_device(_dev(m1), iter=3), plan.map2alm_device(_dev(m2), iter=3)
    return dict(nside=nside, lmax=lmax, m1=m1, m2=m2, a1=a1.cpu().numpy(), a2=a2.cpu().numpy(),
                cl_auto=plan.alm2cl_device(a1).cpu().numpy(), cl_cross=plan.alm2cl_device(a1, a2).cpu().numpy())


@pytest.mark.parametrize('second', [False, True])
@pytest.mark.parametrize('want1,want2', [(False, False), (True, False), (False, True), (True, True)])
def test_anafast_optional_map_and_alm_results(anafast_case, second, want1, want2):
    L = _lib.load()
    c = anafast_case
    nside, lmax = c['nside'], c['lmax']
    cl = np.full(lmax + 1, SENTINEL)
    o1, o2 = np.full(c['a1'].size, SENTINEL + 0j), np.full(c['a1'].size, SENTINEL + 0j)
    _ok(L.bfgx_sht_anafast(0, nside, lmax, lmax, 3, _p(c['m1']), _p(c['m2']) if second else None, _p(cl), _p(o1) if want1 else None,
                           _p(o2) if want2 else None))
    assert np.array_equal(cl, c['cl_cross'] if second else c['cl_auto'])
    assert np.array_equal(o1, c['a1']) if want1 else np.all(o1 == SENTINEL)
    assert np.array_equal(o2, c['a2']) if (want2 and second) else np.all(o2 == SENTINEL)     # (no second map: no second alm)


def test_deposit_particles_2d_without_z_and_mass(gpu):
    L = _lib.load()
    n_grid = 4
    edges = np.array([0.0, 1.0, 2.5, 3.0, 4.0])
    x, y = np.array([0.5, 2.5, 2.6, 4.0, -0.1]), np.array([3.5, 0.0, 0.1, 4.0, 1.0])     # (the last edge counts; the last particle is outside)
    out = np.full((n_grid, n_grid), SENTINEL)
    _ok(L.bfgx_deposit_particles(0, 2, x.size, _p(x), _p(y), None, None, n_grid, _p(edges), _p(out)))
    assert np.array_equal(out, np.histogramdd(np.stack([x, y], axis=1), bins=(edges, edges))[0])
    assert out.sum() == 4


# ------------------------------------------------------------------------------------------------------------------ n == 0
def test_nothing_to_do_leaves_the_results_untouched(gpu):
    L = _lib.load()
    maps, none_f, none_i = np.arange(12.0), np.zeros(1), np.zeros(4, dtype=np.int64)
    out = np.full(3, SENTINEL)
    _ok(L.bfgx_hpx_interp_val(0, 1, 0, 1, 1, _p(maps), 0, _p(none_f), _p(none_f), _p(out)))
    assert np.all(out == SENTINEL)
    nb = np.full(8, -9, dtype=np.int64)
    _ok(L.bfgx_hpx_neighbours(0, 1, 0, 0, _p(none_i), _p(nb)))
    assert np.all(nb == -9)
    hmap = np.full(12, SENTINEL)
    _ok(L.bfgx_hpx_scatter_add(0, 12, _p(hmap), 0, _p(none_f), _p(none_i), _p(none_f)))
    assert np.all(hmap == SENTINEL)


# ------------------------------------------------------------------------------------------------------------------ several results
def test_displacement_rows_returns_both_results(gpu):
    L = _lib.load()
    r = np.array([1.0, 2.0, 4.0])
    M_dmo, M_dmb = np.array([1.0, 2.0, 4.0]), np.array([1.0, 2.5, 4.5])
    d, status = np.full(3, SENTINEL), np.full(1, -9, dtype=np.int32)
    _ok(L.bfgx_displacement_rows(0, 1, 3, _p(r), _p(M_dmo), _p(M_dmb), _p(d), _p(status)))
    # three nodes are not "more than 5": the row is all zeros and its status says so (2)
    assert np.array_equal(d, np.zeros(3)) and status[0] == 2


def test_power_spectrum_three_results_match_the_device_entry(gpu):
    """The counts exactly.  The two sums are atomic additions of positive terms (|F|^2 and |k|) in an order that differs from run to
    run: each of the two runs is within n eps of the exact sum, n <= 8^3 terms per bin, so they agree within 2 * 512 * 2^-53 relative."""
    import torch
    L = _lib.load()
    N, nk, box = 8, 4, 100.0
    Map = np.random.default_rng(4).poisson(4.0, (N, N, N)).astype(np.float64)
    pk, kc, cnt = np.full(nk, SENTINEL), np.full(nk, SENTINEL), np.full(nk, -9, dtype=np.int64)
    _ok(L.bfgx_power_spectrum(0, N, _p(Map), box, nk, _p(pk), _p(kc), _p(cnt)))
    work = torch.empty(engine.power_spectrum_work_doubles(N), dtype=torch.float64, device='cuda')
    sp, sk = torch.zeros(nk, dtype=torch.float64, device='cuda'), torch.zeros(nk, dtype=torch.float64, device='cuda')
    sc = torch.zeros(nk, dtype=torch.int64, device='cuda')
    dmap = _dev(Map)
    engine.power_spectrum_device(dmap.data_ptr(), N, box, nk, work.data_ptr(), sp.data_ptr(), sk.data_ptr(), sc.data_ptr())
    _sync()
    sp, sk, sc = sp.cpu().numpy(), sk.cpu().numpy(), sc.cpu().numpy()
    assert np.array_equal(cnt, sc) and np.all(sc > 0) and sc.max() <= N ** 3
    tol = 2 * N ** 3 * 2.0 ** -53
    for got, sums in ((pk, sp), (kc, sk)):
        ref = sums / sc
        print('power spectrum: max relative difference %.3e (bound %.3e)' % (np.abs(got / ref - 1).max(), tol))
        assert np.all(ref > 0) and np.abs(got / ref - 1).max() <= tol
