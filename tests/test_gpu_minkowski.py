"""GPU derivatives and Minkowski functionals (ShtPlan.alm2map_der_device, bfgx_mapstats_minkowski_device;
baryonification_amd.utils.alm2map_der1 / alm2map_der2 / minkowski_*) against the numpy restatements of minkowski_oracle.py.

Bounds.  Derivative maps: 1e-11 of each map's own maximum, what test_gpu_sht_spin.py holds the spin synthesis to.  Pixel counts, n
and v0: exact.  The per-bin sums: 1e-11 x the sum of the absolute terms of the bin.  The kernel rounds every product of a term as
numpy does (no fused multiply-add), so only the order of the additions differs, which moves a sum of n terms by at most
n eps = 5.5e-12 of their absolute sum for n <= 49 152."""
import functools

import numpy as np
import pytest

import minkowski_oracle as K
import sht_oracle as O

pytestmark = pytest.mark.gpu

UNSEEN = O.UNSEEN


def _random_alm(lmax, mmax, seed):
    rng = np.random.default_rng(seed)
    n = O.alm_size(lmax, mmax)
    alm = rng.normal(size=n) + 1j * rng.normal(size=n)
    return alm / (1.0 + K.ell(lmax, mmax))                                          # a red spectrum: the maps are not pure pixel noise


# ------------------------------------------------------------------------------------------------------- 1. derivatives
@pytest.mark.parametrize('nside,lmax,mmax', [(1, 2, 2), (2, 5, 5), (8, 23, 23), (8, 5, 3)])
def test_derivatives_match_oracle(gpu, nside, lmax, mmax):
    import torch
    from baryonification_amd import utils as U
    alm = _random_alm(lmax, mmax, 10 * nside + mmax)
    ref = K.derivatives(alm, nside, lmax, mmax)
    spin = K.derivatives(alm, nside, lmax, mmax, spin_form=True)
    kw = {} if (lmax, mmax) == (3 * nside - 1, 3 * nside - 1) and nside > 1 else {'lmax': lmax, 'mmax': mmax}
    d2 = U.alm2map_der2(alm, nside, **kw)
    s2 = U.alm2map_der2(alm, nside, spin_form=True, **kw)
    d1 = U.alm2map_der1(alm, nside, **kw)
    npix = 12 * nside * nside
    assert d2.dtype == s2.dtype == d1.dtype == np.float64 and d2.shape == s2.shape == (6, npix) and d1.shape == (3, npix)
    for got, want, name in ((d2, ref, 'der2'), (s2, spin, 'spin form')):
        for a in range(6):
            err = np.abs(got[a] - want[a]).max() / np.abs(want[a]).max()
            assert err <= 1e-11, (name, a, err)
    assert np.array_equal(d1, d2[:3]) and np.array_equal(s2[:3], d2[:3])
    t = torch.from_numpy(alm).cuda()
    for got, want in ((U.alm2map_der1(t, nside, **kw), d1), (U.alm2map_der2(t, nside, **kw), d2),
                      (U.alm2map_der2(t, nside, spin_form=True, **kw), s2)):
        assert got.is_cuda and got.cpu().numpy().tobytes() == want.tobytes()


def test_derivatives_below_the_spins(gpu):
    """lmax 0 and 1: no spin-1 / spin-2 synthesis exists; the gradient / the trace-free Hessian are 0"""
    from baryonification_amd import utils as U
    for lmax in (0, 1):
        alm = _random_alm(lmax, lmax, lmax)
        ref = K.derivatives(alm, 2, lmax, lmax, spin_form=True)
        got = U.alm2map_der2(alm, 2, lmax=lmax, spin_form=True)
        assert np.abs(got - ref).max() <= 1e-11 * np.abs(ref[0]).max() and not got[4:].any() and (lmax == 1 or not got[1:3].any())


# ---------------------------------------------------------------------------------------------- 2. the kernel on identical inputs
@functools.lru_cache(maxsize=None)
def _stack(nside):
    """an oracle-made derivative stack [u, u_t, u_p, u;tt, u;tp, u;pp] of a random band-limited map (lmax <= 24 keeps numpy quick)"""
    lmax = min(3 * nside - 1, 24)
    return K.derivatives(_random_alm(lmax, lmax, nside), nside, lmax, lmax)                # shared: _cases copies before it plants values


def _cases(nside, nb):
    """(ders, edges, mask) variants: clean, masked, and with bad values, pixels on the edges and a block without gradient"""
    rng = np.random.default_rng(1000 * nside + nb)
    d = _stack(nside)
    npix = d.shape[1]
    edges = np.linspace(*np.quantile(d[0], [0.1, 0.9]), nb + 1)
    mask = rng.random(npix) < 0.67
    dirty = d.copy()
    pick = lambda k: rng.choice(npix, size=min(npix, k), replace=False)
    for comp, val in ((0, UNSEEN), (0, np.nan), (1, np.inf), (3, np.nan), (4, -np.inf), (5, np.nan)):
        dirty[comp, pick(max(1, npix // 40))] = val
    dirty[2, pick(1)] = UNSEEN                                                     # in a derivative UNSEEN is a finite value: the pixel stays
    on = pick(6)
    dirty[0, on] = [edges[0], edges[nb], edges[nb // 2], edges[0], edges[nb], np.nextafter(edges[nb], -np.inf)][:on.size]
    flat = slice(npix // 3, npix // 3 + max(2, min(300, npix // 4)))
    dirty[1, flat] = 0.0
    dirty[2, flat] = 0.0
    return [(d, edges, None), (d, edges, mask), (dirty, edges, None), (dirty, edges, mask)]


def _check(got, ref, nb):
    assert isinstance(got['n'], int) and got['n'] == ref['n']
    assert got['count'].dtype == np.int64 and got['count'].shape == (nb,) and np.array_equal(got['count'], ref['count'])
    assert got['v0'].shape == (nb + 1,) and got['v1'].shape == got['v2'].shape == (nb,)
    if ref['n'] == 0:
        assert all(np.isnan(got[k]).all() for k in ('v0', 'v1', 'v2'))
        return
    assert np.array_equal(got['v0'], ref['v0'])
    # v1 and v2 are the sums over one positive factor each: compare them as sums
    for k, a, f in (('v1', 0, 4.0), ('v2', 1, 2.0 * np.pi)):
        norm = f * ref['n'] * ref['width']
        err = np.abs(got[k] * norm - ref['sums'][a])
        tol = 1e-11 * ref['scale'][a]                                                # (to v and back: 6 roundings, 1.3e-15 of it)
        assert (err <= tol).all(), (k, err.max(), (err / np.maximum(ref['scale'][a], 1e-300)).max())


@pytest.mark.parametrize('nside', [1, 2, 16, 64])
@pytest.mark.parametrize('nb', [1, 7, 512])
def test_kernel_matches_oracle(gpu, nside, nb):
    from baryonification_amd import utils as U
    for i, (d, edges, mask) in enumerate(_cases(nside, nb)):
        ref = K.minkowski(d, edges, mask)
        ref['width'] = np.diff(edges)
        _check(U.minkowski_from_derivatives(d, edges, mask=mask), ref, nb)
        if i == 3:
            with np.errstate(invalid='ignore', over='ignore'):
                sp = K.to_spin_form(d)
            _check(U.minkowski_from_derivatives(sp, edges, mask=mask, spin_form=True), ref, nb)
            if nside == 16:
                assert ref['below'] > 0 and ref['above'] > 0 and 0 < ref['n'] < d.shape[1] and ref['count'].sum() > 0
    d, edges, _ = _cases(nside, nb)[0]
    none = K.minkowski(d, edges, np.zeros(d.shape[1]))
    _check(U.minkowski_from_derivatives(d, edges, mask=np.zeros(d.shape[1])), none, nb)   # nothing left: n = 0, NaN
    assert none['n'] == 0


# --------------------------------------------------------------------------------------------------------- 3. determinism
def test_kernel_is_bit_reproducible(gpu):
    import torch
    from baryonification_amd import utils as U
    d, edges, mask = _cases(64, 7)[3]
    a = U.minkowski_from_derivatives(d, edges, mask=mask)
    b = U.minkowski_from_derivatives(d, edges, mask=mask)
    c = U.minkowski_from_derivatives(torch.from_numpy(d).cuda(), edges, mask=torch.from_numpy(mask).cuda())
    assert a['n'] == b['n'] == c['n'] and a['n'] > 0
    for k in ('count', 'v0', 'v1', 'v2'):
        assert c[k].is_cuda and a[k].tobytes() == b[k].tobytes() == c[k].cpu().numpy().tobytes(), k


# ------------------------------------------------------------------------------------------- 4. end to end, a known answer
def test_functionals_of_z_end_to_end(gpu):
    from baryonification_amd import utils as U
    nside = 8
    lmax = 3 * nside - 1
    z = K.pixel_angles(nside)[0]
    edges, zr = K.belt_edges(nside)
    v1, v2 = np.sqrt(1 - zr * zr) / 8, zr / (4 * np.pi)
    # the oracle's own pipeline: its u decides the bins, so no edge may be within rounding of a pixel value
    od = K.derivatives(O.map2alm(z, nside, lmax, lmax, 3), nside, lmax, lmax)
    assert np.abs(od[0][:, None] - edges[None, :]).min() >= 1e-6                      # (0.040 here; 1 / (3 nside) = 0.0417 for u = z itself)
    ora = K.minkowski(od, edges)
    got = U.minkowski_functionals(z, edges, lmax=lmax, iter=3)
    assert got['n'] == z.size and np.array_equal(got['count'], ora['count']) and (got['count'] == 4 * nside).all()
    assert np.array_equal(got['v0'], ora['v0'])
    e1, e2 = np.abs(got['v1'] - v1).max(), np.abs(got['v2'] - v2).max()
    print("minkowski_functionals(u = z, nside 8): max|v1 - closed form| = %.3e  max|v2 - closed form| = %.3e" % (e1, e2))
    # The oracle pipeline itself (sht_oracle.map2alm iter 3, oracle derivatives and binning, on the CPU) is off the closed forms by
    # 5.43e-4 in v1 and 1.88e-4 in v2: map2alm at lmax = 3 nside - 1 recovers u = z only to 4.7e-3 at nside 8.  The GPU is held to
    # 10 x those values.
    assert e1 <= 10 * 5.43e-4 and e2 <= 10 * 1.88e-4
    # Against the oracle pipeline only the rounding differs: 7 transforms of the analysis at <= 1e-11 of max|map| each, carried into
    # the second derivatives by factors up to lmax (lmax + 1) = 552, is 4e-8 of max|u| = 1; v1 and v2 are means of such terms / 3.
    o1, o2 = np.abs(got['v1'] - ora['v1']).max(), np.abs(got['v2'] - ora['v2']).max()
    print("                                     max|v1 - oracle pipeline| = %.3e  max|v2 - oracle pipeline| = %.3e" % (o1, o2))
    assert o1 <= 4e-8 and o2 <= 4e-8


# ------------------------------------------------------------------------------------------------- 5. shell_statistics
ARCMIN = np.pi / 180 / 60
SCALES = [0.0, 120 * ARCMIN]


def _shell_inputs():
    nside = 16
    rng = np.random.default_rng(16)
    npix = 12 * nside * nside
    kappa = rng.normal(size=npix) ** 2
    y = 0.5 * kappa + rng.normal(size=npix)
    y[rng.integers(0, npix, 20)] = UNSEEN
    return nside, np.stack([kappa, y]), rng.random(npix) < 0.8


def test_shell_statistics_with_mf_bins(gpu):
    import torch
    from baryonification_amd import utils as U
    nside, maps, mask = _shell_inputs()
    kw = dict(lmax=2 * nside, iter=1, order=3, mask=mask)
    bins = np.linspace(-1.0, 3.0, 12)
    plain = U.shell_statistics(maps, SCALES, peak_bins=bins, **kw)
    assert sorted(plain) == ['central', 'exponents', 'maxima', 'mean', 'minima', 'n']
    assert sorted(U.shell_statistics(maps, SCALES, **kw)) == ['central', 'exponents', 'mean', 'n']
    res = U.shell_statistics(maps, SCALES, peak_bins=bins, mf_bins=bins, **kw)
    assert sorted(res) == ['central', 'exponents', 'maxima', 'mean', 'minima', 'n', 'v0', 'v1', 'v2']
    for k in plain:                                                                  # what was there is unchanged, bit for bit
        assert k == 'exponents' or res[k].tobytes() == plain[k].tobytes(), k
    assert res['v0'].shape == (2, 2, 12) and res['v1'].shape == res['v2'].shape == (2, 2, 11)
    zeroed = np.where(mask, maps, 0.0)
    for s, scale in enumerate(SCALES):
        for k in range(2):
            one = U.minkowski_functionals(zeroed[k], bins, mask=mask, lmax=2 * nside, iter=1, fwhm=scale)
            for key in ('v0', 'v1', 'v2'):
                assert res[key][s, k].tobytes() == one[key].tobytes(), (key, s, k)
            assert np.isfinite(one['v1']).all() and one['n'] == (mask & K.M.good(maps[k])).sum()
    dev = U.shell_statistics(torch.from_numpy(maps).cuda(), SCALES, peak_bins=bins, mf_bins=bins,
                             **dict(kw, mask=torch.from_numpy(mask).cuda()))
    for k in ('n', 'mean', 'central', 'maxima', 'v0', 'v1', 'v2'):
        assert dev[k].is_cuda and dev[k].cpu().numpy().tobytes() == np.ascontiguousarray(res[k]).tobytes(), k


def test_shell_statistics_with_mf_bins_allocates_no_new_device_memory(gpu):
    import torch
    from baryonification_amd import utils as U
    nside, maps, mask = _shell_inputs()
    kw = dict(lmax=2 * nside, iter=1, mf_bins=np.linspace(-1.0, 3.0, 12), mask=mask)
    U.shell_statistics(maps, SCALES, **kw)
    torch.cuda.synchronize()
    before, reserved = torch.cuda.memory_allocated(), torch.cuda.memory_reserved()
    U.shell_statistics(maps, SCALES, **kw)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() <= before and torch.cuda.memory_reserved() == reserved
