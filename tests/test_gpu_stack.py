"""GPU checks of bfg.Runners.MeasureProfilesShell (csrc/bfgx_stack.hpp): parity with the numpy oracle (stack_oracle.py), full-size counts
against the reference-pinned pair entry, the adjoint identity with the painter, host entry == device entry, and the lensing chain
kappa -> shear -> gamma_t on device tensors.

Bounds (derived, not measured).  Per (halo, bin) cell without an ambiguous pixel: npix, npix_shear equal;
    |sum - sum_o| <= 2 npix eps S,  S = sum |m| over the cell, eps = 2.2e-16  (two fp64 summations in any order);
    |sum_t - sum_t,o|, |sum_x - sum_x,o| <= (2 npix eps + 8 eps / theta_min) S_g,  S_g = sum (|g1| + |g2|)
(the tangent is a difference of unit vectors, so e^{2 i phi} carries an error of order eps / theta).  Cells with ambiguous pixels (within
1e-6 of a bin edge, within 1e-9 of the rim of the disc) get the same bounds widened by those pixels' count and sum |value|; their share is
asserted <= 1e-3."""
import ctypes as C

import numpy as np
import pytest

import stack_oracle as K
from oracle import oracle as O

pytestmark = pytest.mark.gpu

EPS = 2.2e-16


def _objects(cat, nside, hmap=None):
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    Catalog = bfg.utils.HaloLightConeCatalog(ra=cat['ra'], dec=cat['dec'], M=cat['M'], z=cat['z'], cosmo=syn.COSMO)
    Shell = bfg.utils.LightconeShell(map=np.zeros(12 * nside * nside) if hmap is None else hmap, cosmo=syn.COSMO)
    return Catalog, Shell


def _used(Catalog):
    return {k: np.array(Catalog.cat[k], dtype=np.float64) for k in ('M', 'z', 'ra', 'dec')}


def _compare(res, o, label, shear=True):
    """asserts the bounds of the module docstring; returns and prints the ambiguous share and the largest error / bound ratios"""
    get = lambda x: x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)               # noqa: E731
    amb = o['amb_n'] > 0
    share = float(amb.mean())
    stats = {'ambiguous_cell_share': share, 'cells': int(amb.size), 'pairs': o['pairs']}
    npix, s = get(res.npix), get(res.sum)
    assert npix.dtype == np.int64 and s.dtype == np.float64 and npix.shape == o['npix'].shape
    bound = 2 * o['npix'] * EPS * o['S'] + o['amb_abs']
    err = np.abs(s - o['sum'])
    with np.errstate(divide='ignore', invalid='ignore'):
        stats['sum'] = float(np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))))
    if shear:
        ns, st, sx = get(res.npix_shear), get(res.sum_t), get(res.sum_x)
        with np.errstate(divide='ignore', invalid='ignore'):
            bg = (2 * o['npix_shear'] * EPS + 8 * EPS / o['theta_min']) * o['S_g']
            bg = np.where(o['npix_shear'] > 0, bg, 0.0) + o['amb_abs_g']
            for name, mine, ref in (('sum_t', st, o['sum_t']), ('sum_x', sx, o['sum_x'])):
                e = np.abs(mine - ref)
                stats[name] = float(np.nanmax(np.where(bg > 0, e / bg, np.where(e > 0, np.inf, 0.0))))
    print('%s: %s' % (label, stats))
    assert share <= 1e-3, stats
    assert np.array_equal(npix[~amb], o['npix'][~amb]) and np.all(np.abs(npix - o['npix']) <= o['amb_n']), label
    assert np.all(err <= bound), (label, stats)
    if shear:
        assert np.array_equal(ns[~amb], o['npix_shear'][~amb]) and np.all(np.abs(ns - o['npix_shear']) <= o['amb_n']), label
        assert np.all(np.abs(st - o['sum_t']) <= bg) and np.all(np.abs(sx - o['sum_x']) <= bg), (label, stats)
    return stats


PARITY = {
    # nside: (epsilon_max, edges in comoving Mpc, edges in r / R_j): 16 log-spaced bins; at 64 a pixel is 13 Mpc wide, at 1024 0.8 Mpc
    64: (250.0, np.geomspace(8.0, 800.0, 17), np.geomspace(6.6, 260.0, 17)),
    1024: (10.0, np.geomspace(0.25, 30.0, 17), np.geomspace(0.3, 10.5, 17)),
}


@pytest.mark.parametrize('nside', [64, 1024])
def test_parity_with_the_oracle(gpu, nside):
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    eps, edges_mpc, edges_scaled = PARITY[nside]
    if nside == 64:
        cat = syn.make_catalog(1000)
    else:                                                             # a fixed-seed sample of 20 000 of config 2's 1e6 halos
        full = syn.make_catalog(1_000_000)
        pick = np.sort(np.random.default_rng(20250107).choice(1_000_000, 20_000, replace=False))
        cat = {k: v[pick].copy() for k, v in full.items()}
    n = cat['M'].size
    ra_c, dec_c = K.hp.pix2ang(nside, np.array([12 * nside * nside // 3 + 17]), lonlat=True)
    cat['ra'][5], cat['dec'][5] = ra_c[0], dec_c[0]                   # a halo exactly on a pixel centre
    cat['M'][6] = 1e6                                                 # a disc far smaller than a pixel: no pixel centre inside
    cat['M'][7] = -3e13                                               # not a halo
    cat['M'][8] = 0.0
    Catalog, Shell = _objects(cat, nside, syn.make_map(nside))
    used = _used(Catalog)
    bg = O.Background.from_dict(syn.COSMO)
    d = K.discs(nside, used, eps, bg)
    rng = np.random.default_rng(99 + nside)
    npx = 12 * nside * nside
    m, g1, g2 = Shell.map.copy(), rng.normal(size=npx), rng.normal(size=npx)
    inside = d['pix'][d['inside']]                                    # a few bad pixels inside known discs
    m[rng.choice(inside, 40)] = K.UNSEEN
    m[rng.choice(inside, 10)] = np.nan
    g1[rng.choice(inside, 30)] = K.UNSEEN
    g2[rng.choice(inside, 30)] = np.inf
    for scaled, edges in ((False, edges_mpc), (True, edges_scaled)):
        o = K.measure(d, edges, m, (g1, g2), scaled)
        assert o['npix'][5].sum() > 0 and not o['npix'][6].any() and not o['npix'][7].any() and not o['npix'][8].any()
        assert o['npix'].sum() > 0.5 * o['pairs'] and o['npix_shear'].sum() < o['npix'].sum() + 40
        runner = bfg.Runners.MeasureProfilesShell(Catalog, Shell, eps, verbose=False, r_edges=edges, scaled=scaled, shear=(g1, g2))
        res = runner.process(map=m)
        assert isinstance(res.npix, np.ndarray) and res.npix.shape == (n, 16)
        _compare(res, o, 'parity nside %d scaled %s' % (nside, scaled))
        for row in (6, 7, 8):
            assert not res.npix[row].any() and not res.sum[row].any() and not res.npix_shear[row].any() and not res.sum_t[row].any()
        mean = res.mean
        assert np.array_equal(np.isnan(mean), res.npix == 0)
        # the scalar-only kernel writes the same scalar columns
        res1 = bfg.Runners.MeasureProfilesShell(Catalog, Shell, eps, verbose=False, r_edges=edges, scaled=scaled).process(map=m)
        assert res1.sum_t is None and np.array_equal(res1.npix, res.npix)
        _compare(res1, o, 'parity nside %d scaled %s, scalar only' % (nside, scaled), shear=False)
    # the pixel the halo sits on (below the first log-spaced edge above): counted in the scalar sums; it has no position angle, so it is left
    # out of the shear sums when the tangent vanishes exactly and enters them with an arbitrary angle when rounding leaves a tangent of 1e-17
    edges = [0.0, edges_mpc[0]]
    o = K.measure(d, edges, m, (g1, g2))
    res = bfg.Runners.MeasureProfilesShell(Catalog, Shell, eps, verbose=False, r_edges=edges, shear=(g1, g2)).process(map=m)
    assert o['npix'][5, 0] >= 1 and res.npix[5, 0] == o['npix'][5, 0] and res.npix_shear[5, 0] in (o['npix'][5, 0] - 1, o['npix'][5, 0])
    print('halo on a pixel centre: npix %d, npix_shear %d (oracle %d)' % (res.npix[5, 0], res.npix_shear[5, 0], o['npix_shear'][5, 0]))
    rest = np.arange(n) != 5
    assert np.array_equal(res.npix[rest][o['amb_n'][rest] == 0], o['npix'][rest][o['amb_n'][rest] == 0])


def _pair_counts(Catalog, nside, eps, want_H=False):
    """counts_host of bfgx_shell_pairs_begin(paint=1) and, on request, H[pix] = number of discs over each pixel (every pair value 1)"""
    from baryonification_amd import _lib
    from baryonification_amd import synthetic as syn
    from baryonification_amd.Runners._model import _placeholder_model

    class R(object):
        mass_def = None
        epsilon_max = eps
    import baryonification_amd as bfg
    R.mass_def = bfg.utils.MassDef(200, 'critical')
    model, keep = _placeholder_model(R, syn.COSMO)
    cols = [np.ascontiguousarray(Catalog.cat[k], dtype=np.float64) for k in ('M', 'z', 'ra', 'dec')]
    c, ckeep = _lib.make_catalog_host(*cols)
    lib = _lib.load()
    h = C.c_void_p()
    counts = np.zeros(cols[0].size, dtype=np.int64)
    _lib.check(lib.bfgx_shell_pairs_begin(C.byref(c), C.byref(model), nside, 1, 0, C.byref(h), counts.ctypes.data))
    H = None
    try:
        if want_H:
            vals = np.ones(max(int(counts.sum()), 1))
            H = np.zeros(12 * nside * nside)
            _lib.check(lib.bfgx_shell_pairs_apply(h, vals.ctypes.data, None, H.ctypes.data, 0, None))
    finally:
        lib.bfgx_shell_pairs_end(h)
    del keep, ckeep
    return counts, H


@pytest.mark.parametrize('nside', [1024, 2048])
def test_full_size_counts_and_adjoint_identity(gpu, nside):
    """config 2 (1e6 halos, NSIDE 1024) and config 3's NSIDE 2048, epsilon_max 10: every halo's pixel count equals the pair entry's, in one
    bin and in 16; at config 2 the sum over all cells of a Poisson map equals sum_pix H[pix] m[pix], H = discs over each pixel, to
    2 n_pairs eps relative (all terms >= 0)."""
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    eps = 10.0
    cat = syn.make_catalog(1_000_000)
    Catalog, Shell = _objects(cat, nside, np.ones(12 * nside * nside))
    counts, H = _pair_counts(Catalog, nside, eps, want_H=(nside == 1024))
    res = bfg.Runners.MeasureProfilesShell(Catalog, Shell, eps, verbose=False, r_edges=[0.0, 1e30]).process()
    assert res.npix.shape == (counts.size, 1) and np.array_equal(res.npix[:, 0], counts)
    assert np.array_equal(res.sum[:, 0], counts.astype(np.float64))
    edges = np.concatenate([[0.0], np.geomspace(0.3, 1e4, 16)])       # cover every disc (the largest reach ~ 30 comoving Mpc)
    res = bfg.Runners.MeasureProfilesShell(Catalog, Shell, eps, verbose=False, r_edges=edges).process()
    assert np.array_equal(res.npix.sum(1), counts) and np.count_nonzero(res.npix.sum(0)) >= 8
    print('nside %d: %d pairs, largest disc %d pixels, median %d' % (nside, counts.sum(), counts.max(), np.median(counts)))
    if H is not None:
        m = syn.make_map(nside)
        res = bfg.Runners.MeasureProfilesShell(Catalog, Shell, eps, verbose=False, r_edges=edges).process(map=m)
        lhs, rhs = float(res.sum.sum()), float(np.dot(H, m))
        print('adjoint identity: sum_jb sum = %.17g, sum_pix H m = %.17g, rel %.3g (bound %.3g)'
              % (lhs, rhs, abs(lhs - rhs) / rhs, 2 * counts.sum() * EPS))
        assert H.sum() == counts.sum()
        assert abs(lhs - rhs) <= 2 * counts.sum() * EPS * rhs


def test_measures_what_the_painter_painted(gpu):
    """one isolated massive halo painted with the closed-form table of synthetic.paint_table at NSIDE 1024: the measured mean profile equals
    the oracle's on the painted map, and (reported only) follows the table read at the pixel-weighted mean x of each bin"""
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    nside, eps = 1024, 8.0
    cat = {'M': np.array([8e14]), 'z': np.array([0.25]), 'ra': np.array([123.4]), 'dec': np.array([-31.2])}
    z, M, r = syn.table_grid(cat, Nz=4, NM=4, NR=400, R_min=1e-3, R_max=3e2, pad=0.05)
    cosmo = bfg.utils.Cosmology.from_dict(syn.COSMO)
    prof = bfg.utils.TabulatedProfile(None, cosmo)
    prof.set_table(z, M, r, syn.paint_table(z, M, r))
    Catalog, Shell = _objects(cat, nside)
    painter = bfg.Runners.PaintProfilesShell(Catalog, Shell, eps, prof, verbose=False)
    painter.acc_f64 = True
    painted = np.array(painter.process())
    assert np.count_nonzero(painted) > 100
    bgo = O.Background.from_dict(syn.COSMO)
    used = _used(Catalog)
    a, R, D, radius, bad = K.halo_scalars(used, eps, bgo)
    edges = np.geomspace(1.5, eps * R[0] / a[0] * 1.001, 17)
    res = bfg.Runners.MeasureProfilesShell(Catalog, bfg.utils.LightconeShell(map=painted, cosmo=syn.COSMO), eps, verbose=False,
                                           r_edges=edges).process()
    d = K.discs(nside, used, eps, bgo)
    o = K.measure(d, edges, painted)
    _compare(res, o, 'painted halo', shear=False)
    assert np.count_nonzero(res.npix[0]) >= 14 and res.npix[0].sum() > 300
    # reported only: the table's closed form at the pixel-weighted mean x of each bin
    x = D[0] * d['dist'] / a[0]
    xo = K.measure(d, edges, np.bincount(d['pix'][d['inside']], weights=x[d['inside']], minlength=painted.size))
    xc = xo['mean'][0] / (R[0] / a[0])
    table = np.exp(-xc - 2.0 * np.log1p(xc))
    print('measured mean / table(mean x) per bin:', res.mean[0] / table)


def test_host_entry_equals_device_entry_and_the_plan_is_cached(gpu):
    import torch
    import baryonification_amd as bfg
    from baryonification_amd import _lib
    from baryonification_amd import synthetic as syn
    nside, eps = 256, 20.0
    cat = syn.make_catalog(5000, seed=31)
    rng = np.random.default_rng(8)
    npx = 12 * nside * nside
    m, g1, g2 = syn.make_map(nside), rng.normal(size=npx), rng.normal(size=npx)
    Catalog, Shell = _objects(cat, nside, m)
    edges = np.geomspace(1.0, 60.0, 17)
    runner = bfg.Runners.MeasureProfilesShell(Catalog, Shell, eps, verbose=False, r_edges=edges, shear=(g1, g2))
    host = runner.process()
    dev = torch.device('cuda', 0)
    tm, t1, t2 = (torch.from_numpy(x).to(dev) for x in (m, g1, g2))
    ondev = runner.process(map=tm, shear=(t1, t2))
    for name in ('npix', 'sum', 'npix_shear', 'sum_t', 'sum_x', 'mean', 'mean_t'):
        assert getattr(ondev, name).is_cuda and getattr(ondev, name).shape == (5000, 16), name
    torch.cuda.synchronize()
    # the same pixels in the same cells; the sums within two fp64 summations in any order (the bounds of the module docstring, the host
    # result in the oracle's place: no pixel is ambiguous between two runs of one kernel)
    assert np.array_equal(ondev.npix.cpu().numpy(), host.npix) and np.array_equal(ondev.npix_shear.cpu().numpy(), host.npix_shear)
    assert np.all(np.abs(ondev.sum.cpu().numpy() - host.sum) <= 2 * host.npix * EPS * host.sum)         # (m >= 0: S = sum)
    S_g = bfg.Runners.MeasureProfilesShell(Catalog, Shell, eps, verbose=False, r_edges=edges).process(map=np.abs(g1) + np.abs(g2)).sum
    bound = 2 * host.npix_shear * EPS * S_g
    assert np.all(np.abs(ondev.sum_t.cpu().numpy() - host.sum_t) <= bound) and np.all(np.abs(ondev.sum_x.cpu().numpy() - host.sum_x) <= bound)
    st = ondev.stack(select=torch.arange(100, device=dev))
    assert st['mean'].is_cuda and np.allclose(st['mean'].cpu().numpy(), host.stack(select=np.arange(100))['mean'], rtol=1e-12, equal_nan=True)
    # a second process() on the same runner allocates no new device memory: the plan and its buffers are cached
    lib = _lib.load()
    before, reserved = lib.bfgx_debug_alloc_count(), torch.cuda.memory_reserved()
    for _ in range(2):
        again = runner.process()
        runner.process(map=tm, shear=(t1, t2))
    torch.cuda.synchronize()
    assert lib.bfgx_debug_alloc_count() == before
    assert np.array_equal(again.npix, host.npix)
    del reserved


def test_lensing_chain_on_device_tensors(gpu):
    """baryonified shell -> kappa -> map2alm -> E -> alm2map_spin -> gamma_t(R) around the halos, on device tensors end to end, against the
    oracle fed the same shear maps (NSIDE 256)"""
    import torch
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    from baryonification_amd import utils as U
    nside, eps, lmax = 256, 20.0, 512
    cat = syn.make_catalog(2000, seed=77)
    z, M, r = syn.table_grid(cat, Nz=5, NM=6, NR=96, R_min=1e-3, R_max=1e3, pad=1e-9)
    cosmo = bfg.utils.Cosmology.from_dict(syn.COSMO)
    model = bfg.Profiles.Baryonification2D(None, None, cosmo, epsilon_max=eps)
    model.set_table(z, M, r, syn.displacement_table(z, M, r))
    Catalog, Shell = _objects(cat, nside, syn.make_map(nside))
    new_map = np.array(bfg.Runners.BaryonifyShell(Catalog, Shell, eps, model, verbose=False).process())
    dev = torch.device('cuda', 0)
    kappa = torch.from_numpy(new_map / new_map.mean() - 1.0).to(dev)
    klm = U.map2alm(kappa, lmax=lmax, iter=0)
    ell = np.concatenate([np.arange(m_, lmax + 1) for m_ in range(lmax + 1)]).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        fac = np.where(ell >= 2, np.sqrt((ell + 2) * (ell - 1) / (ell * (ell + 1))), 0.0)
    elm = klm * torch.from_numpy(fac).to(dev)
    g = U.alm2map_spin([elm, 0 * elm], nside, 2, lmax)
    assert g.is_cuda and g.shape == (2, 12 * nside * nside)
    edges = np.geomspace(1.0, 40.0, 17)                # (every bin holds pixels of some halo: the largest disc reaches 46 comoving Mpc)
    runner = bfg.Runners.MeasureProfilesShell(Catalog, Shell, eps, verbose=False, r_edges=edges)
    res = runner.process(map=kappa, shear=(g[0], g[1]))
    assert res.sum_t.is_cuda and res.npix.is_cuda
    d = K.discs(nside, _used(Catalog), eps, O.Background.from_dict(syn.COSMO))
    o = K.measure(d, edges, kappa.cpu().numpy(), (g[0].cpu().numpy(), g[1].cpu().numpy()))
    _compare(res, o, 'lensing chain nside 256')
    stacked = res.stack()
    assert torch.isfinite(stacked['mean_t']).all()
    print('stacked gamma_t:', stacked['mean_t'].cpu().numpy())
