"""The fp64 series of the displacement kernels whose constant addends are held in registers and negated in the fma (KReg / fma_k in
bfgx_math.hpp: PMathE and PMath<double> of K1's pair phase), and the small-angle series of the regrid (K2).  What can go wrong there is a
swapped or mis-signed operand, a constant that is not what its step needs, a register that something between the top of the kernel and the
pair loop overwrites (which shows as two calls that differ), and the edges of each function's domain.  The shapes are the smallest that reach
them: one halo per call, so that every pixel receives exactly one pair and pix_offsets are deterministic to the bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 10.0
FORMS = ['0', '1', '2']     # BFGX_K1_FLUID at plan creation: the barrier-per-tile form, the default rule, the fluid form whatever the tile count
ROUTES = ['parity', 'f64']
# what the halo (log10 M, z, dec) and the radial axis (R_min, R_max of the 96-node table) of a case are chosen to reach
CASES = {
    # pixels out to |x| ~ 0.35 - 0.37 rad from the halo's azimuth: the far end of the sine / 1 - cosine series.  (A disc is narrow up to 0.40 rad;
    # beyond that its pairs take the full-range copy, which is not the code under test.)
    'wide_x': dict(logM={64: 15.0, 256: 15.0}, z={64: 0.05, 256: 0.05}, dec=74.4, R=(1e-3, 1e3)),
    # fewer than eight ring rows: one short row pass, a single trip.  (The table of this case is scaled by 30: the offsets of so small a disc
    # are otherwise ~1e-6, and 1e-10 of that lies below the 1e-16 to which the oracle itself can form (v + e) / |v + e| - v of unit vectors.)
    'few_rings': dict(logM={64: 13.9, 256: 12.6}, z={64: 0.05, 256: 0.10}, dec=9.6, R=(1e-3, 1e3), scale=30.0),
    # the disc's inner pixels lie below the first node of the radial axis, its outer ones above the last: clamp and range test, both ends
    'axis_low': dict(logM={64: 15.0, 256: 15.0}, z={64: 0.05, 256: 0.05}, dec=9.6, R=(6.0, 1e3)),
    'axis_high': dict(logM={64: 15.0, 256: 15.0}, z={64: 0.05, 256: 0.05}, dec=9.6, R=(1e-3, 6.0)),
    # the halo 3e-7 rad from a pixel centre: |u|^2 ~ 1e-13 next to the floor of the logarithm's argument, the pair far below the table
    'on_centre': dict(logM={64: 15.0, 256: 15.0}, z={64: 0.05, 256: 0.05}, dec=9.6, R=(1e-3, 1e3), centre=True),
}
_ref = {}


def _table(R_min, R_max):
    from baryonification_amd import synthetic as syn
    z, M, r = syn.table_grid({'z': np.array([0.02, 0.5]), 'M': np.array([1e12, 1e16])}, Nz=4, NM=6, NR=96, R_min=R_min, R_max=R_max, pad=1e-9)
    return [np.log(1 + z), np.log(M), np.log(r)], syn.displacement_table(z, M, r)


def _case(nside, name):
    """catalog, table and the oracle's offsets of one case, computed once and read-only; the properties the case is there for are checked
    on the oracle's side"""
    if (nside, name) in _ref:
        return _ref[(nside, name)]
    from baryonification_amd import synthetic as syn
    from oracle import oracle as O
    c = CASES[name]
    npix = 12 * nside * nside
    vec = O.pix2vec(nside, np.arange(npix, dtype=np.int64)).reshape(npix, 3)
    ra, dec = 45.0, c['dec']
    if c.get('centre'):
        th0, ph0 = np.radians(90.0 - dec), np.radians(ra)
        p = int(np.argmin(np.linalg.norm(vec - np.array([np.sin(th0) * np.cos(ph0), np.sin(th0) * np.sin(ph0), np.cos(th0)]), axis=1)))
        ra, dec = np.degrees(np.arctan2(vec[p, 1], vec[p, 0])), 90.0 - np.degrees(np.arccos(vec[p, 2]) + 3e-7)
    cat = {'M': np.array([10.0 ** c['logM'][nside]]), 'z': np.array([c['z'][nside]]), 'ra': np.array([ra]), 'dec': np.array([dec])}
    axes, table = _table(*c['R'])
    table = table * c.get('scale', 1.0)
    ora, counts = O.baryonify_offsets(nside, cat, O.Table(axes, table, False, EPS), EPS, O.Background.from_dict(syn.COSMO), return_counts=True)
    th0, ph0 = np.radians(90.0 - dec), np.radians(ra)
    v0 = np.array([np.sin(th0) * np.cos(ph0), np.sin(th0) * np.sin(ph0), np.cos(th0)])
    dist = np.linalg.norm(vec - v0, axis=1)
    disc = np.argsort(dist)[:int(counts[0])]                       # the pixels of the disc (the census counts the pixel centres inside it)
    x = (np.arctan2(vec[disc, 1], vec[disc, 0]) - ph0 + np.pi) % (2 * np.pi) - np.pi
    nrings = np.unique(np.round(vec[disc, 2], 12)).size
    # (a pair outside the radial axis leaves (v + 0) / |v + 0| - v in the oracle's sum: rounding noise of 1e-16, not an exact zero)
    moved = np.abs(ora).max(axis=1) > 1e-13                      # (against unit vectors; the offsets of these halos reach 1e-5 .. 1e-4)
    assert counts[0] > 4 and moved.any() and not moved[np.setdiff1d(np.arange(npix), disc)].any()
    assert np.abs(ora).max() > 5e-6                               # (the reference's own rounding stays below a tenth of the 1e-10 bound)
    if name == 'wide_x':
        assert 0.33 < np.abs(x).max() < 0.40
    if name == 'few_rings':
        assert nrings < 8
    if name in ('axis_low', 'axis_high'):
        # some pairs of the disc are outside the radial axis (no offset), the rest inside: on the side the case names
        out, inside = disc[~moved[disc]], disc[moved[disc]]
        assert 0 < out.size < disc.size
        assert (dist[out].max() < dist[inside].min()) if name == 'axis_low' else (dist[out].min() > dist[inside].max())
    if name == 'on_centre':
        assert dist.min() < 1e-6
    ora.setflags(write=False)
    _ref[(nside, name)] = dict(cat=cat, axes=axes, table=table, ora=ora, pairs=int(counts[0]), nrings=nrings, xmax=float(np.abs(x).max()))
    return _ref[(nside, name)]


def _cat_dev(cat):
    import torch
    from baryonification_amd import _lib
    dev = torch.device('cuda', 0)
    cols = {k: torch.from_numpy(np.ascontiguousarray(cat[k])).to(dev) for k in ('M', 'z', 'ra', 'dec')}
    lnz, lnM = _lib.table_coords(cat['M'], cat['z'])
    cols['lnz'], cols['lnM'] = torch.from_numpy(lnz).to(dev), torch.from_numpy(lnM).to(dev)
    return _lib.make_catalog_dev(1, cols['M'].data_ptr(), cols['z'].data_ptr(), cols['ra'].data_ptr(), cols['dec'].data_ptr(),
                                 ln1pz_ptr=cols['lnz'].data_ptr(), lnM_ptr=cols['lnM'].data_ptr()), cols


def _offsets_raw(plan, cd, nside, acc):
    """the 24 bytes per pixel that K1 leaves, as they are (fp64 [npix][3], or fp32 hi [npix][3] followed by fp32 lo [npix][3])"""
    import torch
    npix = 12 * nside * nside
    off = torch.zeros(npix * 3, dtype=torch.float64, device=torch.device('cuda', 0))
    plan.offsets(cd, off.data_ptr(), acc)
    torch.cuda.synchronize()
    plan.status()
    return off.cpu().numpy()


def _joined(raw, nside, parity):
    npix = 12 * nside * nside
    if not parity:
        return raw.reshape(npix, 3)
    o32 = raw.view(np.float32)
    return (o32[:npix * 3].astype(np.float64) + o32[npix * 3:].astype(np.float64)).reshape(npix, 3)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('nside', [64, 256])
def test_k1_single_halo_series_edges(gpu, monkeypatch, nside, route, form):
    """one halo per call at each edge of the pair phase's series (CASES): pix_offsets against the oracle at the bounds the existing tests
    hold these routes to -- 1e-9 of the largest offset for the parity-grade route (test_gpu_k1_pairloop.py: its logarithm and sine are cut at
    5e-11 and 2e-11), 1e-10 for fp64 throughout -- and two consecutive calls bit for bit the same (one pair per pixel: no sum whose order
    could differ)."""
    import torch
    from baryonification_amd import _lib, engine, synthetic as syn
    acc = _lib.ACC_PARITY if route == 'parity' else _lib.ACC_F64
    tol = 1e-9 if route == 'parity' else 1e-10
    monkeypatch.setenv('BFGX_K1_FLUID', form)
    plans = {}
    for name in CASES:
        g = _case(nside, name)
        key = (CASES[name]['R'], CASES[name].get('scale', 1.0))
        if key not in plans:
            model, keep = engine.model_from_tables(g['axes'], g['table'], syn.COSMO, EPS, EPS)
            plans[key] = (engine.ShellPlan(model, keep, nside, 16, 0, torch.cuda.current_stream().cuda_stream), keep)
            assert plans[key][0].precision(acc)[0] == acc
        plan = plans[key][0]
        cd, cols = _cat_dev(g['cat'])
        assert plan.count_pairs(cd, True) == g['pairs']
        raw1 = _offsets_raw(plan, cd, nside, acc)
        raw2 = _offsets_raw(plan, cd, nside, acc)
        got = _joined(raw1, nside, route == 'parity')
        scale = np.abs(g['ora']).max()
        err = np.abs(got - g['ora']).max()
        print("NSIDE %d %s form %s %-9s: %5d pairs, %2d rings, max|x| %.3f: max |hip - oracle| = %.3e of the largest offset %.3e"
              % (nside, route, form, name, g['pairs'], g['nrings'], g['xmax'], err / scale, scale))
        assert np.all(got[np.abs(g['ora']).max(axis=1) == 0.0] == 0.0)             # nothing outside the disc
        assert err <= tol * scale
        assert np.array_equal(raw1.view(np.uint64), raw2.view(np.uint64))
    for plan, keep in plans.values():
        plan.close()


# ---------------------------------------------------------------------------------- K2
def _prescribed_offsets(nside):
    """|offset| from 0 to 16 ring spacings in a random direction, every pixel (the two polar rings included) displaced"""
    rng = np.random.default_rng(640)
    npix = 12 * nside * nside
    ring = np.sqrt(4 * np.pi / npix)                              # ~ the ring spacing at the equator
    mag = 16.0 * ring * rng.random(npix) ** 2
    mag[:8] = 16.0 * ring * np.array([0.0, 0.02, 0.2, 0.5, 0.8, 1.0, 0.05, 0.001])      # first polar ring (4 pixels) and the next one
    mag[-8:] = mag[:8][::-1]
    d = rng.normal(size=(npix, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return d * mag[:, None]


def _k2_ref():
    if 'k2' in _ref:
        return _ref['k2']
    from baryonification_amd import synthetic as syn
    from oracle import oracle as O
    nside = 64
    off = _prescribed_offsets(nside)
    hi = off.astype(np.float32)
    lo = (off - hi.astype(np.float64)).astype(np.float32)
    hmap = syn.make_map(nside)
    hmap[::17] = 0.0
    # each mode against the oracle's regrid of the offsets that mode really holds
    ref = {'f64': O.regrid(nside, hmap, off), 'split': O.regrid(nside, hmap, hi.astype(np.float64) + lo.astype(np.float64))}
    for a in (off, hi, lo, hmap, ref['f64'], ref['split']):
        a.setflags(write=False)
    _ref['k2'] = dict(nside=nside, off=off, hi=hi, lo=lo, hmap=hmap, ref=ref)
    return _ref['k2']


@pytest.mark.parametrize('mode', ['split', 'f64'])
def test_k2_prescribed_displacements_vs_oracle(gpu, mode):
    """K2 on NSIDE 64 with prescribed pix_offsets of 0 to 16 ring spacings, polar rings included, as fp64 and as split hi + lo fp32.
    fp64: 1e-10 of the largest pixel, the bound of test_regrid_any_displacement_vs_oracle.  Split: that test has no such mode; the bound is
    reasoned.  The split offsets are exact to 2^-48 and the oracle regrids the same hi + lo; the parity-grade small-angle series (RMathE, and
    PMathE's sine / 1 - cosine) are cut at <= 1e-11 of the angle they return (sqrt(1 + t^2) - 1: 21 t^12 / 1024 against t^2 / 2 at t = 0.1 is
    4e-12; asin: 1e-15; atan: t^12 / 13 = 8e-14; the Newton steps on fp32 seeds: 3e-14; the sine at 0.45 rad: 8.5e-12), the displacement of a
    gathered pixel is at most 16 pixel sides, so a bilinear weight is off by <= 2e-10; a pixel collects of the order of ten deposits of values
    <= 25 (Poisson(8)): <= 5e-8 against mean(map) = 8.  Bound: 1e-8 mean(map), the bound the parity-grade map is held to elsewhere
    (test_gpu_k1_pairloop.py).  Mass sums to 1e-12; two consecutive calls to 1e-13 mean(map) (the LDS sums are not ordered)."""
    import torch
    from baryonification_amd import _lib, engine, synthetic as syn
    g = _k2_ref()
    nside, npix = g['nside'], 12 * g['nside'] ** 2
    pix = np.sqrt(4 * np.pi / npix)
    reach = np.linalg.norm(g['off'], axis=1) / pix
    assert reach.min() == 0.0 and 15.0 < reach.max() <= 16.0 * (1 + 1e-12) and np.all(reach[[1, 2, 3, npix - 2]] > 0)
    cat = syn.make_catalog(100)
    z, M, r = syn.table_grid(cat, Nz=4, NM=4, NR=96)
    model, keep = engine.model_from_tables([np.log(1 + z), np.log(M), np.log(r)], syn.displacement_table(z, M, r), syn.COSMO, 10.0, 10.0)
    dev = torch.device('cuda', 0)
    plan = engine.ShellPlan(model, keep, nside, 100, device=0, stream=torch.cuda.current_stream().cuda_stream)
    if mode == 'split':
        assert plan.precision(_lib.ACC_PARITY)[0] == _lib.ACC_PARITY
        d_off = torch.from_numpy(np.concatenate([g['hi'].reshape(-1), g['lo'].reshape(-1)])).to(dev)
        acc, tol = _lib.ACC_PARITY, 1e-8 * g['hmap'].mean()
    else:
        d_off = torch.from_numpy(np.array(g['off']).reshape(-1)).to(dev)
        acc, tol = _lib.ACC_F64, 1e-10 * np.abs(g['ref']['f64']).max()
    d_map = torch.from_numpy(np.array(g['hmap'])).to(dev)
    outs = []
    for call in range(2):
        out = torch.full((npix,), np.nan, dtype=torch.float64, device=dev)
        sums = torch.zeros(2, dtype=torch.float64, device=dev)
        plan.regrid(d_map.data_ptr(), d_off.data_ptr(), out.data_ptr(), sums.data_ptr(), acc_f64=acc)
        torch.cuda.synchronize()
        plan.status()
        got, sm = out.cpu().numpy(), sums.cpu().numpy()
        assert np.isfinite(got).all()
        err = np.abs(got - g['ref'][mode]).max()
        print("K2 %s call %d: max |hip - oracle| = %.3e mean(map) = %.3e max(map); sums %.15e -> %.15e" %
              (mode, call, err / g['hmap'].mean(), err / np.abs(g['ref'][mode]).max(), sm[0], sm[1]))
        assert err <= tol
        total = g['hmap'].sum()
        assert abs(sm[0] - total) <= 1e-12 * total and abs(sm[1] - sm[0]) <= 1e-12 * total and abs(got.sum() - total) <= 1e-12 * total
        outs.append(got)
    plan.close()
    assert np.abs(outs[0] - outs[1]).max() <= 1e-13 * g['hmap'].mean()
