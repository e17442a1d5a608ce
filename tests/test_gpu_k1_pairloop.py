"""The parity-grade pair loop of the fast kernel (bfgx_scatter2.hpp: pair_front / pair_back, k1_pairs_rotated): the front half of trip T + 1
runs beside the back half of trip T, two state sets, an epilogue for the last trip.  What can go wrong there are the trip-count edges (one trip,
even and odd counts), the row record / mask word of the NEXT trip, and the unpipelined WIDE copy beside pipelined chunks -- in both forms of
the kernel (BFGX_K1_FLUID=0: a barrier per tile; =2: the fluid form whatever the number of tiles).  Every case first checks that the plan really
runs BFGX_ACC_PARITY (tables without property axes, uniform in ln r), so that it cannot pass on the fp64 path."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FORMS = ['0', '2']          # BFGX_K1_FLUID at plan creation
EPS = 10.0


def _plan(monkeypatch, form, axes, table, nside, nmax, eps_runner=EPS, eps_model=None):
    import torch
    from baryonification_amd import _lib, engine, synthetic as syn
    monkeypatch.setenv('BFGX_K1_FLUID', form)
    model, keep = engine.model_from_tables(axes, table, syn.COSMO, eps_runner, eps_runner if eps_model is None else eps_model)
    plan = engine.ShellPlan(model, keep, nside, nmax, 0, torch.cuda.current_stream().cuda_stream)
    assert plan.precision(_lib.ACC_PARITY)[0] == _lib.ACC_PARITY
    return plan


def _cat_dev(cat):
    import torch
    from baryonification_amd import _lib
    dev = torch.device('cuda', 0)
    cols = {k: torch.from_numpy(np.ascontiguousarray(cat[k])).to(dev) for k in ('M', 'z', 'ra', 'dec')}
    lnz, lnM = _lib.table_coords(cat['M'], cat['z'])
    cols['lnz'], cols['lnM'] = torch.from_numpy(lnz).to(dev), torch.from_numpy(lnM).to(dev)
    n = cols['M'].numel()
    return _lib.make_catalog_dev(n, cols['M'].data_ptr(), cols['z'].data_ptr(), cols['ra'].data_ptr(), cols['dec'].data_ptr(),
                                 ln1pz_ptr=cols['lnz'].data_ptr(), lnM_ptr=cols['lnM'].data_ptr()), cols


def _offsets(plan, cd, nside, acc):
    """pix_offsets [npix][3] as fp64; BFGX_ACC_PARITY: hi [npix][3] fp32, then lo [npix][3] fp32 behind it (include/bfgx.h), joined"""
    import torch
    from baryonification_amd import _lib
    npix = 12 * nside * nside
    off = torch.zeros(npix * 3, dtype=torch.float64, device=torch.device('cuda', 0))        # (24 bytes per pixel either way)
    plan.offsets(cd, off.data_ptr(), acc)
    torch.cuda.synchronize()
    plan.status()
    if acc == _lib.ACC_PARITY:
        o32 = off.view(torch.float32)
        return (o32[:npix * 3].double() + o32[npix * 3:].double()).cpu().numpy().reshape(npix, 3)
    return off.cpu().numpy().reshape(npix, 3)


# ---------------------------------------------------------------------------------- 1. trip-count edges, one halo per run
def _single_table():
    from baryonification_amd import synthetic as syn
    z, M, r = syn.table_grid({'z': np.array([0.02, 0.5]), 'M': np.array([1e12, 1e16])}, Nz=4, NM=6, NR=96, R_min=1e-3, R_max=1e3, pad=1e-9)
    return [np.log(1 + z), np.log(M), np.log(r)], syn.displacement_table(z, M, r)


# (log10 M, z) of one halo at (ra, dec) = (45, 9.6) deg, NSIDE 64, eps = 10 -> pixels in its disc by the oracle's census (56, 122, 161, 220):
# at most one trip, two, three (odd), four.  The tiles of this shell are 8 rings x 32 pixels, so the larger discs reach the loop in parts; the
# last one (938 pixels, 34 rings across) covers whole tiles: row passes of 256 pairs, four trips, beside every smaller count at its rim
TRIPS = [(14.5, 0.05, 1, 63), (15.0, 0.05, 65, 128), (15.2, 0.05, 129, 192), (15.4, 0.05, 193, 256), (15.7, 0.03, 900, 1000)]


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('log10M,z,lo,hi', TRIPS)
def test_trip_count_edges_single_halo(gpu, monkeypatch, form, log10M, z, lo, hi):
    """one halo whose disc holds < 64, 65 - 128, 129 - 192 (three trips: the odd epilogue), 193 - 256 and ~940 pairs: pix_offsets against the oracle.
    Bound: the parity-grade logarithm and sine are cut at 5e-11 and 2e-11 (PMathE), the table's logarithmic slope inside eps R is below ten where
    the offset is not negligible: 1e-9 of the largest offset."""
    from baryonification_amd import _lib, synthetic as syn
    from oracle import oracle as O
    nside = 64
    axes, table = _single_table()
    cat = {'M': np.array([10.0 ** log10M]), 'z': np.array([z]), 'ra': np.array([45.0]), 'dec': np.array([9.6])}
    ora, counts = O.baryonify_offsets(nside, cat, O.Table(axes, table, False, EPS), EPS, O.Background.from_dict(syn.COSMO), return_counts=True)
    plan = _plan(monkeypatch, form, axes, table, nside, 16)
    cd, keep = _cat_dev(cat)
    npairs = plan.count_pairs(cd, True)
    print("form %s, log10 M %.2f: %d pairs (oracle %d), tile shape %s" % (form, log10M, npairs, int(counts[0]), plan.tile_shape()))
    assert npairs == int(counts[0]) and lo <= npairs <= hi
    got = _offsets(plan, cd, nside, _lib.ACC_PARITY)
    plan.close()
    err = np.abs(got - ora).max()
    print("   max |hip - oracle| = %.3e of the largest offset %.3e" % (err / np.abs(ora).max(), np.abs(ora).max()))
    assert np.count_nonzero(np.abs(got).max(axis=1)) == np.count_nonzero(np.abs(ora).max(axis=1)) > 0
    assert err <= 1e-9 * np.abs(ora).max()


# ---------------------------------------------------------------------------------- 2. / 3. many rows per trip, 600 halos
REGIMES = {128: dict(seed=1, zr=(0.05, 0.2), logM=(13.0, 15.5), eps=8.0, scale=400.0),
           512: dict(seed=2, zr=(0.1, 0.2), logM=(13.5, 15.5), eps=6.0, scale=60.0)}      # several tiles per halo, region-B chunks of two entries
_cache = {}


def _regime(nside):
    """inputs and the oracle's results of one regime, computed once: 600 random halos + the four pole / seam halos, a table that is not monotone
    in r and scaled so that the heaviest halo alone moves pixels by about three pixel sides, model epsilon < runner epsilon (the cut bites)"""
    if nside in _cache:
        return _cache[nside]
    from baryonification_amd import synthetic as syn
    from oracle import oracle as O
    g = REGIMES[nside]
    cat = syn.make_catalog(600, seed=2000 + g['seed'], z_lo=g['zr'][0], z_hi=g['zr'][1], logM_lo=g['logM'][0], logM_hi=g['logM'][1])
    cat['dec'][:4] = [90.0 - 1e-8, -90.0 + 1e-8, 89.99, 0.0]          # poles and the phi = 0 seam
    cat['ra'][:4] = [0.0, 123.0, 359.999, 1e-9]
    z, M, r = syn.table_grid(cat, Nz=5, NM=6, NR=96, R_min=1e-3, R_max=1e3, pad=1e-9)
    d = g['scale'] * syn.displacement_table(z, M, r) * (1 + 0.3 * np.sin(3 * np.log(r))[None, None, :])
    axes = [np.log(1 + z), np.log(M), np.log(r)]
    hmap = syn.make_map(nside, seed=g['seed'])
    ora_off = O.baryonify_offsets(nside, cat, O.Table(axes, d, False, 0.7 * g['eps']), g['eps'], O.Background.from_dict(syn.COSMO))
    ora_map = O.regrid(nside, hmap, ora_off)
    for a in (ora_off, ora_map, hmap):
        a.setflags(write=False)
    _cache[nside] = dict(cat=cat, axes=axes, table=d, eps=g['eps'], hmap=hmap, ora_off=ora_off, ora_map=ora_map)
    return _cache[nside]


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('nside', [128, 512])
def test_many_rows_per_trip_vs_oracle(gpu, monkeypatch, form, nside):
    """600 halos, trips that hold many short rows, wide (polar) discs beside pipelined chunks: the map within the parity-grade bound
    1e-8 mean(map) of the oracle's, the mass sum to 1e-12"""
    import torch
    from baryonification_amd import _lib
    g = _regime(nside)
    pix = np.sqrt(4 * np.pi / (12 * nside * nside))
    assert 2.0 < np.linalg.norm(g['ora_off'], axis=1).max() / pix < 12.0             # pixels move by a few pixel sides
    plan = _plan(monkeypatch, form, g['axes'], g['table'], nside, 600, g['eps'], 0.7 * g['eps'])
    cd, keep = _cat_dev(g['cat'])
    dev = torch.device('cuda', 0)
    npix = 12 * nside * nside
    d_map = torch.from_numpy(np.array(g['hmap'])).to(dev)                            # (a writable copy: the shared reference stays read-only)
    off = torch.zeros(npix * 3, dtype=torch.float64, device=dev)
    out = torch.zeros(npix, dtype=torch.float64, device=dev)
    sums = torch.zeros(2, dtype=torch.float64, device=dev)
    plan.baryonify(cd, d_map.data_ptr(), off.data_ptr(), out.data_ptr(), sums.data_ptr(), acc_f64=_lib.ACC_PARITY)
    torch.cuda.synchronize()
    plan.status()
    plan.close()
    got, sm = out.cpu().numpy(), sums.cpu().numpy()
    err = np.abs(got - g['ora_map']).max()
    print("form %s, NSIDE %d: max |hip - oracle| = %.3e mean(map)" % (form, nside, err / g['ora_map'].mean()))
    assert err <= 1e-8 * g['ora_map'].mean()
    assert np.isclose(got.sum(), g['hmap'].sum(), rtol=1e-12) and np.isclose(sm[1], sm[0], rtol=1e-12)


# largest |parity-grade - fp64| of pix_offsets over the largest |offset|, measured on the commit BEFORE the pair loop was rotated, same inputs:
#   NSIDE 128: barrier form 4.2296e-12, fluid form 4.2296e-12;  NSIDE 512: barrier form 8.2750e-12, fluid form 8.2750e-12
PARITY_VS_F64_PARENT = {128: 4.2296e-12, 512: 8.2750e-12}


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('nside', [128, 512])
def test_parity_grade_vs_fp64_same_build(gpu, monkeypatch, form, nside):
    """same inputs, same plan, BFGX_ACC_PARITY against BFGX_ACC_F64 pix_offsets.  The arithmetic per pair is what it was before the loop was
    rotated, only the order of the LDS sums may differ: the bound is twice the larger figure (of the two forms) measured on the parent commit
    (4.2296e-12 of the largest offset at NSIDE 128 and 8.2750e-12 at NSIDE 512, the same in both forms; the rotated loop: 4.2296e-12, 8.2744e-12)."""
    from baryonification_amd import _lib
    g = _regime(nside)
    plan = _plan(monkeypatch, form, g['axes'], g['table'], nside, 600, g['eps'], 0.7 * g['eps'])
    cd, keep = _cat_dev(g['cat'])
    par = _offsets(plan, cd, nside, _lib.ACC_PARITY)
    f64 = _offsets(plan, cd, nside, _lib.ACC_F64)
    plan.close()
    scale = np.abs(f64).max()
    rel = np.abs(par - f64).max() / scale
    print("form %s, NSIDE %d: max |parity - f64| = %.4e of the largest offset %.3e" % (form, nside, rel, scale))
    assert np.abs(f64 - g['ora_off']).max() <= 1e-10 * np.abs(g['ora_off']).max()
    assert rel <= 2.0 * PARITY_VS_F64_PARENT[nside]


# ---------------------------------------------------------------------------------- 4. empty and degenerate row passes
@pytest.mark.parametrize('form', FORMS)
def test_empty_and_degenerate_row_passes(gpu, monkeypatch, form):
    """halos outside the (z, M) table: offsets exactly zero; halos that all take the "< 4 pixels" fallback: the narrow list's row passes see
    no pair of their own (total == 0), the four fallback pixels per halo agree with the oracle (bound as in the single-halo test: the
    fallback pixels lie between ~5 and ~35 R, where the offset falls faster than the logarithmic slope of the table grows)"""
    from baryonification_amd import _lib, synthetic as syn
    from oracle import oracle as O
    nside = 64
    axes, table = _single_table()
    bg = O.Background.from_dict(syn.COSMO)
    plan = _plan(monkeypatch, form, axes, table, nside, 256)
    # (a) every halo above the table's mass range
    cat = syn.make_catalog(200, seed=31, z_lo=0.03, z_hi=0.2, logM_lo=16.5, logM_hi=17.0)
    cd, keep = _cat_dev(cat)
    assert plan.count_pairs(cd, True) > 200 * 64                # (the row passes are full of pairs: none of them may add anything)
    got = _offsets(plan, cd, nside, _lib.ACC_PARITY)
    assert np.all(got == 0.0)
    # (b) every disc holds fewer than four pixel centres
    cat = syn.make_catalog(200, seed=32, z_lo=0.25, z_hi=0.3, logM_lo=13.8, logM_hi=14.3)
    ora, counts = O.baryonify_offsets(nside, cat, O.Table(axes, table, False, EPS), EPS, bg, return_counts=True)
    assert np.all(counts == 4)
    cd, keep = _cat_dev(cat)
    assert plan.count_pairs(cd, True) == 800 and plan.count_pairs(cd, False) < 800
    got = _offsets(plan, cd, nside, _lib.ACC_PARITY)
    plan.close()
    assert np.abs(ora).max() > 0 and np.abs(got - ora).max() <= 1e-9 * np.abs(ora).max()
