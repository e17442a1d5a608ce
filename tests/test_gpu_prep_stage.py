"""The stage in front of K1 -- K0 (halo_prep_kernel: the "fewer than 4 pixels" census, the tile enumeration, the slot reservation, the
record stores) and the placement pass (tile_scan / tile_place: a thread per few-tile halo, the wave per many-tile halo) -- on catalogs built
to reach every path of it, at NSIDE 64 and 256: discs of 0 - 3 pixels (the 4-pixel fallback), of exactly 4 pixels, over a pole, across
phi = 0, over more than 4 tiles and over hundreds of tiles up to every tile of the sphere, one tile listed by more halos than its fixed list
holds, non-finite and non-positive rows inside quads of lanes and at the end, and a catalog length that is no multiple of 4 or 64.

Checked: the per-halo census (count_pairs with counts) equals the oracle's halo by halo and the census through the tile path in total, with
and without the fallback; pix_offsets (fp64) and the baryonified map equal the oracle's at the tolerances tests/test_gpu_parity.py states --
1e-10 max for fp64 throughout, 1e-6 mean(map) for the default (whatever the plan resolves it to) and for fp32 pair math where the table
stays inside its range (0.1 pixel sides), 1e-8 mean(map) for the parity-grade mode.  The library has no entry that reads K0's records back,
so they are checked through what K1 makes of them in the three precisions (PairRecT<float>: fp32; PairRecT<double>: fp64, parity-grade)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 10.0
SHAPES = {64: 2003, 256: 6007}          # NSIDE -> catalog rows (neither a multiple of 4 nor of 64)
LIST_CAP = 64                           # NSIDE 64: a tile's fixed list is cut to this many entries (BFGX_TILE_LIST_CAP), 300 halos share one spot


def _catalog(nside, n_rows):
    """(catalog with invalid rows, index of the valid rows in it)"""
    from baryonification_amd import synthetic as syn
    bad_at = np.array([1, 2, 5, 64, 255, 256, 257, n_rows - 2, n_rows - 1])          # inside quads, across a wave / workgroup edge, the last rows
    nv = n_rows - bad_at.size
    # z 0.2 - 0.3, 1e12 - 1e15 Msun: disc radii of 0.15 - 1.5 (NSIDE 64) / 0.6 - 6 (NSIDE 256) pixel sides: fallback discs, discs of exactly 4 pixels
    cat = syn.make_catalog(nv, seed=4100 + nside, z_lo=0.2, z_hi=0.3, logM_lo=12.0, logM_hi=15.0)
    k = 0

    def put(M, z, ra, dec):
        nonlocal k
        cat['M'][k], cat['z'][k], cat['ra'][k], cat['dec'][k] = M, z, ra, dec
        k += 1
    # discs of 0.14 rad up to the whole sphere (tens to hundreds of tiles, every tile), on and beside the poles, across phi = 0
    for ra, dec, z in ((0.0, 90 - 1e-8, 0.01), (10.0, -90 + 1e-8, 0.012), (359.99, 89.9, 0.02), (0.01, -89.9, 0.015), (0.0, 0.0, 0.008),
                       (359.9999, 12.0, 0.005), (180.0, 89.0, 0.05), (90.0, -88.5, 0.004), (200.0, -35.0, 0.0035), (0.0, 60.0, 0.003),
                       (300.0, 5.0, 0.0025), (45.0, -89.0, 0.002)):
        put(3e15, z, ra, dec)
    # discs over more than 4 tiles (0.05 - 0.1 rad), some across phi = 0, some over a pole
    for i in range(24):
        put(1e15, 0.05 + 0.002 * i, (0.0, 359.95, 0.02, 123.0)[i % 4] + 0.37 * i, (-60.0, 0.0, 41.8, 89.5, -89.7, 19.5)[i % 6])
    # small discs (fallback and just above) on and beside the poles and across phi = 0.  (1e-9 deg off the pole: at dec = +90 exactly
    # pi / 2 - dec pi / 180 rounds to -6e-17 and K0 drops the halo as out of range, as it always has; the oracle keeps it)
    for i in range(24):
        put(10.0 ** (12.0 + 0.12 * i), 0.25, (0.0, 359.9999, 1e-7, 180.0)[i % 4], (90.0 - 1e-9, -90.0 + 1e-9, 89.99, -89.99, 0.0, 30.0)[i % 6])
    # 300 small halos in one spot: more than LIST_CAP in one tile's list
    rng = np.random.default_rng(nside)
    for i in range(300):
        put(10.0 ** rng.uniform(12.0, 13.0), rng.uniform(0.2, 0.3), 77.0 + rng.uniform(-0.2, 0.2), 23.0 + rng.uniform(-0.2, 0.2))
    assert k < nv
    full = {key: np.empty(n_rows) for key in cat}
    valid = np.setdiff1d(np.arange(n_rows), bad_at)
    for key in cat:
        full[key][valid] = cat[key]
        full[key][bad_at] = cat[key][:bad_at.size]
    full['M'][bad_at[0]] = np.nan
    full['M'][bad_at[1]] = -1e14
    full['M'][bad_at[2]] = 0.0
    full['dec'][bad_at[3]] = 91.0
    full['ra'][bad_at[4]] = np.nan
    full['z'][bad_at[5]] = np.nan
    full['M'][bad_at[6]] = np.inf
    full['dec'][bad_at[7]] = np.nan
    full['M'][bad_at[8]] = np.nan
    return full, valid


_shell = {}


def shell(nside):
    """catalog, table, map and the oracle's results for one NSIDE: computed once, shared by the tests, never modified"""
    if nside in _shell:
        return _shell[nside]
    from baryonification_amd import synthetic as syn
    from oracle import oracle as O
    full, valid = _catalog(nside, SHAPES[nside])
    cat = {k: np.ascontiguousarray(v[valid]) for k, v in full.items()}
    z, M, r = syn.table_grid(cat, Nz=6, NM=6, NR=200, pad=1e-9)
    axes = [np.log(1 + z), np.log(M), np.log(r)]
    # a fifth of the plumbing table: the nearest, heaviest halo moves a pixel by 0.05 pixel sides at NSIDE 64 (inside fp32's range), 0.2 at NSIDE 256
    table = 0.2 * syn.displacement_table(z, M, r)
    hmap = syn.make_map(nside, seed=4200 + nside)
    bg = O.Background.from_dict(syn.COSMO)
    tab = O.Table(axes, table, False, EPS)
    off, counts = O.baryonify_offsets(nside, cat, tab, EPS, bg, return_counts=True)
    ora = O.regrid(nside, hmap, off)
    assert np.isclose(ora.sum(), hmap.sum())
    _shell[nside] = dict(full=full, valid=valid, axes=axes, table=table, hmap=hmap, off=off, counts=counts, ora=ora)
    return _shell[nside]


def make_plan(s, nside, monkeypatch):
    import torch
    from baryonification_amd import _lib, engine, synthetic as syn
    if nside == 64:
        monkeypatch.setenv('BFGX_TILE_LIST_CAP', str(LIST_CAP))
    dev = torch.device('cuda', 0)
    n = s['full']['M'].size
    model, keep = engine.model_from_tables(s['axes'], s['table'], syn.COSMO, EPS)
    plan = engine.ShellPlan(model, keep, nside, n, 0, torch.cuda.current_stream().cuda_stream)
    t = {k: torch.from_numpy(v).to(dev) for k, v in s['full'].items()}
    cd = _lib.make_catalog_dev(n, t['M'].data_ptr(), t['z'].data_ptr(), t['ra'].data_ptr(), t['dec'].data_ptr())
    return plan, cd, t


@pytest.mark.parametrize('nside', sorted(SHAPES))
def test_census_through_tiles_equals_per_halo_census(gpu, nside, monkeypatch):
    import torch
    s = shell(nside)
    plan, cd, keep = make_plan(s, nside, monkeypatch)
    n = s['full']['M'].size
    got, through_tiles = {}, {}
    for fb in (True, False):
        plan.set_algo(0)
        c = torch.full((n,), -1, dtype=torch.int64, device='cuda')
        tot = plan.count_pairs(cd, fallback4=fb, counts_ptr=c.data_ptr())          # the per-halo census
        torch.cuda.synchronize()
        got[fb] = c.cpu().numpy()
        assert tot == got[fb].sum()
        plan.set_algo(1)
        through_tiles[fb] = plan.count_pairs(cd, fallback4=fb)                       # K0 + binning + placement + the tile kernel's census
    plan.status()
    br, w = plan.tile_shape()
    plan.close()
    valid = s['valid']
    invalid = np.setdiff1d(np.arange(n), valid)
    for fb in (True, False):
        assert through_tiles[fb] == got[fb].sum() and got[fb].sum() > 0             # no pixel of any disc lost or listed twice
        assert np.all(got[fb][invalid] == 0)
    differ = np.flatnonzero(got[True][valid] != s['counts'])                         # == the oracle, halo by halo
    assert differ.size == 0, [(int(valid[i]), int(got[True][valid][i]), int(s['counts'][i]), int(got[False][valid][i]),
                               {k: float(v[valid[i]]) for k, v in s['full'].items()}) for i in differ[:8]]
    raw, fb4 = got[False][valid], got[True][valid]
    # the catalog holds what it was built for: fallback discs of 0 .. 3 pixels, discs of exactly 4 and just above, very large ones
    for k in (0, 1, 2, 3, 4):
        assert (raw == k).any(), k
    assert ((raw > 4) & (raw <= 8)).any()
    assert np.all(fb4[raw >= 4] == raw[raw >= 4]) and np.all(fb4[raw < 4] >= 1) and np.all(fb4[raw < 4] <= 4)
    # a tile holds at most br x w pixels: discs of more pixels than 4 (100) tiles hold lie over more than 4 (100) tiles -- the placement
    # pass's many-tile halos
    assert ((raw > 4 * br * w) & (raw < 100 * br * w)).sum() >= 2 and (raw > 100 * br * w).sum() >= 2, (br, w, np.sort(raw)[-40:])


@pytest.mark.parametrize('nside', sorted(SHAPES))
def test_offsets_and_map_equal_the_oracle(gpu, nside, monkeypatch):
    import torch
    from baryonification_amd import _lib
    s = shell(nside)
    plan, cd, keep = make_plan(s, nside, monkeypatch)
    npix = 12 * nside * nside
    dev = torch.device('cuda', 0)
    ora, hmap = s['ora'], s['hmap']
    d_map = torch.from_numpy(hmap).to(dev)
    # pix_offsets, fp64 throughout
    off = torch.zeros(npix * 3, dtype=torch.float64, device=dev)
    plan.offsets(cd, off.data_ptr(), _lib.ACC_F64)
    torch.cuda.synchronize()
    d_off = np.abs(off.cpu().numpy().reshape(npix, 3) - s['off']).max(axis=1)
    err = d_off.max() / np.abs(s['off']).max()
    print("nside %d  pix_offsets fp64: %.3e of max|offset| (worst pixel %d, %d pixels beyond the bound)"
          % (nside, err, int(d_off.argmax()), int((d_off > 1e-10 * np.abs(s['off']).max()).sum())))
    assert err <= 1e-10
    resolved, disp = plan.precision(_lib.ACC_AUTO)
    modes = [('default', _lib.ACC_AUTO, 1e-6 / ora.mean()), ('fp64', _lib.ACC_F64, 1e-10 / np.abs(ora).max()),
             ('parity', _lib.ACC_PARITY, 1e-8 / ora.mean())]
    if disp < 0.1:
        modes.append(('fp32', _lib.ACC_F32, 1e-6 / ora.mean()))
    if nside == 64:
        assert disp < 0.1                                                  # the fp32 records are exercised on this shell
    errs = {}
    for name, acc, inv_scale in modes:
        work = torch.zeros(npix * 3, dtype=torch.float64, device=dev)      # 24 bytes per pixel
        out = torch.full((npix,), np.nan, dtype=torch.float64, device=dev)
        sums = torch.zeros(2, dtype=torch.float64, device=dev)
        plan.baryonify(cd, d_map.data_ptr(), work.data_ptr(), out.data_ptr(), sums.data_ptr(), acc)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        errs[name] = np.abs(o - ora).max() * inv_scale
        print("nside %d  %-7s (resolves to %d, table moves %.3f pixel sides): %.3e of its tolerance" % (nside, name, plan.precision(acc)[0], disp, errs[name]))
        sm = sums.cpu().numpy()
        assert np.isclose(sm[1], sm[0]) and np.isclose(o.sum(), hmap.sum())
    plan.status()
    plan.close()
    for name, e in errs.items():
        assert e <= 1.0, (name, e)
