"""The plan's ring table (csrc/bfgx_kernels.hpp RingRec, Tiling.rings): the geometry of every ring, filled once at plan creation and read by
K1 (TileRow / RingC2, the flush's first pixels) and K2 (RegRow / RegRowC / RowScan, the rings beyond a tile's window) instead of being derived
per tile and step.

1. the table against the device functions it replaces, bit for bit;
2. small shells, where the table's edge records (the two "no such ring" records, the rings next to the poles) are in every tile's window, end
   to end against the CPU oracle, in every precision and both forms of the fast K1 kernel;
3. a second plan at another NSIDE in the same process: the table belongs to the plan.
(That the step computes the same map as before the table existed is checked against a build of the parent commit when the change is measured;
a test cannot hold the parent's build.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO_PI = 6.283185307179586476925286766559005768394       # csrc/bfgx_kernels.hpp kTwoPi, kInvTwoPi
INV_TWO_PI = 1.0 / TWO_PI


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _tiny_plan(nside):
    import torch
    from baryonification_amd import engine, synthetic as syn
    z, M, r = np.geomspace(0.1, 0.2, 3), np.geomspace(1e13, 1e14, 3), np.geomspace(1e-2, 10, 8)
    model, keep = engine.model_from_tables([np.log(1 + z), np.log(M), np.log(r)], np.zeros((3, 3, 8)), syn.COSMO, 10.0)
    return engine.ShellPlan(model, keep, nside, 16, 0, torch.cuda.current_stream().cuda_stream)


def _ring_integers(nside, ring):
    """start, length and shift flag of RING-ordered rings from the definition of the pixelisation (Gorski et al. 2005)"""
    ring = np.asarray(ring, dtype=np.int64)
    npix, ncap = 12 * nside * nside, 2 * nside * (nside - 1)
    q = 4 * nside - ring
    north, south = ring < nside, ring >= 3 * nside
    nr = np.where(north, 4 * ring, np.where(south, 4 * q, 4 * nside))
    start = np.where(north, 2 * ring * (ring - 1), np.where(south, npix - 2 * q * (q + 1), ncap + (ring - nside) * 4 * nside))
    shifted = np.where(north | south, 1, ((ring - nside) & 1) == 0)
    return start, nr, shifted.astype(np.int64)


@pytest.mark.parametrize('nside', [1, 2, 4, 16, 64, 1024, 8192])
def test_ring_table_equals_the_device_functions_bit_for_bit(gpu, nside):
    """every field of the table with == on the bit patterns against ring_info_small, ring_z_sth and ring_theta_nolibm called on their own
    (bfgx_debug_ring_table's second mode, and the math probe's ring_theta) and the quotients formed from them in IEEE arithmetic: every ring
    up to NSIDE 64, the rings where the pixelisation changes its rule beyond; the two "no such ring" records; no spacing beyond ring 1 and
    ring 4 NSIDE - 1"""
    from baryonification_amd import engine
    nl4 = 4 * nside
    plan = _tiny_plan(nside)
    tab = plan.ring_table()
    assert tab.size == nl4 + 1
    if nside <= 64:
        rings = np.arange(1, nl4)
    else:
        rings = np.array([1, 2, nside - 1, nside, nside + 1, 2 * nside, 3 * nside - 1, 3 * nside, 3 * nside + 1, nl4 - 1])
    # the functions, ring by ring and for the two neighbours (the spacings); runs of consecutive rings in one call
    want = sorted(set(int(r) + d for r in rings for d in (-1, 0, 1) if 1 <= r + d <= nl4 - 1))
    fn = {}
    i = 0
    while i < len(want):
        j = i
        while j + 1 < len(want) and want[j + 1] == want[j] + 1:
            j += 1
        rec = plan.ring_table(want[i], j - i + 1, from_functions=True)
        for k in range(j - i + 1):
            fn[want[i] + k] = rec[k]
        i = j + 1
    plan.close()
    wr = np.array(want, dtype=np.int64)
    f = np.array([fn[r] for r in want], dtype=tab.dtype)
    theta_probe = engine.math_probe('ring_theta', np.full(wr.size, float(nside)), wr.astype(np.float64))
    assert np.array_equal(_bits(f['theta']), _bits(theta_probe))
    start, nr, shifted = _ring_integers(nside, wr)
    assert np.array_equal(f['start'], start) and np.array_equal(f['nr'], nr) and np.array_equal(f['shifted'], shifted)
    theta = dict(zip(want, f['theta']))
    t = tab[wr]
    for k in ('theta', 'z', 'sth'):
        assert np.array_equal(_bits(t[k]), _bits(f[k])), k
    for k in ('start', 'nr', 'shifted'):
        assert np.array_equal(t[k], f[k]), k
    nrd = f['nr'].astype(np.float64)
    assert np.array_equal(_bits(t['dphi']), _bits(TWO_PI / nrd))
    assert np.array_equal(_bits(t['inv_dphi']), _bits(nrd * INV_TWO_PI))
    sel = np.isin(wr, rings)
    up = np.array([1.0 / (theta[r] - theta[r - 1]) if r > 1 else 0.0 for r in wr[sel]])
    dn = np.array([1.0 / (theta[r + 1] - theta[r]) if r < nl4 - 1 else 0.0 for r in wr[sel]])
    assert np.array_equal(_bits(t['inv_dth_up'][sel]), _bits(up)) and np.array_equal(_bits(t['inv_dth_dn'][sel]), _bits(dn))
    # the edges
    assert tab['inv_dth_up'][1] == 0.0 and tab['inv_dth_dn'][nl4 - 1] == 0.0
    for ring, th in ((0, -1.0e300), (nl4, 1.0e300)):
        e = tab[ring]
        assert e['nr'] == 0 and e['theta'] == th and e['start'] == 0 and e['shifted'] == 0
        assert all(e[k] == 0.0 for k in ('z', 'sth', 'dphi', 'inv_dphi', 'inv_dth_up', 'inv_dth_dn'))
    if nside > 1:
        assert np.all(np.diff(tab['theta'][1:nl4]) > 0) and np.all(tab['inv_dth_dn'][1:nl4 - 1] == tab['inv_dth_up'][2:nl4])


# ------------------------------------------------------------------------------------------ small shells against the oracle
N_HALOS = 2000
MAX_MOVE_PIXELS = 12.0      # the table is scaled so that the pixel that moves furthest moves this many pixel sides (within 5 .. 20)
_shell = {}


def _catalog():
    from baryonification_amd import synthetic as syn
    cat = syn.make_catalog(N_HALOS)
    rng = np.random.default_rng(7)
    cat['dec'][:30] = rng.uniform(85.0, 90.0, 30)               # discs over the north / south pole
    cat['dec'][30:60] = -rng.uniform(85.0, 90.0, 30)
    cat['dec'][60], cat['dec'][61] = 90.0 - 1e-8, -90.0 + 1e-8
    return cat


def _small_shell(nside):
    """inputs, the oracle's map and the oracle's pix_offsets (routes) of one small shell; computed once"""
    if nside in _shell:
        return _shell[nside]
    from baryonification_amd import synthetic as syn
    from oracle import oracle as O
    if 'table' not in _shell:
        cat = _catalog()
        z, M, r = syn.table_grid(cat, Nz=3, NM=8, NR=200, pad=1e-9)
        _shell['table'] = (cat, z, M, r, syn.s19_displacement_table(z, M, r))
    cat, z, M, r, d0 = _shell['table']
    axes = [np.log(1 + z), np.log(M), np.log(r)]
    bg = O.Background.from_dict(syn.COSMO)
    hmap = syn.make_map(nside, seed=100 + nside)
    pix = np.sqrt(4 * np.pi / hmap.size)
    # pix_offsets are linear in the table: one evaluation at scale 1 fixes the scale
    o1 = O.baryonify_offsets(nside, cat, O.Table(axes, d0, False, 10.0), 10.0, bg)
    scale = MAX_MOVE_PIXELS * pix / np.sqrt((o1 ** 2).sum(axis=1)).max()
    off = o1 * scale
    ora = O.baryonify_shell(nside, hmap, cat, O.Table(axes, scale * d0, False, 10.0), 10.0, bg)
    assert np.isclose(ora.sum(), hmap.sum())
    _shell[nside] = dict(cat=cat, axes=axes, table=scale * d0, hmap=hmap, ora=ora, off=off, pix=pix)
    return _shell[nside]


def _routes(nside, s, band_first_pixel):
    """pixels per route of the gathering regrid, from the oracle's pix_offsets alone (csrc/bfgx_regrid2.hpp: gathered <=> |o| < lim(ring)):
    own = gathered, (apron) gathered on the first / last ring of a band of the tiling and moving out of the band, far = not gathered"""
    from oracle import oracle as O
    npix = s['hmap'].size
    v = O.pix2vec(nside, np.arange(npix))
    start, nr, _ = _ring_integers(nside, np.arange(1, 4 * nside))
    ring = np.searchsorted(start, np.arange(npix), side='right')              # 1 .. 4 nside - 1
    theta = np.arccos(np.clip(v[:, 2], -1, 1))
    th_ring = np.array([theta[st] for st in start])
    cap = min(9.9 / nside, 0.02)
    lim = np.minimum(np.minimum(cap, 0.09 * np.sin(theta)), 0.999 * np.minimum(theta - th_ring[0], th_ring[-1] - theta))
    lim[(ring <= 1) | (ring >= 4 * nside - 1)] = 0.0
    mag = np.sqrt((s['off'] ** 2).sum(axis=1))
    live = s['hmap'] > 0
    gathered = live & (mag < lim)
    w = v + s['off']
    znew = w[:, 2] / np.sqrt((w ** 2).sum(axis=1))
    first_ring = np.searchsorted(start, band_first_pixel[:-1], side='right')     # first ring of every band
    on_first, on_last = np.isin(ring, first_ring), np.isin(ring + 1, first_ring)
    apron = gathered & (mag > 0) & ((on_first & (znew > v[:, 2]) & (ring > 1)) | (on_last & (znew < v[:, 2])))
    return dict(own=int((gathered & ~apron).sum()), apron=int(apron.sum()), far=int((live & ~gathered).sum()),
                moved=float(mag.max() / s['pix']))


@pytest.mark.parametrize('fluid', [2, 0])
@pytest.mark.parametrize('nside', [8, 16, 64])
def test_small_shells_vs_oracle_every_precision_both_k1_forms(gpu, monkeypatch, nside, fluid):
    """NSIDE 8 and 16 (every tile is polar or spans whole rings), 64: 2 000 halos, some over the poles, on the Schneider19 table scaled so that
    the pixel that moves furthest moves 12 pixel sides.  fp64 throughout to 1e-10 of the map's scale, the default call (the plan picks the
    parity-grade mode for this table) and the parity-grade mode to 1e-6 mean(map) (tests/test_gpu_parity.py), mass conserved; the fast K1
    kernel in its fluid form (forced) and barrier per tile.
    fp32 pair math does not hold 1e-6 mean(map) on a table that moves pixels this far, with or without the ring table (which is why the plan
    does not pick it; tests/test_gpu_fullsize.py asserts as much on the benchmark table): every (halo, pixel) contribution carries ~4e-7 of
    itself (a few fp32 roundings), so a source pixel that moves P pixel sides is placed to 4e-7 P of a pixel side and the bilinear deposit
    turns that into 4e-7 P of its value.  Its bound here is that model at P = 12 and the largest pixel value: 4e-7 x 12 x max(map), 1.3e-5
    mean(map).  Measured: 1.7e-5 / 3.2e-5 / 3.9e-5 absolute at NSIDE 8 / 16 / 64 (2.1e-6 / 4.0e-6 / 4.9e-6 mean(map)) against bounds of
    9.6e-5 / 1.0e-4 / 1.1e-4; fp64 1.5e-12 / 1.0e-12 / 4.8e-12, parity-grade 1.1e-10 / 6.9e-11 / 3.7e-10; the same in both K1 forms.
    The gathering regrid caps a gathered move at 0.02 rad whatever the NSIDE -- 0.16 pixel sides at NSIDE 8, 1.25 at NSIDE 64 -- so on these
    shells the pixels that move far take the far list, the window holds one ring of apron (two at NSIDE 64, where the walking kernel runs) and
    reaches the "no such ring" records in both polar bands; the many-ring aprons belong to NSIDE >= 256 (tests/test_gpu_fullsize.py)."""
    import torch
    from baryonification_amd import _lib, engine, synthetic as syn
    s = _small_shell(nside)
    monkeypatch.setenv('BFGX_K1_FLUID', str(fluid))
    model, keep = engine.model_from_tables(s['axes'], s['table'], syn.COSMO, 10.0, 10.0)
    dev = torch.device('cuda', 0)
    plan = engine.ShellPlan(model, keep, nside, N_HALOS, 0, torch.cuda.current_stream().cuda_stream)
    routes = _routes(nside, s, plan.bands())
    print("nside %d: routes from the oracle's offsets %s" % (nside, routes))
    assert routes['own'] > 0 and routes['apron'] > 0 and routes['far'] > 0 and 5.0 <= routes['moved'] <= 20.0, routes
    cat = s['cat']
    cols = {k: torch.from_numpy(np.ascontiguousarray(cat[k])).to(dev) for k in ('M', 'z', 'ra', 'dec')}
    lnz, lnM = _lib.table_coords(cat['M'], cat['z'])
    cols['lnz'], cols['lnM'] = torch.from_numpy(lnz).to(dev), torch.from_numpy(lnM).to(dev)
    cd = _lib.make_catalog_dev(N_HALOS, cols['M'].data_ptr(), cols['z'].data_ptr(), cols['ra'].data_ptr(), cols['dec'].data_ptr(),
                               ln1pz_ptr=cols['lnz'].data_ptr(), lnM_ptr=cols['lnM'].data_ptr())
    npix = s['hmap'].size
    d_map = torch.from_numpy(s['hmap']).to(dev)
    ora = s['ora']
    err = {}
    assert plan.precision(_lib.ACC_AUTO)[0] == _lib.ACC_PARITY
    for name, acc, tol in (('f64', _lib.ACC_F64, 1e-10 * np.abs(ora).max()), ('auto', _lib.ACC_AUTO, 1e-6 * ora.mean()),
                           ('parity', _lib.ACC_PARITY, 1e-6 * ora.mean()), ('f32', _lib.ACC_F32, 4e-7 * MAX_MOVE_PIXELS * s['hmap'].max())):
        off = torch.zeros(npix * 3, dtype=torch.float64, device=dev)
        out = torch.zeros(npix, dtype=torch.float64, device=dev)
        sums = torch.zeros(2, dtype=torch.float64, device=dev)
        plan.baryonify(cd, d_map.data_ptr(), off.data_ptr(), out.data_ptr(), sums.data_ptr(), acc_f64=acc)
        torch.cuda.synchronize()
        plan.status()
        st = plan.regrid_stats()
        got, sm = out.cpu().numpy(), sums.cpu().numpy()
        err[name] = (np.abs(got - ora).max(), tol)
        print("nside %d fluid %d %-6s max |hip - oracle| = %.3e (tolerance %.3e)  sums %r  %s" % (nside, fluid, name, err[name][0], tol, sm.tolist(), st))
        assert np.isclose(sm[1], sm[0]) and np.isclose(got.sum(), s['hmap'].sum())          # mass_conserved (HealpixRunner.py:344-346)
        assert st['far_listed'] > 0 and not st['far_overflowed'], st
        if nside == 64:
            assert st['tiles_walked'] > 0 and st['max_reach_rings'] >= 2, st
    plan.close()
    for name, (e, tol) in err.items():
        assert e <= tol, (name, e, tol)


# ------------------------------------------------------------------------------------------ the table belongs to the plan
_FRESH = """
import sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from test_gpu_ring_table import _one_shot
np.save(sys.argv[1], _one_shot(64))
"""


def _one_shot(nside):
    """BaryonifyShell.process() (the one-shot entry and its plan cache) on a small synthetic shell, default precision"""
    import baryonification_amd as bfg
    from baryonification_amd import synthetic as syn
    cat = syn.make_catalog(500, seed=5)
    z, M, r = syn.table_grid(cat, Nz=3, NM=4, NR=64, pad=1e-9)
    d = 40.0 * syn.displacement_table(z, M, r)
    cosmo = bfg.utils.Cosmology.from_dict(syn.COSMO)
    Catalog = bfg.utils.HaloLightConeCatalog(ra=cat['ra'], dec=cat['dec'], M=cat['M'], z=cat['z'], cosmo=syn.COSMO)
    model = bfg.Profiles.Baryonification2D(None, None, cosmo, epsilon_max=10.0)
    model.set_table(z, M, r, d)
    Shell = bfg.utils.LightconeShell(map=syn.make_map(nside, seed=11), cosmo=syn.COSMO)
    return bfg.Runners.BaryonifyShell(Catalog, Shell, 10.0, model, verbose=False).process()


def test_plans_of_two_nsides_in_one_process_keep_their_own_tables(gpu, tmp_path):
    """NSIDE 64, then 16, then 64 again through the plan cache of the one-shot entry: the third map equals the first and what a fresh
    process computes (to the order of LDS accumulation: 1e-12 mean(map)), and the NSIDE-16 map what a lone NSIDE-16 plan gives"""
    a64 = _one_shot(64)
    a16 = _one_shot(16)
    b64 = _one_shot(64)
    assert a64.size == 12 * 64 * 64 and a16.size == 12 * 16 * 16
    assert np.abs(a64 - syn_map(64)).max() > 0                                     # the shell really moved
    assert np.abs(b64 - a64).max() <= 1e-12 * a64.mean()
    path = str(tmp_path / 'fresh64.npy')
    subprocess.run([sys.executable, '-c', _FRESH % (REPO, os.path.join(REPO, 'tests')), path], check=True, timeout=300)
    fresh = np.load(path)
    assert np.abs(b64 - fresh).max() <= 1e-12 * fresh.mean()
    from baryonification_amd import _lib
    _lib.load().bfgx_cache_clear()
    assert np.abs(_one_shot(16) - a16).max() <= 1e-12 * a16.mean()


def syn_map(nside):
    from baryonification_amd import synthetic as syn
    return syn.make_map(nside, seed=11)
