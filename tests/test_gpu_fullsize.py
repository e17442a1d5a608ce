"""BASELINE.json full-size configurations on the GPU: config 2 (1e6 halos, NSIDE 1024, BaryonifyShell) against the
CPU oracle on the FULL input, and size-independent properties (mass conservation, linearity over catalog splits,
shuffle invariance, agreement of the two accumulation algorithms) for configs 2 and 3 (PaintProfilesShell, NSIDE 2048)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _setup(N, nside, paint, pad=1e-9):
    import torch
    from baryonification_amd import _lib, engine, synthetic as syn
    cat = syn.make_catalog(N)
    z, M, r = syn.table_grid(cat, pad=pad)
    table = syn.paint_table(z, M, r) if paint else syn.displacement_table(z, M, r)
    axes = [np.log(1 + z), np.log(M), np.log(r)]
    model, keep = engine.model_from_tables(axes, np.log(table) if paint else table, syn.COSMO, 10.0, 10.0, log_values=paint)
    dev = torch.device('cuda', 0)
    plan = engine.ShellPlan(model, keep, nside, N, 0, torch.cuda.current_stream().cuda_stream)
    return torch, _lib, syn, cat, axes, table, plan, dev


def _cat_dev(torch, _lib, dev, cat, idx=None, coords=False):
    cols = {k: torch.from_numpy(np.ascontiguousarray(v if idx is None else v[idx])).to(dev) for k, v in cat.items()}
    n = cols['M'].numel()
    if coords:        # the (z, M) table coordinates as the caller's numpy computes them (bfgx_catalog.ln1pz / lnM)
        lnz, lnM = _lib.table_coords(cat['M'] if idx is None else cat['M'][idx], cat['z'] if idx is None else cat['z'][idx])
        cols['lnz'], cols['lnM'] = torch.from_numpy(lnz).to(dev), torch.from_numpy(lnM).to(dev)
        return _lib.make_catalog_dev(n, cols['M'].data_ptr(), cols['z'].data_ptr(), cols['ra'].data_ptr(), cols['dec'].data_ptr(),
                                     ln1pz_ptr=cols['lnz'].data_ptr(), lnM_ptr=cols['lnM'].data_ptr()), cols
    return _lib.make_catalog_dev(n, cols['M'].data_ptr(), cols['z'].data_ptr(), cols['ra'].data_ptr(), cols['dec'].data_ptr()), cols


def test_config2_full_size_vs_oracle_and_properties(gpu):
    N, nside = 1_000_000, 1024
    torch, _lib, syn, cat, axes, table, plan, dev = _setup(N, nside, paint=False)
    npix = 12 * nside * nside
    hmap = syn.make_map(nside)
    d_map = torch.from_numpy(hmap).to(dev)

    def offsets(cd, acc_f64, algo):
        plan.set_algo(algo)
        off = torch.zeros(npix * 3, dtype=torch.float64 if acc_f64 else torch.float32, device=dev)
        plan.offsets(cd, off.data_ptr(), acc_f64)
        return off

    def regrid(off, acc_f64):
        out = torch.zeros(npix, dtype=torch.float64, device=dev)
        sums = torch.zeros(2, dtype=torch.float64, device=dev)
        plan.regrid(d_map.data_ptr(), off.data_ptr(), out.data_ptr(), sums.data_ptr(), acc_f64)
        torch.cuda.synchronize()
        return out.cpu().numpy(), sums.cpu().numpy()

    cd, keep1 = _cat_dev(torch, _lib, dev, cat)
    off64 = offsets(cd, True, 1)
    plan.status()
    new_map, sums = regrid(off64, True)
    assert np.isclose(sums[1], sums[0]) and np.isclose(new_map.sum(), hmap.sum())          # HealpixRunner.py:344-346

    # (a) the CPU oracle on the full 1e6-halo input
    from oracle import oracle as O
    tab = O.Table(axes, table, False, 10.0)
    ora = O.baryonify_shell(nside, hmap, cat, tab, 10.0, O.Background.from_dict(syn.COSMO))
    assert np.abs(new_map - ora).max() <= 1e-10 * np.abs(ora).max()
    # default accumulators (f32 pix_offsets): the stated 1e-6 * mean(map) tolerance
    new32, s32 = regrid(offsets(cd, False, 1), False)
    assert np.abs(new32 - ora).max() <= 1e-6 * ora.mean() and np.isclose(s32[1], s32[0])
    # the FUSED call bench.py times (bfgx_baryonify_device: K0 + K1 + K2 in one enqueue, fp32 pix_offsets, K1's per-tile maxima
    # handed to K2), with the caller's table coordinates as bench.py passes them: straight against the oracle, same tolerance
    cdc, keepc = _cat_dev(torch, _lib, dev, cat, coords=True)
    plan.set_algo(1)
    f_off = torch.zeros(npix * 3, dtype=torch.float32, device=dev)
    f_out = torch.zeros(npix, dtype=torch.float64, device=dev)
    f_sums = torch.zeros(2, dtype=torch.float64, device=dev)
    plan.baryonify(cdc, d_map.data_ptr(), f_off.data_ptr(), f_out.data_ptr(), f_sums.data_ptr(), acc_f64=False)
    torch.cuda.synchronize()
    plan.status()
    fused, fs = f_out.cpu().numpy(), f_sums.cpu().numpy()
    assert np.abs(fused - ora).max() <= 1e-6 * ora.mean() and np.isclose(fs[1], fs[0]) and np.isclose(fused.sum(), hmap.sum())
    del f_off, f_out

    # (b) the two accumulation algorithms agree.  pix_offsets are differences of unit vectors, so the rounding
    # floor is absolute (~1e-16 per contribution), not relative to the ~5e-5 offsets
    ATOL = 2e-14
    off_a0 = offsets(cd, True, 0)
    torch.cuda.synchronize()
    assert (off_a0 - off64).abs().max().item() <= ATOL

    # (c) linearity over a catalog split and invariance under a shuffle
    idx = np.random.default_rng(5).permutation(N)
    cdA, kA = _cat_dev(torch, _lib, dev, cat, idx[: N // 3])
    cdB, kB = _cat_dev(torch, _lib, dev, cat, idx[N // 3:])
    lin = offsets(cdA, True, 1) + offsets(cdB, True, 1)
    torch.cuda.synchronize()
    assert (lin - off64).abs().max().item() <= ATOL
    cdS, kS = _cat_dev(torch, _lib, dev, cat, idx)
    sh = offsets(cdS, True, 1)
    torch.cuda.synchronize()
    assert (sh - off64).abs().max().item() <= ATOL
    # pair census: tile path == per-halo path == number of (halo, pixel) pairs the oracle visits on a sample
    plan.set_algo(1); n1 = plan.count_pairs(cd, True)
    plan.set_algo(0); n0 = plan.count_pairs(cd, True)
    assert n0 == n1 > 5e7
    plan.close()


def test_config2_s19_benchmark_table_full_size_vs_oracle(gpu):
    """SURVEY 8(d) table (ii), the BENCHMARK table (Schneider19 one-halo displacements built by K4-K6), at config 2's full size, exactly as
    bench.py's `value_s19` runs it: K0 + K1 + K2 in one call against the CPU oracle on the same table.  Displacements of 1.9 pixels on
    average and 20 at most: every tile takes the walking kernel (window scan + compaction) and the pixels beyond the cap the far list --
    the path the closed-form table never enters."""
    import torch
    from baryonification_amd import _lib, engine, synthetic as syn
    from oracle import oracle as O
    N, nside = 1_000_000, 1024
    npix = 12 * nside * nside
    cat = syn.make_catalog(N)
    z, M, r = syn.table_grid(cat)                                  # edges == catalog min / max, as bench.py (README.md:78-80)
    table = syn.s19_displacement_table(z, M, r)
    axes = [np.log(1 + z), np.log(M), np.log(r)]
    model, keep = engine.model_from_tables(axes, table, syn.COSMO, 10.0, 10.0)
    dev = torch.device('cuda', 0)
    plan = engine.ShellPlan(model, keep, nside, N, 0, torch.cuda.current_stream().cuda_stream)
    hmap = syn.make_map(nside)
    d_map = torch.from_numpy(hmap).to(dev)
    cdc, keepc = _cat_dev(torch, _lib, dev, cat, coords=True)
    ora = O.baryonify_shell(nside, hmap, cat, O.Table(axes, table, False, 10.0), 10.0, O.Background.from_dict(syn.COSMO))
    assert np.isclose(ora.sum(), hmap.sum())
    # what the plan chose for this table: it moves a pixel by ~9 pixel sides per halo, far beyond what fp32 pair math holds to 1e-6 mean(map)
    res_auto, disp_px = plan.precision(_lib.ACC_AUTO)
    assert res_auto == _lib.ACC_PARITY and 5.0 < disp_px < 20.0, (res_auto, disp_px)
    res = {}
    for name, acc in (('auto', _lib.ACC_AUTO), ('f64', _lib.ACC_F64), ('parity', _lib.ACC_PARITY), ('f32', _lib.ACC_F32)):
        off = torch.zeros(npix * 3, dtype=torch.float32 if acc == _lib.ACC_F32 else torch.float64, device=dev)      # (24 bytes per pixel unless fp32)
        out = torch.zeros(npix, dtype=torch.float64, device=dev)
        sums = torch.zeros(2, dtype=torch.float64, device=dev)
        plan.baryonify(cdc, d_map.data_ptr(), off.data_ptr(), out.data_ptr(), sums.data_ptr(), acc_f64=acc)
        torch.cuda.synchronize()
        plan.status()
        st = plan.regrid_stats()
        got, sm = out.cpu().numpy(), sums.cpu().numpy()
        assert np.isclose(sm[1], sm[0]) and np.isclose(got.sum(), hmap.sum())                   # HealpixRunner.py:344-346
        # the tiles really walked and the far list was really used
        assert st['max_reach_rings'] > 8 and st['tiles_walked'] > 5500 and st['far_listed'] > 1000 and not st['far_overflowed'], st
        res[name] = np.abs(got - ora).max()
        if acc in (_lib.ACC_F32, _lib.ACC_F64):
            mag = torch.linalg.norm(off.view(-1, 3).double(), dim=1)
        else:                                                                                    # split pix_offsets: hi [npix][3], then lo [npix][3]
            o32 = off.view(torch.float32)
            mag = torch.linalg.norm(o32[:npix * 3].view(-1, 3).double() + o32[npix * 3:].view(-1, 3).double(), dim=1)
        assert float(mag.max()) > 15 * np.sqrt(4 * np.pi / npix) and float(mag.mean()) > 1.5 * np.sqrt(4 * np.pi / npix)      # pixels move
        del off, out, mag
    print("S19 table, 1e6 / 1024: max |hip - oracle| fp64 %.3e (%.1e of max); of mean(map): default (auto) %.2e, parity-grade %.2e, fp32 pair math %.2e" % (
        res['f64'], res['f64'] / np.abs(ora).max(), res['auto'] / ora.mean(), res['parity'] / ora.mean(), res['f32'] / ora.mean()))
    assert res['f64'] <= 1e-10 * np.abs(ora).max()
    # THE CONTRACT (SURVEY 8(d) "Parity tolerance"): |d| <= 1e-6 mean(map) per pixel -- for the DEFAULT call (BFGX_ACC_AUTO: what the runners
    # pass when acc_f64 is None), on the benchmark table.  The parity-grade mode sits four orders of magnitude inside it (measured 1.7e-10).
    assert res['auto'] <= 1e-6 * ora.mean()
    assert res['parity'] <= 1e-8 * ora.mean()
    # fp32 pair math (--precision f32, what rounds 1-4 ran by default): every (halo, pixel) contribution carries ~4e-7 of itself, i.e.
    # (d / pixel) x 4e-7 of a pixel in the bilinear weights.  Below a pixel of displacement that is the 1e-6 (closed-form table: 2.4e-7
    # measured); this table moves pixels by up to 20: 2.1e-5 mean(map) measured, which is why the plan does not pick it here.
    assert 1e-6 * ora.mean() < res['f32'] <= 5e-5 * ora.mean()
    plan.close()


def test_config3_paint_full_size_properties(gpu):
    N, nside = 1_000_000, 2048
    torch, _lib, syn, cat, axes, table, plan, dev = _setup(N, nside, paint=True)
    npix = 12 * nside * nside

    def paint(cd, algo, acc_f64=True):
        plan.set_algo(algo)
        out = torch.zeros(npix, dtype=torch.float64 if acc_f64 else torch.float32, device=dev)
        plan.paint(cd, out.data_ptr(), acc_f64)
        return out

    cd, keep1 = _cat_dev(torch, _lib, dev, cat)
    full = paint(cd, 1)
    plan.status()
    torch.cuda.synchronize()
    scale = full.abs().max().item()
    assert scale > 0 and torch.isfinite(full).all().item() and full.min().item() >= 0
    assert (paint(cd, 0) - full).abs().max().item() <= 1e-11 * scale                       # algorithms agree (rounding of the azimuth differs)
    idx = np.random.default_rng(6).permutation(N)
    cdA, kA = _cat_dev(torch, _lib, dev, cat, idx[: N // 2])
    cdB, kB = _cat_dev(torch, _lib, dev, cat, idx[N // 2:])
    assert (paint(cdA, 1) + paint(cdB, 1) - full).abs().max().item() <= 1e-11 * scale       # linearity (Parallelize.py:318)
    f32 = paint(cd, 1, acc_f64=False)
    assert (f32.double() - full).abs().max().item() <= 1e-5 * scale                         # stated fp32 tolerance
    # acc_f64 = 2: fp32 pair math accumulated in fp64 into the double map (what bench.py --mode paint times by default).  Stated
    # fp64 -> fp32 tolerance: 5e-5 of the pixel's value (ln r and the read-out of ln P in fp32, then exp)
    mixed = paint(cd, 1, acc_f64=2)
    assert mixed.dtype == torch.float64 and torch.isfinite(mixed).all().item()
    assert ((mixed - full).abs() <= 5e-5 * full + 1e-12 * scale).all().item()
    assert (mixed - full).abs().max().item() <= 1e-5 * scale
    assert abs(mixed.sum().item() / full.sum().item() - 1.0) <= 1e-6
    # oracle on a 20 000-halo sample of the same catalog
    from oracle import oracle as O
    sub = {k: v[:20000] for k, v in cat.items()}
    with np.errstate(divide='ignore'):
        tab = O.Table(axes, np.log(table))
    ora = O.paint_shell(nside, sub, tab, 10.0, O.Background.from_dict(syn.COSMO))
    cdS, kS = _cat_dev(torch, _lib, dev, cat, np.arange(20000))
    got = paint(cdS, 1).cpu().numpy()
    assert np.abs(got - ora).max() <= 1e-10 * np.abs(ora).max()
    plan.close()


def test_banded_regrid_equals_full_regrid(gpu):
    """multi-GPU building block on one GPU: every "rank" regrids the OUTPUT pixels of its bands from the summed pix_offsets of
    those bands + one ring either side (what sliced_reduce + halo_exchange hand it); the disjoint slices put side by side
    (+ the listed far deposits) are the full-map regrid (what N ranks + gather_slices do)"""
    import torch
    from baryonification_amd import _lib, engine, synthetic as syn
    from baryonification_amd.utils.Parallelize import band_partition
    nside, nh = 256, 60_000
    npix = 12 * nside * nside
    cat = syn.make_catalog(nh)
    cat['dec'][:6] = [89.9, -89.95, 89.99, -89.8, 89.7, -89.999]        # some halos on the pole caps: pixels of the first / last rings move
    z, M, r = syn.table_grid(cat)
    model, keep = engine.model_from_tables([np.log(1 + z), np.log(M), np.log(r)], syn.displacement_table(z, M, r), syn.COSMO, 10.0, 10.0)
    dev = torch.device('cuda:0')
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in cat.items()}
    plan = engine.ShellPlan(model, keep, nside, nh, device=0, stream=torch.cuda.current_stream().cuda_stream)
    cd = _lib.make_catalog_dev(nh, t['M'].data_ptr(), t['z'].data_ptr(), t['ra'].data_ptr(), t['dec'].data_ptr())
    off = torch.zeros(npix * 3, dtype=torch.float32, device=dev)
    plan.offsets(cd, off.data_ptr(), acc_f64=False)
    hmap = torch.from_numpy(syn.make_map(nside)).to(dev)
    full = torch.full((npix,), np.nan, dtype=torch.float64, device=dev)          # not zeroed: every pixel must be stored
    sums = torch.zeros(2, dtype=torch.float64, device=dev)
    plan.regrid(hmap.data_ptr(), off.data_ptr(), full.data_ptr(), sums.data_ptr(), acc_f64=False)
    torch.cuda.synchronize()
    assert torch.isfinite(full).all().item() and np.isclose(sums[1].item(), sums[0].item()) and np.isclose(full.sum().item(), hmap.sum().item())
    first = plan.bands()
    assert first[0] == 0 and first[-1] == npix and np.all(np.diff(first) > 0)
    for world in (2, 5):
        cuts = band_partition(first, world)
        pb = first[cuts]
        acc = torch.full((npix,), np.nan, dtype=torch.float64, device=dev)
        s_in = s_out = 0.0
        far_p, far_v = [], []
        for rk in range(world):
            p0, p1 = int(pb[rk]), int(pb[rk + 1])
            olo, ohi = plan.band_apron(int(cuts[rk]), int(cuts[rk + 1]))
            assert olo <= p0 and ohi >= p1 and (rk == 0) == (olo == 0) and (rk == world - 1) == (ohi == npix)
            my_off = off[3 * olo:3 * ohi].clone()                   # what sliced_reduce + halo_exchange hand to rank rk
            sl = acc[p0:p1]
            sm = torch.zeros(2, dtype=torch.float64, device=dev)
            plan.regrid_bands(int(cuts[rk]), int(cuts[rk + 1]), hmap.data_ptr(), my_off.data_ptr(), olo, ohi, sl.data_ptr(), sm.data_ptr())
            fp, fv = plan.far_fetch()
            far_p.append(fp); far_v.append(fv)
            s_in += sm[0].item(); s_out += sm[1].item()
        fp, fv = np.concatenate(far_p), np.concatenate(far_v)
        if fp.size:
            acc.index_add_(0, torch.from_numpy(fp).to(dev), torch.from_numpy(fv).to(dev))
        plan.status()
        torch.cuda.synchronize()
        assert np.isclose(s_in, hmap.sum().item()) and np.isclose(s_out, s_in)
        # identical tiles evaluate identical pixels: the banded slices ARE the full-map regrid up to the order of LDS additions
        assert (acc - full).abs().max().item() <= 1e-12 * full.abs().max().item()
    # an offsets range that does not reach one ring beyond the bands is refused
    p0, p1 = int(pb[1]), int(pb[2])
    with pytest.raises(ValueError, match=r'1 ring\(s\) either side'):
        plan.regrid_bands(int(cuts[1]), int(cuts[2]), hmap.data_ptr(), off[3 * p0:3 * p1].clone().data_ptr(), p0, p1, acc[p0:p1].data_ptr())
    plan.close()


def _random_offsets(nside, scale_pix, seed):
    """a displacement field with |offset| from 0 to `scale_pix` pixel sizes: smooth large-scale part + per-pixel scatter"""
    rng = np.random.default_rng(seed)
    npix = 12 * nside * nside
    pix = np.sqrt(4 * np.pi / npix)
    mag = scale_pix * pix * rng.random(npix) ** 2
    d = rng.normal(size=(npix, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return d * mag[:, None]


@pytest.mark.parametrize('nside,scale', [(128, 0.4), (128, 2.5), (128, 9.0), (128, 40.0), (64, 25.0), (512, 6.0), (512, 60.0), (256, 200.0), (512, 200.0)])
def test_regrid_any_displacement_vs_oracle(gpu, monkeypatch, nside, scale):
    """K2 for displacements from a fraction of a pixel to 200 pixels (the gathering regrid sizes its aprons from the data;
    what it does not gather goes through the far list, and through the in-stream repair pass when that list overflows:
    NSIDE 512 x 60 pixels lists ~8e6 deposits against a capacity forced down to 1e6 -- a plan's own list holds four deposits of every
    pixel): fp64 route against the oracle's get_interpol
    regrid to 1e-10, fp32 route to the accuracy of fp32 weights; every pixel stored, mass conserved."""
    import torch
    from baryonification_amd import engine, synthetic as syn
    from oracle import oracle as O
    npix = 12 * nside * nside
    off = _random_offsets(nside, scale, seed=nside + int(scale * 10))
    hmap = syn.make_map(nside)
    hmap[::17] = 0.0                                                            # empty pixels are skipped (HealpixRunner.py:335)
    ora = O.regrid(nside, hmap, off)
    cat = syn.make_catalog(1000)
    z, M, r = syn.table_grid(cat)
    model, keep = engine.model_from_tables([np.log(1 + z), np.log(M), np.log(r)], syn.displacement_table(z, M, r), syn.COSMO, 10.0, 10.0)
    dev = torch.device('cuda:0')
    if scale == 60:
        monkeypatch.setenv('BFGX_FAR_CAP', '1000000')
    if scale > 60:                  # (a table that moves pixels this far gives its plan such a list; this plan's table moves nothing)
        monkeypatch.setenv('BFGX_FAR_CAP', str(4 * npix))
    plan = engine.ShellPlan(model, keep, nside, 1000, device=0, stream=torch.cuda.current_stream().cuda_stream)
    d_map = torch.from_numpy(hmap).to(dev)
    for f64, tol in ((True, 1e-10), (False, 3e-5 * max(1.0, scale))):
        d_off = torch.from_numpy(off if f64 else off.astype(np.float32)).to(dev).reshape(-1)
        out = torch.full((npix,), np.nan, dtype=torch.float64, device=dev)
        sums = torch.zeros(2, dtype=torch.float64, device=dev)
        plan.regrid(d_map.data_ptr(), d_off.data_ptr(), out.data_ptr(), sums.data_ptr(), acc_f64=f64)
        torch.cuda.synchronize()
        plan.status()
        got = out.cpu().numpy()
        assert np.isfinite(got).all()
        assert abs(sums[0].item() - hmap.sum()) <= 1e-9 * hmap.sum() and abs(sums[1].item() - sums[0].item()) <= 1e-9 * hmap.sum()
        assert abs(got.sum() - hmap.sum()) <= 1e-9 * hmap.sum()
        assert np.abs(got - ora).max() <= tol * np.abs(ora).max(), (f64, np.abs(got - ora).max() / np.abs(ora).max())
        if scale == 60:
            assert plan.regrid_stats()['far_overflowed']                          # (the repair pass was what ran)
        if scale > 60:
            assert not plan.regrid_stats()['far_overflowed']                      # (200 pixels: the plan's own list holds every deposit)
    plan.close()


def test_fused_baryonify_equals_offsets_then_regrid(gpu):
    """bfgx_baryonify_device (K1 leaves the largest displacement per tile for K2's aprons) == offsets + regrid (K2 finds it
    with its own pass), for a table whose displacements reach many pixels (aprons of several rings, far list in use)"""
    N, nside = 200_000, 512
    torch, _lib, syn, cat, axes, table, plan, dev = _setup(N, nside, paint=False)
    from baryonification_amd import engine
    npix = 12 * nside * nside
    hmap = torch.from_numpy(syn.make_map(nside)).to(dev)
    for scale in (1.0, 300.0):                       # closed-form table: a few percent of a pixel; x 300: up to ~10 pixels
        model, keep = engine.model_from_tables(axes, table * scale, syn.COSMO, 10.0, 10.0)
        pl = engine.ShellPlan(model, keep, nside, N, 0, torch.cuda.current_stream().cuda_stream)
        cd, cols = _cat_dev(torch, _lib, dev, cat)
        for f64 in (False, True):
            dt = torch.float64 if f64 else torch.float32
            off_a, off_b = torch.zeros(npix * 3, dtype=dt, device=dev), torch.zeros(npix * 3, dtype=dt, device=dev)
            out_a, out_b = torch.full((npix,), np.nan, dtype=torch.float64, device=dev), torch.full((npix,), np.nan, dtype=torch.float64, device=dev)
            s_a, s_b = torch.zeros(2, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.float64, device=dev)
            pl.offsets(cd, off_a.data_ptr(), acc_f64=f64)
            pl.regrid(hmap.data_ptr(), off_a.data_ptr(), out_a.data_ptr(), s_a.data_ptr(), acc_f64=f64)
            pl.baryonify(cd, hmap.data_ptr(), off_b.data_ptr(), out_b.data_ptr(), s_b.data_ptr(), acc_f64=f64)
            torch.cuda.synchronize()
            pl.status()
            # (K1 adds in LDS with atomics: the order, hence the last bits, differ from run to run)
            assert (off_a - off_b).abs().max().item() <= (1e-12 if f64 else 2e-6) * off_a.abs().max().item()
            pix = np.sqrt(4 * np.pi / npix)
            reach = off_a.view(-1, 3).double().norm(dim=1).max().item() / pix
            assert (reach < 0.2) if scale == 1.0 else (2.0 < reach < 40.0), reach
            assert torch.isfinite(out_b).all().item() and np.isclose(s_b[1].item(), s_b[0].item(), rtol=(1e-12 if f64 else 1e-6))
            # the aprons may differ (K1's bound on |offset| from the largest stored component is looser than K2's own pass): same deposits, other order
            assert (out_a - out_b).abs().max().item() <= (1e-10 if f64 else 1e-5) * max(1.0, reach) * out_a.abs().max().item()
        pl.close()
    plan.close()


@pytest.mark.parametrize('scale', [0.5, 3.0, 12.0])
def test_banded_regrid_with_reach(gpu, scale):
    """the banded regrid with the apron every rank derives from the largest summed |offset| (reach_rings / set_band_reach):
    slices + listed far deposits == the full-map regrid == the oracle"""
    import torch
    from baryonification_amd import engine, synthetic as syn
    from baryonification_amd.utils.Parallelize import band_partition
    from oracle import oracle as O
    nside = 256
    npix = 12 * nside * nside
    off = _random_offsets(nside, scale, seed=7).astype(np.float32)
    hmap = syn.make_map(nside)
    ora = O.regrid(nside, hmap, off.astype(np.float64))
    cat = syn.make_catalog(1000)
    z, M, r = syn.table_grid(cat)
    model, keep = engine.model_from_tables([np.log(1 + z), np.log(M), np.log(r)], syn.displacement_table(z, M, r), syn.COSMO, 10.0, 10.0)
    dev = torch.device('cuda:0')
    plan = engine.ShellPlan(model, keep, nside, 1000, device=0, stream=torch.cuda.current_stream().cuda_stream)
    d_map, d_off = torch.from_numpy(hmap).to(dev), torch.from_numpy(off).to(dev).reshape(-1)
    rings = plan.reach_rings(float(np.linalg.norm(off, axis=1).max()))
    assert 1 <= rings <= 16 and (rings == 1) == (scale < 0.6)
    plan.set_band_reach(rings)
    first = plan.bands()
    world = 3
    cuts = band_partition(first, world)
    pb = first[cuts]
    acc = torch.full((npix,), np.nan, dtype=torch.float64, device=dev)
    far_p, far_v = [], []
    for rk in range(world):
        p0, p1 = int(pb[rk]), int(pb[rk + 1])
        olo, ohi = plan.band_apron(int(cuts[rk]), int(cuts[rk + 1]))
        my_off = d_off[3 * olo:3 * ohi].clone()
        plan.regrid_bands(int(cuts[rk]), int(cuts[rk + 1]), d_map.data_ptr(), my_off.data_ptr(), olo, ohi, acc[p0:p1].data_ptr())
        fp, fv = plan.far_fetch()
        far_p.append(fp); far_v.append(fv)
    fp, fv = np.concatenate(far_p), np.concatenate(far_v)
    if fp.size:
        acc.index_add_(0, torch.from_numpy(fp).to(dev), torch.from_numpy(fv).to(dev))
    plan.status()
    got = acc.cpu().numpy()
    assert np.isfinite(got).all() and abs(got.sum() - hmap.sum()) <= 1e-9 * hmap.sum()
    assert np.abs(got - ora).max() <= 3e-5 * max(1.0, scale) * np.abs(ora).max()
    plan.close()


def test_config2_exact_bench_table_edges(gpu):
    """The headline configuration exactly as bench.py builds it: table edges == catalog min/max (README.md:78-80, pad = 0).
    Whether the four edge halos (min/max z, min/max M) are inside the table hangs on the last bit of np.log(1/a) and
    np.log(M); with the caller's numpy coordinates travelling through the ABI the product classifies them as the oracle
    (= the reference's arithmetic) does.  pix_offsets of the edge halos + 20 000 others against the oracle, and the full
    1e6-halo catalog through properties (mass conservation; equality with the padded table away from the edge halos)."""
    N, nside = 1_000_000, 1024
    torch, _lib, syn, cat, axes, table, plan, dev = _setup(N, nside, paint=False, pad=0.0)
    npix = 12 * nside * nside
    edge = np.array([cat['z'].argmin(), cat['z'].argmax(), cat['M'].argmin(), cat['M'].argmax()])
    idx = np.unique(np.concatenate([edge, np.arange(20000)]))
    sub = {k: v[idx] for k, v in cat.items()}
    from oracle import oracle as O
    tab = O.Table(axes, table, False, 10.0)
    bg = O.Background.from_dict(syn.COSMO)
    ora = O.baryonify_offsets(nside, sub, tab, 10.0, bg)
    # the oracle itself must see both kinds: edge halos that read the table and (possibly) edge halos that read NaN
    lnz, lnM = O.table_coords(sub)
    inside = (lnz >= axes[0][0]) & (lnz <= axes[0][-1]) & (lnM >= axes[1][0]) & (lnM <= axes[1][-1])
    assert inside.sum() >= idx.size - 4
    cd, keep = _cat_dev(torch, _lib, dev, cat, idx, coords=True)
    for acc_f64, tol in ((True, 1e-12), (False, 2e-9)):          # absolute: offsets are ~1e-5; fp32 storage of ~1e-5 numbers
        off = torch.zeros(npix * 3, dtype=torch.float64 if acc_f64 else torch.float32, device=dev)
        plan.offsets(cd, off.data_ptr(), acc_f64)
        torch.cuda.synchronize()
        got = off.cpu().numpy().astype(np.float64).reshape(npix, 3)
        assert np.abs(got - ora).max() <= tol
        # each edge halo alone: contributes exactly when the oracle says it is inside the table
        for e in edge:
            one = {k: v[e:e + 1] for k, v in cat.items()}
            o1 = O.baryonify_offsets(nside, one, tab, 10.0, bg)
            c1, k1 = _cat_dev(torch, _lib, dev, cat, np.array([e]), coords=True)
            off.zero_()
            plan.offsets(c1, off.data_ptr(), acc_f64)
            torch.cuda.synchronize()
            g1 = off.cpu().numpy().astype(np.float64).reshape(npix, 3)
            assert (np.abs(g1).max() > 0) == (np.abs(o1).max() > 0)
            assert np.abs(g1 - o1).max() <= tol
    plan.status()
    # full catalog on the bench's table: mass conservation through the default (fp32) path
    cdf, keepf = _cat_dev(torch, _lib, dev, cat, coords=True)
    hmap = syn.make_map(nside)
    d_map = torch.from_numpy(hmap).to(dev)
    off = torch.zeros(npix * 3, dtype=torch.float32, device=dev)
    out = torch.zeros(npix, dtype=torch.float64, device=dev)
    sums = torch.zeros(2, dtype=torch.float64, device=dev)
    plan.offsets(cdf, off.data_ptr(), False)
    plan.regrid(d_map.data_ptr(), off.data_ptr(), out.data_ptr(), sums.data_ptr(), False)
    torch.cuda.synchronize()
    s_ = sums.cpu().numpy()
    assert np.isclose(s_[1], s_[0]) and np.isclose(out.sum().item(), hmap.sum())
    plan.status()
    plan.close()


def test_config4_share_nside2048(gpu):
    """BASELINE config 4's per-GPU share (1e7 halos over 8 GPUs = 1.25e6 halos, NSIDE 2048, BaryonifyShell): pix_offsets
    of a 20 000-halo sample against the oracle, and the full share through properties (mass conservation, linearity of
    pix_offsets over a catalog split = what the multi-GPU sum relies on, census of the tile path == per-halo path)."""
    N, nside = 1_250_000, 2048
    torch, _lib, syn, cat, axes, table, plan, dev = _setup(N, nside, paint=False)
    npix = 12 * nside * nside
    from oracle import oracle as O
    tab = O.Table(axes, table, False, 10.0)
    bg = O.Background.from_dict(syn.COSMO)
    sub = {k: v[:20000] for k, v in cat.items()}
    ora = O.baryonify_offsets(nside, sub, tab, 10.0, bg)
    cdS, kS = _cat_dev(torch, _lib, dev, cat, np.arange(20000), coords=True)
    off64 = torch.zeros(npix * 3, dtype=torch.float64, device=dev)
    plan.offsets(cdS, off64.data_ptr(), True)
    torch.cuda.synchronize()
    assert np.abs(off64.cpu().numpy().reshape(npix, 3) - ora).max() <= 1e-12
    off32 = torch.zeros(npix * 3, dtype=torch.float32, device=dev)
    plan.offsets(cdS, off32.data_ptr(), False)
    torch.cuda.synchronize()
    assert np.abs(off32.cpu().numpy().astype(np.float64).reshape(npix, 3) - ora).max() <= 2e-9
    del ora
    # the full share
    cd, keep = _cat_dev(torch, _lib, dev, cat, coords=True)
    plan.offsets(cd, off64.data_ptr(), True)
    plan.status()
    idx = np.random.default_rng(7).permutation(N)
    cdA, kA = _cat_dev(torch, _lib, dev, cat, idx[: N // 2], coords=True)
    cdB, kB = _cat_dev(torch, _lib, dev, cat, idx[N // 2:], coords=True)
    lin = torch.zeros_like(off64)
    tmp = torch.zeros_like(off64)
    plan.offsets(cdA, lin.data_ptr(), True)
    plan.offsets(cdB, tmp.data_ptr(), True)
    lin += tmp
    torch.cuda.synchronize()
    assert (lin - off64).abs().max().item() <= 2e-14
    del lin, tmp
    hmap = syn.make_map(nside)
    d_map = torch.from_numpy(hmap).to(dev)
    out = torch.zeros(npix, dtype=torch.float64, device=dev)
    sums = torch.zeros(2, dtype=torch.float64, device=dev)
    plan.offsets(cd, off32.data_ptr(), False)
    plan.regrid(d_map.data_ptr(), off32.data_ptr(), out.data_ptr(), sums.data_ptr(), False)
    torch.cuda.synchronize()
    s_ = sums.cpu().numpy()
    assert np.isclose(s_[1], s_[0]) and np.isclose(out.sum().item(), hmap.sum())      # HealpixRunner.py:344-346
    plan.set_algo(1); n1 = plan.count_pairs(cd, True)
    plan.set_algo(0); n0 = plan.count_pairs(cd, True)
    assert n0 == n1 > 2e8
    plan.status()
    plan.close()


@pytest.mark.parametrize('paint', [False, True])
def test_band_restricted_pass_with_selected_halos_equals_full_pass(gpu, paint):
    """spatially sharded multi-GPU building block on one GPU: every "rank" takes the halos whose ring range (disc_rings) can touch
    its run of bands and runs K0 + K1 (K3) for its tiles only; its slice must be the full-sky result on those pixels -- i.e. the
    ring ranges miss no halo (polar caps, discs across band boundaries, 4-pixel fallbacks) and the kernels clip to the tile range"""
    from baryonification_amd.utils.Parallelize import band_partition, band_ring_bounds
    N, nside = 150_000, 512
    torch, _lib, syn, cat, axes, table, plan, dev = _setup(N, nside, paint=paint)
    cat = {k: v.copy() for k, v in cat.items()}
    cat['dec'][:8] = [89.95, -89.9, 89.999, -89.7, 60.0, -60.0, 0.01, -0.01]
    cat['M'][:4] *= 30.0                                                    # big discs on the pole caps
    npix = 12 * nside * nside
    width, dt = (1, torch.float64) if paint else (3, torch.float32)
    cd, cols = _cat_dev(torch, _lib, dev, cat, coords=True)
    full = torch.zeros(npix * width, dtype=dt, device=dev)
    (plan.paint if paint else plan.offsets)(cd, full.data_ptr(), acc_f64=paint)
    rings = torch.empty((N, 2), dtype=torch.int32, device=dev)
    plan.disc_rings(cd, rings.data_ptr())
    torch.cuda.synchronize()
    assert int((rings[:, 0] <= rings[:, 1]).sum().item()) == N and int(rings.min().item()) >= 1 and int(rings.max().item()) <= 4 * nside - 1
    first = plan.bands()
    BR = plan.tile_shape()[0]
    for world in (3, 8):
        cuts = band_partition(first, world)
        rb = band_ring_bounds(cuts, BR, nside)
        assert rb[0] == 1 and rb[-1] == 4 * nside
        taken = 0
        for rk in range(world):
            sel = ((rings[:, 0].long() < int(rb[rk + 1])) & (rings[:, 1].long() >= int(rb[rk]))).cpu().numpy()
            taken += int(sel.sum())
            cdr, colsr = _cat_dev(torch, _lib, dev, cat, idx=np.nonzero(sel)[0], coords=True)
            p0, p1 = int(first[cuts[rk]]), int(first[cuts[rk + 1]])
            sl = torch.full(((p1 - p0) * width,), float('nan'), dtype=dt, device=dev)           # every element must be stored
            (plan.paint_bands if paint else plan.offsets_bands)(cdr, int(cuts[rk]), int(cuts[rk + 1]), sl.data_ptr(), acc_f64=paint)
            torch.cuda.synchronize()
            plan.status()
            ref = full[p0 * width:p1 * width]
            assert torch.isfinite(sl).all().item()
            assert (sl - ref).abs().max().item() <= (1e-12 if paint else 2e-6) * full.abs().max().item()
            if not paint:
                # the reach of the regrid: the per-tile maxima K1 left behind == a pass over the slice (up to K1's 1e-6 safety factor)
                m_k1, m_pass = torch.empty(1, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.float32, device=dev)
                plan.bands_max_offset2(int(cuts[rk]), int(cuts[rk + 1]), m_k1.data_ptr())
                plan.max_offset2(sl.data_ptr(), p1 - p0, m_pass.data_ptr(), acc_f64=False)
                torch.cuda.synchronize()
                a, b = float(m_k1.item()), float(m_pass.item())
                assert b > 0 and b <= a <= b * (1 + 3e-6), (a, b)
                with pytest.raises(ValueError):                             # not a BFGX_ACC_* value: refused, not read as fp32
                    plan.max_offset2(sl.data_ptr(), p1 - p0, m_pass.data_ptr(), acc_f64=2)
        assert N <= taken <= 1.5 * N                                        # boundary halos go to two ranks, nothing is lost
    plan.close()


def test_route_kernels_pack_every_halo_for_every_rank_it_touches(gpu):
    """bfgx_route_count_device / bfgx_route_fill_device (spatial sharding of scattered halos): per destination rank the packed rows
    are exactly the halos whose ring range touches that rank's rings -- incl. halos that go to several ranks and to none"""
    import torch
    from baryonification_amd import engine, synthetic as syn
    dev = torch.device('cuda:0')
    n, world, nside = 300_000, 5, 512
    rng = np.random.default_rng(3)
    first = rng.integers(1, 4 * nside, n)
    last = np.minimum(first + rng.integers(0, 40, n), 4 * nside - 1)
    last[:50] = 4 * nside - 1; first[:50] = 1                              # discs over the whole sky: every rank
    first[50:80] = 100; last[50:80] = 99                                    # touch nothing
    bounds = np.array([1, 300, 700, 1024, 1500, 4 * nside], dtype=np.int64)
    cols = [torch.from_numpy(rng.normal(size=n)).to(dev) for _ in range(6)]
    cols[0] = torch.arange(n, dtype=torch.float64, device=dev)             # column 0 = halo number: identifies the row
    rings = torch.from_numpy(np.stack([first, last], axis=1).astype(np.int32)).to(dev)
    cat = syn.make_catalog(1000)
    z, M, r = syn.table_grid(cat)
    model, keep = engine.model_from_tables([np.log(1 + z), np.log(M), np.log(r)], syn.displacement_table(z, M, r), syn.COSMO, 10.0, 10.0)
    plan = engine.ShellPlan(model, keep, nside, 1000, device=0, stream=torch.cuda.current_stream().cuda_stream)
    counts = torch.empty(world, dtype=torch.int32, device=dev)
    plan.route_count(n, rings.data_ptr(), bounds, counts.data_ptr())
    c = counts.cpu().numpy().astype(np.int64)
    want = [np.nonzero((first < bounds[j + 1]) & (last >= bounds[j]) & (first <= last))[0] for j in range(world)]
    assert np.array_equal(c, [w.size for w in want]) and c.sum() > n
    start = np.concatenate([[0], np.cumsum(c)[:-1]])
    rows = torch.full((int(c.sum()), 6), float('nan'), dtype=torch.float64, device=dev)
    cursor = torch.empty(world, dtype=torch.int32, device=dev)
    plan.route_fill(n, rings.data_ptr(), bounds, start, [x.data_ptr() for x in cols], cursor.data_ptr(), rows.data_ptr())
    got = rows.cpu().numpy()
    host = np.stack([x.cpu().numpy() for x in cols], axis=1)
    assert np.isfinite(got).all()
    for j in range(world):
        blk = got[start[j]:start[j] + c[j]]
        ids = blk[:, 0].astype(np.int64)
        assert np.array_equal(np.sort(ids), want[j])                       # the right halos, each once
        assert np.array_equal(blk, host[ids])                               # whole rows travel together
    # bfgx_route_pack_device: the same in one pass into fixed-capacity blocks [world][6][cap] (nothing read back inside a step); the rows a
    # destination does not receive keep M = NaN; a block that is too small raises the overflow flag and drops the excess
    for capb, over in ((int(c.max()) + 7, 0), (int(c.max()) - 1, 1)):
        blocks = torch.full((world, 6, capb), -7.0, dtype=torch.float64, device=dev)
        ovf = torch.zeros(1, dtype=torch.int32, device=dev)
        plan.route_pack(n, rings.data_ptr(), bounds, capb, [x.data_ptr() for x in cols], cursor.data_ptr(), blocks.data_ptr(), ovf.data_ptr())
        b = blocks.cpu().numpy()
        assert int(ovf.item()) == over
        for j in range(world):
            valid = ~np.isnan(b[j, 0])
            m = int(valid.sum())
            assert m == min(int(c[j]), capb) and valid[:m].all()            # the received rows are packed at the front of the block
            ids = b[j, 0, :m].astype(np.int64)
            assert np.unique(ids).size == m and np.isin(ids, want[j]).all() and (over or np.array_equal(np.sort(ids), want[j]))
            assert np.array_equal(b[j, :, :m].T, host[ids])
    plan.close()


@pytest.mark.parametrize('nh', [0, 3, 60])
def test_sparse_catalog_still_tiles_are_copied(gpu, nh):
    """a catalog that leaves most of the sphere alone: tiles without an offset in or within reach of them are copied by K2
    (positive pixels only, as the reference regrids them: HealpixRunner.py:335), the others regridded -- fused call and separate
    regrid both == the oracle's regrid of the same pix_offsets"""
    from oracle import oracle as O
    N, nside = 4000, 256
    torch, _lib, syn, cat, axes, table, plan, dev = _setup(N, nside, paint=False)
    npix = 12 * nside * nside
    hmap = syn.make_map(nside)
    rng = np.random.default_rng(nh)
    hmap[rng.integers(0, npix, 500)] = 0.0                                   # empty and negative pixels deposit nothing
    hmap[rng.integers(0, npix, 500)] = -1.5
    d_map = torch.from_numpy(hmap).to(dev)
    cd, cols = _cat_dev(torch, _lib, dev, cat, idx=np.arange(nh))
    off = torch.full((npix * 3,), float('nan'), dtype=torch.float64, device=dev)
    out_f, out_s = torch.full((npix,), float('nan'), dtype=torch.float64, device=dev), torch.full((npix,), float('nan'), dtype=torch.float64, device=dev)
    s_f, s_s = torch.zeros(2, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.float64, device=dev)
    plan.baryonify(cd, d_map.data_ptr(), off.data_ptr(), out_f.data_ptr(), s_f.data_ptr(), acc_f64=True)
    plan.regrid(d_map.data_ptr(), off.data_ptr(), out_s.data_ptr(), s_s.data_ptr(), acc_f64=True)
    torch.cuda.synchronize()
    plan.status()
    o = off.cpu().numpy().reshape(npix, 3)
    assert np.isfinite(o).all()
    moved = int((np.abs(o).sum(axis=1) > 0).sum())
    assert (moved == 0) if nh == 0 else (0 < moved < npix // 4)               # most of the sphere is still
    ora = O.regrid(nside, hmap, o)
    for got, sums in ((out_f, s_f), (out_s, s_s)):
        g = got.cpu().numpy()
        assert np.isfinite(g).all() and np.abs(g - ora).max() <= 1e-10 * np.abs(ora).max()
        assert np.isclose(sums[0].item(), hmap.sum(), rtol=1e-12) and np.isclose(sums[1].item(), hmap[hmap > 0].sum(), rtol=1e-12)
    plan.close()


def test_rank_without_bands_is_a_no_op(gpu):
    """more ranks than ring bands (small NSIDE): band_partition gives a rank the empty range [b, b); its buffers are empty tensors whose
    data pointers are NULL -- the band-restricted passes and the banded regrid return without touching anything"""
    torch, _lib, syn, cat, axes, table, plan, dev = _setup(500, 16, paint=False)
    from baryonification_amd.utils.Parallelize import band_partition
    first = plan.bands()
    cuts = band_partition(first, 16)                         # NSIDE 16: 2 bands of 32 rings for 16 ranks
    assert len(set(cuts.tolist())) < 17
    cd, keepc = _cat_dev(torch, _lib, dev, cat)
    empty = torch.empty(0, dtype=torch.float32, device=dev)
    assert empty.data_ptr() == 0
    sums = torch.full((2,), 7.0, dtype=torch.float64, device=dev)
    for b in sorted(set(int(c) for c in cuts)):
        plan.offsets_bands(cd, b, b, empty.data_ptr(), acc_f64=False)
        lo, hi = plan.band_apron(b, b)
        plan.regrid_bands(b, b, 0, 0, lo, hi, 0, sums.data_ptr(), acc_f64=False)
        torch.cuda.synchronize()
        assert sums.tolist() == [0.0, 0.0]
        sums.fill_(7.0)
    plan.close()


def test_config4_full_size_eight_rank_decomposition_on_one_gpu(gpu):
    """BASELINE config 4 (1e7 halos, BaryonifyShell, NSIDE 2048, 8 GPUs) at FULL size on one GPU, the eight ranks of the spatial sharding
    played one after the other: every rank takes the halos whose discs can touch its ring bands (disc_rings), computes pix_offsets for
    ITS pixels (K0 + K1 on its tiles) and regrids its bands from its slice + the apron rings of its neighbours.  The eight slices ==
    the single-GPU pass (pix_offsets to fp32 rounding, the map to the stated fp32 tolerance), the pair counts add up, the mass is conserved --
    i.e. what the first real 8-GPU run will compute, minus the transport"""
    from baryonification_amd.utils.Parallelize import band_partition, band_ring_bounds
    N, nside, world = 10_000_000, 2048, 8
    torch, _lib, syn, cat, axes, table, plan, dev = _setup(N, nside, paint=False)
    npix = 12 * nside * nside
    hmap = syn.make_map(nside)
    d_map = torch.from_numpy(hmap).to(dev)
    cd, cols = _cat_dev(torch, _lib, dev, cat, coords=True)
    full_off = torch.empty(npix * 3, dtype=torch.float32, device=dev)
    full_out = torch.empty(npix, dtype=torch.float64, device=dev)
    sums = torch.zeros(2, dtype=torch.float64, device=dev)
    plan.baryonify(cd, d_map.data_ptr(), full_off.data_ptr(), full_out.data_ptr(), sums.data_ptr(), acc_f64=False)
    torch.cuda.synchronize()
    plan.status()
    s = sums.cpu().numpy()
    assert np.isclose(s[1], s[0]) and np.isclose(float(full_out.sum().item()), hmap.sum())       # HealpixRunner.py:344-346
    n_full = plan.count_pairs(cd, True)
    assert n_full > 2e9
    rings = torch.empty((N, 2), dtype=torch.int32, device=dev)
    plan.disc_rings(cd, rings.data_ptr())
    first = plan.bands()
    cuts = band_partition(first, world)
    rb = band_ring_bounds(cuts, plan.tile_shape()[0], nside)
    m2 = torch.empty(1, dtype=torch.float32, device=dev)
    plan.max_offset2(full_off.data_ptr(), npix, m2.data_ptr(), acc_f64=False)
    plan.set_band_reach(plan.reach_rings(float(m2.item()) ** 0.5))
    off_scale, map_scale = float(full_off.abs().max().item()), float(full_out.abs().max().item())
    taken, s_in, s_out, n_far = 0, 0.0, 0.0, 0
    new = torch.full((npix,), float('nan'), dtype=torch.float64, device=dev)
    far_acc = torch.zeros(npix, dtype=torch.float64, device=dev)              # far deposits (pole caps) may land in any rank's slice
    for rk in range(world):
        sel = torch.nonzero((rings[:, 0].long() < int(rb[rk + 1])) & (rings[:, 1].long() >= int(rb[rk]))).reshape(-1)
        taken += int(sel.numel())
        t = {k: v[sel].contiguous() for k, v in cols.items()}
        cdr = _lib.make_catalog_dev(int(sel.numel()), t['M'].data_ptr(), t['z'].data_ptr(), t['ra'].data_ptr(), t['dec'].data_ptr(),
                                    ln1pz_ptr=t['lnz'].data_ptr(), lnM_ptr=t['lnM'].data_ptr())
        b0, b1 = int(cuts[rk]), int(cuts[rk + 1])
        p0, p1 = int(first[b0]), int(first[b1])
        lo, hi = plan.band_apron(b0, b1)
        buf = torch.full(((hi - lo) * 3,), float('nan'), dtype=torch.float32, device=dev)
        plan.offsets_bands(cdr, b0, b1, buf[(p0 - lo) * 3:].data_ptr(), acc_f64=False)
        torch.cuda.synchronize()
        plan.status()
        mine = buf[(p0 - lo) * 3:(p1 - lo) * 3]
        assert torch.isfinite(mine).all().item() and (mine - full_off[p0 * 3:p1 * 3]).abs().max().item() <= 2e-6 * off_scale
        # the apron rings come from the neighbours' slices: here from the single-GPU pass, which the neighbours' slices equal
        buf[:(p0 - lo) * 3] = full_off[lo * 3:p0 * 3]
        buf[(p1 - lo) * 3:] = full_off[p1 * 3:hi * 3]
        rs = torch.zeros(2, dtype=torch.float64, device=dev)
        plan.regrid_bands(b0, b1, d_map.data_ptr(), buf.data_ptr(), lo, hi, new[p0:].data_ptr(), rs.data_ptr(), acc_f64=False)
        fp, fv = plan.far_fetch()
        n_far += len(fp)
        if len(fp):
            far_acc.index_add_(0, torch.from_numpy(fp).to(dev), torch.from_numpy(fv).to(dev))
        r2 = rs.cpu().numpy()
        s_in += r2[0]; s_out += r2[1]
        del buf, t
    torch.cuda.synchronize()
    assert N <= taken <= 1.3 * N
    assert np.isclose(s_out, s_in) and np.isclose(s_in, hmap.sum())
    assert torch.isfinite(new).all().item()                                   # every pixel of every slice was stored
    new += far_acc
    # (a slice's fp32 pix_offsets can differ from the single pass in the last bit -- the order of the LDS additions --, which moves a
    # pixel's value by up to ~1e-7 of it: the stated fp32 tolerance, 1e-6 mean(map), applies; most pixels agree exactly)
    diff = (new - full_out).abs()
    assert diff.max().item() <= 1e-6 * hmap.mean() and (diff > 1e-12 * map_scale).float().mean().item() < 0.05 and n_far < npix // 100
    plan.close()


@pytest.mark.parametrize('cap', ['3', '40'])
def test_tile_lists_overflow_into_the_shared_list(gpu, monkeypatch, cap):
    """K0 places a narrow halo directly into its tiles' fixed-capacity lists; what does not fit (here: lists of 3 / 40 entries for ~160
    halos per tile) goes through the per-workgroup slow lists, the scan and the placement pass into region B of the shared list: same
    pix_offsets, same pair census, same map"""
    N, nside = 150_000, 256
    torch, _lib, syn, cat, axes, table, plan, dev = _setup(N, nside, paint=False)
    npix = 12 * nside * nside
    cd, keep1 = _cat_dev(torch, _lib, dev, cat)

    def run(pl):
        off = torch.zeros(npix * 3, dtype=torch.float64, device=dev)
        pl.set_algo(1)
        pl.offsets(cd, off.data_ptr(), True)
        torch.cuda.synchronize()
        pl.status()
        return off, pl.count_pairs(cd, True)

    ref, n_ref = run(plan)
    monkeypatch.setenv('BFGX_TILE_LIST_CAP', cap)
    from baryonification_amd import engine
    model, keep = engine.model_from_tables(axes, table, syn.COSMO, 10.0, 10.0)
    small = engine.ShellPlan(model, keep, nside, N, 0, torch.cuda.current_stream().cuda_stream)
    got, n_got = run(small)
    assert n_got == n_ref > 5e5 and (got - ref).abs().max().item() <= 2e-14
    hmap = syn.make_map(nside)
    d_map = torch.from_numpy(hmap).to(dev)
    out = torch.zeros(npix, dtype=torch.float64, device=dev)
    sums = torch.zeros(2, dtype=torch.float64, device=dev)
    f_off = torch.zeros(npix * 3, dtype=torch.float32, device=dev)
    small.baryonify(cd, d_map.data_ptr(), f_off.data_ptr(), out.data_ptr(), sums.data_ptr(), acc_f64=False)
    torch.cuda.synchronize()
    small.status()
    s = sums.cpu().numpy()
    assert np.isclose(s[1], s[0]) and np.isclose(out.sum().item(), hmap.sum())
    small.close(); plan.close()


@pytest.mark.parametrize('f64', [False, True])
@pytest.mark.parametrize('paint', [False, True])
def test_k1_fluid_form_equals_barrier_form(gpu, monkeypatch, paint, f64):
    """the fast kernel's two forms -- one 1024-thread workgroup per CU with two tile slots and no barrier between tiles (default from 1024
    tiles; BFGX_K1_FLUID=2 at plan creation: always), and two 512-thread workgroups per CU with a barrier per tile (=0) -- run the same chunk code in a
    different order (fp64 pair math: twelve waves per workgroup): the same pair census, outputs equal to the last bits of the fp64 LDS sums, whole sphere and band-restricted passes
    (few tiles per launch: slots without a tile, both draw orders at the end of the sequence), halos on the poles and across phi = 0"""
    N, nside = 400_000, 512
    monkeypatch.setenv('BFGX_K1_FLUID', '2')
    torch, _lib, syn, cat, axes, table, plan, dev = _setup(N, nside, paint=paint)
    cat['dec'][:4] = [90.0 - 1e-7, -90.0 + 1e-7, 89.9, 0.0]
    cat['ra'][:4] = [0.0, 77.0, 359.9999, 1e-9]
    npix = 12 * nside * nside
    cd, keep1 = _cat_dev(torch, _lib, dev, cat)
    from baryonification_amd import engine
    monkeypatch.setenv('BFGX_K1_FLUID', '0')
    model, keep = engine.model_from_tables(axes, np.log(table) if paint else table, syn.COSMO, 10.0, 10.0, log_values=paint)
    barrier = engine.ShellPlan(model, keep, nside, N, 0, torch.cuda.current_stream().cuda_stream)
    monkeypatch.delenv('BFGX_K1_FLUID')

    def full(pl):
        out = torch.zeros(npix * (1 if paint else 3), dtype=torch.float64 if (paint or f64) else torch.float32, device=dev)
        if paint:
            pl.paint(cd, out.data_ptr(), acc_f64=(1 if f64 else 2))    # 2: fp32 pair math into the fp64 map
        else:
            pl.offsets(cd, out.data_ptr(), f64)
        torch.cuda.synchronize()
        pl.status()
        return out

    a, b = full(plan), full(barrier)
    scale = a.abs().max().item()
    tol = 1e-13 if (paint or f64) else 2e-7
    assert scale > 0 and (a - b).abs().max().item() <= tol * scale
    assert plan.count_pairs(cd, not paint) == barrier.count_pairs(cd, not paint) > 4e6
    # band-restricted passes: 1, 2, 3 and 7 bands of 32 rings (a handful of tiles up to a few hundred per launch)
    bounds = plan.bands()
    nb = len(bounds) - 1
    comp = 1 if paint else 3
    for b0, b1 in ((0, 1), (nb // 2, nb // 2 + 2), (nb - 3, nb), (5, 12)):
        p0, p1 = int(bounds[b0]), int(bounds[b1])
        got = []
        for pl in (plan, barrier):
            sl = torch.full(((p1 - p0) * comp,), 7.0, dtype=a.dtype, device=dev)
            if paint:
                pl.paint_bands(cd, b0, b1, sl.data_ptr(), acc_f64=(1 if f64 else 2))
            else:
                pl.offsets_bands(cd, b0, b1, sl.data_ptr(), f64)
            torch.cuda.synchronize()
            pl.status()
            got.append(sl)
        assert (got[0] - got[1]).abs().max().item() <= tol * scale
    plan.close(); barrier.close()


def _twin_tables(axes, values):
    """the same interpolant on a NON-uniform ln r axis: one knot more, at the midpoint of an interior interval, whose values are the mean of
    the two neighbouring nodes (of the array model_from_tables gets: ln(table) for painting).  Linear interpolation is unchanged, but the
    plan cannot take the fast kernel: the generic tile kernel takes every halo, in fp64."""
    lr = axes[2]
    k = len(lr) // 2
    lr_t = np.insert(lr, k + 1, 0.5 * (lr[k] + lr[k + 1]))
    return [axes[0], axes[1], lr_t], np.insert(values, k + 1, 0.5 * (values[..., k] + values[..., k + 1]), axis=-1)


@pytest.mark.parametrize('f64', [False, True])
@pytest.mark.parametrize('paint', [False, True])
def test_wide_discs_in_the_fast_kernel_equal_the_wide_pass(gpu, monkeypatch, paint, f64):
    """wide discs -- a pole inside, pixels further than 0.40 rad from the halo's azimuth, the 4 fallback pixels on the first rings -- go
    through the fast kernel's chunk (general row spans, full-range sin / cos) and must equal what the generic tile kernel, whose row and
    pair code for such discs is the older one, gives for the same interpolant on a TWIN plan (_twin_tables: fp64 throughout).  Same pair
    census; outputs equal to fp32 / fp64 rounding of the different pair arithmetic.  The catalog holds halos on and around both poles,
    discs of 0.3 - 2.5 rad (z = 0.0003 .. 0.003: thousands of tiles each), a disc over the whole sphere and tiny discs on the first rings,
    among 2e5 ordinary ones; both forms of the fast kernel.

    (The name is from when the comparison was the generic kernel's WIDE PASS, which revisited the tiles with wide entries after the fast
    kernel; that pass is gone, its row and pair code is what the twin plan runs.)

    fp32 bounds, from max |difference| / scale measured on the last commit that had the wide pass (default route, wide-pass route and twin
    side by side, two runs each, the same to three digits):
                                         displacement (fp32)   painting (fp32 pairs, fp64 map)
      wide discs alone: default - pass        1.08e-6               2.19e-7       <= 1.5e-6, so the old 3e-6 stays for default - twin
                        default - twin        6.95e-7               2.22e-7
                        pass - twin           8.50e-7               1.94e-7
      full catalog:     default - pass        1.08e-6               2.19e-7
                        default - twin        6.95e-7               9.05e-7       bound: twice that (fp32 results move with the order
                        pass - twin           8.50e-7               9.27e-7       of the LDS additions): 1.39e-6 / 1.81e-6
    fp64: 1.6e-12 / 1.3e-12 against the twin on the full catalog; 1e-10 stays."""
    import torch
    from baryonification_amd import _lib, engine, synthetic as syn
    N, nside = 200_000, 512
    cat = syn.make_catalog(N)
    rng = np.random.default_rng(77)
    k = 64
    cat['dec'][:k] = np.where(rng.random(k) < 0.5, 1.0, -1.0) * (90.0 - rng.random(k) ** 3 * 3.0)          # within 3 degrees of a pole
    cat['dec'][:4] = [90.0 - 1e-7, -90.0 + 1e-7, 89.99, -89.999]
    cat['ra'][:k] = rng.uniform(0, 360, k)
    cat['M'][:k] = 10.0 ** rng.uniform(12.0, 15.0, k)
    # large discs anywhere: the heaviest halo at z = 0.001 (radius > pi: the whole sphere) .. 0.02 (0.24 rad: wide at |dec| > 55 degrees)
    cat['z'][k:k + 12] = np.geomspace(0.001, 0.02, 12)
    cat['M'][k:k + 12] = cat['M'].max()
    cat['dec'][k:k + 12] = rng.uniform(-90, 90, 12)
    z, M, r = syn.table_grid(cat, pad=1e-9)
    table = syn.paint_table(z, M, r) if paint else syn.displacement_table(z, M, r)
    axes = [np.log(1 + z), np.log(M), np.log(r)]
    values = np.log(table) if paint else table
    dev = torch.device('cuda', 0)
    npix = 12 * nside * nside
    cd, keep1 = _cat_dev(torch, _lib, dev, cat)
    cd_wide, keep2 = _cat_dev(torch, _lib, dev, cat, idx=np.arange(k + 12))         # the wide discs alone
    keeps = []

    def make_plan(ax, v):
        model, keep = engine.model_from_tables(ax, v, syn.COSMO, 10.0, 10.0, log_values=paint)
        keeps.append(keep)
        return engine.ShellPlan(model, keep, nside, N, 0, torch.cuda.current_stream().cuda_stream)

    plan = make_plan(axes, values)
    twin = make_plan(*_twin_tables(axes, values))
    assert plan.precision(_lib.ACC_PARITY)[0] == _lib.ACC_PARITY and twin.precision(_lib.ACC_PARITY)[0] == _lib.ACC_F64    # fast / generic kernel
    monkeypatch.setenv('BFGX_K1_FLUID', '0')
    barrier = make_plan(axes, values)
    monkeypatch.delenv('BFGX_K1_FLUID')

    def full(pl, c=cd):
        out = torch.zeros(npix * (1 if paint else 3), dtype=torch.float64 if (paint or f64) else torch.float32, device=dev)
        if paint:
            pl.paint(c, out.data_ptr(), acc_f64=(1 if f64 else 2))
        else:
            pl.offsets(c, out.data_ptr(), f64)
        torch.cuda.synchronize()
        pl.status()
        return out

    a, b, c = full(plan), full(twin), full(barrier)
    scale = b.abs().max().item()
    tol = 1e-10 if f64 else 3e-6          # (fp32 pair math arranged differently; fp64: the two routes' libm-free / libm trigonometry)
    tol_full = 1e-10 if f64 else (2 * 9.05e-7 if paint else 2 * 6.95e-7)
    assert scale > 0
    err_wide = (full(plan, cd_wide) - full(twin, cd_wide)).abs().max().item()
    err_full, err_form = (a - b).abs().max().item(), (c - a).abs().max().item()
    print('wide discs alone %.3e, full catalog %.3e, barrier form vs default %.3e (of scale)' % (err_wide / scale, err_full / scale, err_form / scale))
    assert err_wide <= tol * scale, (err_wide, scale)
    assert err_full <= tol_full * scale, (err_full, scale)
    assert err_form <= tol * scale
    n_twin = twin.count_pairs(cd, not paint)
    assert plan.count_pairs(cd, not paint) == n_twin == barrier.count_pairs(cd, not paint) > 2e6
    # band-restricted passes (what a rank of a spatially sharded run computes): the polar bands, a belt, the cap / belt boundary
    bounds = plan.bands()
    nb = len(bounds) - 1
    comp = 1 if paint else 3
    for b0, b1 in ((0, 2), (nb - 1, nb), (nb // 2 - 1, nb // 2 + 2), (nb // 4, nb // 4 + 3)):
        p0, p1 = int(bounds[b0]), int(bounds[b1])
        got = []
        for pl in (plan, twin):
            sl = torch.full(((p1 - p0) * comp,), 7.0, dtype=a.dtype, device=dev)
            if paint:
                pl.paint_bands(cd, b0, b1, sl.data_ptr(), acc_f64=(1 if f64 else 2))
            else:
                pl.offsets_bands(cd, b0, b1, sl.data_ptr(), f64)
            torch.cuda.synchronize()
            pl.status()
            got.append(sl)
        assert (got[0] - got[1]).abs().max().item() <= tol_full * scale
        assert (got[0] - a[p0 * comp:p1 * comp]).abs().max().item() <= tol * scale
    plan.close(); twin.close(); barrier.close()


def _fast_and_twin_plans(torch, engine, syn, cat, nside, **grid):
    z, M, r = syn.table_grid(cat, pad=1e-9, **grid)
    axes, table = [np.log(1 + z), np.log(M), np.log(r)], syn.displacement_table(z, M, r)
    plans = []
    for ax, v in ((axes, table), _twin_tables(axes, table)):
        model, keep = engine.model_from_tables(ax, v, syn.COSMO, 10.0, 10.0)
        plans.append((engine.ShellPlan(model, keep, nside, cat['M'].size, 0, torch.cuda.current_stream().cuda_stream), keep))
    return plans


def _tiled_equals_per_halo(torch, _lib, dev, plans, cat, nside):
    """fp64 pix_offsets of the tile-owned path (algo 1) against the per-halo path (algo 0) within 2e-14 absolute; the same pair census"""
    cd, cols = _cat_dev(torch, _lib, dev, cat)
    kinds = []
    for plan, keep in plans:
        got = []
        for algo in (0, 1):
            off = torch.zeros(12 * nside * nside * 3, dtype=torch.float64, device=dev)
            plan.set_algo(algo)
            plan.offsets(cd, off.data_ptr(), True)
            torch.cuda.synchronize()
            plan.status()
            got.append((off, plan.count_pairs(cd, True)))
        plan.set_algo(1)
        kinds.append(plan.precision(_lib.ACC_PARITY)[0])
        err = (got[0][0] - got[1][0]).abs().max().item()
        print('algo 1 - algo 0: %.3e, pairs %d' % (err, got[1][1]))
        assert got[0][0].abs().max().item() > 0 and err <= 2e-14
        assert got[0][1] == got[1][1] > 0
        del got
        plan.close()
    assert kinds == [_lib.ACC_PARITY, _lib.ACC_F64]          # the fast kernel, then the generic one


def test_generic_plan_lists_are_placed_by_cursor(gpu):
    """a generic plan (here: a non-uniform ln r axis) lists every halo in the tiles' shared lists: halos over at most kRefMax tiles with
    slot -1, the others through the tile enumeration, all placed by the one cursor of the placement pass.  Four halos within 1e-7 .. 1
    degree of the poles and two discs over more than kRefMax tiles among 3000; the same on the fast plan of the uniform table"""
    import torch
    from baryonification_amd import _lib, engine, synthetic as syn
    N, nside = 3000, 32
    cat = syn.make_catalog(N, seed=321)
    cat['dec'][:4] = [90.0 - 1e-7, -90.0 + 1e-3, 89.0, -89.9]
    cat['ra'][:4] = [0.0, 123.0, 359.9999, 1e-9]
    cat['z'][4:6] = [0.01, 0.008]
    cat['M'][4:6] = 3e15
    cat['dec'][4:6] = [12.0, -47.0]
    plans = _fast_and_twin_plans(torch, engine, syn, cat, nside)
    _tiled_equals_per_halo(torch, _lib, torch.device('cuda', 0), plans, cat, nside)


def test_tile_scan_over_several_workgroups(gpu):
    """above 8192 tiles the scan of the tiles' entry counts is spread over workgroups (block totals, their scan, block offsets): NSIDE 2048
    with its 24 704 tiles is the smallest default tiling that takes it.  2000 halos, the two poles among them; a fast and a generic plan"""
    import torch
    from baryonification_amd import _lib, engine, synthetic as syn
    N, nside = 2000, 2048
    cat = syn.make_catalog(N, seed=654)
    cat['dec'][:2] = [90.0 - 1e-7, -90.0 + 1e-7]
    plans = _fast_and_twin_plans(torch, engine, syn, cat, nside)
    _tiled_equals_per_halo(torch, _lib, torch.device('cuda', 0), plans, cat, nside)


def test_catalog_written_patch_by_patch_equals_shuffled(gpu):
    """a catalog in (band of rings, azimuth) order -- what a lightcone pipeline usually writes -- makes consecutive threads of K0 name the
    same tile: they take their slots with one atomic per run of lanes (wave_run_issue), on counters a cache line apart.  Same census, same
    pix_offsets (to the last bits of the fp64 sums), same map as the same halos in shuffled order; full size, both accumulator types."""
    N, nside = 1_000_000, 1024
    torch, _lib, syn, cat, axes, table, plan, dev = _setup(N, nside, paint=False)
    npix = 12 * nside * nside
    zc = np.sin(np.radians(cat['dec']))
    ring = np.where(np.abs(zc) <= 2 / 3, nside * (2 - 1.5 * zc), np.where(zc > 0, nside * np.sqrt(3 * (1 - np.abs(zc))), 4 * nside - nside * np.sqrt(3 * (1 - np.abs(zc)))))
    order = np.argsort((ring.astype(np.int64) // 32) * 4096 + (cat['ra'] / 360.0 * 4096).astype(np.int64), kind='stable')
    hmap = syn.make_map(nside)
    d_map = torch.from_numpy(hmap).to(dev)
    res = []
    for idx in (None, order):
        cd, keep1 = _cat_dev(torch, _lib, dev, cat, idx)
        off64 = torch.zeros(npix * 3, dtype=torch.float64, device=dev)
        plan.offsets(cd, off64.data_ptr(), True)
        f_off = torch.zeros(npix * 3, dtype=torch.float32, device=dev)
        out = torch.zeros(npix, dtype=torch.float64, device=dev)
        sums = torch.zeros(2, dtype=torch.float64, device=dev)
        plan.baryonify(cd, d_map.data_ptr(), f_off.data_ptr(), out.data_ptr(), sums.data_ptr(), acc_f64=False)
        torch.cuda.synchronize()
        plan.status()
        s = sums.cpu().numpy()
        assert np.isclose(s[1], s[0])
        res.append((off64, out, plan.count_pairs(cd, True)))
    assert res[0][2] == res[1][2] == 53984077
    scale = res[0][0].abs().max().item()
    assert (res[0][0] - res[1][0]).abs().max().item() <= 1e-13 * scale
    assert (res[0][1] - res[1][1]).abs().max().item() <= 1e-6 * hmap.mean()
    plan.close()


@pytest.mark.parametrize('scale', [1.0, 60.0])
def test_fused_band_entry_keeps_the_parity_grade_mode(gpu, scale):
    """bfgx_offsets_regrid_bands_device (a rank's share of a spatially sharded step: K0 .. K2 of its bands + the band either side) with
    BFGX_ACC_PARITY: the split fp32 pix_offsets stay on the device, so the mode is what it is on one GPU -- the slices of three "ranks" put
    together equal the full-map parity-grade call to 1e-9 mean(map) and the fp64 call to 1e-8"""
    import torch
    from baryonification_amd import _lib, engine, synthetic as syn
    nside, nh = 256, 30_000
    cat = syn.make_catalog(nh)
    cat['dec'][:4] = [89.95, -89.9, 89.99, -89.999]
    z, M, r = syn.table_grid(cat)
    model, keep = engine.model_from_tables([np.log(1 + z), np.log(M), np.log(r)], syn.displacement_table(z, M, r) * scale, syn.COSMO, 10.0, 10.0)
    dev = torch.device('cuda:0')
    stream = torch.cuda.current_stream().cuda_stream
    plan = engine.ShellPlan(model, keep, nside, nh, device=0, stream=stream)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in cat.items()}
    lnz, lnM = _lib.table_coords(cat['M'], cat['z'])
    t['lnz'], t['lnM'] = torch.from_numpy(lnz).to(dev), torch.from_numpy(lnM).to(dev)
    cd = _lib.make_catalog_dev(nh, t['M'].data_ptr(), t['z'].data_ptr(), t['ra'].data_ptr(), t['dec'].data_ptr(), ln1pz_ptr=t['lnz'].data_ptr(), lnM_ptr=t['lnM'].data_ptr())
    npix = 12 * nside * nside
    d_map = torch.from_numpy(syn.make_map(nside)).to(dev)
    ref = {}
    for name, acc in (('parity', _lib.ACC_PARITY), ('f64', _lib.ACC_F64)):
        off = torch.zeros(npix * 3, dtype=torch.float64, device=dev)
        out = torch.zeros(npix, dtype=torch.float64, device=dev)
        sums = torch.zeros(2, dtype=torch.float64, device=dev)
        plan.baryonify(cd, d_map.data_ptr(), off.data_ptr(), out.data_ptr(), sums.data_ptr(), acc_f64=acc)
        torch.cuda.synchronize()
        ref[name] = out.cpu().numpy()
    assert np.abs(ref['parity'] - ref['f64']).max() <= 1e-8 * ref['f64'].mean() and np.abs(ref['f64'] - d_map.cpu().numpy()).max() > 0
    first = plan.bands()
    nb = len(first) - 1
    cuts = [0, nb // 3, 2 * nb // 3, nb]
    plan.set_band_reach(16)
    got = np.zeros(npix)
    foreign = torch.zeros(1, dtype=torch.int64, device=dev)
    tot = np.zeros(2)
    for q in range(3):
        b0, b1 = cuts[q], cuts[q + 1]
        B0, B1 = max(b0 - 1, 0), min(b1 + 1, nb)
        wlo, whi, p0, p1 = int(first[B0]), int(first[B1]), int(first[b0]), int(first[b1])
        full = torch.full(((whi - wlo) * 3,), np.nan, dtype=torch.float64, device=dev)                # 24 bytes per pixel: hi + lo halves
        sl = torch.full((p1 - p0,), np.nan, dtype=torch.float64, device=dev)
        sums = torch.zeros(2, dtype=torch.float64, device=dev)
        plan.offsets_regrid_bands(cd, B0, B1, full.data_ptr(), b0, b1, d_map.data_ptr(), sl.data_ptr(), sums.data_ptr(), foreign.data_ptr(),
                                  acc_f64=_lib.ACC_PARITY)
        torch.cuda.synchronize()
        plan.status()
        got[p0:p1] = sl.cpu().numpy()
        tot += sums.cpu().numpy()
    plan.close()
    assert np.isfinite(got).all()
    if int(foreign.item()) == 0:            # (far deposits that leave a slice are the caller's to route: the polar halos here may produce a few)
        assert np.abs(got - ref['parity']).max() <= 1e-9 * ref['parity'].mean(), np.abs(got - ref['parity']).max() / ref['parity'].mean()
        assert abs(tot[1] - tot[0]) <= 1e-9 * tot[0]
    else:
        inside = np.abs(got - ref['parity']) <= 1e-9 * ref['parity'].mean()
        assert (~inside).sum() <= 4 * int(foreign.item())
