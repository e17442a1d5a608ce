#!/usr/bin/env python
"""
Generates tests/golden/callable_*.npz by running the UNMODIFIED reference (imported through the oracle/refshim stand-ins for pyccl /
healpy / numba) with the plain-Python models of tests/callable_models.py.  Build container only:

    python tests/golden/make_golden_callable.py

Reference code exercised as shipped:

    BaryonForge.Runners.BaryonifyGrid.process        (Map2DRunner.py:431-607), 2D, 2D + ellipticity, 3D
    BaryonForge.Runners.PaintProfilesGrid.process    (Map2DRunner.py:676-817), 2D, 2D + ellipticity, 3D
    BaryonForge.Runners.BaryonifySnapshot.process    (SnapshotRunner.py:173-262), 2D and 3D (particles regenerated from a seed by
                                                      tests/helpers.py; only the moved ones are stored)

The models are called once per halo on each cutout (no table); the fixtures store inputs, the reference's map and its number of model
calls (data only).
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from oracle.refshim import install  # noqa: E402

install.install()
import BaryonForge as bfg  # noqa: E402  (the reference)

import make_golden_grid as MGG  # noqa: E402  (catalogs with halos on box edges and corners; COSMO with w0 != -1)
import callable_models as CM  # noqa: E402
import helpers as TH  # noqa: E402


def run(name, kind, shape, L, nh, seed, redshift, eps, ell=False):
    ndim = len(shape)
    N = shape[0]
    bins = (np.arange(N) + 0.5) * (L / N)
    cat, extra = MGG.grid_catalog(nh, L, seed, 13.0, 14.8, ndim, ell)
    cat['M'][6] = 1e11                     # Nsize < 2: BaryonifyGrid skips it and never calls the model (Map2DRunner.py:498)
    HCat = bfg.utils.HaloNDCatalog(x=cat['x'], y=cat['y'], M=cat['M'], redshift=redshift, cosmo=MGG.COSMO, z=cat['z'], **extra)
    used = {k: np.array(HCat.cat[k], dtype=np.float64) for k in ('M', 'x', 'y', 'z')}
    rmat = None
    if ell:         # the matrices the runner builds (float32 columns, Map2DRunner.py:490-493, :528), stored for the product's test
        runner0 = bfg.Runners.DefaultRunnerGrid.__new__(bfg.Runners.DefaultRunnerGrid)
        rmat = np.zeros((nh, 2, 2))
        for j in range(nh):
            A_j = HCat.cat['A_ell'][j]
            rmat[j] = runner0.build_Rmat(A_j / np.sqrt(np.sum(A_j ** 2)), HCat.cat['q_ell'][j])
    t0 = time.time()
    if kind == 'baryonify':
        hmap = np.random.default_rng(seed + 7).poisson(3.0, shape).astype(np.float64)
        GMap = bfg.utils.GriddedMap(map=hmap, redshift=redshift, bins=bins, cosmo=MGG.COSMO)
        model = CM.CallableDisplacement()
        out = bfg.Runners.BaryonifyGrid(HCat, GMap, eps, model, use_ellipticity=ell, verbose=False).process()
    else:
        hmap = np.zeros(shape)
        GMap = bfg.utils.GriddedMap(map=hmap, redshift=redshift, bins=bins, cosmo=MGG.COSMO)
        model = CM.CallableProfile()
        out = bfg.Runners.PaintProfilesGrid(HCat, GMap, eps, model, use_ellipticity=ell, verbose=False).process()
    print(f"{name:24s} {kind:9s} shape={shape} N={nh:4d} calls={model.calls:4d} ref {time.time() - t0:6.1f}s  "
          f"changed px = {int((out != hmap).sum())}  max|out| = {np.abs(out).max():.4g}")
    np.savez_compressed(
        os.path.join(HERE, name + '.npz'), kind=kind, ndim=ndim, npix=N, L=L, bins=bins, redshift=redshift, eps_runner=eps,
        cat_M=used['M'], cat_x=used['x'], cat_y=used['y'], cat_z=used['z'], rmat=rmat if rmat is not None else np.zeros(0),
        map_in=hmap.astype(np.uint8) if kind == 'baryonify' else np.zeros(0, dtype=np.uint8),
        cosmo_runner=np.array([MGG.COSMO[k] for k in ('Omega_m', 'Omega_b', 'h', 'sigma8', 'n_s', 'w0')]),
        calls=model.calls, expected=out)


def run_snapshot(name, ndim, L, npart, nh, seed, redshift, eps):
    cat, _ = MGG.grid_catalog(nh, L, seed, 13.0, 14.8, 3)
    HCat = bfg.utils.HaloNDCatalog(x=cat['x'], y=cat['y'], M=cat['M'], redshift=redshift, cosmo=MGG.COSMO, z=cat['z'] if ndim == 3 else None)
    used = {k: np.array(HCat.cat[k], dtype=np.float64) for k in ('M', 'x', 'y', 'z')}
    halo0 = np.array([used['x'][0], used['y'][0], used['z'][0]])
    part = TH.snapshot_particles(seed, npart, L, halo0)[:, :ndim]
    Snap = bfg.utils.ParticleSnapshot(x=part[:, 0], y=part[:, 1], z=part[:, 2] if ndim == 3 else None, M=np.ones(npart), L=L,
                                      redshift=redshift, cosmo=MGG.COSMO)
    model = CM.CallableDisplacement()
    t0 = time.time()
    new_cat = bfg.Runners.BaryonifySnapshot(HCat, Snap, eps, model, verbose=False).process()
    out = np.stack([new_cat[k] for k in ('x', 'y', 'z')[:ndim]], axis=1)
    moved = ~(out == part).all(axis=1)
    print(f"{name:24s} snapshot  ndim={ndim} npart={npart} nh={nh} calls={model.calls} ref {time.time() - t0:5.1f}s  moved = {int(moved.sum())}"
          f"  nan = {int(np.isnan(out).any(axis=1).sum())}")
    np.savez_compressed(os.path.join(HERE, name + '.npz'), kind='snapshot', ndim=ndim, L=L, redshift=redshift, eps_runner=eps, part_seed=seed,
                        npart=npart, halo0=halo0, moved_idx=np.nonzero(moved)[0], moved_pos=out[moved], cat_M=used['M'], cat_x=used['x'],
                        cat_y=used['y'], cat_z=used['z'],
                        cosmo_runner=np.array([MGG.COSMO[k] for k in ('Omega_m', 'Omega_b', 'h', 'sigma8', 'n_s', 'w0')]),
                        calls=model.calls)


def main():
    run('callable_grid2d_baryonify', 'baryonify', (96, 96), 60.0, 40, 11, 0.2, 4.0)
    run('callable_grid2d_baryonify_ell', 'baryonify', (96, 96), 60.0, 40, 12, 0.2, 4.0, ell=True)
    run('callable_grid3d_baryonify', 'baryonify', (32, 32, 32), 40.0, 24, 13, 0.0, 3.0)
    run('callable_grid2d_paint', 'paint', (96, 96), 60.0, 40, 14, 0.2, 3.0)
    run('callable_grid2d_paint_ell', 'paint', (96, 96), 60.0, 40, 15, 0.2, 3.0, ell=True)
    run('callable_grid3d_paint', 'paint', (32, 32, 32), 40.0, 24, 16, 0.0, 3.0)
    run_snapshot('callable_snap2d', 2, 80.0, 8000, 30, 17, 0.1, 5.0)
    run_snapshot('callable_snap3d', 3, 60.0, 12000, 30, 18, 0.0, 5.0)


if __name__ == '__main__':
    main()
