"""
Time of the per-halo (callable) routes split into the model's Python calls and the rest (device work, transfers, the loop):
BaryonifyGrid / PaintProfilesGrid on a 2D 1024^2 map with 5 000 halos and a 3D 128^3 map with 2 000 halos, BaryonifySnapshot on
10^6 particles with 2 000 halos; the closed-form models of tests/callable_models.py with bfgx_exact = True, the second of two calls.

    python scripts/callable_route_time.py
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import baryonification_amd as bfg
from baryonification_amd import synthetic as syn
import callable_models as CM

def wrap(model, name):
    f = getattr(model, name); acc = [0.0]
    def g(*a):
        t0 = time.perf_counter(); v = f(*a); acc[0] += time.perf_counter() - t0; return v
    setattr(model, name, g); return acc

for ndim, N, nh, kind in [(2, 1024, 5000, 'baryonify'), (2, 1024, 5000, 'paint'), (3, 128, 2000, 'baryonify'), (3, 128, 2000, 'paint')]:
    rng = np.random.default_rng(1)
    L = 1.0 * N if ndim == 2 else 2.0 * N
    bins = (np.arange(N) + 0.5) * (L / N)
    M = 10 ** rng.uniform(12.5, 14.8, nh); x, y, z = rng.uniform(0, L, (3, nh))
    H = bfg.utils.HaloNDCatalog(x=x, y=y, z=z if ndim == 3 else None, M=M, redshift=0.2, cosmo=syn.COSMO)
    mp = rng.poisson(2.0, (N,) * ndim).astype(float) if kind == 'baryonify' else np.zeros((N,) * ndim)
    G = bfg.utils.GriddedMap(map=mp, redshift=0.2, bins=bins, cosmo=syn.COSMO)
    for rep in range(2):
        if kind == 'baryonify':
            m = CM.CallableDisplacement(); acc = wrap(m, 'displacement'); R = bfg.Runners.BaryonifyGrid(H, G, 4.0, m, verbose=False)
        else:
            m = CM.CallableProfile(); acc = wrap(m, 'projected' if ndim == 2 else 'real'); R = bfg.Runners.PaintProfilesGrid(H, G, 4.0, m, verbose=False)
        t0 = time.perf_counter(); R.process(); tt = time.perf_counter() - t0
    print(f"split {kind} {ndim}D {N}^{ndim} {nh} halos: total {tt*1e3:.1f} ms, model calls {acc[0]*1e3:.1f} ms ({m.calls} calls), rest {1e3*(tt-acc[0]):.1f} ms, pairs {R.last_stats['n_pairs']}", flush=True)

for ndim in (3, 2):
    rng = np.random.default_rng(2)
    L, nh, npart = 250.0, 2000, 1_000_000
    M = 10 ** rng.uniform(12.5, 14.8, nh); x, y, z = rng.uniform(0, L, (3, nh))
    P = rng.uniform(0, L, (3, npart))
    H = bfg.utils.HaloNDCatalog(x=x, y=y, z=z if ndim == 3 else None, M=M, redshift=0.0, cosmo=syn.COSMO)
    S = bfg.utils.ParticleSnapshot(x=P[0], y=P[1], z=P[2] if ndim == 3 else None, M=np.ones(npart), L=L, redshift=0.0, cosmo=syn.COSMO)
    for rep in range(2):
        m = CM.CallableDisplacement(); acc = wrap(m, 'displacement'); R = bfg.Runners.BaryonifySnapshot(H, S, 4.0, m, verbose=False)
        t0 = time.perf_counter(); R.process(); tt = time.perf_counter() - t0
    print(f"split snapshot {ndim}D {npart} particles {nh} halos: total {tt*1e3:.1f} ms, model calls {acc[0]*1e3:.1f} ms ({m.calls} calls), rest {1e3*(tt-acc[0]):.1f} ms, pairs {R.last_stats['n_pairs']}", flush=True)
