"""
Time of MeasureProfilesGrid's device entry on one representative case: an ngrid^3 fp64 map on the device, a 205 / h Mpc box, 100 000 halos
of synthetic.make_catalog at uniform positions, epsilon_max 5, z = 0, 16 bins (0, then log-spaced out to the largest ball) -- and of what it
replaces, the numpy restatement (tests/gridprofiles_oracle.py) on the first --oracle-halos halos with the map on the host.

    python scripts/grid_profiles_time.py [--ngrid 512] [--halos 100000] [--reps 20] [--oracle-halos 1000]

The device figure is the median over the timed calls after one warm-up call, a host clock around a call that ends in a device synchronise
(the entry uploads the catalog and allocates its workspace inside the call).  `pairs` are the (pixel, halo) pairs inside the balls;
`algorithmic_bytes` = 8 B per pair of each map + the outputs; `hbm_fraction` relates them to 8 TB/s.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import torch
import baryonification_amd as bfg
from baryonification_amd import _lib
from baryonification_amd import synthetic as syn

HBM_PEAK = 8.0e12             # B/s, the MI355X's specified HBM3E rate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ngrid', type=int, default=512)
    ap.add_argument('--halos', type=int, default=100_000)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--oracle-halos', type=int, default=1000)
    args = ap.parse_args()
    assert _lib.load().bfgx_device_count() > 0, "no HIP device: timings are taken on the GPU only"
    dev = torch.device('cuda', 0)
    N, nh, eps, zr = args.ngrid, args.halos, 5.0, 0.0
    L = 205.0 / syn.COSMO['h']
    bins = (np.arange(N) + 0.5) * L / N
    rng = np.random.default_rng(syn.SEED_CATALOG)
    M = syn.make_catalog(nh, seed=syn.SEED_CATALOG)['M'].astype(np.float32).astype(np.float64)
    pos = rng.uniform(0, L, (nh, 3)).astype(np.float32).astype(np.float64)
    torch.manual_seed(syn.SEED_MAP)
    tmap = torch.rand((N, N, N), dtype=torch.float64, device=dev) + 0.5
    HCat = bfg.utils.HaloNDCatalog(x=pos[:, 0], y=pos[:, 1], z=pos[:, 2], M=M, redshift=zr, cosmo=syn.COSMO)
    Map = bfg.utils.GriddedMap(map=_Shape(N), redshift=zr, bins=bins, cosmo=syn.COSMO)      # (the map lives on the device only)
    R, R_q = bfg.Runners.MeasureProfilesGrid(HCat, Map, eps, verbose=False, r_edges=[0.0, 1.0]).radii()
    edges = np.concatenate([[0.0], np.geomspace(0.3 * L / N, float(R_q.max()), 16)])
    runner = bfg.Runners.MeasureProfilesGrid(HCat, Map, eps, verbose=False, r_edges=edges)
    whole = bfg.Runners.MeasureProfilesGrid(HCat, Map, eps, verbose=False, r_edges=[0.0, L])
    pairs = int(whole.process(map=tmap).npix.sum().item())
    res = [None]

    def device_call():
        res[0] = runner.process(map=tmap)
    device_call()                                                     # warm-up: code objects, first allocations
    t = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        device_call()
        torch.cuda.synchronize()
        t.append(1e3 * (time.perf_counter() - t0))
    ms = float(np.median(t))
    nb = edges.size - 1
    nbytes = 8 * pairs + 16 * nh * nb
    out = {'ngrid': N, 'halos': nh, 'L': L, 'epsilon_max': eps, 'bins': nb, 'reps': args.reps, 'device_entry_ms': [ms, float(np.min(t)), float(np.max(t))],
           'pairs': pairs, 'pairs_in_bins': int(res[0].npix.sum().item()), 'pairs_per_s': pairs / (1e-3 * ms), 'algorithmic_bytes': nbytes,
           'hbm_fraction': nbytes / (1e-3 * ms) / HBM_PEAK, 'R_q_max': float(R_q.max()), 'R_q_median': float(np.median(R_q))}
    if args.oracle_halos > 0:
        import gridprofiles_oracle as K
        from oracle import grid as G
        no = min(args.oracle_halos, nh)
        hmap = tmap.cpu().numpy()
        cat = {k: np.array(HCat.cat[k][:no], dtype=np.float64) for k in ('M', 'x', 'y', 'z')}
        t0 = time.perf_counter()
        o = K.measure(K.pairs(bins, 3, cat, zr, eps, G.grid_background(syn.COSMO)), edges, hmap)
        out['oracle_halos'] = no
        out['oracle_ms'] = 1e3 * (time.perf_counter() - t0)
        out['oracle_equal_counts'] = bool(np.array_equal(o['npix'], res[0].npix[:no].cpu().numpy()))
    print(json.dumps(out))


class _Shape(object):
    """stands in for the host copy of a map that lives on the device only: GriddedMap reads its shape"""

    def __init__(self, N):
        self.shape = (N, N, N)


if __name__ == '__main__':
    main()
