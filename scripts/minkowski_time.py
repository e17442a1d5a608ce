"""Device times of the Minkowski functionals (HIP events around calls on CUDA tensors), one JSON line: at NSIDE 1024 and 2048 the
reduction kernel alone (bfgx_mapstats_minkowski_device, 64 bins over +-4 sigma, and 512 bins) on the six derivative maps of a
Gaussian-smoothed map (FWHM 20') and on six maps of white noise (every lane of a wavefront in another bin: the worst case of the
bin-serving rounds), the mean number of such rounds per wavefront for both, the moments kernels of K = 3 maps and a plain read of
six maps for comparison, the four syntheses of ShtPlan.alm2map_der_device, and a whole minkowski_functionals call (iter = 3,
lmax = 3 nside - 1).  Each is the median of --reps timed calls after one warm-up call.

    python scripts/minkowski_time.py [--reps 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from baryonification_amd import _lib, engine, utils as U  # noqa: E402
from baryonification_amd.utils import mapstats  # noqa: E402
from mapstats_time import timed  # noqa: E402


def rounds_per_wave(u, edges):
    """mean number of distinct bins among the 64 consecutive pixels a wavefront holds (pixels outside the edges take no round)"""
    b = torch.bucketize(u, edges, right=True) - 1
    b = torch.where((b >= 0) & (b < edges.numel() - 1), b, torch.full_like(b, -1)).reshape(-1, 64).sort(dim=1).values
    distinct = (b[:, 1:] != b[:, :-1]).sum(1) + 1 - (b[:, 0] < 0).to(torch.int64)
    return float(distinct.to(torch.float64).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(1)
    res = {'gpu': torch.cuda.get_device_name(0), 'reps': args.reps}
    for nside in (1024, 2048):
        npix = 12 * nside * nside
        lmax = 3 * nside - 1
        key = lambda name: '%s_nside%d_ms' % (name, nside)
        few = max(3, args.reps // 2)
        noise = torch.randn((6, npix), dtype=torch.float64, device=dev, generator=g)
        res[key('plain_read_6_maps')] = round(timed(lambda: torch.sum(noise), args.reps), 4)
        n_out = torch.empty(1, dtype=torch.int64, device=dev)
        out = torch.empty(3 + 31, dtype=torch.float64, device=dev)
        work = torch.empty(_lib.MAPSTATS_WORK_DOUBLES, dtype=torch.float64, device=dev)
        res[key('moments_kernels_K3')] = round(timed(lambda: mapstats._moments_device(noise[:3], None, 4, n_out, out, work), args.reps), 4)
        plan = engine.sht_plan(nside, lmax, lmax)
        alm = plan.map2alm_device(noise[0], iter=0)
        plan.almxfl_device(alm, torch.from_numpy(U.gauss_beam(np.radians(20.0 / 60.0), lmax)).to(dev), out=alm)
        smooth = torch.empty((6, npix), dtype=torch.float64, device=dev)
        res[key('alm2map_der_4_syntheses')] = round(timed(lambda: plan.alm2map_der_device(alm, smooth), few), 3)
        for name, ders in (('smooth', smooth), ('noise', noise)):
            sd = float(ders[0].std())
            for nb in (64, 512):
                edges = np.linspace(-4.0 * sd, 4.0 * sd, nb + 1)
                mf = mapstats._MinkowskiBuffers(npix, edges, (), dev)
                res[key('minkowski_kernel_%s_%dbins' % (name, nb))] = round(timed(lambda: mf.run(ders, None), args.reps), 4)
                res['rounds_per_wave_%s_%dbins_nside%d' % (name, nb, nside)] = round(rounds_per_wave(ders[0], mf.edges), 2)
        res[key('minkowski_functionals_64bins_iter3')] = round(timed(
            lambda: U.minkowski_functionals(noise[0], np.linspace(-4.0, 4.0, 65), fwhm=np.radians(20.0 / 60.0)), few), 3)
        del noise, smooth, alm
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
