"""Device times of the map statistics (HIP events around calls on CUDA tensors, so nothing crosses PCIe inside the window except
the few result numbers of map_moments), one JSON line: at NSIDE 1024 and 2048 a plain read of the map (torch.sum: the floor of the
two reductions), smoothing (Gaussian, iter=3, lmax = 3 nside - 1), map_moments of K = 3 maps (order 4) and peak_counts (64 bins)
of RING and NEST maps (and the stencil kernel on a constant map, with 1 bin and with 4096 bins); at NSIDE 1024 shell_statistics of K = 2 maps at 5 scales with peak counts.  Each is the median of --reps
timed calls after one warm-up call.

    python scripts/mapstats_time.py [--reps 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from baryonification_amd import _lib, utils as U  # noqa: E402
from baryonification_amd.utils import mapstats  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(1)
    res = {'gpu': torch.cuda.get_device_name(0), 'reps': args.reps}
    edges = np.linspace(-4.0, 4.0, 65)
    for nside in (1024, 2048):
        npix = 12 * nside * nside
        maps = torch.randn((3, npix), dtype=torch.float64, device=dev, generator=g)
        key = lambda name: '%s_nside%d_ms' % (name, nside)
        res[key('plain_read')] = round(timed(lambda: torch.sum(maps[0]), args.reps), 4)
        res[key('smoothing_iter3')] = round(timed(lambda: U.smoothing(maps[0], fwhm=np.radians(0.2)), max(3, args.reps // 2)), 3)
        res[key('map_moments_K3')] = round(timed(lambda: U.map_moments(maps), args.reps), 4)
        res[key('map_moments_K1')] = round(timed(lambda: U.map_moments(maps[0]), args.reps), 4)
        # the kernels alone (no result copy): the enqueue-only entry on preallocated outputs
        n_out = torch.empty(1, dtype=torch.int64, device=dev)
        out = torch.empty(3 + 31, dtype=torch.float64, device=dev)
        work = torch.empty(_lib.MAPSTATS_WORK_DOUBLES, dtype=torch.float64, device=dev)
        res[key('moments_kernels_K3')] = round(timed(lambda: mapstats._moments_device(maps, None, 4, n_out, out, work), args.reps), 4)
        res[key('moments_kernels_K1')] = round(timed(lambda: mapstats._moments_device(maps[:1], None, 4, n_out, out, work), args.reps), 4)
        ed = torch.from_numpy(edges).to(dev)
        counts = torch.empty((2, 64), dtype=torch.int64, device=dev)
        flags = torch.empty(npix, dtype=torch.int8, device=dev)
        for nest in (0, 1):
            name = 'peaks_kernel_%s' % ('nest' if nest else 'ring')
            res[key(name)] = round(timed(lambda: mapstats._peaks_device(maps[0], None, nside, nest, ed, counts, None), args.reps), 4)
            res[key(name + '_flags')] = round(timed(lambda: mapstats._peaks_device(maps[0], None, nside, nest, ed, counts, flags), args.reps), 4)
        # what the stencil kernel waits for: no search and no histogram (a constant map has no extrema), one bin (no search), 4096 bins
        const = torch.ones(npix, dtype=torch.float64, device=dev)
        res[key('peaks_kernel_ring_constant_map')] = round(timed(lambda: mapstats._peaks_device(const, None, nside, 0, ed, counts, None), args.reps), 4)
        del const
        for nb in (1, 4096):
            e2 = torch.linspace(-4.0, 4.0, nb + 1, dtype=torch.float64, device=dev)
            c2 = torch.empty((2, nb), dtype=torch.int64, device=dev)
            res[key('peaks_kernel_ring_%dbins' % nb)] = round(timed(lambda: mapstats._peaks_device(maps[0], None, nside, 0, e2, c2, None), args.reps), 4)
        res[key('peak_counts_ring')] = round(timed(lambda: U.peak_counts(maps[0], edges), args.reps), 4)
        res['maxima_nside%d' % nside] = int(U.peak_counts(maps[0], edges)['maxima'].sum())
        if nside == 1024:
            scales = np.radians([0.0, 5.0, 10.0, 20.0, 40.0]) / 60.0
            res['shell_statistics_K2_5scales_nside1024_ms'] = round(timed(
                lambda: U.shell_statistics(maps[:2], scales, peak_bins=edges), max(3, args.reps // 2)), 3)
        del maps, flags
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
