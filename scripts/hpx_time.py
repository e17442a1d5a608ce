"""Device times of the HEALPix pixel functions (HIP events around the bfgx_hpx_*_device entries), one JSON line:
ud_grade 8192 -> 2048 and 4096 -> 1024 (RING -> RING, fp64), get_interp_val at 1e8 points on an NSIDE 4096 map, and
regrid_pixels_hpix of 12.6e6 x 4 contributions.  Each is the median of --reps timed calls after one warm-up call.

    python scripts/hpx_time.py [--reps 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from baryonification_amd import _lib  # noqa: E402


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
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    L = _lib.load()
    dev = torch.device('cuda', 0)
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream or None)
    p = lambda t: C.c_void_p(t.data_ptr())
    g = torch.Generator(device=dev).manual_seed(1)
    res = {'gpu': torch.cuda.get_device_name(0)}

    for ni, no in ((8192, 2048), (4096, 1024)):
        m = torch.rand(12 * ni * ni, dtype=torch.float64, device=dev, generator=g)
        out = torch.empty(12 * no * no, dtype=torch.float64, device=dev)
        for oi in (0, 1):
            def run():
                _lib.check(L.bfgx_hpx_ud_grade_device(0, s, ni, no, 1, oi, oi, 0, 1.0, 1, 1, p(m), p(out)))
            ms = timed(run, args.reps)
            gb = (m.numel() + out.numel()) * 8 / 1e9
            res['ud_grade_%d_%d_%s_ms' % (ni, no, 'nest' if oi else 'ring')] = round(ms, 4)
            res['ud_grade_%d_%d_%s_TBps' % (ni, no, 'nest' if oi else 'ring')] = round(gb / ms, 3)
        del m, out
        torch.cuda.empty_cache()

    nside, n = 4096, 100_000_000
    m = torch.rand(12 * nside * nside, dtype=torch.float64, device=dev, generator=g)
    th = torch.acos(2 * torch.rand(n, dtype=torch.float64, device=dev, generator=g) - 1)
    ph = 2 * np.pi * torch.rand(n, dtype=torch.float64, device=dev, generator=g)
    out = torch.empty(n, dtype=torch.float64, device=dev)

    def interp():
        _lib.check(L.bfgx_hpx_interp_val_device(0, s, nside, 0, 1, 1, p(m), n, p(th), p(ph), p(out)))
    res['interp_val_1e8_nside4096_ms'] = round(timed(interp, args.reps), 3)
    del m, th, ph, out
    torch.cuda.empty_cache()

    nside = 1024
    npix = 12 * nside * nside
    h = torch.zeros(npix, dtype=torch.float64, device=dev)
    base = torch.arange(npix, device=dev)
    pix = torch.stack([base, (base + 1) % npix, (base + 4 * nside) % npix, (base + 4 * nside + 1) % npix], dim=1).contiguous()
    w = torch.full((npix, 4), 0.25, dtype=torch.float64, device=dev)
    vals = torch.rand(npix, dtype=torch.float64, device=dev, generator=g)

    def scatter():
        _lib.check(L.bfgx_hpx_scatter_add_device(0, s, npix, p(h), npix, p(vals), p(pix), p(w)))
    res['scatter_add_12.6e6x4_ms'] = round(timed(scatter, args.reps), 3)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
