"""Device times of the mode-coupling matrices (HIP events around engine.pcl_coupling_device on CUDA tensors: the zeroing of the
matrices and the kernel), one JSON line: kinds 0 (M00), 1 (M0+) and 2 (M++ and M--) at (lmax, lw) = (2047, 4094) and (6143, 6143), a
narrow band (6143, 64), and the recursion steps per second each time amounts to (a step = one l'' of one (l, l') pair with l >= l':
every second l'' up to min(l + l', lw) for kind 0, all 2 l' + 1 of them for kinds 1 and 2).  Each is the median, with the minimum and
maximum, of --reps timed calls after one warm-up call; the outputs are allocated once, outside the timed calls.

    python scripts/pcl_time.py [--reps 5]
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


def steps(lmax, lw, kind):
    """recursion steps of one call (host arithmetic)"""
    lp = np.arange(2 if kind else 0, lmax + 1, dtype=np.int64)
    total = 0
    for c in lp:
        l = np.arange(c, min(lmax, c + lw) + 1, dtype=np.int64)
        if kind:
            total += l.size * (2 * c + 1)
        else:
            total += int(((np.minimum(l + c, lw) - (l - c)) // 2 + 1).sum())
    return int(total)


def times(fn, reps):
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
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    L = _lib.load()
    res = {'gpu': torch.cuda.get_device_name(0), 'reps': args.reps}
    for lmax, lw in ((2047, 4094), (6143, 6143), (6143, 64)):
        wl = torch.from_numpy(np.random.default_rng(1).random(lw + 1)).to(dev)
        m0 = torch.empty((lmax + 1, lmax + 1), dtype=torch.float64, device=dev)
        m1 = torch.empty_like(m0)
        for kind in (0, 1, 2):
            stream = torch.cuda.current_stream(dev).cuda_stream
            call = lambda: _lib.check(L.bfgx_pcl_coupling_device(0, C.c_void_p(stream or None), lmax, lw, kind, C.c_void_p(wl.data_ptr()),
                                                                 C.c_void_p(m0.data_ptr()), C.c_void_p(m1.data_ptr())))
            med, lo, hi = times(call, args.reps)
            key = 'kind%d_lmax%d_lw%d' % (kind, lmax, lw)
            res[key + '_ms'] = [round(med, 3), round(lo, 3), round(hi, 3)]
            res[key + '_gsteps_per_s'] = round(steps(lmax, lw, kind) / med / 1e6, 2)
        del m0, m1
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
