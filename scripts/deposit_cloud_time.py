"""GPU box: times of the CIC / TSC particle deposit (bfgx_deposit_cloud_device) on device-resident columns of random particles, both forms
(BFGX_DEPOSIT=tiled / atomic), next to the NGP deposit in the same run: torch events around every call, medians of the repetitions after
three warm-up calls.  Then the two forms at smaller particle counts on the smaller grid: where their curves cross is where the default
switch belongs.  The kernels' own times (the fold alone, the tile kernel, the sort passes) come from a kernel trace of a short run:
   rocprofv3 --kernel-trace --stats -- python3 scripts/deposit_cloud_time.py 2 --no-sweep
   python3 scripts/deposit_cloud_time.py [reps] [--no-sweep]   (default: 10 repetitions; 6.7e7 particles on 512^3 and 1.6e7 on 256^3)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, '.')
from baryonification_amd import engine          # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith('--')]
reps = int(args[0]) if args else 10
sweep = '--no-sweep' not in sys.argv
dev = torch.device('cuda:0')
L = 1000.0


def timed(call, form):
    os.environ['BFGX_DEPOSIT'] = form
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def columns(n, seed):
    torch.manual_seed(seed)
    cols = torch.rand((3, n), dtype=torch.float64, device=dev) * L
    mass = torch.rand(n, dtype=torch.float64, device=dev) + 0.5
    return cols, mass


def cloud(cols, mass, n, N, order, out):
    return lambda: engine.deposit_cloud_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), mass.data_ptr(), n, N, L, order,
                                               out.data_ptr())


for n, N in ((67_000_000, 512), (16_000_000, 256)):
    cols, mass = columns(n, N)
    edges = torch.linspace(0.0, L, N + 1, dtype=torch.float64, device=dev)
    out = torch.empty(N ** 3, dtype=torch.float64, device=dev)
    ngp = lambda: engine.deposit_particles_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), mass.data_ptr(), n, N,       # noqa: E731
                                                  edges.data_ptr(), out.data_ptr())
    row = {'NGP tiled': timed(ngp, 'tiled'), 'NGP atomic': timed(ngp, 'atomic')}
    total = float(mass.sum())
    for name, order in (('CIC', 2), ('TSC', 3)):
        for form in ('tiled', 'atomic'):
            row['%s %s' % (name, form)] = timed(cloud(cols, mass, n, N, order, out), form)
            torch.cuda.synchronize()
            assert abs(float(out.sum()) / total - 1) < 1e-12          # every particle is inside: the map holds the whole mass
    row['NGP tiled again'] = timed(ngp, 'tiled')
    print('n %.1e on %d^3 [ms]  ' % (n, N) + '   '.join('%s %.3f' % kv for kv in row.items()), flush=True)
    del cols, mass, out
    torch.cuda.empty_cache()

if sweep:
    N = 256
    out = torch.empty(N ** 3, dtype=torch.float64, device=dev)
    for lg in (14, 16, 17, 18, 19, 20, 22):
        n = 1 << lg
        cols, mass = columns(n, lg)
        row = {}
        for name, order in (('CIC', 2), ('TSC', 3)):
            for form in ('tiled', 'atomic'):
                row['%s %s' % (name, form)] = timed(cloud(cols, mass, n, N, order, out), form)
        print('n 2^%d on %d^3 [ms]  ' % (lg, N) + '   '.join('%s %.3f' % kv for kv in row.items()), flush=True)
os.environ.pop('BFGX_DEPOSIT', None)
