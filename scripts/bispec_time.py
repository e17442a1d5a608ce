"""Per-phase times of engine.bispectrum_device (device events, warm, median of 5), with the parent's power_spectrum_device and a
device-to-device copy of the fields as yardsticks.  python scripts/bispec_time.py [--n 256 512] [--once] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from baryonification_amd import engine

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, nargs='+', default=[256, 512])
ap.add_argument('--out', default=None, help='append the JSON lines to this file')
ap.add_argument('--once', action='store_true', help='one warm-up and one timed pass (for a profiler run)')
args = ap.parse_args()
dev = torch.device('cuda:0')
L = 1000.0
kf = 2 * np.pi / L
NB = 16
edges = (0.5 + 2 * np.arange(NB + 1)) * kf
tris = engine.bispectrum_triangles(edges)
eq = engine.bispectrum_triangles(edges, 'equilateral')
reps = 1 if args.once else 5


def timed(fn):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), float(min(out)), float(max(out))


for N in args.n:
    g = torch.Generator(device=dev).manual_seed(N)
    m = torch.randn((N, N, N), dtype=torch.float64, device=dev, generator=g)
    m = m + 0.3 * m * m
    pitch = engine.fft_pitch(N)
    work = torch.empty(engine.bispectrum_work_doubles(N, NB), dtype=torch.float64, device=dev)
    half = 2 * N * N * pitch
    spec, scratch, fields = work[:half], work[half:2 * half], work[2 * half:2 * half + NB * N ** 3]
    res = torch.empty(2 * len(tris) + 2 * NB, dtype=torch.float64, device=dev)
    nt = len(tris)
    outs = (res[:nt], res[nt:2 * nt], res[2 * nt:2 * nt + NB], res[2 * nt + NB:])

    def forward():
        engine.fft_slab_planes_device(m.data_ptr(), N, N, spec.data_ptr())
        engine.fft_slab_axis0_device(spec.data_ptr(), N, N, 0)

    def fields_of(unit):
        return lambda: engine.bispectrum_shell_fields_device(spec.data_ptr(), N, L, edges, unit, scratch.data_ptr(), fields.data_ptr())

    def total(t):
        return lambda: engine.bispectrum_device(m.data_ptr(), N, L, edges, t, work.data_ptr(), *[o.data_ptr() for o in outs])

    pw = torch.empty(engine.power_spectrum_work_doubles(N), dtype=torch.float64, device=dev)
    pk, ks = torch.empty(180, dtype=torch.float64, device=dev), torch.empty(180, dtype=torch.float64, device=dev)
    cnt = torch.empty(180, dtype=torch.int64, device=dev)
    copy_dst = torch.empty_like(fields)
    r = {'N': N, 'nbins': NB, 'ntri': int(nt), 'reps': reps}
    r['forward_ms'] = timed(forward)
    r['fields_data_ms'] = timed(fields_of(0))
    r['fields_unit_ms'] = timed(fields_of(1))
    r['total_all_ms'] = timed(total(tris))
    r['total_equilateral_ms'] = timed(total(eq))
    r['power_spectrum_ms'] = timed(lambda: engine.power_spectrum_device(m.data_ptr(), N, L, 180, pw.data_ptr(), pk.data_ptr(), ks.data_ptr(), cnt.data_ptr()))
    r['copy_fields_ms'] = timed(lambda: copy_dst.copy_(fields))
    tr = r['forward_ms'][0] + r['fields_data_ms'][0] + r['fields_unit_ms'][0]
    r['sweeps_all_ms'] = r['total_all_ms'][0] - tr
    r['sweeps_equilateral_ms'] = r['total_equilateral_ms'][0] - tr
    r['transforms_over_pk'] = tr / r['power_spectrum_ms'][0]
    r['one_sweep_over_copy'] = 0.5 * r['sweeps_all_ms'] / r['copy_fields_ms'][0]
    print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write(json.dumps(r) + '\n')
    del m, work, res, pw, copy_dst
    torch.cuda.empty_cache()
