"""GPU box: times of the spherical-harmonic transforms at NSIDE 1024 and 2048 (lmax = mmax = 3 nside - 1): map2alm(iter=0),
alm2map and anafast(iter=3), device-resident (engine.ShtPlan on torch tensors, device events after warm-up) and through the
one-shot host entries (numpy in / out, PCIe and workspace allocation included, wall clock).  Prints one JSON line with ms per
call and the Legendre-stage recurrence steps per transform, sum_m (lmax - m + 1) x (ring pairs = 2 nside).
    python3 scripts/anafast_time.py [reps] [nside ...]"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, '.')
from baryonification_amd import engine          # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
nsides = [int(a) for a in sys.argv[2:]] or [1024, 2048]
dev = torch.device('cuda:0')


def dev_ms(fn, n):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def wall_ms(fn, n):
    fn()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t) * 1e3 / n


out = {'what': 'spherical-harmonic transforms, fp64, lmax = mmax = 3 nside - 1', 'reps': reps, 'device': torch.cuda.get_device_name(0)}
for nside in nsides:
    lmax = mmax = 3 * nside - 1
    steps = sum(lmax - m + 1 for m in range(mmax + 1)) * 2 * nside
    rng = np.random.default_rng(1)
    mp = rng.normal(size=12 * nside * nside)
    plan = engine.sht_plan(nside, lmax, mmax)
    dm = torch.from_numpy(mp).to(dev)
    alm = plan.map2alm_device(dm, iter=0)
    omap = torch.empty_like(dm)
    cl = torch.empty(lmax + 1, dtype=torch.float64, device=dev)
    r = {'recurrence_steps_per_transform': steps, 'alm': plan.nalm,
         'work_MiB': round(plan.work.numel() * 8 / 2 ** 20, 1)}
    r['map2alm_iter0_dev_ms'] = dev_ms(lambda: plan.map2alm_device(dm, iter=0, out=alm), reps)
    r['alm2map_dev_ms'] = dev_ms(lambda: plan.alm2map_device(alm, out=omap), reps)
    r['anafast_iter3_dev_ms'] = dev_ms(lambda: plan.alm2cl_device(plan.map2alm_device(dm, iter=3, out=alm), out=cl), max(1, reps // 2))
    ah = alm.cpu().numpy()
    r['map2alm_iter0_host_ms'] = wall_ms(lambda: engine.sht_map2alm_host(mp, nside, lmax, mmax, 0), max(1, reps // 2))
    r['alm2map_host_ms'] = wall_ms(lambda: engine.sht_alm2map_host(ah, nside, lmax, mmax), max(1, reps // 2))
    r['anafast_iter3_host_ms'] = wall_ms(lambda: engine.sht_anafast_host(mp, None, nside, lmax, mmax, 3), 1)
    r['legendre_fp64_steps_per_s_map2alm_iter0'] = steps / (r['map2alm_iter0_dev_ms'] * 1e-3)
    out['nside%d' % nside] = {k: (round(v, 3) if isinstance(v, float) and v < 1e6 else v) for k, v in r.items()}
    del plan, dm, alm, omap
    engine.sphere._SHT_PLANS.clear()
    torch.cuda.empty_cache()
print(json.dumps(out))
