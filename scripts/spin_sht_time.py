"""GPU box: times of the spin-weighted transforms at NSIDE 1024 and 2048 (lmax = mmax = 3 nside - 1, spin 2), next to the spin-0
map2alm of the same plan: map2alm_spin and alm2map_spin device-resident (engine.ShtPlan on torch tensors, device events after
warm-up) and through the one-shot host entries (numpy in / out, PCIe and workspace allocation included, wall clock).  Prints one
JSON line with ms per call and the spin Legendre-stage recurrence steps per transform, sum_m (lmax - max(m, s) + 1) x 2 nside.
    python3 scripts/spin_sht_time.py [reps] [nside ...]"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, '.')
from baryonification_amd import engine          # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
nsides = [int(a) for a in sys.argv[2:]] or [1024, 2048]
spin = 2
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


out = {'what': 'spin-%d transforms, fp64, lmax = mmax = 3 nside - 1' % spin, 'reps': reps, 'device': torch.cuda.get_device_name(0)}
for nside in nsides:
    lmax = mmax = 3 * nside - 1
    steps = sum(lmax - max(m, spin) + 1 for m in range(mmax + 1)) * 2 * nside
    rng = np.random.default_rng(1)
    maps = rng.normal(size=(2, 12 * nside * nside))
    plan = engine.sht_plan(nside, lmax, mmax)
    dm = torch.from_numpy(maps).to(dev)
    alms = plan.map2alm_spin_device(dm, spin)
    omaps = torch.empty_like(dm)
    alm0 = torch.empty(plan.nalm, dtype=torch.complex128, device=dev)
    r = {'recurrence_steps_per_transform': steps, 'alm': plan.nalm,
         'work_MiB': round(plan.work.numel() * 8 / 2 ** 20, 1), 'spin_work_MiB': round(plan.spin_work.numel() * 8 / 2 ** 20, 1)}
    r['map2alm_spin0_iter0_dev_ms'] = dev_ms(lambda: plan.map2alm_device(dm[0], iter=0, out=alm0), reps)
    r['map2alm_spin_dev_ms'] = dev_ms(lambda: plan.map2alm_spin_device(dm, spin, out=alms), reps)
    r['alm2map_spin_dev_ms'] = dev_ms(lambda: plan.alm2map_spin_device(alms, spin, out=omaps), reps)
    ah = alms.cpu().numpy()
    r['map2alm_spin_host_ms'] = wall_ms(lambda: engine.sht_map2alm_spin_host(maps, nside, lmax, mmax, spin), max(1, reps // 2))
    r['alm2map_spin_host_ms'] = wall_ms(lambda: engine.sht_alm2map_spin_host(ah, nside, lmax, mmax, spin), max(1, reps // 2))
    r['spin_over_spin0_map2alm'] = r['map2alm_spin_dev_ms'] / r['map2alm_spin0_iter0_dev_ms']
    r['legendre_fp64_steps_per_s_map2alm_spin'] = steps / (r['map2alm_spin_dev_ms'] * 1e-3)
    out['nside%d' % nside] = {k: (round(v, 3) if isinstance(v, float) and v < 1e6 else v) for k, v in r.items()}
    del plan, dm, alms, omaps, alm0
    engine.sphere._SHT_PLANS.clear()
    torch.cuda.empty_cache()
print(json.dumps(out))
