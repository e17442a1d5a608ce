"""GPU box: times of P(k) straight from particles (bfgx_particle_power_spectrum_device, interlace 0 and 1) on device-resident columns of
random particles with masses, next to the parts it is made of in the same run: the deposit, the shifted deposit, the cross spectrum of
the two grids and the interlaced spectrum of the two grids.  Torch events around every call, medians of the repetitions after three
warm-up calls.  The kernels' own times (the twisted store pass next to the plain one) come from a kernel trace of a short run:
   rocprofv3 --kernel-trace --stats -- python3 scripts/interlace_time.py 2
   python3 scripts/interlace_time.py [reps]   (default: 10 repetitions; 6.7e7 particles on 512^3 and 1.6e7 on 256^3)"""
import sys

import numpy as np
import torch

sys.path.insert(0, '.')
from baryonification_amd import engine          # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
dev = torch.device('cuda:0')
L, Nk = 1000.0, 180


def timed(call):
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


for n, N in ((67_000_000, 512), (16_000_000, 256)):
    torch.manual_seed(N)
    cols = torch.rand((3, n), dtype=torch.float64, device=dev) * L
    mass = torch.rand(n, dtype=torch.float64, device=dev) + 0.5
    total = float(mass.sum())
    work = torch.empty(engine.particle_power_spectrum_work_doubles(N), dtype=torch.float64, device=dev)
    map1, map2, spectra = work[:N ** 3], work[N ** 3:2 * N ** 3], work[2 * N ** 3:]
    sums = torch.zeros((4, Nk), dtype=torch.float64, device=dev)
    cnt = torch.zeros(Nk, dtype=torch.int64, device=dev)
    ptrs = (cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), mass.data_ptr())
    for name, order in (('CIC', 2), ('TSC', 3)):
        def whole(interlace):
            return lambda: engine.particle_power_spectrum_device(*ptrs, n, N, L, order, interlace, Nk, work.data_ptr(), sums[0].data_ptr(),
                                                                 sums[1].data_ptr(), sums[2].data_ptr(), cnt.data_ptr())

        def deposit(shift, out):
            return lambda: engine.deposit_cloud_device(*ptrs, n, N, L, order, out.data_ptr(), shift=shift)

        row = {'particles -> P(k), interlaced': timed(whole(1)), 'one grid': timed(whole(0)),
               'deposit': timed(deposit(0, map1)), 'shifted deposit': timed(deposit(1, map2))}
        torch.cuda.synchronize()
        assert abs(float(map1.sum()) / total - 1) < 1e-12 and abs(float(map2.sum()) / total - 1) < 1e-12      # every particle is inside
        row['cross spectrum'] = timed(lambda: engine.cross_power_spectrum_device(
            map1.data_ptr(), map2.data_ptr(), N, L, Nk, order, spectra.data_ptr(), sums[0].data_ptr(), sums[1].data_ptr(), sums[2].data_ptr(),
            sums[3].data_ptr(), cnt.data_ptr()))
        row['interlaced spectrum'] = timed(lambda: engine.interlaced_power_spectrum_device(
            map1.data_ptr(), map2.data_ptr(), N, L, Nk, order, spectra.data_ptr(), sums[0].data_ptr(), sums[1].data_ptr(), sums[2].data_ptr(),
            cnt.data_ptr()))
        row['deposit again'] = timed(deposit(0, map1))
        print('%s  n %.1e on %d^3 [ms]  ' % (name, n, N) + '   '.join('%s %.3f' % kv for kv in row.items()), flush=True)
    del cols, mass, work, map1, map2, spectra
    torch.cuda.empty_cache()
