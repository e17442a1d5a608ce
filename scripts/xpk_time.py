"""GPU box: time of bfgx_cross_power_spectrum_device on two resident N^3 maps (torch events around the call), next to two calls of
bfgx_power_spectrum_device on the same maps in the same run, and a check of the three binned sums against a torch.fft restatement.
   python3 scripts/xpk_time.py [reps] [N ...]   (default: 20 repetitions, N = 256 and 512)"""
import sys
import numpy as np
import torch

sys.path.insert(0, '.')
from baryonification_amd import engine          # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
sizes = [int(a) for a in sys.argv[2:]] or [256, 512]
Nk, L = 180, 1000.0
dev = torch.device('cuda:0')


def timed(call):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


for N in sizes:
    torch.manual_seed(5 + N)
    ma = torch.rand(N ** 3, dtype=torch.float64, device=dev)
    mb = 0.7 * ma + 0.3 * torch.rand(N ** 3, dtype=torch.float64, device=dev)
    work = torch.empty(engine.cross_power_spectrum_work_doubles(N), dtype=torch.float64, device=dev)
    sums = torch.zeros((4, Nk), dtype=torch.float64, device=dev)
    cnt = torch.zeros(Nk, dtype=torch.int64, device=dev)
    pk2, cnt2 = torch.zeros((4, Nk), dtype=torch.float64, device=dev), torch.zeros((2, Nk), dtype=torch.int64, device=dev)

    def cross(p=0):
        engine.cross_power_spectrum_device(ma.data_ptr(), mb.data_ptr(), N, L, Nk, p, work.data_ptr(), sums[0].data_ptr(), sums[1].data_ptr(),
                                           sums[2].data_ptr(), sums[3].data_ptr(), cnt.data_ptr(), 0, 0)

    def two_autos():
        engine.power_spectrum_device(ma.data_ptr(), N, L, Nk, work.data_ptr(), pk2[0].data_ptr(), pk2[1].data_ptr(), cnt2[0].data_ptr(), 0, 0)
        engine.power_spectrum_device(mb.data_ptr(), N, L, Nk, work.data_ptr(), pk2[2].data_ptr(), pk2[3].data_ptr(), cnt2[1].data_ptr(), 0, 0)

    ms_autos = timed(two_autos)
    ms_cross = timed(cross)
    ms_cic = timed(lambda: cross(2))
    ms_autos_again = timed(two_autos)
    cross()
    torch.cuda.synchronize()
    got = sums.cpu().numpy()
    # restatement: rfftn of both maps, the mirrored half weighted 2, linear bins between the fundamental and Nyquist; only the sums over
    # all bins are compared (modes on a bin edge may fall either side in the restatement)
    FA, FB = torch.fft.rfftn(ma.view(N, N, N)), torch.fft.rfftn(mb.view(N, N, N))
    kl = torch.fft.fftfreq(N, d=L / N, device=dev, dtype=torch.float64) * 2 * np.pi
    kz = kl[:N // 2 + 1].abs()
    kz[-1] = abs(float(kl[N // 2]))
    kk = torch.sqrt(kl[:, None, None] ** 2 + kl[None, :, None] ** 2 + kz[None, None, :] ** 2)
    w = torch.full((N // 2 + 1,), 2.0, dtype=torch.float64, device=dev)
    w[0] = 1.0
    w[-1] = 1.0
    ok = (kk >= 2 * np.pi / L) & (kk < np.pi * N / L)
    ref = [float(((q * w[None, None, :])[ok]).sum()) for q in (FA.real ** 2 + FA.imag ** 2, FB.real ** 2 + FB.imag ** 2, FA.real * FB.real + FA.imag * FB.imag)]
    auto = pk2.cpu().numpy()
    print("N %d  cross %.4f ms  (CIC window %.4f ms)   two autos %.4f ms (again %.4f ms)   cross / two autos %.3f   total aa, bb, ab rel diff "
          "%.1e %.1e %.1e   paa, pbb against the autos %.1e %.1e" %
          (N, ms_cross, ms_cic, ms_autos, ms_autos_again, ms_cross / min(ms_autos, ms_autos_again), abs(got[0].sum() / ref[0] - 1), abs(got[1].sum() / ref[1] - 1),
           abs(got[2].sum() / ref[2] - 1), np.abs(got[0] / auto[0] - 1).max(), np.abs(got[1] / auto[2] - 1).max()))
    del ma, mb, work, FA, FB, kk
    torch.cuda.empty_cache()
