"""GPU box: times of the flat-sky functions of baryonification_amd.utils on resident N^2 float64 maps (torch events around the calls), each
next to the same operation written with torch.fft.rfft2 / irfft2 and torch elementwise operations in the same run.  The torch twins get
their k-bin indices, mirror weights, beams and Kaiser-Squires factors precomputed outside the timed window; the library computes them
per mode in every call.  Each library figure is taken twice, before and after its twin.
   python3 scripts/fft2d_time.py [reps] [N ...]   (default: 20 repetitions, N = 1024, 2048 and 4096)"""
import sys
import numpy as np
import torch

sys.path.insert(0, '.')
from baryonification_amd import utils as U          # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
sizes = [int(a) for a in sys.argv[2:]] or [1024, 2048, 4096]
Nk = 180
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
    torch.manual_seed(11 + N)
    L = 0.7 * N
    x = torch.randn((N, N), dtype=torch.float64, device=dev)
    y = torch.randn((N, N), dtype=torch.float64, device=dev)
    sigma = 3.0 * L / N
    # what the twins need, precomputed
    n0 = torch.fft.fftfreq(N, d=1.0 / N, device=dev, dtype=torch.float64)
    n1 = torch.arange(N // 2 + 1, device=dev, dtype=torch.float64)
    d2 = n0[:, None] ** 2 + n1[None, :] ** 2
    kk = 2 * np.pi / L * torch.sqrt(d2)
    k0, dk = 2 * np.pi / L, (np.pi * N / L - 2 * np.pi / L) / Nk
    bins = torch.floor((kk - k0) / dk).to(torch.int64)
    inside = ((bins >= 0) & (bins < Nk)).reshape(-1)
    idx = bins.reshape(-1)[inside]
    w = torch.full((N // 2 + 1,), 2.0, dtype=torch.float64, device=dev)
    w[0] = w[-1] = 1.0
    wk = (w[None, :] * torch.ones_like(kk)).reshape(-1)[inside]
    beam = torch.exp(-0.5 * (kk * sigma) ** 2)
    safe = torch.where(d2 > 0, d2, torch.ones_like(d2))
    c2 = torch.where(d2 > 0, (n0[:, None] ** 2 - n1[None, :] ** 2) / safe, torch.zeros_like(d2))
    s2 = torch.where(d2 > 0, 2 * n0[:, None] * n1[None, :] / safe, torch.zeros_like(d2))
    s2[N // 2, :] = 0
    s2[:, N // 2] = 0

    def t_pk():
        F = torch.fft.rfft2(x)
        p = (F.real ** 2 + F.imag ** 2).reshape(-1)[inside] * wk
        return (torch.bincount(idx, weights=p, minlength=Nk) / torch.bincount(idx, weights=wk, minlength=Nk)).cpu()

    def t_ks():
        F = torch.fft.rfft2(x)
        return torch.fft.irfft2(c2 * F, s=(N, N)), torch.fft.irfft2(s2 * F, s=(N, N))

    def t_eb():
        F1, F2 = torch.fft.rfft2(x), torch.fft.rfft2(y)
        return torch.fft.irfft2(c2 * F1 + s2 * F2, s=(N, N)), torch.fft.irfft2(c2 * F2 - s2 * F1, s=(N, N))

    rows = [
        ('rfft2', lambda: U.rfft2(x), lambda: torch.fft.rfft2(x)),
        ('irfft2(rfft2)', lambda: U.irfft2(U.rfft2(x), N), lambda: torch.fft.irfft2(torch.fft.rfft2(x), s=(N, N))),
        ('power_spectrum_2d', lambda: U.power_spectrum_2d(x, L, Nk), t_pk),
        ('smoothing_2d', lambda: U.smoothing_2d(x, L, sigma=sigma), lambda: torch.fft.irfft2(torch.fft.rfft2(x) * beam, s=(N, N))),
        ('kappa_to_shear_2d', lambda: U.kappa_to_shear_2d(x), t_ks),
        ('shear_to_kappa_2d', lambda: U.shear_to_kappa_2d(x, y), t_eb),
    ]
    # the two sides compute the same thing
    g1, g2 = U.kappa_to_shear_2d(x)
    r1, r2 = t_ks()
    sm, rs = U.smoothing_2d(x, L, sigma=sigma), torch.fft.irfft2(torch.fft.rfft2(x) * beam, s=(N, N))
    pk, rp = U.power_spectrum_2d(x, L, Nk)['pk'], t_pk().numpy()
    print("N %d: library against torch, max differences: shear %.1e  smoothing %.1e  P(k) %.1e (relative)" %
          (N, max(float((g1 - r1).abs().max()), float((g2 - r2).abs().max())), float((sm - rs).abs().max()), float(np.nanmax(np.abs(pk / rp - 1)))))
    for name, lib, twin in rows:
        a = timed(lib)
        t = timed(twin)
        b = timed(lib)
        print("N %4d  %-18s library %8.4f ms (again %8.4f ms)   torch %8.4f ms   library / torch %.2f" % (N, name, a, b, t, min(a, b) / t))
    del x, y, kk, bins, beam, c2, s2, d2, safe
    torch.cuda.empty_cache()
