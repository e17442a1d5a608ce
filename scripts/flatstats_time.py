"""GPU box: times of the flat-patch statistics of baryonification_amd.utils (derivatives_2d, peak_counts_2d, minkowski_functionals_2d,
patch_statistics with 4 scales) on resident N^2 float64 maps (torch events around the calls), each next to the same operation written
with torch in the same run: torch.fft with precomputed factors, max_pool2d on a circularly padded map plus bincount, elementwise torch for
the Minkowski terms.  The twins get their multipliers, beams and edges precomputed outside the timed window; the library computes them
per mode in every call.  Library and twin are taken in turn, twice each; the ratio is that of the lower figures.
   python3 scripts/flatstats_time.py [reps] [N ...]   (default: 20 repetitions, N = 1024, 2048 and 4096)"""
import sys
import numpy as np
import torch

sys.path.insert(0, '.')
from baryonification_amd import utils as U          # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
sizes = [int(a) for a in sys.argv[2:]] or [1024, 2048, 4096]
dev = torch.device('cuda:0')
NB_PEAKS, NB_MF = 18, 12


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
    torch.manual_seed(13 + N)
    L = 0.7 * N
    x = torch.randn((N, N), dtype=torch.float64, device=dev)
    sigma = 3.0 * L / N
    fwhm = sigma * np.sqrt(8 * np.log(2))
    scales = [0.0, fwhm, 2 * fwhm, 4 * fwhm]
    pe = torch.linspace(-4.0, 4.0, NB_PEAKS + 1, dtype=torch.float64, device=dev)
    me = torch.linspace(-0.05, 0.05, NB_MF + 1, dtype=torch.float64, device=dev)
    # what the twins need, precomputed
    h = N // 2
    g0 = (2 * np.pi / L) * torch.fft.fftfreq(N, d=1.0 / N, device=dev, dtype=torch.float64)[:, None]
    g1 = (2 * np.pi / L) * torch.arange(h + 1, device=dev, dtype=torch.float64)[None, :]
    o0, o1 = g0.clone(), g1.clone()
    o0[h] = 0
    o1[:, h] = 0
    kk = torch.sqrt(g0 ** 2 + g1 ** 2)
    beams = [torch.exp(-0.5 * (kk * (s / np.sqrt(8 * np.log(2)))) ** 2) for s in scales]
    spin = [torch.ones_like(kk) + 0j, 1j * o0 * torch.ones_like(kk), 1j * o1 * torch.ones_like(kk), -(g0 ** 2 + g1 ** 2) + 0j,
            -(g0 ** 2 - g1 ** 2) + 0j, -2 * o0 * o1 + 0j]
    mults = [[m * b for m in spin] for b in beams]                     # per scale: the six multipliers times the beam
    mult = mults[1]

    def t_der(F=None, mm=mult):
        F = torch.fft.rfft2(x) if F is None else F
        return [torch.fft.irfft2(F * m, s=(N, N)) for m in mm]

    def t_peaks(u=x):
        p = torch.nn.functional.pad(u[None, None], (1, 1, 1, 1), mode='circular')
        top = torch.nn.functional.max_pool2d(p, 3, stride=1)[0, 0]
        bot = -torch.nn.functional.max_pool2d(-p, 3, stride=1)[0, 0]
        out = []
        for v in (u[u == top], u[u == bot]):
            b = torch.bucketize(v, pe, right=True) - 1
            out.append(torch.bincount(b[(b >= 0) & (b < NB_PEAKS)], minlength=NB_PEAKS))
        return out

    def t_mf_terms(d):
        u, ux, uy, lap, qp, qc = d
        a2, b2 = ux * ux, uy * uy
        g2 = a2 + b2
        c = ux * uy * qc - 0.5 * lap * g2 + 0.5 * qp * (a2 - b2)
        b = (torch.bucketize(u, me, right=True) - 1).reshape(-1)
        ok = (b >= 0) & (b < NB_MF)
        t1, t2 = torch.sqrt(g2).reshape(-1), torch.where(g2 > 0, c / g2, torch.zeros_like(c)).reshape(-1)
        return (torch.bincount(b[ok], minlength=NB_MF), torch.bincount(b[ok], weights=t1[ok], minlength=NB_MF),
                torch.bincount(b[ok], weights=t2[ok], minlength=NB_MF))

    def t_moments(u):
        d = u - u.mean()
        d2 = d * d
        return d2.mean(), (d2 * d).mean(), (d2 * d2).mean()

    def t_patch():
        F = torch.fft.rfft2(x)
        out = []
        for mm in mults:
            d = t_der(F, mm)
            out.append((t_moments(d[0]), t_peaks(d[0]), t_mf_terms(d)))
        return out

    rows = [
        ('derivatives_2d', lambda: U.derivatives_2d(x, L, sigma=sigma, spin_form=True), t_der),
        ('peak_counts_2d', lambda: U.peak_counts_2d(x, pe), t_peaks),
        ('minkowski_functionals_2d', lambda: U.minkowski_functionals_2d(x, L, me, sigma=sigma), lambda: t_mf_terms(t_der())),
        ('patch_statistics, 4 scales', lambda: U.patch_statistics(x, L, scales, peak_bins=pe, mf_bins=me), t_patch),
    ]
    # the two sides compute the same thing
    d, r = U.derivatives_2d(x, L, sigma=sigma, spin_form=True), t_der()
    pk, rp = U.peak_counts_2d(x, pe), t_peaks()
    mf, rm = U.minkowski_functionals_2d(x, L, me, sigma=sigma), t_mf_terms(r)
    print("N %d: library against torch: derivatives max difference %.1e of the map's maximum; peaks differ in %d bins; Minkowski counts differ "
          "in %d bins" % (N, max(float((d[a] - r[a]).abs().max() / r[a].abs().max()) for a in range(6)),
                          int((pk['maxima'] != rp[0]).sum() + (pk['minima'] != rp[1]).sum()), int((mf['count'] != rm[0]).sum())))
    for name, lib, twin in rows:
        a = timed(lib)
        t = timed(twin)
        b = timed(lib)
        t2 = timed(twin)
        print("N %4d  %-28s library %8.4f ms (again %8.4f ms)   torch %8.4f ms (again %8.4f ms)   library / torch %.2f" %
              (N, name, a, b, t, t2, min(a, b) / min(t, t2)))
    del x, kk, beams, spin, mult, mults, d, r
    torch.cuda.empty_cache()
