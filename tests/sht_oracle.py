"""numpy restatement of the spherical-harmonic transforms (tests only; healpy is not installed).

Ring layout from oracle/refshim/healpy.py; per-ring F_m from np.fft.rfft with the aliasing m -> m mod n and the phase
e^{-i m phi0} written out; lambda_lm(x) from the normalised recurrence in l over ALL rings (no north/south symmetry), kept as
(value, power-of-two scale) so that lambda_mm ~ sin^m(theta) does not underflow.  Column entry points (one m at a time) make
single columns at NSIDE 1024 / 2048 cheap; the full transforms are for small nside."""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location(
    '_sht_refshim_healpy', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle', 'refshim', 'healpy.py'))
_hpshim = importlib.util.module_from_spec(_spec)                   # the refshim's ring layout, loaded under a private name
_spec.loader.exec_module(_hpshim)

UNSEEN = -1.6375e30
_SCALE = 512


def alm_size(lmax, mmax):
    return (mmax + 1) * (2 * lmax + 2 - mmax) // 2


def alm_index(lmax, l, m):
    return m * (2 * lmax + 1 - m) // 2 + l


def rings(nside):
    """start pixel, pixels, phi0 and z of the rings 1 .. 4 nside - 1"""
    start, npr, shifted, z = _hpshim._ring_layout(nside, np.arange(1, 4 * nside))
    phi0 = np.where(shifted, np.pi / npr, 0.0)
    return start, npr, phi0, z


def sin2(nside):
    """sin^2(theta) of the rings from 1 - |z|, which is exact in the polar caps (i^2 / (3 nside^2)): (1 - z)(1 + z) from the
    rounded z would lose up to 1e-9 of it next to the poles at NSIDE 2048"""
    i = np.arange(1, 4 * nside)
    j = np.minimum(i, 4 * nside - i).astype(np.float64)
    z = rings(nside)[3]
    omz = np.where(j < nside, j * j / (3.0 * nside * nside), 1.0 - np.abs(z))
    return omz * (2.0 - omz)


def lambda_column(m, lmax, z, s2=None):
    """lambda_lm(z) for l = m .. lmax (rows) and every z (columns), Condon-Shortley phase; entries below 2^-256 come out 0.
    s2 = sin^2(theta) (default (1 - z)(1 + z))"""
    z = np.asarray(z, dtype=np.float64)
    s2 = (1.0 - z) * (1.0 + z) if s2 is None else np.asarray(s2, dtype=np.float64)
    # log2 of |lambda_mm| in long double: (1/2) log2((2m+1)/(4 pi) prod (2k-1)/(2k)) + (m/2) log2(sin^2)
    ks = np.arange(1, m + 1, dtype=np.longdouble)
    lp = 0.5 * (np.log2(np.longdouble(2 * m + 1) / (4 * np.longdouble(np.pi))) + np.sum(np.log2((2 * ks - 1) / (2 * ks))))
    L2 = lp + 0.5 * m * np.log2(np.asarray(s2, dtype=np.longdouble))
    k = np.floor((L2 + 256) / _SCALE).astype(np.int64)
    v1 = np.asarray(np.exp2(L2 - _SCALE * k), dtype=np.float64) * (-1.0 if m & 1 else 1.0)
    v0 = np.zeros_like(v1)
    out = np.zeros((lmax - m + 1, z.size))
    for l in range(m, lmax + 1):
        out[l - m] = np.where(k == 0, v1, 0.0)
        lp1 = l + 1
        if lp1 > lmax:
            break
        c1 = np.sqrt((4.0 * lp1 * lp1 - 1.0) / ((lp1 - m) * (lp1 + m)))
        c2 = 0.0 if lp1 == m + 1 else c1 * np.sqrt(((l - m) * (l + m)) / (4.0 * l * l - 1.0))
        v0, v1 = v1, c1 * z * v1 - c2 * v0
        big = np.abs(v1) > 2.0 ** 256
        if big.any():
            v1 = np.where(big, v1 * 2.0 ** -_SCALE, v1)
            v0 = np.where(big, v0 * 2.0 ** -_SCALE, v0)
            k = k + big
    return out


def clean(map_):
    m = np.array(map_, dtype=np.float64)
    m[np.abs(m - UNSEEN) <= 1e-8 + 1e-5 * abs(UNSEEN)] = 0.0
    return m


def ring_F(map_, nside, ms):
    """F_m(ring) = (4 pi / Npix) e^{-i m phi0} sum_j map_j e^{-2 pi i m j / n}: array [len(ms)][4 nside - 1]"""
    start, npr, phi0, z = rings(nside)
    map_ = clean(map_)
    ms = np.asarray(ms)
    F = np.zeros((ms.size, start.size), dtype=np.complex128)
    norm = 4 * np.pi / map_.size
    for r in range(start.size):
        n = int(npr[r])
        X = np.fft.rfft(map_[start[r]:start[r] + n])
        idx = ms % n
        Xm = np.where(idx <= n // 2, X[np.minimum(idx, n // 2)], np.conj(X[np.minimum(n - idx, n // 2)]))
        F[:, r] = norm * Xm * np.exp(-1j * ms * phi0[r])
    return F


def map2alm_column(F_m, nside, lmax, m):
    """a_lm, l = m .. lmax, of one column from its F_m(ring)"""
    z = rings(nside)[3]
    return lambda_column(m, lmax, z, sin2(nside)) @ F_m


def _pixel_rings(nside):
    start, npr, phi0, z = rings(nside)
    ring = np.repeat(np.arange(start.size), npr)
    j = np.arange(12 * nside * nside) - start[ring]
    return ring, phi0[ring] + 2 * np.pi * j / npr[ring]


def synth_columns(cols, nside, lmax):
    """map of alm that are nonzero only in the given columns {m: a_lm for l = m .. lmax}"""
    z = rings(nside)[3]
    ring, phi = _pixel_rings(nside)
    out = np.zeros(12 * nside * nside)
    for m, a in cols.items():
        a = np.array(a, dtype=np.complex128)
        if m == 0:
            a = a.real.astype(np.complex128)
        G = lambda_column(m, lmax, z, sin2(nside)).T @ a
        w = 1.0 if m == 0 else 2.0
        g = G[ring]
        out += w * (g.real * np.cos(m * phi) - g.imag * np.sin(m * phi))
    return out


def _analysis(map_, nside, lmax, mmax):
    F = ring_F(map_, nside, np.arange(mmax + 1))
    alm = np.zeros(alm_size(lmax, mmax), dtype=np.complex128)
    for m in range(mmax + 1):
        i0 = alm_index(lmax, m, m)
        alm[i0:i0 + lmax - m + 1] = map2alm_column(F[m], nside, lmax, m)
    return alm


def alm2map(alm, nside, lmax, mmax):
    cols = {}
    for m in range(mmax + 1):
        i0 = alm_index(lmax, m, m)
        cols[m] = alm[i0:i0 + lmax - m + 1]
    return synth_columns(cols, nside, lmax)


def map2alm(map_, nside, lmax, mmax, iter=3):
    m = clean(map_)
    alm = _analysis(m, nside, lmax, mmax)
    for _ in range(iter):
        alm = alm + _analysis(m - alm2map(alm, nside, lmax, mmax), nside, lmax, mmax)
    return alm


def alm2cl(a, b, lmax, mmax, lmax_out=None):
    b = a if b is None else b
    lmax_out = lmax if lmax_out is None else lmax_out
    cl = np.zeros(lmax_out + 1)
    for l in range(min(lmax, lmax_out) + 1):
        s = (a[l] * np.conj(b[l])).real
        for m in range(1, min(l, mmax) + 1):
            i = alm_index(lmax, l, m)
            s += 2 * (a[i] * np.conj(b[i])).real
        cl[l] = s / (2 * l + 1)
    return cl


def anafast(map1, map2, nside, lmax, mmax, iter=3):
    a1 = map2alm(map1, nside, lmax, mmax, iter)
    a2 = None if map2 is None else map2alm(map2, nside, lmax, mmax, iter)
    return alm2cl(a1, a2, lmax, mmax), a1, a2
