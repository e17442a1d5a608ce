"""numpy restatement of the spin-weighted transforms (tests only; healpy is not installed).

Convention (HEALPix/libsharp): map0 + i map1 = -sum_{l >= s} sum_{m = -l..l} (G_lm + i C_lm) sY_lm, G and C the coefficients of
real fields, sY_lm = sqrt((l - s)! / (l + s)!) edth^s Y_lm.  For m >= 0 two columns are used:
    lam+_lm = sY_lm(theta, 0),   lam-_lm = (-1)^m sY_{l,-m}(theta, 0),
so that G + i C = -sum lam+ (F0 + i F1) and G - i C = -sum lam- (F0 - i F1) over rings (F0, F1 the per-ring Fourier
coefficients of map0 and map1, from sht_oracle.ring_F), and the synthesis is the transpose.

The columns are computed over ALL rings (no north/south symmetry) from a start value at l0 = max(m, s) taken in log space
(log2 of sqrt((2 l0 + 1) / (4 pi) binom(2 l0, m + s)) cos^a(theta/2) sin^b(theta/2) in long double), then the normalised
three-term Wigner-d recurrence in l, kept as (value, power-of-two scale) per column so that nothing underflows."""
import numpy as np

import sht_oracle as O

_SCALE = 512


def _half_angles2(z, s2):
    """cos^2(theta/2), sin^2(theta/2) in long double, the smaller of the two from sin^2(theta) (exact next to the poles)"""
    z = np.asarray(z, dtype=np.longdouble)
    s2 = np.asarray(s2, dtype=np.longdouble)
    c2, h2 = (1 + z) / 2, (1 - z) / 2
    c2 = np.where(z < 0, s2 / (4 * h2), c2)
    h2 = np.where(z >= 0, s2 / (4 * c2), h2)
    return c2, h2


def spin_columns(m, s, lmax, z, s2=None):
    """(lam+, lam-): arrays [lmax - m + 1][len(z)] for l = m .. lmax (rows with l < max(m, s) are 0); entries below 2^-256 are 0"""
    z = np.asarray(z, dtype=np.float64)
    s2 = (1.0 - z) * (1.0 + z) if s2 is None else np.asarray(s2, dtype=np.float64)
    l0 = max(m, s)
    c2, h2 = _half_angles2(z, s2)
    i = np.arange(1, abs(m - s) + 1, dtype=np.longdouble)
    lbin = np.sum(np.log2((m + s + i) / i))                     # log2 binom(2 l0, m + s)
    lp = 0.5 * (np.log2(np.longdouble(2 * l0 + 1) / (4 * np.longdouble(np.pi))) + lbin)
    cols = []
    for a, b, sign in ((abs(m - s), m + s, -1.0 if m & 1 else 1.0),
                       (m + s, abs(m - s), -1.0 if (m >= s and (m + s) & 1) else 1.0)):
        L2 = lp + 0.5 * (a * np.log2(c2) + b * np.log2(h2))
        k = np.floor((L2 + 256) / _SCALE).astype(np.int64)
        v1 = np.asarray(np.exp2(L2 - _SCALE * k), dtype=np.float64) * sign
        cols.append([v1, np.zeros_like(v1), k])
    out = [np.zeros((lmax - m + 1, z.size)), np.zeros((lmax - m + 1, z.size))]
    for l in range(l0, lmax + 1):
        for c, (v1, v0, k) in enumerate(cols):
            out[c][l - m] = np.where(k == 0, v1, 0.0)
        L = l + 1
        if L > lmax:
            break
        den = float(L * L - m * m) * float(L * L - s * s)
        a = L * np.sqrt((2.0 * L + 1) * (2.0 * L - 1) / den)
        b = m * s / (L * (L - 1.0))
        cc = (L / (L - 1.0)) * np.sqrt((2.0 * L + 1) / (2.0 * L - 3) * (float((L - 1) ** 2 - m * m) * float((L - 1) ** 2 - s * s)) / den)
        for c, sg in ((0, 1.0), (1, -1.0)):
            v1, v0, k = cols[c]
            v0, v1 = v1, a * (z + sg * b) * v1 - cc * v0
            big = np.abs(v1) > 2.0 ** 256
            if big.any():
                v1 = np.where(big, v1 * 2.0 ** -_SCALE, v1)
                v0 = np.where(big, v0 * 2.0 ** -_SCALE, v0)
                k = k + big
            cols[c] = [v1, v0, k]
    return out[0], out[1]


def sY(l, m, s, theta):
    """sY_lm(theta, 0) for any m (a check of the columns against other definitions)"""
    th = np.atleast_1d(np.asarray(theta, dtype=np.float64))
    z = np.cos(th)
    lp, lm = spin_columns(abs(m), s, l, z, np.sin(th) ** 2)
    return lp[l - m] if m >= 0 else (-1.0) ** (-m) * lm[l + m]


def map2alm_spin_column(F0_m, F1_m, nside, s, lmax, m):
    """(G, C) for l = m .. lmax of one column from F0_m, F1_m per ring"""
    z = O.rings(nside)[3]
    lp, lm = spin_columns(m, s, lmax, z, O.sin2(nside))
    Ap, Am = lp @ (F0_m + 1j * F1_m), lm @ (F0_m - 1j * F1_m)
    return -(Ap + Am) / 2, 0.5j * (Ap - Am)


def map2alm_spin(maps, nside, s, lmax, mmax):
    """[G, C] of a pair of maps (plain quadrature)"""
    ms = np.arange(mmax + 1)
    F0, F1 = O.ring_F(maps[0], nside, ms), O.ring_F(maps[1], nside, ms)
    G = np.zeros(O.alm_size(lmax, mmax), dtype=np.complex128)
    C = np.zeros_like(G)
    for m in ms:
        i0 = O.alm_index(lmax, m, m)
        G[i0:i0 + lmax - m + 1], C[i0:i0 + lmax - m + 1] = map2alm_spin_column(F0[m], F1[m], nside, s, lmax, m)
    return np.array([G, C])


def synth_spin_columns(colsG, colsC, nside, s, lmax):
    """[map0, map1] of G, C that are nonzero only in the given columns {m: values for l = m .. lmax}"""
    z = O.rings(nside)[3]
    ring, phi = O._pixel_rings(nside)
    out = np.zeros((2, 12 * nside * nside))
    for m in colsG:
        g = np.array(colsG[m], dtype=np.complex128)
        c = np.array(colsC[m], dtype=np.complex128)
        if m == 0:
            g, c = g.real.astype(np.complex128), c.real.astype(np.complex128)
        lp, lm = spin_columns(m, s, lmax, z, O.sin2(nside))
        Qp, Qm = lp.T @ (g + 1j * c), lm.T @ (g - 1j * c)
        F = [-(Qp + Qm) / 2, 0.5j * (Qp - Qm)]
        w = 1.0 if m == 0 else 2.0
        cs, sn = np.cos(m * phi), np.sin(m * phi)
        for k in range(2):
            f = F[k][ring]
            out[k] += w * (f.real * cs - f.imag * sn)
    return out


def alm2map_spin(alms, nside, s, lmax, mmax):
    colsG, colsC = {}, {}
    for m in range(mmax + 1):
        i0 = O.alm_index(lmax, m, m)
        colsG[m], colsC[m] = alms[0][i0:i0 + lmax - m + 1], alms[1][i0:i0 + lmax - m + 1]
    return synth_spin_columns(colsG, colsC, nside, s, lmax)
