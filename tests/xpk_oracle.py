"""Plain-numpy references for the cross power spectrum of two gridded 3-D maps (no GPU, nothing of the library).

  window_weight             t[i] = s(n_i)^(-2p), s(n) = sin(pi n / N) / (pi n / N), in long double
  axis0_xpk_ref             what the cross form of the binned axis-0 pass must deliver for a block of columns: per linear k-bin the sums of
                            w m |F_A|^2, w m |F_B|^2, w m Re(F_A conj F_B), of m |k| and the counts m (bins as fft_oracle.mode_k_and_bin)
  cross_power_spectrum_ref  the public entry's answer on the full cube through np.fft.fftn, bins as oracle/grid.py:power_spectrum

The per-bin sums are added up in long double, as fft_oracle._bin_sums does."""
import numpy as np

import fft_oracle as O


def window_weight(N, p):
    """t[i] = s(n_i)^(-2p) for the integer wave numbers n = fftfreq(N) N, in np.longdouble (p = 0: exactly 1)"""
    n = np.rint(np.fft.fftfreq(N) * N).astype(np.int64)
    x = 4 * np.arctan(np.longdouble(1)) * n.astype(np.longdouble) / np.longdouble(N)
    s = np.ones(N, dtype=np.longdouble)
    nz = n != 0
    s[nz] = np.sin(x[nz]) / x[nz]
    return s ** (-2 * int(p))


def _sums_ld(bins, values, nk):
    """sum of the long-double `values` per bin (bins already masked to [0, nk)), rounded to fp64 once at the end"""
    out = np.zeros(nk)
    if bins.size:
        order = np.argsort(bins, kind='stable')
        sb = bins[order]
        starts = np.flatnonzero(np.r_[True, sb[1:] != sb[:-1]])
        out[sb[starts]] = np.add.reduceat(values[order].astype(np.longdouble), starts).astype(np.float64)
    return out


def axis0_xpk_ref(spec_a, work_b, N, col0, L, nk, p):
    """spec_a[N][ncols][nz] = map A's finished spectrum of the columns b = col0 .. of the middle axis, work_b[N][ncols][nz] = map B's before
    the transform along axis 0 (nz = N/2 + 1).  Returns (paa_sum, pbb_sum, pab_sum, k_sum, counts) per linear k-bin over exactly these
    columns; a mode with 0 < c < N/2 counts twice (its mirror image), the window weight multiplies the three power sums only."""
    spec_a, work_b = np.asarray(spec_a), np.asarray(work_b)
    ncols, nz = work_b.shape[1], work_b.shape[2]
    assert spec_a.shape == work_b.shape and work_b.shape[0] == N and nz == N // 2 + 1 and 0 <= col0 and col0 + ncols <= N
    FB = np.fft.fft(work_b, axis=0)
    a = np.arange(N)[:, None, None]
    b = (col0 + np.arange(ncols))[None, :, None]
    c = np.arange(nz)[None, None, :]
    k, kinds = O.mode_k_and_bin(N, L, nk, a, b, c)
    m = np.broadcast_to(np.where((c > 0) & (c < N // 2), 2, 1), k.shape)
    t = window_weight(N, p)
    w = m * (t[a] * t[b] * t[c])                                           # long double
    ok = (kinds >= 0) & (kinds < nk)
    sel = kinds[ok]
    ld = np.longdouble
    fa_r, fa_i, fb_r, fb_i = spec_a.real.astype(ld), spec_a.imag.astype(ld), FB.real.astype(ld), FB.imag.astype(ld)
    paa = _sums_ld(sel, (w * (fa_r ** 2 + fa_i ** 2))[ok], nk)
    pbb = _sums_ld(sel, (w * (fb_r ** 2 + fb_i ** 2))[ok], nk)
    pab = _sums_ld(sel, (w * (fa_r * fb_r + fa_i * fb_i))[ok], nk)
    ks = _sums_ld(sel, (m * k)[ok].astype(ld), nk)
    counts = np.bincount(sel, weights=m[ok], minlength=nk).astype(np.int64)
    return paa, pbb, pab, ks, counts


def binned_cube(FA, FB, L, nk, p):
    """{'k', 'paa', 'pbb', 'pab', 'r', 'counts'} from the full spectra FA, FB [N][N][N] (any complex dtype): per linear k-bin the means of
    w |F_A|^2, w |F_B|^2, w Re(F_A conj F_B) and of |k| over all modes of the cube, NaN for empty bins"""
    N = FA.shape[0]
    i = np.arange(N)
    a, b, c = i[:, None, None], i[None, :, None], i[None, None, :]
    k, kinds = O.mode_k_and_bin(N, L, nk, a, b, c)
    t = window_weight(N, p)
    w = t[a] * t[b] * t[c]
    ok = (kinds >= 0) & (kinds < nk)
    sel = kinds[ok]
    counts = np.bincount(sel, minlength=nk).astype(np.int64)
    ld = np.longdouble
    fa_r, fa_i, fb_r, fb_i = FA.real.astype(ld), FA.imag.astype(ld), FB.real.astype(ld), FB.imag.astype(ld)
    with np.errstate(divide='ignore', invalid='ignore'):
        paa = _sums_ld(sel, (w * (fa_r ** 2 + fa_i ** 2))[ok], nk) / counts
        pbb = _sums_ld(sel, (w * (fb_r ** 2 + fb_i ** 2))[ok], nk) / counts
        pab = _sums_ld(sel, (w * (fa_r * fb_r + fa_i * fb_i))[ok], nk) / counts
        kc = _sums_ld(sel, k[ok].astype(ld), nk) / counts
        r = pab / np.sqrt(paa * pbb)
    return {'k': kc, 'paa': paa, 'pbb': pbb, 'pab': pab, 'r': r, 'counts': counts}


def cross_power_spectrum_ref(A, B, L, nk, p=0):
    """engine.cross_power_spectrum(A, B, L, nk, p) by np.fft.fftn on the full cube"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    assert A.ndim == 3 and len(set(A.shape)) == 1 and A.shape == B.shape
    return binned_cube(np.fft.fftn(A), np.fft.fftn(B), L, nk, p)
