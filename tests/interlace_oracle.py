"""Plain-numpy oracle of the interlaced CIC / TSC grids and of P(k) straight from particles (no GPU, nothing of the library), built on
deposit_cloud_oracle.py and xpk_oracle.py as they stand.

The shifted grid.  Grid 2 is grid 1 with every particle moved by +L / (2N) along every axis, periodically, defined in cell units so that
fp64 follows it bit for bit.  Which particles are kept does not change (any coordinate outside [0, L] drops the particle whole).  Per
axis, t = v s with s = N / L:
  CIC (2)   i = floor(t) (0 .. N), f = t - i: cells i mod N and (i + 1) mod N get 1 - f and f
  TSC (3)   t2 = t + 0.5, i = floor(t2) (0 .. N), d = t2 - i - 0.5: cells (i - 1) mod N, i mod N, (i + 1) mod N get 0.5 (0.5 - d)^2,
            0.75 - d^2, 0.5 (0.5 + d)^2
The particle adds ((wx wy) wz) m; v = L gives i = N, which wraps to cell 0.

The spectrum.  phi[i] = exp(+i pi n_i / N) per axis for the integer wave numbers n = fftfreq(N) N, phi[N/2] = 1 (a definition: +i and -i
are equally valid there, a real value keeps the combined field real).  With F1, F2 = np.fft.fftn of the grids, C = (F1 + Phi F2) / 2,
Phi(a, b, c) = phi[a] phi[b] phi[c], and the estimate per linear k-bin of power_spectrum is the mean of w |C|^2, w the window weights of
xpk_oracle."""
import numpy as np

import deposit_cloud_oracle as CO
import fft_oracle as O
import xpk_oracle as X

ORDERS = CO.ORDERS


def shifted_weights(v, N, L, order):
    """(keep [n], cells [n, order] wrapped into 0 .. N - 1, w [n, order]) of one column on the shifted grid"""
    assert order in (2, 3)
    v = np.asarray(v, dtype=np.float64)
    s = N / L
    keep = CO.inside(v, L)
    t = np.where(keep, v, 0.0) * s
    if order == 2:
        fl = np.floor(t)
        f = t - fl
        i = fl.astype(np.int64)
        cells = np.stack([i % N, (i + 1) % N], axis=1)
        w = np.stack([1.0 - f, f], axis=1)
    else:
        t2 = t + 0.5
        fl = np.floor(t2)
        d = t2 - fl - 0.5
        a, b = 0.5 - d, 0.5 + d
        i = fl.astype(np.int64)
        cells = np.stack([(i - 1) % N, i % N, (i + 1) % N], axis=1)
        w = np.stack([0.5 * (a * a), 0.75 - d * d, 0.5 * (b * b)], axis=1)
    return keep, cells, w


def shifted_base_cell(v, N, L, order):
    """the cell a particle is sorted by on the shifted grid: i mod N for both orders"""
    v = np.asarray(v, dtype=np.float64)
    t = np.where(CO.inside(v, L), v, 0.0) * (N / L)
    return np.floor(t if order == 2 else t + 0.5).astype(np.int64) % N


def _deposit_with(weights_fn, coords, mass, N, L, order, unit_weights=False, widen=0):
    """deposit_cloud_oracle.deposit, the per-axis weights from weights_fn"""
    assert unit_weights or not widen
    ndim = len(coords)
    n = np.asarray(coords[0]).size
    per = [weights_fn(c, N, L, order) for c in coords]
    keep = np.ones(n, dtype=bool)
    for k, _, _ in per:
        keep &= k
    m = np.ones(n) if mass is None else np.asarray(mass, dtype=np.float64)
    m = m[keep]
    out = np.zeros(N ** ndim)
    offsets = np.stack(np.meshgrid(*([np.arange(-widen, order + widen)] * ndim), indexing='ij'), axis=-1).reshape(-1, ndim)
    for off in offsets:
        flat = np.zeros(m.size, dtype=np.int64)
        w = None
        for a in range(ndim):
            if unit_weights:
                flat = flat * N + (per[a][1][keep, 0] + off[a]) % N
                continue
            flat = flat * N + per[a][1][keep, off[a]]
            wa = per[a][2][keep, off[a]]
            w = wa if w is None else w * wa
        val = m.copy() if unit_weights else w * m
        out += np.bincount(flat, weights=val, minlength=out.size)
    return out.reshape((N,) * ndim)


def shifted_deposit(coords, mass, N, L, order, unit_weights=False, widen=0):
    """the map [N] * ndim of the particles on the shifted grid; arguments as deposit_cloud_oracle.deposit"""
    return _deposit_with(shifted_weights, coords, mass, N, L, order, unit_weights, widen)


def deposit(coords, mass, N, L, order, shift=0, **kw):
    return shifted_deposit(coords, mass, N, L, order, **kw) if shift else CO.deposit(coords, mass, N, L, order, **kw)


def phi_table(N):
    """phi[i] = exp(+i pi n_i / N), phi[N/2] = 1, cos and sin taken in long double and rounded to fp64 once"""
    n = np.rint(np.fft.fftfreq(N) * N).astype(np.int64)
    x = 4 * np.arctan(np.longdouble(1)) * n.astype(np.longdouble) / np.longdouble(N)
    phi = np.cos(x).astype(np.float64) + 1j * np.sin(x).astype(np.float64)
    if N % 2 == 0:
        phi[N // 2] = 1.0
    return phi


def phase_cube(N):
    phi = phi_table(N)
    return phi[:, None, None] * phi[None, :, None] * phi[None, None, :]


def combined(map1, map2):
    """C = (F1 + Phi F2) / 2 on the full cube"""
    map1, map2 = np.asarray(map1, dtype=np.float64), np.asarray(map2, dtype=np.float64)
    assert map1.ndim == 3 and len(set(map1.shape)) == 1 and map1.shape == map2.shape
    return 0.5 * (np.fft.fftn(map1) + phase_cube(map1.shape[0]) * np.fft.fftn(map2))


def auto_means(spectra, L, nk, p):
    """xpk_oracle.binned_cube's 'paa' of each full spectrum of the list: the same bins, weights and long-double sums, one sort for all"""
    N = spectra[0].shape[0]
    i = np.arange(N)
    a, b, c = i[:, None, None], i[None, :, None], i[None, None, :]
    _, kinds = O.mode_k_and_bin(N, L, nk, a, b, c)
    t = X.window_weight(N, p)
    w = t[a] * t[b] * t[c]
    ok = (kinds >= 0) & (kinds < nk)
    sel = kinds[ok]
    counts = np.bincount(sel, minlength=nk).astype(np.int64)
    order = np.argsort(sel, kind='stable')
    sb = sel[order]
    starts = np.flatnonzero(np.r_[True, sb[1:] != sb[:-1]])
    out = []
    for F in spectra:
        v = (w * (F.real.astype(np.longdouble) ** 2 + F.imag.astype(np.longdouble) ** 2))[ok][order]
        sums = np.zeros(nk)
        if sb.size:
            sums[sb[starts]] = np.add.reduceat(v, starts).astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            out.append(sums / counts)
    return out


def interlaced_ref(map1, map2, L, nk, p):
    """{'k', 'pk', 'pk_grid1', 'counts', 'paa', 'pbb'}: engine.interlaced_power_spectrum by np.fft.fftn on the full cube and
    xpk_oracle.binned_cube(C, C, ...); paa = pk_grid1 and pbb are the windowed auto spectra of the two grids, the scale of the error bound"""
    C = combined(map1, map2)
    b = X.binned_cube(C, C, L, nk, p)
    paa, pbb = auto_means([np.fft.fftn(np.asarray(map1, dtype=np.float64)), np.fft.fftn(np.asarray(map2, dtype=np.float64))], L, nk, p)
    return {'k': b['k'], 'pk': b['paa'], 'pk_grid1': paa, 'counts': b['counts'], 'paa': paa, 'pbb': pbb}


def twisted_route(map1, map2, L, nk, p):
    """(paa + pbb + 2 pab) / 4 with map 1's spectrum twisted, A' = F1 conj(Phi): the route that needs no bin kernel of its own"""
    A = np.fft.fftn(np.asarray(map1, dtype=np.float64)) * np.conj(phase_cube(np.asarray(map1).shape[0]))
    b = X.binned_cube(A, np.fft.fftn(np.asarray(map2, dtype=np.float64)), L, nk, p)
    return (b['paa'] + b['pbb'] + 2 * b['pab']) / 4


def particle_power_spectrum_ref(coords, mass, N, L, nk, order, interlace=True, normalize=False, subtract_shot_noise=False):
    """engine.particle_power_spectrum: deposit, shifted deposit, interlaced spectrum with the order's window divided out"""
    coords = [np.asarray(c, dtype=np.float64) for c in coords]
    map1 = CO.deposit(coords, mass, N, L, order)
    if interlace:
        r = interlaced_ref(map1, shifted_deposit(coords, mass, N, L, order), L, nk, order)
        out = {key: r[key] for key in ('k', 'pk', 'pk_grid1', 'counts')}
    else:
        F = np.fft.fftn(map1)
        b = X.binned_cube(F, F, L, nk, order)
        out = {'k': b['k'], 'pk': b['paa'], 'pk_grid1': b['paa'].copy(), 'counts': b['counts']}
    keep = CO.kept(coords, L)
    m = np.ones(int(keep.sum())) if mass is None else np.asarray(mass, dtype=np.float64)[keep]
    out['mass'], out['shot_noise'] = float(m.sum()), float((m * m).sum())
    if subtract_shot_noise:
        out['pk'], out['pk_grid1'] = out['pk'] - out['shot_noise'], out['pk_grid1'] - out['shot_noise']
    if normalize:
        norm = L ** 3 / out['mass'] ** 2
        out['pk'], out['pk_grid1'], out['shot_noise'] = out['pk'] * norm, out['pk_grid1'] * norm, out['shot_noise'] * norm
    return out
