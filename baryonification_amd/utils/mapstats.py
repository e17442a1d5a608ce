"""Higher-order statistics of HEALPix shells on the GPU (libbfgx: bfgx_mapstats_*, bfgx_sht_almxfl_device):

    map_moments(maps, order=4, mask=None)                   mean, central moments and cross-moments of up to 3 maps
    peak_counts(map, bins, mask=None, nest=False, return_flags=False)     histograms of local maxima and minima
    minkowski_functionals(map, bins, mask=None, lmax=None, iter=3, fwhm=0.0, sigma=None, beam_window=None)
                                                            V0, V1, V2 of the excursion sets of a map, per bin of its value
    minkowski_from_derivatives(ders, bins, mask=None, spin_form=False)    the same from the six maps of alm2map_der2
    minkowski_gaussian(cl, thresholds)                      their expectation for a Gaussian field (host numpy)
    shell_statistics(maps, scales, window='gauss', lmax=None, iter=3, order=4, peak_bins=None, mask=None, mf_bins=None)
                                                            all of them, of the maps smoothed at several scales, resident on the device

A pixel is good if every map is finite and not UNSEEN there (healpy.mask_bad's tolerance) and `mask`, where given, is nonzero.
Inputs are numpy arrays or CUDA torch tensors (processed where they are).  The moments are bit-reproducible: two passes (means,
then central products), fp64 partial sums combined in a fixed order, no float atomics.  The peak counts are integers, so exact.

Minkowski functionals.  With u_t, u_p the gradient and u;tt, u;tp, u;pp the second covariant derivatives of u in the orthonormal
basis (sphtfunc.alm2map_der2), the area, boundary length and integrated geodesic curvature of the excursion set {u >= t}, per
unit area of the sphere and as densities in t estimated over the bin [edges[b], edges[b + 1]) of width D_b, are
    v0[b] = (good pixels with u >= edges[b]) / n                                            (nb + 1 values, exact)
    v1[b] = sum_b sqrt(u_t^2 + u_p^2) / (4 n D_b)
    v2[b] = sum_b (2 u_t u_p u;tp - u_t^2 u;pp - u_p^2 u;tt) / (u_t^2 + u_p^2) / (2 pi n D_b)
over the n good pixels (equal areas: da / A = 1 / n).  The sums are bit-reproducible like the moments.  Thresholds in units of
sigma: edges = mean + sigma nu from map_moments.

Before / after baryonification:

    s0 = shell_statistics(shell, scales)
    s1 = shell_statistics(baryonified_shell, scales)
    ratio = s1['central'][:, s1['exponents'].index((3,))] / s0['central'][:, s0['exponents'].index((3,))]
"""
import numpy as np

from .. import _lib, engine
from .._tensors import is_cuda_tensor, device_index, stream, ptr, mask_u8, need_gpu
from .io import npix2nside
from .pixelfunc import check_nside
from . import sphtfunc

__all__ = ['map_moments', 'peak_counts', 'shell_statistics', 'moment_exponents', 'minkowski_functionals',
           'minkowski_from_derivatives', 'minkowski_gaussian']

MAX_MAPS, MAX_ORDER, MAX_BINS, MAX_MF_BINS = 3, 4, 4096, 512


def moment_exponents(nmaps, order=4):
    """the exponent tuples (e_0, .., e_{nmaps-1}) with 2 <= sum <= order, in the order libbfgx returns the central moments
    (include/bfgx.h): total degree ascending; within a degree e_0 descending, then e_1 descending"""
    nmaps, order = _check_k_order(nmaps, order)
    out = []
    for d in range(2, order + 1):
        if nmaps == 1:
            out.append((d,))
        elif nmaps == 2:
            out += [(e0, d - e0) for e0 in range(d, -1, -1)]
        else:
            out += [(e0, e1, d - e0 - e1) for e0 in range(d, -1, -1) for e1 in range(d - e0, -1, -1)]
    return out


def _check_k_order(nmaps, order):
    if int(order) != order or not 2 <= int(order) <= MAX_ORDER:
        raise ValueError("order must be in [2, %d] (got %r)" % (MAX_ORDER, order))
    if not 1 <= int(nmaps) <= MAX_MAPS:
        raise ValueError("maps must hold 1 to %d maps (got %d)" % (MAX_MAPS, nmaps))
    return int(nmaps), int(order)


def _map_list(maps):
    """the maps as a list of 1-D arrays / tensors of one size; ValueError otherwise (before any device call)"""
    if is_cuda_tensor(maps) or isinstance(maps, np.ndarray):
        ms = [maps] if maps.ndim == 1 else list(maps) if maps.ndim == 2 else None
        if ms is None:
            raise ValueError("maps must be one map (npix,) or several (nmaps, npix) (got shape %s)" % (tuple(maps.shape),))
    elif isinstance(maps, (list, tuple)) and len(maps) and all(np.ndim(m) == 0 for m in maps):
        ms = [np.asarray(maps)]
    elif isinstance(maps, (list, tuple)):
        ms = [m if is_cuda_tensor(m) else np.asarray(m) for m in maps]
    else:
        return _map_list(np.asarray(maps))
    if not 1 <= len(ms) <= MAX_MAPS:
        raise ValueError("maps must hold 1 to %d maps (got %d)" % (MAX_MAPS, len(ms)))
    for m in ms:
        if m.ndim != 1 or m.shape[0] == 0:
            raise ValueError("every map must be 1-D and not empty (got shape %s)" % (tuple(m.shape),))
        if m.shape[0] != ms[0].shape[0]:
            raise ValueError("the maps have different sizes (%d, %d)" % (ms[0].shape[0], m.shape[0]))
        kind = 'c' if (m.dtype.is_complex if is_cuda_tensor(m) else m.dtype.kind == 'c') else 'f'
        if kind == 'c':
            raise ValueError("maps must be real")
    return ms


def _device_of(*xs):
    import torch
    for x in xs:
        if is_cuda_tensor(x):
            return x.device, True
    return torch.device('cuda', 0), False


def _stack(ms, dev, maps=None):
    """float64 [K, npix] on dev; `maps` (what the caller passed) is used as it is when it already is such a tensor"""
    import torch
    if is_cuda_tensor(maps) and maps.dtype == torch.float64 and maps.device == dev and maps.is_contiguous():
        return maps if maps.dim() == 2 else maps.unsqueeze(0)
    ts = [m.to(device=dev, dtype=torch.float64) if is_cuda_tensor(m) else torch.from_numpy(np.ascontiguousarray(m, dtype=np.float64)).to(dev)
          for m in ms]
    return ts[0].contiguous().unsqueeze(0) if len(ts) == 1 else torch.stack(ts)


def _check_mask(mask, npix):
    """mask as an array / tensor of the maps' shape (None stays None); ValueError otherwise (before any device call)"""
    if mask is None:
        return None
    mk = mask if is_cuda_tensor(mask) else np.asarray(mask)
    if tuple(mk.shape) != (npix,):
        raise ValueError("mask must have the maps' shape (%d,) (got %s)" % (npix, tuple(mk.shape)))
    return mk


def _moments_device(stack, mask, order, n_out, out, work):
    """bfgx_mapstats_moments_device on a float64 [K, npix] tensor: n_out int64 [1], out float64 [K + nterms], work scratch"""
    dev = stack.device
    _lib.call('bfgx_mapstats_moments_device', device_index(dev), stream(dev), stack.shape[1], stack.shape[0], order, ptr(stack), ptr(mask),
              ptr(n_out), ptr(out), ptr(work))


def map_moments(maps, order=4, mask=None):
    """Moments of one map, or of K <= 3 maps of equal size (a sequence or a (K, npix) array), over their good pixels, 2 <= order <= 4.
    Returns {'n': good pixels (int), 'mean': float64 [K], 'central': {exponent tuple: value}}, central[(e_0, .., e_{K-1})] = mean
    over the good pixels of prod_a (x_a - mean_a)^{e_a} for every tuple with 2 <= sum e <= order (moment_exponents: 3 entries for
    K = 1, 31 for K = 3 at order 4).  No good pixel: n = 0 and NaN everywhere."""
    import torch
    ms = _map_list(maps)
    K, order = _check_k_order(len(ms), order)
    npix = int(ms[0].shape[0])
    dev, _ = _device_of(*(ms + [mask]))
    mask = _check_mask(mask, npix)
    need_gpu()
    exps = moment_exponents(K, order)
    n_out = torch.empty(1, dtype=torch.int64, device=dev)
    out = torch.empty(K + len(exps), dtype=torch.float64, device=dev)
    work = torch.empty(_lib.MAPSTATS_WORK_DOUBLES, dtype=torch.float64, device=dev)
    _moments_device(_stack(ms, dev, maps), mask_u8(mask, dev), order, n_out, out, work)
    vals = out.cpu().numpy()
    return {'n': int(n_out.item()), 'mean': vals[:K].copy(), 'central': {e: float(v) for e, v in zip(exps, vals[K:])}}


def _edges(bins, max_bins=MAX_BINS):
    e = np.asarray(bins.cpu() if is_cuda_tensor(bins) else bins, dtype=np.float64)
    if e.ndim != 1 or not 2 <= e.size <= max_bins + 1:
        raise ValueError("bins must be 1-D with 2 to %d edges (1 to %d bins) (got shape %s)" % (max_bins + 1, max_bins, e.shape))
    if not np.all(np.isfinite(e)) or not np.all(np.diff(e) > 0):
        raise ValueError("bins must be finite and ascending")
    return np.ascontiguousarray(e)


def _peaks_device(m, mask, nside, nest, edges_dev, counts, flags):
    dev = m.device
    _lib.call('bfgx_mapstats_peaks_device', device_index(dev), stream(dev), nside, bool(nest), ptr(m), ptr(mask), edges_dev.numel() - 1,
              ptr(edges_dev), ptr(counts), ptr(flags))


def peak_counts(map, bins, mask=None, nest=False, return_flags=False):
    """Counts of the local maxima and minima of a map (RING, or NEST with nest=True) by value: a pixel is a maximum if it is strictly
    greater than every existing neighbour (get_all_neighbours), a minimum if strictly less, and only if it and all its existing
    neighbours are good.  `bins` are nb + 1 finite ascending edges (1 <= nb <= 4096); bin b holds edges[b] <= value < edges[b + 1],
    values outside the edges are dropped.  Returns {'maxima': int64 [nb], 'minima': int64 [nb]}; with return_flags also an int8 map,
    +1 at a maximum, -1 at a minimum, 0 elsewhere.  A CUDA tensor gives CUDA results."""
    import torch
    ms = _map_list(map)
    if len(ms) != 1:
        raise ValueError("peak_counts takes one map (got %d)" % len(ms))
    npix = int(ms[0].shape[0])
    nside = check_nside(npix2nside(npix), bool(nest))
    e = _edges(bins)
    mask = _check_mask(mask, npix)
    dev, on_dev = _device_of(ms[0], mask)
    need_gpu()
    m = _stack(ms, dev, map)[0]
    counts = torch.empty((2, e.size - 1), dtype=torch.int64, device=dev)
    flags = torch.empty(npix, dtype=torch.int8, device=dev) if return_flags else None
    _peaks_device(m, mask_u8(mask, dev), nside, nest, torch.from_numpy(e).to(dev), counts, flags)
    if not on_dev:
        counts = counts.cpu().numpy()
        flags = flags.cpu().numpy() if return_flags else None
    res = {'maxima': counts[0], 'minima': counts[1]}
    return (res, flags) if return_flags else res


def _windows(scales, window, lmax):
    if window not in ('gauss', 'tophat'):
        raise ValueError("window must be 'gauss' or 'tophat' (got %r)" % (window,))
    sc = np.atleast_1d(np.asarray(scales, dtype=np.float64))
    if sc.ndim != 1 or sc.size == 0 or not np.all(np.isfinite(sc)) or np.any(sc < 0):
        raise ValueError("scales must be a non-empty 1-D sequence of finite radians >= 0")
    return [sphtfunc.gauss_beam(s, lmax) if window == 'gauss' else sphtfunc.tophat_beam(s, lmax) for s in sc]


def shell_statistics(maps, scales, window='gauss', lmax=None, iter=3, order=4, peak_bins=None, mask=None, mf_bins=None):
    """map_moments (and, with peak_bins, peak_counts of every map) of K <= 3 RING maps (nside <= 2048) smoothed at each of `scales`
    (radians: the FWHM of window='gauss', the radius of window='tophat'; 0 = no filter), without leaving the device: every map gets
    one map2alm; per scale, almxfl writes into a scratch alm and alm2map into a scratch map.  `mask` (nonzero = keep) zeroes pixels
    before the analysis and excludes them from the statistics after it; UNSEEN pixels count as 0 on the way in and are bad after.
    Returns a dict of arrays with a leading n_scales axis (numpy, or CUDA tensors for CUDA input): 'n' int64 [S], 'mean' [S, K],
    'central' [S, nterms] in the order of 'exponents' (moment_exponents(K, order)), and with peak_bins 'maxima' / 'minima' int64
    [S, K, nb].  With mf_bins (1 to 512 bins) also the Minkowski functionals of every map, 'v0' [S, K, nb + 1] and 'v1', 'v2'
    [S, K, nb], from the same alm (four more syntheses per map and scale).  The numbers are those of smoothing, map_moments,
    peak_counts and minkowski_functionals called one by one, bit for bit."""
    import torch
    ms = _map_list(maps)
    K, order = _check_k_order(len(ms), order)
    npix = int(ms[0].shape[0])
    nside = npix2nside(npix)
    lmax, mmax = sphtfunc._shape(nside, lmax, None)
    if int(iter) < 0:
        raise ValueError("iter must be >= 0")
    wins = _windows(scales, window, lmax)
    e = None if peak_bins is None else _edges(peak_bins)
    me = None if mf_bins is None else _edges(mf_bins, MAX_MF_BINS)
    mask = _check_mask(mask, npix)
    dev, on_dev = _device_of(*(ms + [mask]))
    need_gpu()
    plan = engine.sht_plan(nside, lmax, mmax, device=device_index(dev))
    S, exps = len(wins), moment_exponents(K, order)
    mk = mask_u8(mask, dev)
    stack = _stack(ms, dev, maps)
    if mk is not None:
        stack = torch.where(mk.bool().unsqueeze(0), stack, torch.zeros((), dtype=torch.float64, device=dev))
    unseen = sphtfunc.unseen_mask(stack)
    alms = torch.empty((K, plan.nalm), dtype=torch.complex128, device=dev)
    for k in range(K):
        plan.map2alm_device(stack[k], iter=int(iter), out=alms[k])
    fl = torch.from_numpy(np.stack(wins)).to(dev)
    alm_s = torch.empty(plan.nalm, dtype=torch.complex128, device=dev)
    map_s = torch.empty((K, npix), dtype=torch.float64, device=dev)
    n_out = torch.empty(S, dtype=torch.int64, device=dev)
    out = torch.empty((S, K + len(exps)), dtype=torch.float64, device=dev)
    work = torch.empty(_lib.MAPSTATS_WORK_DOUBLES, dtype=torch.float64, device=dev)
    if e is not None:
        edges_dev = torch.from_numpy(e).to(dev)
        counts = torch.empty((S, K, 2, e.size - 1), dtype=torch.int64, device=dev)
    if me is not None:
        mf = _MinkowskiBuffers(npix, me, (S, K), dev)
        ders = torch.empty((6, npix), dtype=torch.float64, device=dev)
    for s in range(S):
        for k in range(K):
            plan.almxfl_device(alms[k], fl[s], out=alm_s)
            if me is None:
                plan.alm2map_device(alm_s, out=map_s[k])
            else:
                plan.alm2map_der_device(alm_s, ders)                               # its first map is alm2map_device(alm_s)
                map_s[k].copy_(ders[0])
                ders[0].masked_fill_(unseen[k], sphtfunc.UNSEEN)
                mf.run(ders, mk, (s, k))
        map_s.masked_fill_(unseen, sphtfunc.UNSEEN)
        _moments_device(map_s, mk, order, n_out[s:s + 1], out[s], work)
        if e is not None:
            for k in range(K):
                _peaks_device(map_s[k], mk, nside, False, edges_dev, counts[s, k], None)
    res = {'n': n_out, 'mean': out[:, :K], 'central': out[:, K:], 'exponents': exps}
    if e is not None:
        res['maxima'], res['minima'] = counts[:, :, 0], counts[:, :, 1]
    if me is not None:
        f = mf.functionals()
        res['v0'], res['v1'], res['v2'] = f['v0'], f['v1'], f['v2']
    if not on_dev:
        res = {k: (v.cpu().numpy() if k != 'exponents' else v) for k, v in res.items()}
    return res


# ---------------------------------------------------------------------------------------------------- Minkowski functionals
class _MinkowskiBuffers(object):
    """the device arrays of bfgx_mapstats_minkowski_device for a batch of maps of one size and one set of edges: counts int64
    [*batch, nb + 3], sums float64 [*batch, 2, nb], the edges and the scratch, allocated once"""

    def __init__(self, npix, edges, batch, dev):
        import torch
        self.npix, self.nb, self.dev = int(npix), edges.size - 1, dev
        nw = int(_lib.call('bfgx_mapstats_minkowski_work_doubles', self.npix, self.nb))
        if nw < 0:
            raise ValueError("minkowski: npix %d or %d bins out of range" % (self.npix, self.nb))
        self.edges = torch.from_numpy(edges).to(dev)
        self.counts = torch.empty(tuple(batch) + (self.nb + 3,), dtype=torch.int64, device=dev)
        self.sums = torch.empty(tuple(batch) + (2, self.nb), dtype=torch.float64, device=dev)
        self.work = torch.empty(nw, dtype=torch.float64, device=dev)

    def run(self, ders, mask, at=()):
        """enqueue the kernel on float64 [6, npix] (spin form) into the slot `at` of the batch"""
        _lib.call('bfgx_mapstats_minkowski_device', device_index(self.dev), stream(self.dev), self.npix, ptr(ders), ptr(mask), self.nb,
                  ptr(self.edges), ptr(self.counts[at]), ptr(self.sums[at]), ptr(self.work))

    def functionals(self):
        """{'n' [*batch], 'count' [*batch, nb], 'v0' [*batch, nb + 1], 'v1', 'v2' [*batch, nb]} as device tensors"""
        import torch
        nb = self.nb
        n = self.counts[..., nb + 2]
        nf = torch.where(n > 0, n.to(torch.float64), torch.full((), float('nan'), dtype=torch.float64, device=self.dev)).unsqueeze(-1)
        # pixels with u >= edges[b]: the bins b, b + 1, .., nb - 1 and those at or above edges[nb] (integers: exact)
        seq = torch.cat([self.counts[..., :nb], self.counts[..., nb + 1:nb + 2]], -1)
        above = seq.sum(-1, keepdim=True) - torch.cumsum(seq, -1) + seq
        width = self.edges[1:] - self.edges[:-1]
        return {'n': n, 'count': self.counts[..., :nb], 'v0': above.to(torch.float64) / nf,
                'v1': self.sums[..., 0, :] / (4.0 * nf * width), 'v2': self.sums[..., 1, :] / (2.0 * np.pi * nf * width)}


def _minkowski_result(f, on_dev):
    if not on_dev:
        f = {k: v.cpu().numpy() for k, v in f.items()}
    f['n'] = int(f['n'].item())
    return f


def minkowski_from_derivatives(ders, bins, mask=None, spin_form=False):
    """The Minkowski functionals of a map u from its derivatives ders [6, npix] = [u, u_t, u_p, u;tt, u;tp, u;pp] (alm2map_der2;
    numpy or a CUDA tensor), or with spin_form=True [u, u_t, u_p, lap, q_plus, q_cross] (alm2map_der2(spin_form=True)), over the
    pixels where all six are finite, u is not UNSEEN and `mask`, where given, is nonzero.  `bins` are nb + 1 finite ascending edges (1 <= nb <= 512).
    Returns {'n': good pixels (int), 'count': int64 [nb] pixels per bin, 'v0': [nb + 1], 'v1': [nb], 'v2': [nb]} (the module
    docstring has the definitions); no good pixel gives n = 0 and NaN.  A CUDA tensor gives CUDA results."""
    import torch
    d = ders if is_cuda_tensor(ders) else np.asarray(ders)
    if d.ndim != 2 or d.shape[0] != 6 or d.shape[1] == 0:
        raise ValueError("ders must hold six maps (6, npix) (got shape %s)" % (tuple(d.shape),))
    if d.dtype.is_complex if is_cuda_tensor(d) else d.dtype.kind == 'c':
        raise ValueError("ders must be real")
    npix = int(d.shape[1])
    e = _edges(bins, MAX_MF_BINS)
    mask = _check_mask(mask, npix)
    dev, on_dev = _device_of(d, mask)
    need_gpu()
    t = d.to(device=dev, dtype=torch.float64) if is_cuda_tensor(d) else torch.from_numpy(np.ascontiguousarray(d, dtype=np.float64)).to(dev)
    if not spin_form:
        t = torch.cat([t[:3], (t[3] + t[5]).unsqueeze(0), (t[3] - t[5]).unsqueeze(0), (2.0 * t[4]).unsqueeze(0)])
    mf = _MinkowskiBuffers(npix, e, (), dev)
    mf.run(t.contiguous(), mask_u8(mask, dev))
    return _minkowski_result(mf.functionals(), on_dev)


def minkowski_functionals(map, bins, mask=None, lmax=None, iter=3, fwhm=0.0, sigma=None, beam_window=None):
    """The Minkowski functionals V0, V1, V2 of the excursion sets of one RING map (nside <= 2048), per bin of its value, without
    leaving the device: map2alm(map, iter), the optional harmonic window (beam_window, else the Gaussian of sigma, else that of
    fwhm, radians, as smoothing takes them), the six derivative maps of the filtered alm (ShtPlan.alm2map_der_device) and one
    reduction.  `mask` (nonzero = keep) zeroes pixels before the analysis and excludes them after it; UNSEEN pixels count as 0 on
    the way in and are excluded after.  Returns what minkowski_from_derivatives returns."""
    import torch
    ms = _map_list(map)
    if len(ms) != 1:
        raise ValueError("minkowski_functionals takes one map (got %d)" % len(ms))
    npix = int(ms[0].shape[0])
    nside = npix2nside(npix)
    lmax, mmax = sphtfunc._shape(nside, lmax, None)
    if int(iter) < 0:
        raise ValueError("iter must be >= 0")
    e = _edges(bins, MAX_MF_BINS)
    filtered = beam_window is not None or sigma is not None or fwhm != 0.0
    fl = sphtfunc._window(lmax, fwhm, sigma, beam_window) if filtered else None
    mask = _check_mask(mask, npix)
    dev, on_dev = _device_of(ms[0], mask)
    need_gpu()
    plan = engine.sht_plan(nside, lmax, mmax, device=device_index(dev))
    mk = mask_u8(mask, dev)
    m = _stack(ms, dev, map)[0]
    if mk is not None:
        m = torch.where(mk.bool(), m, torch.zeros((), dtype=torch.float64, device=dev))
    alm = plan.map2alm_device(m, iter=int(iter))
    if fl is not None:
        plan.almxfl_device(alm, sphtfunc._fl_device(fl, dev), out=alm)
    ders = plan.alm2map_der_device(alm, torch.empty((6, npix), dtype=torch.float64, device=dev))
    ders[0].masked_fill_(sphtfunc.unseen_mask(m), sphtfunc.UNSEEN)
    mf = _MinkowskiBuffers(npix, e, (), dev)
    mf.run(ders, mk)
    return _minkowski_result(mf.functionals(), on_dev)


def minkowski_gaussian(cl, thresholds):
    """The expected Minkowski functionals of a Gaussian random field on the sphere with power spectrum cl[l] (l = 0 ..) at the
    thresholds t (host numpy): with sigma0^2 = sum (2l + 1) C_l / 4 pi, sigma1^2 = sum (2l + 1) l (l + 1) C_l / 4 pi,
    tau = sigma1^2 / (2 sigma0^2) and nu = t / sigma0,
        V0 = erfc(nu / sqrt 2) / 2,   V1 = sqrt(tau) exp(-nu^2 / 2) / 8,   V2 = tau (2 pi)^{-3/2} nu exp(-nu^2 / 2).
    Returns {'v0', 'v1', 'v2'} of the thresholds' shape and 'sigma0', 'sigma1'.  V1 and V2 are per unit of t / sigma0: divide by
    sigma0 to compare with the densities in t that minkowski_functionals returns."""
    from math import erfc
    cl = np.asarray(cl, dtype=np.float64)
    if cl.ndim != 1 or cl.size == 0 or not np.all(np.isfinite(cl)) or np.any(cl < 0):
        raise ValueError("cl must be a non-empty 1-D array of finite values >= 0")
    l = np.arange(cl.size, dtype=np.float64)
    s0 = np.sum((2 * l + 1) * cl) / (4 * np.pi)
    s1 = np.sum((2 * l + 1) * l * (l + 1) * cl) / (4 * np.pi)
    if not s0 > 0:
        raise ValueError("cl has no power")
    tau = s1 / (2 * s0)
    nu = np.asarray(thresholds, dtype=np.float64) / np.sqrt(s0)
    g = np.exp(-0.5 * nu * nu)
    return {'v0': 0.5 * np.vectorize(erfc, otypes=[np.float64])(nu / np.sqrt(2.0)), 'v1': np.sqrt(tau) / 8.0 * g,
            'v2': tau * (2 * np.pi) ** -1.5 * nu * g, 'sigma0': float(np.sqrt(s0)), 'sigma1': float(np.sqrt(s1))}
