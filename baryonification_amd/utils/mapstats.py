"""Higher-order statistics of HEALPix shells on the GPU (libbfgx: bfgx_mapstats_*, bfgx_sht_almxfl_device):

    map_moments(maps, order=4, mask=None)                   mean, central moments and cross-moments of up to 3 maps
    peak_counts(map, bins, mask=None, nest=False, return_flags=False)     histograms of local maxima and minima
    shell_statistics(maps, scales, window='gauss', lmax=None, iter=3, order=4, peak_bins=None, mask=None)
                                                            both, of the maps smoothed at several scales, resident on the device

A pixel is good if every map is finite and not UNSEEN there (healpy.mask_bad's tolerance) and `mask`, where given, is nonzero.
Inputs are numpy arrays or CUDA torch tensors (processed where they are).  The moments are bit-reproducible: two passes (means,
then central products), fp64 partial sums combined in a fixed order, no float atomics.  The peak counts are integers, so exact.

Before / after baryonification:

    s0 = shell_statistics(shell, scales)
    s1 = shell_statistics(baryonified_shell, scales)
    ratio = s1['central'][:, s1['exponents'].index((3,))] / s0['central'][:, s0['exponents'].index((3,))]
"""
import ctypes as C

import numpy as np

from .. import _lib, engine
from .io import npix2nside
from .pixelfunc import check_nside
from . import sphtfunc

__all__ = ['map_moments', 'peak_counts', 'shell_statistics', 'moment_exponents']

MAX_MAPS, MAX_ORDER, MAX_BINS = 3, 4, 4096


def _is_torch(x):
    return type(x).__module__.startswith('torch') and getattr(x, 'is_cuda', False)


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
    if _is_torch(maps) or isinstance(maps, np.ndarray):
        ms = [maps] if maps.ndim == 1 else list(maps) if maps.ndim == 2 else None
        if ms is None:
            raise ValueError("maps must be one map (npix,) or several (nmaps, npix) (got shape %s)" % (tuple(maps.shape),))
    elif isinstance(maps, (list, tuple)) and len(maps) and all(np.ndim(m) == 0 for m in maps):
        ms = [np.asarray(maps)]
    elif isinstance(maps, (list, tuple)):
        ms = [m if _is_torch(m) else np.asarray(m) for m in maps]
    else:
        return _map_list(np.asarray(maps))
    if not 1 <= len(ms) <= MAX_MAPS:
        raise ValueError("maps must hold 1 to %d maps (got %d)" % (MAX_MAPS, len(ms)))
    for m in ms:
        if m.ndim != 1 or m.shape[0] == 0:
            raise ValueError("every map must be 1-D and not empty (got shape %s)" % (tuple(m.shape),))
        if m.shape[0] != ms[0].shape[0]:
            raise ValueError("the maps have different sizes (%d, %d)" % (ms[0].shape[0], m.shape[0]))
        kind = 'c' if (m.dtype.is_complex if _is_torch(m) else m.dtype.kind == 'c') else 'f'
        if kind == 'c':
            raise ValueError("maps must be real")
    return ms


def _device_of(*xs):
    import torch
    for x in xs:
        if _is_torch(x):
            return x.device, True
    return torch.device('cuda', 0), False


def _need_gpu():
    if _lib.load().bfgx_device_count() <= 0:
        raise _lib.BfgxError("bfgx: no HIP device visible: libbfgx has no CPU fallback")


def _stack(ms, dev, maps=None):
    """float64 [K, npix] on dev; `maps` (what the caller passed) is used as it is when it already is such a tensor"""
    import torch
    if _is_torch(maps) and maps.dtype == torch.float64 and maps.device == dev and maps.is_contiguous():
        return maps if maps.dim() == 2 else maps.unsqueeze(0)
    ts = [m.to(device=dev, dtype=torch.float64) if _is_torch(m) else torch.from_numpy(np.ascontiguousarray(m, dtype=np.float64)).to(dev)
          for m in ms]
    return ts[0].contiguous().unsqueeze(0) if len(ts) == 1 else torch.stack(ts)


def _check_mask(mask, npix):
    """mask as an array / tensor of the maps' shape (None stays None); ValueError otherwise (before any device call)"""
    if mask is None:
        return None
    mk = mask if _is_torch(mask) else np.asarray(mask)
    if tuple(mk.shape) != (npix,):
        raise ValueError("mask must have the maps' shape (%d,) (got %s)" % (npix, tuple(mk.shape)))
    return mk


def _mask_u8(mask, npix, dev):
    """uint8 [npix] on dev: 1 where mask is nonzero (None stays None)"""
    import torch
    if mask is None:
        return None
    if _is_torch(mask):
        return (mask != 0).to(device=dev, dtype=torch.uint8).contiguous()
    return torch.from_numpy((mask != 0).astype(np.uint8)).to(dev)


def _stream(dev):
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream or None)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _moments_device(stack, mask, order, n_out, out, work):
    """bfgx_mapstats_moments_device on a float64 [K, npix] tensor: n_out int64 [1], out float64 [K + nterms], work scratch"""
    dev = stack.device
    _lib.check(_lib.load().bfgx_mapstats_moments_device(dev.index or 0, _stream(dev), stack.shape[1], stack.shape[0], order, _p(stack),
                                                       _p(mask), _p(n_out), _p(out), _p(work)))


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
    _need_gpu()
    exps = moment_exponents(K, order)
    n_out = torch.empty(1, dtype=torch.int64, device=dev)
    out = torch.empty(K + len(exps), dtype=torch.float64, device=dev)
    work = torch.empty(_lib.MAPSTATS_WORK_DOUBLES, dtype=torch.float64, device=dev)
    _moments_device(_stack(ms, dev, maps), _mask_u8(mask, npix, dev), order, n_out, out, work)
    vals = out.cpu().numpy()
    return {'n': int(n_out.item()), 'mean': vals[:K].copy(), 'central': {e: float(v) for e, v in zip(exps, vals[K:])}}


def _edges(bins):
    e = np.asarray(bins.cpu() if _is_torch(bins) else bins, dtype=np.float64)
    if e.ndim != 1 or not 2 <= e.size <= MAX_BINS + 1:
        raise ValueError("bins must be 1-D with 2 to %d edges (1 to %d bins) (got shape %s)" % (MAX_BINS + 1, MAX_BINS, e.shape))
    if not np.all(np.isfinite(e)) or not np.all(np.diff(e) > 0):
        raise ValueError("bins must be finite and ascending")
    return np.ascontiguousarray(e)


def _peaks_device(m, mask, nside, nest, edges_dev, counts, flags):
    dev = m.device
    _lib.check(_lib.load().bfgx_mapstats_peaks_device(dev.index or 0, _stream(dev), nside, int(bool(nest)), _p(m), _p(mask),
                                                     edges_dev.numel() - 1, _p(edges_dev), _p(counts), _p(flags)))


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
    _need_gpu()
    m = _stack(ms, dev, map)[0]
    counts = torch.empty((2, e.size - 1), dtype=torch.int64, device=dev)
    flags = torch.empty(npix, dtype=torch.int8, device=dev) if return_flags else None
    _peaks_device(m, _mask_u8(mask, npix, dev), nside, nest, torch.from_numpy(e).to(dev), counts, flags)
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


def shell_statistics(maps, scales, window='gauss', lmax=None, iter=3, order=4, peak_bins=None, mask=None):
    """map_moments (and, with peak_bins, peak_counts of every map) of K <= 3 RING maps (nside <= 2048) smoothed at each of `scales`
    (radians: the FWHM of window='gauss', the radius of window='tophat'; 0 = no filter), without leaving the device: every map gets
    one map2alm; per scale, almxfl writes into a scratch alm and alm2map into a scratch map.  `mask` (nonzero = keep) zeroes pixels
    before the analysis and excludes them from the statistics after it; UNSEEN pixels count as 0 on the way in and are bad after.
    Returns a dict of arrays with a leading n_scales axis (numpy, or CUDA tensors for CUDA input): 'n' int64 [S], 'mean' [S, K],
    'central' [S, nterms] in the order of 'exponents' (moment_exponents(K, order)), and with peak_bins 'maxima' / 'minima' int64
    [S, K, nb].  The numbers are those of smoothing, map_moments and peak_counts called one by one, bit for bit."""
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
    mask = _check_mask(mask, npix)
    dev, on_dev = _device_of(*(ms + [mask]))
    _need_gpu()
    plan = engine.sht_plan(nside, lmax, mmax, device=dev.index or 0)
    S, exps = len(wins), moment_exponents(K, order)
    mk = _mask_u8(mask, npix, dev)
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
    for s in range(S):
        for k in range(K):
            plan.almxfl_device(alms[k], fl[s], out=alm_s)
            plan.alm2map_device(alm_s, out=map_s[k])
        map_s.masked_fill_(unseen, sphtfunc.UNSEEN)
        _moments_device(map_s, mk, order, n_out[s:s + 1], out[s], work)
        if e is not None:
            for k in range(K):
                _peaks_device(map_s[k], mk, nside, False, edges_dev, counts[s, k], None)
    res = {'n': n_out, 'mean': out[:, :K], 'central': out[:, K:], 'exponents': exps}
    if e is not None:
        res['maxima'], res['minima'] = counts[:, :, 0], counts[:, :, 1]
    if not on_dev:
        res = {k: (v.cpu().numpy() if k != 'exponents' else v) for k, v in res.items()}
    return res
