"""Higher-order statistics of square 2-D maps (flat-sky patches) on the GPU, the flat twin of utils/mapstats.py:

    derivatives_2d(Map, L, fwhm=None, sigma=None, tophat=None, beam=None, spin_form=False)
                                                            [u, u_x, u_y, u_xx, u_xy, u_yy] of the (filtered) map
    peak_counts_2d(Map, bins, mask=None, periodic=True, return_flags=False)       histograms of local maxima and minima of a grid
    minkowski_functionals_2d(Map, L, bins, mask=None, fwhm=None, sigma=None, tophat=None, beam=None)
                                                            V0, V1, V2 of the excursion sets, per bin of the map's value
    minkowski_gaussian_2d(sigma0, sigma1, thresholds)       their expectation for a Gaussian field (host numpy)
    patch_statistics(maps, L, scales, window='gauss', order=4, peak_bins=None, mask=None, mf_bins=None, periodic=True)
                                                            all of them, of K <= 3 maps smoothed at several scales, resident on the device

Axis 0 of a map is x and axis 1 is y; L is the side length and every width is in its units.  The spectral functions take a side N that is
a power of two in [8, 4096] (utils/flatsky.py) and treat the patch as periodic; peak_counts_2d takes any side in [3, 16384].  numpy in
gives numpy out (through device 0); a C-contiguous CUDA float64 tensor is processed where it lies, on torch's current stream, and gives
CUDA results.  Mixing the two kinds in one call is a ValueError.

Derivatives are spectral: the half spectrum times i k_x, i k_y, -k_x^2, -k_x k_y, -k_y^2 with k = 2 pi / L n, n = fftfreq's integer wave
numbers; a factor that is odd in an index is set to 0 at that index's Nyquist value (n = N / 2), where it would break the Hermitian
symmetry of a real map's spectrum.  One kernel reads the spectrum once and writes all six products (csrc/bfgx_fft2d.hpp).

A pixel is good if it is finite and not UNSEEN and `mask`, where given, is nonzero (the rule of utils/mapstats.py).  A pixel is a maximum
if it is strictly greater than its 8 neighbours (periodic=True wraps both axes; periodic=False: a border pixel is never an extremum), a
minimum if strictly less, and only if it and all 8 are good.  The Minkowski functionals are those of mapstats.minkowski_from_derivatives
with (u_t, u_p) = (u_x, u_y): v1 and v2 are per unit area in the units of L.

Before / after baryonification:

    s0 = patch_statistics(kappa_dmo, L, scales)['central']
    s1 = patch_statistics(kappa_bar, L, scales)['central']
    ratio = s1[:, 1] / s0[:, 1]                             # the third central moment per smoothing scale
"""
import numpy as np

from .. import _lib, engine
from .._tensors import is_tensor, launch_args, to_cuda, mask_u8, ptr
from . import mapstats as _ms
from .flatsky import _square_maps
from .sphtfunc import UNSEEN, unseen_mask

__all__ = ['derivatives_2d', 'peak_counts_2d', 'minkowski_functionals_2d', 'minkowski_gaussian_2d', 'patch_statistics']

MIN_GRID, MAX_GRID = 3, 16384


def _filter(what, L, fwhm=None, sigma=None, tophat=None, beam=None):
    """(kind, param, table_k, table_b) of at most one filter argument (none: 'unit'); ValueError otherwise"""
    if sum(x is not None for x in (fwhm, sigma, tophat, beam)) > 1:
        raise ValueError("%s takes at most one of fwhm, sigma, tophat, beam" % what)
    if not float(L) > 0:
        raise ValueError("%s needs L > 0" % what)
    tk = tb = None
    if beam is not None:
        kind, param = 'table', 0.0
        tk, tb = (np.ascontiguousarray(x, dtype=np.float64) for x in beam)
        if tk.ndim != 1 or tk.shape != tb.shape or tk.size < 1:
            raise ValueError("%s: beam = (k, b), two 1-D arrays of one length" % what)
        if not (np.isfinite(tk).all() and np.isfinite(tb).all() and (np.diff(tk) > 0).all()):
            raise ValueError("%s: the beam table must be finite with k strictly ascending" % what)
    elif tophat is not None:
        kind, param = 'tophat', float(tophat)
    elif sigma is not None or fwhm is not None:
        kind, param = 'gauss', float(sigma) if sigma is not None else float(fwhm) / np.sqrt(8.0 * np.log(2.0))
    else:
        kind, param = 'unit', 0.0
    if not param >= 0 or not np.isfinite(param):
        raise ValueError("%s needs a finite width >= 0" % what)
    return kind, param, tk, tb


def _check_mask_2d(what, mask, shape, on_dev):
    """mask of the map's shape and kind (None stays None); ValueError otherwise"""
    if mask is None:
        return None
    if is_tensor(mask) != on_dev:
        raise ValueError("%s needs numpy arrays or CUDA tensors, not one of each" % what)
    if on_dev and not mask.is_cuda:
        raise ValueError("%s needs a CUDA mask" % what)
    mk = mask if on_dev else np.asarray(mask)
    if tuple(mk.shape) != tuple(shape):
        raise ValueError("%s: mask must have the map's shape %s (got %s)" % (what, tuple(shape), tuple(mk.shape)))
    return mk


def _flat_mask(mask, dev):
    """uint8 [n * n] on dev, 1 where the mask is nonzero (None stays None)"""
    return None if mask is None else mask_u8(mask.reshape(-1), dev)


class _PatchBuffers(object):
    """the device arrays of one side N, allocated once: the half spectra of K maps, the scratch of the transforms and the nder maps"""

    def __init__(self, N, K, nder, dev):
        import torch
        self.N, self.nder, self.dev = N, nder, dev
        self.spec = torch.empty((K, N, engine.fft_pitch(N), 2), dtype=torch.float64, device=dev)
        nw = max(engine.derivatives_2d_work_doubles(N, nder), engine.fft2_work_doubles(N))
        self.work = torch.empty(nw, dtype=torch.float64, device=dev)
        self.ders = torch.empty((nder, N, N), dtype=torch.float64, device=dev)

    def forward(self, m, k=0):
        engine.rfft2_device(m.data_ptr(), self.N, self.work.data_ptr(), self.spec[k].data_ptr(), **launch_args(m))

    def derivatives(self, L, flt, spin_form, k=0):
        kind, param, tk, tb = flt
        engine.derivatives_2d_device(self.spec[k].data_ptr(), self.N, L, kind, param, tk, tb, self.nder, spin_form, self.work.data_ptr(),
                                     self.ders.data_ptr(), **launch_args(self.ders))
        return self.ders


def derivatives_2d(Map, L, fwhm=None, sigma=None, tophat=None, beam=None, spin_form=False):
    """[u, u_x, u_y, u_xx, u_xy, u_yy] as [6, N, N], u the map convolved (periodically) with at most one of smoothing_2d's kernels (none:
    the map itself); spin_form=True gives [u, u_x, u_y, lap = u_xx + u_yy, q_plus = u_xx - u_yy, q_cross = 2 u_xy], the form
    minkowski_from_derivatives(spin_form=True) takes."""
    what = "derivatives_2d"
    on_dev, (m,) = _square_maps(what, Map)
    flt = _filter(what, L, fwhm, sigma, tophat, beam)
    d = m if on_dev else to_cuda(m)
    buf = _PatchBuffers(int(d.shape[0]), 1, 6, d.device)
    buf.forward(d)
    ders = buf.derivatives(float(L), flt, spin_form)
    return ders if on_dev else ders.cpu().numpy()


def _grid_map(what, Map):
    """(on_device, the map made contiguous float64): a square 2-D grid of a side in [3, 16384]; ValueError otherwise"""
    on_dev = is_tensor(Map)
    if on_dev:
        if not Map.is_cuda or str(Map.dtype) != 'torch.float64':
            raise ValueError("%s needs a CUDA float64 tensor" % what)
        m = Map.contiguous()
    else:
        m = _lib.f8(Map)
    shape = tuple(int(s) for s in m.shape)
    if len(shape) != 2 or shape[0] != shape[1]:
        raise ValueError("%s needs a square 2-D map, not shape %s" % (what, shape))
    if not MIN_GRID <= shape[0] <= MAX_GRID:
        raise ValueError("%s needs a side in [%d, %d], not %d" % (what, MIN_GRID, MAX_GRID, shape[0]))
    return on_dev, m


def _peaks_device(m, mask, periodic, edges_dev, counts, flags):
    engine.peaks_2d_device(m.data_ptr(), int(m.shape[0]), periodic, ptr(mask), edges_dev.numel() - 1, edges_dev.data_ptr(), counts.data_ptr(),
                           ptr(flags), **launch_args(m))


def peak_counts_2d(Map, bins, mask=None, periodic=True, return_flags=False):
    """Counts of the local maxima and minima of a square grid (any side in [3, 16384]) by value.  `bins` are nb + 1 finite ascending
    edges (1 <= nb <= 4096); bin b holds edges[b] <= value < edges[b + 1], values outside the edges are dropped.  Returns what
    mapstats.peak_counts returns: {'maxima': int64 [nb], 'minima': int64 [nb]}, with return_flags also an int8 map [n, n], +1 at a
    maximum, -1 at a minimum, 0 elsewhere."""
    import torch
    what = "peak_counts_2d"
    on_dev, m = _grid_map(what, Map)
    e = _ms._edges(bins)
    mask = _check_mask_2d(what, mask, m.shape, on_dev)
    d = m if on_dev else to_cuda(m)
    dev = d.device
    counts = torch.empty((2, e.size - 1), dtype=torch.int64, device=dev)
    flags = torch.empty(tuple(d.shape), dtype=torch.int8, device=dev) if return_flags else None
    _peaks_device(d, _flat_mask(mask, dev), periodic, torch.from_numpy(e).to(dev), counts, flags)
    if not on_dev:
        counts = counts.cpu().numpy()
        flags = flags.cpu().numpy() if return_flags else None
    res = {'maxima': counts[0], 'minima': counts[1]}
    return (res, flags) if return_flags else res


def _zeroed(d, mk):
    """(the map with masked and UNSEEN pixels at 0, as it enters the transform; the UNSEEN pixels)"""
    import torch
    zero = torch.zeros((), dtype=torch.float64, device=d.device)
    if mk is not None:
        d = torch.where(mk.bool().view(d.shape), d, zero)
    unseen = unseen_mask(d)
    return torch.where(unseen, zero, d), unseen


def minkowski_functionals_2d(Map, L, bins, mask=None, fwhm=None, sigma=None, tophat=None, beam=None):
    """The Minkowski functionals V0, V1, V2 of the excursion sets of one square map, per bin of its value, without leaving the device:
    rfft2, the six derivative maps of the (filtered) spectrum in spin form and mapstats' reduction.  `mask` (nonzero = keep) zeroes pixels
    before the transform and excludes them after it; UNSEEN pixels count as 0 on the way in and are excluded after.  Returns what
    minkowski_from_derivatives returns; v1 and v2 are per unit area in the units of L (`bins`: 1 to 512 bins)."""
    what = "minkowski_functionals_2d"
    on_dev, (m,) = _square_maps(what, Map)
    flt = _filter(what, L, fwhm, sigma, tophat, beam)
    e = _ms._edges(bins, _ms.MAX_MF_BINS)
    mask = _check_mask_2d(what, mask, m.shape, on_dev)
    d = m if on_dev else to_cuda(m)
    N, dev = int(d.shape[0]), d.device
    mk = _flat_mask(mask, dev)
    d, unseen = _zeroed(d, mk)
    buf = _PatchBuffers(N, 1, 6, dev)
    buf.forward(d)
    ders = buf.derivatives(float(L), flt, True)
    ders[0].masked_fill_(unseen, UNSEEN)
    mf = _ms._MinkowskiBuffers(N * N, e, (), dev)
    mf.run(ders, mk)
    return _ms._minkowski_result(mf.functionals(), on_dev)


def minkowski_gaussian_2d(sigma0, sigma1, thresholds):
    """The expected Minkowski functionals of a Gaussian random field on the plane with variance sigma0^2 and gradient variance
    sigma1^2 = <|grad u|^2> at the thresholds t (host numpy): mapstats.minkowski_gaussian's closed forms with tau = sigma1^2 / (2 sigma0^2)
    and nu = t / sigma0.  Returns {'v0', 'v1', 'v2'} of the thresholds' shape and 'sigma0', 'sigma1'; V1 and V2 are per unit of t / sigma0."""
    from math import erfc
    s0, s1 = float(sigma0), float(sigma1)
    if not (s0 > 0 and np.isfinite(s0)) or not (s1 >= 0 and np.isfinite(s1)):
        raise ValueError("minkowski_gaussian_2d needs finite sigma0 > 0 and sigma1 >= 0")
    tau = s1 * s1 / (2 * (s0 * s0))
    nu = np.asarray(thresholds, dtype=np.float64) / s0
    g = np.exp(-0.5 * nu * nu)
    return {'v0': 0.5 * np.vectorize(erfc, otypes=[np.float64])(nu / np.sqrt(2.0)), 'v1': np.sqrt(tau) / 8.0 * g,
            'v2': tau * (2 * np.pi) ** -1.5 * nu * g, 'sigma0': s0, 'sigma1': s1}


def _patch_maps(what, maps):
    """the K <= 3 maps of patch_statistics as a list: one map [N, N], a stack [K, N, N] or a sequence of maps"""
    if is_tensor(maps) or isinstance(maps, np.ndarray):
        ms = [maps] if maps.ndim == 2 else list(maps) if maps.ndim == 3 else None
        if ms is None:
            raise ValueError("%s: maps must be one map (N, N) or several (K, N, N) (got shape %s)" % (what, tuple(maps.shape)))
    elif isinstance(maps, (list, tuple)) and len(maps) and all(getattr(m, 'ndim', 0) == 2 for m in maps):
        ms = list(maps)
    else:
        return _patch_maps(what, np.asarray(maps))
    if not 1 <= len(ms) <= _ms.MAX_MAPS:
        raise ValueError("%s: maps must hold 1 to %d maps (got %d)" % (what, _ms.MAX_MAPS, len(ms)))
    return ms


def _scale_filters(what, L, scales, window):
    if window not in ('gauss', 'tophat'):
        raise ValueError("window must be 'gauss' or 'tophat' (got %r)" % (window,))
    sc = np.atleast_1d(np.asarray(scales, dtype=np.float64))
    if sc.ndim != 1 or sc.size == 0 or not np.all(np.isfinite(sc)) or np.any(sc < 0):
        raise ValueError("scales must be a non-empty 1-D sequence of finite widths >= 0")
    # a scale of 0 is no filter, as the single calls without a filter argument
    return [_filter(what, L) if s == 0 else _filter(what, L, fwhm=s) if window == 'gauss' else _filter(what, L, tophat=s) for s in sc]


def patch_statistics(maps, L, scales, window='gauss', order=4, peak_bins=None, mask=None, mf_bins=None, periodic=True):
    """map_moments (and, with peak_bins, peak_counts_2d of every map) of K <= 3 square maps of side length L smoothed at each of `scales`
    (the FWHM of window='gauss', the radius of window='tophat', in the units of L; 0 = no filter), without leaving the device: every map
    gets one rfft2; per scale and map one kernel forms the filtered spectrum (with mf_bins: and its five derivative spectra) and the
    inverse transforms follow.  `mask` (nonzero = keep) zeroes pixels before the transform and excludes them from the statistics after it;
    UNSEEN pixels count as 0 on the way in and are bad after.  Returns the dict of mapstats.shell_statistics, arrays with a leading
    n_scales axis (numpy, or CUDA tensors for CUDA input): 'n' int64 [S], 'mean' [S, K], 'central' [S, nterms] in the order of 'exponents'
    (moment_exponents(K, order)), with peak_bins 'maxima' / 'minima' int64 [S, K, nb], with mf_bins (1 to 512 bins) 'v0' [S, K, nb + 1]
    and 'v1', 'v2' [S, K, nb].  The numbers are those of derivatives_2d, map_moments, peak_counts_2d and minkowski_functionals_2d called
    one by one, bit for bit."""
    import torch
    what = "patch_statistics"
    ms = _patch_maps(what, maps)
    on_dev, ms = _square_maps(what, *ms)
    K, order = _ms._check_k_order(len(ms), order)
    flts = _scale_filters(what, L, scales, window)
    e = None if peak_bins is None else _ms._edges(peak_bins)
    me = None if mf_bins is None else _ms._edges(mf_bins, _ms.MAX_MF_BINS)
    mask = _check_mask_2d(what, mask, ms[0].shape, on_dev)
    L = float(L)
    ds = ms if on_dev else [to_cuda(m) for m in ms]
    N, dev = int(ds[0].shape[0]), ds[0].device
    npix = N * N
    S, exps = len(flts), _ms.moment_exponents(K, order)
    mk = _flat_mask(mask, dev)
    buf = _PatchBuffers(N, K, 1 if me is None else 6, dev)
    unseen = torch.empty((K, N, N), dtype=torch.bool, device=dev)
    for k in range(K):
        d, unseen[k] = _zeroed(ds[k], mk)
        buf.forward(d, k)
    map_s = torch.empty((K, N, N), dtype=torch.float64, device=dev)
    n_out = torch.empty(S, dtype=torch.int64, device=dev)
    out = torch.empty((S, K + len(exps)), dtype=torch.float64, device=dev)
    work = torch.empty(_lib.MAPSTATS_WORK_DOUBLES, dtype=torch.float64, device=dev)
    if e is not None:
        edges_dev = torch.from_numpy(e).to(dev)
        counts = torch.empty((S, K, 2, e.size - 1), dtype=torch.int64, device=dev)
    if me is not None:
        mf = _ms._MinkowskiBuffers(npix, me, (S, K), dev)
    for s in range(S):
        for k in range(K):
            ders = buf.derivatives(L, flts[s], True, k)
            map_s[k].copy_(ders[0])
            if me is not None:
                ders[0].masked_fill_(unseen[k], UNSEEN)
                mf.run(ders, mk, (s, k))
        map_s.masked_fill_(unseen, UNSEEN)
        _ms._moments_device(map_s.view(K, npix), mk, order, n_out[s:s + 1], out[s], work)
        if e is not None:
            for k in range(K):
                _peaks_device(map_s[k], mk, periodic, edges_dev, counts[s, k], None)
    res = {'n': n_out, 'mean': out[:, :K], 'central': out[:, K:], 'exponents': exps}
    if e is not None:
        res['maxima'], res['minima'] = counts[:, :, 0], counts[:, :, 1]
    if me is not None:
        f = mf.functionals()
        res['v0'], res['v1'], res['v2'] = f['v0'], f['v1'], f['v2']
    if not on_dev:
        res = {k: (v.cpu().numpy() if k != 'exponents' else v) for k, v in res.items()}
    return res
