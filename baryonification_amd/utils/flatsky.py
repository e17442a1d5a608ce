"""Fourier-space tools for square 2-D maps (flat-sky patches) on the GPU: the transform pair, power spectra in linear k-bins, isotropic
smoothing and the Kaiser-Squires pair, on the 2-D FFT of csrc/bfgx_fft2d.hpp.

Axis 0 of a map is x and axis 1 is y (MeasureProfilesGrid's geometry); the side N is a power of two in [8, 4096].  numpy in gives numpy
out (uploaded to device 0); a C-contiguous CUDA float64 tensor is analysed where it lies, on torch's current stream, and maps come back
as tensors on its device.  Per-bin spectra are numpy arrays either way.  Mixing the two kinds in one call is a ValueError."""
import numpy as np

from .. import _lib, _tensors, engine
from .._tensors import is_tensor, launch_args, to_cuda

__all__ = ['rfft2', 'irfft2', 'power_spectrum_2d', 'cross_power_spectrum_2d', 'smoothing_2d', 'kappa_to_shear_2d', 'shear_to_kappa_2d']

MIN_SIDE, MAX_SIDE = 8, 4096


def _check_side(N, what):
    if N < MIN_SIDE or N > MAX_SIDE or N & (N - 1):
        raise ValueError("%s needs a side that is a power of two in [%d, %d], not %d" % (what, MIN_SIDE, MAX_SIDE, N))


def _square_maps(what, *maps):
    """(on_device, maps made contiguous float64): all numpy or all CUDA float64 tensors on one device, square 2-D, one shape, a supported
    side; ValueError otherwise, before the library is touched"""
    kinds = [is_tensor(m) for m in maps]
    if any(kinds) and not all(kinds):
        raise ValueError("%s needs numpy arrays or CUDA float64 tensors, not one of each" % what)
    out = []
    for m in maps:
        if kinds[0]:
            if not m.is_cuda or str(m.dtype) != 'torch.float64':
                raise ValueError("%s needs a CUDA float64 tensor" % what)
            m = m.contiguous()
        else:
            m = _lib.f8(m)
        shape = tuple(int(s) for s in m.shape)
        if len(shape) != 2 or shape[0] != shape[1]:
            raise ValueError("%s needs a square 2-D map, not shape %s" % (what, shape))
        _check_side(shape[0], what)
        out.append(m)
    for m in out[1:]:
        if tuple(m.shape) != tuple(out[0].shape):
            raise ValueError("%s needs maps of one shape" % what)
        if kinds[0] and m.device != out[0].device:
            raise ValueError("%s needs maps on one device" % what)
    return kinds[0], out


def _work(N, like):
    import torch
    return torch.empty(engine.fft2_work_doubles(N), dtype=torch.float64, device=like.device)


def rfft2(Map):
    """The unnormalised transform of a real square map, np.fft.rfft2's coefficients.  numpy in: complex [N][N/2 + 1].  CUDA tensor in:
    a float64 tensor [N][fft_pitch(N)][2] (real, imaginary) whose columns c > N/2 are padding."""
    import torch
    on_dev, (m,) = _square_maps("rfft2", Map)
    d = m if on_dev else to_cuda(m)
    N = int(d.shape[0])
    spec = torch.empty((N, engine.fft_pitch(N), 2), dtype=torch.float64, device=d.device)
    work = _work(N, d)
    engine.rfft2_device(d.data_ptr(), N, work.data_ptr(), spec.data_ptr(), **launch_args(d))
    if on_dev:
        return spec
    return np.ascontiguousarray(spec.cpu().numpy().view(np.complex128)[:, :N // 2 + 1, 0])


def irfft2(spec, N):
    """The normalised inverse of rfft2: either form of its result back to the real map [N][N] (numpy in, numpy out)."""
    import torch
    N = int(N)
    _check_side(N, "irfft2")
    pitch, nz = N // 2 + 1 + 7 & ~7, N // 2 + 1
    on_dev = is_tensor(spec)
    if on_dev:
        if not spec.is_cuda or spec.dtype != torch.float64 or tuple(spec.shape) != (N, pitch, 2):
            raise ValueError("irfft2 needs a CUDA float64 tensor of shape [N][fft_pitch(N)][2]")
        d = spec.contiguous()
    else:
        s = np.asarray(spec)
        if s.shape != (N, nz):
            raise ValueError("irfft2 needs a complex array of shape [N][N/2 + 1]")
        padded = np.zeros((N, pitch), dtype=np.complex128)
        padded[:, :nz] = s
        d = torch.from_numpy(padded.view(np.float64).reshape(N, pitch, 2)).to('cuda:0')
    out = torch.empty((N, N), dtype=torch.float64, device=d.device)
    work = _work(N, d)
    engine.irfft2_device(d.data_ptr(), N, 1.0 / (float(N) * float(N)), work.data_ptr(), out.data_ptr(), **launch_args(d))
    return out if on_dev else out.cpu().numpy()


def _check_bins(what, L, Nk, window):
    p = engine.window_order(window, what)
    if isinstance(Nk, bool) or int(Nk) != Nk or not 1 <= int(Nk) <= 2048:
        raise ValueError("%s needs 1 <= Nk <= 2048" % what)
    if not float(L) > 0:
        raise ValueError("%s needs L > 0" % what)
    return p, int(Nk), float(L)


def cross_power_spectrum_2d(MapA, MapB, L, Nk=180, window='none', normalize=False):
    """Auto and cross power spectra of two square 2-D maps of side length L in the bins and units of engine.power_spectrum (the
    unnormalised transform; Nk linear bins between 2 pi / L and the Nyquist frequency); `window` as in engine.cross_power_spectrum.
    normalize=True multiplies the spectra by L^2 / N^4: the flat-sky C_l when L is in radians.  Returns a dict of numpy arrays k, paa, pbb,
    pab = <Re(F_A conj F_B)>, r = pab / sqrt(paa pbb), counts; empty bins NaN."""
    what = "cross_power_spectrum_2d"
    on_dev, (A, B) = _square_maps(what, MapA, MapB)
    p, Nk, L = _check_bins(what, L, Nk, window)
    N = int(A.shape[0])
    if not on_dev:
        out = np.empty((4, Nk))
        cnt = np.empty(Nk, dtype=np.int64)
        _lib.call('bfgx_power_spectrum_2d', 0, N, A.ctypes.data, B.ctypes.data, L, Nk, p, out[0].ctypes.data, out[1].ctypes.data,
                  out[2].ctypes.data, out[3].ctypes.data, cnt.ctypes.data)
        paa, pbb, pab, k = out
    else:
        work = _work(N, A)
        (paa, pbb, pab, k), cnt = _tensors.bin_means(A.device, 4, Nk, lambda *out: engine.power_spectrum_2d_device(
            A.data_ptr(), B.data_ptr(), N, L, Nk, p, work.data_ptr(), *out, **launch_args(A)))
    with np.errstate(divide='ignore', invalid='ignore'):
        r = pab / np.sqrt(paa * pbb)
    if normalize:
        norm = L * L / float(N) ** 4
        paa, pbb, pab = paa * norm, pbb * norm, pab * norm
    return {'k': k, 'paa': paa, 'pbb': pbb, 'pab': pab, 'r': r, 'counts': cnt}


def power_spectrum_2d(Map, L, Nk=180, window='none', normalize=False):
    """The power spectrum of one square 2-D map: cross_power_spectrum_2d(Map, Map, ...) as a dict of numpy arrays k, pk, counts."""
    x = cross_power_spectrum_2d(Map, Map, L, Nk, window, normalize)
    return {'k': x['k'], 'pk': x['paa'], 'counts': x['counts']}


def smoothing_2d(Map, L, fwhm=None, sigma=None, tophat=None, beam=None):
    """A square 2-D map of side length L convolved (periodically) with an isotropic kernel, exactly one of: a Gaussian of `fwhm` or of
    `sigma` = fwhm / sqrt(8 ln 2), b(k) = exp(-k^2 sigma^2 / 2); a top hat of radius `tophat`, b = 2 J1(kR) / (kR); a table beam=(k, b),
    interpolated linearly in k and held at its end values (np.interp).  Widths are in the units of L; a width of 0 returns the map."""
    what = "smoothing_2d"
    on_dev, (m,) = _square_maps(what, Map)
    if sum(x is not None for x in (fwhm, sigma, tophat, beam)) != 1:
        raise ValueError("%s needs exactly one of fwhm, sigma, tophat, beam" % what)
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
    else:
        kind, param = 'gauss', float(sigma) if sigma is not None else float(fwhm) / np.sqrt(8.0 * np.log(2.0))
    if not param >= 0 or not np.isfinite(param):
        raise ValueError("%s needs a finite width >= 0" % what)
    N = int(m.shape[0])
    if not on_dev:
        out = np.empty((N, N))
        _lib.call('bfgx_filter_map_2d', 0, N, m.ctypes.data, L, engine.FILTER_KINDS_2D[kind], param, _tensors.ptr(tk), _tensors.ptr(tb),
                  0 if tk is None else tk.size, out.ctypes.data)
        return out
    import torch
    out = torch.empty_like(m)
    work = _work(N, m)
    engine.filter_map_2d_device(m.data_ptr(), N, L, kind, param, tk, tb, work.data_ptr(), out.data_ptr(), **launch_args(m))
    return out


def kappa_to_shear_2d(kappa):
    """Kaiser-Squires on a periodic square patch: the shear (g1, g2) of a convergence map.  With axis 0 = x, axis 1 = y and the integer
    wave numbers (n0, n1), g1^ = (n0^2 - n1^2) / (n0^2 + n1^2) kappa^ and g2^ = 2 n0 n1 / (n0^2 + n1^2) kappa^ (0 at the zero mode; g2^ = 0
    where an index is the Nyquist index), which makes gamma_t of MeasureProfilesGrid(..., shear=(g1, g2)) positive around a mass peak.
    A square map's kernel depends on the integer wave numbers alone: no side length is taken."""
    on_dev, (m,) = _square_maps("kappa_to_shear_2d", kappa)
    N = int(m.shape[0])
    if not on_dev:
        g1, g2 = np.empty((N, N)), np.empty((N, N))
        _lib.call('bfgx_kappa_to_shear_2d', 0, N, m.ctypes.data, g1.ctypes.data, g2.ctypes.data)
        return g1, g2
    import torch
    g1, g2 = torch.empty_like(m), torch.empty_like(m)
    work = _work(N, m)
    engine.kappa_to_shear_2d_device(m.data_ptr(), N, work.data_ptr(), g1.data_ptr(), g2.data_ptr(), **launch_args(m))
    return g1, g2


def shear_to_kappa_2d(g1, g2):
    """The inverse rotation: (kappa_E, kappa_B) of a shear pair, kappa_E^ = c2 g1^ + s2 g2^, kappa_B^ = -s2 g1^ + c2 g2^ with the factors
    of kappa_to_shear_2d.  shear_to_kappa_2d(*kappa_to_shear_2d(kappa)) is (kappa - mean(kappa), 0) up to the Nyquist-index modes."""
    on_dev, (a, b) = _square_maps("shear_to_kappa_2d", g1, g2)
    N = int(a.shape[0])
    if not on_dev:
        ke, kb = np.empty((N, N)), np.empty((N, N))
        _lib.call('bfgx_shear_to_kappa_2d', 0, N, a.ctypes.data, b.ctypes.data, ke.ctypes.data, kb.ctypes.data)
        return ke, kb
    import torch
    ke, kb = torch.empty_like(a), torch.empty_like(a)
    work = _work(N, a)
    engine.shear_to_kappa_2d_device(a.data_ptr(), b.data_ptr(), N, work.data_ptr(), ke.data_ptr(), kb.data_ptr(), **launch_args(a))
    return ke, kb
