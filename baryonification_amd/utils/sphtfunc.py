"""Spherical-harmonic transforms of RING-ordered HEALPix maps, named and defaulted after healpy.sphtfunc (healpy >= 1.16),
spin 0, fp64, on the GPU (libbfgx: bfgx_sht_*).  `bfg.utils.anafast(shell_map)` replaces `hp.anafast(shell_map)`.

Inputs are numpy arrays (or anything np.asarray takes); results come back as numpy arrays.  A CUDA torch tensor is analysed
where it is, without crossing PCIe, and the results stay on the device as torch tensors.  Every call of one shape
(nside, lmax, mmax) reuses one cached engine.ShtPlan, so repeated calls allocate no new device workspace.
"""
import numpy as np

from .. import engine
from .io import npix2nside

__all__ = ['map2alm', 'alm2map', 'alm2cl', 'anafast', 'getlmax', 'getidx', 'getsize', 'UNSEEN']

UNSEEN = -1.6375e30


def getsize(lmax, mmax=None):
    """healpy.Alm.getsize"""
    mmax = lmax if mmax is None or mmax < 0 else mmax
    return mmax * (2 * lmax + 1 - mmax) // 2 + lmax + 1


def getidx(lmax, l, m):
    """healpy.Alm.getidx"""
    return m * (2 * lmax + 1 - m) // 2 + l


def getlmax(s, mmax=None):
    """healpy.Alm.getlmax: the lmax of `s` coefficients, -1 if there is none"""
    if mmax is not None and mmax >= 0:
        x = (2 * s + mmax ** 2 - mmax - 2) / (2 * mmax + 2)
    else:
        x = (-3 + np.sqrt(1 + 8 * s)) / 2
    if x != np.floor(x):
        return -1
    return int(x)


def _is_torch(x):
    return type(x).__module__.startswith('torch') and getattr(x, 'is_cuda', False)


def _unsupported(**kw):
    for name, (value, default) in kw.items():
        if value is not default and value != default:
            raise NotImplementedError("%s=%r is not supported (spin-0 transforms without healpy's data files)" % (name, value))


def _map_input(maps, name='maps'):
    """(1-D float64 map, nside, on_device)"""
    if _is_torch(maps):
        import torch
        m = maps
        if m.dim() == 2 and m.shape[0] == 1:
            m = m[0]
        if m.dim() == 2:
            raise NotImplementedError("%s: more than one map (polarisation, TQU) is not supported" % name)
        if m.dim() != 1 or m.dtype not in (torch.float64, torch.float32):
            raise ValueError("%s must be a 1-D float map" % name)
        return m.to(torch.float64).contiguous(), npix2nside(m.numel()), True
    m = np.asarray(maps)
    if m.ndim == 2 and m.shape[0] == 1:
        m = m[0]
    if m.ndim == 2:
        raise NotImplementedError("%s: more than one map (polarisation, TQU) is not supported" % name)
    if m.ndim != 1 or m.dtype not in (np.float64, np.float32):
        raise ValueError("%s must be a 1-D float array of 12 nside^2 pixels (got dtype %s, shape %s)" % (name, m.dtype, m.shape))
    nside = npix2nside(m.size)
    engine.sht_work_doubles(nside, 0, 0)                  # ValueError naming the supported range, before any copy
    return np.ascontiguousarray(m, dtype=np.float64), nside, False


def _shape(nside, lmax, mmax):
    lmax = 3 * nside - 1 if lmax is None else int(lmax)
    mmax = lmax if mmax is None else int(mmax)
    if lmax < 0:
        raise ValueError("lmax must be >= 0 (got %d)" % lmax)
    if mmax < 0 or mmax > lmax:
        raise ValueError("mmax must be in [0, lmax] (got mmax %d, lmax %d)" % (mmax, lmax))
    engine.sht_work_doubles(nside, lmax, mmax)            # ValueError naming the supported range (nside <= 2048)
    return lmax, mmax


def _to_device(m, plan):
    import torch
    return torch.from_numpy(m).to(plan.dev)


def map2alm(maps, lmax=None, mmax=None, iter=3, pol=True, use_weights=False, datapath=None, gal_cut=0, use_pixel_weights=False):
    """alm (complex128, healpy order) of a RING map: alm = A(map), then `iter` times alm += A(map - alm2map(alm)).
    Pixels equal to UNSEEN (healpy.mask_bad) count as 0."""
    _unsupported(use_weights=(use_weights, False), use_pixel_weights=(use_pixel_weights, False), datapath=(datapath, None),
                 gal_cut=(gal_cut, 0))
    m, nside, on_dev = _map_input(maps)
    lmax, mmax = _shape(nside, lmax, mmax)
    if int(iter) < 0:
        raise ValueError("iter must be >= 0")
    plan = engine.sht_plan(nside, lmax, mmax)
    alm = plan.map2alm_device(m if on_dev else _to_device(m, plan), iter=int(iter))
    return alm if on_dev else alm.cpu().numpy()


def _alm_input(alms, lmax, mmax, name='alms'):
    if _is_torch(alms):
        import torch
        a = alms
        if a.dim() == 2 and a.shape[0] == 1:
            a = a[0]
        if a.dim() == 2:
            raise NotImplementedError("%s: more than one set of alm (polarisation) is not supported" % name)
        if a.dim() != 1:
            raise ValueError("%s must be a 1-D complex array" % name)
        a, size, on_dev = a.to(torch.complex128).contiguous(), a.numel(), True
    else:
        a = np.asarray(alms)
        if a.ndim == 2 and a.shape[0] == 1:
            a = a[0]
        if a.ndim == 2:
            raise NotImplementedError("%s: more than one set of alm (polarisation) is not supported" % name)
        if a.ndim != 1 or not (np.iscomplexobj(a) or np.issubdtype(a.dtype, np.floating)):
            raise ValueError("%s must be a 1-D complex array" % name)
        a, size, on_dev = np.ascontiguousarray(a, dtype=np.complex128), a.size, False
    if lmax is None:
        lmax = getlmax(size, mmax)
        if lmax < 0:
            raise ValueError("%s: %d coefficients give no integer lmax" % (name, size))
    lmax = int(lmax)
    mmax = lmax if mmax is None else int(mmax)
    if lmax < 0 or mmax < 0 or mmax > lmax:
        raise ValueError("need 0 <= mmax <= lmax (got mmax %d, lmax %d)" % (mmax, lmax))
    if size != getsize(lmax, mmax):
        raise ValueError("%s has %d coefficients, (lmax, mmax) = (%d, %d) needs %d" % (name, size, lmax, mmax, getsize(lmax, mmax)))
    return a, lmax, mmax, on_dev


def alm2map(alms, nside, lmax=None, mmax=None, pixwin=False, fwhm=0.0, sigma=None, pol=True, inplace=False):
    """float64 RING map of alm: map = sum_l [a_l0 lambda_l0 + 2 Re sum_{m>0} a_lm lambda_lm e^{i m phi}] (Im a_l0 ignored)"""
    _unsupported(pixwin=(pixwin, False), fwhm=(fwhm, 0.0), sigma=(sigma, None))
    a, lmax, mmax, on_dev = _alm_input(alms, lmax, mmax)
    nside = int(nside)
    if nside < 1:
        raise ValueError("nside must be >= 1")
    _shape(nside, lmax, mmax)
    plan = engine.sht_plan(nside, lmax, mmax)
    m = plan.alm2map_device(a if on_dev else _to_device(a, plan))
    return m if on_dev else m.cpu().numpy()


def alm2cl(alms1, alms2=None, lmax=None, mmax=None, lmax_out=None):
    """cl[l] = (Re a_l0 b*_l0 + 2 sum_{m=1}^{min(l, mmax)} Re a_lm b*_lm) / (2l + 1), l <= lmax_out (default lmax; 0 beyond lmax)"""
    a, lmax, mmax, on_dev = _alm_input(alms1, lmax, mmax, 'alms1')
    b = None
    if alms2 is not None:
        b, l2, m2, d2 = _alm_input(alms2, lmax, mmax, 'alms2')
        if d2 != on_dev:
            raise ValueError("alms1 and alms2 must both be on the host or both on the device")
    lmax_out = lmax if lmax_out is None else int(lmax_out)
    if lmax_out < 0:
        raise ValueError("lmax_out must be >= 0")
    if on_dev:
        return engine.alm2cl_device(a, b, lmax, mmax, lmax_out, device=a.device.index or 0)
    return engine.sht_alm2cl_host(a, b, lmax, mmax, lmax_out)


def anafast(map1, map2=None, nspec=None, lmax=None, mmax=None, iter=3, alm=False, pol=True, use_weights=False, datapath=None,
            gal_cut=0, use_pixel_weights=False):
    """C_l of a map (or the cross-spectrum of two): map2alm + alm2cl, the reduction on the device (only cl crosses PCIe unless
    alm=True).  Returns cl, or (cl, alm) / (cl, alm1, alm2) with alm=True."""
    _unsupported(use_weights=(use_weights, False), use_pixel_weights=(use_pixel_weights, False), datapath=(datapath, None),
                 gal_cut=(gal_cut, 0), nspec=(nspec, None))
    m1, nside, on_dev = _map_input(map1, 'map1')
    m2 = None
    if map2 is not None:
        m2, nside2, d2 = _map_input(map2, 'map2')
        if nside2 != nside:
            raise ValueError("map1 and map2 have different nside (%d, %d)" % (nside, nside2))
        if d2 != on_dev:
            raise ValueError("map1 and map2 must both be on the host or both on the device")
    lmax, mmax = _shape(nside, lmax, mmax)
    if int(iter) < 0:
        raise ValueError("iter must be >= 0")
    plan = engine.sht_plan(nside, lmax, mmax)
    a1 = plan.map2alm_device(m1 if on_dev else _to_device(m1, plan), iter=int(iter))
    a2 = None if m2 is None else plan.map2alm_device(m2 if on_dev else _to_device(m2, plan), iter=int(iter))
    cl = plan.alm2cl_device(a1, a2)
    out = [cl] + ([a1] + ([a2] if a2 is not None else []) if alm else [])
    if not on_dev:
        out = [x.cpu().numpy() for x in out]
    return out[0] if len(out) == 1 else tuple(out)
