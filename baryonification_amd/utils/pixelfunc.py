"""HEALPix pixel functions named and defaulted after healpy.pixelfunc, on the GPU (libbfgx: bfgx_hpx_*):

    ud_grade(map_in, nside_out, pess=False, order_in='RING', order_out=None, power=None, dtype=None)
    get_interp_weights(nside, theta, phi=None, nest=False, lonlat=False)
    get_interp_val(m, theta, phi, nest=False, lonlat=False)
    get_all_neighbours(nside, theta, phi=None, nest=False, lonlat=False)       (pixel indices only)

plus UNSEEN (shared with sphtfunc).  `anafast(ud_grade(shell, 2048))` takes the C_l of a shell finer than the transforms accept.

Inputs are numpy arrays (or anything np.asarray takes); results come back as numpy arrays.  CUDA torch tensors are processed where
they are, and the results are torch tensors on the same device (other array arguments of the same call are moved there).

Definitions that differ from, or go beyond, healpy's:
  * ud_grade counts a child as bad when it is within healpy.mask_bad's tolerance of UNSEEN *or not finite* (healpy's product
    `mr * goods` lets a NaN child through).  The sums are fp64, whatever the dtype, in a fixed order per output pixel, so results
    are bit-reproducible; the degraded value is (sum of good children) * ratio / (number of good children).
  * get_interp_weights / get_interp_val reduce phi to [0, 2 pi) before applying healpix_cxx's get_interpol; for phi already in
    [0, 2 pi) the result is healpix_cxx's.  theta outside [0, pi] (after the lonlat conversion) raises ValueError.
  * With phi=None the points are pixel centres and the pixel's own ring is taken as the ring above, which is what the rule gives in
    exact arithmetic (healpy recomputes cos(theta), which can round across the ring).
"""
import numpy as np

from .. import _lib
from .._tensors import is_cuda_tensor, device_index, stream, ptr
from .io import npix2nside
from .sphtfunc import UNSEEN

__all__ = ['ud_grade', 'get_interp_weights', 'get_interp_val', 'get_all_neighbours', 'UNSEEN']

MAX_NSIDE = 8192


def _is_pow2(n):
    return n >= 1 and (n & (n - 1)) == 0


def check_nside(nside, nest=True, name='nside'):
    """nside as an int; ValueError unless 1 <= nside <= 8192 (and a power of two when nest)"""
    try:
        n = int(nside)
    except (TypeError, ValueError):
        raise ValueError("%s must be an integer (got %r)" % (name, nside))
    if n != nside or not 1 <= n <= MAX_NSIDE or (nest and not _is_pow2(n)):
        raise ValueError("%s must be %sin [1, %d] (got %r)" % (name, "a power of two " if nest else "", MAX_NSIDE, nside))
    return n


def _order(o, name):
    s = str(o).upper() if isinstance(o, str) else None
    if s in ('RING',):
        return 0
    if s in ('NESTED', 'NEST'):
        return 1
    raise ValueError("%s must be 'RING', 'NESTED' or 'NEST' (got %r)" % (name, o))


def _like(x, device):
    """x as a torch tensor on `device` (no copy when it already is one)"""
    import torch
    return x if is_cuda_tensor(x) else torch.as_tensor(np.asarray(x), device=device)


def _find_device(*xs):
    for x in xs:
        if is_cuda_tensor(x):
            return x.device
    return None


# ------------------------------------------------------------------------------------------------------------------ ud_grade
def _np_float_dtype(dtype, name='dtype'):
    d = np.dtype(dtype)
    if d not in (np.float32, np.float64):
        raise ValueError("%s must be float32 or float64 (got %s)" % (name, d))
    return d


def ud_grade(map_in, nside_out, pess=False, order_in='RING', order_out=None, power=None, dtype=None):
    """healpy.ud_grade: map(s) at a new nside (and ordering).  map_in is one map (npix,) or several (nmaps, npix); nside_in and
    nside_out are powers of two in [1, 8192].  Degrading averages the good children of each output pixel (UNSEEN where none is good,
    or where any is bad with pess=True), times (nside_out / nside_in)^power; upgrading copies the parent (times the same factor).
    A child is bad if it is UNSEEN (healpy.mask_bad's tolerance) or not finite.  Output dtype: `dtype`, else the input's (float32 /
    float64; other inputs are read as float64)."""
    nest_in = _order(order_in, 'order_in')
    nest_out = nest_in if order_out is None else _order(order_out, 'order_out')
    nside_out = check_nside(nside_out, True, 'nside_out')
    on_dev = is_cuda_tensor(map_in)
    if on_dev:
        import torch
        m = map_in
        if m.dtype not in (torch.float32, torch.float64):
            m = m.to(torch.float64)
        tdt = {torch.float32: np.float32, torch.float64: np.float64}[m.dtype]
    else:
        m = np.asarray(map_in)
        if m.dtype not in (np.float32, np.float64):
            m = m.astype(np.float64)
        tdt = m.dtype
    if m.ndim not in (1, 2) or m.shape[-1] == 0:
        raise ValueError("map_in must be one map (npix,) or several (nmaps, npix) (got shape %s)" % (tuple(m.shape),))
    nside_in = check_nside(npix2nside(m.shape[-1]), True, 'nside_in')
    if dtype is None:
        out_dt = np.dtype(tdt)
    else:
        try:
            import torch
            if isinstance(dtype, torch.dtype):
                dtype = {torch.float32: np.float32, torch.float64: np.float64}.get(dtype, dtype)
        except ImportError:
            pass
        out_dt = _np_float_dtype(dtype)
    ratio = 1.0 if power is None else (float(nside_out) / float(nside_in)) ** float(power)
    nmaps = 1 if m.ndim == 1 else m.shape[0]
    if not 1 <= nmaps <= 65535:
        raise ValueError("map_in must hold 1 to 65535 maps (got %d)" % nmaps)
    npix_out = 12 * nside_out * nside_out
    oshape = (npix_out,) if m.ndim == 1 else (nmaps, npix_out)
    dt_in, dt_out = int(np.dtype(tdt) == np.float64), int(out_dt == np.float64)
    if on_dev:
        import torch
        m = m.contiguous()
        out = torch.empty(oshape, dtype=torch.float64 if dt_out else torch.float32, device=m.device)
        _lib.call('bfgx_hpx_ud_grade_device', device_index(m), stream(m), nside_in, nside_out, nmaps, nest_in, nest_out, bool(pess), ratio, dt_in,
                  dt_out, ptr(m), ptr(out))
        return out
    m = np.ascontiguousarray(m)
    out = np.empty(oshape, dtype=out_dt)
    _lib.call('bfgx_hpx_ud_grade', 0, nside_in, nside_out, nmaps, nest_in, nest_out, bool(pess), ratio, dt_in, dt_out, ptr(m), ptr(out))
    return out


# ------------------------------------------------------------------------------------------------------- interpolation
def _angles(theta, phi, lonlat, device):
    """(theta, phi) in radians as contiguous float64 arrays / tensors of one broadcast shape, checked"""
    if device is not None:
        import torch
        t = _like(theta, device).to(torch.float64)
        p = _like(phi, device).to(torch.float64)
        t, p = torch.broadcast_tensors(t, p)
        if lonlat:
            t, p = np.pi / 2 - torch.deg2rad(p), torch.deg2rad(t)
        t, p = t.contiguous(), p.contiguous()
        if t.numel() and bool(((t < 0) | (t > np.pi) | torch.isnan(t)).any()):
            raise ValueError("THETA is out of range [0,pi]")
        if p.numel() and not bool(torch.isfinite(p).all()):
            raise ValueError("phi must be finite")
        return t, p
    t, p = np.broadcast_arrays(np.asarray(theta, dtype=np.float64), np.asarray(phi, dtype=np.float64))
    if lonlat:
        t, p = np.pi / 2 - np.radians(p), np.radians(t)
    t, p = np.asarray(t, dtype=np.float64, order='C'), np.asarray(p, dtype=np.float64, order='C')       # (0-d stays 0-d)
    if t.size and not np.all((t >= 0) & (t <= np.pi)):
        raise ValueError("THETA is out of range [0,pi]")
    if p.size and not np.all(np.isfinite(p)):
        raise ValueError("phi must be finite")
    return t, p


def get_interp_weights(nside, theta, phi=None, nest=False, lonlat=False):
    """healpy.get_interp_weights: the 4 neighbours (int64) and bilinear weights (float64) of each point, shape (4,) + the points'
    shape.  With phi=None, theta holds pixel indices (RING, or NEST if nest) and the points are their centres.  lonlat=True:
    theta is the longitude and phi the latitude, in degrees.  nest=True needs a power-of-two nside; RING takes 1 <= nside <= 8192."""
    nside = check_nside(nside, bool(nest))
    npix = 12 * nside * nside
    device = _find_device(theta, phi)
    if phi is None:
        if device is not None:
            import torch
            ip = _like(theta, device)
            if ip.dtype.is_floating_point or ip.dtype.is_complex or ip.dtype == torch.bool:
                raise ValueError("with phi=None, theta must hold integer pixel indices")
            ip = ip.to(torch.int64).contiguous()
            if ip.numel() and (int(ip.min()) < 0 or int(ip.max()) >= npix):
                raise ValueError("pixel indices must be in [0, %d)" % npix)
        else:
            ip = np.asarray(theta)
            if ip.dtype.kind not in 'iu':
                raise ValueError("with phi=None, theta must hold integer pixel indices")
            ip = np.asarray(ip, dtype=np.int64, order='C')
            if ip.size and (ip.min() < 0 or ip.max() >= npix):
                raise ValueError("pixel indices must be in [0, %d)" % npix)
        shape, t, p = tuple(ip.shape), None, None
    else:
        t, p = _angles(theta, phi, lonlat, device)
        shape, ip = tuple(t.shape), None
    n = int(np.prod(shape, dtype=np.int64))
    if device is not None:
        import torch
        pix = torch.empty((4,) + shape, dtype=torch.int64, device=device)
        w = torch.empty((4,) + shape, dtype=torch.float64, device=device)
        ref = ip if ip is not None else t
        if n:
            _lib.call('bfgx_hpx_interp_weights_device', device_index(ref), stream(ref), nside, bool(nest), n, ptr(t), ptr(p), ptr(ip), ptr(pix),
                      ptr(w))
        return pix, w
    pix = np.empty((4,) + shape, dtype=np.int64)
    w = np.empty((4,) + shape, dtype=np.float64)
    if n:
        _lib.call('bfgx_hpx_interp_weights', 0, nside, bool(nest), n, ptr(t), ptr(p), ptr(ip), ptr(pix), ptr(w))
    return pix, w


def get_interp_val(m, theta, phi, nest=False, lonlat=False):
    """healpy.get_interp_val: sum_k m[pix_k] w_k with the weights of get_interp_weights, for one map (result of the points' shape)
    or several (nmaps, npix) (one row each).  The map's size sets nside; its ordering follows `nest`.  No UNSEEN masking (healpy
    has none either).  Maps of float32 are read as they are; the result is float64."""
    device = _find_device(m, theta, phi)
    if device is not None:
        import torch
        mm = _like(m, device)
        if mm.dtype not in (torch.float32, torch.float64):
            mm = mm.to(torch.float64)
        mm = mm.contiguous()
        dt = int(mm.dtype == torch.float64)
    else:
        mm = np.asarray(m)
        if mm.dtype not in (np.float32, np.float64):
            mm = mm.astype(np.float64)
        mm = np.ascontiguousarray(mm)
        dt = int(mm.dtype == np.float64)
    if mm.ndim not in (1, 2) or mm.shape[-1] == 0:
        raise ValueError("m must be one map (npix,) or several (nmaps, npix) (got shape %s)" % (tuple(mm.shape),))
    nside = check_nside(npix2nside(mm.shape[-1]), bool(nest))
    nmaps = 1 if mm.ndim == 1 else mm.shape[0]
    t, p = _angles(theta, phi, lonlat, device)
    shape = tuple(t.shape)
    n = int(np.prod(shape, dtype=np.int64))
    oshape = shape if mm.ndim == 1 else (nmaps,) + shape
    if device is not None:
        import torch
        out = torch.empty(oshape, dtype=torch.float64, device=device)
        if n:
            _lib.call('bfgx_hpx_interp_val_device', device_index(mm), stream(mm), nside, bool(nest), nmaps, dt, ptr(mm), n, ptr(t), ptr(p), ptr(out))
        return out
    out = np.empty(oshape, dtype=np.float64)
    if n:
        _lib.call('bfgx_hpx_interp_val', 0, nside, bool(nest), nmaps, dt, ptr(mm), n, ptr(t), ptr(p), ptr(out))
    return out[()] if out.ndim == 0 else out


# ------------------------------------------------------------------------------------------------------------- neighbours
def get_all_neighbours(nside, theta, phi=None, nest=False, lonlat=False):
    """healpy.get_all_neighbours of pixel indices: int64 of shape (8,) for one index or (8, N) for N, in healpy's order SW, W, NW,
    N, NE, E, SE, S, with -1 where a neighbour does not exist (24 entries of a whole map).  `theta` holds the indices (RING, or
    NEST if nest); angles (phi given) are not supported, as this package has no ang2pix.  nest=True needs a power-of-two nside;
    RING takes 1 <= nside <= 8192."""
    if phi is not None:
        raise NotImplementedError("get_all_neighbours takes pixel indices only (phi must be None: there is no ang2pix here)")
    nside = check_nside(nside, bool(nest))
    npix = 12 * nside * nside
    if is_cuda_tensor(theta):
        import torch
        ip = theta
        if ip.dtype.is_floating_point or ip.dtype.is_complex or ip.dtype == torch.bool:
            raise ValueError("theta must hold integer pixel indices")
        if ip.dim() > 1:
            raise ValueError("theta must be one pixel index or a 1-D array of them (got shape %s)" % (tuple(ip.shape),))
        ip = ip.to(torch.int64).contiguous()
        if ip.numel() and (int(ip.min()) < 0 or int(ip.max()) >= npix):
            raise ValueError("pixel indices must be in [0, %d)" % npix)
        out = torch.empty((8,) + tuple(ip.shape), dtype=torch.int64, device=ip.device)
        if ip.numel():
            _lib.call('bfgx_hpx_neighbours_device', device_index(ip), stream(ip), nside, bool(nest), ip.numel(), ptr(ip), ptr(out))
        return out
    ip = np.asarray(theta)
    if ip.dtype.kind not in 'iu':
        raise ValueError("theta must hold integer pixel indices")
    if ip.ndim > 1:
        raise ValueError("theta must be one pixel index or a 1-D array of them (got shape %s)" % (ip.shape,))
    ip = np.asarray(ip, dtype=np.int64, order='C')
    if ip.size and (ip.min() < 0 or ip.max() >= npix):
        raise ValueError("pixel indices must be in [0, %d)" % npix)
    out = np.empty((8,) + ip.shape, dtype=np.int64)
    if ip.size:
        _lib.call('bfgx_hpx_neighbours', 0, nside, bool(nest), ip.size, ptr(ip), ptr(out))
    return out


# ---------------------------------------------------------------------------------------------- regrid_pixels_hpix
def scatter_add(hmap, parent_pix_vals, child_pix, child_weights):
    """hmap[child_pix[i, j]] += child_weights[i, j] * parent_pix_vals[i] in place (Runners.regrid_pixels_hpix)"""
    on_dev = is_cuda_tensor(hmap)
    if on_dev:
        import torch
        if hmap.dtype != torch.float64 or hmap.dim() != 1 or not hmap.is_contiguous():
            raise ValueError("hmap must be a contiguous 1-D float64 tensor")
        dev = hmap.device
        vals, cp, cw = _like(parent_pix_vals, dev), _like(child_pix, dev), _like(child_weights, dev)
        int_pix = not (cp.dtype.is_floating_point or cp.dtype.is_complex or cp.dtype == torch.bool)
    else:
        if not (isinstance(hmap, np.ndarray) and hmap.dtype == np.float64 and hmap.ndim == 1 and hmap.flags.c_contiguous):
            raise ValueError("hmap must be a C-contiguous 1-D float64 numpy array or a CUDA float64 tensor")
        vals, cp, cw = np.asarray(parent_pix_vals), np.asarray(child_pix), np.asarray(child_weights)
        int_pix = cp.dtype.kind in 'iu'
    npix = int(hmap.shape[0])
    if npix < 1:
        raise ValueError("hmap is empty")
    if not int_pix:
        raise ValueError("child_pix must hold integers (got %s)" % cp.dtype)
    N = int(np.prod(tuple(vals.shape), dtype=np.int64))
    if vals.ndim != 1:
        raise ValueError("parent_pix_vals must be 1-D (got shape %s)" % (tuple(vals.shape),))
    for name, a in (('child_pix', cp), ('child_weights', cw)):
        if a.ndim == 2 and a.shape[0] == 4 and a.shape[1] != 4 and a.shape[1] == N:
            raise ValueError("%s has shape (4, N) (as healpy returns it); pass its transpose, shape (N, 4)" % name)
        if tuple(a.shape) != (N, 4):
            raise ValueError("%s must have shape (N, 4) = (%d, 4) (got %s)" % (name, N, tuple(a.shape)))
    if N:
        lo, hi = int(cp.min()), int(cp.max())
        if lo < -npix or hi >= npix:
            raise IndexError("child_pix holds index %d, outside [-%d, %d)" % (lo if lo < -npix else hi, npix, npix))
    if on_dev:
        import torch
        vals, cp, cw = vals.to(torch.float64).contiguous(), cp.to(torch.int64).contiguous(), cw.to(torch.float64).contiguous()
        if N:
            _lib.call('bfgx_hpx_scatter_add_device', device_index(hmap), stream(hmap), npix, ptr(hmap), N, ptr(vals), ptr(cp), ptr(cw))
        return hmap
    vals = np.ascontiguousarray(vals, dtype=np.float64)
    cp = np.ascontiguousarray(cp, dtype=np.int64)
    cw = np.ascontiguousarray(cw, dtype=np.float64)
    if N:
        _lib.call('bfgx_hpx_scatter_add', 0, npix, ptr(hmap), N, ptr(vals), ptr(cp), ptr(cw))
    return hmap
