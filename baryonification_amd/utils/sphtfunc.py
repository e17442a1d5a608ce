"""Spherical-harmonic transforms of RING-ordered HEALPix maps, named and defaulted after healpy.sphtfunc (healpy >= 1.16),
fp64, on the GPU (libbfgx: bfgx_sht_*).  `bfg.utils.anafast(shell_map)` replaces `hp.anafast(shell_map)`.

Inputs are numpy arrays (or anything np.asarray takes); results come back as numpy arrays.  A CUDA torch tensor is analysed
where it is, without crossing PCIe, and the results stay on the device as torch tensors.  Every call of one shape
(nside, lmax, mmax) reuses one cached engine.ShtPlan, so repeated calls allocate no new device workspace.

map2alm / alm2map / alm2cl / anafast are spin 0.  map2alm_spin / alm2map_spin transform a pair of real maps of spin s >= 1
in the HEALPix/libsharp convention:

    map0 + i map1 = -sum_{l >= s} sum_{m = -l..l} (G_lm + i C_lm) sY_lm(theta, phi),

G and C being the coefficients of real fields (X_{l,-m} = (-1)^m conj(X_lm); only m >= 0 is stored, in healpy's alm layout).
sY_lm = sqrt((l - s)! / (l + s)!) edth^s Y_lm, with edth eta = -(sin theta)^s (d_theta + (i / sin theta) d_phi)[(sin theta)^-s eta]
for a spin-s quantity eta and Y_lm the Condon-Shortley harmonic (scipy.special.sph_harm_y).  For s = 2, (map0, map1) = (Q, U)
and (G, C) = (E, B) in HEALPix's polarisation convention.  The analysis is plain quadrature, as healpy's (no iterations).

Convergence to shear (Kaiser-Squires) on a shell map kappa:

    klm = map2alm(kappa, iter=0)                      # or iter=3
    l = l-index of every coefficient (healpy.Alm.getlm)
    elm = sqrt((l + 2) (l - 1) / (l (l + 1))) klm     # 0 for l < 2
    gamma1, gamma2 = alm2map_spin([elm, 0 * elm], nside, 2, lmax)

and back: E, B = map2alm_spin([gamma1, gamma2], 2); alm2cl(E), alm2cl(B), alm2cl(E, B) are the E/B spectra.

Filters in harmonic space: gauss_beam / tophat_beam are windows W_l (host numpy), almxfl multiplies alm by one on the GPU, and
smoothalm / smoothing are healpy's (smoothing = map2alm, almxfl, alm2map on the cached plan of the shape; a single RING map).

Derivatives of the band-limited map u of a set of alm, in the orthonormal basis (e_theta, e_phi): alm2map_der1 is healpy's
([u, d_theta u, d_phi u / sin theta]); alm2map_der2 adds the second covariant derivatives
    u;tt = d_theta^2 u,   u;tp = d_theta d_phi u / sin - cos d_phi u / sin^2,   u;pp = d_phi^2 u / sin^2 + cos d_theta u / sin.
They are syntheses of scaled alm in the spin convention above: spin 1 of [sqrt(l(l+1)) a, 0] is (u_t, u_p), spin 2 of
[-sqrt((l+2)(l+1)l(l-1)) a, 0] is (u;tt - u;pp, 2 u;tp), and spin 0 of -l(l+1) a is the Laplacian u;tt + u;pp.
"""
import numpy as np

from .. import engine
from .._tensors import is_cuda_tensor, device_index
from .io import npix2nside

__all__ = ['map2alm', 'alm2map', 'alm2cl', 'anafast', 'map2alm_spin', 'alm2map_spin', 'getlmax', 'getidx', 'getsize', 'UNSEEN',
           'gauss_beam', 'tophat_beam', 'almxfl', 'smoothalm', 'smoothing', 'alm2map_der1', 'alm2map_der2']

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


def _unsupported(**kw):
    for name, (value, default) in kw.items():
        if value is not default and value != default:
            raise NotImplementedError("%s=%r is not supported (spin-0 transforms without healpy's data files)" % (name, value))


def _map_input(maps, name='maps'):
    """(1-D float64 map, nside, on_device)"""
    if is_cuda_tensor(maps):
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
    if is_cuda_tensor(alms):
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
        return engine.alm2cl_device(a, b, lmax, mmax, lmax_out, device=device_index(a))
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


def _spin_check(spin, lmax):
    spin = int(spin)
    if spin < 1:
        raise ValueError("spin must be >= 1 (got %d); spin-0 transforms are map2alm / alm2map" % spin)
    if spin > lmax:
        raise ValueError("spin must be <= lmax (got spin %d, lmax %d)" % (spin, lmax))
    return spin


def _pair(x, name):
    """the two members of a map or alm pair: a (2, n) array or tensor, or a sequence of two 1-D ones"""
    if is_cuda_tensor(x) or isinstance(x, np.ndarray):
        if x.ndim != 2 or x.shape[0] != 2:
            raise ValueError("%s must hold 2 %s (got shape %s)" % (name, 'maps' if name == 'maps' else 'sets of alm', tuple(x.shape)))
        return x[0], x[1]
    if isinstance(x, (list, tuple)):
        if len(x) != 2:
            raise ValueError("%s must hold 2 %s (got %d)" % (name, 'maps' if name == 'maps' else 'sets of alm', len(x)))
        return x[0], x[1]
    return _pair(np.asarray(x), name)


def _size(x):
    return x.numel() if is_cuda_tensor(x) else np.asarray(x).size


def map2alm_spin(maps, spin, lmax=None, mmax=None):
    """[G, C] (complex128 [2, nalm], healpy order) of a pair of RING maps [map0, map1] of spin `spin` >= 1 (plain quadrature:
    G + i C = -4 pi / Npix sum_p (map0 + i map1)_p sY*_lm(p)).  Output alm with l < spin are 0.  UNSEEN pixels count as 0."""
    m0, m1 = _pair(maps, 'maps')
    if _size(m0) != _size(m1):
        raise ValueError("maps: map0 and map1 have different sizes (%d, %d)" % (_size(m0), _size(m1)))
    a, nside, on_dev = _map_input(m0, 'maps[0]')
    b, _, d1 = _map_input(m1, 'maps[1]')
    if d1 != on_dev:
        raise ValueError("maps: map0 and map1 must both be on the host or both on the device")
    lmax, mmax = _shape(nside, lmax, mmax)
    spin = _spin_check(spin, lmax)
    plan = engine.sht_plan(nside, lmax, mmax)
    if on_dev:
        import torch
        alms = plan.map2alm_spin_device(torch.stack([a, b]), spin)
        return alms
    alms = plan.map2alm_spin_device(_to_device(np.stack([a, b]), plan), spin)
    return alms.cpu().numpy()


def alm2map_spin(alms, nside, spin, lmax, mmax=None):
    """float64 RING maps [map0, map1] ([2, npix]) of [G, C] of spin `spin` >= 1:
    map0 + i map1 = -sum_{l >= spin} sum_m (G_lm + i C_lm) sY_lm.  Input alm with l < spin are ignored."""
    g, c = _pair(alms, 'alms')
    if _size(g) != _size(c):
        raise ValueError("alms: the two sets of alm have different sizes (%d, %d)" % (_size(g), _size(c)))
    a, lmax, mmax, on_dev = _alm_input(g, lmax, mmax, 'alms[0]')
    b, _, _, d1 = _alm_input(c, lmax, mmax, 'alms[1]')
    if d1 != on_dev:
        raise ValueError("alms: the two sets of alm must both be on the host or both on the device")
    nside = int(nside)
    if nside < 1:
        raise ValueError("nside must be >= 1")
    _shape(nside, lmax, mmax)
    spin = _spin_check(spin, lmax)
    plan = engine.sht_plan(nside, lmax, mmax)
    if on_dev:
        import torch
        return plan.alm2map_spin_device(torch.stack([a, b]), spin)
    return plan.alm2map_spin_device(_to_device(np.stack([a, b]), plan), spin).cpu().numpy()


# -------------------------------------------------------------------------------------------------------------- derivatives
def _alm2map_der(alm, nside, lmax, mmax, nmaps):
    a, lmax, mmax, on_dev = _alm_input(alm, lmax, mmax, 'alm')
    nside = int(nside)
    if nside < 1:
        raise ValueError("nside must be >= 1")
    _shape(nside, lmax, mmax)
    plan = engine.sht_plan(nside, lmax, mmax, device=device_index(a) if on_dev else 0)
    import torch
    out = torch.empty((nmaps, plan.npix), dtype=torch.float64, device=plan.dev)
    return plan.alm2map_der_device(a if on_dev else _to_device(a, plan), out), on_dev


def alm2map_der1(alm, nside, lmax=None, mmax=None):
    """healpy.alm2map_der1: float64 RING maps [3, npix] = [m, d_theta m, d_phi m / sin(theta)] of one set of alm (nside <= 2048).
    A CUDA complex128 tensor gives a CUDA result."""
    out, on_dev = _alm2map_der(alm, nside, lmax, mmax, 3)
    return out if on_dev else out.cpu().numpy()


def alm2map_der2(alm, nside, lmax=None, mmax=None, spin_form=False):
    """float64 RING maps [6, npix] = [u, u_t, u_p, u;tt, u;tp, u;pp] of one set of alm (nside <= 2048): the map, its gradient
    (u_t = d_theta u, u_p = d_phi u / sin theta) and its second covariant derivatives in the orthonormal basis (e_theta, e_phi).
    With spin_form=True the last three are, as synthesised, lap = u;tt + u;pp, q_plus = u;tt - u;pp and q_cross = 2 u;tp (what
    minkowski_from_derivatives(spin_form=True) reads).  A CUDA complex128 tensor gives a CUDA result."""
    out, on_dev = _alm2map_der(alm, nside, lmax, mmax, 6)
    if not spin_form:
        lap, qp = out[3].clone(), out[4].clone()
        out[3], out[4], out[5] = 0.5 * (lap + qp), 0.5 * out[5], 0.5 * (lap - qp)
    return out if on_dev else out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------- harmonic filters
def gauss_beam(fwhm, lmax=512, pol=False):
    """healpy.gauss_beam: exp(-l (l + 1) sigma^2 / 2), l = 0..lmax, sigma = fwhm / sqrt(8 ln 2) (fwhm in radians)"""
    if pol:
        raise NotImplementedError("pol=True is not supported (spin-0 window only)")
    lmax = int(lmax)
    if lmax < 0:
        raise ValueError("lmax must be >= 0 (got %d)" % lmax)
    return _gauss_window(float(fwhm) / np.sqrt(8.0 * np.log(2.0)), lmax)


def _gauss_window(sigma, lmax):
    ell = np.arange(lmax + 1, dtype=np.float64)
    return np.exp(-0.5 * ell * (ell + 1.0) * sigma * sigma)


def tophat_beam(radius, lmax):
    """The harmonic window of a disc of angular radius `radius` (radians, in [0, pi]): W_0 = 1 and, with mu = cos(radius),
    W_l = (1 + mu) P'_l(mu) / (l (l + 1)), which equals the textbook (P_{l-1} - P_{l+1}) / ((2l + 1) (1 - mu)) without its
    cancellation at small radii.  P'_l comes from the upward recurrence l P'_{l+1} = (2l + 1) mu P'_l - (l + 1) P'_{l-1}, run on
    the differences D_l = P'_l - P'_{l-1} with t = 1 - mu = 2 sin^2(radius / 2):  l D_{l+1} = (l + 1) D_l - (2l + 1) t P'_l, so an
    arc-minute radius is not lost in the rounding of cos(radius) to fp64.  Host numpy, fp64; radius 0 gives all ones."""
    lmax = int(lmax)
    radius = float(radius)
    if lmax < 0:
        raise ValueError("lmax must be >= 0 (got %d)" % lmax)
    if not 0.0 <= radius <= np.pi:
        raise ValueError("radius must be in [0, pi] (got %r)" % radius)
    t = 2.0 * np.sin(0.5 * radius) ** 2
    onepmu = 2.0 * np.cos(0.5 * radius) ** 2
    w = np.ones(lmax + 1)
    dp, d = 1.0, 1.0                                       # P'_1, D_1
    for l in range(1, lmax + 1):
        w[l] = onepmu * dp / (l * (l + 1.0))
        d = ((l + 1.0) * d - (2.0 * l + 1.0) * t * dp) / l
        dp = dp + d
    return w


def _window(lmax, fwhm, sigma, beam_window):
    """fl[0..lmax] of smoothalm / smoothing: beam_window wins over sigma, sigma over fwhm"""
    if beam_window is not None:
        fl = np.asarray(beam_window, dtype=np.float64)
        if fl.ndim != 1:
            raise ValueError("beam_window must be 1-D (got shape %s)" % (fl.shape,))
        return np.ascontiguousarray(fl)
    return gauss_beam(fwhm, lmax) if sigma is None else _gauss_window(float(sigma), lmax)


def _fl_input(fl):
    if is_cuda_tensor(fl):
        if fl.dim() != 1 or fl.dtype.is_complex:
            raise ValueError("fl must be a 1-D real array")
        return fl
    f = np.asarray(fl)
    if f.ndim != 1 or not (np.issubdtype(f.dtype, np.floating) or np.issubdtype(f.dtype, np.integer)):
        raise ValueError("fl must be a 1-D real array (got dtype %s, shape %s)" % (f.dtype, f.shape))
    return np.ascontiguousarray(f, dtype=np.float64)


def _fl_device(fl, dev):
    """fl as a float64 tensor on dev with at least one element (an empty fl filters everything to 0)"""
    import torch
    f = fl if is_cuda_tensor(fl) else torch.from_numpy(fl)
    f = f.to(device=dev, dtype=torch.float64).contiguous()
    return f if f.numel() else torch.zeros(1, dtype=torch.float64, device=dev)


def almxfl(alm, fl, mmax=None, inplace=False):
    """healpy.almxfl: alm[idx(l, m)] * fl[l] on the GPU.  fl is real; fl[l] counts as 0 for l >= len(fl), entries beyond lmax are
    ignored.  A CUDA complex128 tensor is filtered where it lies (in place with inplace=True); a numpy array goes through the
    one-shot host entry (inplace=True needs a C-contiguous complex128 array, as healpy does)."""
    f = _fl_input(fl)
    a, lmax, mmax, on_dev = _alm_input(alm, None, mmax, 'alm')
    if on_dev:
        if inplace and (a is not alm and a.data_ptr() != alm.data_ptr()):
            raise ValueError("inplace=True needs a contiguous 1-D complex128 tensor")
        out = engine.almxfl_device(a, _fl_device(f, a.device), lmax, mmax, out=a if inplace else None, device=device_index(a))
        return alm if inplace else out
    if inplace and not (isinstance(alm, np.ndarray) and np.shares_memory(a, alm)):
        raise ValueError("inplace=True needs a C-contiguous 1-D complex128 numpy array")
    if is_cuda_tensor(f):
        f = f.cpu().numpy().astype(np.float64)
    if f.size == 0:
        f = np.zeros(1)
    res = engine.sht_almxfl_host(a, f, lmax, mmax, out=a if inplace else None)
    return alm if inplace else res


def smoothalm(alms, fwhm=0.0, sigma=None, beam_window=None, pol=True, mmax=None, verbose=True, inplace=True):
    """healpy.smoothalm of one set of alm: almxfl with beam_window, else the Gaussian of sigma, else that of fwhm (radians)"""
    a, lmax, mmax, on_dev = _alm_input(alms, None, mmax)
    return almxfl(alms, _window(lmax, fwhm, sigma, beam_window), mmax=mmax, inplace=inplace)


def unseen_mask(m):
    """healpy.mask_bad: |m - UNSEEN| <= 1e-8 + 1e-5 |UNSEEN| (numpy array or torch tensor)"""
    return abs(m - UNSEEN) <= 1e-8 + 1e-5 * abs(UNSEEN)


def smoothing(map_in, fwhm=0.0, sigma=None, beam_window=None, pol=True, iter=3, lmax=None, mmax=None, use_weights=False,
              use_pixel_weights=False, datapath=None, verbose=True, nest=False):
    """healpy.smoothing of a single RING map (nside <= 2048): alm2map(almxfl(map2alm(map_in, iter), W)) on the cached plan of the
    shape, W = beam_window, else the Gaussian of sigma, else that of fwhm (radians).  UNSEEN pixels count as 0 on the way in and
    are UNSEEN again in the result.  A CUDA tensor stays on its device."""
    _unsupported(nest=(nest, False), use_weights=(use_weights, False), use_pixel_weights=(use_pixel_weights, False),
                 datapath=(datapath, None))
    m, nside, on_dev = _map_input(map_in, 'map_in')
    lmax, mmax = _shape(nside, lmax, mmax)
    if int(iter) < 0:
        raise ValueError("iter must be >= 0")
    fl = _window(lmax, fwhm, sigma, beam_window)
    plan = engine.sht_plan(nside, lmax, mmax)
    md = m if on_dev else _to_device(m, plan)
    alm = plan.map2alm_device(md, iter=int(iter))
    plan.almxfl_device(alm, _fl_device(fl, plan.dev), out=alm)
    out = plan.alm2map_device(alm)
    out.masked_fill_(unseen_mask(md), UNSEEN)
    return out if on_dev else out.cpu().numpy()
