"""Spherical-harmonic transforms of HEALPix shells and the mode-coupling matrices of a mask: the resident `ShtPlan` (CUDA tensors in
and out; torch is imported when one is made), the device entries on tensors, and the one-shot host entries on numpy arrays."""
import numpy as np

from .. import _lib, _tensors


def sht_alm_size(lmax, mmax):
    """complex coefficients of healpy's alm layout: index m (2 lmax + 1 - m) / 2 + l, 0 <= m <= mmax, m <= l <= lmax"""
    return (mmax + 1) * (2 * lmax + 2 - mmax) // 2


def _work_doubles(symbol, nside, lmax, mmax):
    """a *_work_doubles entry whose negative result means: refused, the reason in bfgx_last_error"""
    n = int(_lib.call(symbol, nside, lmax, mmax))
    if n < 0:
        raise ValueError(_lib.call('bfgx_last_error').decode('utf-8', 'replace'))
    return n


def sht_work_doubles(nside, lmax, mmax):
    """doubles of the transform workspace (ring geometry, Bluestein kernels, lambda_mm prefactors, F_m per ring, one scratch map)"""
    return _work_doubles('bfgx_sht_work_doubles', nside, lmax, mmax)


def sht_spin_work_doubles(nside, lmax, mmax):
    """doubles of the extra workspace of the spin transforms (F_m per ring of the second map)"""
    return _work_doubles('bfgx_sht_spin_work_doubles', nside, lmax, mmax)


class ShtPlan(object):
    """Resident spherical-harmonic transforms of one shape (nside, lmax, mmax) on one device: the workspace (ring geometry,
    Bluestein kernels of the ring FFTs, recurrence prefactors, per-ring F_m and a scratch map) is allocated and filled once;
    the transforms below then allocate only their outputs (or nothing, with out=)."""

    def __init__(self, nside, lmax, mmax, device=0):
        import torch
        self.nside, self.lmax, self.mmax, self.device = int(nside), int(lmax), int(mmax), int(device)
        self.npix = 12 * self.nside * self.nside
        self.nalm = sht_alm_size(self.lmax, self.mmax)
        nw = sht_work_doubles(self.nside, self.lmax, self.mmax)
        _tensors.need_gpu()
        self.dev = torch.device('cuda', self.device)
        self.work = torch.empty(nw, dtype=torch.float64, device=self.dev)
        self.spin_work = None                                 # F of a spin transform's second map, on the first spin call
        self.der_scratch = None                               # l-factors and scaled alm of alm2map_der_device, on its first call
        self._call('bfgx_sht_prepare_device', self.work.data_ptr())

    def _call(self, symbol, *args):
        """an entry of this plan's shape on torch's current stream: (device, stream, nside, lmax, mmax, *args)"""
        _lib.call(symbol, self.device, _tensors.stream(self.dev), self.nside, self.lmax, self.mmax, *args)

    def map2alm_device(self, map_dev, iter=3, out=None):
        """complex128 alm [nalm] of a float64 RING map [npix] on the device"""
        import torch
        alm = out if out is not None else torch.empty(self.nalm, dtype=torch.complex128, device=self.dev)
        self._call('bfgx_sht_map2alm_device', iter, map_dev.data_ptr(), alm.data_ptr(), self.work.data_ptr())
        return alm

    def alm2map_device(self, alm_dev, out=None):
        """float64 RING map [npix] of complex128 alm [nalm] on the device"""
        import torch
        m = out if out is not None else torch.empty(self.npix, dtype=torch.float64, device=self.dev)
        self._call('bfgx_sht_alm2map_device', alm_dev.data_ptr(), m.data_ptr(), self.work.data_ptr())
        return m

    def almxfl_device(self, alm_dev, fl_dev, out=None):
        """alm [nalm] times fl[l] (a float64 device tensor; fl[l] = 0 beyond its end): healpy.almxfl.  out=alm_dev filters in place"""
        return almxfl_device(alm_dev, fl_dev, self.lmax, self.mmax, out=out, device=self.device)

    def alm2cl_device(self, alm1_dev, alm2_dev=None, lmax_out=None, out=None):
        """cl [lmax_out + 1] (auto- or cross-spectrum) of device alm"""
        return alm2cl_device(alm1_dev, alm2_dev, self.lmax, self.mmax, lmax_out, out=out, device=self.device)

    def _spin_work(self):
        if self.spin_work is None:
            import torch
            self.spin_work = torch.empty(sht_spin_work_doubles(self.nside, self.lmax, self.mmax), dtype=torch.float64, device=self.dev)
        return self.spin_work

    def map2alm_spin_device(self, maps_dev, spin, out=None):
        """complex128 [G, C] [2, nalm] of a pair of float64 RING maps [2, npix] on the device (spin >= 1)"""
        import torch
        alms = out if out is not None else torch.empty((2, self.nalm), dtype=torch.complex128, device=self.dev)
        self._call('bfgx_sht_map2alm_spin_device', spin, maps_dev.data_ptr(), alms.data_ptr(), self.work.data_ptr(), self._spin_work().data_ptr())
        return alms

    def alm2map_spin_device(self, alms_dev, spin, out=None):
        """float64 RING maps [2, npix] of complex128 [G, C] [2, nalm] on the device (spin >= 1)"""
        import torch
        maps = out if out is not None else torch.empty((2, self.npix), dtype=torch.float64, device=self.dev)
        self._call('bfgx_sht_alm2map_spin_device', spin, alms_dev.data_ptr(), maps.data_ptr(), self.work.data_ptr(), self._spin_work().data_ptr())
        return maps

    def _der_scratch(self):
        """(fl [3, lmax + 1], alms [2, nalm]): the factors sqrt(l(l+1)), -l(l+1), -sqrt((l+2)(l+1)l(l-1)) that turn the alm of u into
        those of its gradient, Laplacian and trace-free Hessian, and one [G, C] pair whose C stays 0; made on the first call"""
        if self.der_scratch is None:
            import torch
            l = np.arange(self.lmax + 1, dtype=np.float64)
            fl = np.stack([np.sqrt(l * (l + 1.0)), -l * (l + 1.0), -np.sqrt((l + 2.0) * (l + 1.0) * l * np.maximum(l - 1.0, 0.0))])
            self.der_scratch = (torch.from_numpy(fl).to(self.dev), torch.zeros((2, self.nalm), dtype=torch.complex128, device=self.dev))
        return self.der_scratch

    def alm2map_der_device(self, alm_dev, out):
        """the derivatives of the map u of complex128 alm [nalm] in the orthonormal basis (e_theta, e_phi), written into the float64
        RING maps out [3, npix] = [u, u_t, u_p] (u_t = d_theta u, u_p = d_phi u / sin theta) or out [6, npix] = those and the second
        covariant derivatives in spin form, lap = u;tt + u;pp, q_plus = u;tt - u;pp, q_cross = 2 u;tp: one spin-0, one spin-1 and,
        for six maps, another spin-0 and one spin-2 synthesis of the scaled alm.  Nothing is allocated after the first call."""
        fl, pair = self._der_scratch()
        self.alm2map_device(alm_dev, out=out[0])
        if self.lmax >= 1:
            self.almxfl_device(alm_dev, fl[0], out=pair[0])
            self.alm2map_spin_device(pair, 1, out=out[1:3])
        else:
            out[1:3].zero_()
        if out.shape[0] == 6:
            self.almxfl_device(alm_dev, fl[1], out=pair[0])
            self.alm2map_device(pair[0], out=out[3])
            if self.lmax >= 2:
                self.almxfl_device(alm_dev, fl[2], out=pair[0])
                self.alm2map_spin_device(pair, 2, out=out[4:6])
            else:
                out[4:6].zero_()
        return out


def alm2cl_device(alm1_dev, alm2_dev, lmax, mmax, lmax_out=None, out=None, device=0):
    import torch
    lmax_out = int(lmax) if lmax_out is None else int(lmax_out)
    cl = out if out is not None else torch.empty(lmax_out + 1, dtype=torch.float64, device=alm1_dev.device)
    _lib.call('bfgx_sht_alm2cl_device', device, _tensors.stream(alm1_dev), lmax, mmax, lmax_out, alm1_dev.data_ptr(), _tensors.ptr(alm2_dev),
              cl.data_ptr())
    return cl


def almxfl_device(alm_dev, fl_dev, lmax, mmax, out=None, device=0):
    import torch
    res = out if out is not None else torch.empty_like(alm_dev)
    _lib.call('bfgx_sht_almxfl_device', device, _tensors.stream(alm_dev), lmax, mmax, fl_dev.numel(), fl_dev.data_ptr(), alm_dev.data_ptr(),
              res.data_ptr())
    return res


_SHT_PLANS = {}


def sht_plan(nside, lmax, mmax, device=0):
    """the cached ShtPlan of a shape: a repeated call of the same shape allocates no new workspace"""
    key = (int(nside), int(lmax), int(mmax), int(device))
    p = _SHT_PLANS.get(key)
    if p is None:
        p = _SHT_PLANS[key] = ShtPlan(*key)
    return p


def sht_map2alm_host(map_, nside, lmax, mmax, iter, device=0):
    """one-shot host entry (map and alm cross PCIe)"""
    alm = np.empty(sht_alm_size(lmax, mmax), dtype=np.complex128)
    _lib.call('bfgx_sht_map2alm', device, nside, lmax, mmax, iter, map_.ctypes.data, alm.ctypes.data)
    return alm


def sht_alm2map_host(alm, nside, lmax, mmax, device=0):
    m = np.empty(12 * int(nside) ** 2)
    a = np.ascontiguousarray(alm, dtype=np.complex128)
    _lib.call('bfgx_sht_alm2map', device, nside, lmax, mmax, a.ctypes.data, m.ctypes.data)
    return m


def sht_map2alm_spin_host(maps, nside, lmax, mmax, spin, device=0):
    """one-shot host entry of map2alm_spin: float64 [2, npix] in, complex128 [G, C] [2, nalm] out (PCIe included)"""
    m = np.ascontiguousarray(maps, dtype=np.float64)
    alms = np.empty((2, sht_alm_size(lmax, mmax)), dtype=np.complex128)
    _lib.call('bfgx_sht_map2alm_spin', device, nside, lmax, mmax, spin, m.ctypes.data, alms.ctypes.data)
    return alms


def sht_alm2map_spin_host(alms, nside, lmax, mmax, spin, device=0):
    """one-shot host entry of alm2map_spin: complex128 [G, C] [2, nalm] in, float64 [2, npix] out"""
    a = np.ascontiguousarray(alms, dtype=np.complex128)
    m = np.empty((2, 12 * int(nside) ** 2))
    _lib.call('bfgx_sht_alm2map_spin', device, nside, lmax, mmax, spin, a.ctypes.data, m.ctypes.data)
    return m


def sht_almxfl_host(alm, fl, lmax, mmax, out=None, device=0):
    """one-shot host entry of almxfl: complex128 alm and float64 fl in, the filtered alm out (`out` may be `alm`)"""
    res = out if out is not None else np.empty(sht_alm_size(lmax, mmax), dtype=np.complex128)
    _lib.call('bfgx_sht_almxfl', device, lmax, mmax, fl.size, fl.ctypes.data, alm.ctypes.data, res.ctypes.data)
    return res


def sht_alm2cl_host(alm1, alm2, lmax, mmax, lmax_out, device=0):
    a = np.ascontiguousarray(alm1, dtype=np.complex128)
    b = None if alm2 is None else np.ascontiguousarray(alm2, dtype=np.complex128)
    cl = np.empty(int(lmax_out) + 1)
    _lib.call('bfgx_sht_alm2cl', device, lmax, mmax, lmax_out, a.ctypes.data, _tensors.ptr(b), cl.ctypes.data)
    return cl


def sht_anafast_host(map1, map2, nside, lmax, mmax, iter, want_alm=False, device=0):
    cl = np.empty(int(lmax) + 1)
    n = sht_alm_size(lmax, mmax)
    a1 = np.empty(n, dtype=np.complex128) if want_alm else None
    a2 = np.empty(n, dtype=np.complex128) if (want_alm and map2 is not None) else None
    _lib.call('bfgx_sht_anafast', device, nside, lmax, mmax, iter, map1.ctypes.data, _tensors.ptr(map2), cl.ctypes.data, _tensors.ptr(a1),
              _tensors.ptr(a2))
    return cl, a1, a2


# ---------------------------------------------------------------------------------------------- mode-coupling matrices of a mask
PCL_MAX_LMAX, PCL_MAX_LW = 8191, 16383      # include/bfgx.h bfgx_pcl_coupling


def pcl_coupling_host(wl, lmax, kind, device=0):
    """one-shot host entry: float64 wl [lw + 1] in, the matrix [lmax + 1, lmax + 1] of kind 0 (M00) or 1 (M0+), or the pair (M++, M--) of
    kind 2, out (PCIe included)"""
    w = np.ascontiguousarray(wl, dtype=np.float64)
    n = int(lmax) + 1
    m0 = np.empty((n, n))
    m1 = np.empty_like(m0) if int(kind) == 2 else None
    _lib.call('bfgx_pcl_coupling', device, lmax, w.size - 1, kind, w.ctypes.data, m0.ctypes.data, _tensors.ptr(m1))
    return m0 if m1 is None else (m0, m1)


def pcl_coupling_device(wl_dev, lmax, kind, device=0):
    """the same on the device: wl_dev a contiguous float64 CUDA tensor, the matrices CUDA tensors; enqueued on torch's current stream.
    (utils.pseudocl checks lmax against PCL_MAX_LMAX before it comes here, so that a call the C entry refuses allocates nothing.)"""
    import torch
    n = int(lmax) + 1
    m0 = torch.empty((n, n), dtype=torch.float64, device=wl_dev.device)
    m1 = torch.empty_like(m0) if int(kind) == 2 else None
    _lib.call('bfgx_pcl_coupling_device', device, _tensors.stream(wl_dev), lmax, wl_dev.numel() - 1, kind, wl_dev.data_ptr(), m0.data_ptr(),
              _tensors.ptr(m1))
    return m0 if m1 is None else (m0, m1)
