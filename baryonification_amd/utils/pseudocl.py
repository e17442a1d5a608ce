"""Power spectra of masked shells: pseudo-C_l, the mode-coupling matrices of the mask (GPU: libbfgx bfgx_pcl_coupling) and the
binned, decoupled bandpowers that follow from them (the MASTER estimator; Hivon et al. 2002, Alonso et al. 2019 for spin 2).

`anafast(shell * mask)` is the pseudo-C_l: the true spectrum mixed across multipoles by the mask.  With W_l the (cross-)spectrum of the
mask(s), (l l' l''; a b c) the Wigner 3j symbol and L = l + l' + l'',

    M00[l,l'] = (2l'+1)/(4 pi) sum_l'' (2l''+1) W_l'' (l l' l''; 0 0 0)^2
    M0+[l,l'] = (2l'+1)/(4 pi) sum_l'' (2l''+1) W_l'' (l l' l''; 0 0 0) (l l' l''; 2 -2 0)
    M++[l,l'] = (2l'+1)/(4 pi) sum_l'' (2l''+1) W_l'' (l l' l''; 2 -2 0)^2  over even L,      M--: the same over odd L

give <pcl^00> = M00 C^00, <pcl^0E> = M0+ C^0E (and 0B), <pcl^EE> = M++ C^EE + M-- C^BB, <pcl^BB> = M-- C^EE + M++ C^BB and
<pcl^EB> = (M++ - M--) C^EB (and BE).  Spectra are stacked in the order [00], [0E, 0B] or [EE, EB, BE, BB].

Baryonic suppression on a survey footprint, the workspace computed once:

    ws = PseudoClWorkspace(mask, bins=ClBins.linear(2, 3 * nside - 1, 16))
    ratio = decoupled_cl(shell_bfg, mask1=mask, workspace=ws)['cl'] / decoupled_cl(shell_dmo, mask1=mask, workspace=ws)['cl']

numpy in, numpy out; CUDA float64 tensors stay on their device (the coupling matrices then never cross PCIe).  Maps are RING ordered.
A spin-2 field is a pair (q, u) as map2alm_spin takes it.  No purification, no noise bias, no covariance."""
import numpy as np

from .. import engine
from .._tensors import is_cuda_tensor, device_index
from . import sphtfunc
from .sphtfunc import _map_input

__all__ = ['mode_coupling_matrix', 'mask_spectrum', 'ClBins', 'pseudo_cl', 'PseudoClWorkspace', 'decoupled_cl']

_KIND = {(0, 0): 0, (0, 2): 1, (2, 0): 1, (2, 2): 2}
_NSPEC = {0: 1, 1: 2, 2: 4}


def _spins(spin1, spin2):
    if (spin1, spin2) not in _KIND:
        raise NotImplementedError("spins (%r, %r): spin 0 and spin 2 are supported" % (spin1, spin2))
    return _KIND[(spin1, spin2)]


def _no_nest(nest):
    if nest:
        raise NotImplementedError("NEST ordering is not supported: the transforms take RING maps (reorder first)")


def _check_lmax(lmax):
    try:
        n = int(lmax)
    except (TypeError, ValueError):
        raise ValueError("lmax must be an integer (got %r)" % (lmax,))
    if n != lmax or not 0 <= n <= engine.PCL_MAX_LMAX:
        raise ValueError("lmax must be in [0, %d] (got %r)" % (engine.PCL_MAX_LMAX, lmax))
    return n


def mode_coupling_matrix(wl, lmax, spin1=0, spin2=0):
    """The mode-coupling matrix, float64 [lmax + 1, lmax + 1], of the mask spectrum wl = W_0 .. W_lw (0 beyond): M00 for spins (0, 0),
    M0+ for (0, 2) or (2, 0), the pair (M++, M--) for (2, 2); 0 <= lmax <= 8191.  Spin-2 rows and columns below 2 and entries with
    |l - l'| > lw are exactly 0.  A CUDA float64 tensor gives CUDA results."""
    kind = _spins(spin1, spin2)
    lmax = _check_lmax(lmax)
    on_dev = is_cuda_tensor(wl)
    if on_dev:
        import torch
        if wl.dim() != 1 or wl.numel() < 1 or wl.dtype != torch.float64:
            raise ValueError("wl must be a non-empty 1-D float64 array (got dtype %s, shape %s)" % (wl.dtype, tuple(wl.shape)))
        return engine.pcl_coupling_device(wl[:2 * lmax + 1].contiguous(), lmax, kind, device=device_index(wl))
    w = np.asarray(wl)
    if w.ndim != 1 or w.size < 1 or not (np.issubdtype(w.dtype, np.floating) or np.issubdtype(w.dtype, np.integer)):
        raise ValueError("wl must be a non-empty 1-D real array (got dtype %s, shape %s)" % (w.dtype, w.shape))
    # (l'' <= l + l' <= 2 lmax: what lies beyond is never read)
    return engine.pcl_coupling_host(np.ascontiguousarray(w[:2 * lmax + 1], dtype=np.float64), lmax, kind)


def _mask_lmax(nside, lmax):
    return min(2 * lmax, 3 * nside - 1)


def mask_spectrum(mask1, mask2=None, lmax=None, nest=False):
    """W_l, l = 0 .. lmax (default 3 nside - 1), of a mask or the cross-spectrum of two: anafast of the mask(s)"""
    _no_nest(nest)
    return sphtfunc.anafast(mask1, mask2, lmax=lmax)


class ClBins(object):
    """Contiguous multipole bins [e_b, e_{b+1}) with uniform weights: `edges` are nb + 1 ascending integers >= 0.
    ell[b] is the effective (mean) multipole of bin b, lmax the last multipole binned.  Pure host arithmetic."""

    def __init__(self, edges):
        e = np.asarray(edges)
        if e.ndim != 1 or e.size < 2:
            raise ValueError("edges must be a 1-D array of at least 2 bin edges")
        if not np.all(np.isfinite(e)) or not np.all(e == np.floor(e)):
            raise ValueError("edges must be integers")
        e = e.astype(np.int64)
        if e[0] < 0 or not np.all(np.diff(e) > 0):
            raise ValueError("edges must be >= 0 and strictly ascending")
        self.edges = e
        self.nbins = e.size - 1
        self.lmin, self.lmax = int(e[0]), int(e[-1]) - 1
        self.width = np.diff(e).astype(np.float64)
        self.ell = 0.5 * (e[:-1] + e[1:] - 1.0)

    @classmethod
    def linear(cls, lmin, lmax, nlb):
        """bins of nlb multipoles from lmin; what is left over below lmax + 1 is not binned"""
        lmin, lmax, nlb = int(lmin), int(lmax), int(nlb)
        if nlb < 1 or lmin < 0 or lmax - lmin + 1 < nlb:
            raise ValueError("need nlb >= 1, lmin >= 0 and at least one whole bin in [lmin, lmax] (got lmin %d, lmax %d, nlb %d)" % (lmin, lmax, nlb))
        return cls(lmin + nlb * np.arange((lmax + 1 - lmin) // nlb + 1))

    def bin_index(self, lmax):
        """int64 [lmax + 1]: the bin of every multipole, -1 outside the bins"""
        idx = np.full(int(lmax) + 1, -1, dtype=np.int64)
        for b in range(self.nbins):
            idx[self.edges[b]:self.edges[b + 1]] = b
        return idx

    def matrix(self, lmax):
        """B, float64 [nbins, lmax + 1]: B[b, l] = 1 / (e_{b+1} - e_b) on the bin"""
        self._fits(lmax)
        B = np.zeros((self.nbins, int(lmax) + 1))
        for b in range(self.nbins):
            B[b, self.edges[b]:self.edges[b + 1]] = 1.0 / self.width[b]
        return B

    def _fits(self, lmax):
        if self.lmax > int(lmax):
            raise ValueError("the bins reach l = %d, beyond lmax = %d" % (self.lmax, int(lmax)))

    def bin_cell(self, cl):
        """the mean of cl[..., l] over each bin -> [..., nbins] (numpy)"""
        cl = np.asarray(cl, dtype=np.float64)
        self._fits(cl.shape[-1] - 1)
        return cl @ self.matrix(cl.shape[-1] - 1).T

    def unbin_cell(self, cb, lmax=None):
        """the step function: cb[..., b] on each bin, 0 outside -> [..., lmax + 1] (lmax defaults to the bins' own)"""
        cb = np.asarray(cb, dtype=np.float64)
        lmax = self.lmax if lmax is None else int(lmax)
        self._fits(lmax)
        if cb.shape[-1] != self.nbins:
            raise ValueError("cb has %d bins, the binning %d" % (cb.shape[-1], self.nbins))
        idx = self.bin_index(lmax)
        return np.where(idx >= 0, cb[..., np.maximum(idx, 0)], 0.0)


def _field(f, name):
    """(spin, [maps], nside, on_device) of a field: one map (spin 0) or a pair (q, u) (spin 2)"""
    pair = isinstance(f, (list, tuple)) or (getattr(f, 'ndim', 1) == 2 and f.shape[0] == 2)
    if isinstance(f, (list, tuple)) and len(f) != 2:
        raise ValueError("%s: a field is one map (spin 0) or a pair (q, u) (spin 2), got %d maps" % (name, len(f)))
    if not pair:
        m, nside, on_dev = _map_input(f, name)
        return 0, [m], nside, on_dev
    q, nside, on_dev = _map_input(f[0], name + '[0]')
    u, nside_u, dev_u = _map_input(f[1], name + '[1]')
    if nside_u != nside:
        raise ValueError("%s: q and u have different nside (%d, %d)" % (name, nside, nside_u))
    if dev_u != on_dev:
        raise ValueError("%s: q and u must both be on the host or both on the device" % name)
    return 2, [q, u], nside, on_dev


def _mask(mask, nside, on_dev, name):
    if mask is None:
        return None
    m, ns, dev = _map_input(mask, name)
    if ns != nside:
        raise ValueError("%s has nside %d, the map nside %d" % (name, ns, nside))
    if dev != on_dev:
        raise ValueError("%s and the maps must both be on the host or both on the device" % name)
    return m


def _alms(spin, maps, mask, lmax, iter, on_dev):
    """the alm of a masked field: [a] for spin 0, [E, B] for spin 2"""
    if mask is not None:
        maps = [m * mask for m in maps]
    if spin == 0:
        return [sphtfunc.map2alm(maps[0], lmax=lmax, iter=iter)]
    if on_dev:
        import torch
        eb = sphtfunc.map2alm_spin(torch.stack(maps), 2, lmax=lmax)
    else:
        eb = sphtfunc.map2alm_spin(np.stack(maps), 2, lmax=lmax)
    return [eb[0], eb[1]]


def _fields(f1, f2, mask1, mask2):
    s1, m1, nside, on_dev = _field(f1, 'f1')
    if f2 is None:
        s2, m2 = s1, None
    else:
        s2, m2, nside2, dev2 = _field(f2, 'f2')
        if nside2 != nside:
            raise ValueError("f1 and f2 have different nside (%d, %d)" % (nside, nside2))
        if dev2 != on_dev:
            raise ValueError("f1 and f2 must both be on the host or both on the device")
    k1 = _mask(mask1, nside, on_dev, 'mask1')
    k2 = k1 if mask2 is None else _mask(mask2, nside, on_dev, 'mask2')
    return s1, s2, m1, m2, k1, k2, nside, on_dev


def _pseudo_cl(s1, s2, m1, m2, k1, k2, lmax, iter, on_dev):
    a = _alms(s1, m1, k1, lmax, iter, on_dev)
    b = a if (m2 is None and k2 is k1) else _alms(s2, m1 if m2 is None else m2, k2, lmax, iter, on_dev)
    if s1 == 2 and s2 == 0:                                         # [E0, B0]
        cls = [sphtfunc.alm2cl(x, b[0], lmax=lmax) for x in a]
    else:
        cls = [sphtfunc.alm2cl(x, y, lmax=lmax) for x in a for y in b]
    if on_dev:
        import torch
        return torch.stack(cls)
    return np.stack(cls)


def _iter(iter):
    if int(iter) < 0:
        raise ValueError("iter must be >= 0")
    return int(iter)


def _lmax_of(nside, lmax):
    return _check_lmax(3 * nside - 1 if lmax is None else lmax)


def pseudo_cl(f1, f2=None, mask1=None, mask2=None, lmax=None, iter=3, nest=False):
    """The pseudo-C_l of masked fields, float64 [ns, lmax + 1]: each field (f2 defaults to f1, mask2 to mask1) is multiplied by its mask
    and transformed (spin 0: map2alm with `iter` iterations; spin 2: map2alm_spin, plain quadrature), and the spectra are stacked as
    [00], [0E, 0B] (or [E0, B0]) or [EE, EB, BE, BB].  lmax defaults to 3 nside - 1."""
    _no_nest(nest)
    s1, s2, m1, m2, k1, k2, nside, on_dev = _fields(f1, f2, mask1, mask2)
    return _pseudo_cl(s1, s2, m1, m2, k1, k2, _lmax_of(nside, lmax), _iter(iter), on_dev)


class PseudoClWorkspace(object):
    """The coupling matrices of a mask (or a pair of masks) for fields of spins (spin1, spin2), computed once on the GPU, and the factored
    binned matrix BM = B M U (B the bin average, U the step function of `bins`).  numpy in, numpy out; a CUDA tensor gives a CUDA result.

      coupling_matrix()     M00, M0+ or (M++, M--)
      couple(cl)            theory C_l [ns, lmax + 1] -> the expected pseudo-C_l
      decouple(pcl)         pseudo-C_l [ns, lmax + 1] -> bandpowers BM^-1 B pcl, [ns, nbins]
      bandpower_windows()   BM^-1 B M, [ns, nbins, ns, lmax + 1]: bandpowers = windows . C_l
      fsky, wl, ell         mean of mask1 mask2, the mask spectrum the matrices were made from, the bins' effective multipoles

    ns = 1 ([00]), 2 ([0E, 0B]) or 4 ([EE, EB, BE, BB]); for ns = 1 a 1-D cl is taken and a 1-D result returned."""

    def __init__(self, mask1, mask2=None, spin1=0, spin2=0, bins=None, lmax=None, nest=False):
        _no_nest(nest)
        self.kind = _spins(spin1, spin2)
        self.spins = (spin1, spin2)
        self.ns = _NSPEC[self.kind]
        if not isinstance(bins, ClBins):
            raise ValueError("bins must be a ClBins")
        k1, nside, on_dev = _map_input(mask1, 'mask1')
        k2 = None if mask2 is None else _mask(mask2, nside, on_dev, 'mask2')
        self.nside, self.lmax = nside, _lmax_of(nside, lmax)
        bins._fits(self.lmax)
        self.bins, self.ell = bins, bins.ell
        import torch
        wl = mask_spectrum(k1, k2, lmax=_mask_lmax(nside, self.lmax))
        self._wl = wl if on_dev else torch.from_numpy(wl).to(torch.device('cuda', 0))
        dev = self._wl.device
        self.fsky = float((k1 * (k1 if k2 is None else k2)).mean())
        mats = engine.pcl_coupling_device(self._wl.contiguous(), self.lmax, self.kind, device=device_index(dev))
        self._mats = mats if self.kind == 2 else (mats,)
        self._B = torch.from_numpy(bins.matrix(self.lmax)).to(dev)                               # [nb, n]
        U = (self._B > 0).to(torch.float64).T.contiguous()                                        # [n, nb]
        self._BM = [self._B @ m for m in self._mats]                                              # B M of each matrix, [nb, n]
        self._binned = self._blocks([bm @ U for bm in self._BM])                                  # [ns nb, ns nb]
        self._lu = torch.linalg.lu_factor(self._binned)

    @property
    def wl(self):
        return self._wl.cpu().numpy()

    def _blocks(self, m):
        """the coupling of the stacked spectra from the matrices m = [M] or [M++, M--] (any common shape [r, c]) -> [ns r, ns c]"""
        import torch
        if self.kind == 0:
            return m[0]
        Z = torch.zeros_like(m[0])
        if self.kind == 1:
            return torch.cat([torch.cat([m[0], Z], 1), torch.cat([Z, m[0]], 1)], 0)
        p, q, d = m[0], m[1], m[0] - m[1]
        return torch.cat([torch.cat([p, Z, Z, q], 1), torch.cat([Z, d, Z, Z], 1), torch.cat([Z, Z, d, Z], 1), torch.cat([q, Z, Z, p], 1)], 0)

    def _in(self, x, name):
        """(float64 [ns, lmax + 1] on the workspace's device, as given: on_device, 1-D)"""
        import torch
        on_dev = is_cuda_tensor(x)
        t = x if on_dev else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
        flat = t.dim() == 1
        if flat:
            t = t.unsqueeze(0)
        if t.dim() != 2 or tuple(t.shape) != (self.ns, self.lmax + 1):
            raise ValueError("%s must have shape [%d, %d] (got %s)" % (name, self.ns, self.lmax + 1, tuple(x.shape)))
        return t.to(device=self._wl.device, dtype=torch.float64), on_dev, flat

    @staticmethod
    def _out(t, on_dev, flat):
        t = t[0] if flat else t
        return t if on_dev else t.cpu().numpy()

    def coupling_matrix(self, device=False):
        """M00 or M0+ [lmax + 1, lmax + 1], or (M++, M--); numpy unless device=True (the CUDA tensors the workspace holds)"""
        out = self._mats if device else tuple(m.cpu().numpy() for m in self._mats)
        return out if self.kind == 2 else out[0]

    def couple(self, cl):
        t, on_dev, flat = self._in(cl, 'cl')
        m = self._mats
        if self.kind == 2:
            import torch
            d = m[0] - m[1]
            out = torch.stack([m[0] @ t[0] + m[1] @ t[3], d @ t[1], d @ t[2], m[1] @ t[0] + m[0] @ t[3]])
        else:
            out = t @ m[0].T
        return self._out(out, on_dev, flat)

    def decouple(self, pcl):
        import torch
        t, on_dev, flat = self._in(pcl, 'pcl')
        rhs = (t @ self._B.T).reshape(-1, 1)                                                     # B pcl, stacked
        cb = torch.linalg.lu_solve(self._lu[0], self._lu[1], rhs).reshape(self.ns, self.bins.nbins)
        return self._out(cb, on_dev, flat)

    def bandpower_windows(self, device=False):
        import torch
        w = torch.linalg.lu_solve(self._lu[0], self._lu[1], self._blocks(self._BM))
        w = w.reshape(self.ns, self.bins.nbins, self.ns, self.lmax + 1)
        return w if device else w.cpu().numpy()


def decoupled_cl(f1, f2=None, mask1=None, mask2=None, bins=None, lmax=None, iter=3, workspace=None, nest=False):
    """The decoupled bandpowers of masked fields: {'ell': the bins' effective multipoles, 'cl': bandpowers [ns, nbins], 'pcl': the
    pseudo-C_l [ns, lmax + 1], 'fsky': mean(mask1 mask2)}.  Pass `workspace` (a PseudoClWorkspace of the same masks and spins) to reuse
    the coupling matrices, e.g. before and after baryonification; otherwise one is made from mask1 (required), mask2, `bins`, lmax."""
    _no_nest(nest)
    s1, s2, m1, m2, k1, k2, nside, on_dev = _fields(f1, f2, mask1, mask2)
    iter = _iter(iter)
    if workspace is None:
        if mask1 is None:
            raise ValueError("decoupled_cl needs mask1 (or a workspace)")
        workspace = PseudoClWorkspace(mask1, mask2, spin1=s1, spin2=s2, bins=bins, lmax=lmax)
    elif (workspace.spins != (s1, s2) or workspace.nside != nside or (lmax is not None and int(lmax) != workspace.lmax)):
        raise ValueError("the workspace is for spins %s, nside %d, lmax %d; the fields have spins %s, nside %d%s"
                         % (workspace.spins, workspace.nside, workspace.lmax, (s1, s2), nside, '' if lmax is None else ', lmax %d' % int(lmax)))
    pcl = _pseudo_cl(s1, s2, m1, m2, k1, k2, workspace.lmax, iter, on_dev)
    if on_dev:
        import torch
        ell = torch.from_numpy(workspace.ell).to(pcl.device)
    else:
        ell = workspace.ell.copy()
    return {'ell': ell, 'cl': workspace.decouple(pcl), 'pcl': pcl, 'fsky': workspace.fsky}
