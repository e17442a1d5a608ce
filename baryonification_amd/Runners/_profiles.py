"""
What MeasureProfilesShell, MeasureProfilesSnapshot and MeasureProfilesGrid share in Python: the check of `r_edges`, the quotient with NaN
for an empty bin, the result class of the two map measurements, the halo radii of the two box measurements, the result arrays.
"""
import numpy as np

from .._tensors import is_cuda_tensor as _is_cuda_tensor, ptr
from ..utils.cosmology import Cosmology, MassDef, massdef_to_tuple

MAX_PROFILE_BINS = 64          # csrc/bfgx_stack_core.hpp kStackMaxBins: the bins of a halo live on chip


def check_r_edges(r_edges):
    """r_edges as a contiguous float64 array; ValueError unless it holds 2 .. MAX_PROFILE_BINS + 1 finite, >= 0, strictly ascending edges"""
    edges = np.ascontiguousarray(r_edges, dtype=np.float64)
    if edges.ndim != 1 or edges.size < 2:
        raise ValueError("r_edges must be a 1-D array of at least 2 bin edges")
    if edges.size - 1 > MAX_PROFILE_BINS:
        raise ValueError("%d radial bins: at most %d are supported" % (edges.size - 1, MAX_PROFILE_BINS))
    if not np.all(np.isfinite(edges)) or edges[0] < 0 or not np.all(np.diff(edges) > 0):
        raise ValueError("r_edges must be finite, >= 0 and strictly ascending")
    return edges


def ratio(s, n):
    """s / n, NaN where n is 0 (numpy arrays or torch tensors)"""
    if isinstance(s, np.ndarray):
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(n != 0, s / n, np.nan)
    return (s / n).masked_fill(n == 0, float('nan'))


class _MapProfiles(object):
    """The result of a map measurement (ShellProfiles, GridProfiles)"""

    def __init__(self, r_edges, npix, sum, npix_shear=None, sum_t=None, sum_x=None, scaled=False):
        self.r_edges, self.scaled = r_edges, scaled
        self.npix, self.sum = npix, sum
        self.npix_shear, self.sum_t, self.sum_x = npix_shear, sum_t, sum_x

    @property
    def mean(self):
        """sum / npix, NaN where npix is 0"""
        return ratio(self.sum, self.npix)

    @property
    def mean_t(self):
        return None if self.sum_t is None else ratio(self.sum_t, self.npix_shear)

    @property
    def mean_x(self):
        return None if self.sum_x is None else ratio(self.sum_x, self.npix_shear)

    def stack(self, select=None, weights=None):
        """The pixel-weighted mean profile over the chosen halos, sum_j w_j sum[j] / sum_j w_j npix[j] per bin (NaN where the denominator
        is 0): a dict with 'mean' and, with shear, 'mean_t' and 'mean_x'.  select: anything that indexes the halo axis; weights: one per
        chosen halo (default 1)."""
        sel = slice(None) if select is None else select
        out = {}
        for name, s, n in (('mean', self.sum, self.npix), ('mean_t', self.sum_t, self.npix_shear), ('mean_x', self.sum_x, self.npix_shear)):
            if s is None:
                continue
            s, n = s[sel], n[sel].to(s.dtype) if not isinstance(n, np.ndarray) else n[sel].astype(np.float64)
            if weights is not None:
                w = weights if not isinstance(s, np.ndarray) else np.asarray(weights, dtype=np.float64)
                s, n = s * w[:, None], n * w[:, None]
            out[name] = ratio(s.sum(0), n.sum(0))
        return out


def halo_radii(hcat, axes, redshift, mass_def, cosmo_dict, eps, r_clip):
    """(R_com, R_q) per halo on the host: the comoving radius of the mass definition and the radius of the ball,
    clip(eps R_com, 0, r_clip); NaN and 0 for a halo the measurement skips (M not positive / finite, a non-finite coordinate in `axes`)."""
    M = np.asarray(hcat['M'], dtype=np.float64)
    ok = (M > 0) & np.isfinite(M)
    for k in axes:
        ok &= np.isfinite(np.asarray(hcat[k], dtype=np.float64))
    a = 1.0 / (1.0 + float(redshift))
    R = np.full(M.size, np.nan)
    if ok.any():
        R[ok] = MassDef(*massdef_to_tuple(mass_def)).get_radius(Cosmology.from_dict(cosmo_dict), M[ok], a) / a
    with np.errstate(invalid='ignore'):
        R_q = np.where(ok, np.minimum(np.maximum(float(eps) * R, 0.0), float(r_clip)), 0.0)
    return R, R_q


def alloc_profile_outs(n, nb, shear, device=None):
    """(outs, optr): the (n, nb) arrays npix, sum[, npix_shear, sum_t, sum_x] and their five pointers for the C entries (None for the absent
    ones).  Zero-filled numpy arrays, or uninitialised tensors on a torch `device` (the library writes every cell)."""
    kinds = 'ififf' if shear else 'if'
    if device is None:
        outs = [np.zeros((n, nb), dtype=(np.int64 if k == 'i' else np.float64)) for k in kinds]
    else:
        import torch
        outs = [torch.empty((n, nb), dtype=(torch.int64 if k == 'i' else torch.float64), device=device) for k in kinds]
    return outs, [ptr(o) for o in outs] + [None] * (5 - len(outs))
