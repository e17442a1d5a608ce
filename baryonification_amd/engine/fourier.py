"""Fourier statistics of gridded 3-D maps: P(k), cross and interlaced spectra, spectra straight from particle columns, the bispectrum,
and the slab steps of the multi-GPU FFT.  The `_device` entries take raw pointers and do not import torch; the functions that accept
CUDA tensors import it when they are called."""
import numpy as np

from .. import _lib, _tensors

WINDOW_ORDERS = {'none': 0, 'ngp': 1, 'cic': 2, 'tsc': 3}


def window_order(window, what):
    """0 .. 3 of a window given as that number or as a name of WINDOW_ORDERS (ValueError otherwise)"""
    if isinstance(window, str):
        if window.lower() in WINDOW_ORDERS:
            return WINDOW_ORDERS[window.lower()]
    elif not isinstance(window, bool) and window in (0, 1, 2, 3):
        return int(window)
    raise ValueError("%s: window must be 0, 1, 2, 3 or 'none', 'ngp', 'cic', 'tsc'" % what)


# ------------------------------------------------------------------------------------------------------- slab steps
def fft_slab_planes_device(map_ptr, n_grid, planes, work_ptr, device=0, stream=0):
    """slab P(k), step 1: transforms along the last two axes of `planes` planes; work = complex128 [planes][n][n/2+1]"""
    _lib.call('bfgx_fft_slab_planes_device', device, stream, n_grid, planes, map_ptr, work_ptr)


def fft_slab_axis0_pk_device(work_ptr, n_grid, ncols, col0, L, nk, pk_sum_ptr, k_sum_ptr, counts_ptr, device=0, stream=0):
    """slab P(k), step 3 (after the transpose): transform along the first axis of work [n][ncols][n/2+1] + partial bin sums"""
    _lib.call('bfgx_fft_slab_axis0_pk_device', device, stream, n_grid, ncols, col0, work_ptr, L, nk, pk_sum_ptr, k_sum_ptr, counts_ptr)


def fft_slab_axis0_xpk_device(spec_a_ptr, work_b_ptr, n_grid, ncols, col0, L, nk, window_order, paa_sum_ptr, pbb_sum_ptr, pab_sum_ptr, k_sum_ptr,
                              counts_ptr, device=0, stream=0):
    """the last pass of a cross spectrum alone: spec_a [n][ncols][fft_pitch(n)] = map A's finished spectrum of the columns col0 .. of the
    middle axis, work_b = map B's before the transform along the first axis (neither is changed) -> partial bin sums"""
    _lib.call('bfgx_fft_slab_axis0_xpk_device', device, stream, n_grid, ncols, col0, spec_a_ptr, work_b_ptr, L, nk, window_order, paa_sum_ptr,
              pbb_sum_ptr, pab_sum_ptr, k_sum_ptr, counts_ptr)


def fft_slab_axis0_device(work_ptr, n_grid, ncols, inverse=0, device=0, stream=0):
    """in-place complex transforms along the first axis of work [n][ncols][fft_pitch(n)]; inverse: exponent +i, unnormalised"""
    _lib.call('bfgx_fft_slab_axis0_device', device, stream, n_grid, ncols, work_ptr, inverse)


def ifft_slab_planes_device(work_ptr, n_grid, planes, map_out_ptr, device=0, stream=0):
    """the inverse of fft_slab_planes_device, unnormalised: complex work [planes][n][fft_pitch(n)] -> real map_out [planes][n][n];
    work is scratch afterwards"""
    _lib.call('bfgx_ifft_slab_planes_device', device, stream, n_grid, planes, work_ptr, map_out_ptr)


# ------------------------------------------------------------------------------------------------------- P(k)
def fft_pitch(n_grid):
    """complex values per row of the half-spectrum work arrays: n/2 + 1 rounded up to whole 128-byte lines"""
    return int(_lib.call('bfgx_fft_pitch', n_grid))


def power_spectrum_work_doubles(n_grid):
    """doubles of scratch power_spectrum_device needs (half spectrum, rows padded to whole 128-byte lines)"""
    return int(_lib.call('bfgx_power_spectrum_work_doubles', n_grid))


def power_spectrum_device(map_ptr, n_grid, L, nk, work_ptr, pk_sum_ptr, k_sum_ptr, counts_ptr, device=0, stream=0):
    """FFT + |F|^2 + linear k-bins on a device-resident map; work = power_spectrum_work_doubles(n_grid) doubles of scratch"""
    _lib.call('bfgx_power_spectrum_device', device, stream, n_grid, map_ptr, L, nk, work_ptr, pk_sum_ptr, k_sum_ptr, counts_ptr)


def power_spectrum(Map, Lbox, Nk=180, device=0):
    """P(k) summary of a cubic map as in examples/10_Reproduce_Schneider_deltaPk.ipynb (cells 12, 15): |FFT|^2 averaged in
    Nk linear bins between the fundamental and the Nyquist frequency.  Returns (k_cen, Pk, k_count)."""
    Map = _lib.f8(Map)
    if Map.ndim != 3 or len(set(Map.shape)) != 1:
        raise ValueError("power_spectrum needs a cubic 3-D map")
    pk, kc = np.empty(Nk), np.empty(Nk)
    cnt = np.empty(Nk, dtype=np.int64)
    _lib.call('bfgx_power_spectrum', device, Map.shape[0], Map.ctypes.data, Lbox, Nk, pk.ctypes.data, kc.ctypes.data, cnt.ctypes.data)
    return kc, pk, cnt


def _cuda_f8_cube(Map, what):
    """a CUDA float64 tensor holding a cubic 3-D map, contiguous (ValueError otherwise)"""
    import torch
    if not isinstance(Map, torch.Tensor) or not Map.is_cuda or Map.dtype != torch.float64:
        raise ValueError("%s needs a CUDA float64 tensor" % what)
    if Map.dim() != 3 or len(set(Map.shape)) != 1:
        raise ValueError("%s needs a cubic 3-D map" % what)
    return Map.contiguous()


def _work(doubles, like):
    import torch
    return torch.empty(doubles, dtype=torch.float64, device=like.device)


def power_spectrum_tensor(Map, Lbox, Nk=180):
    """power_spectrum for a CUDA float64 tensor, analysed where it lies on the current stream.  Returns (k_cen, Pk, k_count) as numpy
    arrays, empty bins NaN."""
    Map = _cuda_f8_cube(Map, "power_spectrum_tensor")
    N, Nk = int(Map.shape[0]), int(Nk)
    work = _work(power_spectrum_work_doubles(N), Map)
    (pk, k), cnt = _tensors.bin_means(Map.device, 2, Nk, lambda *out: power_spectrum_device(
        Map.data_ptr(), N, Lbox, Nk, work.data_ptr(), *out, **_tensors.launch_args(Map)))
    return k, pk, cnt


# ------------------------------------------------------------------------------------------------------- cross spectra
def cross_power_spectrum_work_doubles(n_grid):
    """doubles of scratch cross_power_spectrum_device needs (two half spectra)"""
    return int(_lib.call('bfgx_cross_power_spectrum_work_doubles', n_grid))


def cross_power_spectrum_device(map_a_ptr, map_b_ptr, n_grid, L, nk, window_order, work_ptr, paa_sum_ptr, pbb_sum_ptr, pab_sum_ptr, k_sum_ptr,
                                counts_ptr, device=0, stream=0):
    """the sums of |F_A|^2, |F_B|^2, Re(F_A conj F_B), |k| and the counts per linear k-bin of two device-resident maps (which may be the
    same); work = cross_power_spectrum_work_doubles(n_grid) doubles of scratch; window_order 0, 1, 2, 3 = none, NGP, CIC, TSC"""
    _lib.call('bfgx_cross_power_spectrum_device', device, stream, n_grid, map_a_ptr, map_b_ptr, L, nk, window_order, work_ptr, paa_sum_ptr,
              pbb_sum_ptr, pab_sum_ptr, k_sum_ptr, counts_ptr)


def _two_cubes(what, MapA, MapB):
    """(on_device, MapA, MapB): two numpy cubes of one shape made float64, or two tensors as they came (ValueError otherwise)"""
    on_dev = _tensors.is_tensor(MapA)
    if on_dev != _tensors.is_tensor(MapB):
        raise ValueError("%s needs two numpy arrays or two CUDA float64 tensors, not one of each" % what)
    if not on_dev:
        MapA, MapB = _lib.f8(MapA), _lib.f8(MapB)
        if MapA.ndim != 3 or len(set(MapA.shape)) != 1:
            raise ValueError("%s needs cubic 3-D maps" % what)
        if MapA.shape != MapB.shape:
            raise ValueError("%s needs two maps of one shape" % what)
    return on_dev, MapA, MapB


def _two_cuda_cubes(what, MapA, MapB):
    MapA, MapB = _cuda_f8_cube(MapA, what), _cuda_f8_cube(MapB, what)
    if MapA.shape != MapB.shape or MapA.device != MapB.device:
        raise ValueError("%s needs two maps of one shape on one device" % what)
    return MapA, MapB


def cross_power_spectrum(MapA, MapB, Lbox, Nk=180, window=0, device=0):
    """Auto and cross power spectra of two cubic 3-D maps of one shape in the bins and units of power_spectrum (the unnormalised fftn).
    MapA, MapB: two numpy arrays, or two CUDA float64 torch tensors, which are analysed where they lie on the current stream.  window:
    0, 1, 2, 3 or 'none', 'ngp', 'cic', 'tsc' divides the mass-assignment window of that order out of every mode.  Returns a dict of numpy
    arrays: k (mean |k| per bin), paa, pbb, pab = <Re(F_A conj F_B)>, r = pab / sqrt(paa pbb), counts (modes per bin); empty bins NaN."""
    what = "cross_power_spectrum"
    p = window_order(window, what)
    Nk = int(Nk)
    on_dev, MapA, MapB = _two_cubes(what, MapA, MapB)
    if not on_dev:
        out = np.empty((4, max(Nk, 1)))
        cnt = np.empty(max(Nk, 1), dtype=np.int64)
        _lib.call('bfgx_cross_power_spectrum', device, MapA.shape[0], MapA.ctypes.data, MapB.ctypes.data, Lbox, Nk, p, out[0].ctypes.data,
                  out[1].ctypes.data, out[2].ctypes.data, out[3].ctypes.data, cnt.ctypes.data)
        paa, pbb, pab, k = out
    else:
        MapA, MapB = _two_cuda_cubes(what, MapA, MapB)
        N = int(MapA.shape[0])
        work = _work(cross_power_spectrum_work_doubles(N), MapA)
        (paa, pbb, pab, k), cnt = _tensors.bin_means(MapA.device, 4, Nk, lambda *out: cross_power_spectrum_device(
            MapA.data_ptr(), MapB.data_ptr(), N, Lbox, Nk, p, work.data_ptr(), *out, **_tensors.launch_args(MapA)))
    with np.errstate(divide='ignore', invalid='ignore'):
        r = pab / np.sqrt(paa * pbb)
    return {'k': k, 'paa': paa, 'pbb': pbb, 'pab': pab, 'r': r, 'counts': cnt}


def interlaced_power_spectrum_device(map1_ptr, map2_ptr, n_grid, L, nk, window_order, work_ptr, p_sum_ptr, p1_sum_ptr, k_sum_ptr, counts_ptr,
                                     device=0, stream=0):
    """the sums of w |F1 + Phi F2|^2 / 4 (p_sum) and of w |F1|^2 (p1_sum), of |k| and the counts per linear k-bin of two device-resident
    grids, the second deposited half a cell away; work = cross_power_spectrum_work_doubles(n_grid) doubles of scratch"""
    _lib.call('bfgx_interlaced_power_spectrum_device', device, stream, n_grid, map1_ptr, map2_ptr, L, nk, window_order, work_ptr, p_sum_ptr,
              p1_sum_ptr, k_sum_ptr, counts_ptr)


def interlaced_power_spectrum(Map1, Map2, Lbox, Nk=180, window='tsc'):
    """P(k) of two grids of ONE particle set, Map2 deposited half a cell away from Map1 (deposit_cloud_device(..., shift=1)), combined in
    Fourier space so that the odd aliased images cancel, in the bins and units of power_spectrum; `window` as in cross_power_spectrum.
    Two numpy cubes (uploaded to device 0) or two CUDA float64 tensors, which are analysed where they lie on the current stream.  Returns
    a dict of numpy arrays: k, pk (the interlaced estimate), pk_grid1 (Map1 alone: the aliased estimate), counts; empty bins NaN."""
    import torch                                                     # noqa: F401  (a missing torch is reported before any argument)
    what = "interlaced_power_spectrum"
    p = window_order(window, what)
    Nk = int(Nk)
    on_dev, Map1, Map2 = _two_cubes(what, Map1, Map2)
    if not on_dev:
        Map1, Map2 = _tensors.to_cuda(Map1), _tensors.to_cuda(Map2)
    Map1, Map2 = _two_cuda_cubes(what, Map1, Map2)
    N = int(Map1.shape[0])
    work = _work(cross_power_spectrum_work_doubles(N), Map1)
    (pk, pk1, k), cnt = _tensors.bin_means(Map1.device, 3, Nk, lambda *out: interlaced_power_spectrum_device(
        Map1.data_ptr(), Map2.data_ptr(), N, Lbox, Nk, p, work.data_ptr(), *out, **_tensors.launch_args(Map1)))
    return {'k': k, 'pk': pk, 'pk_grid1': pk1, 'counts': cnt}


# ------------------------------------------------------------------------------------------------------- spectra of particles
def particle_power_spectrum_work_doubles(n_grid):
    """doubles of scratch particle_power_spectrum_device needs (two maps and two half spectra)"""
    return int(_lib.call('bfgx_particle_power_spectrum_work_doubles', n_grid))


def particle_power_spectrum_device(x_ptr, y_ptr, z_ptr, mass_ptr, n, n_grid, L, order, interlace, nk, work_ptr, p_sum_ptr, p1_sum_ptr, k_sum_ptr,
                                   counts_ptr, device=0, stream=0):
    """device-resident particle columns -> the four sums of interlaced_power_spectrum_device: deposit, shifted deposit, spectrum, enqueue-only;
    order 2 (CIC) or 3 (TSC), whose window is divided out; interlace=0: one deposit, the windowed auto spectrum in both p_sum and p1_sum"""
    _lib.call('bfgx_particle_power_spectrum_device', device, stream, n, x_ptr, y_ptr, z_ptr, mass_ptr, n_grid, L, order, interlace, nk, work_ptr,
              p_sum_ptr, p1_sum_ptr, k_sum_ptr, counts_ptr)


def particle_power_spectrum(coords, mass, N_grid, Lbox, Nk=180, assignment='tsc', interlace=True, normalize=False, subtract_shot_noise=False,
                            device=0):
    """P(k) of particles of the periodic box [0, Lbox]^3 up to the Nyquist frequency of a grid of N_grid cells per axis, without the maps
    ever leaving the device: CIC or TSC deposit (`assignment`), with interlace=True a second deposit half a cell away and the two grids
    combined in Fourier space (the odd aliased images cancel), the assignment's window divided out.  coords = (x, y, z) as numpy arrays
    or as CUDA float64 tensors (analysed where they lie on the current stream; `device` is then theirs); mass: likewise, or None for unit
    masses.  Particles with a coordinate outside [0, Lbox] are dropped, as make_map drops them.
    Returns a dict of numpy arrays k, pk, pk_grid1 (the first grid alone: the aliased estimate; equal to pk without interlacing), counts,
    and the floats shot_noise = sum m^2 and mass = sum m over the kept particles.  The defaults are in the units of power_spectrum (the
    unnormalised fftn of the mass grid); normalize=True multiplies pk, pk_grid1 and shot_noise by Lbox^3 / mass^2 (the spectrum of the
    density contrast); subtract_shot_noise=True subtracts shot_noise from pk and pk_grid1."""
    order = WINDOW_ORDERS.get(assignment.lower(), -1) if isinstance(assignment, str) else -1
    if order < 1:
        raise ValueError("particle_power_spectrum: assignment must be 'cic' or 'tsc', not %r" % (assignment,))
    if order == 1:
        raise ValueError("particle_power_spectrum: assignment 'ngp' has no interlaced form%s; use 'cic' or 'tsc'" % (
            "" if interlace else " and no entry here (make_map and power_spectrum give its spectrum)"))
    if len(coords) != 3:
        raise ValueError("particle_power_spectrum needs coords = (x, y, z): the spectra here are 3-D")
    Nk, N_grid, Lbox = int(Nk), int(N_grid), float(Lbox)
    on_dev = [_tensors.is_tensor(c) for c in coords]
    m_dev = mass is not None and _tensors.is_tensor(mass)
    if any(on_dev) != all(on_dev) or (mass is not None and m_dev != on_dev[0]):
        raise ValueError("particle_power_spectrum needs numpy arrays or CUDA float64 tensors, not some of each")
    if not on_dev[0]:
        out = np.empty((3, max(Nk, 1)))
        cnt = np.empty(max(Nk, 1), dtype=np.int64)
        x, y, z = (_lib.f8(c).ravel() for c in coords)
        m = None if mass is None else _lib.f8(mass).ravel()
        if not (x.size == y.size == z.size and (m is None or m.size == x.size)):
            raise ValueError("particle_power_spectrum needs columns of one length")
        _lib.call('bfgx_particle_power_spectrum', device, x.size, x.ctypes.data, y.ctypes.data, z.ctypes.data, _tensors.ptr(m), N_grid, Lbox,
                  order, bool(interlace), Nk, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, cnt.ctypes.data)
        pk, pk1, k = out
        with np.errstate(invalid='ignore'):
            keep = (x >= 0) & (x <= Lbox) & (y >= 0) & (y <= Lbox) & (z >= 0) & (z <= Lbox)
        mk = np.ones(int(keep.sum())) if m is None else m[keep]
        m_tot, shot = float(mk.sum()), float((mk * mk).sum())
    else:
        import torch
        cols = list(coords) + ([] if mass is None else [mass])
        for c in cols:
            if not isinstance(c, torch.Tensor) or not c.is_cuda or c.dtype != torch.float64 or c.dim() != 1:
                raise ValueError("particle_power_spectrum needs 1-D CUDA float64 tensors")
        if any(c.shape != cols[0].shape or c.device != cols[0].device for c in cols):
            raise ValueError("particle_power_spectrum needs columns of one length on one device")
        cols = [c.contiguous() for c in cols]
        x, y, z = cols[:3]
        m = None if mass is None else cols[3]
        n = int(x.shape[0])
        work = _work(particle_power_spectrum_work_doubles(N_grid), x)
        ptrs = [c.data_ptr() if n else 0 for c in (x, y, z)] + [m.data_ptr() if (m is not None and n) else 0]
        (pk, pk1, k), cnt = _tensors.bin_means(x.device, 3, Nk, lambda *out: particle_power_spectrum_device(
            *ptrs, n, N_grid, Lbox, order, bool(interlace), Nk, work.data_ptr(), *out, **_tensors.launch_args(x)))
        keep = (x >= 0) & (x <= Lbox) & (y >= 0) & (y <= Lbox) & (z >= 0) & (z <= Lbox)
        mk = keep.to(torch.float64) if m is None else torch.where(keep, m, torch.zeros_like(m))
        m_tot, shot = float(mk.sum()), float((mk * mk).sum())
    if subtract_shot_noise:
        pk, pk1 = pk - shot, pk1 - shot
    if normalize:
        norm = Lbox ** 3 / m_tot ** 2 if m_tot != 0 else float('nan')
        pk, pk1, shot = pk * norm, pk1 * norm, shot * norm
    return {'k': k, 'pk': pk, 'pk_grid1': pk1, 'counts': cnt, 'shot_noise': shot, 'mass': m_tot}


# ------------------------------------------------------------------------------------------------------- bispectrum
def bispectrum_work_doubles(n_grid, nbins):
    """doubles of scratch bispectrum_device needs (two half spectra, nbins real fields, partial sums); 0 outside the limits"""
    return int(_lib.call('bfgx_bispectrum_work_doubles', n_grid, nbins))


def bispectrum_shell_fields_device(spec_ptr, n_grid, L, k_edges, unit, scratch_spec_ptr, fields_ptr, device=0, stream=0):
    """fields [nbins][n][n][n] = the unnormalised inverse transforms of the half spectrum spec [n][n][fft_pitch(n)] restricted to each
    k-bin (unit: of a spectrum of ones); scratch_spec: another half spectrum"""
    e = _lib.f8(k_edges)
    _lib.call('bfgx_bispectrum_shell_fields_device', device, stream, n_grid, L, e.size - 1, e.ctypes.data, spec_ptr, unit, scratch_spec_ptr,
              fields_ptr)


def bispectrum_device(map_ptr, n_grid, L, k_edges, triangles, work_ptr, b_sum_ptr, n_tri_ptr, pk_sum_ptr, n_modes_ptr, device=0, stream=0):
    """FFT bispectrum estimator on a device-resident map: b_sum[ntri], n_tri[ntri], pk_sum[nbins], n_modes[nbins] (device arrays);
    work = bispectrum_work_doubles(n_grid, nbins) doubles of scratch; k_edges and triangles [ntri][3] are host arrays"""
    e = _lib.f8(k_edges)
    t = np.ascontiguousarray(triangles, dtype=np.int32)
    _lib.call('bfgx_bispectrum_device', device, stream, n_grid, map_ptr, L, e.size - 1, e.ctypes.data, t.size // 3, t.ctypes.data, work_ptr,
              b_sum_ptr, n_tri_ptr, pk_sum_ptr, n_modes_ptr)


BISPECTRUM_MAX_BINS, BISPECTRUM_MAX_TRIANGLES = 32, 8192


def bispectrum_triangles(k_edges, kind='all'):
    """The bin triples i <= j <= l (int32 [ntri][3]) whose bins can hold a closed triangle: k_edges[l] < k_edges[i + 1] + k_edges[j + 1].
    kind: 'all', 'equilateral' (i = j = l) or 'isosceles' (i = j <= l)."""
    if kind not in ('all', 'equilateral', 'isosceles'):
        raise ValueError("bispectrum_triangles: kind must be 'all', 'equilateral' or 'isosceles'")
    e = _lib.f8(k_edges)
    nb = e.size - 1
    out = [(i, j, l) for i in range(nb) for j in range(i, nb) for l in range(j, nb)
           if e[l] < e[i + 1] + e[j + 1] and (kind == 'all' or (i == j and (kind == 'isosceles' or j == l)))]
    return np.array(out, dtype=np.int32).reshape(-1, 3)


def bispectrum(Map, Lbox, k_edges, triangles='all', normalize=False, device=0):
    """Bispectrum of a cubic 3-D map in the k-bins k_edges (FFT estimator; units of power_spectrum: the unnormalised fftn, no volume
    factors, unless normalize).  Map: a numpy array, or a CUDA float64 torch tensor, which is analysed where it lies.  triangles: a kind
    of bispectrum_triangles or an integer array [ntri][3] of bin indices.  Returns a dict of numpy arrays: k (bin centres), triangles,
    B = b_sum / n_tri (NaN where no closed triangle exists), n_tri, pk = pk_sum / n_modes (NaN for empty bins), n_modes.
    normalize: B times L^6 / N^9, pk times L^3 / N^6."""
    e = _lib.f8(k_edges)
    if e.ndim != 1 or e.size < 2:
        raise ValueError("bispectrum needs at least two bin edges")
    nb = e.size - 1
    if nb > BISPECTRUM_MAX_BINS:
        raise ValueError("bispectrum needs 1 <= nbins <= %d" % BISPECTRUM_MAX_BINS)
    tri = bispectrum_triangles(e, triangles) if isinstance(triangles, str) else np.ascontiguousarray(triangles, dtype=np.int32)
    if tri.ndim != 2 or tri.shape[1] != 3 or not 1 <= tri.shape[0] <= BISPECTRUM_MAX_TRIANGLES:
        raise ValueError("bispectrum needs triangles [ntri][3] with 1 <= ntri <= %d" % BISPECTRUM_MAX_TRIANGLES)
    on_device = _tensors.is_tensor(Map)
    if not on_device:
        Map = _lib.f8(Map)
    if len(Map.shape) != 3 or len(set(Map.shape)) != 1:
        raise ValueError("bispectrum needs a cubic 3-D map")
    N, ntri = int(Map.shape[0]), tri.shape[0]
    if not on_device:
        b_sum, n_tri, pk_sum, n_modes = np.empty(ntri), np.empty(ntri), np.empty(nb), np.empty(nb)
        _lib.call('bfgx_bispectrum', device, N, Map.ctypes.data, Lbox, nb, e.ctypes.data, ntri, tri.ctypes.data, b_sum.ctypes.data,
                  n_tri.ctypes.data, pk_sum.ctypes.data, n_modes.ctypes.data)
    else:
        import torch
        if not Map.is_cuda or Map.dtype != torch.float64:
            raise ValueError("bispectrum needs a numpy array or a CUDA float64 tensor")
        Map = Map.contiguous()
        nw = bispectrum_work_doubles(N, nb)
        if nw <= 0:
            raise NotImplementedError("n_grid must be a power of two with 8 <= n_grid <= 1024")
        work = _work(nw, Map)
        res = torch.empty(2 * ntri + 2 * nb, dtype=torch.float64, device=Map.device)
        bispectrum_device(Map.data_ptr(), N, Lbox, e, tri, work.data_ptr(), res[:ntri].data_ptr(), res[ntri:2 * ntri].data_ptr(),
                          res[2 * ntri:2 * ntri + nb].data_ptr(), res[2 * ntri + nb:].data_ptr(), **_tensors.launch_args(Map))
        r = res.cpu().numpy()
        b_sum, n_tri, pk_sum, n_modes = r[:ntri], r[ntri:2 * ntri], r[2 * ntri:2 * ntri + nb], r[2 * ntri + nb:]
    with np.errstate(divide='ignore', invalid='ignore'):
        # (the counts are integers up to the rounding of the transforms: "none" is less than half a triangle)
        B = np.where(np.abs(n_tri) < 0.5, np.nan, b_sum / n_tri)
        pk = np.where(np.abs(n_modes) < 0.5, np.nan, pk_sum / n_modes)
    if normalize:
        B = B * (float(Lbox) ** 6 / float(N) ** 9)
        pk = pk * (float(Lbox) ** 3 / float(N) ** 6)
    return {'k': 0.5 * (e[:-1] + e[1:]), 'triangles': tri, 'B': B, 'n_tri': n_tri, 'pk': pk, 'n_modes': n_modes}
