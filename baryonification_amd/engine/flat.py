"""The flat-sky family on device-resident square 2-D maps: the transform pair, spectra, filters, spectral derivatives, Kaiser-Squires
and the peak counts of a grid.  Raw pointers in, enqueue-only, no torch."""
import numpy as np

from .. import _lib, _tensors


def fft2_work_doubles(n):
    """doubles of scratch the 2-D entries below need (three half spectra [n][fft_pitch(n)]); 0 for an unsupported n"""
    return int(_lib.call('bfgx_fft2_work_doubles', n))


def rfft2_device(map_ptr, n, work_ptr, spec_out_ptr, device=0, stream=0):
    """map [n][n] -> its half spectrum [n][fft_pitch(n)] complex, unnormalised (enqueue-only, like all 2-D entries here)"""
    _lib.call('bfgx_rfft2_device', device, stream, n, map_ptr, work_ptr, spec_out_ptr)


def irfft2_device(spec_ptr, n, scale, work_ptr, map_out_ptr, device=0, stream=0):
    """half spectrum [n][fft_pitch(n)] (kept) -> map [n][n], times `scale` (1 / n^2 inverts rfft2_device)"""
    _lib.call('bfgx_irfft2_device', device, stream, n, spec_ptr, scale, work_ptr, map_out_ptr)


def power_spectrum_2d_device(map_a_ptr, map_b_ptr, n, L, nk, window_order, work_ptr, paa_sum_ptr, pbb_sum_ptr, pab_sum_ptr, k_sum_ptr,
                             counts_ptr, device=0, stream=0):
    """cross_power_spectrum_device for two square 2-D maps (which may be the same): the five sums per linear k-bin"""
    _lib.call('bfgx_power_spectrum_2d_device', device, stream, n, map_a_ptr, map_b_ptr, L, nk, window_order, work_ptr, paa_sum_ptr, pbb_sum_ptr,
              pab_sum_ptr, k_sum_ptr, counts_ptr)


FILTER_KINDS_2D = {'gauss': 0, 'tophat': 1, 'table': 2}
DERIVATIVE_KINDS_2D = dict(FILTER_KINDS_2D, unit=3)


def _table(table_k, table_b):
    """(address of k, address of b, length, keepalive) of a host beam table; (0, 0, 0) without one"""
    tk = None if table_k is None else np.ascontiguousarray(table_k, dtype=np.float64)
    tb = None if table_b is None else np.ascontiguousarray(table_b, dtype=np.float64)
    return _tensors.ptr(tk), _tensors.ptr(tb), 0 if tk is None else int(tk.size), (tk, tb)


def filter_map_2d_device(map_ptr, n, L, kind, param, table_k, table_b, work_ptr, map_out_ptr, device=0, stream=0):
    """map_out = irfft2(rfft2(map) b(k)); kind as in FILTER_KINDS_2D, param = sigma or R, (table_k, table_b) host arrays for 'table'"""
    kind = FILTER_KINDS_2D[kind] if isinstance(kind, str) else int(kind)
    tk, tb, nt, keep = _table(table_k, table_b)
    _lib.call('bfgx_filter_map_2d_device', device, stream, n, map_ptr, L, kind, param, tk, tb, nt, work_ptr, map_out_ptr)


def derivatives_2d_work_doubles(n, nder=6):
    """doubles of scratch of derivatives_2d_device: nder + 1 half spectra [n][fft_pitch(n)]; 0 for an unsupported n or nder"""
    return int(_lib.call('bfgx_derivatives_2d_work_doubles', n, nder))


def derivatives_2d_device(spec_ptr, n, L, kind, param, table_k, table_b, nder, spin_form, work_ptr, ders_out_ptr, device=0, stream=0):
    """half spectrum [n][fft_pitch(n)] (kept) -> ders_out [nder][n][n], nder = 6: [u, u_x, u_y, u_xx, u_xy, u_yy] of the filtered map (or
    [u, u_x, u_y, lap, q_plus, q_cross] with spin_form), nder = 1: u alone; kind as in DERIVATIVE_KINDS_2D ('unit': no filter)"""
    kind = DERIVATIVE_KINDS_2D[kind] if isinstance(kind, str) else int(kind)
    tk, tb, nt, keep = _table(table_k, table_b)
    _lib.call('bfgx_derivatives_2d_device', device, stream, n, spec_ptr, L, kind, param, tk, tb, nt, nder, bool(spin_form), work_ptr, ders_out_ptr)


def peaks_2d_device(map_ptr, n, periodic, mask_ptr, nb, edges_ptr, counts_ptr, flags_ptr=0, device=0, stream=0):
    """maxima | minima of a square grid [n][n] per bin of their value: counts int64 [2][nb], optional int8 flags [n][n]"""
    _lib.call('bfgx_mapstats_peaks_2d_device', device, stream, n, bool(periodic), map_ptr, mask_ptr, nb, edges_ptr, counts_ptr, flags_ptr)


def kappa_to_shear_2d_device(kappa_ptr, n, work_ptr, g1_out_ptr, g2_out_ptr, device=0, stream=0):
    """Kaiser-Squires, convergence [n][n] -> shear (g1, g2)"""
    _lib.call('bfgx_kappa_to_shear_2d_device', device, stream, n, kappa_ptr, work_ptr, g1_out_ptr, g2_out_ptr)


def shear_to_kappa_2d_device(g1_ptr, g2_ptr, n, work_ptr, kappa_e_out_ptr, kappa_b_out_ptr, device=0, stream=0):
    """Kaiser-Squires, shear (g1, g2) -> convergence E and B modes"""
    _lib.call('bfgx_shear_to_kappa_2d_device', device, stream, n, g1_ptr, g2_ptr, work_ptr, kappa_e_out_ptr, kappa_b_out_ptr)
