"""The C-ABI library loads without a GPU and exports every symbol include/bfgx.h declares; the ctypes
binding covers exactly that set.  No compute entry point is called here."""
import os
import re

import numpy as np
import pytest

from baryonification_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(REPO, 'include', 'bfgx.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(bfgx_[A-Za-z0-9_]+)\s*\(', src)))


def test_header_symbols_exported_and_bound():
    names = header_functions()
    assert len(names) >= 15
    L = _lib.load()
    for n in names:
        assert hasattr(L, n), "libbfgx.so does not export %s" % n
    assert sorted(_lib.SYMBOLS) == names, "ctypes binding and header disagree"


def test_abi_version_and_device_count_callable_without_gpu():
    L = _lib.load()
    assert L.bfgx_abi_version() == 4 == _lib.ABI_VERSION
    assert L.bfgx_device_count() >= 0


def test_struct_sizes_match_header_layout():
    import ctypes as C
    assert C.sizeof(_lib.bfgx_cosmo) == 64
    assert C.sizeof(_lib.bfgx_massdef) == 16
    assert C.sizeof(_lib.bfgx_table) == 4 + 4 * 7 + 8 * 7 + 8 + 4 + 4 + 8       # ndim, n[7], axis[7], values, rdelta, log, eps_model
    assert C.sizeof(_lib.bfgx_catalog) == 8 + 4 * 8 + 4 * 8 + 2 * 8       # n, M z ra dec, extra[4], ln1pz lnM
    assert C.sizeof(_lib.bfgx_opts) == 24 + 8                           # 6 x int32, catalog_token


def test_compute_fails_loudly_without_gpu():
    """no CPU fallback: with no device the plan cannot be created"""
    L = _lib.load()
    if L.bfgx_device_count() > 0:
        pytest.skip("GPU present")
    import ctypes as C
    from baryonification_amd import engine, synthetic as syn
    z, M, r = np.geomspace(0.1, 0.2, 3), np.geomspace(1e13, 1e14, 3), np.geomspace(1e-2, 10, 8)
    model, keep = engine.model_from_tables([np.log(1 + z), np.log(M), np.log(r)], np.zeros((3, 3, 8)), syn.COSMO, 10.0)
    with pytest.raises(_lib.BfgxError, match="no HIP device"):
        engine.ShellPlan(model, keep, 16, 10)


def test_invalid_arguments_map_to_python_exceptions():
    from baryonification_amd import engine, synthetic as syn
    z, M, r = np.geomspace(0.1, 0.2, 3), np.geomspace(1e13, 1e14, 3), np.geomspace(1e-2, 10, 8)
    axes = [np.log(1 + z), np.log(M), np.log(r)]
    bad_axes = [axes[0][::-1].copy(), axes[1], axes[2]]
    model, keep = engine.model_from_tables(bad_axes, np.zeros((3, 3, 8)), syn.COSMO, 10.0)
    with pytest.raises(ValueError, match="ascending"):
        engine.ShellPlan(model, keep, 16, 10)
    model, keep = engine.model_from_tables(axes, np.zeros((3, 3, 8)), syn.COSMO, 10.0)
    with pytest.raises(ValueError, match="nside"):
        engine.ShellPlan(model, keep, 0, 10)
    with pytest.raises(ValueError):
        _lib.make_table(axes, np.zeros((3, 3, 7)))


def test_power_spectrum_work_size_is_host_arithmetic():
    """rows of the half spectrum are padded to whole 128-byte lines (8 complex values): pure host functions, no GPU needed"""
    from baryonification_amd import engine
    for n in (8, 16, 64, 128, 512, 1024):
        pitch = engine.fft_pitch(n)
        assert pitch % 8 == 0 and n // 2 + 1 <= pitch < n // 2 + 1 + 8
        assert engine.power_spectrum_work_doubles(n) == 2 * n * n * pitch
    assert engine.fft_pitch(512) == 264


def test_null_arguments_are_refused_before_any_device_call():
    import ctypes as C
    L = _lib.load()
    n = C.c_int64(0)
    assert L.bfgx_grid_baryonify_device(None, None, None, None, None, C.byref(n)) == _lib.ERR_INVALID
    assert b'NULL' in L.bfgx_last_error()
    assert L.bfgx_power_spectrum_device(0, None, 64, None, 100.0, 10, None, None, None, None) == _lib.ERR_INVALID


@pytest.mark.parametrize('n_grid', [7, 12, 2048])
def test_power_spectrum_device_entries_check_n_grid_before_any_device_call(n_grid):
    """the three 3-D P(k) _device entries refuse a bad n_grid as bfgx_power_spectrum does, code and message, before the device is
    selected: host arrays stand in the device slots, and nothing may touch them with or without a device"""
    import ctypes as C
    L = _lib.load()
    host = np.zeros(64)
    p = host.ctypes.data_as(C.c_void_p)
    assert L.bfgx_power_spectrum(0, n_grid, p, 100.0, 4, p, p, p) == _lib.ERR_UNSUPPORTED
    msg = L.bfgx_last_error()
    assert b'power spectrum needs n_grid = 2^m with 8 <= n_grid <= 1024' == msg
    for rc in (L.bfgx_power_spectrum_device(0, None, n_grid, p, 100.0, 4, p, p, p, p),
               L.bfgx_fft_slab_planes_device(0, None, n_grid, 2, p, p),
               L.bfgx_fft_slab_axis0_pk_device(0, None, n_grid, 1, 0, p, 100.0, 4, p, p, p)):
        assert rc == _lib.ERR_UNSUPPORTED
        assert L.bfgx_last_error() == msg
    assert not host.any()


def test_round5_entries_refuse_bad_arguments_before_any_device_call():
    """the entries added in round 5 (one-call snapshot -> map, per-halo callable bridge, fused band entry) check their arguments first"""
    import ctypes as C
    L = _lib.load()
    n = C.c_int64(0)
    h = C.c_void_p()
    assert L.bfgx_shell_pairs_begin(None, None, 64, 0, 0, C.byref(h), None) == _lib.ERR_INVALID and not h.value
    assert L.bfgx_shell_pairs_radii(None, None) == _lib.ERR_INVALID
    assert L.bfgx_shell_pairs_apply(None, None, None, None, 1, None) == _lib.ERR_INVALID
    L.bfgx_shell_pairs_end(None)                                                  # (a no-op)
    assert L.bfgx_snapshot_displace_deposit_device(None, None, 0, None, None, None, None, 8, None, None, C.byref(n)) == _lib.ERR_INVALID
    st = _lib.bfgx_stats()
    assert L.bfgx_baryonify_snapshot_records_map(None, None, 3, 100.0, 0.0, 0, None, 32, 8, 16, 24, 0, 8, None, None, None, C.byref(st)) == _lib.ERR_INVALID
    assert L.bfgx_offsets_regrid_bands_device(None, None, 0, 1, None, 0, 0, 1, None, None, None, None) == _lib.ERR_INVALID
    assert b'NULL' in L.bfgx_last_error()


def test_displacement_rows_refuses_row_lengths_that_cannot_launch():
    """displacement_kernel holds a row in one workgroup's LDS: 64 B per node (seven doubles, two ints) behind 3104 B of
    reduction arrays, 163 840 B in all, so 2511 nodes at the most.  Longer and too short rows are refused with that
    number before any device call (so also on a machine without a GPU)."""
    import ctypes as C
    from baryonification_amd import tables
    assert tables.MAX_N_R == (160 * 1024 - 3104) // (7 * 8 + 2 * 4) == 2511
    L = _lib.load()
    for nr in (tables.MAX_N_R + 1, 4096, 2):
        r = np.geomspace(1e-3, 1e2, nr)
        M = np.ones((1, nr))
        d, st = np.empty((1, nr)), np.empty(1, dtype=np.int32)
        rc = L.bfgx_displacement_rows(0, 1, nr, r.ctypes.data, M.ctypes.data, M.ctypes.data, d.ctypes.data, st.ctypes.data)
        assert rc == _lib.ERR_INVALID
        assert b'[3, %d]' % tables.MAX_N_R in L.bfgx_last_error()
    with pytest.raises(ValueError, match=str(tables.MAX_N_R)):
        tables.displacement_rows(np.geomspace(1e-3, 1e2, tables.MAX_N_R + 1), np.ones((1, tables.MAX_N_R + 1)), np.ones((1, tables.MAX_N_R + 1)))


def test_math_probe_refuses_bad_arguments_before_any_device_call():
    """bfgx_math_probe (the per-function probe of csrc/bfgx_math.hpp) checks pointers, the function id and n first: the same answers
    with and without a GPU"""
    L = _lib.load()
    x, y = np.ones(4), np.empty(4)
    fn = _lib.MATH_FN
    assert sorted(fn.values()) == list(range(15))
    assert L.bfgx_math_probe(0, fn['rcp'], 4, None, None, y.ctypes.data, None) == _lib.ERR_INVALID             # NULL a
    assert b'NULL' in L.bfgx_last_error()
    assert L.bfgx_math_probe(0, fn['rcp'], 4, x.ctypes.data, None, None, None) == _lib.ERR_INVALID             # NULL out0
    assert L.bfgx_math_probe(0, fn['atan2'], 4, x.ctypes.data, None, y.ctypes.data, None) == _lib.ERR_INVALID  # two arguments, NULL b
    assert L.bfgx_math_probe(0, fn['sincos_small'], 4, x.ctypes.data, None, y.ctypes.data, None) == _lib.ERR_INVALID   # two results, NULL out1
    for bad in (-1, 15, 1000):
        assert L.bfgx_math_probe(0, bad, 4, x.ctypes.data, x.ctypes.data, y.ctypes.data, y.ctypes.data) == _lib.ERR_INVALID
        assert b'unknown function' in L.bfgx_last_error()
    for n in (-1, (1 << 22) + 1):
        assert L.bfgx_math_probe(0, fn['rcp'], n, x.ctypes.data, None, y.ctypes.data, None) == _lib.ERR_INVALID
        assert b'[0, 4194304]' in L.bfgx_last_error()
    assert L.bfgx_math_probe(0, fn['rcp'], 0, x.ctypes.data, None, y.ctypes.data, None) == _lib.OK             # nothing to do, nothing launched
    from baryonification_amd import engine
    with pytest.raises(ValueError, match="unknown function"):
        engine.math_probe('acos_fast', x)
    with pytest.raises(ValueError, match="takes"):
        engine.math_probe('atan2', x)
