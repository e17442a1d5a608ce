"""_lib.call(name, *args): arguments converted once from the signature _lib.SYMBOLS declares, a status mapped to its exception.
Everything here is answered by the library before it touches a device."""
import ctypes as C

import numpy as np
import pytest

from baryonification_amd import _lib, synthetic as syn


def test_numbers_come_back_as_numbers_and_numpy_scalars_are_taken():
    L = _lib.load()
    for n in (8, 64, 512):
        assert _lib.call('bfgx_fft_pitch', n) == L.bfgx_fft_pitch(n) == _lib.call('bfgx_fft_pitch', np.int64(n)) == _lib.call('bfgx_fft_pitch', np.uint8(n) if n < 256 else np.int32(n))
        assert _lib.call('bfgx_power_spectrum_work_doubles', np.int32(n)) == L.bfgx_power_spectrum_work_doubles(n) > 0
    assert _lib.call('bfgx_sht_work_doubles', np.int64(16), 47, np.int16(47)) == L.bfgx_sht_work_doubles(16, 47, 47) > 0
    assert _lib.call('bfgx_sht_work_doubles', 4096, 10, 10) < 0                    # refused: a negative count, not a status to raise on
    assert _lib.call('bfgx_mapstats_moment_terms', 3, 4) == 31
    assert _lib.call('bfgx_abi_version') == _lib.ABI_VERSION and _lib.call('bfgx_device_count') >= 0        # c_int, but no statuses
    assert isinstance(_lib.call('bfgx_last_error'), bytes)
    assert _lib.NOT_STATUS <= set(_lib.SYMBOLS)


def test_zero_and_none_both_arrive_as_null():
    for null in (0, None, np.int64(0)):
        with pytest.raises(ValueError, match='NULL'):
            _lib.call('bfgx_power_spectrum_device', 0, null, 64, null, np.float32(100.0), np.int64(10), null, null, null, null)
        n = C.c_int64(0)
        with pytest.raises(ValueError, match='NULL'):
            _lib.call('bfgx_grid_baryonify_device', null, None, null, null, null, C.byref(n))
    with pytest.raises(TypeError):                                                   # an integer argument is not optional
        _lib.call('bfgx_power_spectrum_device', 0, None, None, None, 100.0, 10, None, None, None, None)


def test_a_status_maps_to_the_exception_of_check():
    host = np.zeros(64)
    p = host.ctypes.data
    with pytest.raises(NotImplementedError, match=r"^power spectrum needs n_grid = 2\^m with 8 <= n_grid <= 1024$"):
        _lib.call('bfgx_power_spectrum_device', 0, None, 12, p, 100.0, 4, p, p, p, p)
    rc = _lib.load().bfgx_power_spectrum_device(0, None, 12, p, 100.0, 4, p, p, p, p)
    assert rc == _lib.ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError, match="power spectrum needs n_grid"):
        _lib.check(rc)
    st = _lib.bfgx_stats()
    with pytest.raises(ValueError):
        _lib.call('bfgx_baryonify_snapshot_records_map', None, None, 3, 100.0, 0.0, 0, None, 32, 8, 16, 24, 0, 8, None, None, None, st)
    assert not host.any()


def test_struct_instances_go_by_reference_and_references_pass_as_they_are():
    cosmo = _lib.make_cosmo(syn.COSMO)
    a = np.array([1.0, 0.5, 0.25])
    by_value, by_ref, by_hand = np.zeros(3), np.zeros(3), np.zeros(3)
    assert _lib.call('bfgx_cosmo_E2', cosmo, a.size, a.ctypes.data, by_value.ctypes.data) is None             # OK: nothing to return
    _lib.call('bfgx_cosmo_E2', C.byref(cosmo), np.int64(a.size), a.ctypes.data, by_ref.ctypes.data)
    assert _lib.load().bfgx_cosmo_E2(C.byref(cosmo), a.size, a.ctypes.data, by_hand.ctypes.data) == _lib.OK
    assert abs(by_hand[0] - 1.0) < 1e-3 and by_hand[2] > by_hand[1] > 1.0
    assert np.array_equal(by_value, by_hand) and np.array_equal(by_ref, by_hand)
    # out-arguments and ctypes arrays reach the function untouched
    lo, hi, least = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
    _lib.call('bfgx_debug_host_spans', C.byref(lo), C.byref(hi), C.byref(least))
    assert lo.value >= 0 and hi.value >= 0
    h = C.c_void_p()
    devs = (C.c_int32 * 1)(0)
    with pytest.raises(ValueError):
        _lib.call('bfgx_shell_pairs_begin', None, None, 64, 0, 0, C.byref(h), devs)
    assert not h.value


def test_a_wrong_argument_count_names_the_symbol():
    with pytest.raises(TypeError, match=r"^bfgx_fft_pitch takes 1 arguments \(0 given\)$"):
        _lib.call('bfgx_fft_pitch')
    with pytest.raises(TypeError, match=r"^bfgx_power_spectrum_device takes 10 arguments \(3 given\)$"):
        _lib.call('bfgx_power_spectrum_device', 0, 0, 64)
    with pytest.raises(KeyError):
        _lib.call('bfgx_no_such_entry')


def test_every_symbol_has_one_converter_per_argument():
    _lib.load()
    assert set(_lib._calls) == set(_lib.SYMBOLS)
    for name, (res, args) in _lib.SYMBOLS.items():
        fn, conv, status = _lib._calls[name]
        assert len(conv) == len(args)
        assert status == (res is C.c_int and name not in _lib.NOT_STATUS)
        for t, c in zip(args, conv):
            if t is C.c_void_p:
                assert c(0) is None and c(None) is None and c(np.uint64(7)) == 7
            elif t is C.c_double:
                assert c is float
            elif isinstance(t, type) and issubclass(t, C._Pointer):
                ref = C.byref(C.c_int64(0))
                assert c(ref) is ref
            else:
                assert c is int
