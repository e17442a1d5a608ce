"""What every synchronous host entry of libbfgx (numpy in, numpy out: the entries built on HostCall, csrc/bfgx_hostcall.hpp) refuses,
without a GPU: a NULL required pointer; a bad scalar, with the very message its _device sibling gives (the checks are stated once); and,
where no device is visible, the call itself, with the results untouched."""
import numpy as np
import pytest

from baryonification_amd import _lib

SENTINEL = -7.5


def _f(n, start=1.0):
    return np.arange(n, dtype=np.float64) + start


def _out(n, dtype=np.float64):
    return np.full(n, SENTINEL, dtype=dtype)


def _aligned16(n):
    """n float64 that start on a 16-byte boundary (the work arrays of the SHT _device entries)"""
    a = np.zeros(n + 1)
    return a[(a.ctypes.data // 8) % 2:][:n]


# name -> (valid small arguments after `device`, positions of the results among them).  Every array is a required pointer; an optional
# argument that is left out is None.  alm of lmax = mmax = 2 are 6 complex numbers, a map of nside 1 is 12 pixels.
def entries():
    r4 = np.array([1.0, 2.0, 4.0, 8.0])
    i64 = lambda *v: np.array(v, dtype=np.int64)
    return {
        'bfgx_project_profile': ([1, 2, _f(2), _f(2), 1, _f(1), 1.0, _out(1)], [7]),
        'bfgx_enclosed_mass_from_sigma': ([1, 3, _f(3), _f(3), 1, _f(1), _out(1)], [6]),
        'bfgx_enclosed_mass_3d': ([1, 3, _f(3), _f(3), 1, _f(1), _out(1)], [6]),
        'bfgx_enclosed_mass_2d': ([1, 2, _f(2), _f(2), 1.0, 3, _f(3), 1, _f(1), _out(1)], [9]),
        'bfgx_displacement_rows': ([1, 3, _f(3), _f(3), _f(3), _out(3), _out(1, np.int32)], [5, 6]),
        'bfgx_pressure_profile': ([1, _f(500), _f(500), _f(500), 1, _f(1), 4.0, _out(1)], [7]),
        'bfgx_fftlog_transform': ([1, 4, r4, _f(4), 3, 0.0, 0.0, _out(4), _out(4)], [7, 8]),
        'bfgx_fftlog_convolve': ([1, 4, r4, _f(4), 3, 0.0, 0.0, 0.0, _f(4), 1, _f(1), 1.0, _out(1)], [12]),
        'bfgx_pchip_rows': ([1, 4, r4, _f(4), 1, _f(1), _out(1)], [6]),
        'bfgx_math_probe': ([_lib.MATH_FN['mul_add_nc'], 1, _f(1), _f(1), _out(1), None], [4]),
        'bfgx_regrid_pixels': ([2, 5, 1, _f(2), _f(1), _out(25)], [5]),
        'bfgx_deposit_particles': ([3, 1, _f(1), _f(1), _f(1), None, 1, _f(2), _out(1)], [8]),
        'bfgx_power_spectrum': ([8, _f(512), 1.0, 4, _out(4), _out(4), _out(4, np.int64)], [4, 5, 6]),
        'bfgx_sht_almxfl': ([2, 2, 1, _f(1), _f(12), _out(12)], [5]),
        'bfgx_sht_map2alm': ([1, 2, 2, 0, _f(12), _out(12)], [5]),
        'bfgx_sht_alm2map': ([1, 2, 2, _f(12), _out(12)], [4]),
        'bfgx_sht_alm2cl': ([2, 2, 2, _f(12), None, _out(3)], [5]),
        'bfgx_sht_anafast': ([1, 2, 2, 0, _f(12), None, _out(3), None, None], [6]),
        'bfgx_sht_map2alm_spin': ([1, 2, 2, 1, _f(24), _out(24)], [5]),
        'bfgx_sht_alm2map_spin': ([1, 2, 2, 1, _f(24), _out(24)], [5]),
        'bfgx_hpx_ud_grade': ([2, 1, 1, 0, 0, 0, 1.0, 1, 1, _f(48), _out(12)], [10]),
        'bfgx_hpx_interp_weights': ([1, 0, 1, _f(1), _f(1), None, _out(4, np.int64), _out(4)], [6, 7]),
        'bfgx_hpx_interp_val': ([1, 0, 1, 1, _f(12), 1, _f(1), _f(1), _out(1)], [8]),
        'bfgx_hpx_neighbours': ([1, 0, 1, i64(3), _out(8, np.int64)], [4]),
        'bfgx_hpx_scatter_add': ([12, _out(12), 1, _f(1), i64(0, 1, 2, 3), _f(4)], [1]),
    }


NAMES = sorted(entries())


def _call(name, args):
    L = _lib.load()
    rc = getattr(L, name)(0, *[a.ctypes.data if isinstance(a, np.ndarray) else a for a in args])
    return rc, L.bfgx_last_error()


@pytest.mark.parametrize('name', NAMES)
def test_null_required_pointer_is_refused(name):
    args, _ = entries()[name]
    pointers = [i for i, a in enumerate(args) if isinstance(a, np.ndarray)]
    assert pointers
    for i in pointers:
        bad = list(args)
        bad[i] = None
        rc, msg = _call(name, bad)
        assert rc == _lib.ERR_INVALID and b'NULL' in msg, (name, i, rc, msg)


# operations whose host entry and _device entry take the same arguments (the _device entry: a stream after `device`, and work arrays at
# the end): (host entry, position of a scalar among the arguments above, a value it may not have, work arrays of the _device entry)
SIBLINGS = [
    ('bfgx_hpx_ud_grade', 0, 3, 0),                       # nside_in: no power of two
    ('bfgx_hpx_ud_grade', 1, 16384, 0),                   # nside_out > 8192
    ('bfgx_hpx_ud_grade', 2, 0, 0),                       # nmaps
    ('bfgx_hpx_interp_weights', 0, 0, 0),                 # nside
    ('bfgx_hpx_interp_weights', 2, -1, 0),                # n
    ('bfgx_hpx_interp_val', 2, 0, 0),                     # nmaps
    ('bfgx_hpx_interp_val', 3, 2, 0),                     # dtype
    ('bfgx_hpx_neighbours', 0, 8193, 0),                  # nside
    ('bfgx_hpx_neighbours', 2, 2 ** 60, 0),               # n: 8 n overflows
    ('bfgx_hpx_scatter_add', 0, 0, 0),                    # npix
    ('bfgx_hpx_scatter_add', 2, 2 ** 61, 0),              # n: 4 n overflows
    ('bfgx_sht_almxfl', 2, -1, 0),                        # nfl
    ('bfgx_sht_almxfl', 1, 3, 0),                         # mmax > lmax
    ('bfgx_sht_alm2cl', 2, -1, 0),                        # lmax_out
    ('bfgx_sht_map2alm', 3, -1, 1),                       # iter
    ('bfgx_sht_map2alm', 0, 0, 1),                        # nside
    ('bfgx_sht_alm2map', 2, 3, 1),                        # mmax > lmax
    ('bfgx_sht_alm2map', 1, 40000, 1),                    # lmax
    ('bfgx_sht_map2alm_spin', 3, 0, 2),                   # spin 0
    ('bfgx_sht_alm2map_spin', 3, 3, 2),                   # spin > lmax
    ('bfgx_sht_alm2map_spin', 0, -1, 2),                  # nside
]


@pytest.mark.parametrize('name,pos,value,nwork', SIBLINGS)
def test_bad_scalar_is_refused_alike_by_host_and_device_entry(name, pos, value, nwork):
    args, _ = entries()[name]
    bad = list(args)
    assert not isinstance(bad[pos], np.ndarray)
    bad[pos] = value
    rc_h, msg_h = _call(name, bad)
    # (host arrays stand in for device arrays: the call is refused before any of them is used)
    rc_d, msg_d = _call(name + '_device', [None] + bad + [_aligned16(8) for _ in range(nwork)])
    assert rc_h == rc_d == _lib.ERR_INVALID, (rc_h, msg_h, rc_d, msg_d)
    assert msg_h == msg_d and msg_h, (msg_h, msg_d)


def test_sibling_table_names_every_operation_with_a_device_entry_of_the_same_arguments():
    with_device = {n for n in NAMES if n + '_device' in _lib.SYMBOLS} - {'bfgx_deposit_particles', 'bfgx_power_spectrum'}
    assert with_device == {s[0] for s in SIBLINGS}


@pytest.mark.parametrize('name', NAMES)
def test_without_a_device_the_call_is_refused_and_the_results_stay(name):
    if _lib.load().bfgx_device_count() > 0:
        pytest.skip("GPU present")
    args, outs = entries()[name]
    rc, msg = _call(name, args)
    assert rc == _lib.ERR_NO_DEVICE and b'no HIP device' in msg, (rc, msg)
    for i in outs:
        assert np.all(args[i] == np.asarray(SENTINEL).astype(args[i].dtype)), (name, i)
