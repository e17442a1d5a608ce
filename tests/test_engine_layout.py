"""baryonification_amd.engine is a package split by topic; every name the single module engine.py held is still a name of the
package, the same object as in the module that defines it, and importing the package does not import torch."""
import importlib
import os
import subprocess
import sys

import pytest

from baryonification_amd import engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the public names of engine.py before the split (those it defined: not C, np, _lib), by the module that holds them now
HOME = {
    'shell': ['ShellPlan', 'model_from_tables'],
    'grid': ['GridPlan', 'deposit_particles_slab_device', 'deposit_particles_device', 'deposit_cloud_device', 'route_particles_count_device',
             'route_particles_fill_device'],
    'snapshot': ['SnapshotPlan', 'baryonify_snapshot_device'],
    'fourier': ['fft_slab_planes_device', 'fft_slab_axis0_pk_device', 'fft_slab_axis0_xpk_device', 'fft_slab_axis0_device',
                'ifft_slab_planes_device', 'fft_pitch', 'power_spectrum_work_doubles', 'power_spectrum_device', 'power_spectrum',
                'power_spectrum_tensor', 'cross_power_spectrum_work_doubles', 'cross_power_spectrum_device', 'WINDOW_ORDERS',
                'cross_power_spectrum', 'interlaced_power_spectrum_device', 'interlaced_power_spectrum', 'particle_power_spectrum_work_doubles',
                'particle_power_spectrum_device', 'particle_power_spectrum', 'bispectrum_work_doubles', 'bispectrum_shell_fields_device',
                'bispectrum_device', 'BISPECTRUM_MAX_BINS', 'BISPECTRUM_MAX_TRIANGLES', 'bispectrum_triangles', 'bispectrum'],
    'flat': ['fft2_work_doubles', 'rfft2_device', 'irfft2_device', 'power_spectrum_2d_device', 'FILTER_KINDS_2D', 'filter_map_2d_device',
             'DERIVATIVE_KINDS_2D', 'derivatives_2d_work_doubles', 'derivatives_2d_device', 'peaks_2d_device', 'kappa_to_shear_2d_device',
             'shear_to_kappa_2d_device'],
    'sphere': ['sht_alm_size', 'sht_work_doubles', 'sht_spin_work_doubles', 'ShtPlan', 'alm2cl_device', 'almxfl_device', 'sht_plan',
               'sht_map2alm_host', 'sht_alm2map_host', 'sht_map2alm_spin_host', 'sht_alm2map_spin_host', 'sht_almxfl_host', 'sht_alm2cl_host',
               'sht_anafast_host', 'PCL_MAX_LMAX', 'PCL_MAX_LW', 'pcl_coupling_host', 'pcl_coupling_device'],
    'probe': ['math_probe'],
}
NAMES = [(module, name) for module, names in HOME.items() for name in names]


def test_the_list_is_the_67_names_of_the_single_module():
    assert len(NAMES) == 67 == len(set(name for _, name in NAMES))


@pytest.mark.parametrize('module,name', NAMES, ids=[name for _, name in NAMES])
def test_a_public_name_is_the_object_of_its_home_module(module, name):
    home = importlib.import_module('baryonification_amd.engine.' + module)
    assert hasattr(engine, name), "engine.%s is gone" % name
    assert getattr(engine, name) is getattr(home, name)
    obj = getattr(home, name)
    if callable(obj):
        assert obj.__module__ == home.__name__, "%s is defined in %s, not in %s" % (name, obj.__module__, home.__name__)


def test_window_order_is_public_and_says_who_asked():
    assert engine.window_order is engine.fourier.window_order
    assert [engine.window_order(w, "x") for w in (0, 3, 'none', 'NGP', 'cic', 'Tsc')] == [0, 3, 0, 1, 2, 3]
    for bad in (True, 4, -1, 'pcs', 1.5, None):
        with pytest.raises(ValueError, match="^flat: window must be 0, 1, 2, 3 or 'none', 'ngp', 'cic', 'tsc'$"):
            engine.window_order(bad, "flat")


def test_the_plans_share_one_base_that_releases_the_handle():
    from baryonification_amd.engine._plan import Plan, TimedPlan
    assert issubclass(engine.ShellPlan, TimedPlan) and issubclass(engine.GridPlan, TimedPlan) and issubclass(engine.SnapshotPlan, Plan)
    assert not issubclass(engine.SnapshotPlan, TimedPlan) and not hasattr(engine.SnapshotPlan, 'timing_read')       # the C side has none
    for cls in (engine.ShellPlan, engine.GridPlan, engine.SnapshotPlan):
        assert 'close' not in vars(cls) and '__del__' not in vars(cls) and cls.__del__ is Plan.close
        p = cls.__new__(cls)                  # never created: close() and __del__ have nothing to release
        p.close()
        assert getattr(p, '_h', None) is None


def test_importing_the_package_does_not_import_torch():
    code = ("import sys; import baryonification_amd.engine as e; from baryonification_amd import _tensors; "
            "assert e.ShtPlan and e.rfft2_device and e.power_spectrum_tensor; print('torch' in sys.modules)")
    out = subprocess.run([sys.executable, '-c', code], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == 'False'
