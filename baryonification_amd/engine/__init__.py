"""
Front-end of the C ABI for inputs that already lie in HBM, split by topic as the C side is:

    shell.py      ShellPlan (bfgx_plan), model_from_tables
    grid.py       GridPlan (bfgx_grid_plan), the particle deposits and the particle routing of a slab-decomposed grid
    snapshot.py   SnapshotPlan (bfgx_snapshot_plan), baryonify_snapshot_device
    fourier.py    3-D P(k), cross / interlaced / particle spectra, the bispectrum, the slab FFT steps, WINDOW_ORDERS
    flat.py       the 2-D `_device` entries (transforms, spectra, filters, derivatives, Kaiser-Squires, peaks_2d_device)
    sphere.py     ShtPlan and sht_plan, the SHT device and host entries, pcl_coupling_*
    probe.py      math_probe (test infrastructure)

Every public name of these modules is also a name of this package (`engine.ShellPlan`, `engine.rfft2_device`, ...), the same object.

Pointers are plain integers (`tensor.data_ptr()`, `array.ctypes.data`; 0 is NULL), the stream a raw hipStream_t handle
(`torch.cuda.current_stream().cuda_stream`); `_lib.call` converts them from the declared signature.  Importing this package does
not import torch.  The plans and the `_device` entries that take pointers never do; what takes or returns tensors -- ShtPlan and the
tensor entries of sphere.py, and power_spectrum_tensor, cross_power_spectrum, interlaced_power_spectrum, particle_power_spectrum and
bispectrum of fourier.py when given tensors -- imports it when called.

Used by bench.py, by utils/ and by the multi-GPU drivers (utils/Parallelize.py, utils/GridSlabs.py); the drop-in runners use the
one-shot host entry points instead.
"""
from .shell import ShellPlan, model_from_tables
from .grid import (GridPlan, deposit_particles_slab_device, deposit_particles_device, deposit_cloud_device, route_particles_count_device,
                   route_particles_fill_device)
from .snapshot import SnapshotPlan, baryonify_snapshot_device
from .fourier import (WINDOW_ORDERS, window_order, fft_slab_planes_device, fft_slab_axis0_pk_device, fft_slab_axis0_xpk_device,
                      fft_slab_axis0_device, ifft_slab_planes_device, fft_pitch, power_spectrum_work_doubles, power_spectrum_device,
                      power_spectrum, power_spectrum_tensor, cross_power_spectrum_work_doubles, cross_power_spectrum_device,
                      cross_power_spectrum, interlaced_power_spectrum_device, interlaced_power_spectrum, particle_power_spectrum_work_doubles,
                      particle_power_spectrum_device, particle_power_spectrum, bispectrum_work_doubles, bispectrum_shell_fields_device,
                      bispectrum_device, BISPECTRUM_MAX_BINS, BISPECTRUM_MAX_TRIANGLES, bispectrum_triangles, bispectrum)
from .flat import (fft2_work_doubles, rfft2_device, irfft2_device, power_spectrum_2d_device, FILTER_KINDS_2D, DERIVATIVE_KINDS_2D,
                   filter_map_2d_device, derivatives_2d_work_doubles, derivatives_2d_device, peaks_2d_device, kappa_to_shear_2d_device,
                   shear_to_kappa_2d_device)
from .sphere import (sht_alm_size, sht_work_doubles, sht_spin_work_doubles, ShtPlan, alm2cl_device, almxfl_device, sht_plan, sht_map2alm_host,
                     sht_alm2map_host, sht_map2alm_spin_host, sht_alm2map_spin_host, sht_almxfl_host, sht_alm2cl_host, sht_anafast_host,
                     PCL_MAX_LMAX, PCL_MAX_LW, pcl_coupling_host, pcl_coupling_device)
from .probe import math_probe
