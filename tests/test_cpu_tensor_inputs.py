"""What every public function that takes "a numpy array or a CUDA tensor" does with a torch tensor that lives on the CPU, pinned
without a GPU: every input below is refused (or not) by the function's own checks before the library touches a device.

The package has two tests for "this is a device tensor", both in baryonification_amd/_tensors.py, and they disagree on a CPU tensor:

  is_cuda_tensor  (sphtfunc, mapstats, pixelfunc, pseudocl): a torch object whose is_cuda is set.  A CPU tensor is NOT one: it is read
                  through np.asarray like any other array, so the function's numpy path and that path's messages apply.
  is_tensor       (flatsky, flatstats and the spectra of engine.fourier): anything with a data_ptr that is not a numpy array.  A CPU
                  tensor IS one, and the check that follows refuses it by name: "... needs a CUDA float64 tensor".

So the outcomes differ and every module keeps its own predicate.  Where the two paths of a function say the same up to the first
device call (mapstats, and ud_grade / get_interp_* / get_all_neighbours of pixelfunc) the case cannot be decided without a GPU; those
keep their predicate too, and the cases below pin only that their numpy-path checks see the tensor."""
import numpy as np
import pytest
import torch

from baryonification_amd import engine
from baryonification_amd.utils import flatsky, flatstats, mapstats, pixelfunc, sphtfunc


def _f8(*shape):
    return torch.zeros(shape, dtype=torch.float64)


I12 = torch.zeros(12, dtype=torch.int64)              # a map of the wrong dtype: _map_input's numpy path names dtype and shape
I3 = torch.zeros(3, dtype=torch.int64)                # alm of an integer dtype: the numpy path refuses, the tensor path would convert
NUMPY_MAP = r"must be a 1-D float array of 12 nside\^2 pixels \(got dtype int64, shape \(12,\)\)"
NUMPY_ALM = r"must be a 1-D complex array$"

# (function, args, kwargs, exception, message): read as an array -- the message is the numpy path's
AS_ARRAY = [
    (sphtfunc.map2alm, (I12,), {}, ValueError, "maps " + NUMPY_MAP),
    (sphtfunc.anafast, (I12,), {}, ValueError, "map1 " + NUMPY_MAP),
    (sphtfunc.smoothing, (I12,), {}, ValueError, "map_in " + NUMPY_MAP),
    (sphtfunc.map2alm_spin, (torch.zeros((2, 12), dtype=torch.int64), 2), {}, ValueError, r"maps\[0\] " + NUMPY_MAP),
    (sphtfunc.alm2map, (I3, 1), {}, ValueError, "alms " + NUMPY_ALM),
    (sphtfunc.alm2cl, (I3,), {}, ValueError, "alms1 " + NUMPY_ALM),
    (sphtfunc.alm2map_spin, (torch.zeros((2, 3), dtype=torch.int64), 1, 1, 1), {}, ValueError, r"alms\[0\] " + NUMPY_ALM),
    (sphtfunc.alm2map_der1, (I3, 1), {}, ValueError, "alm " + NUMPY_ALM),
    (sphtfunc.alm2map_der2, (I3, 1), {}, ValueError, "alm " + NUMPY_ALM),
    (sphtfunc.smoothalm, (I3,), {}, ValueError, "alms " + NUMPY_ALM),
    (sphtfunc.almxfl, (np.zeros(3, dtype=np.complex128), torch.zeros(2, dtype=torch.complex128)), {}, ValueError,
     r"fl must be a 1-D real array \(got dtype complex128, shape \(2,\)\)"),
    (pixelfunc.scatter_add, (_f8(12), np.zeros(1), np.zeros((1, 4), dtype=np.int64), np.zeros((1, 4))), {}, ValueError,
     "hmap must be a C-contiguous 1-D float64 numpy array or a CUDA float64 tensor"),
    # the two paths of these say the same before the first device call: undecidable here, the predicate stays
    (pixelfunc.ud_grade, (_f8(2, 2, 12), 1), {}, ValueError, r"map_in must be one map \(npix,\) or several \(nmaps, npix\) \(got shape \(2, 2, 12\)\)"),
    (pixelfunc.get_interp_weights, (1, _f8(3)), {}, ValueError, "with phi=None, theta must hold integer pixel indices"),
    (pixelfunc.get_interp_val, (_f8(2, 2, 12), 0.0, 0.0), {}, ValueError, r"m must be one map \(npix,\) or several \(nmaps, npix\) \(got shape \(2, 2, 12\)\)"),
    (pixelfunc.get_all_neighbours, (1, _f8(3)), {}, ValueError, "theta must hold integer pixel indices"),
    (mapstats.map_moments, (_f8(2, 2, 12),), {}, ValueError, r"maps must be one map \(npix,\) or several \(nmaps, npix\) \(got shape \(2, 2, 12\)\)"),
    (mapstats.peak_counts, (_f8(2, 12), [0.0, 1.0]), {}, ValueError, r"peak_counts takes one map \(got 2\)"),
    (mapstats.shell_statistics, (_f8(12), [0.0]), {'mask': _f8(11)}, ValueError, r"mask must have the maps' shape \(12,\) \(got \(11,\)\)"),
    (mapstats.minkowski_functionals, (_f8(2, 12), [0.0, 1.0]), {}, ValueError, r"minkowski_functionals takes one map \(got 2\)"),
    (mapstats.minkowski_from_derivatives, (_f8(5, 12), [0.0, 1.0]), {}, ValueError, r"ders must hold six maps \(6, npix\) \(got shape \(5, 12\)\)"),
]

M8, C8 = _f8(8, 8), _f8(8, 8, 8)
X = _f8(4)

# (function, args, kwargs, message): taken for a tensor and refused by name, ValueError
AS_TENSOR = [
    (flatsky.rfft2, (M8,), {}, "rfft2 needs a CUDA float64 tensor"),
    (flatsky.irfft2, (_f8(8, 8, 2), 8), {}, r"irfft2 needs a CUDA float64 tensor of shape \[N\]\[fft_pitch\(N\)\]\[2\]"),
    (flatsky.power_spectrum_2d, (M8, 1.0), {}, "cross_power_spectrum_2d needs a CUDA float64 tensor"),
    (flatsky.cross_power_spectrum_2d, (M8, M8, 1.0), {}, "cross_power_spectrum_2d needs a CUDA float64 tensor"),
    (flatsky.cross_power_spectrum_2d, (M8, np.zeros((8, 8)), 1.0), {}, "cross_power_spectrum_2d needs numpy arrays or CUDA float64 tensors, not one of each"),
    (flatsky.smoothing_2d, (M8, 1.0), {'sigma': 0.1}, "smoothing_2d needs a CUDA float64 tensor"),
    (flatsky.kappa_to_shear_2d, (M8,), {}, "kappa_to_shear_2d needs a CUDA float64 tensor"),
    (flatsky.shear_to_kappa_2d, (M8, M8), {}, "shear_to_kappa_2d needs a CUDA float64 tensor"),
    (flatstats.derivatives_2d, (M8, 1.0), {}, "derivatives_2d needs a CUDA float64 tensor"),
    (flatstats.peak_counts_2d, (M8, [0.0, 1.0]), {}, "peak_counts_2d needs a CUDA float64 tensor"),
    (flatstats.peak_counts_2d, (np.zeros((8, 8)), [0.0, 1.0]), {'mask': M8}, "peak_counts_2d needs numpy arrays or CUDA tensors, not one of each"),
    (flatstats.minkowski_functionals_2d, (M8, 1.0, [0.0, 1.0]), {}, "minkowski_functionals_2d needs a CUDA float64 tensor"),
    (flatstats.patch_statistics, (M8, 1.0, [0.0]), {}, "patch_statistics needs a CUDA float64 tensor"),
    (flatstats.patch_statistics, (_f8(2, 8, 8), 1.0, [0.0]), {}, "patch_statistics needs a CUDA float64 tensor"),
    (engine.cross_power_spectrum, (C8, C8, 1.0), {}, "cross_power_spectrum needs a CUDA float64 tensor"),
    (engine.cross_power_spectrum, (C8, np.zeros((8, 8, 8)), 1.0), {}, "cross_power_spectrum needs two numpy arrays or two CUDA float64 tensors, not one of each"),
    (engine.interlaced_power_spectrum, (C8, C8, 1.0), {}, "interlaced_power_spectrum needs a CUDA float64 tensor"),
    (engine.interlaced_power_spectrum, (np.zeros((8, 8, 8)), C8, 1.0), {},
     "interlaced_power_spectrum needs two numpy arrays or two CUDA float64 tensors, not one of each"),
    (engine.particle_power_spectrum, ((X, X, X), None, 8, 1.0), {}, "particle_power_spectrum needs 1-D CUDA float64 tensors"),
    (engine.particle_power_spectrum, ((X, X, np.zeros(4)), None, 8, 1.0), {}, "particle_power_spectrum needs numpy arrays or CUDA float64 tensors, not some of each"),
    (engine.particle_power_spectrum, ((np.zeros(4),) * 3, X, 8, 1.0), {}, "particle_power_spectrum needs numpy arrays or CUDA float64 tensors, not some of each"),
    (engine.bispectrum, (C8, 1.0, [1.0, 2.0, 3.0]), {}, "bispectrum needs a numpy array or a CUDA float64 tensor"),
]


def _name(case):
    return "%s.%s" % (case[0].__module__.rsplit('.', 1)[-1], case[0].__name__)


@pytest.mark.parametrize('case', AS_ARRAY, ids=[_name(c) + '-%d' % i for i, c in enumerate(AS_ARRAY)])
def test_a_cpu_tensor_is_read_as_an_array(case):
    fn, args, kwargs, exc, message = case
    with pytest.raises(exc, match=message):
        fn(*args, **kwargs)


@pytest.mark.parametrize('case', AS_TENSOR, ids=[_name(c) + '-%d' % i for i, c in enumerate(AS_TENSOR)])
def test_a_cpu_tensor_is_refused_as_a_tensor_that_is_not_on_the_device(case):
    fn, args, kwargs, message = case
    with pytest.raises(ValueError, match="^" + message + "$"):
        fn(*args, **kwargs)


def test_the_two_predicates_as_they_stand():
    from baryonification_amd import _tensors
    t = _f8(3)
    assert not _tensors.is_cuda_tensor(t) and _tensors.is_tensor(t)
    for x in (np.zeros(3), [0.0], None, 1.0):
        assert not _tensors.is_cuda_tensor(x) and not _tensors.is_tensor(x)
    assert sphtfunc.unseen_mask(torch.full((2,), sphtfunc.UNSEEN, dtype=torch.float64)).all()       # array or tensor alike: no predicate
