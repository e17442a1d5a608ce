from .io import *
from .cosmology import *
from .Tabulate import *
from .Parallelize import *
from .Pixel import *
from .sphtfunc import map2alm, alm2map, alm2cl, anafast, map2alm_spin, alm2map_spin, gauss_beam, tophat_beam, almxfl, smoothalm, smoothing, alm2map_der1, alm2map_der2
from .pixelfunc import ud_grade, get_interp_weights, get_interp_val, get_all_neighbours, UNSEEN
from .mapstats import (map_moments, peak_counts, shell_statistics, moment_exponents, minkowski_functionals,
                       minkowski_from_derivatives, minkowski_gaussian)
from .flatsky import rfft2, irfft2, power_spectrum_2d, cross_power_spectrum_2d, smoothing_2d, kappa_to_shear_2d, shear_to_kappa_2d
from .flatstats import derivatives_2d, peak_counts_2d, minkowski_functionals_2d, minkowski_gaussian_2d, patch_statistics
from .pseudocl import mode_coupling_matrix, mask_spectrum, ClBins, pseudo_cl, PseudoClWorkspace, decoupled_cl
