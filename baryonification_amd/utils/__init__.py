from .io import *
from .cosmology import *
from .Tabulate import *
from .Parallelize import *
from .Pixel import *
from .sphtfunc import map2alm, alm2map, alm2cl, anafast, map2alm_spin, alm2map_spin
from .pixelfunc import ud_grade, get_interp_weights, get_interp_val, UNSEEN
