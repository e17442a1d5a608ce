"""
Plain-Python models for the per-halo (callable) routes of the grid runners: closed forms with a radius of their own, from M
and a only (no cosmology calls), so that the reference (tests/golden/make_golden_callable.py) and this package evaluate the very
same function.  Each has a NaN band and non-zero values beyond epsilon_max * R: the runners' isfinite / radius masks are exercised.
A model counts its calls and, when `record` is set, keeps the arguments of the first `record` calls.
"""
import numpy as np


def own_radius(M, a):
    """comoving radius of the models, Mpc: ~R200c-sized, a closed form of M and a"""
    return 0.9 * (M / 1e14) ** (1.0 / 3.0) * (1.0 + 0.1 * (1.0 / a - 1.0))


class _Recording(object):
    bfgx_exact = True

    def __init__(self, record=0):
        self.calls = 0
        self.record = record
        self.seen = []

    def _note(self, r, M, a):
        self.calls += 1
        if len(self.seen) < self.record:
            self.seen.append((np.array(r, copy=True), M, a))


class CallableDisplacement(_Recording):
    """displacement(r, M, a): an inward pull with a NaN band at 1.30 < r / R < 1.33 and a tail that runs past any epsilon_max"""

    def displacement(self, r, M, a):
        self._note(r, M, a)
        R = own_radius(M, a)
        x = np.asarray(r) / R
        d = -0.06 * R * x * np.exp(-x) / (1.0 + x * x) + 1e-4 * R / (1.0 + x)
        return np.where((x > 1.30) & (x < 1.33), np.nan, d)


class CallableProfile(_Recording):
    """projected / real (cosmo, r, M, a): a cored profile with a NaN band at 0.50 < r / R < 0.52, non-zero out to any radius"""

    def _f(self, r, M, a, s):
        R = own_radius(M, a)
        x = np.asarray(r) / R
        P = s * (M / 1e14) * np.exp(-0.5 * x) / (1.0 + x) ** 2
        return np.where((x > 0.50) & (x < 0.52), np.nan, P)

    def projected(self, cosmo, r, M, a):
        self._note(r, M, a)
        return self._f(r, M, a, 1.0)

    def real(self, cosmo, r, M, a):
        self._note(r, M, a)
        return self._f(r, M, a, 3.0)
