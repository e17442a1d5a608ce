"""One device function of csrc/bfgx_math.hpp at a time, for the tests that check them against mpmath."""
import numpy as np

from .. import _lib, _tensors


def math_probe(fn_name, a, b=None, c=None, device=0):
    """One function of csrc/bfgx_math.hpp evaluated elementwise on the GPU (bfgx_math_probe; names in _lib.MATH_FN).  Returns one array,
    or (sin, cos) for the sincos functions.  'atan2' takes (a, b) = (y, x), 'mul_add_nc' computes a * b + c without contraction,
    'ring_theta' takes a = nside, b = ring.  Test infrastructure: no product path calls it."""
    if fn_name not in _lib.MATH_FN:
        raise ValueError("math_probe: unknown function %r" % (fn_name,))
    a = _lib.f8(a).ravel()
    two = fn_name in _lib.MATH_FN_TWO_ARGS
    if two != (b is not None) or (fn_name == 'mul_add_nc') != (c is not None):
        raise ValueError("math_probe: %s takes %s" % (fn_name, "(a, b, c)" if fn_name == 'mul_add_nc' else "(a, b)" if two else "(a)"))
    b = _lib.f8(b).ravel() if two else None
    out0 = _lib.f8(c).ravel().copy() if c is not None else np.empty(a.size)
    out1 = np.empty(a.size) if fn_name in _lib.MATH_FN_TWO_RESULTS else None
    if (two and b.size != a.size) or out0.size != a.size:
        raise ValueError("math_probe: arguments differ in length")
    _lib.call('bfgx_math_probe', device, _lib.MATH_FN[fn_name], a.size, a.ctypes.data, _tensors.ptr(b), out0.ctypes.data, _tensors.ptr(out1))
    return out0 if out1 is None else (out0, out1)
