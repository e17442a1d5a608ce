"""What the resident plans share: the handle of the C-side object, its release, and the kernel timers where the C side has them."""
import ctypes as C

import numpy as np

from .. import _lib


class Plan(object):
    """The handle of a C-side plan.  A subclass names the symbol that destroys it (`_destroy`) and makes it with `_create`."""
    _destroy = None

    def _create(self, symbol, *args):
        """self._h = the plan `symbol` makes of args (its last argument, the handle's address, is added here)"""
        h = C.c_void_p()
        _lib.call(symbol, *(args + (C.byref(h),)))
        self._h = h

    def close(self):
        if getattr(self, '_h', None):
            try:
                _lib.call(self._destroy, self._h)
            except Exception:          # interpreter shutdown: module globals may already be gone
                pass
            self._h = None

    __del__ = close


class TimedPlan(Plan):
    """A plan whose kernels the C side can time: `_timing` is the stem of its *_enable / *_read symbols."""
    _timing = None

    def timing_enable(self, on=True):
        _lib.call(self._timing + '_enable', self._h, on)

    def timing_read(self):
        """{kernel kind: (summed ms, launches)} since the last read; synchronises the stream"""
        ms = np.zeros(len(_lib.KERNEL_KINDS))
        n = np.zeros(len(_lib.KERNEL_KINDS), dtype=np.int64)
        _lib.call(self._timing + '_read', self._h, ms.ctypes.data, n.ctypes.data)
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(_lib.KERNEL_KINDS)}
