"""IQ balance per wideband source over the C ABI of ``include/rtlfm_iq.h``: the policy between the second moments the
device takes of every source's raw bytes (option ``source_iq``, ``GpuDemod.source_iq_sums``) and the four Q14 coefficients
the device applies (``GpuDemod.set_source_iq``).

The engine is host code inside ``librtlfm_hip.so``; this class only marshals records into it.  The loop::

    demod.run(...); iq.update(demod); events = iq.poll(); demod.set_source_iq(iq.coeffs())
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import RtlfmIqEvent, check


def compute(total, deadband: int = 164, min_rms: int = 2):
    """``rtlfm_iq_compute`` on one set of totals (a record of ``capi.IQ_SUMS_DTYPE``): (verdict, coef, g_q14, s_q14) with
    verdict one of ``capi.IQ_OK`` / ``IQ_WEAK`` / ``IQ_REJECTED``; coef is None unless the verdict is ``IQ_OK``."""
    lib = capi.load()
    t = np.ascontiguousarray(total, dtype=capi.IQ_SUMS_DTYPE).reshape(1)
    coef = np.zeros(4, dtype=np.int16)
    g, s = C.c_int32(), C.c_int32()
    v = check(lib.rtlfm_iq_compute(t.ctypes.data, deadband, min_rms, coef.ctypes.data, C.byref(g), C.byref(s)), "rtlfm_iq_compute")
    return v, (tuple(int(c) for c in coef) if v == capi.IQ_OK else None), g.value, s.value


class IqBalance:
    """One estimator per source; events come out in the order the decisions fell."""

    def __init__(self, nsources: int, window: int | None = None, deadband: int | None = None, min_rms: int | None = None,
                 min_step: int | None = None):
        self.lib = capi.load()
        self.nsources = int(nsources)
        e = C.c_void_p()
        check(self.lib.rtlfm_iq_create(self.nsources, C.byref(e)), "rtlfm_iq_create")
        self._e = e
        if any(v is not None for v in (window, deadband, min_rms, min_step)):
            self.set_params(16 if window is None else window, 164 if deadband is None else deadband,
                            2 if min_rms is None else min_rms, 8 if min_step is None else min_step)

    def close(self):
        if getattr(self, "_e", None):
            self.lib.rtlfm_iq_destroy(self._e)
            self._e = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, window: int = 16, deadband: int = 164, min_rms: int = 2, min_step: int = 8):
        check(self.lib.rtlfm_iq_set_params(self._e, window, deadband, min_rms, min_step), "rtlfm_iq_set_params")

    def feed(self, source: int, records):
        """Consecutive buffers of ``source``: records of ``capi.IQ_SUMS_DTYPE``."""
        r = np.ascontiguousarray(records, dtype=capi.IQ_SUMS_DTYPE).ravel()
        check(self.lib.rtlfm_iq_feed(self._e, source, r.ctypes.data, r.size), "rtlfm_iq_feed")

    def update(self, demod):
        """Feed every source from the last run of a ``GpuDemod`` with channels on and ``set_option("source_iq", 1)``."""
        check(self.lib.rtlfm_iq_update(self._e, demod._h), "rtlfm_iq_update")

    def poll(self, cap: int = 1024) -> list[dict]:
        """Every decision so far, as dictionaries (the fields of ``rtlfm_iq_event``)."""
        out = []
        ev = (RtlfmIqEvent * cap)()
        n = C.c_int()
        while True:
            check(self.lib.rtlfm_iq_poll(self._e, ev, cap, C.byref(n)), "rtlfm_iq_poll")
            out += [ev[i].as_dict() for i in range(n.value)]
            if n.value < cap:
                return out

    def coeffs(self) -> np.ndarray:
        """The coefficients as they rule now, int16 [nsources, 4]: what ``GpuDemod.set_source_iq`` takes."""
        out = np.zeros((self.nsources, 4), dtype=np.int16)
        check(self.lib.rtlfm_iq_coeffs(self._e, out.ctypes.data), "rtlfm_iq_coeffs")
        return out
