"""The channel bank's slot allocator over the C ABI of ``include/rtlfm_slots.h``: a few demodulator slots per source
that follow the activity the bank's survey (``GpuDemod.bank_survey``) shows.

The engine is host code inside ``librtlfm_hip.so``, integers only; this class only marshals arrays into it.  One
``step`` per run; ``bins`` is ready for ``GpuDemod.set_channel_bins``.  A decision made from run r's survey acts on run
r + 1: a transmission's first buffer is lost.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import RtlfmSlotsCfg, RtlfmSlotsEvent, check


class SlotAllocator:
    """``slots`` slots for each of ``nsources`` sources over ``K`` bins."""

    def __init__(self, nsources: int, K: int, slots: int, open_level: int, close_level: int, hang: int = 0, park: int = 0,
                 mask=None):
        self.lib = capi.load()
        self.nsources, self.K, self.slots = int(nsources), int(K), int(slots)
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, dtype=np.uint8)
            if m.shape != (self.K,):
                raise ValueError(f"mask: one entry per bin: {self.K}, not {m.shape}")
        cfg = RtlfmSlotsCfg(int(open_level), int(close_level), int(hang), int(park), m.ctypes.data if m is not None else None)
        a = C.c_void_p()
        check(self.lib.rtlfm_slots_create(self.nsources, self.K, self.slots, C.byref(cfg), C.byref(a)), "rtlfm_slots_create")
        self._a = a

    def close(self):
        if getattr(self, "_a", None):
            self.lib.rtlfm_slots_destroy(self._a)
            self._a = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step(self, power, frames):
        """One run's survey: ``power`` uint64 [nsources, K], ``frames`` int32 [nsources]."""
        p = np.ascontiguousarray(power, dtype=np.uint64)
        f = np.ascontiguousarray(frames, dtype=np.int32)
        if p.shape != (self.nsources, self.K) or f.shape != (self.nsources,):
            raise ValueError(f"power [{self.nsources}, {self.K}] and frames [{self.nsources}], not {p.shape} and {f.shape}")
        check(self.lib.rtlfm_slots_step(self._a, p.ctypes.data, f.ctypes.data), "rtlfm_slots_step")

    def bins(self) -> np.ndarray:
        """int32 [nsources, slots]: idle slots carry ``park``."""
        out = np.zeros((self.nsources, self.slots), dtype=np.int32)
        check(self.lib.rtlfm_slots_bins(self._a, out.ctypes.data), "rtlfm_slots_bins")
        return out

    def idle(self) -> np.ndarray:
        """bool [nsources, slots]."""
        out = np.zeros((self.nsources, self.slots), dtype=np.uint8)
        check(self.lib.rtlfm_slots_idle(self._a, out.ctypes.data), "rtlfm_slots_idle")
        return out.astype(bool)

    def events(self) -> list[dict]:
        """The changes of the last step (the fields of ``rtlfm_slots_event``; an idle slot is bin -1)."""
        cap = self.nsources * self.slots
        ev = (RtlfmSlotsEvent * cap)()
        n = C.c_int()
        check(self.lib.rtlfm_slots_events(self._a, ev, cap, C.byref(n)), "rtlfm_slots_events")
        return [ev[i].as_dict() for i in range(n.value)]
