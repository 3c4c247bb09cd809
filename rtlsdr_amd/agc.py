"""Input health over the C ABI of ``include/rtlfm_agc.h``: the reference's software AGC (gain mode 2, ``softagc``,
src/librtlsdr.c:3288-3327), rtl_tcp's overload report (src/rtl_tcp.c:235-244) and rtl_test's continuity check
(src/rtl_test.c:121-151) for N streams.

The engine is host code inside ``librtlfm_hip.so``; this class only marshals records into it.  It is fed with the
per-buffer records of the raw input (``GpuDemod.input_health``, taken on the GPU), either by hand (``feed``) or from a
handle's last run (``update``).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import RtlfmAgcEvent, check


class SoftAgc:
    """One gain table size per stream; events come out in the order the decisions fell."""

    def __init__(self, gain_counts, enable=None):
        self.lib = capi.load()
        gc = np.ascontiguousarray(gain_counts, dtype=np.int32)
        self.nstreams = int(gc.size)
        en = None if enable is None else np.ascontiguousarray(enable, dtype=np.int32)
        if en is not None and en.size != gc.size:
            raise ValueError("one enable flag per stream")
        a = C.c_void_p()
        check(self.lib.rtlfm_agc_create(self.nstreams, gc.ctypes.data, en.ctypes.data if en is not None else None, C.byref(a)),
              "rtlfm_agc_create")
        self._a = a

    def close(self):
        if getattr(self, "_a", None):
            self.lib.rtlfm_agc_destroy(self._a)
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

    def feed(self, stream: int, records, lens):
        """Consecutive buffers of ``stream``: records (an array of ``capi.INPUT_HEALTH_DTYPE``) and each buffer's own
        length in bytes (one number for all, or as many as records)."""
        r = np.ascontiguousarray(records, dtype=capi.INPUT_HEALTH_DTYPE).ravel()
        ln = np.ascontiguousarray(np.broadcast_to(np.asarray(lens, dtype=np.uint32), r.shape))
        check(self.lib.rtlfm_agc_feed(self._a, stream, r.ctypes.data, ln.ctypes.data, r.size), "rtlfm_agc_feed")

    def update(self, demod):
        """Feed every stream from the last run of a ``GpuDemod`` (needs ``set_option("input_health", 1)``).  A demod with
        channels on and the option ``source_health`` set feeds SOURCE i's records to input i instead: one input per wideband
        source (``nstreams // per_source``), ``ValueError`` otherwise."""
        per = getattr(demod, "_per_source", 0)
        if per and demod.get_option("source_health"):
            nsrc = demod.nstreams // per
            if self.nstreams != nsrc:
                raise ValueError(f"one input per source: the demod has {nsrc}, this engine {self.nstreams}")
            recs = demod.source_health_all()
            for i in range(nsrc):
                self.feed(i, recs[i], int(demod.cfg.block_len))
            return
        check(self.lib.rtlfm_agc_update(self._a, demod._h), "rtlfm_agc_update")

    def poll(self, cap: int = 1024) -> list[dict]:
        """Every index change so far, as dictionaries (the fields of ``rtlfm_agc_event``)."""
        out = []
        ev = (RtlfmAgcEvent * cap)()
        n = C.c_int()
        while True:
            check(self.lib.rtlfm_agc_poll(self._a, ev, cap, C.byref(n)), "rtlfm_agc_poll")
            out += [ev[i].as_dict() for i in range(n.value)]
            if n.value < cap:
                return out

    def state(self, stream: int) -> dict:
        idx, ov, tot, drop = C.c_int32(), C.c_int32(), C.c_uint64(), C.c_uint64()
        check(self.lib.rtlfm_agc_state(self._a, stream, C.byref(idx), C.byref(ov), C.byref(tot), C.byref(drop)), "rtlfm_agc_state")
        return {"index": idx.value, "overloaded": ov.value, "total_samples": tot.value, "dropped_samples": drop.value}

    def set_index(self, stream: int, index: int):
        check(self.lib.rtlfm_agc_set_index(self._a, stream, index), "rtlfm_agc_set_index")

    def set_settle(self, k: int):
        check(self.lib.rtlfm_agc_set_settle(self._a, k), "rtlfm_agc_set_settle")
