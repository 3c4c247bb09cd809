"""The scanner's hop engine over the C ABI of ``include/rtlfm_scan.h``: what rtl_fm's controller thread does with several
``-f`` (src/rtl_fm.c:1495-1507), for N streams.

The engine is host code inside ``librtlfm_hip.so``; this class only marshals records into it.  It is fed with the squelch
gate's per-buffer records (``GpuDemod.gate``, taken on the GPU), either by hand (``feed``) or from a handle's last run
(``update``); ``apply`` hands the hop mutes to the handle.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import RtlfmScanEvent, check

DEFAULT_DUMP = 4096  # RTLFM_SCAN_DEFAULT_DUMP = DEFAULT_BUFFER_DUMP, src/rtl_fm.c:1507


def parse_list(text: str) -> list[int]:
    """``rtlfm_scan_parse_list``: single frequencies and a:b:step ranges with k / M / G suffixes."""
    lib = capi.load()
    n = C.c_int()
    r = lib.rtlfm_scan_parse_list(text.encode(), None, 0, C.byref(n))
    if r < 0 and r != -105:  # -ENOBUFS: the size
        check(r, "rtlfm_scan_parse_list")
    out = np.zeros(n.value, dtype=np.uint32)
    check(lib.rtlfm_scan_parse_list(text.encode(), out.ctypes.data, out.size, C.byref(n)), "rtlfm_scan_parse_list")
    return [int(v) for v in out]


class Scanner:
    """One frequency list per stream; events come out in the order the hops fell."""

    def __init__(self, nstreams: int, dump_bytes: int = DEFAULT_DUMP, settle: int = 0):
        self.lib = capi.load()
        self.nstreams = int(nstreams)
        a = C.c_void_p()
        check(self.lib.rtlfm_scan_create(self.nstreams, dump_bytes, settle, C.byref(a)), "rtlfm_scan_create")
        self._a = a

    def close(self):
        if getattr(self, "_a", None):
            self.lib.rtlfm_scan_destroy(self._a)
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

    def set_list(self, stream: int, freqs):
        """``freqs``: numbers, or a text in ``parse_list``'s grammar."""
        if isinstance(freqs, str):
            freqs = parse_list(freqs)
        f = np.ascontiguousarray(freqs, dtype=np.uint32)
        check(self.lib.rtlfm_scan_set_list(self._a, stream, f.ctypes.data, f.size), "rtlfm_scan_set_list")

    def feed(self, stream: int, records):
        """One run of ``stream``: its gate records (an array of ``capi.GATE_REC_DTYPE``) in order."""
        r = np.ascontiguousarray(records, dtype=capi.GATE_REC_DTYPE).ravel()
        check(self.lib.rtlfm_scan_feed(self._a, stream, r.ctypes.data, r.size), "rtlfm_scan_feed")

    def update(self, demod):
        """Feed every stream from the last run of a ``GpuDemod`` (needs ``squelch_gate``)."""
        check(self.lib.rtlfm_scan_update(self._a, demod._h), "rtlfm_scan_update")

    def apply(self, demod):
        """``demod.mute(stream, dump_bytes)`` for every stream that has hopped since the last call."""
        check(self.lib.rtlfm_scan_apply(self._a, demod._h), "rtlfm_scan_apply")

    def take_hopped(self) -> list[int]:
        """The streams that have hopped since the last call / ``apply`` (and forgets them)."""
        out = np.zeros(self.nstreams, dtype=np.int32)
        n = C.c_int()
        check(self.lib.rtlfm_scan_take_hopped(self._a, out.ctypes.data, out.size, C.byref(n)), "rtlfm_scan_take_hopped")
        return [int(v) for v in out[:n.value]]

    def events(self, cap: int = 1024) -> list[dict]:
        """Every hop so far, as dictionaries (the fields of ``rtlfm_scan_event``)."""
        out = []
        ev = (RtlfmScanEvent * cap)()
        n = C.c_int()
        while True:
            check(self.lib.rtlfm_scan_events(self._a, ev, cap, C.byref(n)), "rtlfm_scan_events")
            out += [ev[i].as_dict() for i in range(n.value)]
            if n.value < cap:
                return out

    def freq(self, stream: int) -> dict:
        f, i, h, b, d = C.c_uint32(), C.c_int32(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(self.lib.rtlfm_scan_freq(self._a, stream, C.byref(f), C.byref(i), C.byref(h), C.byref(b), C.byref(d)), "rtlfm_scan_freq")
        return {"freq": f.value, "index": i.value, "hops": h.value, "buffers": b.value, "held": d.value}
