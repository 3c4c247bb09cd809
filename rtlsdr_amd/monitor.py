"""The level monitor over the C ABI of ``include/rtlfm_monitor.h``: rtl_fm's command file (``-C``,
reference src/rtl_fm.c:527-736) for N streams, line i of the file watched permanently by stream i.

The engine is host code inside ``librtlfm_hip.so``; this class only marshals records into it.  It is fed
with the per-buffer ``rms()`` levels (``GpuDemod.levels``) and the per-buffer ADC statistics of the raw input
(``GpuDemod.input_stats``, taken on the GPU), either by hand (``feed``) or from a handle's last run (``update``).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import RtlfmMonitorEvent, RtlfmMonitorRule, RtlfmMonitorStat, check


def parse_file(path: str, cap: int = 65536):
    """``rtlfm_monitor_parse_file``: (rules, check_adc_max, check_adc_rms) of a command file."""
    lib = capi.load()
    rules = (RtlfmMonitorRule * cap)()
    n, amax, arms = C.c_int(), C.c_int(), C.c_int()
    check(lib.rtlfm_monitor_parse_file(str(path).encode(), rules, cap, C.byref(n), C.byref(amax), C.byref(arms)),
          "rtlfm_monitor_parse_file")
    return [RtlfmMonitorRule.from_buffer_copy(rules[i]) for i in range(n.value)], bool(amax.value), bool(arms.value)


class Monitor:
    """One rule per stream; events come out in the order their cycles ended."""

    def __init__(self, rules):
        self.lib = capi.load()
        self.nstreams = len(rules)
        arr = (RtlfmMonitorRule * self.nstreams)(*rules)
        m = C.c_void_p()
        check(self.lib.rtlfm_monitor_create(self.nstreams, arr, C.byref(m)), "rtlfm_monitor_create")
        self._m = m

    def close(self):
        if getattr(self, "_m", None):
            self.lib.rtlfm_monitor_destroy(self._m)
            self._m = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def feed(self, stream: int, rms, stats=None):
        """Consecutive buffers of ``stream``: int32 levels and, optionally, as many ADC records
        (an array of ``capi.INPUT_STAT_DTYPE``)."""
        r = np.ascontiguousarray(rms, dtype=np.int32)
        st = None
        if stats is not None:
            st = np.ascontiguousarray(stats, dtype=capi.INPUT_STAT_DTYPE)
            if st.size != r.size:
                raise ValueError("as many records as levels")
        check(self.lib.rtlfm_monitor_feed(self._m, stream, r.ctypes.data, st.ctypes.data if st is not None else None, r.size),
              "rtlfm_monitor_feed")

    def update(self, demod):
        """Feed every stream from the last run of a ``GpuDemod`` (needs report_levels or squelch_level)."""
        check(self.lib.rtlfm_monitor_update(self._m, demod._h), "rtlfm_monitor_update")

    def poll(self, cap: int = 1024) -> list[dict]:
        """Every finished event so far, as dictionaries (the fields of ``rtlfm_monitor_event``)."""
        out = []
        ev = (RtlfmMonitorEvent * cap)()
        n = C.c_int()
        while True:
            check(self.lib.rtlfm_monitor_poll(self._m, ev, cap, C.byref(n)), "rtlfm_monitor_poll")
            out += [ev[i].as_dict() for i in range(n.value)]
            if n.value < cap:
                return out

    def stats(self, stream: int) -> dict:
        """count / mean / min / max of the stream's cycle levels (what the reference prints at exit)."""
        st = RtlfmMonitorStat()
        check(self.lib.rtlfm_monitor_stats(self._m, stream, C.byref(st)), "rtlfm_monitor_stats")
        return {"count": st.count, "min": st.min_level, "max": st.max_level, "sum": st.sum_levels,
                "mean": st.sum_levels / st.count if st.count else None}

    def rule(self, stream: int) -> RtlfmMonitorRule:
        r = RtlfmMonitorRule()
        check(self.lib.rtlfm_monitor_rule_get(self._m, stream, C.byref(r)), "rtlfm_monitor_rule_get")
        return r

    def format_event(self, ev: dict) -> str:
        """The ``-v`` line of an event in the reference's wording."""
        e = RtlfmMonitorEvent(**ev)
        r = self.rule(ev["stream"])
        buf = C.create_string_buffer(512)
        check(self.lib.rtlfm_monitor_format_event(C.byref(r), C.byref(e), buf, 512), "rtlfm_monitor_format_event")
        return buf.value.decode()
