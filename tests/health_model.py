"""A restatement of the reference's three other passes over the raw bytes of a transfer, loop by loop:

  softagc()          src/librtlsdr.c:3288-3327   overload / high_level counts and the index step
  detect_overload()  src/rtl_tcp.c:235-244       8000 * overload_count >= len
  underrun_test()    src/rtl_test.c:121-151      the continuity counter with its two function statics

The reference's own functions are static and sit inside tools that link libusb: the loop model below is the definition
the product is held to.  A vectorised numpy twin sits beside each loop and is used for the large cases
(tests/test_health_model_cpu.py holds the twin to the loops).
"""
from __future__ import annotations

import numpy as np

HEALTH_DTYPE = [("overload", "<u4"), ("high", "<u4"), ("lost", "<u4"), ("first", "u1"), ("last", "u1"), ("pad_", "<u2")]


# ------------------------------------------------------------------ the loops ----

def softagc_counts_loop(buf) -> tuple[int, int]:
    """(overload, high_level) of softagc(), :3299-3306."""
    overload = high_level = 0
    for u in bytes(buf):
        if u == 0 or u == 255:  # 0 dBFS, :3302
            overload += 1
        if u < 64 or u > 191:   # -6 dBFS, :3304
            high_level += 1
    return overload, high_level


def detect_overload_loop(buf) -> bool:
    """src/rtl_tcp.c:235-244."""
    overload_count = 0
    for u in bytes(buf):
        if u == 0 or u == 255:
            overload_count += 1
    return 8000 * overload_count >= len(buf)


class Underrun:
    """underrun_test() with its statics `bcnt` and `uninit` (src/rtl_test.c:124) and the two globals it adds to."""

    def __init__(self):
        self.bcnt = 0
        self.uninit = True
        self.total_samples = 0
        self.dropped_samples = 0

    def call(self, buf) -> int:
        """One call on one buffer; returns its `lost`."""
        b = bytes(buf)
        lost = 0
        if self.uninit:          # :126-130
            self.bcnt = b[0]
            self.uninit = False
        for x in b:              # :131-142
            if self.bcnt != x:
                lost += x - self.bcnt if x > self.bcnt else self.bcnt - x
                self.bcnt = x
            self.bcnt = (self.bcnt + 1) & 0xFF  # uint8_t bcnt++
        self.total_samples += len(b)   # :144
        self.dropped_samples += lost   # :145
        return lost


def record_loop(buf) -> tuple:
    """The record of one buffer from the loops: `lost` is what underrun_test adds at positions 1 .. len-1, that is a
    call whose counter arrives matching buf[0] (the term at position 0 is the engine's)."""
    b = bytes(buf)
    u = Underrun()
    u.uninit = False
    u.bcnt = b[0]
    lost = u.call(b)
    ov, hi = softagc_counts_loop(b)
    return (ov, hi, lost, b[0], b[-1], 0)


# ------------------------------------------------------------------ the twin ----

def _records_rows(a: np.ndarray) -> np.ndarray:
    """uint8 [n, L] -> HEALTH_DTYPE [n], in uint8 arithmetic (wrapping is the reference's (uint8_t) cast)."""
    out = np.zeros(a.shape[0], dtype=HEALTH_DTYPE)
    one = np.uint8(1)
    for i, row in enumerate(a):  # a row at a time: the temporaries stay in cache
        out["overload"][i] = np.count_nonzero((row + one) < 2)                  # 0 and 255
        out["high"][i] = np.count_nonzero((row + np.uint8(64)) < 128)           # < 64 or > 191
        e = row[:-1] + one                                                      # what the counter expects at i = 1 .. len-1
        b = row[1:]
        out["lost"][i] = (np.maximum(b, e) - np.minimum(b, e)).sum(dtype=np.uint64)
        out["first"][i], out["last"][i] = row[0], row[-1]
    return out


def records(buffers) -> np.ndarray:
    """uint8 [..., L] -> HEALTH_DTYPE [...]: one record per buffer, vectorised (large inputs on a few threads)."""
    a = np.ascontiguousarray(buffers, dtype=np.uint8)
    rows = a.reshape(-1, a.shape[-1])
    if rows.size >= 1 << 24 and rows.shape[0] >= 8:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(8) as ex:
            parts = list(ex.map(_records_rows, np.array_split(rows, 8)))
        return np.concatenate(parts).reshape(a.shape[:-1])
    return _records_rows(rows).reshape(a.shape[:-1])


# ------------------------------------------------------------------ the engine ----

class StreamModel:
    """One stream of include/rtlfm_agc.h: continuity with the carried counter, detect_overload's verdict, softagc's
    step with the index moved at once, `settle` buffers without a decision after a change."""

    def __init__(self, stream: int, gain_count: int, enabled: bool = True, settle: int = 0):
        self.stream, self.gain_count, self.enabled, self.settle = stream, gain_count, enabled, settle
        self.index = 0          # mode 2 starts at 0, src/librtlsdr.c:1547
        self.hold = 0
        self.uninit, self.bcnt = True, 0
        self.overloaded = 0
        self.serial = 0
        self.total_samples = self.dropped_samples = 0
        self.events = []

    def feed(self, recs, lens):
        recs = np.asarray(recs, dtype=HEALTH_DTYPE).ravel()
        lens = np.broadcast_to(np.asarray(lens), recs.shape)
        for r, ln in zip(recs, lens):
            first, last, ln = int(r["first"]), int(r["last"]), int(ln)
            if self.uninit:
                self.bcnt, self.uninit = first, False
            lost = int(r["lost"]) + abs(first - self.bcnt)
            self.bcnt = (last + 1) & 0xFF
            self.total_samples += ln
            self.dropped_samples += lost
            self.overloaded = int(8000 * int(r["overload"]) >= ln)
            serial = self.serial
            self.serial += 1
            if not self.enabled:
                continue
            if self.hold > 0:
                self.hold -= 1
                continue
            new = self.index
            if self.overloaded:
                if self.index > 0:
                    new = self.index - 1
            elif 8000 * int(r["high"]) <= ln:
                if self.index < self.gain_count - 1:
                    new = self.index + 1
            if new != self.index:
                self.events.append({"stream": self.stream, "old_index": self.index, "new_index": new,
                                    "overloaded": self.overloaded, "buffer_serial": serial})
                self.index = new
                self.hold = self.settle

    def state(self) -> dict:
        return {"index": self.index, "overloaded": self.overloaded, "total_samples": self.total_samples,
                "dropped_samples": self.dropped_samples}


# ------------------------------------------------------------------ inputs ----

def counter(shape, start=0) -> np.ndarray:
    """A running byte counter along the last axis of every row (what rtl_test's test mode sends): nothing lost."""
    n = int(np.prod(shape[1:]))
    rows = [(np.arange(n, dtype=np.int64) + start + 7 * s) % 256 for s in range(shape[0])]
    return np.stack(rows).astype(np.uint8).reshape(shape)


def boundary_positions(L: int):
    """Byte positions whose predecessor belongs to another 16-byte unit, wave, workgroup stride or unrolled-by-eight
    stride of the kernel, and the first and last bytes."""
    return [p for p in (0, 1, 15, 16, 1023, 1024, 4095, 4096, 32767, 32768, L - 2, L - 1) if 0 <= p < L]


def plant_gaps(iq: np.ndarray, L: int) -> np.ndarray:
    """A discontinuity of +1, -1, +128 or 255 -> 1 at one of the boundary positions, another variant per (stream,
    buffer): from that byte to the end of the buffer the counter is shifted."""
    out = iq.copy()
    S, nb = out.shape[0], out.shape[1] // L
    pos = boundary_positions(L)
    k = 0
    for s in range(S):
        for b in range(nb):
            p = pos[k % len(pos)]
            kind = (k // len(pos)) % 4
            seg = out[s, b * L:(b + 1) * L]
            if kind == 3:
                if p > 0:
                    seg[p - 1] = 255
                seg[p] = 1
            else:
                seg[p:] = (seg[p:].astype(np.int32) + (1, -1, 128)[kind]) & 0xFF
            k += 1
    return out


def plant_values(iq: np.ndarray, L: int) -> np.ndarray:
    """The values 0, 255, 63, 64, 191, 192 singly at a boundary position, another variant per (stream, buffer)."""
    out = iq.copy()
    S, nb = out.shape[0], out.shape[1] // L
    pos = boundary_positions(L)
    vals = (0, 255, 63, 64, 191, 192)
    k = 0
    for s in range(S):
        for b in range(nb):
            out[s, b * L + pos[k % len(pos)]] = vals[(k // len(pos) + k) % len(vals)]
            k += 1
    return out
