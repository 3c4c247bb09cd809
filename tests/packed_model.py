"""Packed results in numpy (include/rtlfm_hip.h, rtlfm_gpu_fetch_packed), for tests/test_packed_*.py.

The index: every row's length rounded up to 8 int16, the exclusive prefix sum of those over the streams, and zeros
between a row's last sample and the next row's start.  The rule: the demod thread's (demod_thread_fn,
src/rtl_fm.c:1366-1370) on the counter full_demod() keeps (:1206-1213), walked over a run's levels from the counter the
run started with - clamped in a LOCAL copy only, as the pack does; the carried counter is whatever the caller carries.
"""
import numpy as np

PACKED_ROW = [("offset", "<u8"), ("len", "<i4"), ("held", "<i4")]


def round8(n: int) -> int:
    return (int(n) + 7) & ~7


def index_of(lens, held=None):
    """(index [streams] of PACKED_ROW, total int16) for rows of these lengths (a negative length counts as 0)."""
    lens = np.maximum(np.asarray(lens, dtype=np.int64), 0)
    padded = (lens + 7) & ~7
    idx = np.zeros(lens.size, dtype=PACKED_ROW)
    idx["offset"] = np.concatenate(([0], np.cumsum(padded)[:-1])) if lens.size else []
    idx["len"] = lens
    idx["held"] = 0 if held is None else held
    return idx, int(padded.sum())


def pack(rows, held=None):
    """(packed int16 [total], index) of the rows (a list of int16 arrays), in order."""
    idx, total = index_of([len(r) for r in rows], held)
    out = np.zeros(total, dtype=np.int16)
    for r, rec in zip(rows, idx):
        out[int(rec["offset"]):int(rec["offset"]) + len(r)] = r
    return out, idx


def unpack(packed, index):
    return [packed[int(r["offset"]):int(r["offset"]) + int(r["len"])] for r in index]


def rule(levels, level: int, conseq: int, hits: int):
    """One stream, one run: (emit flags, the counter behind the run as full_demod() alone leaves it - never clamped).
    The decisions come from a local copy that is clamped to conseq + 1 whenever a buffer is held."""
    emit = np.zeros(len(levels), dtype=bool)
    local = carried = int(hits)
    for b, sr in enumerate(levels):
        if sr >= 0:
            local = local + 1 if sr < level else 0       # :1206-1213
            carried = carried + 1 if sr < level else 0
        if local > conseq:                                 # :1366
            local = conseq + 1                             # :1368
        else:
            emit[b] = True
    return emit, carried


def extents(nblocks: int, N: int, D: int, p0: int, mul: int = 1):
    """begin [nblocks + 1] of the buffers of a run in a stream's row: N input samples per buffer through a boxcar of D that
    starts the run at phase p0 (D == 1: N outputs per buffer); mul = 2 for -M raw's I, Q pairs."""
    if D <= 1:
        p0 = 0
    return np.array([mul * ((p0 + b * N) // D) for b in range(nblocks + 1)], dtype=np.int64)


def gated(row, emit, begin):
    """The emitted buffers' parts of the row, in order."""
    parts = [row[begin[b]:begin[b + 1]] for b in range(len(emit)) if emit[b]]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int16)


class Gate:
    """The rule over consecutive runs of many streams, on rows and levels a handle WITHOUT the option returned: per run the
    gated rows and the held counts.  p0 of a run = the boxcar phase its rows started at, carried here from the extents."""

    def __init__(self, streams: int, N: int, D: int, mul: int, level: int, conseq: int, hits: int = 11):
        self.N, self.D, self.mul, self.level, self.conseq = N, D, mul, level, conseq
        self.hits = [hits] * streams  # demod_init(): squelch_hits = 11 (src/rtl_fm.c:1615), silence until it first opens
        self.p0 = [0] * streams

    def run(self, rows, levels):
        out, held = [], []
        for s, row in enumerate(rows):
            nb = len(levels[s])
            emit, self.hits[s] = rule(levels[s], self.level, self.conseq, self.hits[s])
            begin = extents(nb, self.N, self.D, self.p0[s], self.mul)
            assert begin[-1] == len(row), (s, begin[-1], len(row))
            if self.D > 1:
                self.p0[s] = (self.p0[s] + nb * self.N) % self.D
            out.append(gated(row, emit, begin))
            held.append(int((~emit).sum()))
        return out, held
