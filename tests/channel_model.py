"""The channelizer's arithmetic in numpy, integers only (include/rtlfm_hip.h, rtlfm_gpu_set_channels):

  table    c[i] = lround(16384 cos(2 pi i / 1024)), s[i] = lround(16384 sin(2 pi i / 1024)), in double
  step     round_half_up(shift_hz 2^32 / capture_rate) modulo 2^32, in Python's big integers
  phase    (uint32)((pos + n) step), index = phase >> 22
  mixer    x = I - 127, y = Q - 127:  I' = (x c + y s + 8192) >> 14,  Q' = (y c - x s + 8192) >> 14

Stream s is channel s % per_source of source s // per_source.  The chain BEHIND the mixer is not restated here:
model_via_oracle hands the mixed samples, as bytes, to the existing oracle with offset_tuning = 1.  Only for full-scale
inputs, whose mixed samples do not fit a byte, model_raw_boxcar adds low_pass() (src/rtl_fm.c:461-481) for -M raw.
"""
import math

import numpy as np

from rtlsdr_amd.capi import RtlfmCfg

TABLE_SIZE = 1024
M32 = (1 << 32) - 1


def _lround(v: float) -> int:
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def table() -> np.ndarray:
    """int16 [1024, 2] = (cos, sin), Q14."""
    out = np.zeros((TABLE_SIZE, 2), dtype=np.int16)
    for i in range(TABLE_SIZE):
        a = 2.0 * math.pi * float(i) / float(TABLE_SIZE)
        out[i, 0] = _lround(16384.0 * math.cos(a))
        out[i, 1] = _lround(16384.0 * math.sin(a))
    return out


_TABLE = None


def _tab():
    global _TABLE
    if _TABLE is None:
        _TABLE = table().astype(np.int64)
    return _TABLE


def step_from_hz(shift_hz: int, capture_rate: int) -> int:
    if capture_rate == 0:
        return 0
    return ((2 * int(shift_hz) * (1 << 32) + int(capture_rate)) // (2 * int(capture_rate))) & M32


def mix(src_u8, steps, per_source: int, pos: int):
    """src_u8: uint8 [sources, 2 n] interleaved I, Q.  Returns (I', Q') int64 [sources * per_source, n]."""
    src = np.asarray(src_u8, dtype=np.uint8)
    nsrc, n = src.shape[0], src.shape[1] // 2
    steps = [int(v) for v in steps]
    assert len(steps) == nsrc * per_source
    x = src[:, 0::2].astype(np.int64) - 127
    y = src[:, 1::2].astype(np.int64) - 127
    tab = _tab()
    at = (np.uint64(pos & M32) + np.arange(n, dtype=np.uint64)) & np.uint64(M32)
    oi = np.empty((len(steps), n), dtype=np.int64)
    oq = np.empty((len(steps), n), dtype=np.int64)
    for s, step in enumerate(steps):
        ph = (at * np.uint64(step)) & np.uint64(M32)
        idx = (ph >> np.uint64(22)).astype(np.int64)
        c, sn = tab[idx, 0], tab[idx, 1]
        xs, ys = x[s // per_source], y[s // per_source]
        oi[s] = (xs * c + ys * sn + 8192) >> 14
        oq[s] = (ys * c - xs * sn + 8192) >> 14
    return oi, oq


def copy_cfg(cfg: RtlfmCfg, **ov) -> RtlfmCfg:
    c = RtlfmCfg.from_buffer_copy(bytes(cfg))
    for k, v in ov.items():
        setattr(c, k, v)
    return c


def mixed_bytes(src_u8, steps, per_source: int, pos: int) -> np.ndarray:
    """Every stream's mixed samples as the bytes a dongle tuned to that channel would have delivered: uint8
    [streams, 2 n].  The inputs must keep the mixed samples inside a byte: that is asserted, never clipped."""
    oi, oq = mix(src_u8, steps, per_source, pos)
    assert oi.min() >= -127 and oi.max() <= 128 and oq.min() >= -127 and oq.max() <= 128, "mixed samples do not fit a byte"
    by = np.empty((oi.shape[0], 2 * oi.shape[1]), dtype=np.uint8)
    by[:, 0::2] = (oi + 127).astype(np.uint8)
    by[:, 1::2] = (oq + 127).astype(np.uint8)
    return by


def model_via_oracle(cfg: RtlfmCfg, src_u8, steps, per_source: int, pos: int, states=None):
    """The mixed samples of every stream through the existing oracle with offset_tuning = 1.
    Returns pyoracle.run_batch's (out, out_len, states); `states` (as it returns them) carries on from an earlier call."""
    from oracle import pyoracle as po
    return po.run_batch(copy_cfg(cfg, offset_tuning=1), mixed_bytes(src_u8, steps, per_source, pos), states, nthreads=4)


def model_levels(cfg: RtlfmCfg, src_u8, steps, per_source: int, pos: int) -> np.ndarray:
    """rms() of the decimated IQ of every buffer (what the squelch compares, src/rtl_fm.c:1204-1237), int32
    [streams, buffers], from demod_init()'s state: the oracle's rms() on what it leaves in -M raw for the mixed bytes."""
    import ctypes as C

    from oracle import pyoracle as po
    lib = po.oracle()
    lib.orc_rms.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.orc_rms.restype = C.c_int
    by = mixed_bytes(src_u8, steps, per_source, pos)
    L = int(cfg.block_len)
    raw = copy_cfg(cfg, offset_tuning=1, mode=4, squelch_level=0, report_levels=0, max_blocks=1)
    out = np.zeros((by.shape[0], by.shape[1] // L), dtype=np.int32)
    scratch = np.zeros(2 * L + 64, dtype=np.int16)
    for s in range(by.shape[0]):
        st = po.new_states(1)[0]
        for b in range(out.shape[1]):
            k = lib.orc_block(C.byref(raw), C.byref(st), np.ascontiguousarray(by[s, b * L:(b + 1) * L]), L, scratch)
            out[s, b] = lib.orc_rms(scratch.ctypes.data, k, 1, 0)
    return out


def _i32(v: int) -> int:
    v &= M32
    return v - (1 << 32) if v >= (1 << 31) else v


def model_raw_boxcar(src_u8, steps, D: int, state=None, per_source: int = 1, pos: int = 0):
    """Mixer + low_pass() with its int16 stores, for -M raw on full-scale inputs.  state: per stream a dict with now_r,
    now_j, prev_index (None: zeros).  Returns (rows, state): rows[s] = int16 [2 outputs] interleaved I, Q."""
    oi, oq = mix(src_u8, steps, per_source, pos)
    S, T = oi.shape
    if state is None:
        state = [dict(now_r=0, now_j=0, prev_index=0) for _ in range(S)]
    rows, after = [], []
    for s in range(S):
        p0 = state[s]["prev_index"]
        E = (p0 + T) // D
        ends = (np.arange(E, dtype=np.int64) + 1) * D - p0  # output k ends behind run sample ends[k] - 1
        row = np.empty(2 * E, dtype=np.int16)
        new = dict(prev_index=p0 + T - E * D)
        for half, (v, carried) in enumerate(((oi[s], "now_r"), (oq[s], "now_j"))):
            P = np.concatenate(([0], np.cumsum(v))) + state[s][carried]  # int64: no wrap before the stores below
            sums = np.diff(np.concatenate(([0], P[ends])))
            row[half::2] = (sums & 0xffff).astype(np.uint16).view(np.int16)
            new[carried] = _i32(int(P[T] - (P[ends[-1]] if E else 0)))
        rows.append(row)
        after.append(new)
    return rows, after
