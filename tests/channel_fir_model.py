"""The channel filter's arithmetic in numpy, integers only (include/rtlfm_hip.h, rtlfm_gpu_set_channel_filter):

  m[n]     channel_model.mix() of the source bytes, n counted from where the history was last cleared; m[n < 0] = 0
  outputs  at the samples e at which low_pass() emits one: e = (k + 1) D - prev_index - 1 of the run
  value    sat16((sum_j taps[j] m[e - j] + r) >> shift), r = shift ? 1 << (shift - 1) : 0, summed in int64

FirModel carries what the handle carries: every source's bytes since the last clear (the handle keeps the last 1023 of
them; the model keeps all it needs), pos, and every stream's prev_index.  The chain BEHIND the filter is the existing
oracle's: via_oracle() hands the filtered samples, as bytes, to it with downsample = 1 and offset_tuning = 1 - the oracle's
own boxcar of length 1 passes them through, its rms(), squelch, demodulators and tails follow.
"""
import numpy as np

import channel_model as cm

MAX_TAPS = 1024


def sat16(v):
    return np.clip(v, -32768, 32767)


def fir_decimate(m, hist, taps, shift, D, p0):
    """m: int64 [T] mixed samples of a run, hist: int64 [>= ntaps - 1] the ones in front of it (oldest first).
    Returns (int64 outputs, new prev_index)."""
    taps = np.asarray(taps, dtype=np.int64)
    nt = taps.size
    T = m.size
    E = (p0 + T) // D
    x = np.concatenate((hist[hist.size - (nt - 1):] if nt > 1 else hist[:0], m))  # x[i] = sample i - (nt - 1) of the run
    e = (np.arange(E, dtype=np.int64) + 1) * D - p0 - 1
    r = (1 << (shift - 1)) if shift else 0
    out = np.empty(E, dtype=np.int64)
    rev = taps[::-1].copy()
    win = np.lib.stride_tricks.sliding_window_view(x, nt)  # win[i] = samples i - nt + 1 .. i of the run
    for k0 in range(0, E, 2048):  # (in pieces: the gathered windows are outputs x taps int64)
        out[k0:k0 + 2048] = win[e[k0:k0 + 2048]] @ rev
    assert np.abs(out).max(initial=0) + r <= (1 << 31) - 1, "the int32 sum would overflow: rtlfm_channel_filter_check"
    return sat16((out + r) >> shift), p0 + T - E * D


class FirModel:
    """Runs of source bytes through mixer and filter, the history carried as the handle carries it."""

    def __init__(self, steps, per_source, D, taps, shift, nsrc):
        self.steps, self.per, self.D = [int(v) for v in steps], per_source, D
        self.taps, self.shift = np.asarray(taps, dtype=np.int64), int(shift)
        self.nsrc = nsrc
        self.S = nsrc * per_source
        self.p0 = [0] * self.S
        self.pos = 0
        self.clear()

    def clear(self):
        """What set_channel_filter, set_channels, reset and channels_seek do to the history: bytes 127."""
        self.hist = np.full((self.nsrc, 2 * (MAX_TAPS - 1)), 127, dtype=np.uint8)

    def seek(self, pos):
        self.pos = int(pos)
        self.clear()

    def run(self, src_u8):
        """src_u8: uint8 [sources, 2 T].  Returns (I, Q): per stream int64 arrays of the run's outputs."""
        src = np.asarray(src_u8, dtype=np.uint8)
        H = self.hist.shape[1] // 2
        both = np.concatenate((self.hist, src), axis=1)
        oi, oq = cm.mix(both, self.steps, self.per, (self.pos - H) & cm.M32)
        I, Q = [], []
        for s in range(self.S):
            a, p1 = fir_decimate(oi[s, H:], oi[s, :H], self.taps, self.shift, self.D, self.p0[s])
            b, _ = fir_decimate(oq[s, H:], oq[s, :H], self.taps, self.shift, self.D, self.p0[s])
            I.append(a)
            Q.append(b)
            self.p0[s] = p1
        self.hist = both[:, both.shape[1] - 2 * H:].copy()  # (a run shorter than the history shifts it)
        self.pos += src.shape[1] // 2
        return I, Q


def raw_rows(I, Q):
    """-M raw: the filtered samples themselves, interleaved int16."""
    rows = []
    for a, b in zip(I, Q, strict=True):
        r = np.empty(2 * a.size, dtype=np.int16)
        r[0::2], r[1::2] = a, b
        rows.append(r)
    return rows


def filtered_bytes(I, Q):
    """A run's filtered samples as the bytes a dongle at the decimated rate would have delivered (asserted to fit)."""
    out = []
    for a, b in zip(I, Q, strict=True):
        assert a.size == 0 or (min(a.min(), b.min()) >= -127 and max(a.max(), b.max()) <= 128), "filtered samples do not fit a byte"
        by = np.empty(2 * a.size, dtype=np.uint8)
        by[0::2], by[1::2] = (a + 127).astype(np.uint8), (b + 127).astype(np.uint8)
        out.append(by)
    return out


def via_oracle(cfg, runs_IQ, nblocks_of_run, N0):
    """The back half by the existing oracle.  runs_IQ: per run the (I, Q) FirModel.run returned; the run had
    nblocks_of_run[r] buffers of N0 complex samples, and every buffer must have given the same number of outputs (N0 a
    multiple of D), because full_demod() works buffer by buffer: the oracle gets buffers of 2 N0 / D bytes at downsample 1.
    Returns (per stream PCM of all runs, oracle states)."""
    from oracle import pyoracle as po
    D = int(cfg.downsample)
    assert N0 % D == 0
    by_runs = [filtered_bytes(I, Q) for I, Q in runs_IQ]
    S = len(by_runs[0])
    rows = np.stack([np.concatenate([by_runs[r][s] for r in range(len(by_runs))]) for s in range(S)])
    assert rows.shape[1] == sum(nblocks_of_run) * 2 * N0 // D
    c = cm.copy_cfg(cfg, offset_tuning=1, downsample=1, block_len=2 * N0 // D, max_blocks=sum(nblocks_of_run))
    out, out_len, states = po.run_batch(c, rows, None, nthreads=4)
    return [out[s, :out_len[s]] for s in range(S)], states


def levels_of(I, Q, nblocks, per_block):
    """rms() of every buffer's decimated IQ as the squelch sees it (src/rtl_fm.c:1093-1110), int32 [streams, buffers]:
    the oracle's own rms() on the filtered samples."""
    import ctypes as C

    from oracle import pyoracle as po
    lib = po.oracle()
    lib.orc_rms.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.orc_rms.restype = C.c_int
    out = np.zeros((len(I), nblocks), dtype=np.int32)
    for s, row in enumerate(raw_rows(I, Q)):
        for blk in range(nblocks):
            v = np.ascontiguousarray(row[2 * blk * per_block:2 * (blk + 1) * per_block])
            out[s, blk] = lib.orc_rms(v.ctypes.data, v.size, 1, 0)
    return out
