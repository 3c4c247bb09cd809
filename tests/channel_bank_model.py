"""The channel bank's arithmetic, integers only (include/rtlfm_hip.h, rtlfm_gpu_set_channel_bank):

  x[n]     (I - 127, Q - 127) of the source, n = pos + the index within the run; x = 0 before the last clear
  outputs  at the samples e at which low_pass() emits one for the source's channel 0: e = (k + 1) D - prev_index - 1
  sums     u_r = sum over j < ntaps with (e - j) mod K == r of taps[j] x[e - j], in numpy int64;
           v_r = sat16((u_r + rnd) >> shift), rnd = shift ? 1 << (shift - 1) : 0
  Y        = fix_fft(v): the oracle's orcp_fix_fft with orcp_sine_table(m) (oracle/rtlpower_oracle.c), N_WAVE = K
  channel c of a source is Y[bins[c]]

BankModel carries what the handle carries: every source's last 4096 samples as bytes, pos, every stream's prev_index.
The chain BEHIND the bank is the existing oracle's, as for the channel filter: channel_fir_model.via_oracle / raw_rows /
levels_of take the (I, Q) that run() returns.
"""
import ctypes as C

import numpy as np

from channel_fir_model import levels_of, raw_rows, sat16, via_oracle  # noqa: F401  (the back half, shared)

MAX_TAPS = 4096
HIST = 4096
M32 = (1 << 32) - 1


def polyphase_sums(x, e, pos, taps, K):
    """x: int64 [HIST + T] one component, the history in front of the run; e: int64 [E] run samples the frames are due at.
    Returns int64 [E, K]: u_r of every frame."""
    taps = np.asarray(taps, dtype=np.int64)
    nt = taps.size
    Q = (nt + K - 1) // K
    tp = np.zeros(Q * K, dtype=np.int64)
    tp[:nt] = taps
    xp = np.concatenate((np.zeros(Q * K, dtype=np.int64), x))  # (zeros where only zero taps reach)
    off = Q * K + HIST
    u = np.zeros((e.size, K), dtype=np.int64)
    j = np.arange(Q * K, dtype=np.int64)
    for k0 in range(0, e.size, 512):
        ee = e[k0:k0 + 512]
        win = xp[off + ee[:, None] - j[None, :]]                     # win[k, j] = x[e_k - j]
        branch = (win * tp[None, :]).reshape(ee.size, Q, K).sum(axis=1)  # branch[k, b] = sum_q taps[b + q K] x[e_k - b - q K]
        r = ((pos + ee[:, None] - np.arange(K, dtype=np.int64)[None, :]) & M32) % K  # the residue branch b meets at frame k
        np.put_along_axis(u[k0:k0 + 512], r, branch, axis=1)
    return u


_sine = {}


def fix_fft_rows(v_i, v_q, m):
    """v_i, v_q: int64 [E, K] (int16 values).  The oracle's fix_fft of every row: (Y_i, Y_q) int64 [E, K]."""
    from oracle import pyoracle as po
    lib = po._power_lib()
    if m not in _sine:
        _sine[m] = lib.orcp_sine_table(m)
    K = 1 << m
    buf = np.empty((v_i.shape[0], 2 * K), dtype=np.int16)
    buf[:, 0::2], buf[:, 1::2] = v_i, v_q
    for k in range(buf.shape[0]):
        assert lib.orcp_fix_fft(buf[k].ctypes.data, m, _sine[m], m) == 0
    return buf[:, 0::2].astype(np.int64), buf[:, 1::2].astype(np.int64)


class BankModel:
    """Runs of source bytes through the bank, the history carried as the handle carries it."""

    def __init__(self, K, taps, shift, D, nsrc, bins=None):
        self.K, self.m = int(K), int(K).bit_length() - 1
        assert 1 << self.m == self.K
        self.taps, self.shift, self.D = np.asarray(taps, dtype=np.int64), int(shift), int(D)
        self.bins = list(range(self.K)) if bins is None else [int(b) for b in bins]
        self.per, self.nsrc = len(self.bins), nsrc
        self.S = nsrc * self.per
        self.p0 = [0] * self.S
        self.pos = 0
        self.clear()

    def clear(self):
        """What set_channel_bank, set_channels, reset and channels_seek do to the history: bytes 127."""
        self.hist = np.full((self.nsrc, 2 * HIST), 127, dtype=np.uint8)

    def seek(self, pos):
        self.pos = int(pos)
        self.clear()

    def frames(self, src_u8):
        """(v_i, v_q, Y_i, Y_q) per source, each int64 [E, K] - and the state moves on."""
        src = np.asarray(src_u8, dtype=np.uint8)
        T = src.shape[1] // 2
        both = np.concatenate((self.hist, src), axis=1).astype(np.int64) - 127
        rnd = (1 << (self.shift - 1)) if self.shift else 0
        out = []
        for a in range(self.nsrc):
            p0 = self.p0[a * self.per]  # one schedule per source: channel 0's
            E = (p0 + T) // self.D
            e = (np.arange(E, dtype=np.int64) + 1) * self.D - p0 - 1
            v = []
            for comp in (0, 1):
                u = polyphase_sums(both[a, comp::2], e, self.pos & M32, self.taps, self.K)
                assert np.abs(u).max(initial=0) + rnd <= (1 << 31) - 1, "an int32 sum would overflow: rtlfm_channel_bank_check"
                v.append(sat16((u + rnd) >> self.shift))
            yi, yq = fix_fft_rows(v[0], v[1], self.m)
            out.append((v[0], v[1], yi, yq))
            for c in range(self.per):
                self.p0[a * self.per + c] = p0 + T - E * self.D
        self.hist = np.concatenate((self.hist, src), axis=1)[:, -2 * HIST:].copy()  # (a run shorter than the history shifts it)
        self.pos += T
        return out

    def run(self, src_u8):
        """src_u8: uint8 [sources, 2 T].  Returns (I, Q): per stream int64 arrays of the run's outputs."""
        I, Q = [], []
        for _, _, yi, yq in self.frames(src_u8):
            for b in self.bins:
                I.append(yi[:, b].copy())
                Q.append(yq[:, b].copy())
        return I, Q
