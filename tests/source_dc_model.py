"""Option source_dc in Python integers (include/rtlfm_hip.h, "source_dc"): the raw DC block per source in front of the
channel front ends.

  averages   per source a and buffer b of L bytes:  mI = trunc(sum(I - 127) / (L / 2)),
             aI[b] = trunc((mI + aI[b-1] k) / (k + 1)),  aI[-1] = clamp(dc_avgI of the source's channel 0, -128, 128)
  x, y       I - 127 - aI[b],  Q - 127 - aQ[b]  for every sample of buffer b
  record     every channel of the source carries a[nblocks - 1]

Everything behind x, y is the existing models' arithmetic, imported: channel_model's table and phase, channel_fir_model's
fir_decimate, channel_bank_model's polyphase_sums and fix_fft_rows.  Those models carry the history as bytes; here it is
carried as x, y - what the samples were consumed with."""
import numpy as np

import channel_model as cm
from channel_bank_model import fix_fft_rows, polyphase_sums
from channel_fir_model import fir_decimate, raw_rows, sat16  # noqa: F401  (raw_rows: for the callers)

HIST = 4096
M32 = cm.M32


def trunc_div(n: int, d: int) -> int:
    """C's division."""
    q = abs(n) // abs(d)
    return q if (n < 0) == (d < 0) else -q


def clamp(v: int, lo: int, hi: int) -> int:
    return lo if v < lo else hi if v > hi else v


def averages(row_u8, L: int, k: int, carried):
    """One source's buffers of L bytes: [(aI, aQ)] per buffer, from carried = (dc_avgI, dc_avgQ) as the record holds them."""
    row = np.asarray(row_u8, dtype=np.uint8)
    assert row.size % L == 0 and L % 512 == 0
    a = [clamp(int(carried[0]), -128, 128), clamp(int(carried[1]), -128, 128)]
    out = []
    for b in range(row.size // L):
        buf = row[b * L:(b + 1) * L].astype(np.int64) - 127
        for comp in (0, 1):
            m = trunc_div(int(buf[comp::2].sum()), L // 2)
            a[comp] = trunc_div(m + a[comp] * k, k + 1)
        out.append((a[0], a[1]))
    return out


def mix_xy(x, y, steps, per_source: int, pos: int):
    """channel_model.mix() on x, y int64 [sources, n] instead of bytes: (I', Q') int64 [sources * per_source, n]."""
    n = x.shape[1]
    tab = cm._tab()
    at = (np.uint64(pos & M32) + np.arange(n, dtype=np.uint64)) & np.uint64(M32)
    oi = np.empty((len(steps), n), dtype=np.int64)
    oq = np.empty((len(steps), n), dtype=np.int64)
    for s, step in enumerate(steps):
        ph = (at * np.uint64(int(step))) & np.uint64(M32)
        idx = (ph >> np.uint64(22)).astype(np.int64)
        c, sn = tab[idx, 0], tab[idx, 1]
        xs, ys = x[s // per_source], y[s // per_source]
        oi[s] = (xs * c + ys * sn + 8192) >> 14
        oq[s] = (ys * c - xs * sn + 8192) >> 14
    return oi, oq


def boxcar(oi, oq, D: int, state):
    """channel_model.model_raw_boxcar's low_pass() on mixed samples: (rows, state)."""
    S, T = oi.shape
    rows, after = [], []
    for s in range(S):
        p0 = state[s]["prev_index"]
        E = (p0 + T) // D
        ends = (np.arange(E, dtype=np.int64) + 1) * D - p0
        row = np.empty(2 * E, dtype=np.int16)
        new = dict(prev_index=p0 + T - E * D)
        for half, (v, carried) in enumerate(((oi[s], "now_r"), (oq[s], "now_j"))):
            P = np.concatenate(([0], np.cumsum(v))) + state[s][carried]
            sums = np.diff(np.concatenate(([0], P[ends])))
            row[half::2] = (sums & 0xffff).astype(np.uint16).view(np.int16)
            new[carried] = cm._i32(int(P[T] - (P[ends[-1]] if E else 0)))
        rows.append(row)
        after.append(new)
    return rows, after


class SourceDc:
    """What the option carries: every stream's (dc_avgI, dc_avgQ), and the source history as x, y."""

    def __init__(self, nsrc, per_source, k=9):
        self.nsrc, self.per, self.k = nsrc, per_source, int(k)
        self.S = nsrc * per_source
        self.rec = [[0, 0] for _ in range(self.S)]
        self.pos = 0
        self.L = None  # the buffer length of runs that do not name theirs
        self.clear()

    def clear(self):
        """Every clearing call: x = y = 0 in front of the next run."""
        self.hx = np.zeros((self.nsrc, HIST), dtype=np.int64)
        self.hy = np.zeros((self.nsrc, HIST), dtype=np.int64)

    def seek(self, pos):
        self.pos = int(pos)
        self.clear()

    def front(self, src_u8, L=None):
        """x, y int64 [sources, T] of a run of buffers of L bytes; the records move on."""
        src = np.asarray(src_u8, dtype=np.uint8)
        L = L or self.L
        T = src.shape[1] // 2
        x = src[:, 0::2].astype(np.int64) - 127
        y = src[:, 1::2].astype(np.int64) - 127
        self.last_avgs = []
        for a in range(self.nsrc):
            av = averages(src[a], L, self.k, self.rec[a * self.per])
            self.last_avgs.append(av)
            for b, (ai, aq) in enumerate(av):
                x[a, b * (L // 2):(b + 1) * (L // 2)] -= ai
                y[a, b * (L // 2):(b + 1) * (L // 2)] -= aq
            for c in range(self.per):
                self.rec[a * self.per + c] = [av[-1][0], av[-1][1]]
        assert np.abs(x).max() <= 256 and np.abs(y).max() <= 256 and x.shape[1] == T
        return x, y

    def push(self, x, y):
        self.hx = np.concatenate((self.hx, x), axis=1)[:, -HIST:].copy()  # (a run shorter than the history shifts it)
        self.hy = np.concatenate((self.hy, y), axis=1)[:, -HIST:].copy()
        self.pos += x.shape[1]


class DcBoxModel(SourceDc):
    """The mixers and the boxcar: -M raw rows (run), or the mixed samples as bytes for the oracle (mixed_bytes)."""

    def __init__(self, steps, per_source, D, nsrc, k=9):
        super().__init__(nsrc, per_source, k)
        self.steps, self.D = [int(v) for v in steps], int(D)
        self.state = [dict(now_r=0, now_j=0, prev_index=0) for _ in range(self.S)]

    def mixed(self, src_u8, L=None):
        x, y = self.front(src_u8, L)
        oi, oq = mix_xy(x, y, self.steps, self.per, self.pos)
        assert np.abs(oi).max() <= 362 and np.abs(oq).max() <= 362
        self.pos += x.shape[1]
        return oi, oq

    def run(self, src_u8, L=None):
        oi, oq = self.mixed(src_u8, L)
        rows, self.state = boxcar(oi, oq, self.D, self.state)
        return rows

    def mixed_bytes(self, src_u8, L=None):
        """As channel_model.mixed_bytes: asserted to fit a byte, never clipped."""
        oi, oq = self.mixed(src_u8, L)
        assert oi.min() >= -127 and oi.max() <= 128 and oq.min() >= -127 and oq.max() <= 128, "mixed samples do not fit a byte"
        by = np.empty((oi.shape[0], 2 * oi.shape[1]), dtype=np.uint8)
        by[:, 0::2] = (oi + 127).astype(np.uint8)
        by[:, 1::2] = (oq + 127).astype(np.uint8)
        return by


class DcFirModel(SourceDc):
    def __init__(self, steps, per_source, D, taps, shift, nsrc, k=9):
        super().__init__(nsrc, per_source, k)
        self.steps, self.D = [int(v) for v in steps], int(D)
        self.taps, self.shift = np.asarray(taps, dtype=np.int64), int(shift)
        self.p0 = [0] * self.S

    def run(self, src_u8, L=None):
        """(I, Q): per stream int64 arrays of the run's outputs."""
        x, y = self.front(src_u8, L)
        bx, by = np.concatenate((self.hx, x), axis=1), np.concatenate((self.hy, y), axis=1)
        oi, oq = mix_xy(bx, by, self.steps, self.per, (self.pos - HIST) & M32)
        I, Q = [], []
        for s in range(self.S):
            a, p1 = fir_decimate(oi[s, HIST:], oi[s, :HIST], self.taps, self.shift, self.D, self.p0[s])
            b, _ = fir_decimate(oq[s, HIST:], oq[s, :HIST], self.taps, self.shift, self.D, self.p0[s])
            I.append(a)
            Q.append(b)
            self.p0[s] = p1
        self.push(x, y)
        return I, Q


class DcBankModel(SourceDc):
    def __init__(self, K, taps, shift, D, nsrc, bins=None, k=9):
        self.K, self.m = int(K), int(K).bit_length() - 1
        self.bins = list(range(self.K)) if bins is None else [int(b) for b in bins]
        super().__init__(nsrc, len(self.bins), k)
        self.taps, self.shift, self.D = np.asarray(taps, dtype=np.int64), int(shift), int(D)
        self.p0 = [0] * self.S

    def frames(self, src_u8, L=None):
        """(Y_i, Y_q) per source, each int64 [E, K] - and the state moves on."""
        x, y = self.front(src_u8, L)
        T = x.shape[1]
        bx, by = np.concatenate((self.hx, x), axis=1), np.concatenate((self.hy, y), axis=1)
        rnd = (1 << (self.shift - 1)) if self.shift else 0
        out = []
        for a in range(self.nsrc):
            p0 = self.p0[a * self.per]
            E = (p0 + T) // self.D
            e = (np.arange(E, dtype=np.int64) + 1) * self.D - p0 - 1
            v = []
            for comp in (bx[a], by[a]):
                u = polyphase_sums(comp, e, self.pos & M32, self.taps, self.K)
                assert np.abs(u).max(initial=0) + rnd <= (1 << 31) - 1, "an int32 sum would overflow: rtlfm_channel_bank_check_dc"
                v.append(sat16((u + rnd) >> self.shift))
            out.append(fix_fft_rows(v[0], v[1], self.m))
            for c in range(self.per):
                self.p0[a * self.per + c] = p0 + T - E * self.D
        self.push(x, y)
        return out

    def run(self, src_u8, L=None, survey=False):
        """(I, Q) per stream; survey: also (power uint64 [sources, K], frames int32 [sources])."""
        I, Q, power, count = [], [], [], []
        for yi, yq in self.frames(src_u8, L):
            for b in self.bins:
                I.append(yi[:, b].copy())
                Q.append(yq[:, b].copy())
            power.append((yi * yi + yq * yq).sum(axis=0).astype(np.uint64))
            count.append(yi.shape[0])
        if survey:
            return I, Q, np.stack(power), np.asarray(count, dtype=np.int32)
        return I, Q
