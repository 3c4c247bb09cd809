"""Option source_iq and the engine of include/rtlfm_iq.h, restated in Python integers and math.sqrt: what k_source_iq
leaves (``sums``, ``apply``), what rtlfm_iq_compute decides (``compute``) and what the engine does with windows of records
(``Engine``).  A plain module, like source_dc_model.py; the tests hold the C code and the kernel to it bit for bit.

The floating-point steps are one IEEE operation per line, in the order csrc/iq.cpp takes them (the build keeps
-ffp-contract=off), so the int16 coefficients are equal, not close."""
import math

import numpy as np

IDENTITY = (16384, 0, 0, 16384)
OK, WEAK, REJECTED = range(3)
CHANGED, REJECTED_EVENT = range(2)
SUMS_DTYPE = [("n", "<u4"), ("clipped", "<u4"), ("si", "<u8"), ("sq", "<u8"), ("sii", "<u8"), ("sqq", "<u8"), ("siq", "<u8")]


def apply(buf, coef):
    """uint8 [..., L] interleaved I Q and coef [4] or [..., 4] (one set per leading index) -> (corrected uint8 of the same
    shape, number of output bytes the clamp changed per leading index)."""
    a = np.ascontiguousarray(buf, dtype=np.uint8)
    c = np.asarray(coef, dtype=np.int64)
    c = np.broadcast_to(c, a.shape[:-1] + (4,))[..., None, :]
    x = a[..., 0::2].astype(np.int64) - 127
    y = a[..., 1::2].astype(np.int64) - 127
    i = ((c[..., 0] * x + c[..., 1] * y + 8192) >> 14) + 127
    q = ((c[..., 2] * x + c[..., 3] * y + 8192) >> 14) + 127
    out = np.empty(a.shape, dtype=np.int64)
    out[..., 0::2] = i
    out[..., 1::2] = q
    clamped = np.clip(out, 0, 255)
    return clamped.astype(np.uint8), (clamped != out).sum(axis=-1)


def sums(buf, coef=IDENTITY):
    """uint8 [..., L] -> records [...] of the RAW bytes; ``clipped`` is what ``apply`` with ``coef`` clamps."""
    a = np.ascontiguousarray(buf, dtype=np.uint8)
    i = a[..., 0::2].astype(np.uint64)
    q = a[..., 1::2].astype(np.uint64)
    out = np.zeros(a.shape[:-1], dtype=SUMS_DTYPE)
    out["n"] = a.shape[-1] // 2
    out["clipped"] = apply(a, coef)[1]
    out["si"] = i.sum(axis=-1)
    out["sq"] = q.sum(axis=-1)
    out["sii"] = (i * i).sum(axis=-1)
    out["sqq"] = (q * q).sum(axis=-1)
    out["siq"] = (i * q).sum(axis=-1)
    return out


def total_of(records):
    """The field-wise sum of records as a dict of Python ints."""
    r = np.asarray(records, dtype=SUMS_DTYPE).ravel()
    return {k: sum(int(v) for v in r[k]) for k, _ in SUMS_DTYPE}


def q14(v):
    return math.floor(v * 16384.0 + 0.5)


def compute(t, deadband=164, min_rms=2):
    """t: a dict (or record) with n, si, sq, sii, sqq, siq -> (verdict, coef or None, g_q14 or None, s_q14 or None)."""
    N, SI, SQ, SII, SQQ, SIQ = (int(t[k]) for k in ("n", "si", "sq", "sii", "sqq", "siq"))
    A = N * SII - SI * SI
    B = N * SQQ - SQ * SQ
    Cc = N * SIQ - SI * SQ
    floor_ = N * N * min_rms * min_rms
    if N == 0 or A <= 0 or B <= 0 or A < floor_ or B < floor_:
        return WEAK, None, None, None
    a_, b_, c_ = float(A), float(B), float(Cc)
    ratio = b_ / a_
    g = math.sqrt(ratio)
    ab = a_ * b_
    root = math.sqrt(ab)
    s = c_ / root
    gq = min(q14(g), 1 << 30)
    sq = q14(s)
    if g < 0.5 or g > 2.0 or abs(s) > 0.5:
        return REJECTED, None, gq, sq
    dg = abs(g - 1.0) * 16384.0
    ds = abs(s) * 16384.0
    if dg < float(deadband) and ds < float(deadband):
        return OK, IDENTITY, gq, sq
    ss = s * s
    one_ss = 1.0 - ss
    c = math.sqrt(one_ss)
    gc = g * c
    if gc >= 1.0:
        a = 1.0
        sc = s / c
        p = -sc
        q = 1.0 / gc
    else:
        a = gc
        sg = s * g
        p = -sg
        q = 1.0
    return OK, (q14(a), 0, q14(p), q14(q)), gq, sq


class Engine:
    def __init__(self, nsources, window=16, deadband=164, min_rms=2, min_step=8):
        self.window, self.deadband, self.min_rms, self.min_step = window, deadband, min_rms, min_step
        self.coef = [IDENTITY] * nsources
        self.tot = [dict.fromkeys([k for k, _ in SUMS_DTYPE], 0) for _ in range(nsources)]
        self.buffers = [0] * nsources
        self.serial = [0] * nsources
        self.events = []

    def feed(self, source, records):
        for r in np.asarray(records, dtype=SUMS_DTYPE).ravel():
            t = self.tot[source]
            for k, _ in SUMS_DTYPE:
                t[k] += int(r[k])
            self.buffers[source] += 1
            if self.buffers[source] < self.window:
                continue
            verdict, coef, g, s = compute(t, self.deadband, self.min_rms)
            self.tot[source] = dict.fromkeys(t, 0)
            self.buffers[source] = 0
            serial = self.serial[source]
            self.serial[source] += 1
            if verdict == WEAK:
                continue
            ev = {"source": source, "g_q14": g, "s_q14": s, "window_serial": serial}
            if verdict == REJECTED:
                self.events.append(dict(ev, kind=REJECTED_EVENT, coef=tuple(self.coef[source])))
                continue
            if max(abs(n - o) for n, o in zip(coef, self.coef[source])) <= self.min_step:
                continue
            self.coef[source] = tuple(coef)
            self.events.append(dict(ev, kind=CHANGED, coef=tuple(coef)))

    def poll(self):
        out, self.events = self.events, []
        return out

    def coeffs(self):
        return np.array(self.coef, dtype=np.int16)


# ------------------------------------------------------------ the image-rejection signal ----

def image_signal(n=131072, g=0.8, phi_deg=10.0, seed=5, amplitude=60.0, bin_=37, nfft=256, sigma=4.0):
    """A carrier at bin ``bin_`` of ``nfft`` with noise, through a front end whose Q has gain g and phase error phi:
    interleaved bytes rint(v + 127.4), uint8 [2 n]."""
    rng = np.random.default_rng(seed)
    th = 2.0 * np.pi * bin_ / nfft * np.arange(n)
    it = amplitude * np.cos(th) + rng.normal(0.0, sigma, n)
    qt = amplitude * np.sin(th) + rng.normal(0.0, sigma, n)
    phi = np.deg2rad(phi_deg)
    x = it
    y = g * (qt * np.cos(phi) + it * np.sin(phi))
    out = np.empty(2 * n, dtype=np.float64)
    out[0::2] = np.rint(x + 127.4)
    out[1::2] = np.rint(y + 127.4)
    return np.clip(out, 0, 255).astype(np.uint8)


def image_ratio_db(buf, bin_=37, nfft=256):
    """Power at bin ``bin_`` over power at its mirror bin, Hann-windowed ``nfft``-point frames, in dB."""
    z = buf[0::2].astype(np.float64) - 127.0 + 1j * (buf[1::2].astype(np.float64) - 127.0)
    frames = z[: z.size // nfft * nfft].reshape(-1, nfft) * np.hanning(nfft)
    p = (np.abs(np.fft.fft(frames, axis=1)) ** 2).sum(axis=0)
    return 10.0 * np.log10(p[bin_] / p[nfft - bin_])
