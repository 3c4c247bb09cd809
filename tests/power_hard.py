"""Inputs on which fix_fft's int16 stores wrap, and a model of scanner() that counts them: what tests/golden/power_hard.json
(tests/golden/gen_power_hard.py) records and what test_power_hard_cpu.py / test_power_hard_gpu.py read.

fix_fft (src/rtl_power.c:271-327) computes tr, ti, qr +- tr and qi +- ti in int and stores them to int16_t.  A store can wrap
only where a butterfly's operands are large along an axis: |q / 2| + |t| > 32767 with |t| <= |x| / 2 needs a complex
magnitude above 32768.  Behind the rectangle window (x 256) a byte stream between the rails 0 and 254 is a square of
+-32512 whose fundamental is 4 / pi times that, about 41400: a station that drives the ADC into its rails.  Stages 0 and 1
cannot wrap (their twiddles lie on the axes: 16384 + 16384 at most).

The model is a second spelling of the chain, in numpy int64 with every int16 store written out as wrap16(); it shares no
code with the oracle (oracle/rtlpower_oracle.c) or with tests/channel_bank_model.py."""
import hashlib
import json
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "power_hard.json")
RAILS = ((0, 254), (1, 255), (0, 255))  # the symmetric pair; the two whose upper rail is +128, which x 256 folds to -32768
READS = 3                               # reads of a recorded stream


def load():
    with open(FIXTURE) as f:
        return json.load(f)


# ---- the inputs: integer arithmetic only, the same bytes on every machine ----

def _phase(inc, phase, nsamples):
    n = np.arange(nsamples, dtype=np.uint64)
    return (n * np.uint64(inc & 0xFFFFFFFF) + np.uint64(phase & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)


def square_iq(inc, phase, nsamples, lo, hi):
    """A hard-limited tone from a 32-bit phase accumulator: I is `hi` while (n inc + phase) mod 2^32 < 2^31, else `lo`;
    Q is I a quarter period later.  uint8 [2 nsamples], interleaved."""
    p = _phase(inc, phase, nsamples)
    q = (p + np.uint64(0xC0000000)) & np.uint64(0xFFFFFFFF)  # phase - 2^30
    out = np.empty(2 * nsamples, dtype=np.uint8)
    out[0::2] = np.where(p < np.uint64(1 << 31), hi, lo)
    out[1::2] = np.where(q < np.uint64(1 << 31), hi, lo)
    return out


def stream(rec, nsamples):
    """The bytes of a recorded parameter set {inc, phase, lo, hi}."""
    return square_iq(rec["inc"], rec["phase"], nsamples, rec["lo"], rec["hi"])


def sha(iq):
    return hashlib.sha256(np.ascontiguousarray(iq, dtype=np.uint8).tobytes()).hexdigest()


def rail_streams(nbytes):
    """The streams at the rails themselves: constant 0, 254, 255 and 1, the alternations 0 / 254 and 0 / 255 (sample by
    sample: the Nyquist tone), an impulse.  uint8 [7, nbytes]."""
    rows = [np.full(nbytes, b, dtype=np.uint8) for b in (0, 254, 255, 1)]
    for hi in (254, 255):
        a = np.zeros(nbytes, dtype=np.uint8)
        a[2::4] = hi; a[3::4] = hi
        rows.append(a)
    imp = np.full(nbytes, 127, dtype=np.uint8)
    imp[0] = 255; imp[1] = 0
    rows.append(imp)
    return np.stack(rows)


# ---- the model ----

def _fits(x):
    return isinstance(x, np.ndarray) and x.size > 0 and x.max() <= 32767 and x.min() >= -32768


def wrap16(x):
    """What a store to int16_t keeps of an int (an array that fits is returned as it is: two reductions, not three passes)."""
    return x if _fits(x) else ((x + 32768) & 0xFFFF) - 32768


def _outside(x):
    """How many of x a store to int16_t changes."""
    return 0 if _fits(x) else int(np.count_nonzero((x + 32768) >> 16))


def sine_table(bin_e):
    """sine_table(), src/rtl_power.c:247-261: three quarters of a period."""
    n = 1 << bin_e
    return np.round(32767 * np.sin(np.arange(n * 3 // 4, dtype=np.float64) * 2.0 * np.pi / n)).astype(np.int64)


def window_coefs(window, n):
    """(int)(256 w(i)), src/rtl_power.c:985-988.  The rectangle is spelled here; the other windows are the oracle's table
    (pinned to the reference's by test_power_functions_against_live_reference) - the window's shape is not what the model
    is a second opinion on."""
    if window == 0:
        return np.full(n, 256, dtype=np.int64)
    from oracle import pyoracle as po
    return po.power_window_coefs(window, n).astype(np.int64)


def _fix_mpy(a, b):
    """FIX_MPY, :263-269; returns (the int16 it stores, stores that wrapped)."""
    c = (a * b) >> 14
    v = (c >> 1) + (c & 1)
    return wrap16(v), _outside(v)


def fix_fft(re, im, bin_e):
    """fix_fft, :271-327, on frames [F, N] (int64 holding int16 values) -> (re, im, wraps int[bin_e]): wraps[s] counts the
    int16 stores of stage s - FIX_MPY's result, tr, ti and the four outputs - whose exact value lay outside int16."""
    n = 1 << bin_e
    F = re.shape[0]
    idx = np.arange(n)
    rev = np.zeros(n, dtype=np.int64)
    for b in range(bin_e):
        rev |= ((idx >> b) & 1) << (bin_e - 1 - b)
    re, im = re[:, rev], im[:, rev]  # :282-297: swaps m <-> mr once per pair
    sine = sine_table(bin_e)
    wraps = np.zeros(bin_e, dtype=np.int64)
    for s in range(bin_e):
        half = 1 << s
        j = np.arange(half) << (bin_e - 1 - s)
        wr = wrap16(sine[j + n // 4]) >> 1   # :305-308, int16_t wr, wi
        wi = wrap16(-sine[j]) >> 1
        re = re.reshape(F, n // (2 * half), 2, half)
        im = im.reshape(F, n // (2 * half), 2, half)
        xr, xi = re[:, :, 1, :], im[:, :, 1, :]
        a, w0 = _fix_mpy(wr, xr); b, w1 = _fix_mpy(wi, xi)
        c, w2 = _fix_mpy(wr, xi); d, w3 = _fix_mpy(wi, xr)
        tr, ti = a - b, c + d
        count = w0 + w1 + w2 + w3 + _outside(tr) + _outside(ti)
        tr, ti = wrap16(tr), wrap16(ti)      # :311-312
        qr, qi = re[:, :, 0, :] >> 1, im[:, :, 0, :] >> 1  # :313-316
        outs = (qr + tr, qi + ti, qr - tr, qi - ti)        # :317-320
        count += sum(_outside(o) for o in outs)
        re = np.stack([wrap16(outs[0]), wrap16(outs[2])], axis=2).reshape(F, n)
        im = np.stack([wrap16(outs[1]), wrap16(outs[3])], axis=2).reshape(F, n)
        wraps[s] = count
    return re, im, wraps


def _remove_dc(x, length):
    """remove_dc, :581-596, on the elements 0, 2, ... below `length` of x: the sum over length / 2 of them divided by
    `length` (C division: toward zero)."""
    k = (length + 1) // 2
    total = int(x[:k].sum())
    ave = wrap16(abs(total) // length * (1 if total >= 0 else -1))
    if ave:
        x[:k] = wrap16(x[:k] - ave)


def _decimated_by_oracle(cfg, read):
    """One read's int16 elements after downsample_iq x passes and generic_fir (:682-691), by the oracle's functions."""
    from oracle import pyoracle as po
    lib = po._power_lib()
    L = int(cfg.buf_len)
    buf = np.zeros(L + 32, dtype=np.int16)
    buf[:L] = read.astype(np.int16) - 127
    p0 = buf.ctypes.data
    for j in range(int(cfg.downsample_passes)):
        lib.orcp_fifth_order(p0, L >> j)
        lib.orcp_fifth_order(p0 + 2, (L >> j) - 1)
    if cfg.comp_fir_size == 9 and cfg.downsample_passes <= 10:
        lib.orcp_generic_fir(p0, L >> int(cfg.downsample_passes), int(cfg.downsample_passes))
        lib.orcp_generic_fir(p0 + 2, (L >> int(cfg.downsample_passes)) - 1, int(cfg.downsample_passes))
    return buf[:L].astype(np.int64)


class Scan(tuple):
    """(avg int64[N], samples, wraps int[bin_e]) with .window_wraps - window products outside int16 - and .big_bins -
    bins of a frame with |X|^2 > 2^31 - 1, which is (-32768, -32768) alone: exactly 2^31."""
    def __new__(cls, avg, samples, wraps, window_wraps, big_bins):
        t = super().__new__(cls, (avg, samples, wraps))
        t.window_wraps, t.big_bins = window_wraps, big_bins
        return t


def model_scan(cfg, iq, peak_hold=None):
    """scanner(), :657-718, for the reads of one stream iq (uint8, whole reads of cfg.buf_len bytes), undecimated, boxcar or
    fifth_order (+ FIR): - 127, the boxcar sums, remove_dc's half average, the window product and its wrap, fix_fft,
    real_conj in int64, then sum or maximum over the frames.  peak_hold = (0, 1): one Scan per way of folding the same
    frames (cfg.peak_hold is not read then)."""
    L, bin_e = int(cfg.buf_len), int(cfg.bin_e)
    n, ds = 1 << bin_e, max(1, int(cfg.downsample))
    iq = np.ascontiguousarray(iq, dtype=np.uint8).ravel()
    nreads = iq.size // L
    length = L // ds  # what remove_dc and the frame loop see
    assert bin_e >= 1 and nreads * L == iq.size and length % (2 * n) == 0, "whole reads of whole frames"
    coefs = window_coefs(int(cfg.window), n)
    frames_re, frames_im = [], []
    for r in range(nreads):
        read = iq[r * L:(r + 1) * L]
        if cfg.boxcar and ds > 1:
            assert (L // 2) % ds == 0
            x = read.astype(np.int64) - 127                                   # :666-668
            x = wrap16(x.reshape(L // 2 // ds, ds, 2).sum(axis=1)).ravel()    # :671-681 (int16 +=: wraps as the sum does)
        elif not cfg.boxcar and cfg.downsample_passes:
            x = _decimated_by_oracle(cfg, read)[:length]
        else:
            assert ds == 1
            x = read.astype(np.int64) - 127
        re, im = x[0::2].copy(), x[1::2].copy()
        _remove_dc(re, length)       # :692-693
        _remove_dc(im, length - 1)
        frames_re.append(re.reshape(-1, n)); frames_im.append(im.reshape(-1, n))
    re, im = np.concatenate(frames_re), np.concatenate(frames_im)
    pr, pi = re * coefs, im * coefs  # :697-706
    window_wraps = _outside(pr) + _outside(pi)
    re, im, wraps = fix_fft(wrap16(pr), wrap16(pi), bin_e)
    power = re * re + im * im        # real_conj, :636-640
    big_bins = int((power > (1 << 31) - 1).sum())
    def fold(peak):  # :708-716 (avg starts at 0 and no power is negative)
        return Scan(power.max(axis=0) if peak else power.sum(axis=0), ds * power.shape[0], wraps, window_wraps, big_bins)
    return fold(cfg.peak_hold) if peak_hold is None else [fold(p) for p in peak_hold]
