"""Full-scale audio and resampling-ratio edges for the stages behind the demodulator - low_pass_simple, deemph_filter,
dc_block_audio_filter, low_pass_real, arbitrary_upsample, arbitrary_downsample (src/rtl_fm.c:739-775, 1011-1041, 1114-1166):
the inputs, a model that counts, and the case table that tests/golden/tail_hard.json (tests/golden/gen_tail_hard.py)
records and test_tail_hard_cpu.py / test_tail_hard_gpu.py read.

The suite's other inputs never put a sample beyond half of int16 behind the demodulator (FM is bounded by 16384, the
AM / USB / LSB audio of the sweeps peaks near 7300), and draw their rate pairs from a dozen ratios.  Here the audio spans
int16 (rtl_fm -M am / usb / lsb with the planner's own output_scale on bytes at the rails, and a scale of 181 behind a
single pass), and the rate pairs are chosen per class of the resamplers' index maps: len2 == len1, len1 +- 1, 0, 1,
buffers of 2 and 3 samples, runs whose short buffers are downsampled and whose long ones are upsampled, x 10.

The model is a second spelling of the six stages in Python integers (doubles where the reference computes in double);
it shares no code with oracle/rtlfm_oracle.c, takes the demodulated samples from the oracle run with the tail switched
off (the demodulators are not what it is a second opinion on), writes every int16 / int32 store out as a wrap and counts
the stores whose exact value lay outside the stored type.

Doubt flags: an output of arbitrary_upsample is trunc(a (1 - t / len2) + b t / len2) computed in double; a term of
arbitrary_downsample is trunc(b (len1 - tick) / len2 + carry).  Where the exact rational value (denominator len2) is not
an integer it lies at least 1 / len2 > 1e-5 from one and a few roundings of doubles (1e-11 at these magnitudes) or a
contracted multiply-add cannot change the truncation: the output is determined.  Where it is an integer v, a rounding may
leave v - epsilon or v + epsilon and the truncation is v or the integer next to it towards zero: the output is flagged,
and `alts` holds every value it may take (the other truncation pushed through the rest of the stage).  Terms the double
arithmetic computes exactly whatever the contraction - a fraction of exactly 0 or 1 - are not flagged."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

import power_hard as ph
from rtlsdr_amd import capi, synth
from rtlsdr_amd.capi import RtlfmCfg

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tail_hard.json")
FLAG_CAP = 0.05   # the most of a case's resampled outputs that may be flagged
BIG_D = 49152     # |x - avg| beyond this: the numerators deemph_filter's division forms had not seen
WRAPS = ("post", "adc", "lpr16", "lpr32", "down_cast", "down_acc")  # + deemph's max_d: the seven of the issue
TAIL_STATE = ("now_lpr", "prev_lpr_index", "deemph_avg", "dc_avg")
I16 = (-32768, 32767)
I32 = (-(1 << 31), (1 << 31) - 1)


def load():
    with open(FIXTURE) as f:
        return json.load(f)


# ---- the inputs: integer arithmetic only (and numpy's seeded generator for the random bytes) ----

def stream(rec, nbytes):
    """The bytes of a stream record:
    {"kind": "square", inc, phase, lo, hi[, key]}  a hard-limited carrier (power_hard.square_iq); with `key`, keyed on and
        off: the samples n with (n key) mod 2^32 >= 2^31 read 127 / 127; with `flip`, its phase reversed (lo <-> hi) on
        the samples n with (n flip) mod 2^32 >= 2^31.  inc = 2^30, phase = 0x60000000 is the carrier a quarter of the sample
        rate up that the callback's rotation turns into the constant (127, 127): a constant envelope, and with `flip` an
        audio that jumps between the two ends of its range;
    {"kind": "random", seed}  full-scale random bytes (synth.random_u8)."""
    if rec["kind"] == "random":
        return synth.random_u8(1, nbytes, seed=rec["seed"])[0]
    assert rec["kind"] == "square"
    iq = ph.square_iq(rec["inc"], rec["phase"], nbytes // 2, rec["lo"], rec["hi"])
    if rec.get("flip"):
        rev = ((np.arange(nbytes // 2, dtype=np.uint64) * np.uint64(rec["flip"])) & np.uint64(0xFFFFFFFF)) >= np.uint64(1 << 31)
        iq[np.repeat(rev, 2)] = (rec["lo"] + rec["hi"]) - iq[np.repeat(rev, 2)]
    if rec.get("key"):
        off = ((np.arange(nbytes // 2, dtype=np.uint64) * np.uint64(rec["key"])) & np.uint64(0xFFFFFFFF)) >= np.uint64(1 << 31)
        iq[0::2][off] = 127
        iq[1::2][off] = 127
    return iq


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


RAIL = dict(kind="square", inc=1 << 30, phase=0x60000000, lo=0, hi=254)               # constant envelope at the rails
KEYED = dict(kind="square", inc=1 << 30, phase=0x60000000, lo=0, hi=254, key=1 << 21)   # ... keyed: 1024 samples on, 1024 off
SLOW = dict(kind="square", inc=(1 << 30) + (1 << 19), phase=0x60000000, lo=0, hi=254)  # ... slipping a quadrant every 2048 samples
FLIP = dict(RAIL, flip=1 << 21)                                                        # ... reversed every 1024 samples
HALF = dict(kind="square", inc=(1 << 30) + (1 << 20), phase=0x60000000, lo=64, hi=190)  # half the rails: x scale stays inside int16


HALF_FLIP = dict(HALF, inc=1 << 30, flip=1 << 21)


def rnd(seed):
    return dict(kind="random", seed=seed)


# ---- the model ----

def wrap(v, bits=16):
    h = 1 << (bits - 1)
    return ((v + h) & ((1 << bits) - 1)) - h


def _cdiv(a, b):
    """C's division: toward zero."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


class Info(dict):
    """Per-stage counts of the stores whose exact value lay outside the stored type (WRAPS, "deemph_store"), max_d = the
    largest |x - avg| deemph_filter divided, peak = the largest |sample| any stage was handed, outputs / flagged of the
    arbitrary resamplers."""
    def __init__(self):
        super().__init__({k: 0 for k in WRAPS + ("deemph_store", "max_d", "peak", "outputs", "flagged")})

    def add(self, other):
        for k, v in other.items():
            self[k] = max(self[k], v) if k in ("max_d", "peak") else self[k] + v


def low_pass_simple(x, step, info):
    """:739-753: sums of `step` samples stored to int16."""
    out = []
    for base in range(0, len(x) - len(x) % step, step):
        acc = sum(x[base:base + step])
        info["post"] += not I16[0] <= acc <= I16[1]
        out.append(wrap(acc))
    return out


def deemph_filter(x, a, avg, info):
    """:1011-1026: avg += (d +- a / 2) / a with C's division, d = x - avg; the sample becomes (int16_t)avg."""
    half, out, big = a // 2, [], info["max_d"]
    for v in x:
        d = v - avg
        if d > 0:
            avg += (d + half) // a
            big = d if d > big else big
        else:
            avg -= (half - d) // a
            big = -d if -d > big else big
        if not -32768 <= avg <= 32767:
            info["deemph_store"] += 1
            out.append(wrap(avg))
        else:
            out.append(avg)
    info["max_d"] = big
    return out, avg


def dc_block_audio(x, k, dc_avg, info):
    """:1028-1041: the buffer's mean (C division of the int64 sum), smoothed over k + 1, subtracted in int16."""
    if not x:
        return x, dc_avg
    mean = _cdiv(sum(x), len(x))
    mean = _cdiv(mean + dc_avg * k, k + 1)
    assert I32[0] <= dc_avg * k <= I32[1]
    out = []
    for v in x:
        info["adc"] += not I16[0] <= v - mean <= I16[1]
        out.append(wrap(v - mean))
    return out, mean


def low_pass_real(x, fast, slow, now, idx, info):
    """:755-775: now_lpr += x (int); prev_lpr_index += slow; at >= fast: (int16_t)(now_lpr / (fast / slow))."""
    div, out = fast // slow, []
    for v in x:
        now += v
        if not I32[0] <= now <= I32[1]:
            info["lpr32"] += 1
            now = wrap(now, 32)
        idx += slow
        assert I32[0] <= idx <= I32[1]
        if idx >= fast:
            q = _cdiv(now, div)
            info["lpr16"] += not I16[0] <= q <= I16[1]
            out.append(wrap(q))
            idx -= fast
            now = 0
    return out, now, idx


def _other(v):
    """The values trunc() may leave of a double next to the integer v."""
    return {v, v - 1} if v > 0 else {v, v + 1} if v < 0 else {0}


def arbitrary_upsample(b1, len2, info, alts, base):
    """:1114-1135.  alts[base + j]: what a flagged output j may be."""
    len1, out = len(b1), []
    src, tick = 1, 0
    for j in range(len2):
        frac = tick / len2
        out.append(wrap(int(b1[src - 1] * (1 - frac) + b1[src] * frac)))
        num = b1[src - 1] * (len2 - tick) + b1[src] * tick
        if tick not in (0, len2) and num % len2 == 0:
            info["flagged"] += 1
            alts[base + j] = _other(num // len2)
        tick += len1
        if tick > len2:
            tick -= len2
            src += 1
        if src >= len1:
            src, tick = len1 - 1, len2
    info["outputs"] += len2
    return out


def arbitrary_downsample(b1, len2, info, alts, base):
    """:1137-1166: a fractional boxcar from b1[1] on; the term is converted to int and stored to int16 (the x86 build's
    convert-then-truncate), the int16 accumulator wraps, and cur * len2 / len1 at the end is int arithmetic: a product
    outside int32 is undefined in the reference, so a case that gets there is refused here."""
    len1, out = len(b1), []
    src, j, tick = 1, 0, 0
    carry, carry_num, exact_carry = 0.0, 0, True
    cur, curs = 0, {0}   # the accumulator, and every value it may have where terms were flagged

    def scaled(c):
        assert I32[0] <= c * len2 <= I32[1], "cur * len2 leaves int32: undefined in the reference"
        return wrap(_cdiv(c * len2, len1))
    while j < len2:
        frac, fnum = 1.0, len2
        if tick + len2 > len1:
            fnum = len1 - tick
            frac = fnum / len2
        t = int(b1[src] * frac + carry)
        num = b1[src] * fnum + carry_num
        cands = {t}
        if not (fnum in (0, len2) and exact_carry) and num % len2 == 0:
            cands = _other(num // len2)
            assert t in cands, (t, cands)
        info["down_cast"] += not I16[0] <= t <= I16[1]
        info["down_acc"] += not I16[0] <= cur + wrap(t) <= I16[1]
        curs = {wrap(c + wrap(o)) for c in curs for o in cands}
        cur = wrap(cur + wrap(t))
        carry = b1[src] * (1.0 - frac)
        carry_num, exact_carry = b1[src] * (len2 - fnum), fnum in (0, len2)
        tick += len2
        src += 1
        if tick > len1:
            out.append(scaled(cur))
            if len(curs) > 1:
                info["flagged"] += 1
                alts[base + j] = {scaled(c) for c in curs}
            j += 1
            cur, curs = 0, {0}
            tick -= len1
        if src >= len1:
            src, tick = len1 - 1, len1
    info["outputs"] += len2
    return out


def model_tail(cfg, blocks, state=None):
    """full_demod() behind mode_demod (:1260-1271) on the demodulated buffers `blocks` (lists of ints) of one stream ->
    (the output samples, the carried fields TAIL_STATE, Info, alts {output index: set of values a flagged output may take},
    the output length per buffer)."""
    st = dict.fromkeys(TAIL_STATE, 0)
    st.update(state or {})
    info, alts, out, lens = Info(), {}, [], []
    for x in blocks:
        x = [int(v) for v in x]
        peak = lambda: info.__setitem__("peak", max([info["peak"]] + [abs(v) for v in x]))  # noqa: E731
        peak()
        if cfg.post_downsample > 1:
            assert len(x) % cfg.post_downsample == 0
            x = low_pass_simple(x, cfg.post_downsample, info); peak()
        if cfg.deemph:
            x, st["deemph_avg"] = deemph_filter(x, cfg.deemph_a, st["deemph_avg"], info); peak()
        if cfg.dc_block_audio:
            x, st["dc_avg"] = dc_block_audio(x, cfg.adc_block_const, st["dc_avg"], info); peak()
        if cfg.rate_out2 > 0:
            if cfg.resampler == capi.RESAMPLE_ARBITRARY:
                len2 = len(x) * cfg.rate_out2 // cfg.rate_out
                x = (arbitrary_upsample if len(x) < len2 else arbitrary_downsample)(x, len2, info, alts, len(out))
            else:
                x, st["now_lpr"], st["prev_lpr_index"] = low_pass_real(x, cfg.rate_out, cfg.rate_out2, st["now_lpr"], st["prev_lpr_index"], info)
        out += x
        lens.append(len(x))
    return np.array(out, dtype=np.int64).astype(np.int16), st, info, alts, lens


# ---- the oracle's side: the demodulated samples, and the chain ----

def tail_off(cfg):
    c = RtlfmCfg.from_buffer_copy(bytes(cfg))
    c.post_downsample, c.deemph, c.dc_block_audio, c.rate_out2 = 1, 0, 0, -1
    return c


def demodulated(po, cfg, row):
    """The buffers of one stream as mode_demod leaves them: the oracle with the tail switched off, buffer by buffer."""
    lib, c = po.oracle(), tail_off(cfg)
    L = int(c.block_len)
    st = po.new_states(1)
    scratch = np.zeros(po.result_cap(c), dtype=np.int16)
    row = np.ascontiguousarray(row, dtype=np.uint8)
    blocks = []
    for b in range(row.size // L):
        n = lib.orc_block(C.byref(c), C.byref(st[0]), row[b * L:(b + 1) * L], L, scratch)
        assert n >= 0, n
        blocks.append(scratch[:n].astype(np.int64))
    return blocks


def planner_scale(po, mode, downsample, passes):
    """output_scale as optimal_settings() (:1407-1445) leaves it for this decimation."""
    c = RtlfmCfg.default(mode=mode)
    po.oracle().orc_optimal_settings(C.byref(c), 100000000, 1, downsample - 1 if not passes else (1 << (passes - 1)) - 1, 1 if passes else 0, 0, None, None)
    assert c.downsample == downsample and c.downsample_passes == passes, (c.downsample, c.downsample_passes)
    return int(c.output_scale)


# ---- the case table ----

AM, USB, LSB, FM = capi.MODE_AM, capi.MODE_USB, capi.MODE_LSB, capi.MODE_FM
ARB, LPR = capi.RESAMPLE_ARBITRARY, capi.RESAMPLE_LOW_PASS_REAL
P1 = dict(downsample=2, downsample_passes=1)   # one fifth_order pass: L / 4 samples per buffer


def box(d):
    return dict(downsample=d, downsample_passes=0)


FM_STREAMS = "fm"   # the control: synth.fm_iq_u8, which wraps nowhere
HARD3 = [KEYED, RAIL, rnd(501), SLOW, FLIP, HALF_FLIP, HALF, rnd(502)]
UPS = [rnd(511), rnd(512), rnd(513), rnd(514)]  # in front of arbitrary_upsample: no stretches of equal samples, whose interpolation is an integer throughout
SCALE = "planner"
STREAM_SETS = {"HARD3": HARD3, "UPS": UPS, "fm": FM_STREAMS}  # what the record names; any other row lists its streams itself


def stream_set_name(c):
    """The name of a row's streams in the record, or the stream records themselves."""
    return next((k for k, v in STREAM_SETS.items() if c["streams"] == v), c["streams"])


def record_lens(rec):
    """The output length of every buffer, per stream, of a recorded case."""
    return [rec["lens"]["rows"][k] for k in rec["lens"]["of_stream"]]


def _row(name, klass, front, cfg, streams=None, L=8192, nb=3, scale=SCALE, inject=None, uniform=True):
    """klass: the stage or ratio class the row is in the table for; uniform: every buffer leaves the same count."""
    return dict(name=name, klass=klass, uniform=uniform, cfg=dict(front, **cfg), scale=scale, streams=HARD3 if streams is None else streams,
                L=L, nb=nb, inject=inject or {})


def _arb(r1, r2):
    return dict(rate_out=r1, rate_out2=r2, resampler=ARB)


def _lpr(r1, r2):
    return dict(rate_out=r1, rate_out2=r2, resampler=LPR)


CASES = [
    # -- the stages, at full scale (2048 samples per buffer behind P1: deemph_scans' one-pass and four-pass forms engage)
    _row("post4_usb", "post", P1, dict(mode=USB, post_downsample=4)),
    _row("post2_am_box1", "post", box(1), dict(mode=AM, post_downsample=2)),
    _row("post4_fm", "post", P1, dict(mode=FM, post_downsample=4), streams=FM_STREAMS),
    _row("deemph2_usb181", "deemph", P1, dict(mode=USB, deemph=1, deemph_a=2), scale=181),
    _row("deemph4_lsb", "deemph", P1, dict(mode=LSB, deemph=1, deemph_a=4)),
    _row("deemph13_usb", "deemph", P1, dict(mode=USB, deemph=1, deemph_a=13)),
    _row("deemph30_am", "deemph", box(1), dict(mode=AM, deemph=1, deemph_a=30)),
    _row("deemph40000_usb181", "deemph", P1, dict(mode=USB, deemph=1, deemph_a=40000), scale=181,
         inject=dict(deemph_avg=[-32768, 32767, -30000, 30000, -32768, 32767, 0])),
    _row("deemph13_fm", "deemph", P1, dict(mode=FM, deemph=1, deemph_a=13), streams=FM_STREAMS),
    _row("adc_usb", "adc", P1, dict(mode=USB, dc_block_audio=1), inject=dict(dc_avg=[40000, -40000, 0, 40000, -40000, 0, 40000])),
    _row("adc_am_box10", "adc", box(10), dict(mode=AM, dc_block_audio=1), uniform=False),
    _row("adc_fm", "adc", P1, dict(mode=FM, dc_block_audio=1), streams=FM_STREAMS),
    _row("deemph13_adc_usb", "adc", P1, dict(mode=USB, deemph=1, deemph_a=13, dc_block_audio=1)),
    # -- low_pass_real
    _row("lpr_div1_usb", "lpr div 1", P1, dict(mode=USB, **_lpr(24000, 12001))),          # fast / slow == 1, two inputs per output
    _row("lpr_same_am", "lpr same rate", box(1), dict(mode=AM, **_lpr(24000, 24000))),
    _row("lpr_rate1_usb181", "lpr rate 1", P1, dict(mode=USB, **_lpr(24000, 1)), scale=181,
         inject=dict(prev_lpr_index=[23990, 0, 20000, 23999, 17857, 1, 22000])),
    _row("lpr_fits_usb", "lpr phase outside", P1, dict(mode=USB, **_lpr(24000, 11025)),
         inject=dict(prev_lpr_index=[-5 * 24000, -1, 24000, 3 * 24000 + 7, 0, 23999, -24000],
                     now_lpr=[I32[1] - 3, I32[0] + 7, I32[1] - 10, I32[0] + 1, 0, 12345, -1])),
    _row("lpr_fits_box10_lsb", "lpr phase outside", box(10), dict(mode=LSB, **_lpr(170000, 32000)), uniform=False,
         inject=dict(prev_lpr_index=[-5 * 170000, -1, 170000, 3 * 170000 + 7, 0, 169999, -170000],
                     now_lpr=[I32[1] - 3, I32[0] + 7, I32[1] - 10, I32[0] + 1, 0, 12345, -1])),
    _row("lpr_div1_box10_am", "lpr div 1", box(10), dict(mode=AM, **_lpr(24000, 12001)), uniform=False),
    _row("lpr_same_box10_lsb", "lpr same rate", box(10), dict(mode=LSB, **_lpr(170000, 170000)), uniform=False),
    _row("lpr_rate1_box10_usb", "lpr rate 1", box(10), dict(mode=USB, **_lpr(24000, 1)), uniform=False,
         inject=dict(prev_lpr_index=[23990, 0, 23700, 23999, 23591, 1, 23180])),
    # ... and the injected phases in front of the kernels that run low_pass_real behind deemph_filter: k_deemph_spec_lpr,
    # k_deemph_scan_c_lpr + k_lpr_fixup, and k_low_pass_real behind the four passes (lpr_separate)
    _row("deemph13_lpr_fits_usb", "lpr phase outside", P1, dict(mode=USB, deemph=1, deemph_a=13, **_lpr(24000, 11025)),
         inject=dict(prev_lpr_index=[-5 * 24000, -1, 24000, 3 * 24000 + 7, 0, 23999, -24000],
                     now_lpr=[I32[1] - 3, I32[0] + 7, I32[1] - 10, I32[0] + 1, 0, 12345, -1],
                     deemph_avg=[0, 100, -32768, 32767, 70000, 5, -40000])),
    _row("lpr_wrap32_am", "lpr int32", box(1), dict(mode=AM, **_lpr(70000, 1)), streams=[RAIL], L=262144, nb=1, scale=181),
    _row("deemph13_lpr_usb", "lpr div 1", P1, dict(mode=USB, deemph=1, deemph_a=13, **_lpr(24000, 12001))),  # the one-pass and four-pass lpr forms
    _row("deemph13_lpr_wbfm", "lpr", box(2), dict(mode=FM, custom_atan=1, deemph=1, deemph_a=13, **_lpr(170000, 32000)), streams=FM_STREAMS),
    # -- arbitrary_resample: the ratio classes, each behind a front that gives uniform counts and one that does not
    _row("arb_same_usb", "len2 == len1", P1, dict(mode=USB, **_arb(24000, 24000))),
    _row("arb_same_box10_am", "len2 == len1", box(10), dict(mode=AM, **_arb(24000, 24000)), uniform=False),
    _row("arb_same_plus_usb181", "len2 == len1", P1, dict(mode=USB, **_arb(24000, 24001)), scale=181),       # 2048 * 24001 / 24000 floors to 2048
    _row("arb_same_plus_box372_lsb", "len2 == len1", box(372), dict(mode=LSB, **_arb(24000, 24001)), uniform=False),
    _row("arb_plus1_usb", "len2 == len1 + 1", P1, dict(mode=USB, **_arb(24000, 24012)), streams=UPS),            # 2048 -> 2049
    _row("arb_plus1_box68_am", "len2 == len1 + 1", box(68), dict(mode=AM, **_arb(100000, 102500)), streams=UPS, nb=5, uniform=False),  # 60 -> 61, 61 -> 62 (/ 372's 11 -> 12: a sixth flagged).
    # Five buffers, one more than the other rows have at most: 4096 = 60 * 68 + 16, so the long count of 61 first comes with the fifth.
    _row("arb_minus1_usb181", "len2 == len1 - 1", P1, dict(mode=USB, **_arb(24000, 23999)), scale=181),      # 2048 -> 2047
    _row("arb_minus1_box10_lsb", "len2 == len1 - 1", box(10), dict(mode=LSB, **_arb(24000, 23999)), uniform=False),  # 409 -> 408, 410 -> 409
    _row("arb_zero_usb", "len2 == 0", P1, dict(mode=USB, **_arb(24000, 11))),                        # 2048 * 11 / 24000 = 0
    _row("arb_zero_box372_am", "len2 == 0", box(372), dict(mode=AM, **_arb(24000, 1)), uniform=False),
    _row("arb_one_usb", "len2 == 1", P1, dict(mode=USB, **_arb(24000, 12))),                         # 2048 * 12 / 24000 = 1
    _row("arb_one_box1365_lsb", "len2 == 1", box(1365), dict(mode=LSB, **_arb(24000, 8000)), uniform=False),  # 3 -> 1, 4 -> 1
    _row("arb_len2_box2048_usb", "len1 in (2, 3)", box(2048), dict(mode=USB, **_arb(24000, 1212000)), streams=UPS),  # 2 -> 101 (2 -> 4: 4 | (b - a) tick for a fifth)
    _row("arb_len23_box1500_am", "len1 in (2, 3)", box(1500), dict(mode=AM, **_arb(24000, 24000)), uniform=False),  # 2 -> 2, 3 -> 3
    # (/ 1500 at a ratio of 1.4 - 2 -> 2 down, 3 -> 4 up - flags a sixth of its outputs: 4 | (b - a) tick; / 103 takes its place)
    _row("arb_mixed_box103_usb", "mixed down and up", box(103), dict(mode=USB, **_arb(100000, 102530)), streams=UPS, uniform=False),  # 39 -> 39 down, 40 -> 41 up
    _row("arb_mixed_box10_lsb", "mixed down and up", box(10), dict(mode=LSB, **_arb(170000, 170415)), streams=UPS, uniform=False),   # 409 -> 409, 410 -> 411
    _row("arb_x10_usb", "x 10", P1, dict(mode=USB, **_arb(24000, 240088)), streams=UPS),   # 2048 -> 20487 (20480 would flag a sixth: 10 | (b - a) m)
    _row("arb_x10_box10_am", "x 10", box(10), dict(mode=AM, **_arb(24000, 240088)), streams=UPS, uniform=False),
    _row("arb_down_usb181", "down", P1, dict(mode=USB, **_arb(24000, 13000)), scale=181),            # the inner cast and the accumulator
    _row("arb_down_box10_am", "down", box(10), dict(mode=AM, **_arb(24000, 9001)), uniform=False),
    _row("arb_down_fm", "down", P1, dict(mode=FM, **_arb(24000, 13000)), streams=FM_STREAMS),
    _row("deemph2_arb_up_usb181", "up", P1, dict(mode=USB, deemph=1, deemph_a=2, **_arb(16000, 22050)), streams=UPS, scale=181),  # the one kernel of config 3's tail
    _row("deemph13_arb_up_lsb", "up", P1, dict(mode=LSB, deemph=1, deemph_a=13, **_arb(16000, 22050)), streams=UPS),
    _row("arb_up64_usb", "64-bit index", box(1), dict(mode=USB, **_arb(100000, 100010)), streams=[rnd(503)], L=262144, nb=1),  # (nlo + 1) len2 >= 2^31
    _row("post2_deemph4_adc_arb_usb", "chain", P1, dict(mode=USB, post_downsample=2, deemph=1, deemph_a=4, dc_block_audio=1, **_arb(24000, 26300)), streams=UPS),
]
CLASSES_BOTH_FRONTS = ("len2 == len1", "len2 == len1 + 1", "len2 == len1 - 1", "len2 == 0", "len2 == 1", "len1 in (2, 3)", "x 10")


def case(name):
    return next(c for c in CASES if c["name"] == name)


def build(po, c):
    """(cfg, iq uint8 [ns, nb L], the injected states as the oracle's array or None) of a row."""
    kw = dict(c["cfg"])
    fm = c["streams"] == FM_STREAMS
    if kw["mode"] != FM:
        kw["output_scale"] = planner_scale(po, kw["mode"], kw["downsample"], kw["downsample_passes"]) if c["scale"] == SCALE else c["scale"]
    cfg = RtlfmCfg.default(block_len=c["L"], max_blocks=c["nb"], **kw)
    n = c["L"] * c["nb"]
    if fm:
        iq = synth.fm_iq_u8(4, n // 2, seed=600 + len(c["name"]), fs=1.024e6, dev_hz=75e3, amplitude=50.0)
    else:
        iq = np.stack([stream(rec, n) for rec in c["streams"]])
    st = None
    if c["inject"]:
        st = po.new_states(len(iq))
        for field, vals in c["inject"].items():
            for s in range(len(iq)):
                setattr(st[s], field, vals[s % len(vals)])
    return cfg, iq, st


def copy_states(st):
    arr = (capi.RtlfmStreamState * len(st))()
    for s in range(len(st)):
        arr[s] = capi.RtlfmStreamState.from_buffer_copy(bytes(st[s]))
    return arr


def model_case(po, c, cfg, iq):
    """The model on every stream of a row: [(out, state, Info, alts, lens)]."""
    res = []
    for s, row in enumerate(iq):
        st = {f: vals[s % len(vals)] for f, vals in c["inject"].items()}
        res.append(model_tail(cfg, demodulated(po, cfg, row), st))
    return res


def totals(res):
    t = Info()
    for r in res:
        t.add(r[2])
    return t
