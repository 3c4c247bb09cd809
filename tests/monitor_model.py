"""A restatement of the level monitor for the tests: the per-buffer ADC records in numpy, the trigger engine
in plain Python floats (math.log10 / math.sqrt, i.e. glibc's, as the C engine uses).

What it restates (reference src/rtl_fm.c): rtlsdr_callback's ADC statistics (:1302-1324), full_demod's level sum
(:1248-1253), checkTriggerCommand (:652-736) with testTrigCrit (:640-650), and the reset the controller makes on its
hop (:1556-1566) - with line i of the command file watched permanently by stream i (include/rtlfm_monitor.h).
"""
import math
import os

import numpy as np

STAT_DTYPE = np.dtype([("pow_sum", "<u4"), ("pow_count", "<i4"), ("max", "<i4"), ("step", "<i4")])
CRIT_IN, CRIT_OUT, CRIT_LT, CRIT_GT = range(4)
CRIT_NAMES = ("in", "out", "<", ">")
AUTO_GAIN = -100


def step_count(length: int):
    step = 2
    while length >= 16384 * step:
        step += 2
    return step, len(range(0, length, step))


def records(buffers) -> np.ndarray:
    """buffers: uint8 [..., block_len] -> records [...] (one per buffer)."""
    b = np.asarray(buffers, dtype=np.uint8)
    length = b.shape[-1]
    step, count = step_count(length)
    out = np.zeros(b.shape[:-1], dtype=STAT_DTYPE)
    out["max"] = b.max(axis=-1)
    i = b[..., 0::step].astype(np.int64) - 127
    q = b[..., 1::step].astype(np.int64) - 127
    assert i.shape[-1] == count and q.shape[-1] == count
    s = (i * i + q * q).sum(axis=-1)
    assert int(np.max(s)) < 2 ** 32
    out["pow_sum"] = s.astype(np.uint32)
    out["pow_count"] = count
    out["step"] = step
    return out


def rule(freq=100000000, gain=AUTO_GAIN, crit=CRIT_GT, ref_level=0.0, ref_tol=0.0, num_meas=10, num_block_trigger=0,
         check_adc_max=0, check_adc_rms=0, omit_first=3, command="", args=""):
    return dict(freq=freq, gain=gain, crit=crit, ref_level=ref_level, ref_tol=ref_tol, num_meas=num_meas,
                num_block_trigger=num_block_trigger, check_adc_max=check_adc_max, check_adc_rms=check_adc_rms,
                omit_first=omit_first, command=command, args=args)


def crit_holds(r, level):
    lo, hi = r["ref_level"] - r["ref_tol"], r["ref_level"] + r["ref_tol"]
    return {CRIT_IN: lo <= level <= hi, CRIT_OUT: lo > level or level > hi, CRIT_LT: level < lo, CRIT_GT: level > hi}[r["crit"]]


class StreamModel:
    """One stream's engine."""

    def __init__(self, stream: int, r: dict):
        self.stream = stream
        self.r = dict(r)
        if self.r["num_meas"] <= 0:
            self.r["num_meas"] = 10  # :611
        self.pow_sum, self.pow_count, self.sample_max = 0.0, 0, 0
        self.level_sum, self.num_summed = 0.0, 0
        self.omit_left = max(0, self.r["omit_first"])
        self.wait = 0
        self.cycle = 0
        self.stat = dict(count=0, sum=0.0, min=np.float32(0), max=np.float32(0))
        self.events = []

    def feed(self, rms, stats=None):
        r = self.r
        for b, level in enumerate(rms):
            if stats is not None:
                if r["check_adc_max"]:
                    self.sample_max = max(self.sample_max, int(stats[b]["max"]))
                if r["check_adc_rms"]:
                    self.pow_sum += float(int(stats[b]["pow_sum"])) / int(stats[b]["pow_count"])
                    self.pow_count += 1
            if self.num_summed < r["num_meas"] and level >= 0:
                self.level_sum += float(int(level))
                self.num_summed += 1
            if self.num_summed >= r["num_meas"]:
                self._end_cycle()

    def _end_cycle(self):
        r = self.r
        cycle = self.cycle
        self.cycle += 1
        if self.omit_left > 0:
            self.omit_left -= 1
        else:
            if self.wait > 0:
                self.wait = max(0, self.wait - r["num_meas"])
            level = 20.0 * math.log10(1E-10 + self.level_sum / self.num_summed)
            crit = crit_holds(r, level)
            st = self.stat
            f = np.float32(level)
            if st["count"] == 0:
                st.update(count=1, sum=level, min=f, max=f)
            else:
                st["count"] += 1
                st["sum"] += level
                st["min"] = min(st["min"], f)
                st["max"] = max(st["max"], f)
            ev = dict(stream=self.stream, cycle=cycle, crit_met=int(crit), adc_max=self.sample_max - 127,
                      adc_rms=math.sqrt(self.pow_sum / self.pow_count) if self.pow_count > 0 else -1.0, level_db=level)
            if self.wait <= 0:
                self.wait = r["num_block_trigger"] if crit else 0
                ev.update(fired=int(crit), blocked_for=0)
            else:
                ev.update(fired=0, blocked_for=self.wait)
            self.events.append(ev)
        self.level_sum, self.num_summed = 0.0, 0
        self.pow_sum, self.pow_count, self.sample_max = 0.0, 0, 0


def format_event(r: dict, ev: dict) -> str:
    """The -v line in the reference's wording (:704-733)."""
    mark = ("!!" if ev["adc_max"] >= 120 else "! ") if ev["adc_max"] >= 64 else "  "
    adc = ""
    if r["check_adc_max"] and r["check_adc_rms"]:
        adc = "adc max %3d%s rms %5.1f " % (ev["adc_max"], mark, ev["adc_rms"])
    elif r["check_adc_max"]:
        adc = "adc max %3d%s " % (ev["adc_max"], mark)
    elif r["check_adc_rms"]:
        adc = "adc rms %5.1f " % ev["adc_rms"]
    head = "%.3f kHz: gain %4.1f + level %4.1f dB %s=> " % (r["freq"] / 1000.0, 0.1 * r["gain"], ev["level_db"], adc)
    if ev["blocked_for"] <= 0:
        return head + ("activates trigger" if ev["fired"] else "does not trigger")
    return head + ("would trigger" if ev["crit_met"] else "does not trigger") + ", blocks for %d" % ev["blocked_for"]


def command_argv(r: dict, ev: dict):
    """argv of the triggered command: the arguments split at blanks, the placeholders replaced (:722-727)."""
    sub = {"!freq!": "%d" % r["freq"], "!gain!": "%d" % r["gain"], "!mlevel!": "%d" % int(0.5 + ev["level_db"] * 10.0),
           "!crit!": CRIT_NAMES[r["crit"]], "!reflevel!": "%d" % int(0.5 + r["ref_level"] * 10.0),
           "!reftol!": "%d" % int(0.5 + r["ref_tol"] * 10.0)}
    return [r["command"]] + [sub.get(a, a) for a in r["args"].split()]


def assert_events_equal(got, want, rel=1e-12):
    """Integers and flags exactly, dB values to `rel` relative."""
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        for k in ("stream", "cycle", "crit_met", "fired", "blocked_for", "adc_max"):
            assert g[k] == w[k], (k, g, w)
        for k in ("level_db", "adc_rms"):
            assert abs(g[k] - w[k]) <= rel * abs(w[k]), (k, g, w)


# ------------------------------------------------------------------ the reference's own accumulators ----

ACC_LENGTHS = (512, 16384, 16896, 32768, 65536, 131072, 262144)
ACC_BUFFERS, ACC_MEAS = 4, 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "monitor", "accumulators.npz")


def acc_input(length: int) -> np.ndarray:
    """Four buffers of one stream: full-scale and 0 ... 199 random bytes alternating (fixed seed)."""
    rng = np.random.default_rng(7000 + length)
    return np.stack([rng.integers(0, 256 if b % 2 == 0 else 200, length, dtype=np.uint8) for b in range(ACC_BUFFERS)])


def model_accumulators(bufs: np.ndarray, levels, num_meas: int):
    """(sampleMax, samplePowSum, samplePowCount, levelSum, numSummed) after the buffers, no cycle end in between."""
    m = StreamModel(0, rule(num_meas=10 ** 9, check_adc_max=1, check_adc_rms=1))
    m.feed([-1] * len(bufs), records(bufs))  # negative levels: the callback side only
    level_sum, n = 0.0, 0
    for lv in levels:
        if n < num_meas and lv >= 0:
            level_sum += float(int(lv))
            n += 1
    return m.sample_max, m.pow_sum, m.pow_count, level_sum, n
