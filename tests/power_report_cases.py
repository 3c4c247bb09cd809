"""Shared inputs of the rtl_power report tests (tests/test_power_report_cpu.py, tests/test_power_report_gpu.py):
plans, accumulator rows over many decades, and the edge cases of "%.2f" of 10 log10."""
import ctypes as C
import ctypes.util
import functools

import numpy as np

from rtlsdr_amd import build as hipbuild
from rtlsdr_amd import capi

CROPS = (0.0, 0.2, 0.5)


def lib():
    hipbuild.build()
    return capi.load()


def plan_of(lo, hi, step, crop=0.0, boxcar=1):
    p = capi.RtlpowerPlan()
    r = lib().rtlpower_frequency_range(int(lo), int(hi), int(step), float(crop), int(boxcar), C.byref(p))
    return p if r == 0 and p.tune_count > 0 else None


# -f arguments that plan bin_e == 0 (giant bins: rms_power), 1 and 21
PLAN_BIN_E0 = (50_000_000, 60_000_000, 2_000_000)
PLAN_BIN_E1 = (100_000_000, 101_500_000, 800_000)
PLAN_BIN_E21 = (100_000_000, 102_000_000, 1)


def random_plan(rng, max_bin_e=14):
    """(arg triple, crop, boxcar, plan) of a random range the planner accepts."""
    while True:
        lo = int(rng.integers(24_000_000, 1_600_000_000))
        width = int(rng.choice([rng.integers(20_000, 900_000), rng.integers(900_000, 3_000_000),
                                rng.integers(3_000_000, 400_000_000)]))
        step = int(rng.choice([rng.integers(200, 20_000), rng.integers(20_000, 900_000), rng.integers(1_000_000, 2_500_000)]))
        crop = float(rng.choice(CROPS))
        boxcar = int(rng.integers(0, 2))
        p = plan_of(lo, lo + width, step, crop, boxcar)
        if p is not None and p.bin_e <= max_bin_e:
            return (lo, lo + width, step), crop, boxcar, p


def random_avg(rng, n, zeros=True):
    """Accumulators over seventeen decades, some of them empty."""
    a = np.floor(10.0 ** rng.uniform(0.0, 17.0, size=n)).astype(np.int64)
    if zeros and n > 1:
        a[rng.random(n) < 0.03] = 0
    return a


_libm = None


def _log10(x):
    global _libm
    if _libm is None:
        _libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.log10.restype = C.c_double
        _libm.log10.argtypes = [C.c_double]
    return _libm.log10(x)


def dbm_of(avg, rate, samples):
    """csv_dbm()'s expression (src/rtl_power.c:749-752) with the C library's log10."""
    return 10 * _log10(float(int(avg)) / float(rate) / float(samples))


@functools.lru_cache(maxsize=None)
def find_ties(rate, want=12):
    """(avg, samples) whose dBm is EXACTLY k + 0.125 / 0.375 / 0.625 / 0.875: "%.2f" has to round an exact tie.
    avg of the order 1e15 makes one unit of avg a few ulps of the result, so a search over samples finds hits."""
    out = []
    for d in (m + f for m in (-2, 7, -5, 3, 0, -8, 5, 1, -4, 8, -1, 2, 6, -7, 4, -3, -6) for f in (0.125, 0.375, 0.625, 0.875)):
        x = 10.0 ** (d / 10.0)
        for samples in range(400_000_000, 400_000_300):
            a0 = int(round(x * rate * samples))
            for a in range(a0 - 3, a0 + 4):
                if 0 < a < (1 << 53) and dbm_of(a, rate, samples) == d:
                    out.append((a, samples, d))
                    break
            else:
                continue
            break
        if len(out) >= want:
            break
    return tuple(out)  # (searched once per rate and shared: do not change it)


def edge_row(rate, samples, n):
    """A row of n >= 16 accumulators for (rate, samples): empty bins, -0.00, 0.00, the neighbours of 0 dB, huge and tiny."""
    one = int(rate) * int(samples)
    vals = [0, 1, 2, one - 1, one, one + 1, one - one // 1000, one + one // 2000, 1 << 52, (1 << 62) + 12345,
            9_007_199_254_740_993, 10 * one, one // 10 + 1, 3, 7, 0]
    a = np.array((vals * ((n + len(vals) - 1) // len(vals)))[:n], dtype=np.int64)
    return a
