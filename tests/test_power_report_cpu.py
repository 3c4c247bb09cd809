"""rtl_power's report without a GPU: rtlpower_report_host (the definition of every value rtlpower_gpu_report returns)
and rtlpower_csv_report (the line from such values) against csv_dbm() - the product's own rtlpower_csv_dbm always,
the reference's csv_dbm() compiled in place (oracle/_ref) where it exists."""
import ctypes as C

import numpy as np
import pytest

import power_report_cases as prc
from rtlsdr_amd import capi, power


def _mine(plan, tune, avg, samples):
    """The new path: values by rtlpower_report_host, line by rtlpower_csv_report; avg must come back untouched."""
    keep = avg.copy()
    centi = power.report_host(avg, samples, float(plan.rate), plan.bin_e, plan.crop)
    assert np.array_equal(avg, keep), "rtlpower_report_host changed its input"
    return centi, power.csv_report(plan, tune, centi, samples)


def _old(plan, tune, avg, samples):
    a = avg.copy()
    buf = C.create_string_buffer(a.size * 16 + 512)
    n = prc.lib().rtlpower_csv_dbm(C.byref(plan), tune, a.ctypes.data, samples, buf, len(buf))
    assert n > 0
    return buf.raw[:n]


class _Ref:
    """The reference's csv_dbm() through ref_frequency_range / ref_csv_dbm, as tests/test_power_oracle.py reaches it."""

    def __init__(self, oracle_lib):
        self.ref = oracle_lib.PowerReference()
        self.ref.lib.ref_frequency_range.argtypes = [C.c_char_p, C.c_double, C.c_int, C.c_void_p, C.POINTER(C.c_double)]
        self.ref.lib.ref_csv_dbm.argtypes = [C.c_int, C.c_void_p, C.c_int32, C.c_char_p, C.c_size_t]

    def line(self, arg, crop, boxcar, tune, avg, samples):
        o = np.zeros(10, dtype=np.int32)
        rc = C.c_double()
        self.ref.lib.ref_frequency_range(("%d:%d:%d" % arg).encode(), crop, boxcar, o.ctypes.data, C.byref(rc))
        buf = C.create_string_buffer(avg.size * 16 + 512)
        n = self.ref.lib.ref_csv_dbm(tune, avg.ctypes.data, samples, buf, len(buf))
        assert n > 0
        return buf.raw[:n]

    def close(self):
        self.ref.close()


def _triples():
    """At least 200 (arg, crop, boxcar, plan, tune, avg, samples)."""
    rng = np.random.default_rng(20261)
    out = []
    for k in range(220):
        arg, crop, boxcar, plan = prc.random_plan(rng, max_bin_e=12 if k % 8 else 14)
        tune = int(rng.integers(0, plan.tune_count))
        samples = int(rng.choice([1, 7, int(rng.integers(1, 2000)), int(rng.integers(1, 1 << 30))]))
        avg = prc.random_avg(rng, 1 << plan.bin_e)
        if k % 5 == 0:  # the edge values in every position a crop leaves
            e = prc.edge_row(plan.rate, samples, max(16, avg.size))[:avg.size]
            at = rng.permutation(avg.size)[:e.size]
            avg[at] = e[:at.size]
        out.append((arg, crop, boxcar, plan, tune, avg, samples))
    for arg in (prc.PLAN_BIN_E0, prc.PLAN_BIN_E1, prc.PLAN_BIN_E21):  # (the test asserts that bin_e 0, 1 and 21 were seen)
        for crop in prc.CROPS:
            plan = prc.plan_of(*arg, crop)
            avg = prc.random_avg(rng, 1 << plan.bin_e)
            out.append((arg, crop, 1, plan, plan.tune_count - 1, avg, 1234))
    return out


def test_report_host_and_csv_report_equal_csv_dbm():
    """Always: the product's own csv_dbm on a copy of the same array, byte for byte."""
    triples = _triples()
    assert len(triples) >= 200
    seen = set()
    for arg, crop, boxcar, plan, tune, avg, samples in triples:
        centi, line = _mine(plan, tune, avg, samples)
        assert line == _old(plan, tune, avg, samples), (arg, crop, boxcar, tune, samples)
        seen.add(plan.bin_e)
    assert {0, 1, 21} <= seen and len(seen) >= 8, sorted(seen)


def test_report_host_and_csv_report_equal_the_live_reference(oracle_lib):
    if not oracle_lib.have_power_reference():
        pytest.skip("oracle/_ref is not built here")
    ref = _Ref(oracle_lib)
    try:
        for arg, crop, boxcar, plan, tune, avg, samples in _triples():
            _, line = _mine(plan, tune, avg, samples)
            assert line == ref.line(arg, crop, boxcar, tune, avg, samples), (arg, crop, boxcar, tune, samples)
    finally:
        ref.close()


def _one_bin_plan():
    plan = prc.plan_of(100_000_000, 102_000_000, 1_000)  # one hop
    assert plan.tune_count == 1
    return plan


def test_empty_bins_print_minus_inf():
    plan = _one_bin_plan()
    avg = np.zeros(1 << plan.bin_e, dtype=np.int64)
    avg[5] = 1000
    centi, line = _mine(plan, 0, avg, 3)
    assert (centi.view(np.uint32) == 0xFFFFFFFF).sum() == avg.size + 1 - 1
    assert line == _old(plan, 0, avg, 3) and b"-inf, -inf" in line and line.endswith(b"-inf\n")


def test_minus_zero_and_zero():
    """avg = rate * samples - 1 lies in (-0.005, 0) dB and prints "-0.00"; avg = rate * samples prints "0.00"."""
    plan = _one_bin_plan()
    samples = 1000
    one = plan.rate * samples
    avg = np.full(1 << plan.bin_e, one, dtype=np.int64)
    avg[2::2] = one - 1
    centi, line = _mine(plan, 0, avg, samples)
    u = centi.view(np.uint32)
    assert set(u.tolist()) == {0, capi.CENTI_SIGN}
    assert line == _old(plan, 0, avg, samples) and b", -0.00, 0.00, -0.00, " in line


def test_exact_ties_round_as_printf_does():
    """dBm values that ARE k + 0.125 etc. in binary: "%.2f" rounds the exact tie to even; whatever glibc does is the law."""
    plan = _one_bin_plan()
    ties = prc.find_ties(plan.rate)
    assert len(ties) >= 4, ties
    for a, samples, d in ties:
        assert prc.dbm_of(a, plan.rate, samples) == d
        avg = np.full(1 << plan.bin_e, a, dtype=np.int64)
        centi, line = _mine(plan, 0, avg, samples)
        assert line == _old(plan, 0, avg, samples), (a, samples, d)
        want = ("%.2f" % d).encode()
        fields = line.rstrip(b"\n").split(b", ")
        assert len(fields) == 4 + avg.size + 1 and set(fields[4:-1]) == {want}, (d, line[-40:])  # (the trailing value is another expression)
        mag = int(centi.view(np.uint32)[0] & 0x7FFFFFFF)
        assert mag == int(want.lstrip(b"-").replace(b".", b"")), (d, mag)
        assert abs(mag - abs(d) * 100) == 0.5


def test_live_reference_on_the_edge_cases(oracle_lib):
    if not oracle_lib.have_power_reference():
        pytest.skip("oracle/_ref is not built here")
    ref = _Ref(oracle_lib)
    try:
        arg = (100_000_000, 102_000_000, 1_000)
        plan = _one_bin_plan()
        for a, samples, d in prc.find_ties(plan.rate):
            avg = np.full(1 << plan.bin_e, a, dtype=np.int64)
            assert _mine(plan, 0, avg, samples)[1] == ref.line(arg, 0.0, 1, 0, avg, samples), (a, samples, d)
        for crop in prc.CROPS:
            plan = prc.plan_of(*arg, crop)
            for samples in (1, 1000, 123456):
                avg = prc.edge_row(plan.rate, samples, 1 << plan.bin_e)
                assert _mine(plan, 0, avg, samples)[1] == ref.line(arg, crop, 1, 0, avg, samples), (crop, samples)
    finally:
        ref.close()


def test_a_hop_without_samples_reports_nothing():
    plan = _one_bin_plan()
    avg = np.zeros(1 << plan.bin_e, dtype=np.int64)
    centi = power.report_host(avg, 0, float(plan.rate), plan.bin_e, plan.crop)
    assert centi.size == 0
    assert power.csv_report(plan, 0, centi, 0) == b""


def test_bad_arguments_are_refused():
    lib = prc.lib()
    avg = np.ones(16, dtype=np.int64)
    out = np.zeros(17, dtype=np.int32)
    n = C.c_int()
    assert lib.rtlpower_report_host(avg.ctypes.data, 1, 2.0e6, 4, 1.0, out.ctypes.data, C.byref(n)) == -22  # crop 1: no bins
    assert lib.rtlpower_report_host(avg.ctypes.data, 1, 0.0, 4, 0.0, out.ctypes.data, C.byref(n)) == -22
    assert lib.rtlpower_report_host(avg.ctypes.data, 1, 2.0e6, 22, 0.0, out.ctypes.data, C.byref(n)) == -22
    plan = _one_bin_plan()
    small = C.create_string_buffer(64)
    assert lib.rtlpower_csv_report(C.byref(plan), 0, out.ctypes.data, 16, 5, small, len(small)) == -105  # -ENOBUFS


def test_report_without_a_gpu_fails_as_create_does():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = C.c_void_p()
    cfg = capi.RtlpowerCfg.default()
    assert prc.lib().rtlpower_gpu_create(C.byref(cfg), 1, 0, C.byref(h)) == -19
    assert prc.lib().rtlpower_gpu_report(None, 2.0e6, 0.0, 1) == -22
