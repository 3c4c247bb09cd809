"""rtl_power on overdriven tones, without a GPU: the recorded inputs of tests/golden/power_hard.json are what they were, wrap
fix_fft's int16 stores in every stage they promise, and on them the counting model (tests/power_hard.py), the oracle and
the reference's own scanner() give the same avg[] and samples.  The suite's other inputs wrap none - the reason these exist."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import power_hard as ph
import reference_record as rr
from rtlsdr_amd import synth
from rtlsdr_amd.capi import RtlpowerCfg

RECORD = ph.load()
CASES = sorted(RECORD["cases"], key=lambda c: (RECORD["cases"][c]["cfg"]["bin_e"], c))
OTHER_WINDOW = 3  # Blackman-Harris: the non-rectangular window of the comparison


def _streams(case):
    kw = RECORD["cases"][case]["cfg"]
    n = kw["buf_len"] // 2 * RECORD["reads"]
    return kw, np.stack([ph.stream(rec, n) for rec in RECORD["cases"][case]["sets"]])


@pytest.mark.parametrize("case", CASES)
def test_bytes_match_the_record(case):
    kw, iq = _streams(case)
    assert RECORD["reads"] == ph.READS
    for rec, row in zip(RECORD["cases"][case]["sets"], iq):
        assert ph.sha(row) == rec["sha256"], (case, rec["inc"], rec["phase"])
        assert set(np.unique(row)) <= {rec["lo"], rec["hi"]}


def test_model_tables_are_the_oracles(oracle_lib):
    lib = oracle_lib._power_lib()
    for bin_e in sorted({RECORD["cases"][c]["cfg"]["bin_e"] for c in CASES} | {1}):
        n = 1 << bin_e
        mine = np.ctypeslib.as_array(C.cast(lib.orcp_sine_table(bin_e), C.POINTER(C.c_int16)), shape=(n * 3 // 4,))
        assert np.array_equal(ph.sine_table(bin_e), mine), bin_e
        assert np.array_equal(ph.window_coefs(0, n), oracle_lib.power_window_coefs(0, n)), bin_e


@pytest.mark.parametrize("case", CASES)
def test_model_equals_oracle(oracle_lib, case):
    """avg[] and samples of the model and of the oracle on every recorded set: the rectangle and one other window, sum and
    peak hold; under the rectangle the model's per-stage counts are the recorded ones, and stages 0 and 1 count nothing
    under either window (|q / 2| + |t| <= 16384 + 16384 behind twiddles on the axes)."""
    kw, iq = _streams(case)
    for window in (0, OTHER_WINDOW):
        cfgs = [RtlpowerCfg.default(window=window, peak_hold=peak, **kw) for peak in (0, 1)]
        wants = [oracle_lib.power_scan_batch(cfg, iq, nthreads=2) for cfg in cfgs]
        for k, rec in enumerate(RECORD["cases"][case]["sets"]):
            for peak, m in enumerate(ph.model_scan(cfgs[0], iq[k], peak_hold=(0, 1))):
                want, wn = wants[peak]
                assert m[1] == wn[k], (case, window, peak, k)
                assert np.array_equal(m[0], want[k]), (case, window, peak, k, np.flatnonzero(m[0] != want[k])[:8])
                assert m[2][0] == 0 and (len(m[2]) < 2 or m[2][1] == 0), (case, window, k, m[2])
                if window == 0:
                    assert [int(w) for w in m[2]] == rec["wraps"], (case, k)
                    assert (m.window_wraps, m.big_bins) == (rec["window_wraps"], rec["big_bins"]), (case, k)


@pytest.mark.parametrize("case", CASES)
def test_oracle_equals_live_reference(oracle_lib, case):
    """The oracle against the reference's scanner() (compiled in place where oracle/_ref is built, recorded from it
    otherwise) on every recorded set, rectangle window, sum and peak hold.  The record keeps a digest of each avg[] with
    its sum and maximum, not the spectra: 2^17 int64 bins per set would not fit a committed file."""
    kw, iq = _streams(case)
    cfgs = [RtlpowerCfg.default(window=0, peak_hold=peak, **kw) for peak in (0, 1)]

    def summary(rows):
        return {"sha256": np.array([hashlib.sha256(np.ascontiguousarray(a, dtype=np.int64).tobytes()).hexdigest() for a, _ in rows]),
                "sum": np.array([int(a.sum()) for a, _ in rows], dtype=np.int64), "max": np.array([int(a.max()) for a, _ in rows], dtype=np.int64),
                "samples": np.array([n for _, n in rows], dtype=np.int64)}

    def live():
        ref = oracle_lib.PowerReference()
        try:
            return summary([ref.scan_stream(cfg, row) for cfg in cfgs for row in iq])
        finally:
            ref.close()
    want = rr.result(oracle_lib.have_power_reference(), f"power_hard/scan/{case}", live, (sorted(kw.items()), iq))
    mine = []
    for cfg in cfgs:
        avg, n = oracle_lib.power_scan_batch(cfg, iq, nthreads=2)
        mine += [(avg[k], int(n[k])) for k in range(len(iq))]
    got = summary(mine)
    for name in ("samples", "sum", "max", "sha256"):
        assert np.array_equal(got[name], want[name]), (case, name, got[name], want[name])


@pytest.mark.parametrize("case", CASES)
def test_every_stage_has_an_input_that_wraps_there(case):
    """Up to 2^14 points every stage 2 .. bin_e - 1 has a recorded set that wraps in it; above, the search may have missed
    one stage per size, which the record names."""
    c = RECORD["cases"][case]
    bin_e = c["cfg"]["bin_e"]
    for s in range(2, bin_e):
        hit = [k for k, rec in enumerate(c["sets"]) if rec["wraps"][s] > 0]
        assert hit == c["stages"].get(str(s), []), (case, s)
        assert bool(hit) != (s in c["missing"]), (case, s)
    assert len(c["missing"]) <= (0 if bin_e <= 14 else 1), (case, c["missing"])
    assert c["total_wraps"] == [sum(rec["wraps"][s] for rec in c["sets"]) for s in range(bin_e)]
    for rec in c["sets"]:
        assert rec["wraps"][0] == 0 and rec["wraps"][1] == 0, (case, rec)
    # a bin at exactly 2^31 (what power_of reads as unsigned): used where the search met one, and the record says whether
    assert c["over_2_31"] is None or c["sets"][c["over_2_31"]]["big_bins"] > 0
    assert (case in RECORD["over_2_31_found"]) == (c["over_2_31"] is not None)
    assert (c["over_2_31"] is None) == all(rec["big_bins"] == 0 for rec in c["sets"])


@pytest.mark.parametrize("kw", [dict(bin_e=10, buf_len=16384), dict(bin_e=14, buf_len=32768)], ids=lambda kw: f"b{kw['bin_e']}")
def test_the_suites_other_inputs_wrap_nowhere(kw):
    """The control: the FM signal and the random bytes every other rtl_power test feeds (test_power_batched_vs_oracle's
    seeds and amplitude), and the bytes at the rails, wrap no store of any stage under the rectangle window."""
    cfg = RtlpowerCfg.default(window=0, **kw)
    L, nr = int(cfg.buf_len), 5
    iq = np.concatenate([synth.fm_iq_u8(6, L // 2 * nr, fs=2.048e6, dev_hz=30e3, seed=77), synth.random_u8(6, L * nr, seed=78),
                         ph.rail_streams(L * nr)])
    for s, row in enumerate(iq):
        m = ph.model_scan(cfg, row)
        assert not m[2].any(), (kw, s, m[2])
