"""The level monitor without a GPU: the restatement (tests/monitor_model.py) against the reference's own accumulators,
the C engine (rtlfm_monitor_*, host code inside librtlfm_hip.so) against the restatement, the command file's grammar,
and the new symbols."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import monitor_model as mm
from rtlsdr_amd import build as hipbuild
from rtlsdr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MIN = -2 ** 31


@pytest.fixture(scope="module")
def lib():
    hipbuild.build()
    return capi.load()


# ------------------------------------------------------------ the restatement against the reference ----

class CmdState(C.Structure):
    """struct cmd_state of the reference (src/rtl_fm.c:118-147), FREQUENCIES_LIMIT = 1024."""
    _fields_ = [("filename", C.c_char_p), ("file", C.c_void_p), ("lineNo", C.c_int), ("acLine", C.c_char * 4096),
                ("checkADCmax", C.c_int), ("checkADCrms", C.c_int), ("prevFreq", C.c_uint32), ("prevGain", C.c_int),
                ("prevBandwidth", C.c_uint32), ("freq", C.c_uint32), ("gain", C.c_int), ("trigCrit", C.c_int),
                ("refLevel", C.c_double), ("refLevelTol", C.c_double), ("numMeas", C.c_int), ("numBlockTrigger", C.c_int),
                ("command", C.c_char_p), ("args", C.c_char_p), ("levelSum", C.c_double), ("numSummed", C.c_int),
                ("omitFirstFreqLevels", C.c_int), ("waitTrigger", C.c_int * 1024), ("statNumLevels", C.c_int * 1024),
                ("statFreq", C.c_uint32 * 1024), ("statSumLevels", C.c_double * 1024), ("statMinLevel", C.c_float * 1024),
                ("statMaxLevel", C.c_float * 1024)]


class DongleState(C.Structure):
    """struct dongle_state of the reference (src/rtl_fm.c:149-170), MAXIMUM_BUF_LENGTH = 262144."""
    _fields_ = [("exit_flag", C.c_int), ("thread", C.c_ulong), ("dev", C.c_void_p), ("dev_index", C.c_int),
                ("userFreq", C.c_uint32), ("freq", C.c_uint32), ("rate", C.c_uint32), ("bandwidth", C.c_uint32),
                ("gain", C.c_int), ("buf16", C.c_int16 * 262144), ("buf_len", C.c_uint32), ("ppm_error", C.c_float),
                ("offset_tuning", C.c_int), ("direct_sampling", C.c_int), ("mute", C.c_int), ("demod_target", C.c_void_p),
                ("samplePowSum", C.c_double), ("samplePowCount", C.c_int), ("sampleMax", C.c_ubyte)]


def acc_cfg(length):
    # offset tuning and no decimation: what rms() sees is the converted buffer itself
    return capi.RtlfmCfg.default(offset_tuning=1, block_len=length, max_blocks=mm.ACC_BUFFERS)


def acc_levels(oracle_lib, bufs):
    out = []
    for b in bufs:
        x = (b.astype(np.int16) - 127)
        out.append(oracle_lib.oracle().orc_rms(x.ctypes.data, x.size, 1, 0))
    return out


def live_accumulators(oracle_lib):
    """The reference's own callback and full_demod over mm.acc_input(): its five accumulators per block length."""
    rows = []
    for length in mm.ACC_LENGTHS:
        bufs = mm.acc_input(length)
        ref = oracle_lib.Reference()
        try:
            ref.configure(acc_cfg(length))
            cmd = CmdState.in_dll(ref.lib, "cmd")
            dongle = DongleState.in_dll(ref.lib, "dongle")
            cmd.filename = b"monitor"
            cmd.checkADCmax = cmd.checkADCrms = 1
            cmd.numMeas = mm.ACC_MEAS
            scratch = np.zeros(oracle_lib.result_cap(acc_cfg(length)) + 16, dtype=np.int16)
            for b in bufs:
                assert ref.lib.ref_block(np.ascontiguousarray(b), length, scratch) >= 0
            rows.append([float(dongle.sampleMax), dongle.samplePowSum, float(dongle.samplePowCount), cmd.levelSum,
                         float(cmd.numSummed)])
        finally:
            ref.close()
    return np.array(rows, dtype=np.float64)


def input_digest():
    import reference_record as rr
    return rr.digest(*[mm.acc_input(length) for length in mm.ACC_LENGTHS])


def test_model_accumulators_equal_the_reference(oracle_lib):
    """sampleMax / samplePowSum / samplePowCount and levelSum / numSummed, bit for bit (the doubles included): live where
    oracle/_ref is built, else the fixture tests/golden/gen_monitor_golden.py wrote from the live reference."""
    if oracle_lib.have_reference():
        want = live_accumulators(oracle_lib)
    else:
        rec = np.load(mm.GOLDEN)
        assert str(rec["inputs"]) == input_digest(), "the inputs differ from those the fixture was computed from"
        want = rec["accumulators"]
    assert want.shape == (len(mm.ACC_LENGTHS), 5)
    for length, w in zip(mm.ACC_LENGTHS, want):
        bufs = mm.acc_input(length)
        got = mm.model_accumulators(bufs, acc_levels(oracle_lib, bufs), mm.ACC_MEAS)
        assert np.array(got, dtype=np.float64).tobytes() == w.tobytes(), (length, got, list(w))
        assert got[4] == mm.ACC_MEAS and got[2] == mm.ACC_BUFFERS  # levelSum stops after M buffers, the callback does not


def test_step_and_count_of_the_lengths_in_use():
    want = {512: (2, 256), 16384: (2, 8192), 16896: (2, 8448), 32768: (4, 8192), 65536: (6, 10923), 131072: (10, 13108),
            262144: (18, 14564)}
    for length, sc in want.items():
        assert mm.step_count(length) == sc


# ------------------------------------------------------------ the C engine against the restatement ----

def c_rule(r):
    return capi.RtlfmMonitorRule.default(**r)


def rec(n, mx=127, pow_sum=1000, pow_count=10, step=2):
    a = np.zeros(n, dtype=mm.STAT_DTYPE)
    a["max"], a["pow_sum"], a["pow_count"], a["step"] = mx, pow_sum, pow_count, step
    return a


def scenarios():
    """(rule, levels, records or None) per stream.  Levels of 100 / 200 / 500 / 1000 are 40.00 / 46.02 / 53.98 / 60.00 dB:
    on both sides of 50 +- 5 dB and a decibel away from either bound."""
    ladder = [100, 100, 200, 200, 500, 500, 1000, 1000, 500, 500, 100, 100]
    out = []
    for crit in (mm.CRIT_IN, mm.CRIT_OUT, mm.CRIT_LT, mm.CRIT_GT):
        out.append((mm.rule(crit=crit, ref_level=50.0, ref_tol=5.0, num_meas=2, omit_first=0), ladder, None))
    # a negative rms() inside a cycle: skipped, the cycle gets a buffer longer
    out.append((mm.rule(crit=mm.CRIT_GT, ref_level=30.0, num_meas=3, omit_first=0),
                [100, INT32_MIN, 100, 100, 1000, -5, -5, 1000, 1000, 10, 10, 10], None))
    # omit_first (the default, 3)
    out.append((mm.rule(crit=mm.CRIT_GT, ref_level=30.0, num_meas=2), [100] * 12, None))
    # the hold-off: fires, is blocked while the counter (5, lowered by 2 per cycle) is above 0, fires again; the
    # level drops below the criterion while blocked ("does not trigger, blocks for")
    out.append((mm.rule(crit=mm.CRIT_GT, ref_level=30.0, num_meas=2, num_block_trigger=5, omit_first=0),
                [100, 100, 100, 100, 10, 10, 100, 100, 100, 100, 100, 100, 100, 100, 10, 10, 100, 100], None))
    # num_meas <= 0 is 10
    out.append((mm.rule(crit=mm.CRIT_LT, ref_level=50.0, num_meas=0, omit_first=0), [200] * 25, None))
    out.append((mm.rule(crit=mm.CRIT_LT, ref_level=50.0, num_meas=-4, omit_first=1), [700] * 25, None))
    # the ADC marks: 64 ("! ") and 120 ("!!"), one below each
    for mx in (127 + 63, 127 + 64, 127 + 119, 127 + 120, 255, 0):
        st = rec(8, mx=100, pow_sum=123457, pow_count=8192)
        st["max"][3] = mx
        st["pow_sum"] = [123457, 7, 2 ** 32 - 1, 55555, 1, 2, 3, 536870912]
        out.append((mm.rule(crit=mm.CRIT_GT, ref_level=30.0, num_meas=4, omit_first=0, check_adc_max=1, check_adc_rms=1),
                    [100] * 8, st))
    out.append((mm.rule(crit=mm.CRIT_GT, ref_level=30.0, num_meas=4, omit_first=0, check_adc_max=1), [100] * 8, rec(8, mx=200)))
    out.append((mm.rule(crit=mm.CRIT_GT, ref_level=30.0, num_meas=4, omit_first=0, check_adc_rms=1), [100] * 8, rec(8, mx=200)))
    # no statistics asked: records come, nothing is kept (adc_rms = -1, adc_max = -127) ...
    out.append((mm.rule(crit=mm.CRIT_GT, ref_level=30.0, num_meas=4, omit_first=0), [100] * 8, rec(8, mx=200)))
    # ... and asked, but no records fed
    out.append((mm.rule(crit=mm.CRIT_GT, ref_level=30.0, num_meas=4, omit_first=0, check_adc_max=1, check_adc_rms=1), [100] * 8, None))
    return out


def model_events(sc):
    models = []
    for s, (r, levels, st) in enumerate(sc):
        m = mm.StreamModel(s, r)
        m.feed(levels, st)
        models.append(m)
    return models


def test_scenarios_cover_what_they_claim():
    models = model_events(scenarios())
    ev = [e for m in models for e in m.events]
    for s in range(4):  # every criterion met and not met
        assert {e["crit_met"] for e in models[s].events} == {0, 1}, s
    assert len(models[4].events) == 3 and models[4].events[1]["level_db"] == pytest.approx(60.0)
    assert [e["cycle"] for e in models[5].events] == [3, 4, 5]
    h = models[6].events
    assert [(e["fired"], e["blocked_for"], e["crit_met"]) for e in h[:5]] == [(1, 0, 1), (0, 3, 1), (0, 1, 0), (1, 0, 1), (0, 3, 1)]
    assert any(e["fired"] for e in h[5:])
    assert len(models[7].events) == 2 and len(models[8].events) == 1
    assert [models[9 + k].events[0]["adc_max"] for k in range(6)] == [63, 64, 119, 120, 128, -27]
    assert all(e["adc_rms"] == -1.0 and e["adc_max"] == -127 for e in models[17].events + models[18].events)
    assert any(e["adc_rms"] > 0 for e in ev)
    for m in models:  # no decision hangs on a last bit: every level at least 0.01 dB from both bounds
        for e in m.events:
            for bound in (m.r["ref_level"] - m.r["ref_tol"], m.r["ref_level"] + m.r["ref_tol"]):
                assert abs(e["level_db"] - bound) > 0.01


@pytest.mark.parametrize("chunk", [1, 4, 1000])
def test_engine_equals_model(lib, chunk):
    from rtlsdr_amd.monitor import Monitor
    sc = scenarios()
    models = model_events(sc)
    with Monitor([c_rule(r) for r, _, _ in sc]) as mon:
        longest = max(len(levels) for _, levels, _ in sc)
        for at in range(0, longest, chunk):  # the streams interleaved, `chunk` buffers at a time
            for s, (_, levels, st) in enumerate(sc):
                part = levels[at:at + chunk]
                if part:
                    mon.feed(s, part, None if st is None else st[at:at + chunk])
        got = mon.poll(cap=7)
        for s, m in enumerate(models):
            mine = [e for e in got if e["stream"] == s]
            mm.assert_events_equal(mine, m.events)
            for e, w in zip(mine, m.events):
                assert mon.format_event(e) == mm.format_event(m.r, w)
            st = mon.stats(s)
            assert st["count"] == m.stat["count"] == len(m.events)
            if st["count"]:
                assert np.float32(st["min"]) == m.stat["min"] and np.float32(st["max"]) == m.stat["max"]
                assert abs(st["sum"] - m.stat["sum"]) <= 1e-12 * abs(m.stat["sum"])
        assert mon.poll() == []
        assert mon.rule(7).num_meas == 10


def test_event_lines_in_the_reference_wording(lib):
    from rtlsdr_amd.monitor import Monitor
    r = mm.rule(freq=433920000, gain=297, crit=mm.CRIT_GT, ref_level=30.0, num_meas=1, num_block_trigger=2, omit_first=0,
                check_adc_max=1, check_adc_rms=1)
    with Monitor([c_rule(r)]) as mon:
        mon.feed(0, [100, 100, 10], rec(3, mx=127 + 120, pow_sum=8192 * 50, pow_count=8192))
        lines = [mon.format_event(e) for e in mon.poll()]
    assert lines == ["433920.000 kHz: gain 29.7 + level 40.0 dB adc max 120!! rms   7.1 => activates trigger",
                     "433920.000 kHz: gain 29.7 + level 40.0 dB adc max 120!! rms   7.1 => would trigger, blocks for 1",
                     "433920.000 kHz: gain 29.7 + level 20.0 dB adc max 120!! rms   7.1 => does not trigger"]


def test_engine_rejects_bad_arguments(lib):
    m = C.c_void_p()
    r = c_rule(mm.rule())
    assert lib.rtlfm_monitor_create(0, C.byref(r), C.byref(m)) == -22
    assert lib.rtlfm_monitor_create(1, None, C.byref(m)) == -22
    bad = c_rule(mm.rule(crit=7))
    assert lib.rtlfm_monitor_create(1, C.byref(bad), C.byref(m)) == -22 and m.value is None
    assert lib.rtlfm_monitor_create(1, C.byref(r), C.byref(m)) == 0
    lv = np.zeros(4, dtype=np.int32)
    assert lib.rtlfm_monitor_feed(m, 1, lv.ctypes.data, None, 4) == -22
    assert lib.rtlfm_monitor_feed(m, 0, None, None, 4) == -22
    assert lib.rtlfm_monitor_update(m, None) == -22  # no handle: nothing to read, and it says so
    assert lib.rtlfm_monitor_destroy(m) == 0
    assert lib.rtlfm_monitor_destroy(None) == -22


# ------------------------------------------------------------------------------ the command file ----

CMD_FILE = """# level monitor
adc

  100M, 29.7, in, -20, 3.5, 4, 8, /bin/notify, !freq! !mlevel! up
433.92M , auto,==,-30,2,10,0
144800k,a,out,-31.5,1.5,5,10,  ./run.sh  ,  !crit!  !reflevel! !reftol! !gain!
1G, 0, !=, 1, 2, 3, 4
adcrms
88100000, 12.5, <>, -10, 0, 0, 4, cmd
1000, 1, lt, 5, 1, 2, 3
2000, 1, <, 5, 1, 2, 3
3000, 1, gt, 5, 1, 2, 3
4000, 1, >, 5, 1, 2, 3,
5000, 1, between, 5, 1, 2, 3
6000, 1, gt, 5, 1
7000
adcmax
8000, 2, gt
"""


def test_parse_file(lib, tmp_path, capfd):
    from rtlsdr_amd import monitor
    p = tmp_path / "cmd.csv"
    p.write_text(CMD_FILE)
    rules, amax, arms = monitor.parse_file(p)
    err = capfd.readouterr().err
    assert amax and arms
    got = [(r.freq, r.gain, r.crit, r.ref_level, r.ref_tol, r.num_meas, r.num_block_trigger, r.command.decode(), r.args.decode())
           for r in rules]
    assert got == [
        (100000000, 297, mm.CRIT_IN, -20.0, 3.5, 4, 8, "/bin/notify", "!freq! !mlevel! up"),
        (433920000, mm.AUTO_GAIN, mm.CRIT_IN, -30.0, 2.0, 10, 0, "", ""),
        (144800000, mm.AUTO_GAIN, mm.CRIT_OUT, -31.5, 1.5, 5, 10, "./run.sh", "!crit!  !reflevel! !reftol! !gain!"),
        (1000000000, 0, mm.CRIT_OUT, 1.0, 2.0, 3, 4, "", ""),
        (88100000, 125, mm.CRIT_OUT, -10.0, 0.0, 10, 4, "cmd", ""),
        (1000, 10, mm.CRIT_LT, 5.0, 1.0, 2, 3, "", ""),
        (2000, 10, mm.CRIT_LT, 5.0, 1.0, 2, 3, "", ""),
        (3000, 10, mm.CRIT_GT, 5.0, 1.0, 2, 3, "", ""),
        (4000, 10, mm.CRIT_GT, 5.0, 1.0, 2, 3, "", ""),
    ]
    assert all(r.check_adc_max == 1 and r.check_adc_rms == 1 and r.omit_first == 3 for r in rules)
    # the broken lines: skipped with the reference's messages, not fatal
    assert "warning: fixed #measurements from 0 to 10 in line 9 of command file!" in err
    assert "error parsing expr in line 14 of command file!" in err
    assert "error parsing #measurements in line 15 of command file!" in err
    assert "error parsing gain in line 16 of command file!" in err
    assert "error parsing level in line 18 of command file!" in err
    assert err.count("error parsing") == 4


def test_parse_file_errors(lib, tmp_path, capfd):
    rules = (capi.RtlfmMonitorRule * 2)()
    n = C.c_int()
    assert lib.rtlfm_monitor_parse_file(str(tmp_path / "missing").encode(), rules, 2, C.byref(n), None, None) == -2  # -ENOENT
    p = tmp_path / "empty.csv"
    p.write_text("# nothing\n\nadc\n")
    assert lib.rtlfm_monitor_parse_file(str(p).encode(), rules, 2, C.byref(n), None, None) == -61  # -ENODATA
    assert "does not contain any valid lines" in capfd.readouterr().err
    p = tmp_path / "three.csv"
    p.write_text("1k,1,gt,1,1,1,1\n2k,1,gt,1,1,1,1\n3k,1,gt,1,1,1,1\n")
    assert lib.rtlfm_monitor_parse_file(str(p).encode(), rules, 2, C.byref(n), None, None) == -105  # -ENOBUFS
    assert n.value == 3 and rules[1].freq == 2000


# ------------------------------------------------------------------------------------ the symbols ----

def test_new_symbols_are_exported_and_fail_loudly(lib):
    import re
    text = open(os.path.join(ROOT, "include", "rtlfm_monitor.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(rtlfm_monitor_[a-z_0-9]+)\s*\(", text)))
    assert declared == sorted(capi.DECLARED_MONITOR_SYMBOLS) and len(declared) >= 8
    for name in declared + ["rtlfm_gpu_input_stats", "rtlfm_gpu_input_stats_all", "rtlfm_gpu_input_stats_device", "rtlfm_gpu_levels_all"]:
        assert hasattr(lib, name), name
    out = (capi.RtlfmInputStat * 4)()
    n = C.c_int()
    assert lib.rtlfm_gpu_input_stats(None, 0, out, 4, C.byref(n)) == -22     # no handle: -EINVAL, no fallback
    assert lib.rtlfm_gpu_input_stats_all(None, out, 4, C.byref(n)) == -22
    assert lib.rtlfm_gpu_levels_all(None, out, 4, C.byref(n)) == -22
    assert lib.rtlfm_gpu_input_stats_device(0, None, 16384, 16384, 1, 1, out, 1, None) == -22
    import torch
    if not torch.cuda.is_available():
        assert lib.rtlfm_gpu_input_stats_device(0, 4096, 16384, 16384, 1, 1, out, 1, None) == -19  # -ENODEV: no CPU fallback


def test_struct_layouts(lib, tmp_path):
    """rtlfm_cfg and rtlfm_stream_state keep their sizes (oracle/pyoracle.py mirrors them); the new structs are laid out
    as the C compiler lays them out."""
    src = ('#include <stdio.h>\n#include "rtlfm_monitor.h"\n'
           'int main(){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(rtlfm_cfg), sizeof(rtlfm_stream_state), sizeof(rtlfm_input_stat),'
           ' sizeof(rtlfm_monitor_rule), sizeof(rtlfm_monitor_event), sizeof(rtlfm_monitor_stat));return 0;}\n')
    p = tmp_path / "s.c"
    p.write_text(src)
    exe = str(tmp_path / "s")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(p), "-o", exe])
    sizes = list(map(int, subprocess.check_output([exe]).split()))
    assert sizes[:2] == [84, 328]
    assert sizes == [C.sizeof(t) for t in (capi.RtlfmCfg, capi.RtlfmStreamState, capi.RtlfmInputStat, capi.RtlfmMonitorRule,
                                           capi.RtlfmMonitorEvent, capi.RtlfmMonitorStat)]
    assert np.dtype(capi.INPUT_STAT_DTYPE).itemsize == C.sizeof(capi.RtlfmInputStat) == 16
