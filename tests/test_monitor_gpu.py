"""The level monitor end to end on the GPU: 64 keyed carriers, the levels from the front end (rtlfm_gpu_levels), the ADC
statistics from k_input_stats, Monitor.update() after every run - against the restatement of tests/monitor_model.py fed
with the oracle's rms() levels and its own records."""
import ctypes as C

import numpy as np
import pytest

import monitor_model as mm
from cases import make_cfg
from rtlsdr_amd import capi, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

S, NB, L, RUN = 64, 40, 16384, 4
OV = dict(downsample=16, downsample_passes=4, rate_out=150000)
CLIPPING = (5, 41)


def keyed_streams():
    """Every stream's carrier keyed on and off buffer by buffer with a pattern of its own (silent buffers keep one LSB of
    noise); two streams driven into clipping."""
    iq = np.empty((S, NB * L), dtype=np.uint8)
    for s in range(S):
        amp = 200.0 if s in CLIPPING else 20.0 + s % 7 * 5
        loud = synth.fm_iq_u8(1, NB * L // 2, amplitude=amp, first_stream=s, seed=4242)[0]
        quiet = synth.fm_iq_u8(1, NB * L // 2, amplitude=0.0, noise_lsb=1, first_stream=s, seed=777)[0]
        period, on = 6 + s % 5, 3 + s % 3
        for b in range(NB):
            src = loud if (b + s) % period < on else quiet
            iq[s, b * L:(b + 1) * L] = src[b * L:(b + 1) * L]
    return iq


def rules():
    out = []
    for s in range(S):
        out.append(mm.rule(freq=100000000 + 25000 * s, gain=(mm.AUTO_GAIN if s % 3 == 0 else 10 * (s % 40)),
                           crit=(mm.CRIT_GT, mm.CRIT_GT, mm.CRIT_GT, mm.CRIT_LT, mm.CRIT_IN, mm.CRIT_OUT)[s % 6],
                           ref_level=50.0, ref_tol=(0.0 if s % 6 < 4 else 15.0), num_meas=(2, 3, 4, 1)[s % 4],
                           num_block_trigger=(5, 0, 9)[s % 3], check_adc_max=1, check_adc_rms=int(s % 5 != 0), omit_first=s % 3))
    return out


def oracle_levels(oracle_lib, iq):
    lib = oracle_lib.oracle()
    raw_cfg = make_cfg(dict(OV, mode=capi.MODE_RAW), L, 1)
    want = np.zeros((S, NB), dtype=np.int64)
    for s in range(S):
        st = oracle_lib.new_states(1)[0]
        scratch = np.zeros(2 * L + 64, dtype=np.int16)
        for b in range(NB):
            k = lib.orc_block(C.byref(raw_cfg), C.byref(st), np.ascontiguousarray(iq[s, b * L:(b + 1) * L]), L, scratch)
            want[s, b] = lib.orc_rms(scratch.ctypes.data, k, 1, 0)
    return want


def test_monitor_follows_64_keyed_streams(oracle_lib):
    from rtlsdr_amd.demod import GpuDemod
    from rtlsdr_amd.monitor import Monitor
    iq = keyed_streams()
    rs = rules()
    levels = oracle_levels(oracle_lib, iq)
    records = mm.records(iq.reshape(S, NB, L))
    models = []
    for s in range(S):
        m = mm.StreamModel(s, rs[s])
        m.feed(levels[s], records[s])
        models.append(m)
    # the model alone: the keying yields fired, blocked and silent cycles on at least 8 streams each, both clipping
    # streams are marked, and no decision hangs on a last bit
    fired = sum(any(e["fired"] for e in m.events) for m in models)
    blocked = sum(any(e["blocked_for"] > 0 for e in m.events) for m in models)
    silent = sum(any(not e["fired"] and not e["blocked_for"] for e in m.events) for m in models)
    assert fired >= 8 and blocked >= 8 and silent >= 8, (fired, blocked, silent)
    for s in CLIPPING:
        assert any(e["adc_max"] >= 120 for e in models[s].events)
    assert sum(any(e["adc_max"] >= 64 for e in m.events) for m in models) < S
    for m in models:
        for e in m.events:
            for bound in (m.r["ref_level"] - m.r["ref_tol"], m.r["ref_level"] + m.r["ref_tol"]):
                assert abs(e["level_db"] - bound) > 0.01, (m.stream, e)

    cfg = make_cfg(dict(OV, report_levels=1), L, RUN)
    d = torch.from_numpy(iq).cuda()
    got = []
    with GpuDemod(cfg, S, 0, options={"input_stats": 1}) as g, Monitor([capi.RtlfmMonitorRule.default(**r) for r in rs]) as mon:
        for r in range(NB // RUN):
            g.run_torch(d[:, r * RUN * L:(r + 1) * RUN * L].contiguous())
            mon.update(g)
            got += mon.poll()
        assert mon.poll() == []
        for s, m in enumerate(models):
            mm.assert_events_equal([e for e in got if e["stream"] == s], m.events)
            st = mon.stats(s)
            assert st["count"] == m.stat["count"]
            if st["count"]:
                assert np.float32(st["min"]) == m.stat["min"] and np.float32(st["max"]) == m.stat["max"]
    assert len(got) == sum(len(m.events) for m in models) > 10 * S


def test_update_needs_levels_and_the_same_streams():
    from rtlsdr_amd.capi import RtlfmError
    from rtlsdr_amd.demod import GpuDemod
    from rtlsdr_amd.monitor import Monitor
    iq = torch.from_numpy(synth.fm_iq_u8(3, 2 * L // 2)).cuda()
    rule = capi.RtlfmMonitorRule.default(crit=capi.CRIT_GT, ref_level=30.0, num_meas=1, omit_first=0, check_adc_max=1, check_adc_rms=1)
    with GpuDemod(make_cfg(OV, L, 2), 3, 0) as g, Monitor([rule] * 3) as mon:
        g.run_torch(iq)
        with pytest.raises(RtlfmError) as e:
            mon.update(g)
        assert e.value.code == -61  # -ENODATA: the handle keeps no levels
    with GpuDemod(make_cfg(dict(OV, report_levels=1), L, 2), 3, 0) as g:
        g.run_torch(iq)
        for n in (2, 4):
            with Monitor([rule] * n) as mon, pytest.raises(RtlfmError) as e:
                mon.update(g)
            assert e.value.code == -22
        with Monitor([rule] * 3) as mon:  # without the option input_stats: levels only
            mon.update(g)
            ev = mon.poll()
            assert len(ev) == 6 and all(e["adc_max"] == -127 and e["adc_rms"] == -1.0 for e in ev)
