"""The input-health engine (rtlfm_agc_*, host code inside librtlfm_hip.so) through ctypes against the restatement of
tests/health_model.py: index sequences, clamping, the thresholds' boundaries, settle, event order, ragged lengths,
continuity across buffers, totals and error codes.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import health_model as hm
from rtlsdr_amd import build as hipbuild
from rtlsdr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 16384


@pytest.fixture(scope="module")
def lib():
    hipbuild.build()
    return capi.load()


def agc(*a, **k):
    from rtlsdr_amd.agc import SoftAgc
    return SoftAgc(*a, **k)


def rec(overload=0, high=0, lost=0, first=0, last=255, n=1):
    r = np.zeros(n, dtype=hm.HEALTH_DTYPE)
    r["overload"], r["high"], r["lost"], r["first"], r["last"] = overload, high, lost, first, last
    return r


LOUD, QUIET, MID = rec(overload=100, high=5000), rec(), rec(high=5000)  # MID: neither overloaded nor low: no change


def run_both(lib, streams, gain_counts, settle=0, enable=None):
    """streams[s] = list of (records, lens) feeds; returns the engine's and the model's (events, states)."""
    S = len(streams)
    models = [hm.StreamModel(s, gain_counts[s], enabled=True if enable is None else bool(enable[s]), settle=settle) for s in range(S)]
    with agc(gain_counts, enable) as a:
        a.set_settle(settle)
        rounds = max(len(f) for f in streams)
        for k in range(rounds):  # interleaved like runs: every stream's k-th feed, then the next
            for s in range(S):
                if k < len(streams[s]):
                    r, ln = streams[s][k]
                    a.feed(s, r, ln)
                    models[s].feed(r, ln)
        got_ev = a.poll(cap=7)  # a small cap: poll loops
        got_st = [a.state(s) for s in range(S)]
        assert a.poll() == []
    return got_ev, got_st, models


def test_capi_matches_header(lib):
    text = open(os.path.join(ROOT, "include", "rtlfm_agc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(rtlfm_agc_[a-z_0-9]+)\s*\(", text)))
    assert declared == sorted(capi.DECLARED_AGC_SYMBOLS) and len(declared) == 8
    for name in declared:
        assert hasattr(lib, name)
    assert C.sizeof(capi.RtlfmInputHealth) == 16 == np.dtype(capi.INPUT_HEALTH_DTYPE).itemsize
    assert np.dtype(capi.INPUT_HEALTH_DTYPE) == np.dtype(hm.HEALTH_DTYPE)
    assert C.sizeof(capi.RtlfmAgcEvent) == 24


def test_struct_sizes_match_header():
    import subprocess
    import tempfile
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "rtlfm_agc.h"\n'
           'int main(){printf("%zu %zu %zu %zu\\n", sizeof(rtlfm_input_health), offsetof(rtlfm_input_health, first), '
           'sizeof(rtlfm_agc_event), offsetof(rtlfm_agc_event, buffer_serial));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "s.c")
        open(p, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), p, "-o", exe])
        assert subprocess.check_output([exe]).split() == [b"16", b"12", b"24", b"16"]


@pytest.mark.parametrize("settle", [0, 1, 3])
def test_index_sequences_against_model(lib, settle):
    rng = np.random.default_rng(5 + settle)
    mixed = [(np.concatenate([(LOUD, QUIET, MID)[int(k)] for k in rng.integers(0, 3, 4)]), L) for _ in range(12)]
    streams = [[(np.concatenate([LOUD] * 4), L)] * 5, [(np.concatenate([QUIET] * 4), L)] * 5, mixed,
               [(np.concatenate([QUIET] * 3 + [LOUD] * 3), L)] * 6]
    ev, st, models = run_both(lib, streams, [29, 5, 29, 4], settle=settle)
    for s, m in enumerate(models):
        assert [e for e in ev if e["stream"] == s] == m.events, s  # every stream's events in its own order
        assert st[s] == m.state(), s
    assert st[0]["index"] == 0 and not [e for e in ev if e["stream"] == 0]        # loud from index 0: clamped, no event
    assert st[1]["index"] == 4                                                     # quiet: up to gain_count - 1 and no further
    if settle == 0:
        assert [e["new_index"] for e in ev if e["stream"] == 1] == [1, 2, 3, 4]
        assert [e["buffer_serial"] for e in ev if e["stream"] == 1] == [0, 1, 2, 3]
    else:
        assert [e["buffer_serial"] for e in ev if e["stream"] == 1] == [k * (settle + 1) for k in range(4)]


def test_clamping_and_single_gain(lib):
    ev, st, models = run_both(lib, [[(np.concatenate([QUIET] * 6 + [LOUD] * 6), L)], [(np.concatenate([QUIET, LOUD, QUIET]), L)]], [3, 1])
    assert [(e["old_index"], e["new_index"], e["overloaded"]) for e in ev if e["stream"] == 0] == [(0, 1, 0), (1, 2, 0), (2, 1, 1), (1, 0, 1)]
    assert not [e for e in ev if e["stream"] == 1] and st[1]["index"] == 0  # gain_count == 1: nowhere to go
    assert st[0] == models[0].state() and st[1]["overloaded"] == 0


@pytest.mark.parametrize("ln", [8000, 16000, 262144 // 512 * 512])
def test_threshold_boundaries(lib, ln):
    """8000 * n == len, len - 1, len + 1 for the overload test (>=) and the level test (<=)."""
    n = ln // 8000
    assert 8000 * n <= ln
    # lengths chosen around 8000 * n: exactly, one more, one less
    for length, over_expect, up_expect in ((8000 * n, True, True), (8000 * n + 1, False, True), (8000 * n - 1, True, False)):
        with agc([9]) as a:  # overload count n, no high bytes beside them
            a.set_index(0, 4)
            a.feed(0, rec(overload=n, high=8000), length)
            assert a.state(0)["overloaded"] == int(over_expect)
            assert a.state(0)["index"] == (3 if over_expect else 4)  # high is far above: no step up
        with agc([9]) as a:  # high count n, nothing overloads
            a.set_index(0, 4)
            a.feed(0, rec(overload=0, high=n), length)
            assert a.state(0)["index"] == (5 if up_expect else 4)
        m = hm.StreamModel(0, 9)
        m.index = 4
        m.feed(rec(overload=n, high=8000), length)
        assert m.overloaded == int(over_expect)


def test_ragged_lengths(lib):
    """The same record decides differently under another length; totals add each buffer's own length."""
    r = rec(overload=1, high=1, n=4)
    lens = np.array([512, 8192, 7999, 8000], dtype=np.uint32)  # 8000 >= len for the first, third and fourth
    ev, st, models = run_both(lib, [[(r, lens)]], [9])
    assert st[0] == models[0].state() and ev == models[0].events
    assert st[0]["total_samples"] == int(lens.sum())
    with agc([9]) as a:
        a.set_index(0, 5)
        a.feed(0, r, lens)
        assert [(e["old_index"], e["new_index"]) for e in a.poll()] == [(5, 4), (4, 5), (5, 4), (4, 3)]


def test_continuity_from_200(lib):
    """A first buffer that starts at byte 200 and goes on 201, 202, ...: nothing lost, over several buffers."""
    seq = hm.counter((1, 4 * L), start=200)[0]
    recs = hm.records(seq.reshape(4, L))
    assert int(recs["first"][0]) == 200 and not recs["lost"].any()
    with agc([9], enable=[0]) as a:
        a.feed(0, recs[:1], L)
        a.feed(0, recs[1:], L)
        # (a counter passes through 0 and 255 once per 256 bytes: detect_overload's verdict on it is "overloaded")
        assert a.state(0) == {"index": 0, "overloaded": 1, "total_samples": 4 * L, "dropped_samples": 0}
        assert a.poll() == []  # not enabled: no AGC decision


def test_gap_at_a_buffer_boundary(lib):
    seq = hm.counter((1, 2 * 512), start=0)[0].copy()
    seq[512:] = (seq[512:].astype(np.int32) + 5) & 0xFF
    recs = hm.records(seq.reshape(2, 512))
    assert not recs["lost"].any()  # no record sees it
    ref = hm.Underrun()
    want = [ref.call(seq[:512]), ref.call(seq[512:])]
    assert want == [0, 5]
    with agc([9]) as a:
        a.feed(0, recs, 512)
        assert a.state(0)["dropped_samples"] == 5 and a.state(0)["total_samples"] == 1024


def test_totals_on_random_bytes(lib):
    from rtlsdr_amd import synth
    seq = synth.random_u8(1, 6 * 512, seed=9)[0]
    ref = hm.Underrun()
    for b in seq.reshape(6, 512):
        ref.call(b)
    with agc([9]) as a:
        a.feed(0, hm.records(seq.reshape(6, 512)), 512)
        st = a.state(0)
    assert (st["total_samples"], st["dropped_samples"]) == (ref.total_samples, ref.dropped_samples)


def test_error_codes(lib):
    a = C.c_void_p()
    gc = (C.c_int32 * 2)(5, 0)
    assert lib.rtlfm_agc_create(0, gc, None, C.byref(a)) == -22
    assert lib.rtlfm_agc_create(2, gc, None, C.byref(a)) == -22 and a.value is None  # a gain table without entries
    assert lib.rtlfm_agc_create(1, None, None, C.byref(a)) == -22
    assert lib.rtlfm_agc_create(1, gc, None, C.byref(a)) == 0
    r = rec()
    ln = (C.c_uint32 * 1)(512)
    zero = (C.c_uint32 * 1)(0)
    assert lib.rtlfm_agc_feed(a, 1, r.ctypes.data, ln, 1) == -22
    assert lib.rtlfm_agc_feed(a, -1, r.ctypes.data, ln, 1) == -22
    assert lib.rtlfm_agc_feed(a, 0, r.ctypes.data, zero, 1) == -22
    assert lib.rtlfm_agc_feed(a, 0, None, ln, 1) == -22
    assert lib.rtlfm_agc_feed(a, 0, None, None, 0) == 0
    assert lib.rtlfm_agc_set_index(a, 0, 5) == -22 and lib.rtlfm_agc_set_index(a, 0, -1) == -22
    assert lib.rtlfm_agc_set_index(a, 0, 4) == 0
    assert lib.rtlfm_agc_set_settle(a, -1) == -22
    assert lib.rtlfm_agc_update(a, None) == -22 and lib.rtlfm_agc_update(None, None) == -22
    assert lib.rtlfm_agc_state(a, 1, None, None, None, None) == -22
    idx = C.c_int32()
    assert lib.rtlfm_agc_state(a, 0, C.byref(idx), None, None, None) == 0 and idx.value == 4
    n = C.c_int()
    assert lib.rtlfm_agc_poll(a, None, 1, C.byref(n)) == -22
    assert lib.rtlfm_agc_destroy(a) == 0 and lib.rtlfm_agc_destroy(None) == -22
