"""The scanner's hop engine (rtlfm_scan_*, host code inside librtlfm_hip.so) through ctypes against the restatement of
tests/scan_model.py: hops, settle, lists of one, event order, counters; the list grammar; the exported symbols and their
Python mirrors; the header as C.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import scan_model as sm
from rtlsdr_amd import build as hipbuild
from rtlsdr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOBUFS, E2BIG = -22, -105, -7


@pytest.fixture(scope="module")
def lib():
    hipbuild.build()
    return capi.load()


def recs(emits):
    r = np.zeros(len(emits), dtype=capi.GATE_REC_DTYPE)
    r["emit"] = emits
    r["hits_after"] = [0 if e else 11 for e in emits]
    return r


@pytest.mark.parametrize("settle", [0, 2])
def test_engine_against_model(lib, settle):
    """7 streams, lists of length 1, 2 and 5, seeded random gate records in runs of 1 .. 6 buffers."""
    from rtlsdr_amd.scan import Scanner
    rng = np.random.default_rng(100 + settle)
    S = 7
    lists = [[100_000_000], [101_000_000, 102_000_000], list(range(144_000_000, 144_000_005)), [5], [6, 7],
             [10, 20, 30, 40, 50], [433_920_000, 868_000_000]]
    models = [sm.EngineModel(s, lists[s], settle) for s in range(S)]
    with Scanner(S, 4096, settle) as sc:
        for s in range(S):
            sc.set_list(s, lists[s])
        want_hopped = []
        for run in range(40):
            n = int(rng.integers(1, 7))
            hopped = []
            for s in range(S):
                p_emit = (1.0, 0.0, 0.5, 0.3, 0.8, 0.6, 0.95)[s]
                r = recs((rng.random(n) < p_emit).astype(np.uint8))
                sc.feed(s, r)
                if models[s].feed(r):
                    hopped.append(s)
            assert sc.take_hopped() == hopped, run
            assert sc.take_hopped() == []
            want_hopped += hopped
        got = sc.events(cap=5)  # a small cap: the call loops
        assert sc.events() == []
        for s in range(S):
            assert [e for e in got if e["stream"] == s] == models[s].events, s
            assert sc.freq(s) == models[s].state(), s
        # every stream's events in run order: the engine queues them as the feeds come
        assert [e["stream"] for e in got] == want_hopped
    assert not models[0].events and not models[3].events           # nothing held / a list of one never hops
    assert models[3].held > 0 and models[1].hops > 0 and models[5].hops > 5
    assert models[1].held == models[1].serial                       # everything held is still counted


def test_one_hop_per_run_and_settle(lib):
    from rtlsdr_amd.scan import Scanner
    with Scanner(1, 4096, 0) as sc:
        sc.set_list(0, [1, 2, 3])
        sc.feed(0, recs([1, 0, 0, 0]))  # three held buffers in one run: one hop, asked by the first of them
        sc.feed(0, recs([0]))
        sc.feed(0, recs([1, 1]))
        sc.feed(0, recs([1, 0]))
        ev = sc.events()
        assert [(e["from_index"], e["to_index"], e["freq"], e["buffer_serial"]) for e in ev] == [(0, 1, 2, 1), (1, 2, 3, 4), (2, 0, 1, 8)]
    with Scanner(1, 4096, 2) as sc:
        sc.set_list(0, [1, 2])
        sc.feed(0, recs([0]))            # hop; the next two buffers ask for nothing
        sc.feed(0, recs([0, 0, 0]))      # ... the third does
        sc.feed(0, recs([0]))            # settle again
        assert [e["buffer_serial"] for e in sc.events()] == [0, 3]
        assert sc.freq(0) == {"freq": 1, "index": 0, "hops": 2, "buffers": 5, "held": 5}


def test_errors(lib):
    a = C.c_void_p()
    assert lib.rtlfm_scan_create(0, 4096, 0, C.byref(a)) == EINVAL
    assert lib.rtlfm_scan_create(2, 4096, -1, C.byref(a)) == EINVAL and not a.value
    assert lib.rtlfm_scan_create(2, 4096, 0, C.byref(a)) == 0
    f = np.array([1, 2], dtype=np.uint32)
    assert lib.rtlfm_scan_set_list(a, 2, f.ctypes.data, 2) == EINVAL
    assert lib.rtlfm_scan_set_list(a, 0, f.ctypes.data, 0) == EINVAL
    assert lib.rtlfm_scan_feed(a, -1, None, 0) == EINVAL
    assert lib.rtlfm_scan_feed(a, 0, None, 1) == EINVAL
    assert lib.rtlfm_scan_feed(a, 1, None, 0) == 0
    r = recs([0])
    assert lib.rtlfm_scan_feed(a, 1, r.ctypes.data, 1) == 0  # a stream without a list: counted, no hop
    n = C.c_int()
    assert lib.rtlfm_scan_take_hopped(a, None, 0, C.byref(n)) == 0 and n.value == 0
    assert lib.rtlfm_scan_update(a, None) == EINVAL and lib.rtlfm_scan_apply(a, None) == EINVAL
    assert lib.rtlfm_scan_destroy(a) == 0 and lib.rtlfm_scan_destroy(None) == EINVAL


@pytest.mark.parametrize("text,want", [
    ("100M", [100_000_000]),
    ("144.5M 433920k\t868M,1.2G", [144_500_000, 433_920_000, 868_000_000, 1_200_000_000]),
    ("88M:90M:1M", [88_000_000, 89_000_000, 90_000_000]),
    ("100k:105k:2k 7", [100_000, 102_000, 104_000, 7]),       # the last step beyond b is not taken
    ("5:5:1", [5]),
    ("1e3 2.5k 3999.9", [1000, 2500, 3999]),                    # cut to an integer, as (uint32_t)atofs()
    ("  162.400M:162.550M:25k \n", [162_400_000 + 25_000 * i for i in range(7)]),
    ("4294967295", [4294967295]),
])
def test_parse_list(lib, text, want):
    from rtlsdr_amd.scan import parse_list
    assert parse_list(text) == want
    n = C.c_int()
    assert lib.rtlfm_scan_parse_list(text.encode(), None, 0, C.byref(n)) == ENOBUFS and n.value == len(want)
    out = np.zeros(len(want) + 2, dtype=np.uint32)
    assert lib.rtlfm_scan_parse_list(text.encode(), out.ctypes.data, out.size, C.byref(n)) == 0 and n.value == len(want)
    if len(want) > 1:  # too small: nothing beyond cap is written
        out[:] = 77
        assert lib.rtlfm_scan_parse_list(text.encode(), out.ctypes.data, 1, C.byref(n)) == ENOBUFS
        assert out[0] == want[0] and (out[1:] == 77).all()


@pytest.mark.parametrize("text", ["", "   ", "abc", "100M:", "1:2", "1:2:3:4", "3:1:1", "1:9:0", "1:9:-1", "1::2", ":1:2", "M", "12q",
                                  "0x10", "nan", "inf", "-5", "5G", "1 2 x", "1:5G:1", "1k:2k:"])
def test_parse_list_malformed(lib, text):
    n = C.c_int(5)
    out = np.zeros(16, dtype=np.uint32)
    assert lib.rtlfm_scan_parse_list(text.encode(), out.ctypes.data, 16, C.byref(n)) == EINVAL
    assert n.value == 0


def test_parse_list_too_many(lib):
    n = C.c_int()
    assert lib.rtlfm_scan_parse_list(b"0:4G:1", None, 0, C.byref(n)) == E2BIG
    assert lib.rtlfm_scan_parse_list(None, None, 0, C.byref(n)) == EINVAL


def test_capi_matches_header(lib):
    text = open(os.path.join(ROOT, "include", "rtlfm_scan.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(rtlfm_scan_[a-z_0-9]+)\s*\(", text)))
    assert declared == sorted(capi.DECLARED_SCAN_SYMBOLS) and len(declared) == 10
    for name in declared + ["rtlfm_gpu_gate", "rtlfm_gpu_gate_all", "rtlfm_gpu_mute", "rtlfm_gpu_mute_device"]:
        assert hasattr(lib, name), name
    for name in ("rtlfm_gpu_gate", "rtlfm_gpu_gate_all", "rtlfm_gpu_mute", "rtlfm_gpu_mute_device"):
        assert name in capi.DECLARED_FM_SYMBOLS
    assert C.sizeof(capi.RtlfmGateRec) == 8 == np.dtype(capi.GATE_REC_DTYPE).itemsize
    assert np.dtype(capi.GATE_REC_DTYPE) == np.dtype(sm.GATE_DTYPE)
    assert C.sizeof(capi.RtlfmScanEvent) == 32
    from rtlsdr_amd.demod import GpuDemod
    for name in ("mute", "gate"):
        assert callable(getattr(GpuDemod, name))


def test_header_compiles_as_c_and_struct_sizes():
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "rtlfm_scan.h"\n'
           'int main(void){printf("%zu %zu %zu %zu %u\\n", sizeof(rtlfm_gate_rec), offsetof(rtlfm_gate_rec, emit), '
           'sizeof(rtlfm_scan_event), offsetof(rtlfm_scan_event, buffer_serial), RTLFM_SCAN_DEFAULT_DUMP);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "s.c")
        open(p, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), p, "-o", exe])
        assert subprocess.check_output([exe]).split() == [b"8", b"4", b"32", b"24", b"4096"]


def test_options_without_gpu(lib):
    """The gate and the mute need a handle: without one they say -EINVAL, not a crash."""
    n = C.c_int()
    assert lib.rtlfm_gpu_gate(None, 0, None, 0, C.byref(n)) == EINVAL
    assert lib.rtlfm_gpu_gate_all(None, None, 0, C.byref(n)) == EINVAL
    assert lib.rtlfm_gpu_mute(None, 0, 16) == EINVAL
    assert lib.rtlfm_gpu_mute_device(0, None, 0, 1, 16, None, None) == EINVAL
    assert b"squelch_gate" in lib.rtlfm_gpu_strerror(-95) and b"rtlfm_gpu_mute" in lib.rtlfm_gpu_strerror(-16)
