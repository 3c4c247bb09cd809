"""rtl_fm_hip -S: scanning for -N sources.  Every output file must be what the model of tests/scan_model.py - the reference's
demod-thread rule and mute around the oracle, with the hop engine's bookkeeping - gives for that source alone; the hop
lines and the exit counts are the model's events."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import scan_model as sm
from rtlsdr_amd import build as hipbuild
from rtlsdr_amd.capi import ATAN_FAST, RtlfmCfg

pytestmark = pytest.mark.gpu

L, LEVEL, CONSEQ = 16384, 500, 1
ARGV = ["-M", "fm", "-s", "24k", "-A", "fast", "-l", str(LEVEL), "-t", str(CONSEQ), "-v"]
#          source 0: closes long enough to hop twice (the buffer behind a hop asks for nothing: settle = 1), then stays open
PATTERNS = ["LLqqqqLLLLLLLLLLLLLLLLLL",
            "LLLLLLLLLLLLLLLLLLLLLLLL",    # never closes: a list of two and no hop
            "LLqqqqqqLLLLqqqqqLLLLLLL"]    # closes, and is held: a list of one never hops
LISTS = ["100M 101M 102M", "433.92M:434M:80k", "144.8M"]


def plan(po):
    cfg = RtlfmCfg.default(custom_atan=ATAN_FAST, rate_out=24000, squelch_level=LEVEL, block_len=L)
    cf, cr = C.c_uint32(), C.c_uint32()
    po.oracle().orc_optimal_settings(C.byref(cfg), 100000000, 24000, 1000000, 0, 0, C.byref(cf), C.byref(cr))
    return cfg


def source(pattern, seed):
    rng = np.random.default_rng(seed)
    return [sm.tone_or_noise(rng, L, c == "L") for c in pattern]


def model(po, cfg, bufs, freqs, stream):
    """One buffer per run (the tool's -l rule), settle = 1; returns (pcm, events, engine state)."""
    st, eng = sm.StreamModel(po, cfg, CONSEQ), sm.EngineModel(stream, freqs, settle=1)
    out = []
    for b in bufs:
        pcm, recs = st.run([b])
        out.append(pcm)
        if eng.feed(recs):
            st.mute = sm.DEFAULT_DUMP
    return np.concatenate(out), eng.events, eng.state()


def run_cli(tmp_path, sources, argv, env_extra=None):
    _, cli = hipbuild.build_host()
    env = {k: v for k, v in os.environ.items() if k not in ("RTLSDR_FILE", "RTLSDR_FILE_LIST")}
    if sources is not None:
        lst = tmp_path / "sources.txt"
        lst.write_text("\n".join(str(s) for s in sources) + "\n")
        env["RTLSDR_FILE_LIST"] = str(lst)
    env.update(env_extra or {})
    return subprocess.run([cli] + argv, env=env, capture_output=True, text=True, timeout=300)


def parse_lists():
    from rtlsdr_amd.scan import parse_list
    return [parse_list(t) for t in LISTS]


def test_three_sources(oracle_lib, tmp_path):
    cfg = plan(oracle_lib)
    freqs = parse_lists()
    assert [len(f) for f in freqs] == [3, 2, 1]
    bufs = [source(p, 40 + i) for i, p in enumerate(PATTERNS)]
    want = [model(oracle_lib, cfg, bufs[i], freqs[i], i) for i in range(3)]
    assert [w[2]["hops"] for w in want] == [2, 0, 0] and want[2][2]["held"] > 0 and want[1][2]["held"] == 0
    srcs = []
    for i in range(3):
        p = tmp_path / f"src{i}.bin"
        np.concatenate(bufs[i]).tofile(p)
        srcs.append(p)
    scan = tmp_path / "lists.txt"
    scan.write_text("# one list per source\n" + LISTS[0] + "\n\n" + LISTS[1] + "\n  # indented comment\n" + LISTS[2] + "\n")
    r = run_cli(tmp_path, srcs, ["-N", "3", "-S", str(scan)] + ARGV + [str(tmp_path / "out_%d.raw")])
    assert r.returncode == 0, r.stderr[-2000:]
    for i in range(3):
        got = np.fromfile(tmp_path / f"out_{i}.raw", dtype=np.int16)
        assert got.size == want[i][0].size and np.array_equal(got, want[i][0]), i
    hops = re.findall(r"^stream (\d+): hop (\d+) -> (\d+) at buffer (\d+)$", r.stderr, flags=re.M)
    want_hops = []
    for i in range(3):
        f_now = freqs[i][0]
        for e in want[i][1]:
            want_hops.append((str(i), str(f_now), str(e["freq"]), str(e["buffer_serial"])))
            f_now = e["freq"]
    assert hops == want_hops and len(hops) == 2
    for i in range(3):
        st = want[i][2]
        assert f"stream {i}: {st['hops']} hops, {st['held']} buffers held, last on {st['freq']} Hz" in r.stderr
    held = sum(w[2]["held"] for w in want)
    assert f"{held} buffers held back by the squelch" in r.stderr


def test_one_source(oracle_lib, tmp_path):
    cfg = plan(oracle_lib)
    freqs = parse_lists()[0]
    bufs = source(PATTERNS[0], 7)
    pcm, events, st = model(oracle_lib, cfg, bufs, freqs, 0)
    src = tmp_path / "one.bin"
    np.concatenate(bufs).tofile(src)
    scan = tmp_path / "list.txt"
    scan.write_text(LISTS[0] + "\n")
    out = tmp_path / "one.raw"
    r = run_cli(tmp_path, None, ["-S", str(scan)] + ARGV + [str(out)], {"RTLSDR_FILE": str(src)})
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(np.fromfile(out, dtype=np.int16), pcm)
    assert len(re.findall(r"^stream 0: hop ", r.stderr, flags=re.M)) == len(events) == 2
    assert f"stream 0: 2 hops, {st['held']} buffers held, last on {st['freq']} Hz" in r.stderr


def test_refusals_before_a_device_is_opened(tmp_path):
    """No device exists here (neither RTLSDR_FILE nor RTLSDR_FILE_LIST): what is refused must be refused for its own reason."""
    scan = tmp_path / "lists.txt"
    scan.write_text("100M 101M\n102M\n")
    cmd = tmp_path / "cmd.csv"
    cmd.write_text("100M, 0, gt, -30, 1, 10, 0, ,\n101M, 0, gt, -30, 1, 10, 0, ,\n")
    out = str(tmp_path / "o_%d.raw")
    r = run_cli(tmp_path, None, ["-N", "2", "-S", str(scan), "-M", "fm", out])
    assert r.returncode != 0 and "squelch level" in r.stderr and "No supported devices" not in r.stderr
    r = run_cli(tmp_path, None, ["-N", "2", "-S", str(scan), "-l", "50", "-C", str(cmd), out])
    assert r.returncode != 0 and "exclude each other" in r.stderr and "No supported devices" not in r.stderr
    r = run_cli(tmp_path, None, ["-N", "3", "-S", str(scan), "-l", "50", out])
    assert r.returncode != 0 and "holds 2 lists" in r.stderr and "No supported devices" not in r.stderr
    bad = tmp_path / "bad.txt"
    bad.write_text("100M\n1:2\n")
    r = run_cli(tmp_path, None, ["-N", "2", "-S", str(bad), "-l", "50", out])
    assert r.returncode != 0 and "line 2 is no frequency list" in r.stderr
    assert not list(tmp_path.glob("o_*.raw"))
