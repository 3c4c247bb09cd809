"""rtl_fm_hip -N n -C file: line i of the command file watched by source i.  stderr's event lines against the restatement
of tests/monitor_model.py fed with the oracle's rms() levels; the triggered command really runs, with its placeholders
replaced; a file with the wrong number of lines is a usage error."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import monitor_model as mm
from rtlsdr_amd import build as hipbuild
from rtlsdr_amd import synth
from rtlsdr_amd.capi import MODE_RAW, RtlfmCfg

pytestmark = pytest.mark.gpu

N, NB = 8, 24
ARGV = ["-s", "150k", "-m", "1.3M", "-F", "0"]


def plan(oracle_lib, freq):
    cfg = RtlfmCfg.default(mode=MODE_RAW, rate_out=150000)
    cf, cr = C.c_uint32(), C.c_uint32()
    oracle_lib.oracle().orc_optimal_settings(C.byref(cfg), freq, 150000, 1300000, 1, 0, C.byref(cf), C.byref(cr))
    return cfg


def sources(L):
    """Eight carriers keyed buffer by buffer, each with its own pattern; source 6 clips."""
    iq = np.empty((N, NB * L), dtype=np.uint8)
    for s in range(N):
        loud = synth.fm_iq_u8(1, NB * L // 2, amplitude=(220.0 if s == 6 else 30.0 + 5 * s), dev_hz=5e3, first_stream=s, seed=911)[0]
        quiet = synth.fm_iq_u8(1, NB * L // 2, amplitude=0.0, noise_lsb=1, first_stream=s, seed=912)[0]
        for b in range(NB):
            src = loud if (b + s) % (5 + s % 3) < 3 else quiet
            iq[s, b * L:(b + 1) * L] = src[b * L:(b + 1) * L]
    return iq


def rules(script):
    out = []
    for s in range(N):
        out.append(mm.rule(freq=100000000 + 200000 * s, gain=(mm.AUTO_GAIN if s % 2 else 100 + 5 * s), crit=(mm.CRIT_GT, mm.CRIT_LT)[s % 2],
                           ref_level=45.0 + s, ref_tol=1.5, num_meas=(2, 3)[s % 2], num_block_trigger=(0, 4, 7)[s % 3],
                           check_adc_max=1, check_adc_rms=1, command=("" if s == 3 else script),
                           args=f"{s} !freq! !mlevel! !crit! !gain! !reflevel! !reftol! end"))
    return out


def command_file(rs):
    lines = ["# one measurement line per source", "adc", ""]
    names = {mm.CRIT_GT: "gt", mm.CRIT_LT: "<"}
    for r in rs:
        gain = "auto" if r["gain"] == mm.AUTO_GAIN else "%.1f" % (r["gain"] / 10.0)
        lines.append(f'{r["freq"] // 1000}k, {gain}, {names[r["crit"]]}, {r["ref_level"]}, {r["ref_tol"]}, {r["num_meas"]}, '
                     f'{r["num_block_trigger"]}, {r["command"]}, {r["args"]}')
    lines.insert(6, "adcrms")
    return "\n".join(lines) + "\n"


def run_cli(tmp_path, srcs, argv, timeout=300):
    _, cli = hipbuild.build_host()
    lst = tmp_path / "sources.txt"
    lst.write_text("\n".join(str(s) for s in srcs) + "\n")
    env = {k: v for k, v in os.environ.items() if k != "RTLSDR_FILE"}
    env["RTLSDR_FILE_LIST"] = str(lst)
    return subprocess.run(["timeout", "-k", "10", str(timeout), cli] + argv, env=env, capture_output=True, text=True, timeout=timeout + 30)


def test_cli_monitor_events_and_commands(oracle_lib, tmp_path):
    lib = oracle_lib.oracle()
    cfg = plan(oracle_lib, 100000000)
    L = int(cfg.block_len)
    iq = sources(L)
    script = tmp_path / "fired.sh"
    log = tmp_path / "fired.log"
    script.write_text(f'#!/bin/sh\necho "$@" >> {log}\n')
    script.chmod(0o755)
    rs = rules(str(script))
    cmd = tmp_path / "monitor.csv"
    cmd.write_text(command_file(rs))
    srcs = []
    for s in range(N):
        p = tmp_path / f"in_{s}.bin"
        iq[s].tofile(p)
        srcs.append(p)

    # the model: the oracle's decimated IQ in raw mode, its rms() per buffer, the records of the raw bytes
    models, want_raw = [], []
    for s in range(N):
        st = oracle_lib.new_states(1)[0]
        scratch = np.zeros(2 * L + 64, dtype=np.int16)
        levels, raw = [], []
        for b in range(NB):
            k = lib.orc_block(C.byref(cfg), C.byref(st), np.ascontiguousarray(iq[s, b * L:(b + 1) * L]), L, scratch)
            levels.append(lib.orc_rms(scratch.ctypes.data, k, 1, 0))
            raw.append(scratch[:k].copy())
        m = mm.StreamModel(s, rs[s])
        m.feed(levels, mm.records(iq[s].reshape(NB, L)))
        models.append(m)
        want_raw.append(np.concatenate(raw))
    assert sum(e["fired"] for m in models for e in m.events) >= 8
    assert any(e["blocked_for"] > 0 for m in models for e in m.events)
    assert any(e["adc_max"] >= 120 for e in models[6].events)
    for m in models:
        for e in m.events:
            for bound in (m.r["ref_level"] - m.r["ref_tol"], m.r["ref_level"] + m.r["ref_tol"]):
                assert abs(e["level_db"] - bound) > 0.01

    r = run_cli(tmp_path, srcs, ["-N", str(N), "-C", str(cmd), "-v"] + ARGV + [str(tmp_path / "out_%d.raw")])
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"{N * NB} buffers in" in r.stderr
    # every event line, per stream in order, in the reference's wording
    for s, m in enumerate(models):
        got = re.findall(rf"^stream {s}: (.* kHz: gain .*)$", r.stderr, re.M)
        assert got == [mm.format_event(m.r, e) for e in m.events], (s, got[:3])
    # the commands: one line per fired event with a command, the placeholders replaced (the order between streams is free)
    want_lines = sorted(" ".join(mm.command_argv(m.r, e)[1:]) for m in models for e in m.events if e["fired"] and m.r["command"])
    assert sorted(log.read_text().splitlines()) == want_lines and len(want_lines) >= 6
    assert r.stderr.count("command to trigger is") == len(want_lines)
    assert any(e["fired"] for e in models[3].events)  # ... a line without a command fires and starts nothing
    # the exit statistics per line (src/rtl_fm.c:2033-2040)
    for m in models:
        st = m.stat
        assert "%u, %.1f, %.2f, %.1f" % (m.r["freq"], st["min"], st["sum"] / st["count"], st["max"]) in r.stderr
    # the raw IQ is written as -M raw writes it: every buffer of every source
    for s in range(N):
        assert np.array_equal(np.fromfile(tmp_path / f"out_{s}.raw", dtype=np.int16), want_raw[s]), s


def test_cli_monitor_needs_one_line_per_source(tmp_path):
    rs = rules("")[:7]
    cmd = tmp_path / "seven.csv"
    cmd.write_text(command_file(rs))
    r = run_cli(tmp_path, ["/dev/null"] * 8, ["-N", "8", "-C", str(cmd), str(tmp_path / "out_%d.raw")], timeout=60)
    assert r.returncode != 0
    assert "holds 7 measurement lines, -N 8 needs exactly 8" in r.stderr and "Use:" in r.stderr
