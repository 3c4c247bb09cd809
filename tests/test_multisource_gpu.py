"""rtl_fm_hip -N n: n devices (RTLSDR_FILE_LIST) demodulated as n streams of one handle.  Every stream's
file must be what the oracle computes on that source alone, whatever the other sources do: their
content, their length, how their bytes arrive."""
import ctypes as C
import os
import socket
import subprocess
import threading
import time

import numpy as np
import pytest

from rtlsdr_amd import build as hipbuild
from rtlsdr_amd import synth
from rtlsdr_amd.capi import (ATAN_FAST, ATAN_STD, MODE_AM, MODE_FM, MODE_RAW, RESAMPLE_LOW_PASS_REAL, RtlfmCfg)

pytestmark = pytest.mark.gpu

WBFM = dict(rate_out=170000, rate_out2=32000, custom_atan=ATAN_FAST, deemph=1, resampler=RESAMPLE_LOW_PASS_REAL)
CASES = [
    # argv, planner inputs (rate_in, min_capture, fifth, cfg overrides), fs of the synthetic capture - as tests/test_cli_gpu.py
    (["-M", "fm", "-s", "150k", "-m", "1.3M", "-F", "0", "-A", "std"], (150000, 1300000, 1, dict(rate_out=150000)), 2.4e6),
    (["-s", "24k", "-E", "dc"], (24000, 1000000, 0, dict(rate_out=24000, dc_block_audio=1)), 1.008e6),
    (["-M", "wbfm"], (170000, 1000000, 0, WBFM), 1.02e6),
    (["-M", "am", "-s", "24k", "-F", "9"], (24000, 1000000, 1, dict(mode=MODE_AM, rate_out=24000, comp_fir_size=9)), 1.536e6),
    (["-M", "raw", "-s", "150k", "-m", "1.3M", "-F", "0"], (150000, 1300000, 1, dict(mode=MODE_RAW, rate_out=150000)), 2.4e6),
    (["-M", "fm", "-s", "150k", "-m", "1.3M", "-F", "0", "-E", "rdc"], (150000, 1300000, 1, dict(rate_out=150000, dc_block_raw=1)), 2.4e6),
]


def _plan(oracle_lib, argv, plan, freq=100000000):
    rate_in, min_capture, fifth, ov = plan
    cfg = RtlfmCfg.default(**ov)
    cf, cr = C.c_uint32(), C.c_uint32()
    oracle_lib.oracle().orc_optimal_settings(C.byref(cfg), freq + (16000 if "wbfm" in argv else 0), rate_in, min_capture,
                                             fifth, 0, C.byref(cf), C.byref(cr))
    if cfg.deemph:
        cfg.deemph_a = oracle_lib.oracle().orc_deemph_a(cfg.rate_out, 75)
    return cfg


def _close(cfg, got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    exact_needed = cfg.mode == MODE_FM and cfg.custom_atan != ATAN_STD
    assert d.max(initial=0) <= (0 if exact_needed else 1) and (d != 0).mean() <= 1e-4, (what, int(d.max()), int((d != 0).sum()))


def _run(tmp_path, sources, argv, timeout=600):
    """The CLI over RTLSDR_FILE_LIST = sources; returns the CompletedProcess."""
    _, cli = hipbuild.build_host()
    lst = tmp_path / "sources.txt"
    lst.write_text("# rtl_fm_hip -N\n" + "\n".join(str(s) for s in sources) + "\n")
    env = {k: v for k, v in os.environ.items() if k != "RTLSDR_FILE"}
    env["RTLSDR_FILE_LIST"] = str(lst)
    return subprocess.run([cli] + argv, env=env, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("argv,plan,fs", CASES)
def test_256_sources_each_match_the_oracle(oracle_lib, tmp_path, argv, plan, fs):
    n, nb = 256, 3
    cfg = _plan(oracle_lib, argv, plan)
    L = int(cfg.block_len)
    amp = 30.0 if cfg.custom_atan == ATAN_FAST else 60.0
    iq = synth.fm_iq_u8(n, L // 2 * nb, fs=fs, dev_hz=5e3, amplitude=amp, seed=606)
    srcs = []
    for i in range(n):
        p = tmp_path / f"in_{i}.bin"
        iq[i].tofile(p)
        srcs.append(p)
    r = _run(tmp_path, srcs, ["-N", str(n), "-f", "100M"] + argv + [str(tmp_path / "out_%d.raw")])
    assert r.returncode == 0, r.stderr[-1500:]
    assert f"{n * nb} buffers in" in r.stderr, r.stderr[-400:]
    for i in range(n):
        want, _ = oracle_lib.run_stream(cfg, iq[i])
        _close(cfg, np.fromfile(tmp_path / f"out_{i}.raw", dtype=np.int16), want, i)


def test_32_slow_rtl_tcp_sources(oracle_lib, tmp_path):
    """32 rtl_tcp servers that send in chunks of different sizes, with pauses, and end after different numbers of
    buffers (plus a few bytes that are not a whole packet): every whole buffer that arrived is demodulated once."""
    n = 32
    argv = ["-M", "fm", "-s", "150k", "-m", "1.3M", "-F", "0"]
    cfg = _plan(oracle_lib, argv, (150000, 1300000, 1, dict(rate_out=150000)))
    L = int(cfg.block_len)
    nbs = [3 + i % 5 for i in range(n)]
    iq = synth.fm_iq_u8(n, L // 2 * max(nbs), fs=2.4e6, dev_hz=5e3, amplitude=60.0, seed=707)
    servers, threads, urls = [], [], []
    for i in range(n):
        payload = iq[i, :L * nbs[i]].tobytes() + bytes(range(7 * i % 300))
        srv = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
        srv.bind(("127.0.0.1", 0))
        srv.listen(1)
        servers.append(srv)
        urls.append(f"tcp://127.0.0.1:{srv.getsockname()[1]}")
        chunk = 1000 + 397 * i

        def serve(srv=srv, payload=payload, chunk=chunk, i=i):
            c, _ = srv.accept()
            c.sendall(b"RTL0" + (5).to_bytes(4, "big") + (29).to_bytes(4, "big"))
            for at in range(0, len(payload), chunk):
                c.sendall(payload[at:at + chunk])
                time.sleep(0.001 if (at // chunk + i) % 5 else 0.01)
            # as test_cli_on_a_slow_rtl_tcp_source_loses_nothing: finish sending, drain until the client leaves
            c.shutdown(socket.SHUT_WR)
            c.settimeout(30.0)
            try:
                while c.recv(4096):
                    pass
            except OSError:
                pass
            c.close()
        t = threading.Thread(target=serve, daemon=True)
        t.start()
        threads.append(t)
    r = _run(tmp_path, urls, ["-N", str(n), "-v", "-f", "100M"] + argv + [str(tmp_path / "out_%d.raw")])
    for t in threads:
        t.join(10)
    for s in servers:
        s.close()
    assert r.returncode == 0, r.stderr[-1500:]
    for i in range(n):
        assert f"stream {i}: {nbs[i]} buffers in" in r.stderr, (i, r.stderr[-2000:])
        want, _ = oracle_lib.run_stream(cfg, iq[i, :L * nbs[i]])
        _close(cfg, np.fromfile(tmp_path / f"out_{i}.raw", dtype=np.int16), want, i)


@pytest.mark.parametrize("argv,plan,fs", [CASES[0], CASES[2]], ids=["fm", "wbfm"])
def test_sources_of_different_lengths(oracle_lib, tmp_path, argv, plan, fs):
    """8 files of 1 .. 8 buffers, each with a last part that is not a whole buffer (nor a whole packet): streams leave
    the batch as their sources end, the others go on with their state on a smaller handle."""
    n = 8
    cfg = _plan(oracle_lib, argv, plan)
    L = int(cfg.block_len)
    amp = 30.0 if cfg.custom_atan == ATAN_FAST else 60.0
    iq = synth.fm_iq_u8(n, L // 2 * (n + 1), fs=fs, dev_hz=5e3, amplitude=amp, seed=808)
    order = [5, 0, 7, 2, 1, 6, 3, 4]  # buffers - 1 of stream i: the lengths are not sorted by stream
    srcs = []
    for i in range(n):
        p = tmp_path / f"in_{i}.bin"
        iq[i, :L * (order[i] + 1) + 100 + 50 * i].tofile(p)
        srcs.append(p)
    r = _run(tmp_path, srcs, ["-N", str(n), "-v", "-f", "100M"] + argv + [str(tmp_path / "out_%d.raw")])
    assert r.returncode == 0, r.stderr[-1500:]
    for i in range(n):
        assert f"stream {i}: {order[i] + 1} buffers in" in r.stderr, (i, r.stderr[-1500:])
        want, _ = oracle_lib.run_stream(cfg, iq[i, :L * (order[i] + 1)])
        _close(cfg, np.fromfile(tmp_path / f"out_{i}.raw", dtype=np.int16), want, i)


def test_squelch_per_stream(oracle_lib, tmp_path):
    """-l / -t with 16 streams: each file is demod_thread_fn's hold-back rule over that stream's own buffers
    (as test_cli_squelch_holds_output_back_like_demod_thread_fn for one stream)."""
    n, L, nb, t = 16, 16384, 24, 3
    cfg = RtlfmCfg.default(rate_out=24000, squelch_level=40)
    cf, cr = C.c_uint32(), C.c_uint32()
    oracle_lib.oracle().orc_optimal_settings(C.byref(cfg), 100000000, 24000, 1000000, 0, 0, C.byref(cf), C.byref(cr))
    sig = synth.fm_iq_u8(n, L // 2 * nb, fs=1.008e6, dev_hz=2.5e3, amplitude=60.0, seed=77).reshape(n, nb, L)
    quiet = synth.fm_iq_u8(n, L // 2 * nb, fs=1.008e6, dev_hz=2.5e3, amplitude=0.0, noise_lsb=1, seed=78).reshape(n, nb, L)
    iq, srcs = [], []
    for i in range(n):
        a, b = 2 + i % 5, 10 + i % 7  # signal in buffers a .. b-1, silence around it
        x = np.concatenate([quiet[i, :a], sig[i, a:b], quiet[i, b:]]).ravel()
        iq.append(x)
        p = tmp_path / f"in_{i}.bin"
        x.tofile(p)
        srcs.append(p)
    r = _run(tmp_path, srcs, ["-N", str(n), "-v", "-f", "100M", "-s", "24k", "-l", "40", "-t", str(t),
                              str(tmp_path / "out_%d.raw")])
    assert r.returncode == 0, r.stderr[-1500:]
    lib = oracle_lib.oracle()
    scratch = np.zeros(L, dtype=np.int16)
    total_held = 0
    for i in range(n):
        st = oracle_lib.new_states(1)[0]
        want, held = [], 0
        for b in range(nb):
            k = lib.orc_block(C.byref(cfg), C.byref(st), np.ascontiguousarray(iq[i][b * L:(b + 1) * L]), L, scratch)
            if st.squelch_hits > t:
                st.squelch_hits = t + 1
                held += 1
                continue
            want.append(scratch[:k].copy())
        want = np.concatenate(want)
        total_held += held
        assert 5 < held < nb - 5 and f"stream {i}: {nb} buffers in, {want.size} samples out, {held} buffers held back" in r.stderr, \
            (i, held, r.stderr[-1500:])
        got = np.fromfile(tmp_path / f"out_{i}.raw", dtype=np.int16)
        assert got.shape == want.shape and np.abs(got.astype(np.int32) - want.astype(np.int32)).max() <= 1, i
    assert f"{n * nb} buffers in, " in r.stderr and f"{total_held} buffers held back" in r.stderr


def _keyed(seed, L, nb, first, last, fs):
    """nb buffers of L bytes: noise of one LSB, and an FM signal in buffers first .. last-1."""
    sig = synth.fm_iq_u8(1, L // 2 * nb, fs=fs, dev_hz=2.5e3, amplitude=60.0, seed=seed)[0].reshape(nb, L)
    quiet = synth.fm_iq_u8(1, L // 2 * nb, fs=fs, dev_hz=2.5e3, amplitude=0.0, noise_lsb=1, seed=seed + 1)[0].reshape(nb, L)
    return np.concatenate([quiet[:first], sig[first:last], quiet[last:]]).ravel()


def _held_back(oracle_lib, cfg, iq, L, t):
    """demod_thread_fn's rule (src/rtl_fm.c:1366-1370) over the oracle's per-buffer outputs: (the PCM, buffers held)."""
    lib = oracle_lib.oracle()
    st = oracle_lib.new_states(1)[0]
    scratch = np.zeros(L, dtype=np.int16)
    want, held = [np.zeros(0, dtype=np.int16)], 0
    for b in range(iq.size // L):
        k = lib.orc_block(C.byref(cfg), C.byref(st), np.ascontiguousarray(iq[b * L:(b + 1) * L]), L, scratch)
        if st.squelch_hits > t:
            st.squelch_hits = t + 1
            held += 1
            continue
        want.append(scratch[:k].copy())
    return np.concatenate(want), held


def squelch_behind_resampler_case(oracle_lib):
    """-s 96k -r 32k -A fast -l 40 -t 3 -W 4 (/11 at 1 056 000 S/s, which does not divide a buffer's 1024 samples; rtl_fm's
    low_pass_real wants -r below -s): (cfg, L, t, the two captures).  Source 0: 9 buffers, signal in 2 and 3; source 1: 4
    buffers, signal in 1 and 2.  A stream is silent until its signal comes (squelch_hits starts at 11) and again from the
    fourth buffer the squelch finds closed: by the oracle, source 0 holds 4 of its 9 buffers and source 1 one of its 4."""
    L, t = 2048, 3
    cfg = RtlfmCfg.default(rate_out=96000, rate_out2=32000, custom_atan=ATAN_FAST, squelch_level=40, block_len=L)
    cf, cr = C.c_uint32(), C.c_uint32()
    oracle_lib.oracle().orc_optimal_settings(C.byref(cfg), 100000000, 96000, 1000000, 0, 0, C.byref(cf), C.byref(cr))
    assert cr.value == 1056000 and cfg.downsample == 11
    return cfg, L, t, [_keyed(31, L, 9, 2, 4, 1.056e6), _keyed(41, L, 4, 1, 3, 1.056e6)]


def test_squelch_behind_a_resampler_across_a_shrink(oracle_lib, tmp_path):
    """-N 2 -l 40 -t 3 -r 32k: behind the resampler the handle has no squelch gate (-ENOTSUP), so the hold-back rule runs
    from the carried state (rtlfm_gpu_state_get_all / _set_all), stream k of the handle for source live[k].  Source 1 ends
    after 4 of source 0's 9 buffers: the rule goes on over source 0 on the handle it moved to."""
    cfg, L, t, iq = squelch_behind_resampler_case(oracle_lib)
    srcs = []
    for i, x in enumerate(iq):
        p = tmp_path / f"in_{i}.bin"
        x.tofile(p)
        srcs.append(p)
    r = _run(tmp_path, srcs, ["-N", "2", "-v", "-f", "100M", "-s", "96k", "-r", "32k", "-A", "fast", "-l", "40", "-t", str(t), "-W", "4",
                              str(tmp_path / "out_%d.raw")])
    assert r.returncode == 0, r.stderr[-1500:]
    assert "1 of 2 streams go on" in r.stderr, r.stderr[-1500:]
    total = 0
    for i, x in enumerate(iq):
        nb = x.size // L
        want, held = _held_back(oracle_lib, cfg, x, L, t)
        total += held
        assert 0 < held < nb and want.size > 0, (i, held)
        assert f"stream {i}: {nb} buffers in, {want.size} samples out, {held} buffers held back" in r.stderr, (i, held, r.stderr[-1500:])
        _close(cfg, np.fromfile(tmp_path / f"out_{i}.raw", dtype=np.int16), want, i)
    assert "13 buffers in, " in r.stderr and f" samples out, {total} buffers held back by the squelch" in r.stderr


def test_levels_per_stream(oracle_lib, tmp_path):
    """-L with 4 streams, each tuned to its own -f: every stream's level lines (prefixed 'stream i: ') are
    full_demod()'s bookkeeping over that stream's rms() values."""
    import math
    from rtlsdr_amd import capi
    n, L, nb, n_every = 4, 16384, 9, 4
    freqs = [100000000, 101000000, 102500000, 97000000]
    cfg = RtlfmCfg.default(rate_out=150000)
    cf, cr = C.c_uint32(), C.c_uint32()
    oracle_lib.oracle().orc_optimal_settings(C.byref(cfg), freqs[0], 150000, 1300000, 1, 0, C.byref(cf), C.byref(cr))
    iq = synth.fm_iq_u8(n, L // 2 * nb, fs=2.4e6, dev_hz=75e3, amplitude=55.0, seed=12)
    srcs = []
    for i in range(n):
        p = tmp_path / f"in_{i}.bin"
        iq[i].tofile(p)
        srcs.append(p)
    fargs = [a for f in freqs for a in ("-f", str(f))]
    r = _run(tmp_path, srcs, ["-N", str(n)] + fargs + ["-M", "fm", "-s", "150k", "-m", "1.3M", "-F", "0", "-L", str(n_every),
                                                       str(tmp_path / "out_%d.raw")])
    assert r.returncode == 0, r.stderr[-1500:]
    lib = oracle_lib.oracle()
    lib.orc_rms.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.orc_rms.restype = C.c_int
    raw = RtlfmCfg.from_buffer_copy(bytes(cfg))
    raw.mode = capi.MODE_RAW
    scratch = np.zeros(2 * L, dtype=np.int16)
    for i in range(n):
        lines = [ln for ln in r.stderr.splitlines() if ln.startswith(f"stream {i}: ") and " avg rms, " in ln]
        st = oracle_lib.new_states(1)[0]
        want, no, lsum, lmax, lmaxmax = [], 1, 0.0, 0, 0
        for b in range(nb):
            k = lib.orc_block(C.byref(raw), C.byref(st), np.ascontiguousarray(iq[i, b * L:(b + 1) * L]), L, scratch)
            sr = lib.orc_rms(scratch.ctypes.data, k, 1, 0)
            no -= 1
            lsum += sr; lmax = max(lmax, sr); lmaxmax = max(lmaxmax, sr)
            if no == 0:
                no = n_every
                avg = lsum / n_every
                want.append("stream %d: %.3f kHz, %.1f avg rms, %d max rms, %d max max rms, %d squelch rms, %d rms, %.1f dB rms level, %.2f dB avg rms level"
                            % (i, freqs[i] / 1000.0, avg, lmax, lmaxmax, 0, sr, 20 * math.log10(1e-10 + sr), 20 * math.log10(1e-10 + avg)))
                lmax, lsum = 0, 0.0
        assert lines == want, i
        ref, _ = oracle_lib.run_stream(cfg, iq[i])
        got = np.fromfile(tmp_path / f"out_{i}.raw", dtype=np.int16)
        assert got.shape == ref.shape and np.abs(got.astype(np.int32) - ref.astype(np.int32)).max() <= 1, i


def test_wav_header_per_file(oracle_lib, tmp_path):
    """-H with -N: one header per file, with that stream's frequency (+16 kHz under -M wbfm) and its own data size."""
    n = 3
    cfg = _plan(oracle_lib, ["-M", "wbfm"], (170000, 1000000, 0, WBFM))
    L = int(cfg.block_len)
    iq = synth.fm_iq_u8(n, L // 2 * 4, fs=1.02e6, dev_hz=5e3, amplitude=30.0, seed=909)
    srcs = []
    for i in range(n):
        p = tmp_path / f"in_{i}.bin"
        iq[i, :L * (2 + i)].tofile(p)
        srcs.append(p)
    freqs = [88100000, 95300000, 101700000]
    fargs = [a for f in freqs for a in ("-f", str(f))]
    r = _run(tmp_path, srcs, ["-N", str(n), "-M", "wbfm", "-H"] + fargs + [str(tmp_path / "fm%d.wav")])
    assert r.returncode == 0, r.stderr[-1500:]
    for i in range(n):
        b = (tmp_path / f"fm{i}.wav").read_bytes()
        assert b[:4] == b"RIFF" and b[112:116] == b"data"
        assert int.from_bytes(b[76:80], "little") == freqs[i] + 16000
        assert int.from_bytes(b[116:120], "little") == len(b) - 120
        want, _ = oracle_lib.run_stream(cfg, iq[i, :L * (2 + i)])
        _close(cfg, np.frombuffer(b[120:], dtype=np.int16), want, i)


@pytest.mark.parametrize("argv", [["-M", "wbfm"], ["-M", "fm", "-s", "150k", "-m", "1.3M", "-F", "0", "-l", "30"]])
def test_N1_is_the_plain_program(tmp_path, argv):
    """-N 1 is today's single-stream program: the same bytes as without -N."""
    _, cli = hipbuild.build_host()
    iq = synth.fm_iq_u8(1, 16384 // 2 * 11 + 300, fs=1.02e6, dev_hz=5e3, amplitude=40.0, seed=1001)[0]
    src = tmp_path / "c.bin"
    iq.tofile(src)
    env = dict(os.environ, RTLSDR_FILE=str(src))
    outs = []
    for extra in ([], ["-N", "1"]):
        out = tmp_path / f"o{len(outs)}.raw"
        r = subprocess.run([cli, "-f", "100M"] + extra + argv + [str(out)], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-1500:]
        outs.append(out.read_bytes())
    assert len(outs[0]) > 0 and outs[0] == outs[1]
