"""rtl_fm_hip -X: n sources (RTLSDR_FILE_LIST) x K channels as n x K streams of one handle over the source-indexed ring.
File s belongs to channel s % K of source s // K, mixed down by rtlfm_channel_step(channel_freq - f_source, capture_rate)
from the source tuned to its -f as given; it must be what the model computes on that source's bytes alone - completed
with bytes 127 to a whole buffer where the source ended in the middle of one - whatever the other sources do."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import channel_model as cm
from channel_common import assert_row_cfg, assert_rows, bounded, full_scale, tone_fit
from channel_fir_model import FirModel, raw_rows
from rtlsdr_amd import build as hipbuild
from rtlsdr_amd.capi import MODE_RAW, RtlfmCfg, RtlfmError
from rtlsdr_amd.demod import channel_lowpass

pytestmark = pytest.mark.gpu

BOUND = 89


def plan(oracle_lib, rate_in, min_capture=1000000, **ov):
    cfg = RtlfmCfg.default(**ov)
    cf, cr = C.c_uint32(), C.c_uint32()
    oracle_lib.oracle().orc_optimal_settings(C.byref(cfg), 100000000, rate_in, min_capture, 0, 0, C.byref(cf), C.byref(cr))
    return cfg, cr.value


def run_cli(tmp_path, sources, argv, timeout=300):
    _, cli = hipbuild.build_host()
    lst = tmp_path / "sources.txt"
    lst.write_text("\n".join(str(s) for s in sources) + "\n")
    env = {k: v for k, v in os.environ.items() if k != "RTLSDR_FILE"}
    env["RTLSDR_FILE_LIST"] = str(lst)
    return subprocess.run([cli] + argv, env=env, capture_output=True, text=True, timeout=timeout)


def out_file(tmp_path, s):
    return np.fromfile(tmp_path / f"out_{s}.raw", dtype=np.int16)


@pytest.mark.parametrize("raw_fir", [False, True], ids=["fm_dc_boxcar", "raw_fir33"])
def test_two_sources_of_different_lengths_three_channels_each(oracle_lib, tmp_path, raw_fir):
    """-s 24k -E dc -W 4 (2048-byte buffers, /42 at 1 008 000 S/s), and the same with -M raw -x 33.  Source 0 has 5 buffers
    and 700 bytes - one whole packet of them arrives and is completed with 127s -, source 1 has 3 buffers: its three files
    end there, source 0's go on.  (33 taps at /42: rtlfm_channel_lowpass(33, 0.4 / 42, 42) has taps beyond an int16 and
    says -ERANGE; the tool then takes the same filter at half the scale and one bit less shift - gain 21 at shift 13, the
    boxcar's DC gain of 42 all the same.)"""
    L, K = 2048, 3
    ov = dict(rate_out=24000, dc_block_audio=1, block_len=L)
    if raw_fir:
        ov["mode"] = MODE_RAW
    cfg, rate = plan(oracle_lib, 24000, **ov)
    assert rate == 1008000 and cfg.downsample == 42
    f_src = (100000000, 200000000)
    f_chan = ((100100000, 99800000, 100000000), (200250000, 199900000, 200100000))
    (tmp_path / "chan.txt").write_text("# source 0\n100.1M 99.8M,100M\n\n# source 1: one frequency and a range\n200.25M\t199.9M:200.1M:200k\n")
    nbytes = (5 * L + 700, 3 * L)
    make = full_scale if raw_fir else (lambda rows, n, seed: bounded(rows, n, seed, BOUND))
    srcs, data = [], []
    for i in range(2):
        x = make(1, 6 * L, 40 + i)[0]
        data.append(x)
        p = tmp_path / f"in_{i}.bin"
        x[:nbytes[i]].tofile(p)
        srcs.append(p)
    argv = ["-N", "2", "-f", "100M", "-f", "200M", "-X", str(tmp_path / "chan.txt"), "-s", "24k", "-E", "dc", "-W", "4"]
    if raw_fir:
        argv += ["-M", "raw", "-x", "33"]
    r = run_cli(tmp_path, srcs, argv + ["-v", str(tmp_path / "out_%d.raw")])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "9 buffers in" in r.stderr, r.stderr[-600:]
    for i in range(2):
        whole = nbytes[i] - nbytes[i] % 512
        done = (whole + L - 1) // L * L
        seen = np.concatenate([data[i][:whole], np.full(done - whole, 127, dtype=np.uint8)])[None, :]
        steps = [cm.step_from_hz(f - f_src[i], rate) for f in f_chan[i]]
        for c, st in enumerate(steps):
            assert f"stream {i * K + c}: source {i}, {f_chan[i][c]} Hz, step {st}" in r.stderr, (i, c, r.stderr[:3000])
        if raw_fir:
            with pytest.raises(RtlfmError):
                channel_lowpass(33, 0.4 / 42, 42)
            taps, shift = channel_lowpass(33, 0.4 / 42, 21)
            shift -= 1
            assert "-x 33: gain 21 at shift 13" in r.stderr, r.stderr[:3000]
            want = raw_rows(*FirModel(steps, K, 42, taps, shift, 1).run(seen))
            assert_rows([out_file(tmp_path, i * K + c) for c in range(K)], want, f"source {i}")
        else:
            want, wn, _ = cm.model_via_oracle(cm.copy_cfg(cfg, max_blocks=8), seen, steps, K, 0)
            for c in range(K):
                assert_row_cfg(out_file(tmp_path, i * K + c), want[c, :wn[c]], cfg, f"source {i} channel {c}")


def test_two_carriers_of_one_source_as_two_files(tmp_path):
    """One source with FM carriers 200 kHz above and 150 kHz below its -f, modulated with 2 kHz and 5 kHz (30 kHz
    deviation), -s 240k -m 2.2M -A fast (/10 at 2.4 MS/s).  Each channel's audio is its own tone: fast_atan2 scales pi to
    16384, so a deviation of 30 kHz at 240 kS/s is an amplitude of 16384 * 30 / 120 = 4096 - asserted within a quarter -
    and the other carrier's tone, which only crosstalk could bring, stays below a tenth of that."""
    fs, L, nb = 2_400_000, 16384, 8
    offs, tones = (200_000, -150_000), (2000.0, 5000.0)
    n = np.arange(nb * L // 2, dtype=np.float64)
    sig = np.zeros(n.size, dtype=np.complex128)
    for f, tone in zip(offs, tones):
        sig += 40.0 * np.exp(1j * (2 * np.pi * f * n / fs + (30e3 / tone) * np.sin(2 * np.pi * tone * n / fs)))
    src = np.empty(nb * L, dtype=np.uint8)
    src[0::2] = np.rint(127 + sig.real).astype(np.uint8)
    src[1::2] = np.rint(127 + sig.imag).astype(np.uint8)
    src.tofile(tmp_path / "in.bin")
    (tmp_path / "chan.txt").write_text("100.2M 99.85M\n")
    r = run_cli(tmp_path, [tmp_path / "in.bin"], ["-f", "100M", "-X", str(tmp_path / "chan.txt"), "-s", "240k", "-m", "2.2M", "-A", "fast",
                                                 str(tmp_path / "out_%d.raw")])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Sampling at 2400000 S/s" in r.stderr and "tuned to 100000000 Hz" in r.stderr, r.stderr[:1000]
    for c in range(2):
        pcm = out_file(tmp_path, c)
        assert pcm.size == nb * L // 2 // 10, pcm.size
        _, own = tone_fit(pcm, tones[c], fs / 10, 256)
        _, other = tone_fit(pcm, tones[1 - c], fs / 10, 256)
        print(f"channel {c}: own tone {own:.1f}, the other's {other:.1f}")
        assert abs(own - 4096.0) <= 1024.0 and other <= 409.6, (c, own, other)


def test_squelch_holds_back_per_channel(oracle_lib, tmp_path):
    """-l 100 -t 3, one source x two channels: a keyed carrier 96 kHz above -f (silence, signal, silence) and nothing at
    192 kHz below it.  Each file is demod_thread_fn's hold-back rule (src/rtl_fm.c:1366-1370) over that channel's own
    buffers, as test_cli_squelch_holds_output_back_like_demod_thread_fn builds it for one stream; the empty channel's
    squelch never opens."""
    L, nb, t = 16384, 30, 3
    cfg, rate = plan(oracle_lib, 24000, rate_out=24000, squelch_level=100)
    assert rate == 1008000
    n = np.arange(nb * L // 2, dtype=np.float64)
    keyed = ((n >= 6 * L // 2) & (n < 18 * L // 2)).astype(np.float64)
    sig = 60.0 * keyed * np.exp(1j * (2 * np.pi * 96000 * n / rate + (2500.0 / 1000.0) * np.sin(2 * np.pi * 1000.0 * n / rate)))
    rng = np.random.default_rng(5)
    src = np.empty(nb * L, dtype=np.uint8)
    src[0::2] = np.rint(127 + sig.real + rng.integers(-1, 2, n.size)).astype(np.uint8)
    src[1::2] = np.rint(127 + sig.imag + rng.integers(-1, 2, n.size)).astype(np.uint8)
    src.tofile(tmp_path / "in.bin")
    (tmp_path / "chan.txt").write_text("100.096M 99.808M\n")
    r = run_cli(tmp_path, [tmp_path / "in.bin"], ["-f", "100M", "-X", str(tmp_path / "chan.txt"), "-s", "24k", "-l", "100", "-t", str(t), "-v",
                                                 str(tmp_path / "out_%d.raw")])
    assert r.returncode == 0, r.stderr[-2000:]
    steps = [cm.step_from_hz(96000, rate), cm.step_from_hz(-192000, rate)]
    by = cm.mixed_bytes(src[None, :], steps, 2, 0)
    ocfg = cm.copy_cfg(cfg, offset_tuning=1)
    lib = oracle_lib.oracle()
    scratch = np.zeros(L, dtype=np.int16)
    helds = []
    for c in range(2):
        st = oracle_lib.new_states(1)[0]
        want, held = [np.zeros(0, dtype=np.int16)], 0
        for b in range(nb):
            k = lib.orc_block(C.byref(ocfg), C.byref(st), np.ascontiguousarray(by[c, b * L:(b + 1) * L]), L, scratch)
            if st.squelch_hits > t:
                st.squelch_hits = t + 1
                held += 1
                continue
            want.append(scratch[:k].copy())
        want = np.concatenate(want)
        helds.append(held)
        assert f"stream {c}: {want.size} samples out, {held} buffers held back" in r.stderr, (c, held, r.stderr[-1500:])
        assert_row_cfg(out_file(tmp_path, c), want, cfg, f"channel {c}")
    assert 8 < helds[0] < nb - 8 and helds[1] == nb, helds
    assert f"{nb} buffers in" in r.stderr and f"{sum(helds)} buffers held back" in r.stderr


def keyed_carriers(nb, L, rate, windows, seed):
    """nb buffers of L bytes: noise of one LSB and, for each (offset Hz, first, last) of windows, an FM carrier of amplitude 40
    at that offset from the centre in buffers first .. last-1."""
    n = np.arange(nb * L // 2, dtype=np.float64)
    sig = np.zeros(n.size, dtype=np.complex128)
    for off, first, last in windows:
        on = ((n >= first * L // 2) & (n < last * L // 2)).astype(np.float64)
        sig += 40.0 * on * np.exp(1j * (2 * np.pi * off * n / rate + (2500.0 / 1000.0) * np.sin(2 * np.pi * 1000.0 * n / rate)))
    rng = np.random.default_rng(seed)
    src = np.empty(nb * L, dtype=np.uint8)
    src[0::2] = np.rint(127 + sig.real + rng.integers(-1, 2, n.size)).astype(np.uint8)
    src[1::2] = np.rint(127 + sig.imag + rng.integers(-1, 2, n.size)).astype(np.uint8)
    return src


def held_back_per_channel(oracle_lib, cfg, rate, src, offsets, L, t):
    """demod_thread_fn's rule (src/rtl_fm.c:1366-1370) over each channel's own buffers of one source: [(PCM, buffers held)]."""
    steps = [cm.step_from_hz(off, rate) for off in offsets]
    by = cm.mixed_bytes(src[None, :], steps, len(steps), 0)
    ocfg = cm.copy_cfg(cfg, offset_tuning=1)
    lib = oracle_lib.oracle()
    scratch = np.zeros(L, dtype=np.int16)
    res = []
    for c in range(len(steps)):
        st = oracle_lib.new_states(1)[0]
        want, held = [np.zeros(0, dtype=np.int16)], 0
        for b in range(src.size // L):
            k = lib.orc_block(C.byref(ocfg), C.byref(st), np.ascontiguousarray(by[c, b * L:(b + 1) * L]), L, scratch)
            if st.squelch_hits > t:
                st.squelch_hits = t + 1
                held += 1
                continue
            want.append(scratch[:k].copy())
        res.append((np.concatenate(want), held))
    return res


OFFSETS = (96000, -192000)


def squelch_two_sources_case(oracle_lib):
    """-s 24k -l 100 -t 3 -W 4, two sources x two channels 96 kHz above and 192 kHz below each -f: (cfg, rate, L, t, captures).
    Source 0, 9 buffers: carriers in buffers 2 .. 3 and 4 .. 6; source 1, 4 buffers: carriers in 1 .. 2 and 2 .. 3.  A
    channel is silent until its carrier comes (squelch_hits starts at 11) and again from the fourth buffer the squelch finds
    closed; the buffer behind a carrier still opens it (the boxcar's sum across the boundary).  By the oracle the four
    streams hold 3 (buffers 0, 1, 8), 4 (0 .. 3), 1 and 2 buffers."""
    L, t = 2048, 3
    cfg, rate = plan(oracle_lib, 24000, rate_out=24000, squelch_level=100, block_len=L)
    assert rate == 1008000
    return cfg, rate, L, t, [keyed_carriers(9, L, rate, ((OFFSETS[0], 2, 4), (OFFSETS[1], 4, 7)), 7),
                             keyed_carriers(4, L, rate, ((OFFSETS[0], 1, 3), (OFFSETS[1], 2, 4)), 8)]


def test_squelch_per_channel_when_a_source_ends(oracle_lib, tmp_path):
    """-N 2 -X, two channels each, -l 100 -t 3: source 1 ends after 4 of source 0's 9 buffers and is fed bytes 127 from
    then on.  Its two files stop growing and its counters stop - each is the hold-back rule over its channel's 4 buffers -,
    and the files and counts of source 0 are the rule over its own 9 buffers."""
    cfg, rate, L, t, data = squelch_two_sources_case(oracle_lib)
    f_src = (100000000, 200000000)
    (tmp_path / "chan.txt").write_text("".join(" ".join(str(f + off) for off in OFFSETS) + "\n" for f in f_src))
    srcs = []
    for i, x in enumerate(data):
        p = tmp_path / f"in_{i}.bin"
        x.tofile(p)
        srcs.append(p)
    r = run_cli(tmp_path, srcs, ["-N", "2", "-f", "100M", "-f", "200M", "-X", str(tmp_path / "chan.txt"), "-s", "24k", "-l", "100", "-t", str(t),
                                 "-W", "4", "-v", str(tmp_path / "out_%d.raw")])
    assert r.returncode == 0, r.stderr[-2000:]
    total, samples = 0, 0
    for i, x in enumerate(data):
        nb = x.size // L
        for c, (want, held) in enumerate(held_back_per_channel(oracle_lib, cfg, rate, x, OFFSETS, L, t)):
            s = 2 * i + c
            total += held
            samples += want.size
            assert 0 < held < nb and want.size > 0, (s, held)
            assert f"stream {s}: {want.size} samples out, {held} buffers held back" in r.stderr, (s, held, r.stderr[-1500:])
            assert_row_cfg(out_file(tmp_path, s), want, cfg, f"source {i} channel {c}")
    assert f"13 buffers in, {samples} samples out, {total} buffers held back by the squelch" in r.stderr, r.stderr[-1500:]
