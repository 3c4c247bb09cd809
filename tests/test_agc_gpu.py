"""The soft AGC on a handle: SoftAgc.update() after every run against the restatement fed with the model's records, and
rtl_fm_hip -N 3 -O agc=2 -v against the same model, its PCM byte-identical to the run without -O."""
import os
import re
import subprocess

import numpy as np
import pytest

import health_model as hm
from rtlsdr_amd import build as hipbuild
from rtlsdr_amd import synth
from rtlsdr_amd.capi import RtlfmCfg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

C2 = dict(downsample=16, downsample_passes=4, rate_out=150000)


def loudness_streams(L, nbuf):
    """Four streams: quiet (amplitude 5), middling (60), clipped (127 and more) and one that alternates buffer by buffer."""
    quiet = synth.fm_iq_u8(1, nbuf * L // 2, amplitude=5.0, first_stream=0)[0]
    mid = synth.fm_iq_u8(1, nbuf * L // 2, amplitude=60.0, first_stream=1)[0]
    loud = synth.fm_iq_u8(1, nbuf * L // 2, amplitude=127.0, first_stream=2)[0]
    alt = quiet.copy()
    for b in range(0, nbuf, 2):
        alt[b * L:(b + 1) * L] = loud[b * L:(b + 1) * L]
    return np.stack([quiet, mid, loud, alt])


@pytest.mark.parametrize("settle", [0, 4])
def test_update_against_model(settle):
    from rtlsdr_amd.agc import SoftAgc
    from rtlsdr_amd.demod import GpuDemod
    S, L, nb, runs = 4, 16384, 4, 6
    gain_counts = [29, 29, 5, 3]
    iq = loudness_streams(L, nb * runs)
    want = hm.records(iq.reshape(S, nb * runs, L))
    assert (8000 * want["overload"][2].astype(np.int64) >= L).all() and not want["overload"][0].any()  # clipped / quiet for real
    models = [hm.StreamModel(s, gain_counts[s], settle=settle) for s in range(S)]
    cfg = RtlfmCfg.default(block_len=L, max_blocks=nb, **C2)
    with GpuDemod(cfg, S, 0, options={"input_health": 1}) as g, SoftAgc(gain_counts) as a:
        a.set_settle(settle)
        a.set_index(2, 4)
        models[2].index = 4
        got = []
        for r in range(runs):
            g.run_torch(torch.from_numpy(iq[:, r * nb * L:(r + 1) * nb * L].copy()).cuda())
            a.update(g)
            for s in range(S):
                models[s].feed(want[s, r * nb:(r + 1) * nb], L)
            got += a.poll()
            assert [a.state(s) for s in range(S)] == [m.state() for m in models], r
        for s in range(S):
            assert [e for e in got if e["stream"] == s] == models[s].events, s
    assert models[0].events and models[2].events and models[3].events
    assert models[2].index == 0 and models[0].index > 0


def test_cli_agc2(tmp_path):
    """rtl_fm_hip -N 3 -O agc=2 -v: printed changes, overload flips and final indices equal the model's; the PCM files are
    byte-identical to the same command without -O."""
    _, cli = hipbuild.build_host()
    L, NB = 16384, 21  # the tool's default buffer; 21 buffers: runs of up to 8
    iq = loudness_streams(L, NB)[[0, 2, 3]]
    iq = np.concatenate([iq, iq[:, :1536]], axis=1)  # a short last buffer of 1536 bytes: its record over its own length
    srcs = []
    for s in range(3):
        p = tmp_path / f"in_{s}.bin"
        iq[s].tofile(p)
        srcs.append(str(p))
    (tmp_path / "sources.txt").write_text("\n".join(srcs) + "\n")
    env = {k: v for k, v in os.environ.items() if k != "RTLSDR_FILE"}
    env["RTLSDR_FILE_LIST"] = str(tmp_path / "sources.txt")
    outs = {}
    for key, extra in (("plain", ["-v"]), ("bw", ["-O", "bw=1500", "-v"]), ("agc", ["-O", "bw=1500:agc=2", "-v"])):
        d = tmp_path / key
        d.mkdir()
        r = subprocess.run(["timeout", "-k", "10", "120", cli, "-f", "100M", "-s", "150k", "-m", "1.3M", "-F", "0", "-N", "3"] + extra
                           + [str(d / "out_%d.raw")], env=env, capture_output=True, text=True, timeout=150)
        assert r.returncode == 0, r.stderr
        outs[key] = (r.stderr, [(d / f"out_{s}.raw").read_bytes() for s in range(3)])
    assert outs["plain"][1] == outs["agc"][1] and all(len(b) > 0 for b in outs["plain"][1])
    # a -O string without agc= leaves everything as it is without -O
    assert outs["bw"][1] == outs["plain"][1]
    assert "gain index" not in outs["plain"][0] + outs["bw"][0] and "overload" not in outs["plain"][0] + outs["bw"][0]
    # the model: every source's buffers in order, each over its own length, settle = the tool's 8 buffers per run
    gains = [0, 9, 14, 27, 37, 77, 87, 125, 144, 157, 166, 197, 207, 229, 254, 280, 297, 328, 338, 364, 372, 386, 402, 421, 434, 439,
             445, 480, 496]
    want_changes, want_flips, want_final = [], [], []
    for s in range(3):
        m = hm.StreamModel(s, len(gains), settle=8)
        ov = 0
        for b in range(NB + 1):
            buf = iq[s, b * L:(b + 1) * L]
            m.feed(hm.records(buf), len(buf))
            if m.overloaded != ov:
                want_flips.append((s, b, "begins" if m.overloaded else "ends"))
                ov = m.overloaded
        want_changes += [(s, e["buffer_serial"], e["old_index"], e["new_index"], gains[e["new_index"]],
                          "overload" if e["overloaded"] else "low level") for e in m.events]
        want_final.append((s, m.index, gains[m.index]))
    err = outs["agc"][0]
    got_changes = [(int(a), int(b), int(c), int(d), int(e), f) for a, b, c, d, e, f in
                   re.findall(r"^stream (\d+): buffer (\d+): gain index (\d+) -> (\d+), gain (\d+) \((overload|low level)\)$", err, re.M)]
    got_flips = [(int(a), int(b), c) for a, b, c in re.findall(r"^stream (\d+): buffer (\d+): overload (begins|ends)$", err, re.M)]
    got_final = [(int(a), int(b), int(c)) for a, b, c in re.findall(r"^stream (\d+): final gain index (\d+), gain (\d+)$", err, re.M)]
    assert want_changes and want_flips
    assert sorted(got_changes) == sorted(want_changes)
    for s in range(3):  # every source's lines in its own order
        assert [c for c in got_changes if c[0] == s] == [c for c in want_changes if c[0] == s]
        assert [f for f in got_flips if f[0] == s] == [f for f in want_flips if f[0] == s]
    assert got_final == want_final
