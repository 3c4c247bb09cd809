"""rtl_fm_hip -N 2 -X ... -E srciq -v: every output file equals, byte for byte, the Python loop over the same runs -
GpuDemod with the option source_iq and IqBalance: run, update, poll, set_source_iq - and the printed coefficient lines are
the engine's events.  -l 1 makes every run one buffer (the tool's rule for -l), so the runs are known: the coefficients of
a window rule from the buffer behind it.  Source 0 has a gain and phase mismatch that changes half way, source 1 is
balanced and ends earlier (it is fed bytes 127 from there on: weak windows, which change nothing)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import channel_model as cm
import source_iq_model as model
from rtlsdr_amd import build as hipbuild
from rtlsdr_amd import capi
from rtlsdr_amd.capi import RtlfmCfg

pytestmark = pytest.mark.gpu


def test_srciq_equals_the_python_loop(oracle_lib, tmp_path):
    from rtlsdr_amd.demod import GpuDemod
    from rtlsdr_amd.iq import IqBalance
    _, cli = hipbuild.build_host()
    L, K, NB = 16384, 2, (50, 20)
    cfg = RtlfmCfg.default(rate_out=24000, squelch_level=1)
    cf, cr = C.c_uint32(), C.c_uint32()
    oracle_lib.oracle().orc_optimal_settings(C.byref(cfg), 100000000, 24000, 1000000, 0, 0, C.byref(cf), C.byref(cr))
    rate = cr.value
    half = NB[0] // 2 * L // 2
    data = [np.concatenate([model.image_signal(n=half, g=0.8, phi_deg=10.0, seed=5), model.image_signal(n=half, g=1.2, phi_deg=-6.0, seed=6)]),
            model.image_signal(n=NB[1] * L // 2, g=1.0, phi_deg=0.0, seed=7)]
    srcs = []
    for i in range(2):
        p = tmp_path / f"in_{i}.bin"
        data[i].tofile(p)
        srcs.append(str(p))
    (tmp_path / "sources.txt").write_text("\n".join(srcs) + "\n")
    off = round(37 / 256 * rate)
    f_chan = (100000000 + off, 100000000 - off)
    (tmp_path / "chan.txt").write_text(f"{f_chan[0]} {f_chan[1]}\n{f_chan[0]} {f_chan[1]}\n")
    env = {k: v for k, v in os.environ.items() if k != "RTLSDR_FILE"}
    env["RTLSDR_FILE_LIST"] = str(tmp_path / "sources.txt")
    r = subprocess.run(["timeout", "-k", "10", "120", cli, "-N", "2", "-f", "100M", "-X", str(tmp_path / "chan.txt"), "-s", "24k", "-l", "1", "-v",
                        "-E", "srciq", str(tmp_path / "out_%d.raw")], env=env, capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, r.stderr[-3000:]
    # the Python loop: one buffer per run, an ended source fed bytes 127
    steps = [cm.step_from_hz(f - 100000000, rate) for f in f_chan] * 2
    outs = [[] for _ in range(2 * K)]
    events = []
    silence = np.full(L, 127, dtype=np.uint8)
    with GpuDemod(cm.copy_cfg(cfg, max_blocks=1), 2 * K, options=dict(source_ring=1), source_iq=True) as g, IqBalance(2) as e:
        g.set_channels(K, steps=steps)
        for b in range(max(NB)):
            for i in range(2):
                g.rtlsdr_callback(data[i][b * L:(b + 1) * L] if b < NB[i] else silence, stream=i)
            g.full_demod()
            o, n = g.fetch_all()
            for s in range(2 * K):
                if b < NB[s // K]:
                    outs[s].append(o[s, :n[s]].copy())
            e.update(g)
            ev = e.poll()
            events += ev
            if any(x["kind"] == capi.IQ_EVENT_CHANGED for x in ev):
                g.set_source_iq(e.coeffs())
        final = e.coeffs().tolist()
    for s in range(2 * K):
        want = np.concatenate(outs[s])
        got = np.fromfile(tmp_path / f"out_{s}.raw", dtype=np.int16)
        assert got.size == want.size and np.array_equal(got, want), (s, got.size, want.size)
    changed = [(x["source"],) + tuple(x["coef"]) for x in events if x["kind"] == capi.IQ_EVENT_CHANGED]
    rejected = [(x["source"], x["g_q14"], x["s_q14"]) for x in events if x["kind"] == capi.IQ_EVENT_REJECTED]
    got_changed = [tuple(int(v) for v in m) for m in re.findall(r"^source (\d+): iq (-?\d+) (-?\d+) (-?\d+) (-?\d+)$", r.stderr, re.M)]
    got_rejected = [tuple(int(v) for v in m) for m in re.findall(r"^source (\d+): iq rejected (-?\d+) (-?\d+)$", r.stderr, re.M)]
    got_final = [[int(v) for v in m[1:]] for m in re.findall(r"^source (\d+): iq (-?\d+) (-?\d+) (-?\d+) (-?\d+) at exit$", r.stderr, re.M)]
    assert len(changed) >= 2 and all(c[0] == 0 for c in changed), changed  # source 0 twice at least, the balanced source never
    assert got_changed == changed and got_rejected == rejected
    assert got_final == final and final[1] == list(model.IDENTITY) and final[0] != list(model.IDENTITY)
