"""rtl_fm_hip -N 3 -X ... -E srcagc -v on three files of different loudness and length: the printed gain changes, overload
flips and final indices equal tests/health_model.py fed as the tool feeds its engine - every live source's buffers in
order, a short last buffer completed with bytes 127 and counted at the full length, nothing for a source that has ended -
and every output file is byte-identical to the run without -E srcagc."""
import os
import re
import subprocess

import numpy as np
import pytest

import health_model as hm
from rtlsdr_amd import build as hipbuild
from test_source_health_gpu import loudness_sources

pytestmark = pytest.mark.gpu

# the file-backed device layer's gain table (tenths of a dB), as tests/test_agc_gpu.py has it
GAINS = [0, 9, 14, 27, 37, 77, 87, 125, 144, 157, 166, 197, 207, 229, 254, 280, 297, 328, 338, 364, 372, 386, 402, 421, 434, 439,
         445, 480, 496]


def test_srcagc_against_the_model_and_the_plain_run(tmp_path):
    _, cli = hipbuild.build_host()
    L, NB, K = 16384, 21, 2  # the tool's default buffer; 21 buffers: runs of up to 8
    iq = loudness_sources(L, NB)[[0, 2, 3]]  # quiet, clipped, alternating
    # source 0 ends with a short buffer of 1536 bytes, source 1 - the clipped one - eight buffers earlier, source 2 on a whole buffer
    data = [np.concatenate([iq[0], iq[0, :1536]]), iq[1, :(NB - 8) * L].copy(), iq[2].copy()]
    srcs = []
    for s in range(3):
        p = tmp_path / f"in_{s}.bin"
        data[s].tofile(p)
        srcs.append(str(p))
    (tmp_path / "sources.txt").write_text("\n".join(srcs) + "\n")
    (tmp_path / "chan.txt").write_text("100.1M 99.9M\n100.1M 99.9M\n100.1M 99.9M\n")
    env = {k: v for k, v in os.environ.items() if k != "RTLSDR_FILE"}
    env["RTLSDR_FILE_LIST"] = str(tmp_path / "sources.txt")
    outs = {}
    for key, extra in (("plain", []), ("agc", ["-E", "srcagc"])):
        d = tmp_path / key
        d.mkdir()
        r = subprocess.run(["timeout", "-k", "10", "120", cli, "-N", "3", "-f", "100M", "-X", str(tmp_path / "chan.txt"), "-s", "24k", "-v"]
                           + extra + [str(d / "out_%d.raw")], env=env, capture_output=True, text=True, timeout=150)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[key] = (r.stderr, [(d / f"out_{s}.raw").read_bytes() for s in range(3 * K)])
    assert outs["plain"][1] == outs["agc"][1] and all(len(b) > 0 for b in outs["plain"][1])
    assert "gain index" not in outs["plain"][0] and "overload" not in outs["plain"][0]
    # the model: settle = the tool's 8 buffers per run
    want_changes, want_flips, want_final = [], [], []
    for s in range(3):
        m = hm.StreamModel(s, len(GAINS), settle=8)
        ov = 0
        nbuf = (data[s].size + L - 1) // L
        for b in range(nbuf):
            buf = np.full(L, 127, dtype=np.uint8)
            piece = data[s][b * L:(b + 1) * L]
            buf[:piece.size] = piece
            m.feed(hm.records(buf), L)
            if m.overloaded != ov:
                want_flips.append((s, b, "begins" if m.overloaded else "ends"))
                ov = m.overloaded
        assert m.total_samples == nbuf * L
        want_changes += [(s, e["buffer_serial"], e["old_index"], e["new_index"], GAINS[e["new_index"]],
                          "overload" if e["overloaded"] else "low level") for e in m.events]
        want_final.append((s, m.index, GAINS[m.index]))
    err = outs["agc"][0]
    got_changes = [(int(a), int(b), int(c), int(d), int(e), f) for a, b, c, d, e, f in
                   re.findall(r"^source (\d+): buffer (\d+): gain index (\d+) -> (\d+), gain (\d+) \((overload|low level)\)$", err, re.M)]
    got_flips = [(int(a), int(b), c) for a, b, c in re.findall(r"^source (\d+): buffer (\d+): overload (begins|ends)$", err, re.M)]
    got_final = [(int(a), int(b), int(c)) for a, b, c in re.findall(r"^source (\d+): final gain index (\d+), gain (\d+)$", err, re.M)]
    assert want_changes and want_flips
    assert sorted(got_changes) == sorted(want_changes)
    for s in range(3):  # every source's lines in its own order
        assert [c for c in got_changes if c[0] == s] == [c for c in want_changes if c[0] == s]
        assert [f for f in got_flips if f[0] == s] == [f for f in want_flips if f[0] == s]
    assert got_final == want_final
    assert not re.search(r"^stream \d+: (buffer|final gain)", err, re.M)  # (under -X a stream is a channel)
