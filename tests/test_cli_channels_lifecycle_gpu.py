"""rtl_fm_hip -X with -k / -u: the first half of two captures with -k KEEP, the second half with -u KEEP - every out_%d.raw of
the two runs, one behind the other, is that of one run over the whole captures, byte for byte.  Cut at a buffer boundary."""
import os
import subprocess

import numpy as np
import pytest

from channel_common import bounded
from rtlsdr_amd import build as hipbuild

pytestmark = pytest.mark.gpu

L, NB, CUT, K = 2048, 9, 4, 2   # 1024 samples a buffer at /10: 102.4 outputs, prev_index is not 0 at the cut


def run_cli(tmp_path, sources, argv, outdir):
    _, cli = hipbuild.build_host()
    outdir.mkdir()
    lst = outdir / "sources.txt"
    lst.write_text("\n".join(str(s) for s in sources) + "\n")
    env = {k: v for k, v in os.environ.items() if k != "RTLSDR_FILE"}
    env["RTLSDR_FILE_LIST"] = str(lst)
    r = subprocess.run([cli] + argv + [str(outdir / "out_%d.raw")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return [np.fromfile(outdir / f"out_{s}.raw", dtype=np.int16) for s in range(2 * K)]


@pytest.mark.parametrize("extra", [["-x", "33"], [], ["-E", "srcdc"], ["-x", "33", "-E", "srcdc"]], ids=["fir33", "boxcar", "boxcar_srcdc", "fir33_srcdc"])
def test_first_half_kept_second_half_taken_up(tmp_path, extra):
    (tmp_path / "chan.txt").write_text("100.2M 99.85M\n100.1M 100.4M\n")
    parts = {"whole": [], "first": [], "second": []}
    for i in range(2):
        x = (bounded(1, NB * L, 60 + i, 70)[0].astype(np.int16) + (11 if i else -6)).astype(np.uint8)
        for name, piece in (("whole", x), ("first", x[:CUT * L]), ("second", x[CUT * L:])):
            p = tmp_path / f"{name}_{i}.bin"
            piece.tofile(p)
            parts[name].append(p)
    argv = ["-N", "2", "-f", "100M", "-X", str(tmp_path / "chan.txt"), "-s", "240k", "-m", "2.2M", "-A", "fast", "-W", "4"] + extra
    keep = str(tmp_path / "KEEP")
    whole = run_cli(tmp_path, parts["whole"], argv, tmp_path / "w")
    first = run_cli(tmp_path, parts["first"], argv + ["-k", keep], tmp_path / "a")
    assert os.path.exists(keep) and open(keep, "rb").read(8) == b"RTLFMCHN"
    second = run_cli(tmp_path, parts["second"], argv + ["-u", keep], tmp_path / "b")
    for s in range(2 * K):
        assert whole[s].size == NB * (L // 2) // 10
        assert first[s].size == CUT * (L // 2) // 10 and np.array_equal(np.concatenate((first[s], second[s])), whole[s]), s
    # and without -u the second half is another one: the file is what made the difference
    cold = run_cli(tmp_path, parts["second"], argv, tmp_path / "c")
    assert any(not np.array_equal(cold[s], second[s]) for s in range(2 * K))
