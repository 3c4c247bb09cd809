"""rtl_power_hip -N n: n devices (RTLSDR_FILE_LIST) scan one -f plan as n x hops streams of one handle, reported by
rtlpower_gpu_report.  Every source's CSV file - the two timestamp fields aside - must be, byte for byte, what the
unchanged single-device program writes for that source alone (rtlpower_gpu_scan / _fetch / rtlpower_csv_dbm / _clear)."""
import os
import subprocess

import numpy as np
import pytest

from rtlsdr_amd import build as hipbuild
from rtlsdr_amd import synth

pytestmark = pytest.mark.gpu

PLANS = [
    # a range below 1 MHz: one hop, decimated by fifth_order passes and the compensating FIR (-F 9)
    (["-f", "433M:433.5M:1k", "-F", "9", "-w", "hamming"], 1, 16384),
    # four hops, cropped, peak hold
    (["-f", "88M:96M:10k", "-c", "20%", "-w", "blackman", "-P"], 4, 16384),
]


def _cli():
    hipbuild.build()
    hipbuild.build_host()
    return hipbuild.POWER_CLI_OUT


def _strip(text):
    """Lines without main()'s "date, time, " prefix (src/rtl_power.c:996-998)."""
    out = []
    for ln in text.splitlines(keepends=True):
        parts = ln.split(b", ", 2)
        assert len(parts) == 3 and len(parts[0]) == 10 and len(parts[1]) == 8, ln[:60]
        out.append(parts[2])
    return out


@pytest.mark.parametrize("argv,hops,buf_len", PLANS, ids=["decimated", "multihop"])
def test_six_sources_each_match_the_single_source_program(tmp_path, argv, hops, buf_len):
    n, passes, reports = 6, 3, 2
    cli = _cli()
    whole = buf_len * hops * passes * reports
    iq = np.concatenate([synth.fm_iq_u8(4, (whole + buf_len) // 2, fs=2.0e6, dev_hz=40e3, seed=61),
                         synth.random_u8(2, whole + buf_len, seed=62)])
    srcs = []
    for i in range(n):
        p = tmp_path / f"in_{i}.bin"
        iq[i, :whole + 100 + 333 * i].tofile(p)  # two reports' worth and a part of a buffer
        srcs.append(p)
    env = {k: v for k, v in os.environ.items() if k not in ("RTLSDR_FILE", "RTLSDR_FILE_LIST")}
    env["RTLPOWER_PASSES"] = str(passes)
    lst = tmp_path / "sources.txt"
    lst.write_text("\n".join(str(s) for s in srcs) + "\n")
    r = subprocess.run([cli, "-N", str(n)] + argv + [str(tmp_path / "out_%d.csv")], env=dict(env, RTLSDR_FILE_LIST=str(lst)),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    assert f"Number of frequency hops: {hops}\n" in r.stderr and f"{n} sources x {hops} hops" in r.stderr, r.stderr[-1500:]
    stamps = set()
    for i in range(n):
        one = subprocess.run([cli] + argv + [str(tmp_path / f"single_{i}.csv")], env=dict(env, RTLSDR_FILE=str(srcs[i])),
                             capture_output=True, text=True, timeout=600)
        assert one.returncode == 0, one.stderr[-1500:]
        want = (tmp_path / f"single_{i}.csv").read_bytes()
        got = (tmp_path / f"out_{i}.csv").read_bytes()
        assert len(_strip(want)) == hops * reports, (i, one.stderr[-800:])
        assert _strip(got) == _strip(want), i
        stamps.add(tuple(ln[:20] for ln in got.splitlines()))
    assert len(stamps) == 1  # every source of a report carries the same timestamp
    assert len({(tmp_path / f"out_{i}.csv").read_bytes() for i in range(n)}) == n  # six different sources


def test_fewer_devices_than_sources_is_refused(tmp_path):
    src = tmp_path / "a.bin"
    synth.random_u8(1, 16384 * 3, seed=1)[0].tofile(src)
    lst = tmp_path / "sources.txt"
    lst.write_text(f"{src}\n")
    env = {k: v for k, v in os.environ.items() if k != "RTLSDR_FILE"}
    r = subprocess.run([_cli(), "-N", "2", "-f", "88M:90M:10k", str(tmp_path / "o_%d.csv")], env=dict(env, RTLSDR_FILE_LIST=str(lst)),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "needs devices 0 .. 1" in r.stderr


def test_full_crop_is_refused_under_n(tmp_path):
    """-c 100% leaves no bin: rtlpower_gpu_report takes crop < 1, so -N says so instead of failing at the first report."""
    r = subprocess.run([_cli(), "-N", "2", "-f", "88M:90M:10k", "-c", "100%", str(tmp_path / "o_%d.csv")],
                       env={k: v for k, v in os.environ.items() if k not in ("RTLSDR_FILE", "RTLSDR_FILE_LIST")},
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "use -c below 1" in r.stderr, r.stderr[-500:]
