"""rtl_fm_hip -E srcagc without a GPU: what it does not go with is refused before a device is opened or a handle created -
exit status 1, a sentence that names both sides, and neither "Failed to open" nor a GPU error in stderr - and the usage
text names it.  (The source files named here do not exist: opening one would say so.)"""
import os
import subprocess

import pytest

from rtlsdr_amd import build as hipbuild


def cli(argv, tmp_path):
    _, exe = hipbuild.build_host()
    env = {k: v for k, v in os.environ.items() if k not in ("RTLSDR_FILE", "RTLSDR_FILE_LIST")}
    env["RTLSDR_FILE_LIST"] = str(tmp_path / "missing.txt")
    r = subprocess.run([exe] + argv, env=env, capture_output=True, text=True, timeout=120)
    assert not list(tmp_path.glob("out*")), "an output file was created"
    return r


def refused(r, *words):
    assert r.returncode == 1, (r.returncode, r.stderr)
    for w in words:
        assert w in r.stderr, (w, r.stderr)
    for bad in ("Failed to open", "No supported devices", "rtlfm_gpu_", "hip", "HIP"):
        assert bad not in r.stderr, (bad, r.stderr)


@pytest.fixture
def chan(tmp_path):
    p = tmp_path / "chan.txt"
    p.write_text("100.1M 100.2M\n")
    return str(p)


@pytest.mark.parametrize("extra", [[], ["-N", "2"], ["-N", "2", "-O", "agc=2"]], ids=["single", "N2", "N2-agc2"])
def test_srcagc_needs_the_channel_file(extra, tmp_path):
    name = "out_%d.raw" if extra else "out.raw"
    refused(cli(["-f", "100M", "-E", "srcagc"] + extra + [str(tmp_path / name)], tmp_path), "-E srcagc", "-X", "needs")


@pytest.mark.parametrize("opts, named", [("agc=0", "agc=0"), ("agc=1", "agc=1"), ("bw=1500:agc=1", "agc=1"), ("agc=1:agc=0", "agc=0")])
def test_srcagc_does_not_go_with_an_agc_part_in_the_driver_options(opts, named, tmp_path, chan):
    """Whichever order the two come in.  (agc=2 with -X is refused as ever, by -X's own sentence: tests/test_cli_channels_cpu.py.)"""
    for argv in (["-E", "srcagc", "-O", opts], ["-O", opts, "-E", "srcagc"]):
        r = cli(["-f", "100M", "-X", chan] + argv + [str(tmp_path / "out_%d.raw")], tmp_path)
        refused(r, "-E srcagc", named, "-O", "does not go with")


def test_agc_2_with_channels_stays_refused_as_it_is(tmp_path, chan):
    r = cli(["-f", "100M", "-X", chan, "-O", "agc=2", str(tmp_path / "out_%d.raw")], tmp_path)
    refused(r, "-X", "-O agc=2", "does not go with", "input_health")
    assert "srcagc" not in r.stderr


def test_a_driver_string_without_agc_goes_with_srcagc(tmp_path, chan):
    """Accepted: the run gets as far as the device layer."""
    r = cli(["-f", "100M", "-X", chan, "-E", "srcagc", "-O", "bw=1500", str(tmp_path / "out_%d.raw")], tmp_path)
    assert r.returncode == 1 and "No supported devices" in r.stderr and "srcagc" not in r.stderr


def test_usage_names_srcagc(tmp_path):
    r = cli(["-h"], tmp_path)
    assert "srcagc" in r.stderr and "-X" in r.stderr
    line = [ln for ln in r.stderr.splitlines() if "[-E enable_option]" in ln]
    assert line and "srcagc" in line[0]
