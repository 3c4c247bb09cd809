"""rtl_fm_hip -E srciq without a GPU: what it does not go with is refused before a device is opened or a handle created -
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


@pytest.mark.parametrize("extra", [[], ["-N", "2"]], ids=["single", "N2"])
def test_srciq_needs_the_channel_file(extra, tmp_path):
    name = "out_%d.raw" if extra else "out.raw"
    refused(cli(["-f", "100M", "-E", "srciq"] + extra + [str(tmp_path / name)], tmp_path), "-E srciq", "-X", "needs")


@pytest.mark.parametrize("letter", ["-k", "-u"])
def test_srciq_does_not_go_with_keep_or_take_up(letter, tmp_path, chan):
    """For the reason -E srcagc is refused there: the engine carries state of its own that the channel snapshot does not hold."""
    for argv in (["-E", "srciq", letter, str(tmp_path / "snap.bin")], [letter, str(tmp_path / "snap.bin"), "-E", "srciq"]):
        r = cli(["-f", "100M", "-X", chan] + argv + [str(tmp_path / "out_%d.raw")], tmp_path)
        refused(r, "-E srciq", letter, "does not go with")
    assert not (tmp_path / "snap.bin").exists()


def test_srciq_with_the_channel_file_is_accepted(tmp_path, chan):
    """Accepted: the run gets as far as the device layer."""
    r = cli(["-f", "100M", "-X", chan, "-E", "srciq", str(tmp_path / "out_%d.raw")], tmp_path)
    assert r.returncode == 1 and "No supported devices" in r.stderr and "srciq" not in r.stderr


def test_usage_names_srciq(tmp_path):
    r = cli(["-h"], tmp_path)
    assert "srciq" in r.stderr and "-X" in r.stderr
    block = r.stderr[r.stderr.index("[-E enable_option]"):]
    assert "srciq (with -X only)" in block[:400]
