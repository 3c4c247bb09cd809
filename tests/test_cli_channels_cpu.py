"""rtl_fm_hip -X / -x without a GPU: everything the channel option refuses is refused before a device is opened or a
handle created - exit status 1, a sentence that names both options, and neither "Failed to open" nor a GPU error in
stderr.  (The source files named here do not exist: opening one would say "Failed to open rtlsdr device".)"""
import os
import subprocess

import pytest

from rtlsdr_amd import build as hipbuild


def cli(argv, env_extra):
    _, exe = hipbuild.build_host()
    env = {k: v for k, v in os.environ.items() if k not in ("RTLSDR_FILE", "RTLSDR_FILE_LIST")}
    env.update(env_extra)
    return subprocess.run([exe] + argv, env=env, capture_output=True, text=True, timeout=120)


@pytest.fixture
def chan(tmp_path):
    def write(text, name="chan.txt"):
        p = tmp_path / name
        p.write_text(text)
        return str(p)
    return write


def refused(r, *words):
    assert r.returncode == 1, (r.returncode, r.stderr)
    for w in words:
        assert w in r.stderr, (w, r.stderr)
    for bad in ("Failed to open", "No supported devices", "rtlfm_gpu_", "hip", "HIP"):
        assert bad not in r.stderr, (bad, r.stderr)


def run(tmp_path, extra, out="out_%d.raw", n=None, f=("100M",)):
    argv = []
    for x in f:
        argv += ["-f", x]
    if n is not None:
        argv += ["-N", str(n)]
    r = cli(argv + extra + [str(tmp_path / out)], {"RTLSDR_FILE_LIST": str(tmp_path / "missing.txt")})
    assert not list(tmp_path.glob("out_*")), "an output file was created"
    return r


COMBINATIONS = [
    (["-l", "10", "-S", "SCAN"], "-S"),
    (["-C", "CMD"], "-C"),
    (["-K", "KEEP"], "-K"),
    (["-R", "KEEP"], "-R"),
    (["-Z"], "-Z"),
    (["-O", "agc=2"], "-O agc=2"),
    (["-O", "bw=1500:agc=2"], "-O agc=2"),
    (["-E", "rdc"], "-E rdc"),
    (["-F", "9", "-x", "33"], "-F"),
]


@pytest.mark.parametrize("extra, named", COMBINATIONS, ids=[c[1] + str(i) for i, c in enumerate(COMBINATIONS)])
def test_options_that_do_not_go_with_channels(extra, named, tmp_path, chan):
    """Each of them needs what the library refuses while channels are on.  The files they name do not exist either:
    the refusal comes before they are read."""
    x = chan("100.1M 100.2M\n")
    r = run(tmp_path, ["-X", x] + [str(tmp_path / e) if e in ("SCAN", "CMD", "KEEP") else e for e in extra])
    refused(r, "-X", named, "does not go with")


def test_filter_taps_need_the_channel_file(tmp_path):
    r = run(tmp_path, ["-x", "33"], out="out.raw")
    refused(r, "-x", "-X")


@pytest.mark.parametrize("ntaps", ["0", "-3", "1025"])
def test_filter_taps_out_of_range(ntaps, tmp_path, chan):
    r = run(tmp_path, ["-X", chan("100.1M\n"), "-x", ntaps], out="out.raw")
    refused(r, "-x", "-X", "1 .. 1024")


def test_missing_channel_file(tmp_path):
    r = run(tmp_path, ["-X", str(tmp_path / "nothing.txt")])
    refused(r, "-X", "cannot open the channel file")


def test_a_line_that_is_no_list(tmp_path, chan):
    r = run(tmp_path, ["-X", chan("# channels\n100.1M 100.2M\n100.1M:100.3M\n")], n=2)
    refused(r, "-X", "line 3 is no frequency list")


@pytest.mark.parametrize("text, n", [("100.1M 100.2M\n100.1M 100.2M\n", None), ("100.1M 100.2M\n", 2),
                                     ("100.1M\n\n# a comment\n100.2M\n100.3M\n", 2)])
def test_line_count_must_be_the_source_count(text, n, tmp_path, chan):
    r = run(tmp_path, ["-X", chan(text)], n=n)
    refused(r, "-X", "-N %d needs exactly %d" % (n or 1, n or 1), "holds %d lists" % (len([ln for ln in text.split("\n") if ln and ln[0] != "#"])))


def test_every_line_the_same_number_of_channels(tmp_path, chan):
    r = run(tmp_path, ["-X", chan("100.1M 100.2M\n# ranges count by their entries\n100.0M:100.2M:100k\n")], n=2)
    refused(r, "-X", "line 3 stands for 3 channels and line 1 for 2")


def test_a_range_counts_as_its_entries(tmp_path, chan):
    """Two lines of three channels each, one of them a range: accepted - the run gets as far as the device layer."""
    r = run(tmp_path, ["-X", chan("100.0M:100.2M:100k\n99.9M, 100M\t100.1M\n")], n=2)
    assert r.returncode == 1 and "No supported devices" in r.stderr and "-X" not in r.stderr


def test_filename_needs_one_stream_index(tmp_path, chan):
    x = chan("100.1M 100.2M\n")
    refused(run(tmp_path, ["-X", x], out="out.raw"), "-X", "exactly one %d")
    refused(run(tmp_path, ["-X", x], out="out_%d_%d.raw"), "-X", "exactly one %d")
    r = cli(["-f", "100M", "-X", x, "-"], {"RTLSDR_FILE_LIST": str(tmp_path / "missing.txt")})
    refused(r, "-X", "%d")
    # one source, one channel: the name as it is
    r = run(tmp_path, ["-X", chan("100.1M\n", "one.txt")], out="single.raw")
    assert r.returncode == 1 and "No supported devices" in r.stderr and "-X" not in r.stderr
    assert not (tmp_path / "single.raw").exists()


def test_number_of_frequencies(tmp_path, chan):
    r = run(tmp_path, ["-X", chan("100.1M\n100.2M\n100.3M\n")], n=3, f=("100M", "100.1M"))
    refused(r, "-X", "-f once", "not 2 times")


@pytest.mark.parametrize("extra, half", [(["-s", "24k"], 504000), (["-M", "wbfm"], 510000)], ids=["fm24k", "wbfm"])
def test_channel_outside_the_capture_is_refused_with_line_and_entry(extra, half, tmp_path, chan):
    """-s 24k under -m 1M: 42 x 24 000 = 1 008 000 S/s; -M wbfm: 6 x 170 000 = 1 020 000 S/s.  The distance counts from -f
    as given - -M wbfm's 16 kHz are not added, or 200M + half + 1 kHz would be inside."""
    x = chan(f"100.1M {100000000 + half}\n# the second source\n200M {200000000 + half + 1000}\n")
    ok = chan(f"100.1M {100000000 + half}\n200M {200000000 - half}\n", "ok.txt")
    r = run(tmp_path, ["-X", x] + extra, n=2, f=("100M", "200M"))
    refused(r, "-X", "line 3, entry 2", f"{200000000 + half + 1000} Hz", f"capture_rate / 2 = {half} Hz", "source 1, 200000000 Hz")
    r = run(tmp_path, ["-X", ok] + extra, n=2, f=("100M", "200M"))
    assert r.returncode == 1 and "No supported devices" in r.stderr and "capture_rate / 2" not in r.stderr
