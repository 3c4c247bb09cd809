"""rtl_fm_hip -k / -u (keep / take up a channel snapshot, with -X) without a GPU: what they do not go with is refused before
a device is opened - exit status 1 and a sentence that names both letters -, and -u's file is checked against what the
command line plans before a device is opened as well: exit status 2 behind the library's text.  (The source files named
here do not exist: opening one would say "Failed to open rtlsdr device".)"""
import os
import subprocess

import numpy as np
import pytest

from rtlsdr_amd import build as hipbuild
from rtlsdr_amd import capi
from rtlsdr_amd.capi import RtlfmCfg, RtlfmStreamState
from rtlsdr_amd.demod import channel_lowpass, optimal_settings


def cli(argv, tmp_path):
    _, exe = hipbuild.build_host()
    env = {k: v for k, v in os.environ.items() if k not in ("RTLSDR_FILE", "RTLSDR_FILE_LIST")}
    env["RTLSDR_FILE_LIST"] = str(tmp_path / "missing.txt")
    r = subprocess.run([exe] + argv + [str(tmp_path / "out_%d.raw")], env=env, capture_output=True, text=True, timeout=120)
    assert not list(tmp_path.glob("out_*")), "an output file was created"
    return r


def refused(r, status, *words):
    assert r.returncode == status, (r.returncode, r.stderr)
    for w in words:
        assert w in r.stderr, (w, r.stderr)
    for bad in ("Failed to open", "No supported devices", "rtlfm_gpu_create", "hip", "HIP"):
        assert bad not in r.stderr, (bad, r.stderr)


@pytest.fixture
def chan(tmp_path):
    p = tmp_path / "chan.txt"
    p.write_text("100.1M 100.2M\n99.9M 100.3M\n")
    return str(p)


BASE = ["-N", "2", "-f", "100M", "-s", "240k", "-m", "2.2M", "-A", "fast", "-W", "4"]


@pytest.mark.parametrize("letter", ["-k", "-u"])
def test_keep_and_take_up_need_the_channel_file(letter, tmp_path):
    r = cli(BASE + [letter, str(tmp_path / "KEEP")], tmp_path)
    refused(r, 1, letter, "-X", "-K / -R")


@pytest.mark.parametrize("letter", ["-k", "-u"])
@pytest.mark.parametrize("extra, named", [(["-l", "10", "-S", "SCAN"], "-S"), (["-C", "CMD"], "-C"), (["-E", "srcagc"], "-E srcagc")])
def test_engines_with_state_of_their_own(letter, extra, named, tmp_path, chan):
    """(The files they name do not exist either: the refusal comes before they are read.)"""
    r = cli(BASE + ["-X", chan, letter, str(tmp_path / "KEEP")] + [str(tmp_path / e) if e in ("SCAN", "CMD") else e for e in extra], tmp_path)
    refused(r, 1, letter, named, "does not go with", "state of their own")


def planned_cfg(**ov):
    """What BASE plans: -s 240k -m 2.2M -A fast -W 4, /10 at 2.4 MS/s."""
    cfg = RtlfmCfg.default(custom_atan=capi.ATAN_FAST, rate_out=240000, block_len=2048, **ov)
    _, rate = optimal_settings(cfg, 100000000, 240000, 2200000)
    assert rate == 2400000 and cfg.downsample == 10
    cfg.max_blocks = 5  # (whatever the tool takes per run: not compared)
    return cfg


def write_snapshot(path, cfg, nsrc=2, per=2, ntaps=0, source_dc=False, gain=10):
    n = nsrc * per
    taps, shift = channel_lowpass(ntaps, 0.4 / 10, gain) if ntaps else (None, 0)
    capi.chansnap_write(path, cfg, per, 4096, np.arange(n, dtype=np.uint32), (RtlfmStreamState * n)(), fir_taps=taps, fir_shift=shift,
                        hist=np.full((nsrc, 8192), 127, np.uint8) if ntaps else None, source_dc=source_dc)


def test_take_up_checks_the_file_before_a_device_is_opened(tmp_path, chan):
    keep = str(tmp_path / "keep.chn")
    argv = BASE + ["-X", chan, "-x", "33", "-u", keep]
    refused(cli(argv, tmp_path), 2, "-u", keep, "No such file")                                       # missing
    write_snapshot(keep, planned_cfg(), ntaps=33)
    r = cli(argv, tmp_path)                                                                             # the file fits: as far as the device layer
    assert r.returncode == 1 and "No supported devices" in r.stderr and "-u" not in r.stderr, r.stderr
    raw = bytearray(open(keep, "rb").read())
    raw[len(raw) // 2] ^= 4
    open(keep, "wb").write(bytes(raw))
    refused(cli(argv, tmp_path), 2, "-u", capi.strerror(-84))                                           # damaged: -EILSEQ
    write_snapshot(keep, planned_cfg(), per=4, ntaps=33)
    refused(cli(argv, tmp_path), 2, "-u", capi.strerror(-34))                                           # another K: another count, -ERANGE
    write_snapshot(keep, planned_cfg(), nsrc=1, per=4, ntaps=33)
    refused(cli(argv, tmp_path), 2, "-u", capi.strerror(-124))                                          # ... or the same count: -EMEDIUMTYPE
    for kw in (dict(ntaps=31), dict(ntaps=0), dict(ntaps=33, gain=5), dict(ntaps=33, source_dc=True)):
        write_snapshot(keep, planned_cfg(), **kw)
        refused(cli(argv, tmp_path), 2, "-u", capi.strerror(-124))                                      # other taps, no filter, -E srcdc
    write_snapshot(keep, planned_cfg(squelch_level=7), ntaps=33)
    refused(cli(argv, tmp_path), 2, "-u", capi.strerror(-124))                                          # another cfg
    write_snapshot(keep, planned_cfg(), ntaps=33)
    refused(cli(BASE + ["-X", chan, "-u", keep], tmp_path), 2, "-u", capi.strerror(-124))               # the command line without -x
    lib = capi.load()
    assert lib.rtlfm_snapshot_write(os.fsencode(keep), planned_cfg(), 4, (RtlfmStreamState * 4)(), None) == 0
    refused(cli(argv, tmp_path), 2, "-u", capi.strerror(-84))                                           # a -K file
