"""rtl_fm_hip -K / -R: stop and go on without a click.  The PCM of "the first k buffers with -K st" followed by "the last k
buffers with -R st" must be byte for byte the PCM of the whole capture in one go - for one source and for -N 3, where a
source that leaves the batch early contributes the record it had when it left.  GPU against GPU, so every case is exact."""
import os
import re
import subprocess

import numpy as np
import pytest

import scan_model as sm
from rtlsdr_amd import build as hipbuild
from rtlsdr_amd import capi, synth

pytestmark = pytest.mark.gpu

L, K = 2048, 10
# four fifth_order passes (-m 1.4M over 170 kHz: /16), generic_fir, deemph, low_pass_real 170000 -> 32000
FIFTH4 = ["-M", "wbfm", "-F", "9", "-m", "1.4M", "-W", "4"]
# a boxcar of 7 (1 MHz over 150 kHz), which does not divide the buffer, dc_block_raw, dc_block_audio, the squelch on the
# device's gate: squelch_hits is carried across the stop
BOX7 = ["-M", "fm", "-s", "150k", "-A", "fast", "-E", "rdc", "-E", "dc", "-l", "60", "-t", "5", "-W", "4"]
# the squelch behind a resampler has no device gate: the tool's own rule over rtlfm_gpu_state_get_all / _set_all
FIFTH4_SQ = FIFTH4 + ["-l", "60", "-t", "5"]
# the squelch is open, then closed for four buffers at the stop (at most 4 hits <= 5: all still emitted); the second half
# opens with five more quiet buffers, of which the CARRIED count holds the last ones - a fresh start (11 hits) holds all five
PATTERN = "LLLLLLqqqq" + "qqqqqLLLqq"
CASES = {"fifth4_fir_deemph_lpr": FIFTH4, "box7_rdc_adc_sq": BOX7, "fifth4_squelch_no_gate": FIFTH4_SQ}


def capture(name, seed, nbuf=2 * K):
    if name == "fifth4_fir_deemph_lpr":
        return synth.fm_iq_u8(1, L // 2 * nbuf, fs=2.72e6, dev_hz=5e3, amplitude=30.0, seed=seed)[0]
    rng = np.random.default_rng(seed)
    return np.concatenate([sm.tone_or_noise(rng, L, PATTERN[b % len(PATTERN)] == "L") for b in range(nbuf)])


def cli(argv, env_extra, timeout=300):
    _, exe = hipbuild.build_host()
    env = {k: v for k, v in os.environ.items() if k not in ("RTLSDR_FILE", "RTLSDR_FILE_LIST")}
    env.update(env_extra)
    return subprocess.run([exe, "-f", "100M"] + argv, env=env, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("name", list(CASES))
def test_one_source_stops_and_goes_on(tmp_path, name):
    iq = capture(name, 5)
    parts = {"whole": iq, "first": iq[:K * L], "last": iq[K * L:]}
    for k, v in parts.items():
        v.tofile(tmp_path / f"{k}.bin")
    st = tmp_path / "st.snap"
    extra = {"whole": [], "first": ["-K", str(st)], "last": ["-R", str(st)]}
    pcm, held = {}, {}
    for k in parts:
        r = cli(CASES[name] + extra[k] + [str(tmp_path / f"{k}.raw")], {"RTLSDR_FILE": str(tmp_path / f"{k}.bin")})
        assert r.returncode == 0, (k, r.stderr[-1500:])
        assert f"{len(parts[k]) // L} buffers in" in r.stderr, (k, r.stderr[-400:])
        pcm[k] = (tmp_path / f"{k}.raw").read_bytes()
        held[k] = int(re.search(r"(\d+) buffers held back", r.stderr).group(1))
    assert capi.snapshot_info(st)[1] == 1
    assert len(pcm["first"]) > 0 and len(pcm["last"]) > 0
    assert pcm["first"] + pcm["last"] == pcm["whole"]
    assert held["first"] + held["last"] == held["whole"] and (held["last"] > 0) == ("-l" in CASES[name]), held
    # ... and the carried state is what made it so: the second half from a fresh start is another file
    r = cli(CASES[name] + [str(tmp_path / "cold.raw")], {"RTLSDR_FILE": str(tmp_path / "last.bin")})
    assert r.returncode == 0 and (tmp_path / "cold.raw").read_bytes() != pcm["last"]


@pytest.mark.parametrize("name,short", [("box7_rdc_adc_sq", None), ("fifth4_fir_deemph_lpr", 1)],
                         ids=["equal_lengths", "one_source_a_buffer_shorter"])
def test_three_sources_stop_and_go_on(tmp_path, name, short):
    """-N 3.  `short`: that source's first half is one buffer shorter, so it leaves the batch before the stop (the others
    move to a smaller handle) and its record in the file is the one it had when it left."""
    n = 3
    lists = {}
    for part in ("whole", "first", "last"):
        (tmp_path / part).mkdir()
        srcs = []
        for i in range(n):
            iq = capture(name, 20 + i)
            k_first = K - 1 if i == short else K
            first, last = iq[:k_first * L], iq[K * L:]
            x = {"whole": np.concatenate([first, last]), "first": first, "last": last}[part]
            p = tmp_path / part / f"in_{i}.bin"
            x.tofile(p)
            srcs.append(str(p))
        lists[part] = tmp_path / part / "sources.txt"
        lists[part].write_text("\n".join(srcs) + "\n")
    st = tmp_path / "st.snap"
    extra = {"whole": [], "first": ["-K", str(st)], "last": ["-R", str(st)]}
    for part in lists:
        r = cli(["-N", str(n), "-v"] + CASES[name] + extra[part] + [str(tmp_path / part / "out_%d.raw")],
                {"RTLSDR_FILE_LIST": str(lists[part])})
        assert r.returncode == 0, (part, r.stderr[-1500:])
        if short is not None and part != "last":
            assert "2 of 3 streams go on" in r.stderr, (part, r.stderr[-600:])
    assert capi.snapshot_info(st)[1] == n
    for i in range(n):
        whole = (tmp_path / "whole" / f"out_{i}.raw").read_bytes()
        first = (tmp_path / "first" / f"out_{i}.raw").read_bytes()
        last = (tmp_path / "last" / f"out_{i}.raw").read_bytes()
        assert len(first) > 0 and len(last) > 0 and first + last == whole, i


def test_refusals_write_nothing(tmp_path):
    """A snapshot of one source under BOX7; then everything -R and -K must refuse - with NO source configured, so that
    whatever is refused is refused before a device is looked for."""
    iq = capture("box7_rdc_adc_sq", 9, K)
    iq.tofile(tmp_path / "in.bin")
    st = tmp_path / "st.snap"
    r = cli(BOX7 + ["-K", str(st), str(tmp_path / "first.raw")], {"RTLSDR_FILE": str(tmp_path / "in.bin")})
    assert r.returncode == 0, r.stderr[-1500:]
    out1, outn = str(tmp_path / "refused.raw"), str(tmp_path / "refused_%d.raw")

    def refused(argv, text, status=2):
        r = cli(argv, {})
        assert r.returncode == status if status else r.returncode != 0, (argv, r.returncode, r.stderr[-600:])
        assert text in r.stderr and "No supported devices" not in r.stderr, (argv, r.stderr[-600:])
    refused(["-N", "3"] + BOX7 + ["-R", str(st), outn], capi.strerror(-34))                      # another n: -ERANGE
    other_rate = [a if a != "150k" else "140k" for a in BOX7]
    refused(other_rate + ["-R", str(st), out1], capi.strerror(-124))                             # another -s: -EMEDIUMTYPE
    b = bytearray(st.read_bytes())
    b[40] ^= 1
    bad = tmp_path / "bad.snap"
    bad.write_bytes(bytes(b))
    refused(BOX7 + ["-R", str(bad), out1], capi.strerror(-84))                                   # damaged: -EILSEQ
    refused(BOX7 + ["-R", str(tmp_path / "missing.snap"), out1], "No such file")
    scan = tmp_path / "lists.txt"
    scan.write_text("100M 101M\n")
    refused(BOX7 + ["-S", str(scan), "-K", str(tmp_path / "k.snap"), out1], "do not go with -S", status=None)
    refused(BOX7 + ["-O", "agc=2", "-R", str(st), out1], "do not go with -S", status=None)
    assert not list(tmp_path.glob("refused*")) and not (tmp_path / "k.snap").exists()
    # the same file and the same command line are accepted (now with a source)
    r = cli(BOX7 + ["-R", str(st), str(tmp_path / "second.raw")], {"RTLSDR_FILE": str(tmp_path / "in.bin")})
    assert r.returncode == 0, r.stderr[-1500:]
