"""rtl_fm_hip -X with -l: the squelch rule runs on the device (option pack_results 2) and only what it lets through comes
back (rtlfm_gpu_fetch_packed).  The files are demod_thread_fn's rule (src/rtl_fm.c:1366-1370) over each channel's own
buffers by the oracle, and the summary counts the buffers it held.  -A fast: equality of every sample."""
import numpy as np
import pytest

from channel_common import assert_rows
from rtlsdr_amd.capi import ATAN_FAST
from test_cli_channels_gpu import held_back_per_channel, keyed_carriers, out_file, plan, run_cli

pytestmark = pytest.mark.gpu

OFFSETS = (96000, -192000)


def test_two_carriers_with_a_silent_stretch(oracle_lib, tmp_path):
    """-N 1 -X, two channels, -s 24k -A fast -l 100 -t 2 -W 4, 14 buffers of 2048 bytes: the carrier 96 kHz above -f in
    buffers 1 .. 3 and 9 .. 11, the one 192 kHz below in 2 .. 5 and 10 .. 12, nothing in between - both channels close
    in the stretch, are held from the third closed buffer on and open again."""
    L, t, nb = 2048, 2, 14
    cfg, rate = plan(oracle_lib, 24000, rate_out=24000, squelch_level=100, block_len=L, custom_atan=ATAN_FAST)
    assert rate == 1008000
    src = keyed_carriers(nb, L, rate, ((OFFSETS[0], 1, 4), (OFFSETS[0], 9, 12), (OFFSETS[1], 2, 6), (OFFSETS[1], 10, 13)), 17)
    src.tofile(tmp_path / "in.bin")
    (tmp_path / "chan.txt").write_text(" ".join(str(100000000 + off) for off in OFFSETS) + "\n")
    r = run_cli(tmp_path, [tmp_path / "in.bin"], ["-N", "1", "-f", "100M", "-X", str(tmp_path / "chan.txt"), "-s", "24k", "-A", "fast",
                                                 "-l", "100", "-t", str(t), "-W", "4", "-v", str(tmp_path / "out_%d.raw")])
    assert r.returncode == 0, r.stderr[-2000:]
    want = held_back_per_channel(oracle_lib, cfg, rate, src, OFFSETS, L, t)
    total = 0
    for c, (pcm, held) in enumerate(want):
        # held at the start (squelch_hits starts at 11), in the silent stretch and at the end - and open twice
        assert 3 <= held < nb - 4 and pcm.size > 0, (c, held)
        assert f"stream {c}: {pcm.size} samples out, {held} buffers held back" in r.stderr, (c, held, r.stderr[-1500:])
        total += held
    assert_rows([out_file(tmp_path, c) for c in range(2)], [w[0] for w in want], "the files")
    assert f"{nb} buffers in, {sum(w[0].size for w in want)} samples out, {total} buffers held back by the squelch" in r.stderr, r.stderr[-1500:]
