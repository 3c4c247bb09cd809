"""rtl_fm_hip -N 2 -X ... -E srcdc on file sources with a DC offset: every stream's file equals the library's row of a handle
with the option source_dc on - and the model's (tests/source_dc_model.py) - and differs from the file without -E srcdc."""
import numpy as np
import pytest

import channel_model as cm
import source_dc_model as sdm
from channel_common import assert_rows, demod, run_once, to_device
from channel_fir_model import raw_rows
from rtlsdr_amd.capi import MODE_RAW
from rtlsdr_amd.demod import channel_lowpass
from test_cli_channels_gpu import out_file, plan, run_cli

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fir", [False, True], ids=["boxcar", "fir33"])
def test_files_equal_the_librarys_rows(oracle_lib, tmp_path, fir):
    """-M raw -s 24k -W 4 (2048-byte buffers, /42 at 1 008 000 S/s), two sources of four buffers with offsets of their own,
    two channels each - one of them AT the source's -f, where the spike is."""
    L, K, nb = 2048, 2, 4
    cfg, rate = plan(oracle_lib, 24000, rate_out=24000, block_len=L, mode=MODE_RAW, max_blocks=nb)
    assert rate == 1008000 and cfg.downsample == 42
    f_src = (100000000, 200000000)
    f_chan = ((100000000, 100100000), (199900000, 200000000))
    (tmp_path / "chan.txt").write_text("100M 100.1M\n199.9M 200M\n")
    rng = np.random.default_rng(7)
    data, srcs = [], []
    for i, (oi, oq) in enumerate(((9, -14), (-14, 30))):
        x = rng.integers(-40, 41, size=nb * L).astype(np.int64) + 127
        x[0::2] += oi
        x[1::2] += oq
        data.append(x.astype(np.uint8))
        data[i].tofile(tmp_path / f"in_{i}.bin")
        srcs.append(tmp_path / f"in_{i}.bin")
    argv = ["-N", "2", "-f", "100M", "-f", "200M", "-X", str(tmp_path / "chan.txt"), "-M", "raw", "-s", "24k", "-W", "4"]
    if fir:
        argv += ["-x", "33"]
        taps, shift = channel_lowpass(33, 0.4 / 42, 21)  # (the tool's own fallback: gain 21 at shift 13 - test_cli_channels_gpu.py)
        shift -= 1
    steps = [cm.step_from_hz(f - f_src[i], rate) for i in range(2) for f in f_chan[i]]
    src = np.stack(data)
    files = {}
    for on in (True, False):
        r = run_cli(tmp_path, srcs, argv + (["-E", "srcdc"] if on else []) + [str(tmp_path / "out_%d.raw")])
        assert r.returncode == 0, r.stderr[-2000:]
        files[on] = [out_file(tmp_path, s) for s in range(2 * K)]
    # the library's rows: one handle, one run of all four buffers (the averages go buffer by buffer whatever the runs are)
    with demod(cfg, 2 * K, source_dc=1) as g:
        g.set_channels(K, steps=steps)
        if fir:
            g.set_channel_filter(taps, shift)
        rows, _ = run_once(g, to_device(src), L, 0, nb)
    assert_rows(files[True], rows, "the files against the library's rows")
    if fir:
        want = raw_rows(*sdm.DcFirModel(steps, K, 42, taps, shift, 2).run(src, L))
    else:
        want = sdm.DcBoxModel(steps, K, 42, 2).run(src, L)
    assert_rows(files[True], want, "the files against the model")
    for s in range(2 * K):
        assert files[False][s].shape == files[True][s].shape and not np.array_equal(files[False][s], files[True][s]), s
