"""rtl_power on input rows of any placement (include/rtlpower_hip.h, rtlpower_gpu_scan_device): the library accepts any
pointer and any stride that holds the reads, and chooses its kernels by alignment - the fast families where pointer and
stride are multiples of 16, the general (or staged) kernels elsewhere.  One configuration per transform family, the rows
from tests/row_geometry.py: avg[] and samples against the oracle, last_kernel, nothing read from around the rows, and a
scan split over two calls."""
import numpy as np
import pytest

import row_geometry as rg
from rtlsdr_amd import synth
from rtlsdr_amd.capi import RtlpowerCfg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GENERAL, BIG, FRAMES, DECIMATED, STAGED, STAGED_FAST = 1, 2, 3, 4, 5, 6   # enum rtlpower_kernel

# id -> (configuration, the family on 16-byte aligned rows, the family elsewhere, reads, streams)
# (A read of 16384 bytes is 8192 points, so with 32 bins, too, k_power_scan_frames is what aligned rows get; the general
# in-LDS kernel takes aligned rows where "scan_frames" is 0 - the same configuration once more, see OPTIONS.)
CONFIGS = {
    "frames_e5": (dict(bin_e=5, window=7, buf_len=16384), FRAMES, GENERAL, 5, 3),
    "general_e5": (dict(bin_e=5, window=7, buf_len=16384), GENERAL, GENERAL, 5, 3),
    "frames_e10": (dict(bin_e=10, window=2, buf_len=16384), FRAMES, GENERAL, 5, 3),
    "big_e13": (dict(bin_e=13, window=1, buf_len=16384), BIG, GENERAL, 5, 3),
    "big_e14": (dict(bin_e=14, window=1, buf_len=32768), BIG, GENERAL, 5, 3),
    "dec_fifth_e9": (dict(bin_e=9, window=3, downsample=4, downsample_passes=2, boxcar=0, comp_fir_size=9, buf_len=16384),
                     DECIMATED, GENERAL, 5, 3),
    "dec_boxcar_e9": (dict(bin_e=9, window=4, downsample=4, boxcar=1, buf_len=16384), DECIMATED, GENERAL, 5, 3),
    "staged_e15": (dict(bin_e=15, window=1, buf_len=65536), STAGED_FAST, STAGED, 3, 2),
}
OPTIONS = {"general_e5": dict(scan_frames=0)}
# (byte offset from a 128-byte line, pad behind every row)
PLACES = [(0, 0), (16, 16), (48, 80), (4, 8), (1, 1), (16, 8)]

_case = {}


def power_case(oracle_lib, name):
    if name not in _case:
        kw, _, _, nr, ns = CONFIGS[name]
        cfg = RtlpowerCfg.default(**kw)
        L = int(cfg.buf_len)
        iq = np.concatenate([synth.fm_iq_u8(ns - 1, L // 2 * nr, fs=2.048e6, dev_hz=30e3, seed=177),
                             synth.random_u8(1, L * nr, seed=178)])
        _case[name] = (cfg, iq, oracle_lib.power_scan_batch(cfg, iq, nthreads=3))
    return _case[name]


def scan(cfg, iq, off, pad, fill, nr, split=None, options=None):
    """(avg per stream, samples per stream, last_kernel of every call) of the reads in rows at (off, pad)."""
    from rtlsdr_amd.power import GpuPower
    L = int(cfg.buf_len)
    din = rg.DeviceInput(iq, off, pad, fill)
    kernels = []
    with GpuPower(cfg, iq.shape[0], 0) as g:
        for k, v in (options or {}).items():
            g.set_option(k, v)
        for r0, n in ([(0, nr)] if split is None else [(0, split), (split, nr - split)]):
            g.scan_device(din.ptr + r0 * L, din.stride, n)
            kernels.append(g.last_kernel)
        g.sync()
        res = [g.fetch(s) for s in range(iq.shape[0])]
    return [a for a, _ in res], [n for _, n in res], kernels


@pytest.mark.parametrize("off,pad", PLACES, ids=[f"off{o}_pad{p}" for o, p in PLACES])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_power_rows_of_any_placement(oracle_lib, name, off, pad):
    _, fast, slow, nr, ns = CONFIGS[name]
    cfg, iq, (want, wn) = power_case(oracle_lib, name)
    family = fast if off % 16 == 0 and pad % 16 == 0 else slow
    runs = {}
    for what, fill, split in (("0x00", 0x00, None), ("0xFF", 0xFF, None), ("split", 0x00, 2)):
        avg, samples, kernels = scan(cfg, iq, off, pad, fill, nr, split, OPTIONS.get(name))
        runs[what] = (avg, samples)
        assert kernels == [family] * len(kernels), (name, off, pad, what, kernels)
        for s in range(ns):
            assert samples[s] == wn[s], (name, off, pad, what, s, kernels)
            if not np.array_equal(avg[s], want[s]):
                d = np.flatnonzero(avg[s] != want[s])
                raise AssertionError(f"{name} off={off} pad={pad} {what} last_kernel={kernels} stream {s}: {d.size} of {want[s].size} "
                                     f"bins differ from the oracle, first at {d[:8].tolist()}")
    for what in ("0xFF", "split"):
        for s in range(ns):
            assert runs[what][1][s] == runs["0x00"][1][s] and np.array_equal(runs[what][0][s], runs["0x00"][0][s]), (name, off, pad, what, s)
