"""Packed results without a GPU: the numpy statement of the index and of the rule (tests/packed_model.py) against the
scanner's model, the record's size as the C compiler lays it out, and the library built for gfx950 with the new names."""
import ctypes as C
import errno
import os
import subprocess
import tempfile

import numpy as np
import pytest

import packed_model as pm
import scan_model as sm
from rtlsdr_amd import build as hipbuild
from rtlsdr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
assert np.dtype(pm.PACKED_ROW) == np.dtype(capi.PACKED_ROW)  # the model speaks of the library's record


class LevelOracle:
    """What scan_model.StreamModel asks of the oracle, for a prescribed sequence of rms() levels: every buffer moves
    squelch_hits as full_demod() moves it (src/rtl_fm.c:1206-1213) and has one sample, its own number."""

    def __init__(self, levels, level):
        self.levels, self.level, self.at = list(levels), level, 0

    def new_states(self, n):
        return (capi.RtlfmStreamState * n)()

    def run_stream(self, cfg, buf, state):
        sr = self.levels[self.at]
        if sr >= 0:
            state.squelch_hits = state.squelch_hits + 1 if sr < self.level else 0
        self.at += 1
        return np.array([self.at - 1], dtype=np.int16), state


@pytest.mark.parametrize("conseq", [0, 1, 2, 10])
def test_rule_on_an_unclamped_counter_decides_as_the_scanner_model(conseq):
    """The walk from the counter a run started with - NEVER clamped between runs - gives StreamModel's decisions, which
    clamps its carried counter after every held buffer.  The sequence has negative levels, and the start is far above
    conseq + 1."""
    level, start = 50, 1000
    rng = np.random.default_rng(conseq)
    levels = np.where(rng.random(240) < 0.35, 80, 5).astype(np.int64)
    levels[rng.random(240) < 0.1] = -1  # rms() of nothing: no decision, the counter stays
    levels[:conseq + 3] = 5             # closed at first, from a counter no clamp has touched
    levels[conseq + 3] = -1
    runs = [1, 3, 2, 7, 1, 1, 5] * 12
    assert sum(runs) == levels.size
    cfg = capi.RtlfmCfg.default(block_len=512, squelch_level=level)
    model = sm.StreamModel(LevelOracle(levels, level), cfg, conseq)
    model.state.squelch_hits = start
    hits, b0 = start, 0
    seen_unclamped = False
    for nb in runs:
        pcm, recs = model.run([np.zeros(512, dtype=np.uint8)] * nb)
        emit, hits = pm.rule(levels[b0:b0 + nb], level, conseq, hits)
        assert np.array_equal(emit, recs["emit"] == 1), (b0, nb)
        assert np.array_equal(pcm, np.arange(b0, b0 + nb, dtype=np.int16)[emit])
        seen_unclamped |= hits > conseq + 1
        b0 += nb
    assert seen_unclamped, "the carried counter never ran beyond the clamp: the test shows nothing"


def test_index_rounds_to_eight_and_pads_with_zeros():
    rng = np.random.default_rng(1)
    lens = [0, 1, 7, 8, 9, 63, 64, 65, 0, 0, 17, -3]
    rows = [rng.integers(-32768, 32768, size=max(n, 0)).astype(np.int16) | 1 for n in lens]  # (| 1: no sample is 0)
    packed, idx = pm.pack(rows)
    want_off = [0, 0, 8, 16, 24, 40, 104, 168, 240, 240, 240, 264]
    assert idx["offset"].tolist() == want_off
    assert idx["len"].tolist() == [max(n, 0) for n in lens] and not idx["held"].any()
    assert packed.size == 264 and (idx["offset"] % 8 == 0).all()
    used = np.zeros(packed.size, dtype=bool)
    for r, rec in zip(rows, idx):
        at = int(rec["offset"])
        assert np.array_equal(packed[at:at + r.size], r)
        used[at:at + r.size] = True
    assert not packed[~used].any() and packed[used].all()
    for a, b in zip(pm.unpack(packed, idx), rows):
        assert np.array_equal(a, b)
    idx0, total0 = pm.index_of([0, 0, 0])
    assert total0 == 0 and not idx0["offset"].any()


def test_extents_follow_the_boxcar_phase():
    # N = 1024 input samples per buffer through /7 from phase 3, I, Q pairs: pieces at every int16 alignment
    begin = pm.extents(4, 1024, 7, 3, 2)
    assert begin.tolist() == [2 * ((3 + b * 1024) // 7) for b in range(5)]
    assert len({int(v) % 8 for v in begin}) > 2
    assert pm.extents(3, 128, 1, 5, 1).tolist() == [0, 128, 256, 384]
    row = np.arange(begin[-1], dtype=np.int16)
    out = pm.gated(row, np.array([True, False, False, True]), begin)
    assert np.array_equal(out, np.concatenate([row[:begin[1]], row[begin[3]:]]))


def test_packed_row_is_16_bytes_in_c():
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "rtlfm_hip.h"\n'
           'int main(){printf("%zu %zu %zu %zu\\n", sizeof(rtlfm_packed_row), offsetof(rtlfm_packed_row, offset), '
           'offsetof(rtlfm_packed_row, len), offsetof(rtlfm_packed_row, held));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "s.c")
        with open(p, "w") as f:
            f.write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), p, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [16, 0, 8, 12]
    assert C.sizeof(capi.RtlfmPackedRow) == 16 and np.dtype(capi.PACKED_ROW).itemsize == 16
    assert np.dtype(capi.PACKED_ROW) == np.dtype(pm.PACKED_ROW)
    assert [getattr(capi.RtlfmPackedRow, n).offset for n in ("offset", "len", "held")] == [0, 8, 12]


def test_library_builds_for_gfx950_and_exports_the_packed_names():
    hipbuild.build()
    lib = capi.load()
    names = ("rtlfm_gpu_fetch_packed", "rtlfm_gpu_fetch_packed_prev", "rtlfm_gpu_pack_device")
    for name in names:
        assert hasattr(lib, name) and name in capi.DECLARED_SYMBOLS
    # the argument checks that come before the device is looked at
    assert lib.rtlfm_gpu_pack_device(0, None, 0, None, 1, None, 0, None, None, None) == -errno.EINVAL
    assert lib.rtlfm_gpu_fetch_packed(None, None, 0, None, None) == -errno.EINVAL
    assert lib.rtlfm_gpu_fetch_packed_prev(None, None, 0, None, None) == -errno.EINVAL
    for code in (-errno.ENODATA, -errno.ENOTSUP, -errno.EBUSY):
        assert b"pack" in lib.rtlfm_gpu_strerror(code)
    from rtlsdr_amd import demod
    assert callable(demod.pack_device) and callable(demod.GpuDemod.fetch_packed)
