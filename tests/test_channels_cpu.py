"""The channelizer's host side without a GPU: the symbols, the step planner and the table of the library against the
numpy model (tests/channel_model.py), and the model itself against the oracle where the two meet - step = 2^30 is
rotate16_neg90, step = 0 the identity."""
import ctypes as C

import numpy as np
import pytest

import channel_model as cm
from rtlsdr_amd import build as hipbuild
from rtlsdr_amd import capi


@pytest.fixture(scope="module")
def lib():
    hipbuild.build()
    return capi.load()


CHANNEL_SYMBOLS = ("rtlfm_channel_step", "rtlfm_channel_table", "rtlfm_gpu_set_channels", "rtlfm_gpu_channels_seek",
                   "rtlfm_gpu_channels_tell")


def test_channel_symbols_are_exported_and_declared(lib):
    for name in CHANNEL_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.DECLARED_SYMBOLS, name


def test_channel_step_equals_the_model(lib):
    rng = np.random.default_rng(20261019)
    for _ in range(2000):
        rate = int(rng.choice([int(rng.integers(1, 1 << 32)), int(rng.integers(225_001, 3_200_001)), 1_000_000, 2_400_000]))
        shift = int(rng.choice([int(rng.integers(-(1 << 31), 1 << 31)), int(rng.integers(-rate, rate + 1)) if rate < (1 << 31) else 0]))
        assert lib.rtlfm_channel_step(shift, rate) == cm.step_from_hz(shift, rate), (shift, rate)
    for rate in (1_000_000, 1_024_000, 2_400_000, 3_200_000, 225_004, 4, 1 << 31):
        assert rate % 4 == 0
        assert lib.rtlfm_channel_step(rate // 4, rate) == 1 << 30
        assert lib.rtlfm_channel_step(-(rate // 4), rate) == 3 << 30
        assert lib.rtlfm_channel_step(0, rate) == 0
    assert lib.rtlfm_channel_step(12345, 0) == 0
    # half-way cases round up, also below zero: 2^32 / 2^33 = 0.5 -> 1, -0.5 -> 0
    assert cm.step_from_hz(1, 1 << 33) == 1 and cm.step_from_hz(-1, 1 << 33) == 0
    assert lib.rtlfm_channel_step(1, 2) == 1 << 31 and lib.rtlfm_channel_step(-1, 2) == 1 << 31


def test_channel_table_equals_the_model(lib):
    from rtlsdr_amd.demod import channel_step, channel_table
    got = np.zeros((1024, 2), dtype=np.int16)
    assert lib.rtlfm_channel_table(got.ctypes.data) == 0
    want = cm.table()
    assert np.array_equal(got, want)
    assert np.array_equal(channel_table(), want)
    assert channel_step(600_000, 2_400_000) == 1 << 30
    assert tuple(want[0]) == (16384, 0) and tuple(want[256]) == (0, 16384) and tuple(want[512]) == (-16384, 0) and tuple(want[768]) == (0, -16384)
    assert lib.rtlfm_channel_table(None) == -22


def test_model_meets_the_oracle_at_quarter_rate_and_at_zero(oracle_lib):
    """Arbitrary full-scale bytes: step = 2^30 is orc_rotate16_neg90 of the converted samples - at any pos that is a
    multiple of four, which buffers keep it -, step = 0 leaves them as they are."""
    orc = oracle_lib.oracle()
    rng = np.random.default_rng(7)
    src = rng.integers(0, 256, size=(2, 4096), dtype=np.uint8)
    src[0, :64] = np.tile(np.array([0, 255, 255, 0], dtype=np.uint8), 16)
    conv = np.zeros(src.shape, dtype=np.int16)
    for s in range(2):
        orc.orc_u8_to_i16(src[s].ctypes.data, conv[s].ctypes.data, src.shape[1])
    for pos in (0, 4, (1 << 32) - 4, 123456 * 4):
        oi, oq = cm.mix(src, [0, 0], 1, pos)
        assert np.array_equal(oi, conv[:, 0::2]) and np.array_equal(oq, conv[:, 1::2])
        rot = conv.copy()
        for s in range(2):
            orc.orc_rotate16_neg90(rot[s].ctypes.data, src.shape[1])
        oi, oq = cm.mix(src, [1 << 30, 1 << 30], 1, pos)
        assert np.array_equal(oi, rot[:, 0::2]) and np.array_equal(oq, rot[:, 1::2])
    # and the chain behind it: the model through the oracle with step 2^30 = the oracle's own chain with the rotation
    cfg = capi.RtlfmCfg.default(downsample=10, custom_atan=capi.ATAN_FAST, block_len=2048, max_blocks=2)
    quiet = (rng.integers(-60, 61, size=(2, 4096)) + 127).astype(np.uint8)
    want = oracle_lib.run_batch(cfg, quiet)
    got = cm.model_via_oracle(cfg, quiet, [1 << 30, 1 << 30], 1, 0)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])
