"""The lane-to-lane hand-offs of k_fused (passes 1-3 and the discriminator) against the oracle.

Whole-tile kernels from three passes on keep the hand-offs' carries in VGPRs: lane l takes lane l - 1's values
through DPP wave_shr:1 whose `old` operand is the carry, and a second DPP move (wave_ror:1) leaves lane 63's values
in lane 0 for the next tile.  A tile in front of a buffer start leaves the five values BEFORE its newest (the
reference's archive never holds the newest input), chosen by a scalar branch.  The partial-tile kernels keep the
SGPR carries (their last lane is not lane 63).

Shapes: 3 streams x 5 buffers x 16384 B - two tiles per buffer, so every second tile starts a buffer and the two
carry forms alternate; full-scale random bytes, where a carry taken from the wrong lane or the wrong tile shows in
the integer stages, next to one synthetic FM signal.  `-A fast` is compared bit for bit, `-A std` with the suite's
tolerance (assert_parity)."""
import numpy as np
import pytest

import golden_util as gu
from cases import make_cfg
from rtlsdr_amd import synth
from test_parity_gpu import assert_parity, gpu_run

pytestmark = pytest.mark.gpu

NS, NB = 3, 5
SEGMENTATIONS = [None, dict(fused_waves=1), dict(fused_tiles_per_seg=1), dict(fused_tiles_per_seg=3)]
SPLITS = [(0, 1), (1, 3), (3, 5)]


def _inputs(L, atan, seed):
    """stream 0: a synthetic FM signal; streams 1, 2: full-scale random bytes (0 and 255 included)"""
    iq = synth.random_u8(NS, L * NB, seed=seed)
    amp = 30.0 if atan == 1 else 60.0
    iq[0] = synth.fm_iq_u8(1, L // 2 * NB, seed=seed + 1, fs=2.4e6, dev_hz=75e3, amplitude=amp)[0]
    return iq


def _check(cfg, outs, sts, want, want_len, wst, atan, what):
    for s in range(NS):
        w = want[s, :want_len[s]]
        if atan == 1:  # integer only
            assert outs[s].shape == w.shape, (what, s)
            bad = np.flatnonzero(outs[s] != w)
            assert bad.size == 0, f"{what} stream {s}: {bad.size} of {w.size} differ, first at {bad[:8].tolist()}"
        else:
            assert_parity(outs[s], w, cfg, f"{what} stream {s}")
        assert gu.state_dict(sts[s], False) == gu.state_dict(wst[s], False), f"{what} stream {s}: state"


def _run_all(oracle_lib, ov, L, atan, seed, what):
    cfg = make_cfg(dict(ov, custom_atan=atan), L, NB)
    iq = _inputs(L, atan, seed)
    want, want_len, wst = oracle_lib.run_batch(cfg, iq, nthreads=3)
    for seg in SEGMENTATIONS:
        for splits in ((None, SPLITS) if seg is None or "fused_tiles_per_seg" in seg else (None,)):
            outs, sts, used = gpu_run(cfg, iq, path=2, splits=splits, options=seg)
            assert used == 2, "the one-launch front end must take this"
            _check(cfg, outs, sts, want, want_len, wst, atan, f"{what} atan={atan} {seg} {splits}")


@pytest.mark.parametrize("rdc", [0, 1])
@pytest.mark.parametrize("offs", [0, 1])
@pytest.mark.parametrize("fir9", [0, 1])
@pytest.mark.parametrize("passes", [3, 4, 5, 6])
def test_hand_offs_whole_tiles(oracle_lib, passes, fir9, offs, rdc):
    """Every whole-tile instantiation from three passes on (both discriminator families, with and without the FIR, the
    rotation and the raw DC block): one wave per stream, a wave per tile (every warm-up starts at a tile that either
    begins a buffer or lies inside one), segments of three tiles, the planner's own choice; in one run and in three
    (the carry then goes through the state record)."""
    ov = dict(downsample=1 << passes, downsample_passes=passes, comp_fir_size=9 if fir9 else 0, offset_tuning=offs,
              dc_block_raw=rdc, rate_out=int(2.4e6) >> passes)
    for atan in (0, 1):
        _run_all(oracle_lib, ov, 16384, atan, 4100 + 16 * passes + 8 * fir9 + 4 * offs + 2 * rdc + atan,
                 f"P={passes} fir9={fir9} offs={offs} rdc={rdc}")


@pytest.mark.parametrize("L", [8704, 512 * 3])
@pytest.mark.parametrize("passes,fir9,offs,rdc", [(3, 0, 0, 0), (4, 0, 0, 1), (4, 1, 1, 0), (5, 0, 1, 1), (6, 1, 0, 0)])
def test_hand_offs_partial_tiles(oracle_lib, passes, fir9, offs, rdc, L):
    """Buffers that are not whole tiles (8704 B: a whole tile and four lanes; 1536 B: twelve lanes): these kernels keep
    the carries in SGPRs, read from the tile's last ACTIVE lane."""
    ov = dict(downsample=1 << passes, downsample_passes=passes, comp_fir_size=9 if fir9 else 0, offset_tuning=offs,
              dc_block_raw=rdc, rate_out=int(2.4e6) >> passes)
    for atan in (0, 1):
        _run_all(oracle_lib, ov, L, atan, 4700 + 16 * passes + atan + L, f"L={L} P={passes} fir9={fir9} offs={offs} rdc={rdc}")
