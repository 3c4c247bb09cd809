"""Option source_dc without a GPU (include/rtlfm_hip.h, "source_dc"): the model's recurrence against the oracle's
dc_block_raw_filter, the mixer's wider bound, the two wider host checks at their edges, and rtl_fm_hip's refusals."""
import errno

import numpy as np
import pytest

import channel_model as cm
import source_dc_model as sdm
from cases import make_cfg
from rtlsdr_amd import capi
from rtlsdr_amd.capi import MODE_RAW
from test_cli_channels_cpu import chan, refused, run  # noqa: F401  (chan: a fixture)


# ---------------------------------------------------------------- the recurrence ----

@pytest.mark.parametrize("L, k, offs", [(512, 9, (9, -14)), (2048, 9, (30, 9)), (16384, 0, (-14, 30)), (1024, 100, (-100, 90))])
def test_recurrence_equals_the_oracles_dc_block_raw_filter(L, k, offs):
    """The oracle with dc_block_raw = 1, offset_tuning = 1, -M raw at downsample 1 hands back I - 127 - avgI, Q - 127 - avgQ
    of every sample: what it subtracted is read off that, buffer by buffer, and the record it carries afterwards."""
    from oracle import pyoracle as po
    nb = 6
    rng = np.random.default_rng(L + k)
    iq = rng.integers(-20, 21, size=nb * L) + 127
    for b in range(nb):  # another offset per buffer and component
        iq[b * L:(b + 1) * L:2] += offs[0] * (1 + b % 3) // 2
        iq[b * L + 1:(b + 1) * L:2] += offs[1] * (1 + (b + 1) % 3) // 2
    iq = np.clip(iq, 0, 255).astype(np.uint8)
    cfg = make_cfg(dict(mode=MODE_RAW, downsample=1, rate_out=1000000, dc_block_raw=1, offset_tuning=1, rdc_block_const=k), L, nb)
    out, st = po.run_stream(cfg, iq)
    assert out.size == nb * L
    sub = (iq.astype(np.int64) - 127) - out.astype(np.int64)
    want = sdm.averages(iq, L, k, (0, 0))
    for b in range(nb):
        assert set(sub[b * L:(b + 1) * L:2].tolist()) == {want[b][0]}, (b, want[b])
        assert set(sub[b * L + 1:(b + 1) * L:2].tolist()) == {want[b][1]}, (b, want[b])
    assert (st.dc_avgI, st.dc_avgQ) == want[-1]
    assert len({w for w in want}) > 1  # (the buffers did differ)
    # ... and carried on from that record: one run of six is two runs of three
    half = sdm.averages(iq[:3 * L], L, k, (0, 0))
    assert half + sdm.averages(iq[3 * L:], L, k, half[-1]) == want


def test_carried_value_is_clamped_and_the_averages_stay_inside_128():
    L = 512
    for byte, carried in ((255, (1000000, -1000000)), (0, (-129, 129)), (255, (128, 128))):
        av = sdm.averages(np.full(4 * L, byte, dtype=np.uint8), L, 9, carried)
        first = [sdm.trunc_div((byte - 127) + sdm.clamp(c, -128, 128) * 9, 10) for c in carried]
        assert list(av[0]) == first
        assert all(abs(v) <= 128 for pair in av for v in pair)


# ---------------------------------------------------------------- the mixer's bound ----

def test_mixer_bound_with_the_option_is_362_over_the_whole_table():
    """|x|, |y| <= 256: |I'|, |Q'| <= (256 (|c| + |s|) + 8192) >> 14 for every one of the 1024 entries - and the table's worst
    entry reaches 362 with real inputs, so the bound is the least one."""
    tab = cm.table().astype(np.int64)
    assert tab.shape == (1024, 2)
    worst = 0
    for c, s in tab:
        bound = (256 * (abs(int(c)) + abs(int(s))) + 8192) >> 14
        got = 0
        for x in (-256, 256):
            for y in (-256, 256):
                got = max(got, abs((x * c + y * s + 8192) >> 14), abs((y * c - x * s + 8192) >> 14))
        assert got <= 362 and bound <= 362, (c, s, got, bound)
        worst = max(worst, got)
    assert worst == 362
    # without the option: the 182 the existing check stands on
    assert max((128 * (abs(int(c)) + abs(int(s))) + 8192) >> 14 for c, s in tab) <= 182


# ---------------------------------------------------------------- the wider checks ----

def _fcheck(lib, fn, taps, shift):
    t = np.ascontiguousarray(taps, dtype=np.int16)
    return getattr(lib, fn)(t.ctypes.data, t.size, shift)


def _bcheck(lib, fn, K, taps, shift):
    t = np.ascontiguousarray(taps, dtype=np.int16)
    return getattr(lib, fn)(K, t.ctypes.data, t.size, shift)


def _taps_with_abs_sum(total, n):
    """n int16 taps, alternating in sign, whose absolute values add up to total."""
    t = np.full(n, total // n, dtype=np.int64)
    t[: total - int(t.sum())] += 1
    assert t.sum() == total and t.max() <= 32767
    t[1::2] *= -1
    return t.astype(np.int16)


@pytest.mark.parametrize("shift", [0, 14])
def test_filter_check_dc_at_the_edge(shift):
    lib = capi.load()
    r = (1 << (shift - 1)) if shift else 0
    limit = ((1 << 31) - 1 - r) // 362          # the largest sum of |taps| the wider check lets through
    at = _taps_with_abs_sum(limit, 1024)
    over = _taps_with_abs_sum(limit + 1, 1024)
    assert _fcheck(lib, "rtlfm_channel_filter_check_dc", at, shift) == 0
    assert _fcheck(lib, "rtlfm_channel_filter_check_dc", over, shift) == -errno.ERANGE
    assert _fcheck(lib, "rtlfm_channel_filter_check", over, shift) == 0  # (passes the old check, fails the new)
    old = _taps_with_abs_sum(((1 << 31) - 1 - r) // 182, 1024)
    assert _fcheck(lib, "rtlfm_channel_filter_check", old, shift) == 0
    assert _fcheck(lib, "rtlfm_channel_filter_check_dc", old, shift) == -errno.ERANGE
    # the arguments, as the existing check
    assert _fcheck(lib, "rtlfm_channel_filter_check_dc", at[:0], shift) == -errno.EINVAL
    assert _fcheck(lib, "rtlfm_channel_filter_check_dc", at, 31) == -errno.EINVAL
    assert lib.rtlfm_channel_filter_check_dc(None, 4, 0) == -errno.EINVAL


@pytest.mark.parametrize("K, shift", [(4, 0), (8, 9), (256, 9)])
def test_bank_check_dc_at_the_edge(K, shift):
    """The check is per branch: only branch 1 carries the weight here, the others a tap of 1."""
    lib = capi.load()
    r = (1 << (shift - 1)) if shift else 0
    ntaps = 4096
    Q = ntaps // K

    def bank(total):
        need = -(-total // 32767)
        assert need <= Q
        t = np.ones(ntaps, dtype=np.int64)
        t[1::K][:need] = _taps_with_abs_sum(total, need)
        t[1::K][need:] = 0
        return t.astype(np.int16)
    limit = ((1 << 31) - 1 - r) // 256
    if limit > 32767 * Q:  # (K = 256: sixteen taps per branch cannot reach the limit - the check can never fail there)
        assert _bcheck(lib, "rtlfm_channel_bank_check_dc", K, bank(32767 * Q), shift) == 0
        return
    assert _bcheck(lib, "rtlfm_channel_bank_check_dc", K, bank(limit), shift) == 0
    assert _bcheck(lib, "rtlfm_channel_bank_check_dc", K, bank(limit + 1), shift) == -errno.ERANGE
    assert _bcheck(lib, "rtlfm_channel_bank_check", K, bank(limit + 1), shift) == 0
    old = bank(min(((1 << 31) - 1 - r) // 128, 32767 * Q))  # (the old limit, or all a branch can hold: K = 8 cannot reach it)
    assert _bcheck(lib, "rtlfm_channel_bank_check", K, old, shift) == 0
    assert _bcheck(lib, "rtlfm_channel_bank_check_dc", K, old, shift) == -errno.ERANGE
    assert _bcheck(lib, "rtlfm_channel_bank_check_dc", 3, old, shift) == -errno.EINVAL
    assert _bcheck(lib, "rtlfm_channel_bank_check_dc", K, old, 31) == -errno.EINVAL


# ---------------------------------------------------------------- rtl_fm_hip ----

def test_srcdc_needs_the_channel_file(tmp_path):
    """Without -X: refused before a device is opened."""
    r = run(tmp_path, ["-E", "srcdc"], out="out.raw")
    refused(r, "-E srcdc", "-X", "needs")


def test_srcdc_does_not_go_with_rdc(tmp_path, chan):  # noqa: F811
    x = chan("100.1M 100.2M\n")
    refused(run(tmp_path, ["-X", x, "-E", "srcdc", "-E", "rdc"]), "-E srcdc", "-E rdc", "does not go with")
    refused(run(tmp_path, ["-E", "rdc", "-E", "srcdc"], out="out.raw"), "-E srcdc", "-E rdc", "does not go with")


def test_rdc_with_channels_stays_refused_with_its_text_and_srcdc_is_accepted(tmp_path, chan):  # noqa: F811
    x = chan("100.1M 100.2M\n")
    refused(run(tmp_path, ["-X", x, "-E", "rdc"]), "-X", "-E rdc", "it rides on the rotation's kernel, whose place the mixers take")
    # -E srcdc with -X: accepted - the run gets as far as the device layer
    r = run(tmp_path, ["-X", x, "-E", "srcdc"])
    assert r.returncode == 1 and "No supported devices" in r.stderr and "srcdc" not in r.stderr
