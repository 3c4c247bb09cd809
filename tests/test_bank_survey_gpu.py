"""The channel bank's survey (include/rtlfm_hip.h, rtlfm_gpu_bank_survey; option bank_survey; k_channel_bank_survey,
k_bank_survey_reduce, k_bank_power_plain) against tests/channel_bank_model.py: power[a][k] = sum over the frames the run
emitted of Yi^2 + Yq^2 in uint64, frames[a] = their number - equality of every bit, on both paths."""
import ctypes as C
import errno

import numpy as np
import pytest

import channel_bank_model as bm
from bank_survey_common import assert_survey, model_run
from cases import case, make_cfg
from channel_common import BACK, assert_rows, bank_handle, demod, full_scale, raw_cfg, run_once, to_device
from channel_common import random_bank_taps as random_taps
from channel_fir_model import raw_rows
from rtlsdr_amd import synth
from rtlsdr_amd.demod import channel_lowpass

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def surveyed_runs(g, model, src, L, runs, paths=None, what=""):
    """Consecutive runs on handle and model: every run's survey and -M raw rows equal the model's."""
    d, b0 = to_device(src), 0
    for r, nb in enumerate(runs):
        if paths is not None:
            g.set_path(paths[r])
        (I, Q), power, frames = model_run(model, src[:, b0 * L:(b0 + nb) * L])
        rows, _ = run_once(g, d, L, b0, nb)
        assert_survey(g.bank_survey(), power, frames, f"{what} run {r}")
        assert_rows(rows, raw_rows(I, Q), f"{what} run {r}")
        b0 += nb


# ------------------------------------------------------------ 1. shapes, both paths ----

SHAPES = [
    # nsrc, K, bins, D, L, ntaps
    (1, 4, [2], 3, 2048, 3),               # 32 frames a batch; 341 frames a buffer: tiles of 256 and 85
    (3, 4, None, 8, 512, 20),              # per_source == K, D divides the run
    (3, 16, [5, 5, 9], 10, 2048, 128),     # a duplicate bin, D does not divide the run: the history and prev_index carry
    (1, 16, None, 64, 16384, 4096),
    (1, 128, None, 8, 4096, 300),          # one frame a batch
    (3, 128, [127], 100, 2048, 643),
    (1, 128, [5, 100], 48, 4096, 4096),    # the survey's 2 KiB of LDS halve F here (32 -> 16): other tiles than the option off
    (1, 256, None, 7, 2048, 1283),         # two butterflies a lane; F = 16
    (3, 256, [0, 255, 0], 10, 2048, 2048),
]


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("nsrc,K,bins,D,L,ntaps", [pytest.param(*s, id="{}x{}_{}_D{}_L{}_t{}".format(
    s[0], s[1], "id" if s[2] is None else len(s[2]), *s[3:])) for s in SHAPES])
def test_survey_equals_the_model(nsrc, K, bins, D, L, ntaps, path):
    runs = (1, 3, 2)
    taps, shift = random_taps(K, ntaps, 7 * K + D)
    src = full_scale(nsrc, sum(runs) * L, 900 + K + D)
    model = bm.BankModel(K, taps, shift, D, nsrc, bins=bins)
    with bank_handle(raw_cfg(D, L), nsrc, K, bins, taps, shift, path, bank_survey=1) as g:
        surveyed_runs(g, model, src, L, runs, what=f"path {path}")
        assert g.last_path == (2 if path == 0 else 1)


# -------------------------------------------------------------------- 2. segments ----

def test_segments_give_the_same_survey():
    """4 x 16384 bytes at / 8: 4096 frames = 16 full tiles, and the plan counts a seventeenth that owns no frame - with one
    tile per segment a whole segment breaks out at once and must store zeros."""
    nsrc, K, L, D, runs = 2, 16, 16384, 8, (4, 4)
    taps, shift = random_taps(K, 128, 33)
    src = full_scale(nsrc, 8 * L, 34)
    for opts in (dict(fused_tiles_per_seg=1), dict(fused_tiles_per_seg=3), dict(fused_min_tiles=1, fused_waves=4096)):
        model = bm.BankModel(K, taps, shift, D, nsrc, bins=[3, 12])
        with bank_handle(raw_cfg(D, L, 4), nsrc, K, [3, 12], taps, shift, 0, bank_survey=1, **opts) as g:
            surveyed_runs(g, model, src, L, runs, what=str(opts))


# ------------------------------------------------------------------ 3. an E == 0 run ----

@pytest.mark.parametrize("path", [0, 1])
def test_a_run_without_frames_leaves_zeros(path):
    """A buffer is never shorter than D, so a run emits no frame only from a record whose prev_index says that more than a
    run is still owed: prev_index = -100 with D = 200 and 256 samples.  Directly after a loud run: frames 0, power all zero -
    not the partial sums the loud run left."""
    nsrc, K, L, D = 2, 16, 512, 200
    bins = [1, 7]
    taps, shift = random_taps(K, 100, 55)
    src = full_scale(nsrc, 3 * L, 56)
    model = bm.BankModel(K, taps, shift, D, nsrc, bins=bins)
    with bank_handle(raw_cfg(D, L, 1), nsrc, K, bins, taps, shift, path, bank_survey=1) as g:
        d = to_device(src)
        (I, Q), power, frames = model_run(model, src[:, :L])
        run_once(g, d, L, 0, 1)
        assert power.max() > 0 and frames.tolist() == [1, 1]
        assert_survey(g.bank_survey(), power, frames, "the loud run")
        for s in range(g.nstreams):
            st = g.state_get(s)
            st.prev_index = -100
            g.state_set(s, st)
        model.p0 = [-100] * model.S
        (I, Q), power, frames = model_run(model, src[:, L:2 * L])
        assert frames.tolist() == [0, 0] and not power.any()
        rows, _ = run_once(g, d, L, 1, 1)
        assert_survey(g.bank_survey(), power, frames, "the run without frames")
        assert [r.size for r in rows] == [0] * g.nstreams
        (I, Q), power, frames = model_run(model, src[:, 2 * L:])  # ... and the run behind it: prev_index 156, two frames
        rows, _ = run_once(g, d, L, 2, 1)
        assert frames.tolist() == [2, 2]
        assert_survey(g.bank_survey(), power, frames, "the run behind it")


# ------------------------------------------------------------- 4. 64-bit accumulation ----

@pytest.mark.parametrize("path", [0, 1])
def test_sums_pass_two_to_the_32(path):
    """The saturating taps of test_saturation_and_wrap_equal_the_model on bytes 255: every v is 32767, bin 0 is near full
    scale in both components - one term is near 2^31, three frames pass a uint32."""
    nsrc, K, D, L = 1, 16, 4, 2048
    taps = np.full(64, 32767, dtype=np.int16)
    src = np.full((nsrc, 2 * L), 255, dtype=np.uint8)
    model = bm.BankModel(K, taps, 0, D, nsrc)
    want = [model_run(model, src[:, :L]), model_run(model, src[:, L:])]
    assert all(int(p[0, 0]) > 1 << 32 for _, p, _ in want), [int(p[0, 0]) for _, p, _ in want]  # the precondition, on the model
    with bank_handle(raw_cfg(D, L, 1), nsrc, K, None, taps, 0, path, bank_survey=1) as g:
        d = to_device(src)
        for r, (_, power, frames) in enumerate(want):
            run_once(g, d, L, r, 1)
            assert_survey(g.bank_survey(), power, frames, f"path {path} run {r}")


# ------------------------------------------------------------------- 5. sign and place ----

@pytest.mark.parametrize("k", [3, 13])
def test_a_carrier_is_the_maximum_of_its_bin(k):
    """One carrier at +k fs / K: bin k is the survey's maximum, below and above K / 2."""
    K, D, L = 16, 8, 4096
    n = np.arange(L // 2, dtype=np.float64)
    sig = 60.0 * np.exp(2j * np.pi * k * n / K)
    src = np.empty((1, L), dtype=np.uint8)
    src[0, 0::2] = np.rint(127 + sig.real).astype(np.uint8)
    src[0, 1::2] = np.rint(127 + sig.imag).astype(np.uint8)
    taps, shift = channel_lowpass(128, 0.4 / K, 1)
    shift -= 4
    model = bm.BankModel(K, taps, shift, D, 1, bins=[0])
    _, power, frames = model_run(model, src)
    with bank_handle(raw_cfg(D, L, 1), 1, K, [0], taps, shift, 0, bank_survey=1) as g:
        run_once(g, to_device(src), L, 0, 1)
        got = g.bank_survey()
    assert_survey(got, power, frames, f"carrier {k}")
    assert int(np.argmax(got[0][0])) == k and int(got[0][0, k]) > 20 * int(np.delete(got[0][0], k).max())


# ------------------------------------------------------ 6. survey on changes nothing else ----

def test_survey_on_changes_nothing_else():
    """fm -A fast with the squelch behind the bank, twin handles: rows, lengths, levels, every state record and the next
    run equal bit for bit; the surveyed run is path 2 and one timed front-end launch (the reduce inside its pair)."""
    nsrc, K, L, D, runs = 2, 16, 2048, 8, (1, 2, 1)
    bins = [0, 1, 15, 0]
    taps, shift = channel_lowpass(128, 0.4 / K, 1)
    shift -= 4
    src = synth.fm_iq_u8(nsrc, sum(runs) * L // 2, fs=2.4e6, dev_hz=30e3, amplitude=55.0, seed=191)
    src[:, L:2 * L] = 127
    cfg = make_cfg(dict(BACK["fmfast_squelch"], downsample=D), L, 2)
    seen = {}
    for on in (0, 1):
        with bank_handle(cfg, nsrc, K, bins, taps, shift, 0, bank_survey=on) as g:
            g.timing_enable(True)
            g.timing_read()
            d, b0, out = to_device(src), 0, []
            for nb in runs:
                rows, p = run_once(g, d, L, b0, nb)
                assert p == 2
                out.append((rows, g.levels_all()[:, :nb].copy(), bytes(g.state_get_all()), g.timing_read()[1]))
                b0 += nb
            seen[on] = out
    for r, (a, b) in enumerate(zip(seen[0], seen[1], strict=True)):
        assert_rows(b[0], a[0], f"run {r}")
        assert np.array_equal(a[1], b[1]) and a[2] == b[2], r
        assert a[3] == b[3], (r, a[3], b[3])  # timed front-end launches: the same count


# ------------------------------------------------ 7. verify_twice, path switching, the ring ----

@pytest.mark.parametrize("path", [0, 1])
def test_verify_twice_surveys_one_execution(path):
    nsrc, K, L, D = 1, 16, 2048, 10
    taps, shift = random_taps(K, 500, 123)
    src = full_scale(nsrc, 4 * L, 121)
    model = bm.BankModel(K, taps, shift, D, nsrc)
    with bank_handle(raw_cfg(D, L, 2), nsrc, K, None, taps, shift, path, verify_twice=1, bank_survey=1) as g:
        surveyed_runs(g, model, src, L, (2, 1, 1), what=f"path {path}")
        assert g.get_option("verify_runs") == 3 and g.get_option("verify_mismatches") == 0


def test_switching_paths_between_runs():
    nsrc, K, L, D = 2, 16, 2048, 10
    runs = (1, 2, 1, 1, 1)
    taps, shift = random_taps(K, 403, 73)
    src = full_scale(nsrc, sum(runs) * L, 71)
    model = bm.BankModel(K, taps, shift, D, nsrc, bins=[4, 9])
    with bank_handle(raw_cfg(D, L, 2), nsrc, K, [4, 9], taps, shift, bank_survey=1) as g:
        surveyed_runs(g, model, src, L, runs, paths=(1, 2, 1, 0, 1), what="switching")


def test_the_source_ring_and_prev():
    """Over the source ring: bank_survey(prev=True) is the run before the last one's, bank_survey() the last one's."""
    nsrc, K, L, D = 2, 16, 2048, 10
    bins = [2, 11, 2]
    taps, shift = random_taps(K, 200, 83)
    src = full_scale(nsrc, 3 * L, 84)
    model = bm.BankModel(K, taps, shift, D, nsrc, bins=bins)
    want = [model_run(model, src[:, r * L:(r + 1) * L]) for r in range(3)]
    with bank_handle(raw_cfg(D, L, 1), nsrc, K, bins, taps, shift, 0, source_ring=1, bank_survey=1) as g:
        for r in range(3):
            for a in range(nsrc):
                g.push(src[a, r * L:(r + 1) * L], a)
            g.run()
            if r:
                assert_survey(g.bank_survey(prev=True), want[r - 1][1], want[r - 1][2], f"prev of run {r}")
            assert_survey(g.bank_survey(), want[r][1], want[r][2], f"run {r}")
            out, lens = g.fetch_all()
            assert_rows([out[s, :lens[s]] for s in range(g.nstreams)], raw_rows(*want[r][0]), f"run {r}")


# ------------------------------------------------------------------- 8. the contract ----

def test_enodata_enobufs_and_the_option():
    nsrc, K, L, D = 2, 16, 2048, 10
    taps, shift = random_taps(K, 77, 131)
    src = full_scale(nsrc, 3 * L, 132)
    power = np.zeros((nsrc, K), dtype=np.uint64)
    frames = np.zeros(nsrc, dtype=np.int32)
    k_ = C.c_int(-1)

    def fetch(g, cap=power.size, prev=False):
        fn = g.lib.rtlfm_gpu_bank_survey_prev if prev else g.lib.rtlfm_gpu_bank_survey
        return fn(g._h, power.ctypes.data, cap, frames.ctypes.data, C.byref(k_))
    with bank_handle(raw_cfg(D, L, 1), nsrc, K, [1, 2], taps, shift) as g:
        d = to_device(src)
        assert g.get_option("bank_survey") == 0
        g.set_option("bank_survey", 1)
        assert fetch(g) == -errno.ENODATA and fetch(g, prev=True) == -errno.ENODATA  # no run yet
        for bad in (2, -1):
            assert g.lib.rtlfm_gpu_set_option(g._h, b"bank_survey", bad) == -errno.EINVAL
        assert g.get_option("bank_survey") == 1
        run_once(g, d, L, 0, 1)
        assert fetch(g) == 0 and k_.value == K and frames.tolist() == [102, 102]
        assert fetch(g, prev=True) == -errno.ENODATA  # (the run before the first)
        k_.value = -1
        assert fetch(g, cap=power.size - 1) == -errno.ENOBUFS and k_.value == K  # *K still written
        assert g.lib.rtlfm_gpu_bank_survey(g._h, power.ctypes.data, power.size, None, C.byref(k_)) == -errno.EINVAL
        g.set_option("bank_survey", 0)  # the option off: the next run carries none, and what the last one left is freed
        assert fetch(g) == -errno.ENODATA
        run_once(g, d, L, 1, 1)
        assert fetch(g) == -errno.ENODATA
        g.set_option("bank_survey", 1)
        g.set_channel_bank(0)  # the bank off: the boxcar takes the run
        run_once(g, d, L, 2, 1)
        assert fetch(g) == -errno.ENODATA
    # it may be set with channels off; -EBUSY inside a begun run (the ring: channels off), and the run is what it was
    cfg = make_cfg(case("c1_boxcar10_fast")[0], L, 1)
    rows = synth.random_u8(2, L, seed=135)
    outs = []
    for inside in (False, True):
        with demod(cfg, 2) as g:
            g.set_option("bank_survey", 1)
            for s in range(2):
                g.push(rows[s], s)
            assert g.run_begin() == 1
            if inside:
                assert g.lib.rtlfm_gpu_set_option(g._h, b"bank_survey", 0) == -errno.EBUSY
                assert g.get_option("bank_survey") == 1
            g.run_end()
            out, lens = g.fetch_all()
            assert fetch(g) == -errno.ENODATA
            outs.append([out[s, :lens[s]].copy() for s in range(2)])
    assert_rows(outs[1], outs[0], "after -EBUSY")
