"""The channel bank on the GPU (include/rtlfm_hip.h, rtlfm_gpu_set_channel_bank; csrc/channel_bank_kernel.h) against
tests/channel_bank_model.py: equality of every bit, on both paths, and of the paths with each other.

The bank's own output is compared in -M raw, where it IS the output and full-scale bytes (0 and 255 included) may be used.
The chain behind it is compared through the existing oracle, which reads bytes: there the inputs are bounded and the taps
have a DC gain of 1 or 2, so that the bins fit a byte (the model asserts it), and buffers are multiples of D.

The shapes test meets every number of sources, K, kind of bins, D, block length and number of taps the feature was specified
with; the values go round a list of cases so that the suite stays quick - every value meets several cases, not all."""
import ctypes as C
import errno

import numpy as np
import pytest

import channel_bank_model as bm
import channel_model as cm
from cases import case, make_cfg
from channel_common import (BACK, SEEK_TO, assert_call_clears_the_history, assert_rows, bank_handle, bounded, demod, full_scale,
                            model_runs, raw_cfg, run_gpu, run_once, steps_for, tone_fit)
from channel_common import random_bank_taps as random_taps
from rtlsdr_amd import capi, synth
from rtlsdr_amd.capi import MODE_FM

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RUNS = (1, 3, 2)


def bins_of(kind, K, seed=0):
    rng = np.random.default_rng(1000 + seed)
    if kind == "id":
        return None
    if kind == "subset":
        return sorted(int(v) for v in rng.choice(K, size=max(1, K // 4 - 1), replace=False))
    if kind == "perm":
        return [int(v) for v in rng.permutation(K)]
    b = [int(v) for v in rng.integers(0, K, size=5)]  # "dup"
    return b + [b[0], K - 1, b[0]]


def ntaps_of(kind, K):
    return {"1": 1, "K-1": K - 1, "K": K, "8K": 8 * K, "5K+3": 5 * K + 3, "4096": 4096}[kind]


# ------------------------------------------- 1. shapes x taps, the model, both paths ----

SHAPES = [
    # nsrc, K, bins, D, L, taps
    (1, 4, "id", 1, 512, "1"),
    (3, 4, "dup", 3, 2048, "K-1"),
    (1, 4, "subset", 100, 16384, "4096"),
    (1, 16, "id", 10, 2048, "8K"),
    (3, 16, "subset", 64, 16384, "4096"),
    (1, 16, "perm", 3, 512, "K"),
    (1, 64, "id", 10, 2048, "8K"),
    (3, 64, "perm", 100, 2048, "5K+3"),   # D > K, 1024 % 100 != 0: variable counts
    (1, 64, "subset", 1, 512, "K"),
    (1, 64, "id", 32, 16384, "8K"),
    (3, 128, "perm", 3, 512, "4096"),     # a history of 4096 samples, runs of 256: longer than a run
    (1, 128, "id", 64, 16384, "K-1"),
    (1, 128, "dup", 10, 2048, "1"),
    (1, 256, "id", 10, 2048, "8K"),
    (3, 256, "dup", 64, 2048, "4096"),
    (1, 256, "subset", 1, 512, "5K+3"),
]


@pytest.mark.parametrize("nsrc,K,kind,D,L,tk", [pytest.param(*s, id="{}x{}{}_D{}_L{}_taps{}".format(*s)) for s in SHAPES])
def test_bank_equals_the_model_on_both_paths(nsrc, K, kind, D, L, tk):
    """-M raw on full-scale bytes over runs of 1, 3 and 2 buffers: PCM, lengths and prev_index of path 2 and of path 1
    equal the model's (and so each other's)."""
    seed = K * 7 + D
    bins = bins_of(kind, K, seed)
    ntaps = ntaps_of(tk, K)
    taps, shift = random_taps(K, ntaps, seed + ntaps)
    src = full_scale(nsrc, sum(RUNS) * L, 300 + seed)
    model = bm.BankModel(K, taps, shift, D, nsrc, bins=bins)
    want, _ = model_runs(model, src, L, RUNS)
    for path in (0, 1):
        with bank_handle(raw_cfg(D, L), nsrc, K, bins, taps, shift, path) as g:
            got, paths = run_gpu(g, src, L, RUNS)
            st = g.state_get_all()
            assert g.channels_tell() == sum(RUNS) * L // 2
        assert paths == [2 if path == 0 else 1] * len(RUNS), (path, paths)
        assert_rows(got, want, f"path {path}")
        assert [st[s].prev_index for s in range(model.S)] == model.p0, path


# ------------------------------------------------------------------ 2. position ----

@pytest.mark.parametrize("pos", [12345, (1 << 32) - 100])
@pytest.mark.parametrize("path", [0, 1])
def test_residues_come_from_the_absolute_index(pos, path):
    """channels_seek to an odd pos, and to just below 2^32: residues are taken from pos + index, across the wrap (the second
    run's history lies on both sides of it)."""
    nsrc, K, D, L = 2, 64, 10, 2048
    bins = bins_of("subset", K, 5)
    taps, shift = random_taps(K, 5 * K + 3, 201)
    src = full_scale(nsrc, 3 * L, 202)
    model = bm.BankModel(K, taps, shift, D, nsrc, bins=bins)
    model.seek(pos)
    want, _ = model_runs(model, src, L, (1, 2))
    unmoved = bm.BankModel(K, taps, shift, D, nsrc, bins=bins)
    assert not np.array_equal(model_runs(unmoved, src, L, (1, 2))[0][0], want[0])  # (pos matters: another residue per sample)
    with bank_handle(raw_cfg(D, L, 2), nsrc, K, bins, taps, shift, path) as g:
        g.channels_seek(pos)
        got, _ = run_gpu(g, src, L, (1, 2))
        assert g.channels_tell() == pos + 3 * L // 2
    assert_rows(got, want, f"pos {pos} path {path}")


# -------------------------------------------------------------------- 3. saturation ----

@pytest.mark.parametrize("path", [0, 1])
def test_saturation_and_wrap_equal_the_model(path):
    """Bytes 0 and 255 in runs of equal samples, 64 taps of 32767 and shift 0: sat16 is reached at both ends in v, and the
    butterflies' int16 stores wrap (the sums of saturated points pass an int16 in spite of the halving) - both are what
    the model defines."""
    nsrc, K, D, L = 1, 16, 4, 2048
    rng = np.random.default_rng(81)
    src = np.repeat(rng.integers(0, 2, size=(nsrc, 3 * L // 64)).astype(np.uint8) * 255, 64, axis=1)  # 32 equal samples
    taps = np.full(64, 32767, dtype=np.int16)
    assert capi.load().rtlfm_channel_bank_check(K, taps.ctypes.data, 64, 0) == 0
    probe = bm.BankModel(K, taps, 0, D, nsrc)
    vi, vq, _, _ = probe.frames(src)[0]
    assert max(vi.max(), vq.max()) == 32767 and min(vi.min(), vq.min()) == -32768
    model = bm.BankModel(K, taps, 0, D, nsrc)
    want, _ = model_runs(model, src, L, (1, 2))
    with bank_handle(raw_cfg(D, L, 2), nsrc, K, None, taps, 0, path) as g:
        got, _ = run_gpu(g, src, L, (1, 2))
    assert_rows(got, want, f"path {path}")


# ------------------------------------------------------- 4. several segments per source ----

@pytest.mark.parametrize("K,tk", [(64, "8K"), (16, "4096")])
def test_segments_equal_the_model(K, tk):
    """4 x 16384 bytes cut into segments of 1 and of 3 tiles, by fused_min_tiles, and left whole: windows cross tile and
    segment borders, and a second run takes its first windows from the carried history."""
    nsrc, L, D, runs = 2, 16384, 10, (4, 4)
    bins = bins_of("subset", K, 6)
    taps, shift = random_taps(K, ntaps_of(tk, K), 63)
    src = full_scale(nsrc, 8 * L, 61)
    model = bm.BankModel(K, taps, shift, D, nsrc, bins=bins)
    want, _ = model_runs(model, src, L, runs)
    for opts in (dict(fused_tiles_per_seg=1), dict(fused_tiles_per_seg=3), dict(fused_min_tiles=1, fused_waves=4096),
                 dict(fused_min_tiles=5, fused_waves=4096), dict(fused_min_tiles=64)):
        with bank_handle(raw_cfg(D, L, 4), nsrc, K, bins, taps, shift, 0, **opts) as g:
            got, paths = run_gpu(g, src, L, runs)
        assert paths == [2, 2]
        assert_rows(got, want, str(opts))


# --------------------------------------------------------------- 5. path switching ----

def test_switching_paths_between_runs_changes_nothing():
    nsrc, K, L, D = 2, 16, 2048, 10
    runs = (1, 2, 1, 3, 1, 1)
    taps, shift = random_taps(K, 403, 73)
    src = full_scale(nsrc, sum(runs) * L, 71)
    model = bm.BankModel(K, taps, shift, D, nsrc)
    want, _ = model_runs(model, src, L, runs)
    for paths in ((1, 2, 1, 2, 2, 1), (2, 1, 1, 0, 1, 2)):
        with bank_handle(raw_cfg(D, L, 3), nsrc, K, None, taps, shift) as g:
            got, seen = run_gpu(g, src, L, runs, paths=paths)
        assert seen == [1 if p == 1 else 2 for p in paths]
        assert_rows(got, want, str(paths))


# ------------------------------------------------------------------------ 6. state ----

@pytest.mark.parametrize("path", [0, 1])
def test_verify_twice_sees_one_pos_and_one_history(path):
    nsrc, K, L, D = 1, 16, 2048, 10
    taps, shift = random_taps(K, 500, 123)
    src = full_scale(nsrc, 4 * L, 121)
    model = bm.BankModel(K, taps, shift, D, nsrc)
    want, _ = model_runs(model, src, L, (2, 1, 1))
    with bank_handle(raw_cfg(D, L, 2), nsrc, K, None, taps, shift, path, verify_twice=1) as g:
        got, _ = run_gpu(g, src, L, (2, 1, 1))
        assert g.channels_tell() == 4 * L // 2
        assert g.get_option("verify_runs") == 3 and g.get_option("verify_mismatches") == 0
    assert_rows(got, want, f"path {path}")


CLEARERS = ("set_channel_bank", "set_channels", "reset", "channels_seek")


@pytest.mark.parametrize("what", CLEARERS)
@pytest.mark.parametrize("path", [0, 1])
def test_each_of_the_four_calls_clears_the_history(what, path):
    """A run, the call, a run: the second run equals the model with the history cleared by the call - and differs from
    the model that kept it, so a call that does not clear fails here."""
    nsrc, K, L, D = 2, 16, 512, 8  # (256 % 8 == 0: prev_index stays 0 whatever the call does to the records)
    bins = bins_of("subset", K, 7)
    taps, shift = random_taps(K, 300, 113)
    src = full_scale(nsrc, 2 * L, 111)

    def again(g):
        g.set_channels(len(bins), steps=steps_for(g.nstreams))
        assert g.get_channel_bank()[0] == 0  # (set_channels removes the bank: bins belongs to the old per_source)
        g.set_channel_bank(K, taps, shift, bins=bins)
    calls = {"set_channel_bank": lambda g: g.set_channel_bank(K, taps, shift, bins=bins),
             "set_channels": again,
             "reset": lambda g: g.reset(),
             "channels_seek": lambda g: g.channels_seek(SEEK_TO)}
    assert_call_clears_the_history(lambda: bm.BankModel(K, taps, shift, D, nsrc, bins=bins),
                                   lambda: bank_handle(raw_cfg(D, L, 1), nsrc, K, bins, taps, shift, path), calls, what, src, L,
                                   f"{what} path {path}")


@pytest.mark.parametrize("path", [0, 1])
def test_channel_zero_rules_the_schedule(path):
    """prev_index set differently per channel through state_set: the source's channel 0 decides where outputs are due, and
    every channel of the source leaves the run with the same prev_index and count."""
    nsrc, K, L, D = 2, 16, 2048, 10
    bins = [3, 3, 0, 15, 8]
    per = len(bins)
    taps, shift = random_taps(K, 100, 141)
    src = full_scale(nsrc, 3 * L, 142)
    model = bm.BankModel(K, taps, shift, D, nsrc, bins=bins)
    p0 = [7, 1, 9, 0, 4, 2, 8, 8, 5, 3]  # channel 0 of source 0 starts at 7, of source 1 at 2
    model.p0 = list(p0)
    want, _ = model_runs(model, src, L, (1, 2))
    assert model.p0[:per] == [model.p0[0]] * per and model.p0[per:] == [model.p0[per]] * per
    with bank_handle(raw_cfg(D, L, 2), nsrc, K, bins, taps, shift, path) as g:
        for s in range(nsrc * per):
            st = g.state_get(s)
            st.prev_index = p0[s]
            g.state_set(s, st)
        got, _ = run_gpu(g, src, L, (1, 2))
        st = g.state_get_all()
    assert_rows(got, want, f"path {path}")
    assert [st[s].prev_index for s in range(nsrc * per)] == model.p0
    assert len({got[s].size for s in range(per)}) == 1


# ------------------------------------------------------ 7. the back half, bank on ----

def gain_taps(K, ntaps, gain):
    """A Hamming sinc over 0.4 of a channel spacing whose bins have the DC gain `gain`: (taps, shift = 14 - m)."""
    from rtlsdr_amd.demod import channel_lowpass
    taps, shift = channel_lowpass(ntaps, 0.4 / K, gain)
    return taps, shift - (K.bit_length() - 1)


@pytest.mark.parametrize("name", list(BACK))
@pytest.mark.parametrize("path", [0, 1])
def test_back_half_behind_the_bank(oracle_lib, name, path):
    """-A fast FM, AM, the squelch and -L behind the bank equal the existing oracle on the model's bins; the levels equal
    the oracle's rms() of them.  Buffer 1 of every source is silent, for the squelch."""
    nsrc, K, L, D, runs = 2, 16, 2048, 8, (1, 2)
    bins = [0, 1, 15, 0]
    S = nsrc * len(bins)
    taps, shift = gain_taps(K, 128, 1)  # DC gain 1: the bins of bounded bytes fit a byte
    if name.startswith("fm"):
        src = synth.fm_iq_u8(nsrc, 3 * L // 2, fs=2.4e6, dev_hz=30e3, amplitude=55.0, seed=91)
    else:
        src = bounded(nsrc, 3 * L, 92, 60)
    src[:, L:2 * L] = 127
    cfg = make_cfg(dict(BACK[name], downsample=D), L, 2)
    model = bm.BankModel(K, taps, shift, D, nsrc, bins=bins)
    _, per_run = model_runs(model, src, L, runs)
    want, _ = bm.via_oracle(cfg, per_run, runs, L // 2)
    with_levels = bool(cfg.squelch_level or cfg.report_levels)
    with bank_handle(cfg, nsrc, K, bins, taps, shift, path) as g:
        d = torch.from_numpy(src).cuda()
        got, b0 = [[] for _ in range(S)], 0
        for (I, Q), nb in zip(per_run, runs, strict=True):
            rows, _ = run_once(g, d, L, b0, nb)
            for s in range(S):
                got[s].append(rows[s])
            if with_levels:
                assert np.array_equal(g.levels_all()[:, :nb], bm.levels_of(I, Q, nb, L // 2 // D)), (name, b0)
            b0 += nb
    assert_rows([np.concatenate(x) for x in got], want, f"{name} path {path}")


def test_two_fm_carriers_on_their_bins(oracle_lib):
    """Two FM carriers at +5 fs / K and -3 fs / K in one source, demodulated as bins 5 and K - 3 with /10 and -A fast: each
    channel carries its own modulating tone and next to nothing of the other's - and with the bins swapped the tones are
    swapped.  The device's PCM equals the model's both times."""
    fs, L, nb, D, K = 2_400_000, 20480, 2, 10, 16  # (buffers of 10240 samples: a multiple of D, for the oracle behind the model)
    ks, tones = (5, -3), (2000.0, 3000.0)
    n = np.arange(nb * L // 2, dtype=np.float64)
    sig = np.zeros(n.size, dtype=np.complex128)
    for k, tone in zip(ks, tones, strict=True):
        sig += 40.0 * np.exp(1j * (2 * np.pi * k * n / K + (30e3 / tone) * np.sin(2 * np.pi * tone * n / fs)))
    src = np.empty((1, nb * L), dtype=np.uint8)
    src[0, 0::2] = np.rint(127 + sig.real).astype(np.uint8)
    src[0, 1::2] = np.rint(127 + sig.imag).astype(np.uint8)
    cfg = make_cfg(case("c1_boxcar10_fast")[0], L, nb)
    assert cfg.downsample == D and cfg.mode == MODE_FM
    taps, shift = gain_taps(K, 128, 2)  # DC gain 2: amplitude 80, inside a byte
    for bins, mine in (([5, K - 3], (0, 1)), ([K - 3, 5], (1, 0))):
        model = bm.BankModel(K, taps, shift, D, 1, bins=bins)
        _, per_run = model_runs(model, src, L, (nb,))
        want, _ = bm.via_oracle(cfg, per_run, (nb,), L // 2)
        with bank_handle(cfg, 1, K, bins, taps, shift) as g:
            got, paths = run_gpu(g, src, L, (nb,))
        assert paths == [2]
        assert_rows(got, want, f"bins {bins}")
        for s in range(2):
            _, own = tone_fit(got[s], tones[mine[s]], fs / D, 32)
            _, other = tone_fit(got[s], tones[1 - mine[s]], fs / D, 32)
            assert own > 1000 and other < own / 20, (bins, s, own, other)


# ---------------------------------------- 8. refusals, removal, the getter, launch counts ----

def test_refusals_change_nothing_and_the_getter(oracle_lib):
    nsrc, K, L, D = 1, 16, 2048, 10
    bins = [4, 4, 11]
    per = len(bins)
    taps, shift = random_taps(K, 77, 131)
    keep = []  # (the arrays behind the pointers below)

    def ct(a, dtype=np.int16):
        keep.append(np.ascontiguousarray(a, dtype=dtype))
        return keep[-1].ctypes.data
    good_bins = ct(bins, np.int32)
    # every refusal with a bank set and a history carried: the bank, and the history, stay
    bad = [(K, good_bins, ct([1]), 1, 31, -errno.EINVAL), (K, good_bins, ct([1]), 1, -1, -errno.EINVAL),
           (K, good_bins, None, 3, 0, -errno.EINVAL), (K, good_bins, ct([1]), 0, 0, -errno.EINVAL),
           (K, good_bins, ct([1] * 4097), 4097, 0, -errno.EINVAL), (12, good_bins, ct([1]), 1, 0, -errno.EINVAL),
           (2, good_bins, ct([1]), 1, 0, -errno.EINVAL), (512, good_bins, ct([1]), 1, 0, -errno.EINVAL),
           (4, good_bins, ct([32767] * 4096), 4096, 0, -errno.ERANGE),
           (K, ct([4, K, 11], np.int32), ct([1]), 1, 0, -errno.EINVAL), (K, ct([4, -1, 11], np.int32), ct([1]), 1, 0, -errno.EINVAL),
           (K, None, ct([1]), 1, 0, -errno.EINVAL)]  # (bins == NULL needs per_source == K)
    src = full_scale(nsrc, (len(bad) + 1) * L, 132)
    model = bm.BankModel(K, taps, shift, D, nsrc, bins=bins)
    want, _ = model_runs(model, src, L, (1,) * (len(bad) + 1))
    with demod(raw_cfg(D, L, 1), per) as g:
        assert g.get_channel_bank()[0] == 0
        # channels off: -EINVAL
        assert g.lib.rtlfm_gpu_set_channel_bank(g._h, K, good_bins, ct(taps), taps.size, shift) == -errno.EINVAL
        g.set_channels(per, steps=steps_for(per))
        g.set_channel_bank(K, taps, shift, bins=bins)
        d = torch.from_numpy(src).cuda()
        got = [[] for _ in range(per)]
        for b in range(len(bad) + 1):
            rows, _ = run_once(g, d, L, b, 1)
            for s in range(per):
                got[s].append(rows[s])
            if b < len(bad):
                k_, bp, tp, n, s_, code = bad[b]
                assert g.lib.rtlfm_gpu_set_channel_bank(g._h, k_, bp, tp, n, s_) == code, bad[b]
            gk, gb, gt, gs = g.get_channel_bank()
            assert gk == K and list(gb) == bins and np.array_equal(gt, taps) and gs == shift
        assert_rows([np.concatenate(x) for x in got], want, "after the refusals")
        # the getter's own contract: K, ntaps and shift are written where bins or taps do not fit
        k_, n, s_ = C.c_int(), C.c_int(), C.c_int()
        small = np.zeros(8, dtype=np.int16)
        sb = np.zeros(8, dtype=np.int32)
        assert g.lib.rtlfm_gpu_get_channel_bank(g._h, C.byref(k_), sb.ctypes.data, 8, small.ctypes.data, 8, C.byref(n), C.byref(s_)) == -errno.ENOBUFS
        assert (k_.value, n.value, s_.value) == (K, 77, shift)
        big = np.zeros(4096, dtype=np.int16)
        assert g.lib.rtlfm_gpu_get_channel_bank(g._h, C.byref(k_), sb.ctypes.data, 2, big.ctypes.data, 4096, C.byref(n), C.byref(s_)) == -errno.ENOBUFS
        assert g.lib.rtlfm_gpu_get_channel_bank(g._h, None, sb.ctypes.data, 8, big.ctypes.data, 4096, C.byref(n), C.byref(s_)) == -errno.EINVAL
    # K == 0: the mixer path's bits again, with and without a channel filter that rested while the bank was on, after a
    # bank that was never run and after one that was (D = 8 divides the buffer: the boxcar's partial sums, which the bank
    # does not keep, are zero at every run's end)
    D8 = 8
    src = full_scale(nsrc, 3 * L, 133)
    steps = [12345678, (1 << 32) - 987654321, 1 << 30]
    fir_taps = np.arange(1, 31, dtype=np.int16)
    for with_filter in (False, True):
        with demod(raw_cfg(D8, L, 1), per) as g:
            g.set_channels(per, steps=steps)
            if with_filter:
                g.set_channel_filter(fir_taps, 4)
            want, _ = run_gpu(g, src, L, (1, 1, 1))
            want_st = bytes(g.state_get_all())
        for ran in (False, True):
            with demod(raw_cfg(D8, L, 1), per) as g:
                g.set_channels(per, steps=steps)
                if with_filter:
                    g.set_channel_filter(fir_taps, 4)
                g.set_channel_bank(K, taps, shift, bins=bins)
                d = torch.from_numpy(src).cuda()
                if ran:
                    run_once(g, d, L, 0, 1)
                    g.reset()  # (back to pos 0 and silence, as the handle without a bank starts)
                g.set_channel_bank(0)
                assert g.get_channel_bank()[0] == 0
                if with_filter:
                    assert np.array_equal(g.channel_filter()[0], fir_taps)
                parts = [run_once(g, d, L, b, 1) for b in range(3)]
                assert [p for _, p in parts] == [2] * 3
                assert bytes(g.state_get_all()) == want_st
            assert_rows([np.concatenate([rows[s] for rows, _ in parts]) for s in range(per)], want, f"bank removed, ran={ran}")
    # -ENOTSUP with fifth_order passes, then a run that still equals the model
    cfg = make_cfg(case("p2_fir9")[0], L, 2)
    src = bounded(2, 2 * L, 134, 89)
    st4 = [7 << 20, 3 << 29, 1, 0]
    want, want_len, _ = cm.model_via_oracle(cfg, src, st4, 2, 0)
    with demod(cfg, 4) as g:
        g.set_channels(2, steps=st4)
        assert g.lib.rtlfm_gpu_set_channel_bank(g._h, 4, ct([1, 2], np.int32), ct([1, 2, 1]), 3, 2) == -errno.ENOTSUP
        assert g.get_channel_bank()[0] == 0
        got, paths = run_gpu(g, src, L, (2,))
        assert paths == [1]
    for s in range(4):
        a, b = got[s].astype(np.int32), want[s, :want_len[s]].astype(np.int32)
        assert a.shape == b.shape and np.abs(a - b).max() <= 1 and (a != b).sum() <= max(1, int(1e-4 * a.size)), s  # (-A std: the project's stated tolerance)
    # -EBUSY in a run begun and not ended (the ring: channels off), then the run still equals the oracle
    cfg = make_cfg(case("c1_boxcar10_fast")[0], L, 1)
    rows = synth.random_u8(2, L, seed=135)
    with demod(cfg, 2) as g:
        for s in range(2):
            g.push(rows[s], s)
        assert g.run_begin() == 1
        assert g.lib.rtlfm_gpu_set_channel_bank(g._h, 4, ct([1, 2], np.int32), ct([1, 2, 1]), 3, 2) == -errno.EBUSY
        g.run_end()
        out, lens = g.fetch_all()
        assert g.get_channel_bank()[0] == 0
    want, want_len, _ = oracle_lib.run_batch(cfg, rows)
    for s in range(2):
        assert np.array_equal(out[s, :lens[s]], want[s, :want_len[s]]), s


def test_the_bank_is_one_front_end_launch():
    """timing_read()'s count of a run's front-end launches: the one-launch bank's equals the boxcar's, one; path 1 runs its
    kernels inside one timed pair as well, and last_path tells the two apart."""
    nsrc, K, L, D = 2, 16, 2048, 10
    taps, shift = random_taps(K, 80, 143)
    src = full_scale(nsrc, 3 * L, 141)
    counts = {}
    for kind in ("boxcar", "bank"):
        with demod(raw_cfg(D, L, 3), nsrc * K) as g:
            g.set_channels(K, steps=steps_for(nsrc * K))
            if kind == "bank":
                g.set_channel_bank(K, taps, shift)
            g.timing_enable(True)
            g.timing_read()
            _, paths = run_gpu(g, src, L, (3,))
            assert paths == [2]
            counts[kind] = g.timing_read()[1]
    assert counts["bank"] == counts["boxcar"] == 1, counts
