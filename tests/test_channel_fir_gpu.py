"""The channel filter on the GPU (include/rtlfm_hip.h, rtlfm_gpu_set_channel_filter; csrc/channel_fir_kernel.h) against
tests/channel_fir_model.py: equality of every bit, everywhere.

The filter's own output is compared in -M raw, where it IS the output and full-scale bytes may be used.  The chain behind
it is compared through the existing oracle, which reads bytes: there the inputs are bounded and the taps have a DC gain
of 1 or 2, so that the filtered samples fit a byte (the model asserts it), and buffers are multiples of D, because
full_demod() works buffer by buffer.

The shapes x filters test meets every number of sources, channels per source, block length, D and number of taps the
feature was specified with on both paths; the (D, taps) pairs go round the shapes, three per shape, so that the suite
stays quick - every pair meets at least three shapes, not all eighteen."""
import ctypes as C
import errno
import functools

import numpy as np
import pytest

import channel_fir_model as fm
import channel_model as cm
from cases import case, make_cfg
from channel_common import (BACK, SEEK_TO, assert_call_clears_the_history, assert_rows, bounded, demod, full_scale, make_steps,
                            model_runs, raw_cfg, run_once)
from channel_common import random_fir_taps as random_taps
from channel_common import run_gpu_per_run as run_gpu
from channel_common import tone_fit as tone_error
from rtlsdr_amd import capi, synth
from rtlsdr_amd.capi import ATAN_FAST, MODE_FM

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RUNS = (1, 3, 2)


# ---------------------------------------------------------------- 1. the anchor ----

@pytest.mark.parametrize("D", [4, 10])
@pytest.mark.parametrize("L", [512, 2048])
def test_anchor_ones_are_the_boxcar(D, L):
    """Taps of D ones with shift 0 against the same handle with no filter (k_channel_boxcar): PCM, lengths and the state
    records, -A fast FM on full-scale bytes over runs of 2 and 3 buffers, on both paths.  The records are equal in every
    field but now_r / now_j, which the boxcar uses for its partial sum and the filter carries along unchanged (the
    contract: "copied, not used") - here demod_init()'s zeros."""
    nsrc, per, runs = 2, 3, (2, 3)
    S = nsrc * per
    cfg = make_cfg(dict(mode=MODE_FM, custom_atan=ATAN_FAST, downsample=D), L, 3)
    src = synth.random_u8(nsrc, 5 * L, seed=D * 100 + L)
    steps = make_steps(S, D + L)
    with demod(cfg, S) as g:
        g.set_channels(per, steps=steps)
        want, _, paths = run_gpu(g, src, L, runs)
        want_st = [st.as_dict() for st in g.state_get_all()]
        assert paths == [2, 2]
    for path in (0, 1):
        with demod(cfg, S) as g:
            g.set_path(path)
            g.set_channels(per, steps=steps)
            g.set_channel_filter([1] * D, 0)
            got, _, paths = run_gpu(g, src, L, runs)
            got_st = [st.as_dict() for st in g.state_get_all()]
        assert paths == [2 if path == 0 else 1] * 2
        assert_rows(got, want, f"D={D} L={L} path {path}")
        for s in range(S):
            assert got_st[s]["now_r"] == 0 and got_st[s]["now_j"] == 0
            a = {k: v for k, v in got_st[s].items() if k not in ("now_r", "now_j")}
            b = {k: v for k, v in want_st[s].items() if k not in ("now_r", "now_j")}
            assert a == b, (D, L, path, s)


# ------------------------------------------- 2. shapes x filters, the model, both paths ----

GEOMS = [(nsrc, per, L) for nsrc in (1, 3) for per in (1, 4, 5) for L in (512, 2048, 16384)]
FILTERS = [(D, kind) for D in (4, 10, 64) for kind in ("1", "D", "4D", "8D+3", "1024")]


def ntaps_of(D, kind):
    return {"1": 1, "D": D, "4D": 4 * D, "8D+3": 8 * D + 3, "1024": 1024}[kind]


def general_params():
    out = []
    for gi, (nsrc, per, L) in enumerate(GEOMS):
        for j in range(3):
            D, kind = FILTERS[(gi * 3 + j) % len(FILTERS)]
            out.append(pytest.param(gi, D, kind, id=f"{nsrc}x{per}_L{L}_D{D}_taps{kind}"))
    return out


@functools.lru_cache(maxsize=2)
def geometry(gi):
    nsrc, per, L = GEOMS[gi]
    return nsrc, per, L, full_scale(nsrc, sum(RUNS) * L, 300 + gi), make_steps(nsrc * per, gi)


@pytest.mark.parametrize("gi,D,kind", general_params())
def test_filter_equals_the_model_on_both_paths(gi, D, kind):
    """-M raw on full-scale bytes over runs of 1, 3 and 2 buffers: PCM, lengths and prev_index of path 2 and of path 1
    equal the model's (and so each other's).  256 % 10 != 0: variable counts."""
    nsrc, per, L, src, steps = geometry(gi)
    S = nsrc * per
    ntaps = ntaps_of(D, kind)
    taps, shift = random_taps(ntaps, gi * 31 + ntaps, small=(kind == "D"))
    cfg = raw_cfg(D, L)
    model = fm.FirModel(steps, per, D, taps, shift, nsrc)
    want, _ = model_runs(model, src, L, RUNS)
    for path in (0, 1):
        with demod(cfg, S) as g:
            g.set_path(path)
            g.set_channels(per, steps=steps)
            g.set_channel_filter(taps, shift)
            got, _, paths = run_gpu(g, src, L, RUNS)
            st = g.state_get_all()
            assert g.channels_tell() == sum(RUNS) * L // 2
        assert paths == [2 if path == 0 else 1] * len(RUNS), (path, paths)
        assert_rows(got, want, f"path {path}")
        assert [st[s].prev_index for s in range(S)] == model.p0, path


# ------------------------------------------------------------------ 3. short runs ----

@pytest.mark.parametrize("path", [0, 1])
def test_history_longer_than_a_run_is_shifted(path):
    """1024 taps and single-buffer runs of 256 samples: a run's windows reach four runs back, the tail is shifted."""
    nsrc, per, L, D, nruns = 2, 2, 512, 10, 7
    src = full_scale(nsrc, nruns * L, 51)
    steps = make_steps(nsrc * per, 52)
    taps, shift = random_taps(1024, 53)
    model = fm.FirModel(steps, per, D, taps, shift, nsrc)
    want, _ = model_runs(model, src, L, (1,) * nruns)
    with demod(raw_cfg(D, L, 1), nsrc * per) as g:
        g.set_path(path)
        g.set_channels(per, steps=steps)
        g.set_channel_filter(taps, shift)
        got, _, _ = run_gpu(g, src, L, (1,) * nruns)
    assert_rows(got, want, f"path {path}")


# ------------------------------------------------------- 4. several segments per stream ----

@pytest.mark.parametrize("ntaps", [83, 1024])
def test_segments_equal_the_model(ntaps):
    """4 x 16384 bytes = 32 tiles of the one-launch kernel cut into segments of 1 and of 3 tiles, by fused_min_tiles, and
    left whole: the halo (82 and 1023 samples: less than a tile, and all of one) crosses tile and segment borders, and a
    second run takes its first halo from the carried tail."""
    nsrc, per, L, D, runs = 2, 5, 16384, 10, (4, 4)
    src = full_scale(nsrc, 8 * L, 61)
    steps = make_steps(nsrc * per, 62)
    taps, shift = random_taps(ntaps, 63)
    model = fm.FirModel(steps, per, D, taps, shift, nsrc)
    want, _ = model_runs(model, src, L, runs)
    for opts in (dict(fused_tiles_per_seg=1), dict(fused_tiles_per_seg=3), dict(fused_min_tiles=1, fused_waves=4096),
                 dict(fused_min_tiles=5, fused_waves=4096), dict(fused_min_tiles=64)):
        with demod(raw_cfg(D, L, 4), nsrc * per, **opts) as g:
            g.set_channels(per, steps=steps)
            g.set_channel_filter(taps, shift)
            got, _, paths = run_gpu(g, src, L, runs)
        assert paths == [2, 2]
        assert_rows(got, want, str(opts))


# --------------------------------------------------------------- 5. path switching ----

def test_switching_paths_between_runs_changes_nothing():
    nsrc, per, L, D = 2, 4, 2048, 10
    runs = (1, 2, 1, 3, 1, 1)
    src = full_scale(nsrc, sum(runs) * L, 71)
    steps = make_steps(nsrc * per, 72)
    taps, shift = random_taps(403, 73)
    model = fm.FirModel(steps, per, D, taps, shift, nsrc)
    want, _ = model_runs(model, src, L, runs)
    for paths in ((1, 2, 1, 2, 2, 1), (2, 1, 1, 0, 1, 2)):
        with demod(raw_cfg(D, L, 3), nsrc * per) as g:
            g.set_channels(per, steps=steps)
            g.set_channel_filter(taps, shift)
            got, _, seen = run_gpu(g, src, L, runs, paths=paths)
        assert seen == [1 if p == 1 else 2 for p in paths]
        assert_rows(got, want, str(paths))


# -------------------------------------------------------------------- 6. saturation ----

@pytest.mark.parametrize("path", [0, 1])
def test_saturation_is_reached_and_equals_the_model(path):
    """Bytes 0 and 255 with 64 taps of 32767 and shift 0, the largest filter the check lets through at that length:
    sat16 is reached at both ends, in the model as on the device."""
    nsrc, per, L, D = 1, 5, 2048, 4
    rng = np.random.default_rng(81)
    src = np.repeat(rng.integers(0, 2, size=(nsrc, 3 * L // 32)).astype(np.uint8) * 255, 32, axis=1)  # runs of 16 equal samples
    steps = [0, 1 << 30, 1 << 29, 12345, (1 << 32) - 1]
    taps = np.full(64, 32767, dtype=np.int16)
    assert capi.load().rtlfm_channel_filter_check(taps.ctypes.data, 64, 0) == 0
    model = fm.FirModel(steps, per, D, taps, 0, nsrc)
    want, _ = model_runs(model, src, L, (1, 2))
    assert max(w.max() for w in want) == 32767 and min(w.min() for w in want) == -32768
    with demod(raw_cfg(D, L, 2), nsrc * per) as g:
        g.set_path(path)
        g.set_channels(per, steps=steps)
        g.set_channel_filter(taps, 0)
        got, _, _ = run_gpu(g, src, L, (1, 2))
    assert_rows(got, want, f"path {path}")


# ------------------------------------------------------ 7. the back half, filter on ----

@pytest.mark.parametrize("name", list(BACK))
@pytest.mark.parametrize("path", [0, 1])
def test_back_half_behind_the_filter(oracle_lib, name, path):
    """-A fast FM, AM, the squelch and -L behind the filter equal the existing oracle on the model's filtered samples;
    the levels equal the oracle's rms() of them.  Buffer 1 of every source is silent, for the squelch."""
    nsrc, per, L, D, runs = 2, 3, 2048, 8, (1, 2)
    S = nsrc * per
    from rtlsdr_amd.demod import channel_lowpass
    taps, shift = channel_lowpass(40, 0.4 / D, 1)  # DC gain 1: the filtered samples of bounded bytes fit a byte
    if name.startswith("fm"):
        src = synth.fm_iq_u8(nsrc, 3 * L // 2, fs=2.4e6, dev_hz=50e3, amplitude=55.0, seed=91)
    else:
        src = bounded(nsrc, 3 * L, 92, 60)
    src[:, L:2 * L] = 127
    steps = make_steps(S, 93)
    cfg = make_cfg(dict(BACK[name], downsample=D), L, 2)
    model = fm.FirModel(steps, per, D, taps, shift, nsrc)
    _, per_run = model_runs(model, src, L, runs)
    want, _ = fm.via_oracle(cfg, per_run, runs, L // 2)
    with_levels = bool(cfg.squelch_level or cfg.report_levels)
    with demod(cfg, S) as g:
        g.set_path(path)
        g.set_channels(per, steps=steps)
        g.set_channel_filter(taps, shift)
        d = torch.from_numpy(src).cuda()
        got, b0 = [[] for _ in range(S)], 0
        for (I, Q), nb in zip(per_run, runs, strict=True):
            rows, _ = run_once(g, d, L, b0, nb)
            for s in range(S):
                got[s].append(rows[s])
            if with_levels:
                assert np.array_equal(g.levels_all()[:, :nb], fm.levels_of(I, Q, nb, L // 2 // D)), (name, b0)
            b0 += nb
    assert_rows([np.concatenate(x) for x in got], want, f"{name} path {path}")


# ------------------------------------------------------------------ 8. pos wraps ----

@pytest.mark.parametrize("path", [0, 1])
def test_pos_wraps_at_two_to_the_32(path):
    """channels_seek to just below 2^32, then two runs across it: the tail in front of the second run lies on both
    sides of the wrap."""
    nsrc, per, L, D = 2, 4, 2048, 10
    pos = (1 << 32) - 700
    src = full_scale(nsrc, 3 * L, 101)
    steps = make_steps(nsrc * per, 102)
    taps, shift = random_taps(803, 103)
    model = fm.FirModel(steps, per, D, taps, shift, nsrc)
    model.seek(pos)
    want, _ = model_runs(model, src, L, (1, 2))
    with demod(raw_cfg(D, L, 2), nsrc * per) as g:
        g.set_path(path)
        g.set_channels(per, steps=steps)
        g.set_channel_filter(taps, shift)
        g.channels_seek(pos)
        got, _, _ = run_gpu(g, src, L, (1, 2))
        assert g.channels_tell() == pos + 3 * L // 2
    assert_rows(got, want, f"path {path}")


# -------------------------------------------------------------------- 9. clearing ----

CLEARERS = ("set_channel_filter", "set_channels", "reset", "channels_seek")


@pytest.mark.parametrize("what", CLEARERS)
@pytest.mark.parametrize("path", [0, 1])
def test_each_of_the_four_calls_clears_the_history(what, path):
    """A run, the call, a run: the second run equals the model with the history cleared by the call - and differs from
    the model that kept it, so a call that does not clear fails here."""
    nsrc, per, L, D = 2, 2, 512, 8  # (256 % 8 == 0: prev_index stays 0 whatever the call does to the records)
    src = full_scale(nsrc, 2 * L, 111)
    steps = make_steps(nsrc * per, 112)
    taps, shift = random_taps(300, 113)

    def handle():
        g = demod(raw_cfg(D, L, 1), nsrc * per)
        g.set_path(path)
        g.set_channels(per, steps=steps)
        g.set_channel_filter(taps, shift)
        return g
    calls = {"set_channel_filter": lambda g: g.set_channel_filter(taps, shift),
             "set_channels": lambda g: g.set_channels(per, steps=steps),
             "reset": lambda g: g.reset(),
             "channels_seek": lambda g: g.channels_seek(SEEK_TO)}
    assert_call_clears_the_history(lambda: fm.FirModel(steps, per, D, taps, shift, nsrc), handle, calls, what, src, L,
                                   f"{what} path {path}")


# ---------------------------------------------------------------- 10. verify_twice ----

@pytest.mark.parametrize("path", [0, 1])
def test_verify_twice_sees_one_pos_and_one_tail(path):
    nsrc, per, L, D = 1, 4, 2048, 10
    src = full_scale(nsrc, 4 * L, 121)
    steps = make_steps(nsrc * per, 122)
    taps, shift = random_taps(500, 123)
    model = fm.FirModel(steps, per, D, taps, shift, nsrc)
    want, _ = model_runs(model, src, L, (2, 1, 1))
    with demod(raw_cfg(D, L, 2), nsrc * per, verify_twice=1) as g:
        g.set_path(path)
        g.set_channels(per, steps=steps)
        g.set_channel_filter(taps, shift)
        got, _, _ = run_gpu(g, src, L, (2, 1, 1))
        assert g.channels_tell() == 4 * L // 2
        assert g.get_option("verify_runs") == 3 and g.get_option("verify_mismatches") == 0
    assert_rows(got, want, f"path {path}")


# ----------------------------------------------------------- 11. adjacent channels ----

def test_two_fm_carriers_one_spacing_apart(oracle_lib):
    """Two FM carriers one channel spacing (fs / D) apart in one source, demodulated as two channels with /10 and -A fast.
    Behind rtlfm_channel_lowpass(80, 0.04) the device's PCM equals the model's, and the model's audio is closer to the
    modulating tone than the boxcar model's, in both channels."""
    from rtlsdr_amd.demod import channel_lowpass
    fs, L, nb, D = 2_400_000, 20480, 2, 10  # (buffers of 10240 samples: a multiple of D, for the oracle behind the model)
    offs, tones = (-120_000, 120_000), (2000.0, 3000.0)
    n = np.arange(nb * L // 2, dtype=np.float64)
    sig = np.zeros(n.size, dtype=np.complex128)
    for f, tone in zip(offs, tones, strict=True):
        sig += 40.0 * np.exp(1j * (2 * np.pi * f * n / fs + (30e3 / tone) * np.sin(2 * np.pi * tone * n / fs)))
    src = np.empty((1, nb * L), dtype=np.uint8)
    src[0, 0::2] = np.rint(127 + sig.real).astype(np.uint8)
    src[0, 1::2] = np.rint(127 + sig.imag).astype(np.uint8)
    steps = [cm.step_from_hz(f, fs) for f in offs]
    cfg = make_cfg(case("c1_boxcar10_fast")[0], L, nb)
    assert cfg.downsample == D and cfg.mode == MODE_FM
    taps, shift = channel_lowpass(80, 0.04, 2)  # DC gain 2: amplitude 80, inside a byte
    model = fm.FirModel(steps, 2, D, taps, shift, 1)
    _, per_run = model_runs(model, src, L, (nb,))
    want, _ = fm.via_oracle(cfg, per_run, (nb,), L // 2)
    box, box_len, _ = cm.model_via_oracle(cfg, src, steps, 2, 0)
    with demod(cfg, 2) as g:
        g.set_channels(2, steps=steps)
        g.set_channel_filter(taps, shift)
        got, _, paths = run_gpu(g, src, L, (nb,))
    assert paths == [2]
    assert_rows(got, want, "two carriers")
    for s in range(2):
        e_fir, a_fir = tone_error(want[s], tones[s], fs / D, 16)
        e_box, a_box = tone_error(box[s, :box_len[s]], tones[s], fs / D, 16)
        assert a_fir > 1000 and a_box > 1000, (s, a_fir, a_box)  # both did demodulate the tone
        assert e_fir < e_box, (s, e_fir, e_box)


# ------------------------------------------------------ 12. refusals and the getter ----

def test_refusals_change_nothing_and_the_getter(oracle_lib):
    nsrc, per, L, D = 1, 2, 2048, 10
    S = nsrc * per
    steps = [12345678, (1 << 32) - 987654321]
    taps, shift = random_taps(77, 131)
    keep = []  # (the arrays behind the pointers below)

    def ct(a):
        keep.append(np.ascontiguousarray(a, dtype=np.int16))
        return keep[-1].ctypes.data
    # -EINVAL / -ERANGE with a filter set and a history carried: the filter, and the history, stay
    bad = [(ct([1]), 1, 31, -errno.EINVAL), (ct([1]), 1, -1, -errno.EINVAL), (None, 3, 0, -errno.EINVAL), (ct([1]), -1, 0, -errno.EINVAL),
           (ct([1] * 1025), 1025, 0, -errno.EINVAL), (ct([32767] * 1024), 1024, 0, -errno.ERANGE)]
    src = full_scale(nsrc, (len(bad) + 1) * L, 132)
    model = fm.FirModel(steps, per, D, taps, shift, nsrc)
    want, _ = model_runs(model, src, L, (1,) * (len(bad) + 1))
    with demod(raw_cfg(D, L, 1), S) as g:
        t, sh = g.channel_filter()
        assert t.size == 0 and sh == 0
        g.set_channel_filter(taps, shift)  # (channels still off: kept)
        g.set_channels(per, steps=steps)
        d = torch.from_numpy(src).cuda()
        got = [[] for _ in range(S)]
        for b in range(len(bad) + 1):
            rows, _ = run_once(g, d, L, b, 1)
            for s in range(S):
                got[s].append(rows[s])
            if b < len(bad):
                p, n, s_, code = bad[b]
                assert g.lib.rtlfm_gpu_set_channel_filter(g._h, p, n, s_) == code, bad[b][1:]
            t, sh = g.channel_filter()
            assert np.array_equal(t, taps) and sh == shift
        assert_rows([np.concatenate(x) for x in got], want, "after -EINVAL / -ERANGE")
        # the getter's own contract: the count is written where the taps do not fit
        n, s_ = C.c_int(), C.c_int()
        small = np.zeros(8, dtype=np.int16)
        assert g.lib.rtlfm_gpu_get_channel_filter(g._h, small.ctypes.data, 8, C.byref(n), C.byref(s_)) == -errno.ENOBUFS
        assert n.value == 77 and s_.value == shift
        assert g.lib.rtlfm_gpu_get_channel_filter(g._h, small.ctypes.data, 8, None, C.byref(s_)) == -errno.EINVAL
    # ntaps == 0: the boxcar's bits again, after a filter that was never run and after one that was (D = 8 divides the
    # buffer: the boxcar's partial sums, which the filter does not keep, are zero at every run's end)
    D8 = 8
    src = full_scale(nsrc, 3 * L, 133)
    with demod(raw_cfg(D8, L, 1), S) as g:
        g.set_channels(per, steps=steps)
        want, _, _ = run_gpu(g, src, L, (1, 1, 1))
        want_st = bytes(g.state_get_all())
    for ran in (False, True):
        with demod(raw_cfg(D8, L, 1), S) as g:
            g.set_channels(per, steps=steps)
            g.set_channel_filter([1] * D8, 0)
            d = torch.from_numpy(src).cuda()
            parts = [run_once(g, d, L, 0, 1)] if ran else []
            g.set_channel_filter(None)
            assert g.channel_filter()[0].size == 0
            parts += [run_once(g, d, L, b, 1) for b in range(len(parts), 3)]
            assert [p for _, p in parts] == [2] * 3
            assert bytes(g.state_get_all()) == want_st
        assert_rows([np.concatenate([rows[s] for rows, _ in parts]) for s in range(S)], want, f"filter removed, ran={ran}")
    # -ENOTSUP with fifth_order passes, then a run that still equals the model
    cfg = make_cfg(case("p2_fir9")[0], L, 2)
    src = bounded(2, 2 * L, 134, 89)
    st4 = [7 << 20, 3 << 29, 1, 0]
    want, want_len, _ = cm.model_via_oracle(cfg, src, st4, 2, 0)
    with demod(cfg, 4) as g:
        g.set_channels(2, steps=st4)
        assert g.lib.rtlfm_gpu_set_channel_filter(g._h, ct([1, 2, 1]), 3, 2) == -errno.ENOTSUP
        assert g.lib.rtlfm_gpu_set_channel_filter(g._h, None, 0, 0) == -errno.ENOTSUP
        assert g.channel_filter()[0].size == 0
        got, _, paths = run_gpu(g, src, L, (2,))
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
        assert g.lib.rtlfm_gpu_set_channel_filter(g._h, ct([1, 2, 1]), 3, 2) == -errno.EBUSY
        g.run_end()
        out, lens = g.fetch_all()
        assert g.channel_filter()[0].size == 0
    want, want_len, _ = oracle_lib.run_batch(cfg, rows)
    for s in range(2):
        assert np.array_equal(out[s, :lens[s]], want[s, :want_len[s]]), s


# ------------------------------------------------------------------ 13. launch counts ----

def test_the_filter_adds_no_launch():
    """timing_read()'s count of a run's front-end launches: the one-launch filter's equals the boxcar's."""
    nsrc, per, L, D = 2, 4, 2048, 10
    src = full_scale(nsrc, 3 * L, 141)
    steps = make_steps(nsrc * per, 142)
    taps, shift = random_taps(80, 143)
    counts = {}
    for kind in ("boxcar", "filter"):
        with demod(raw_cfg(D, L, 3), nsrc * per) as g:
            g.set_channels(per, steps=steps)
            if kind == "filter":
                g.set_channel_filter(taps, shift)
            g.timing_enable(True)
            g.timing_read()
            _, _, paths = run_gpu(g, src, L, (3,))
            assert paths == [2]
            counts[kind] = g.timing_read()[1]
    assert counts["filter"] == counts["boxcar"] == 1, counts
