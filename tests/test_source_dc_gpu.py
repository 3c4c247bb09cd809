"""Option source_dc on the GPU (include/rtlfm_hip.h, "source_dc"): the raw DC block per source in front of the boxcar, the
channel filter and the bank, bit for bit against tests/source_dc_model.py on paths 0 / 2 and 1, with the path switched
between runs.  Shapes: the smallest at which each mechanism can fail - buffers of 512 bytes (16 per boxcar tile, 4 per
filter tile) up to 16384 (two boxcar tiles), runs of 1, 3 and 17 buffers (17 x 256 samples replace the whole history, 3
shift it), 1 and 3 sources, 1 and 5 channels (two workgroup groups, one with idle waves)."""
import ctypes as C
import errno

import numpy as np
import pytest

import channel_bank_model as bm
import channel_fir_model as fm
import channel_model as cm
import packed_model as pm
import source_dc_model as sdm
from cases import case, make_cfg
from channel_common import (SEEK_TO, assert_call_clears_the_history, assert_row_cfg, assert_rows, demod, make_steps, random_bank_taps,
                            random_fir_taps, raw_cfg, run_gpu_per_run, run_once, steps_for, to_device)
from channel_fir_model import raw_rows
from rtlsdr_amd import channel_lowpass
from rtlsdr_amd.capi import ATAN_FAST, MODE_FM

pytestmark = pytest.mark.gpu

OFFS = (9, -14, 30)


def offsets(nsrc, nbuf):
    """Another offset per source, per buffer and per component, I != Q: a wrong buffer or source index shows."""
    o = np.empty((nsrc, nbuf, 2), dtype=np.int64)
    for a in range(nsrc):
        for b in range(nbuf):
            o[a, b] = (OFFS[(a + b) % 3], OFFS[(a + b + 1) % 3])
    return o


def with_offsets(noise, L):
    """noise: int64 [sources, bytes] around 0 -> uint8 bytes around 127 + the buffer's offset, clipped to a byte."""
    nsrc, nbuf = noise.shape[0], noise.shape[1] // L
    v = noise.reshape(nsrc, nbuf, L // 2, 2) + offsets(nsrc, nbuf)[:, :, None, :] + 127
    return np.clip(v, 0, 255).astype(np.uint8).reshape(nsrc, nbuf * L)


def bounded_src(nsrc, L, nbuf, seed, bound=30):
    rng = np.random.default_rng(seed)
    return with_offsets(rng.integers(-bound, bound + 1, size=(nsrc, nbuf * L)).astype(np.int64), L)


def full_scale_src(nsrc, L, nbuf, seed):
    """Every byte value, stretches of pure 0 / 255 in source 0 - the offsets ride on the buffers that do not clip."""
    rng = np.random.default_rng(seed)
    src = with_offsets(rng.integers(-127, 129, size=(nsrc, nbuf * L)).astype(np.int64), L)
    src[0, : L // 2] = rng.integers(0, 2, size=L // 2).astype(np.uint8) * 255
    return src


def chan_handle(cfg, nsrc, per, steps, path=0, dc=1, **options):
    g = demod(cfg, nsrc * per, **options)
    g.set_path(path)
    g.set_channels(per, steps=steps)
    if dc:
        g.set_option("source_dc", 1)
    return g


def fir_handle(cfg, nsrc, per, steps, taps, shift, path=0, dc=1, **options):
    g = chan_handle(cfg, nsrc, per, steps, path, dc, **options)
    g.set_channel_filter(taps, shift)
    return g


def bank_handle(cfg, nsrc, K, bins, taps, shift, path=0, dc=1, **options):
    per = K if bins is None else len(bins)
    g = chan_handle(cfg, nsrc, per, steps_for(nsrc * per), path, dc, **options)
    g.set_channel_bank(K, taps, shift, bins=bins)
    return g


def assert_records(g, model, what):
    """Every channel of a source holds the model's averages."""
    st = g.state_get_all()
    got = [[st[s].dc_avgI, st[s].dc_avgQ] for s in range(g.nstreams)]
    assert got == model.rec, (what, got, model.rec)


def model_rows(model, src, L, runs):
    per_run, b0 = [], 0
    for nb in runs:
        per_run.append(raw_rows(*model.run(src[:, b0 * L:(b0 + nb) * L], L)))
        b0 += nb
    return [np.concatenate([r[s] for r in per_run]) for s in range(model.S)], per_run


def paths_for(runs, first):
    return [(first + r) % 2 for r in range(len(runs))]  # 0 (-> 2 or 1, the handle's own choice) and 1, switched between runs


# ------------------------------------------------------------------- the boxcar ----

BOX_FM = [(1, 1, 512, (1, 3, 17)), (3, 5, 2048, (1, 3, 17)), (1, 5, 8192, (1, 3, 2)), (3, 1, 16384, (1, 3, 1))]


@pytest.mark.parametrize("nsrc, per, L, runs", BOX_FM)
@pytest.mark.parametrize("first", [0, 1])
def test_boxcar_fm_through_the_oracle(oracle_lib, nsrc, per, L, runs, first):
    """/10 -M fm -A fast: the model's mixed samples, asserted to fit a byte, through the existing oracle with the handle's own
    cfg and offset_tuning = 1 - rms() keeps its DC fix, as cfg.dc_block_raw is 0.  Three runs, the state carried."""
    from oracle import pyoracle as po
    cfg = make_cfg(case("c1_boxcar10_fast")[0], L, max(runs))
    steps = make_steps(nsrc * per, 3 + L)
    src = bounded_src(nsrc, L, sum(runs), L + per)
    model = sdm.DcBoxModel(steps, per, cfg.downsample, nsrc)
    want, states, b0 = [], None, 0
    for nb in runs:
        out, n, states = po.run_batch(cm.copy_cfg(cfg, offset_tuning=1), model.mixed_bytes(src[:, b0 * L:(b0 + nb) * L], L), states, nthreads=4)
        want.append([out[s, :n[s]].copy() for s in range(nsrc * per)])
        b0 += nb
    paths = paths_for(runs, first)
    with chan_handle(cfg, nsrc, per, steps) as g:
        _, got, seen = run_gpu_per_run(g, src, L, runs, paths)
        assert seen == [2 if p == 0 else 1 for p in paths], seen
        assert_records(g, model, "after the runs")
        st = g.state_get_all()
        for s in range(nsrc * per):
            assert st[s].prev_index == states[s].prev_index and st[s].now_r == states[s].now_r and st[s].now_j == states[s].now_j
    for r in range(len(runs)):
        assert_rows(got[r], want[r], f"run {r} path {paths[r]}")


BOX_RAW = [(3, 5, 512, (1, 3, 17), {}), (3, 5, 2048, (3, 17, 1), dict(fused_tiles_per_seg=1)),
           (1, 5, 2048, (3, 17, 1), dict(fused_tiles_per_seg=3)), (1, 1, 16384, (1, 3, 1), dict(fused_tiles_per_seg=1)),
           (3, 1, 8192, (1, 3, 2), dict(fused_min_tiles=1, fused_waves=4096))]


@pytest.mark.parametrize("nsrc, per, L, runs, opts", BOX_RAW, ids=[f"{c[0]}x{c[1]}-{c[2]}-{i}" for i, c in enumerate(BOX_RAW)])
def test_boxcar_raw_full_scale_and_segments(nsrc, per, L, runs, opts):
    """/7 -M raw on full-scale bytes, the launch's rows being the output.  Segments of one tile: at 2048-byte buffers a later
    segment's warm-up tile crosses buffer boundaries, at 16384 a segment boundary falls inside a buffer."""
    D = 7
    steps = make_steps(nsrc * per, 11 + L)
    src = full_scale_src(nsrc, L, sum(runs), 5 + L)
    model = sdm.DcBoxModel(steps, per, D, nsrc)
    want, b0 = [], 0
    for nb in runs:
        want.append(model.run(src[:, b0 * L:(b0 + nb) * L], L))
        b0 += nb
    paths = paths_for(runs, 0)
    with chan_handle(raw_cfg(D, L, max(runs)), nsrc, per, steps, **opts) as g:
        _, got, seen = run_gpu_per_run(g, src, L, runs, paths)
        assert seen == [2 if p == 0 else 1 for p in paths], seen
        assert_records(g, model, "after the runs")
        st = g.state_get_all()
        for s in range(nsrc * per):
            assert {k: getattr(st[s], k) for k in ("now_r", "now_j", "prev_index")} == model.state[s], s
    for r in range(len(runs)):
        assert_rows(got[r], want[r], f"run {r} path {paths[r]}")


def test_fifth_order_passes_behind_the_mixers(oracle_lib):
    """p2_fir9: no boxcar, so path 0 is the staged kernels behind k_channel_mix - with the option, k_channel_mix<true>."""
    from oracle import pyoracle as po
    nsrc, per, L, runs = 2, 2, 2048, (1, 3)
    cfg = make_cfg(case("p2_fir9")[0], L, max(runs))
    steps = make_steps(nsrc * per, 17)
    src = bounded_src(nsrc, L, sum(runs), 77)
    model = sdm.DcBoxModel(steps, per, 1, nsrc)
    want, states, b0 = [], None, 0
    for nb in runs:
        out, n, states = po.run_batch(cm.copy_cfg(cfg, offset_tuning=1), model.mixed_bytes(src[:, b0 * L:(b0 + nb) * L], L), states, nthreads=4)
        want.append([out[s, :n[s]].copy() for s in range(nsrc * per)])
        b0 += nb
    with chan_handle(cfg, nsrc, per, steps) as g:
        _, got, seen = run_gpu_per_run(g, src, L, runs)
        assert seen == [1, 1]
        assert_records(g, model, "after the runs")
    for r in range(len(runs)):
        for s in range(nsrc * per):
            assert_row_cfg(got[r][s], want[r][s], cfg, f"run {r} stream {s}")


# ------------------------------------------------------------------- the filter ----

FIR = [(33, 7, 512, 3, 5, (1, 3, 17), {}), (1024, 10, 512, 1, 5, (1, 3, 17), {}), (1024, 7, 2048, 3, 1, (3, 1, 17), dict(fused_tiles_per_seg=1)),
       (33, 10, 16384, 1, 1, (1, 3, 1), {}), (1024, 10, 8192, 1, 5, (1, 3, 2), dict(fused_tiles_per_seg=3))]


@pytest.mark.parametrize("ntaps, D, L, nsrc, per, runs, opts", FIR, ids=[f"{c[0]}taps-{c[2]}" for c in FIR])
@pytest.mark.parametrize("first", [0, 1])
def test_filter_equals_the_model(ntaps, D, L, nsrc, per, runs, opts, first):
    """-M raw on full-scale bytes.  At 512-byte buffers the 1024-tap halo reaches four buffers back and, in a run's first
    tiles, into the history: every dword finds the pair it was consumed with."""
    taps, shift = random_fir_taps(ntaps, 100 + ntaps)
    steps = make_steps(nsrc * per, 7 + L)
    src = full_scale_src(nsrc, L, sum(runs), 9 + ntaps + L)
    model = sdm.DcFirModel(steps, per, D, taps, shift, nsrc)
    _, want = model_rows(model, src, L, runs)
    paths = paths_for(runs, first)
    with fir_handle(raw_cfg(D, L, max(runs)), nsrc, per, steps, taps, shift, **opts) as g:
        _, got, seen = run_gpu_per_run(g, src, L, runs, paths)
        assert seen == [2 if p == 0 else 1 for p in paths], seen
        assert_records(g, model, "after the runs")
        st = g.state_get_all()
        assert [st[s].prev_index for s in range(nsrc * per)] == model.p0
    for r in range(len(runs)):
        assert_rows(got[r], want[r], f"run {r} path {paths[r]}")


# --------------------------------------------------------------------- the bank ----

BANK = [(4, None, 64, 10, 512, 3, (1, 3, 17)), (16, [0, 5, 5], 300, 7, 2048, 3, (3, 17, 1)), (256, [0], 1024, 10, 8192, 1, (1, 3, 2)),
        (16, None, 4096, 10, 16384, 1, (1, 3, 1)), (256, None, 512, 10, 2048, 1, (1, 3))]


@pytest.mark.parametrize("K, bins, ntaps, D, L, nsrc, runs", BANK, ids=[f"K{c[0]}-{c[2]}taps-{c[4]}" for c in BANK])
@pytest.mark.parametrize("first", [0, 1])
def test_bank_equals_the_model(K, bins, ntaps, D, L, nsrc, runs, first):
    taps, shift = random_bank_taps(K, ntaps, 200 + K)
    src = full_scale_src(nsrc, L, sum(runs), 13 + K + L)
    model = sdm.DcBankModel(K, taps, shift, D, nsrc, bins=bins)
    _, want = model_rows(model, src, L, runs)
    paths = paths_for(runs, first)
    with bank_handle(raw_cfg(D, L, max(runs)), nsrc, K, bins, taps, shift) as g:
        _, got, seen = run_gpu_per_run(g, src, L, runs, paths)
        assert seen == [2 if p == 0 else 1 for p in paths], seen
        assert_records(g, model, "after the runs")
        st = g.state_get_all()
        assert [st[s].prev_index for s in range(g.nstreams)] == model.p0
    for r in range(len(runs)):
        assert_rows(got[r], want[r], f"run {r} path {paths[r]}")


@pytest.mark.parametrize("first", [0, 1])
def test_bank_survey_equals_the_model(first):
    """bank_survey on: every bin's power and the frames of every run, on both paths, segments of one tile."""
    nsrc, K, L, D, runs = 3, 16, 2048, 7, (3, 17, 1)
    bins = [3, 0]
    taps, shift = random_bank_taps(K, 300, 31)
    src = full_scale_src(nsrc, L, sum(runs), 41)
    model = sdm.DcBankModel(K, taps, shift, D, nsrc, bins=bins)
    paths = paths_for(runs, first)
    with bank_handle(raw_cfg(D, L, max(runs)), nsrc, K, bins, taps, shift, bank_survey=1, fused_tiles_per_seg=1) as g:
        d, b0 = to_device(src), 0
        for r, nb in enumerate(runs):
            g.set_path(paths[r])
            got, _ = run_once(g, d, L, b0, nb)
            power, frames = g.bank_survey()
            I, Q, want_power, want_frames = model.run(src[:, b0 * L:(b0 + nb) * L], L, survey=True)
            assert_rows(got, raw_rows(I, Q), f"run {r} path {paths[r]}")
            assert np.array_equal(frames, want_frames), (r, frames, want_frames)
            assert np.array_equal(power, want_power), (r, np.argwhere(power != want_power)[:4])
            b0 += nb


def test_bin_0_loses_the_spike():
    """What the option is for: constant bytes (140, 110) - a DC spike of (13, -17) - plus a carrier of amplitude 8 in bin 3.
    With the option on, after the averages have settled, bin 0's power is below bin 3's; on a twin with it off it is above.
    (rdc_block_const 1: the integer recurrence stops within k of the mean, as the reference's does - at k = 9 what is left of
    this spike would still outweigh so small a carrier.)"""
    K, L, D, nb = 16, 2048, 8, 8
    taps, shift = channel_lowpass(128, 0.4 / K, K)  # (gain K: fix_fft's halvings take it back, a bin holds the carrier's amplitude)
    n = np.arange(2 * nb * L // 2)
    src = np.empty((1, 2 * nb * L), dtype=np.uint8)
    src[0, 0::2] = np.rint(140 + 8 * np.cos(2 * np.pi * 3 * n / K)).astype(np.uint8)
    src[0, 1::2] = np.rint(110 + 8 * np.sin(2 * np.pi * 3 * n / K)).astype(np.uint8)
    cfg = raw_cfg(D, L, nb, rdc_block_const=1)
    power = {}
    for dc in (1, 0):
        with bank_handle(cfg, 1, K, [0, 3], taps, shift, dc=dc, bank_survey=1) as g:
            d = to_device(src)
            run_once(g, d, L, 0, nb)
            run_once(g, d, L, nb, nb)
            power[dc], _ = g.bank_survey()
            if dc:
                assert_records(g, sdm_settled(src, L), "settled")
    assert power[1][0, 0] < power[1][0, 3], power[1][0, :4]
    assert power[0][0, 0] > power[0][0, 3], power[0][0, :4]


def sdm_settled(src, L):
    m = sdm.SourceDc(1, 2, k=1)
    m.front(src, L)
    assert m.rec[0] == [12, -16]  # (13, -17), within k = 1
    return m


# ------------------------------------------------------------------- the record ----

@pytest.mark.parametrize("path", [0, 1])
def test_channel_zero_rules_and_a_broken_record_is_clamped(path):
    """state_set with other averages on channel 0 and channel 1: channel 0's are the source's.  dc_avgI = 1000000: clamped on
    the way in - the run equals the model, which clamps."""
    nsrc, per, L, D = 2, 2, 512, 7
    taps, shift = random_fir_taps(33, 5)
    steps = make_steps(nsrc * per, 23)
    src = full_scale_src(nsrc, L, 4, 61)
    model = sdm.DcFirModel(steps, per, D, taps, shift, nsrc)
    with fir_handle(raw_cfg(D, L, 3), nsrc, per, steps, taps, shift, path) as g:
        d = to_device(src)
        got0, _ = run_once(g, d, L, 0, 1)
        assert_rows(got0, raw_rows(*model.run(src[:, :L], L)), "run 0")
        model.rec = [[50, -60], [-3, 7], [1000000, -1000000], [1, 2]]
        for s, (ai, aq) in enumerate(model.rec):
            st = g.state_get(s)
            st.dc_avgI, st.dc_avgQ = ai, aq
            g.state_set(s, st)
        st = g.state_get_all()
        assert [[st[s].dc_avgI, st[s].dc_avgQ] for s in range(4)] == model.rec  # (seen per channel, as set)
        got1, _ = run_once(g, d, L, 1, 3)
        assert_rows(got1, raw_rows(*model.run(src[:, L:], L)), "run 1")
        assert_records(g, model, "after run 1")
    assert model.rec[0] == model.rec[1] and model.rec[2] == model.rec[3] and model.rec[0] != model.rec[2]


# ---------------------------------------------------------------- the lifecycle ----

def lifecycle_case():
    nsrc, per, L, D = 2, 2, 512, 8  # (256 % 8 == 0: prev_index stays 0 whatever a call does to the records)
    taps, shift = random_fir_taps(300, 71)
    return nsrc, per, L, D, taps, shift, steps_for(nsrc * per), full_scale_src(nsrc, L, 2, 73)


@pytest.mark.parametrize("path", [0, 1])
def test_switching_the_option_clears_the_history_and_leaves_the_records(path):
    nsrc, per, L, D, taps, shift, steps, src = lifecycle_case()

    def new_model():
        m = sdm.DcFirModel(steps, per, D, taps, shift, nsrc)
        m.L = L
        return m

    def off_on(g):
        before = bytes(g.state_get_all())
        g.set_option("source_dc", 0)
        assert g.get_option("source_dc") == 0
        g.set_option("source_dc", 1)
        assert bytes(g.state_get_all()) == before
    assert_call_clears_the_history(new_model, lambda: fir_handle(raw_cfg(D, L, 1), nsrc, per, steps, taps, shift, path),
                                   {"source_dc": off_on}, "source_dc", src, L, f"off and on, path {path}")
    # on -> off: the next run is the existing model's on a cleared history, at the handle's pos
    m = new_model()
    m.run(src[:, :L])
    plain = fm.FirModel(steps, per, D, taps, shift, nsrc)
    plain.pos, plain.p0 = m.pos, list(m.p0)
    with fir_handle(raw_cfg(D, L, 1), nsrc, per, steps, taps, shift, path) as g:
        d = to_device(src)
        run_once(g, d, L, 0, 1)
        g.set_option("source_dc", 0)
        got, _ = run_once(g, d, L, 1, 1)
        assert_records(g, m, "the records stay where the last run with the option left them")
    assert_rows(got, raw_rows(*plain.run(src[:, L:])), f"on and off, path {path}")


CLEARERS = ("set_channel_filter", "set_channel_bank", "set_channels", "reset", "channels_seek")


@pytest.mark.parametrize("what", CLEARERS)
@pytest.mark.parametrize("path", [0, 1])
def test_each_clearing_call_clears_what_was_subtracted_too(what, path):
    """A run, the call, a run: the second run equals the model with x = y = 0 in front of it - the bytes back at 127 AND
    nothing subtracted from them; pairs left standing would make the cleared history -a instead of 0."""
    nsrc, per, L, D, taps, shift, steps, src = lifecycle_case()
    K, bins = 16, [1, 6]
    btaps, bshift = random_bank_taps(K, 300, 79)
    bank = what == "set_channel_bank"

    def new_model():
        return sdm.DcBankModel(K, btaps, bshift, D, nsrc, bins=bins) if bank else sdm.DcFirModel(steps, per, D, taps, shift, nsrc)

    def again(g):
        g.set_channels(per, steps=steps)
        g.set_channel_filter(taps, shift)
    calls = {"set_channel_filter": lambda g: g.set_channel_filter(taps, shift),
             "set_channel_bank": lambda g: g.set_channel_bank(K, btaps, bshift, bins=bins),
             "set_channels": again,
             "reset": lambda g: g.reset(),
             "channels_seek": lambda g: g.channels_seek(SEEK_TO)}
    cleared, kept = new_model(), new_model()
    for m in (cleared, kept):
        m.run(src[:, :L], L)
        if what in ("set_channels", "reset"):
            m.pos = 0
        if what == "reset":
            m.rec = [[0, 0] for _ in range(m.S)]
        if what == "channels_seek":
            m.pos = SEEK_TO
    cleared.clear()
    want, unwanted = raw_rows(*cleared.run(src[:, L:], L)), raw_rows(*kept.run(src[:, L:], L))
    assert not any(np.array_equal(a, b) for a, b in zip(want, unwanted, strict=True))
    cfg = raw_cfg(D, L, 1)
    with (bank_handle(cfg, nsrc, K, bins, btaps, bshift, path) if bank else fir_handle(cfg, nsrc, per, steps, taps, shift, path)) as g:
        d = to_device(src)
        run_once(g, d, L, 0, 1)
        calls[what](g)
        assert g.get_option("source_dc") == 1
        got, _ = run_once(g, d, L, 1, 1)
    assert_rows(got, want, f"{what} path {path}")


@pytest.mark.parametrize("front", ["boxcar", "fir", "bank"])
@pytest.mark.parametrize("path", [0, 1])
def test_verify_twice_uses_one_set_of_averages_and_one_history(front, path):
    nsrc, per, L, D, runs = 2, 2, 2048, 7, (2, 1, 1)
    steps = make_steps(nsrc * per, 29)
    src = full_scale_src(nsrc, L, sum(runs), 83)
    cfg = raw_cfg(D, L, 2)
    if front == "boxcar":
        model = sdm.DcBoxModel(steps, per, D, nsrc)
        open_it = lambda: chan_handle(cfg, nsrc, per, steps, path, verify_twice=1)  # noqa: E731
    elif front == "fir":
        taps, shift = random_fir_taps(200, 3)
        model = sdm.DcFirModel(steps, per, D, taps, shift, nsrc)
        open_it = lambda: fir_handle(cfg, nsrc, per, steps, taps, shift, path, verify_twice=1)  # noqa: E731
    else:
        taps, shift = random_bank_taps(16, 200, 3)
        model = sdm.DcBankModel(16, taps, shift, D, nsrc, bins=[2, 9])
        open_it = lambda: bank_handle(cfg, nsrc, 16, [2, 9], taps, shift, path, verify_twice=1)  # noqa: E731
    want, b0 = [], 0
    for nb in runs:
        out = model.run(src[:, b0 * L:(b0 + nb) * L], L)
        want.append(out if front == "boxcar" else raw_rows(*out))
        b0 += nb
    with open_it() as g:
        _, got, _ = run_gpu_per_run(g, src, L, runs)
        assert g.get_option("verify_runs") == 3 and g.get_option("verify_mismatches") == 0
        assert_records(g, model, "after the runs")
    for r in range(len(runs)):
        assert_rows(got[r], want[r], f"{front} run {r} path {path}")


def push_run(g, src, pieces):
    for i in range(src.shape[0]):
        for at, n in pieces:
            g.rtlsdr_callback(src[i, at:at + n], stream=i)


def fetch_rows(g, prev=False):
    o, n = g.fetch_all_prev() if prev else g.fetch_all()
    return [o[s, :n[s]].copy() for s in range(g.nstreams)]


@pytest.mark.parametrize("front", ["fir", "bank"])
def test_source_ring_with_a_short_buffer_and_prev(front):
    """A 512-byte buffer among 2048-byte ones over the source ring: a short buffer is a run of one buffer of its own length -
    its own average, its own pieces of the history.  The run before the last stays fetchable."""
    nsrc, per, L, D = 2, 2, 2048, 7
    steps = make_steps(nsrc * per, 37)
    src = full_scale_src(nsrc, 512, 18, 89)  # (offsets change every 512 bytes)
    cfg = raw_cfg(D, L, 3)
    if front == "fir":
        taps, shift = random_fir_taps(300, 7)
        model = sdm.DcFirModel(steps, per, D, taps, shift, nsrc)
        g = fir_handle(cfg, nsrc, per, steps, taps, shift, source_ring=1)
    else:
        taps, shift = random_bank_taps(16, 300, 7)
        model = sdm.DcBankModel(16, taps, shift, D, nsrc, bins=[0, 7])
        g = bank_handle(cfg, nsrc, 16, [0, 7], taps, shift, source_ring=1)
    run_a = [(0, 2048), (2048, 512), (2560, 2048)]
    run_b = [(4608, 2048), (6656, 2048)]
    want = []
    for pieces in (run_a, run_b):
        if len({n for _, n in pieces}) == 1:  # (one run of whole buffers)
            parts = [raw_rows(*model.run(src[:, pieces[0][0]:pieces[-1][0] + pieces[-1][1]], L))]
        else:
            parts = [raw_rows(*model.run(src[:, at:at + n], n)) for at, n in pieces]
        want.append([np.concatenate([p[s] for p in parts]) for s in range(nsrc * per)])
    with g:
        push_run(g, src, run_a)
        g.full_demod()
        assert_rows(fetch_rows(g), want[0], f"{front}: the run with the short buffer")
        push_run(g, src, run_b)
        g.full_demod()
        assert_rows(fetch_rows(g, prev=True), want[0], f"{front}: the same through _prev")
        assert_rows(fetch_rows(g), want[1], f"{front}: the run behind it")
        assert_records(g, model, "after the runs")


def test_pack_results_2_on_top(oracle_lib):
    """-M fm with a squelch that everything passes, over the source ring with pack_results 2: the packed rows are the
    oracle's on the model's mixed samples, nothing held."""
    from oracle import pyoracle as po
    nsrc, per, L, runs = 2, 2, 2048, (1, 3)
    cfg = make_cfg(dict(case("c1_boxcar10_fast")[0], squelch_level=1), L, 3)
    steps = make_steps(nsrc * per, 43)
    src = bounded_src(nsrc, L, sum(runs), 97)
    model = sdm.DcBoxModel(steps, per, cfg.downsample, nsrc)
    with chan_handle(cfg, nsrc, per, steps, source_ring=1, pack_results=2) as g:
        states, b0 = None, 0
        for nb in runs:
            out, n, states = po.run_batch(cm.copy_cfg(cfg, offset_tuning=1), model.mixed_bytes(src[:, b0 * L:(b0 + nb) * L], L), states,
                                          nthreads=4)
            rows = [out[s, :n[s]].copy() for s in range(nsrc * per)]
            push_run(g, src, [((b0 + j) * L, L) for j in range(nb)])
            g.full_demod()
            packed, idx = g.fetch_packed()
            want, want_idx = pm.pack(rows, None)
            assert np.array_equal(idx, want_idx), (b0, idx, want_idx)
            assert np.array_equal(packed, want), b0
            b0 += nb
        assert_records(g, model, "after the runs")


# ------------------------------------------------------------------ the refusals ----

def test_refusals_change_nothing():
    nsrc, per, L, D = 1, 2, 2048, 7
    steps = make_steps(nsrc * per, 47)
    src = full_scale_src(nsrc, L, 6, 101)
    taps, shift = random_fir_taps(100, 9)

    def fails(g, value, code):
        before = g.get_option("source_dc")
        assert g.lib.rtlfm_gpu_set_option(g._h, b"source_dc", value) == code, (value, code)
        assert g.get_option("source_dc") == before

    model = sdm.DcFirModel(steps, per, D, taps, shift, nsrc)
    at = [0]

    def run_equals_the_model(g, d, what):
        got, _ = run_once(g, d, L, at[0], 1)
        assert_rows(got, raw_rows(*model.run(src[:, at[0] * L:(at[0] + 1) * L], L)), what)
        at[0] += 1

    with fir_handle(raw_cfg(D, L, 3), nsrc, per, steps, taps, shift, source_ring=1) as g:
        d = to_device(src)
        run_equals_the_model(g, d, "the first run")
        # -EINVAL: a value other than 0 / 1
        for v in (-1, 2):
            fails(g, v, -errno.EINVAL)
        run_equals_the_model(g, d, "behind -EINVAL")
        # -EBUSY: buffers queued over the source ring, a slot open, a run begun
        g.rtlsdr_callback(src[0, :L], stream=0)
        for v in (0, 1):
            fails(g, v, -errno.EBUSY)
        p, cap = C.c_void_p(), C.c_uint32()
        assert g.lib.rtlfm_gpu_acquire(g._h, 0, C.byref(p), C.byref(cap)) == 0
        fails(g, 0, -errno.EBUSY)
        C.memmove(p.value, np.ascontiguousarray(src[0, L:2 * L]).ctypes.data, L)
        assert g.lib.rtlfm_gpu_commit(g._h, 0, L) == 0
        assert g.run_begin() == 2
        fails(g, 0, -errno.EBUSY)
        g.run_end()
        assert_rows(fetch_rows(g), raw_rows(*model.run(src[:, :2 * L], L)), "the ring's run behind -EBUSY")
        run_equals_the_model(g, d, "behind -EBUSY")
        # -ERANGE: taps the wider check refuses, through the setter while the option is 1 ...
        wide = np.full(1024, 8000, dtype=np.int16)  # 362 x 8 192 000 > 2^31 > 182 x 8 192 000
        assert g.lib.rtlfm_channel_filter_check(wide.ctypes.data, 1024, 0) == 0
        assert g.lib.rtlfm_gpu_set_channel_filter(g._h, wide.ctypes.data, 1024, 0) == -errno.ERANGE
        run_equals_the_model(g, d, "behind the setter's -ERANGE")
    # ... and setting 1 while such a filter is set; the bank alike
    with fir_handle(raw_cfg(D, L, 1), nsrc, per, steps, wide, 0, dc=0) as g:
        fails(g, 1, -errno.ERANGE)
        plain = fm.FirModel(steps, per, D, wide, 0, nsrc)
        got, _ = run_once(g, to_device(src), L, 0, 1)
        assert_rows(got, raw_rows(*plain.run(src[:, :L])), "behind -ERANGE: the option stays off")
    K = 4
    btaps = np.zeros(4096, dtype=np.int16)
    btaps[1::K][:300] = 32767  # one branch: 256 x 9 830 100 > 2^31 > 128 x 9 830 100
    with bank_handle(raw_cfg(D, L, 1), nsrc, K, None, btaps, 0, dc=0) as g:
        fails(g, 1, -errno.ERANGE)
        plain = bm.BankModel(K, btaps, 0, D, nsrc)
        got, _ = run_once(g, to_device(src), L, 0, 1)
        assert_rows(got, raw_rows(*plain.run(src[:, :L])), "behind the bank's -ERANGE: the option stays off")
        g.set_channel_bank(K, btaps[:64], 0)
        g.set_option("source_dc", 1)
        assert g.lib.rtlfm_gpu_set_channel_bank(g._h, K, None, btaps.ctypes.data, 4096, 0) == -errno.ERANGE
        assert g.get_channel_bank()[0] == K
    # -ENOTSUP on a handle with cfg.dc_block_raw; -EINVAL for a constant outside 0 .. 65535 when setting 1 (0 goes)
    with demod(raw_cfg(D, L, 1, dc_block_raw=1), 2) as g:
        fails(g, 1, -errno.ENOTSUP)
        fails(g, 0, -errno.ENOTSUP)
    for k in (-1, 65536):
        with demod(raw_cfg(D, L, 1, rdc_block_const=k), 2) as g:
            fails(g, 1, -errno.EINVAL)
            g.set_option("source_dc", 0)
    # it may be set with channels off, and acts on nothing there
    with demod(raw_cfg(D, L, 1, rdc_block_const=65535), 2, source_dc=1) as g, demod(raw_cfg(D, L, 1, rdc_block_const=65535), 2) as twin:
        rows = np.repeat(src, 2, axis=0)
        a, _ = run_once(g, to_device(rows), L, 0, 1)
        b, _ = run_once(twin, to_device(rows), L, 0, 1)
        assert_rows(a, b, "channels off")
        assert bytes(g.state_get_all()) == bytes(twin.state_get_all())


# -------------------------------------------------------------------- off is off ----

@pytest.mark.parametrize("front", ["boxcar", "fir", "bank"])
@pytest.mark.parametrize("path", [0, 1])
def test_off_is_off(front, path):
    """A handle with the option at 0 - never set, or set and put back - equals the existing models, with the same count of timed
    front-end launches as a handle that never heard of it; with the option on, the pre-pass rides inside the same pair."""
    from rtlsdr_amd.demod import GpuDemod
    nsrc, per, L, D, runs = 2, 2, 2048, 7, (1, 2)
    steps = make_steps(nsrc * per, 53)
    src = full_scale_src(nsrc, L, sum(runs), 103)
    cfg = raw_cfg(D, L, 2)
    taps, shift = random_fir_taps(100, 11)
    btaps, bshift = random_bank_taps(16, 100, 11)
    want, state, b0 = [], None, 0
    plain = fm.FirModel(steps, per, D, taps, shift, nsrc) if front == "fir" else bm.BankModel(16, btaps, bshift, D, nsrc, bins=[1, 4])
    for nb in runs:
        piece = src[:, b0 * L:(b0 + nb) * L]
        if front == "boxcar":
            rows, state = cm.model_raw_boxcar(piece, steps, D, state, per_source=per, pos=b0 * L // 2)
        else:
            rows = raw_rows(*plain.run(piece))
        want.append(rows)
        b0 += nb
    counts = {}
    for kind in ("never", "back", "on"):
        g = GpuDemod(cfg, nsrc * per, 0, source_dc=None if kind == "never" else True)
        with g:
            g.set_path(path)
            g.set_channels(per, steps=steps if front != "bank" else steps_for(nsrc * per))
            if front == "fir":
                g.set_channel_filter(taps, shift)
            if front == "bank":
                g.set_channel_bank(16, btaps, bshift, bins=[1, 4])
            if kind == "back":
                g.set_option("source_dc", 0)
            g.timing_enable(True)
            g.timing_read()
            d, b0, seen = to_device(src), 0, []
            for r, nb in enumerate(runs):
                got, _ = run_once(g, d, L, b0, nb)
                seen.append(g.timing_read()[1])
                if kind != "on":
                    assert_rows(got, want[r], f"{front} {kind} run {r} path {path}")
                b0 += nb
            counts[kind] = seen
    assert counts["never"] == counts["back"] == counts["on"], counts
