"""The carried source history that the channel filter and the channel bank share (include/rtlfm_hip.h, "History"; csrc/
channel_kernel.h, kHist): run lengths around its size, the two front ends taking turns on one handle, the source count
changing under a filter that stays, and verify_twice.  -M raw on full-scale bytes, every bit equal to tests/
channel_fir_model.py and tests/channel_bank_model.py."""
import functools

import numpy as np
import pytest

import channel_bank_model as bm
import channel_fir_model as fm
from channel_common import (assert_rows, bank_handle, demod, full_scale, make_steps, model_runs, random_bank_taps, random_fir_taps,
                            raw_cfg, raw_rows, run_gpu, run_once, to_device)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PATHS = pytest.mark.parametrize("path", [0, 1])


def seen_on(path, n):
    return [2 if path == 0 else 1] * n


# ------------------------------------------------- 1. runs as long as the history, and shorter ----

@functools.lru_cache(maxsize=None)
def long_filter_case(L, nruns):
    """2 sources x 3 channels, 1024 taps, D = 4, single-buffer runs of L bytes: (src, steps, taps, shift, the model's rows)."""
    nsrc, per, D = 2, 3, 4
    src = full_scale(nsrc, nruns * L, 1000 + L)
    steps = make_steps(nsrc * per, 11)
    taps, shift = random_fir_taps(1024, 12)
    want, _ = model_runs(fm.FirModel(steps, per, D, taps, shift, nsrc), src, L, (1,) * nruns)
    return src, steps, taps, shift, want


@pytest.mark.parametrize("L", [4096, 8192])
@PATHS
def test_runs_between_the_longest_halo_and_the_history(L, path):
    """Runs of 2048 samples - more than the filter's longest halo, less than the history, whose new copy is then part old
    history, part run - and of 4096, the history's own length, where it is the run."""
    nsrc, per, D, nruns = 2, 3, 4, 7
    src, steps, taps, shift, want = long_filter_case(L, nruns)
    with demod(raw_cfg(D, L, 1), nsrc * per) as g:
        g.set_path(path)
        g.set_channels(per, steps=steps)
        g.set_channel_filter(taps, shift)
        got, seen = run_gpu(g, src, L, (1,) * nruns)
    assert seen == seen_on(path, nruns)
    assert_rows(got, want, f"L {L} path {path}")


# --------------------------------------------------- 2. filter, bank, filter on one handle ----

@PATHS
def test_filter_then_bank_then_filter_on_one_handle(path):
    """Two runs behind a 40-tap filter, two behind a bank of K = 4 with 16 taps, two behind the filter again once the bank
    is removed: each phase equals its model started from silence at the handle's position - neither front end sees what
    the other left in the history."""
    nsrc, per, L, D, K = 2, 4, 512, 4, 4
    S = nsrc * per
    src = full_scale(nsrc, 6 * L, 21)
    steps = make_steps(S, 22)
    ftaps, fshift = random_fir_taps(40, 23)
    btaps, bshift = random_bank_taps(K, 16, 24)
    with demod(raw_cfg(D, L, 1), S) as g:
        g.set_path(path)
        g.set_channels(per, steps=steps)
        g.set_channel_filter(ftaps, fshift)
        d = to_device(src)
        for phase, b0 in (("filter", 0), ("bank", 2), ("filter again", 4)):
            if phase == "bank":
                g.set_channel_bank(K, btaps, bshift)
                model = bm.BankModel(K, btaps, bshift, D, nsrc)
            else:
                if phase == "filter again":
                    g.set_channel_bank(0)
                model = fm.FirModel(steps, per, D, ftaps, fshift, nsrc)
            assert g.channels_tell() == b0 * L // 2
            model.seek(g.channels_tell())
            for b in (b0, b0 + 1):
                got, p = run_once(g, d, L, b, 1)
                assert p == seen_on(path, 1)[0]
                assert_rows(got, raw_rows(*model.run(src[:, b * L:(b + 1) * L])), f"{phase} buffer {b} path {path}")
        ft, fs = g.channel_filter()
        assert np.array_equal(ft, ftaps) and fs == fshift


# ------------------------------------------- 3. set_channel_filter while the bank is on ----

@PATHS
def test_set_channel_filter_clears_the_history_under_the_bank(path):
    """A run of the bank, set_channel_filter, a run: the filter rests while the bank is on, but the call clears the history
    the two share - the second run equals the bank's model started from silence, and differs from the one that kept it."""
    nsrc, K, L, D = 2, 16, 512, 8
    taps, shift = random_bank_taps(K, 300, 31)
    ftaps, fshift = random_fir_taps(83, 32)
    src = full_scale(nsrc, 2 * L, 33)
    cleared, kept = (bm.BankModel(K, taps, shift, D, nsrc) for _ in range(2))
    for m in (cleared, kept):
        m.run(src[:, :L])
    cleared.clear()
    want = raw_rows(*cleared.run(src[:, L:]))
    unwanted = raw_rows(*kept.run(src[:, L:]))
    assert not any(np.array_equal(a, b) for a, b in zip(want, unwanted, strict=True))
    with bank_handle(raw_cfg(D, L, 1), nsrc, K, None, taps, shift, path) as g:
        d = to_device(src)
        run_once(g, d, L, 0, 1)
        g.set_channel_filter(ftaps, fshift)
        assert g.get_channel_bank()[0] == K and g.channels_tell() == L // 2
        got, p = run_once(g, d, L, 1, 1)
    assert p == seen_on(path, 1)[0]
    assert_rows(got, want, f"path {path}")


# ----------------------------- 4. a filter set with channels off, and the source count changing ----

def test_filter_set_with_channels_off_then_the_source_count_changes():
    """A handle of 6 streams: the filter is set while channels are off, then 6 sources x 1 channel, 2 sources x 3, and 6 x 1
    again, two runs each, the filter staying: set_channels starts every phase from pos 0 and silence, whatever the number
    of sources before it was.  The paths alternate between the runs."""
    S, L, D = 6, 512, 4
    paths = (0, 1, 1, 0, 0, 1)
    taps, shift = random_fir_taps(83, 41)
    src = full_scale(S, 2 * L, 42)
    with demod(raw_cfg(D, L, 1), S) as g:
        g.set_channel_filter(taps, shift)
        for phase, per in enumerate((1, 3, 1)):
            nsrc = S // per
            steps = make_steps(S, 43 + phase)
            g.set_channels(per, steps=steps)
            assert g.channels_tell() == 0
            want, _ = model_runs(fm.FirModel(steps, per, D, taps, shift, nsrc), src[:nsrc], L, (1, 1))
            got, seen = run_gpu(g, src[:nsrc], L, (1, 1), paths=paths[2 * phase:2 * phase + 2])
            assert seen == [2 if p == 0 else 1 for p in paths[2 * phase:2 * phase + 2]]
            assert_rows(got, want, f"phase {phase}: {nsrc} sources x {per}")


# ---------------------------------------------------------------- 5. verify_twice ----

@PATHS
def test_verify_twice_reads_one_history_in_both_executions(path):
    """Three runs of 2048 samples behind 1024 taps under verify_twice: both executions of a run read the same history (no
    mismatch), which moves on once per run (the model's bits)."""
    nsrc, per, D, L, nruns = 2, 3, 4, 4096, 3
    src, steps, taps, shift, want = long_filter_case(L, 7)
    with demod(raw_cfg(D, L, 1), nsrc * per, verify_twice=1) as g:
        g.set_path(path)
        g.set_channels(per, steps=steps)
        g.set_channel_filter(taps, shift)
        got, seen = run_gpu(g, src[:, :nruns * L], L, (1,) * nruns)
        assert g.channels_tell() == nruns * L // 2
        assert g.get_option("verify_runs") == nruns and g.get_option("verify_mismatches") == 0
    assert seen == seen_on(path, nruns)
    n = [w.size * nruns // 7 for w in want]  # (D divides a run: every run has the same number of outputs)
    assert_rows(got, [w[:k] for w, k in zip(want, n, strict=True)], f"path {path}")
