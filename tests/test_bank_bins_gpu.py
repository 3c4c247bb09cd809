"""Rebinding the channel bank's bins per source and in flight (include/rtlfm_hip.h, rtlfm_gpu_set_channel_bins), and the
loop run -> bank_survey -> SlotAllocator.step -> set_channel_bins, against tests/channel_bank_model.py and
tests/slots_model.py: equality of every bit.  The model is never cleared between runs: whatever the call touched besides
the bins would show in the next run."""
import errno

import numpy as np
import pytest

import channel_bank_model as bm
from bank_survey_common import assert_survey, model_run
from cases import make_cfg
from channel_common import BACK, assert_rows, bank_handle, bounded, demod, full_scale, raw_cfg, run_once, steps_for, to_device
from channel_common import random_bank_taps as random_taps
from channel_fir_model import raw_rows
from rtlsdr_amd import synth
from rtlsdr_amd.capi import ATAN_FAST, MODE_FM
from rtlsdr_amd.demod import channel_lowpass
from slots_model import SlotsModel

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def random_bins(rng, nsrc, per, K):
    return rng.integers(0, K, size=(nsrc, per)).astype(np.int32)


# ------------------------------------------------------------------------- 1. -M raw ----

@pytest.mark.parametrize("path", [0, 1])
def test_rows_follow_the_bins_of_every_run(path):
    """Different bins per source, changed before every run (not before the first: the shared list rules there): the rows of
    run r are the model's Y[bins_r[a][c]]; prev_index, pos and the next run prove that nothing else was touched."""
    nsrc, K, per, L, D = 3, 16, 3, 2048, 10
    runs = (1, 2, 1, 2)
    shared = [4, 4, 11]
    taps, shift = random_taps(K, 5 * K + 3, 301)
    src = full_scale(nsrc, sum(runs) * L, 302)
    rng = np.random.default_rng(303)
    model = bm.BankModel(K, taps, shift, D, nsrc, bins=shared)
    with bank_handle(raw_cfg(D, L, 2), nsrc, K, shared, taps, shift, path) as g:
        assert g.channel_bins().tolist() == [shared] * nsrc
        d, b0 = to_device(src), 0
        for r, nb in enumerate(runs):
            bins = None
            if r:
                bins = random_bins(rng, nsrc, per, K)
                bins[0] = bins[0][::-1] if r == 2 else bins[0]
                g.set_channel_bins(bins)
                assert np.array_equal(g.channel_bins(), bins)
                gk, gb, gt, gs = g.get_channel_bank()  # per_source bins: source 0's
                assert gk == K and gb.tolist() == bins[0].tolist() and np.array_equal(gt, taps) and gs == shift
            (I, Q), _, _ = model_run(model, src[:, b0 * L:(b0 + nb) * L], bins)
            rows, p = run_once(g, d, L, b0, nb)
            assert p == (2 if path == 0 else 1)
            assert_rows(rows, raw_rows(I, Q), f"path {path} run {r}")
            b0 += nb
            st = g.state_get_all()
            assert [st[s].prev_index for s in range(model.S)] == model.p0, r
            assert g.channels_tell() == b0 * L // 2
        # set_channel_bank afterwards: the shared list again (it clears the history, as ever)
        g.set_channel_bank(K, taps, shift, bins=shared)
        assert g.channel_bins().tolist() == [shared] * nsrc
        model.clear()
        (I, Q), _, _ = model_run(model, src[:, :L])
        rows, _ = run_once(g, d, L, 0, 1)
        assert_rows(rows, raw_rows(I, Q), f"path {path}, the shared list again")


# ------------------------------------------------------------------ 2. the back half ----

@pytest.mark.parametrize("name", ["fmfast", "fmfast_deemph"])
@pytest.mark.parametrize("path", [0, 1])
def test_the_back_half_keeps_its_state_across_a_rebinding(oracle_lib, name, path):
    """fm -A fast, and fm with deemph: the PCM equals the oracle fed the model's per-run selection as ONE stream per slot -
    the discriminator's previous sample and the deemph average are carried across the change of bin."""
    nsrc, K, per, L, D, runs = 2, 16, 2, 2048, 8, (1, 2, 1)
    ov = dict(BACK["fmfast"]) if name == "fmfast" else dict(mode=MODE_FM, custom_atan=ATAN_FAST, deemph=1, deemph_a=13)
    cfg = make_cfg(dict(ov, downsample=D), L, 2)
    taps, shift = channel_lowpass(128, 0.4 / K, 1)
    shift -= 4
    src = bounded(nsrc, sum(runs) * L, 311, 60)
    rng = np.random.default_rng(312)
    model = bm.BankModel(K, taps, shift, D, nsrc, bins=[1, 15])
    all_bins = [None] + [random_bins(rng, nsrc, per, K) for _ in runs[1:]]
    per_run, b0 = [], 0
    for nb, bins in zip(runs, all_bins, strict=True):
        per_run.append(model_run(model, src[:, b0 * L:(b0 + nb) * L], bins)[0])
        b0 += nb
    want, _ = bm.via_oracle(cfg, per_run, runs, L // 2)
    with bank_handle(cfg, nsrc, K, [1, 15], taps, shift, path) as g:
        d, b0, got = to_device(src), 0, [[] for _ in range(nsrc * per)]
        for nb, bins in zip(runs, all_bins, strict=True):
            if bins is not None:
                g.set_channel_bins(bins)
            rows, _ = run_once(g, d, L, b0, nb)
            for s in range(nsrc * per):
                got[s].append(rows[s])
            b0 += nb
    assert_rows([np.concatenate(x) for x in got], want, f"{name} path {path}")


# ------------------------------------------------------------- 3. the same bins again ----

def test_rebinding_to_the_same_bins_is_no_call_at_all():
    nsrc, K, L, D, runs = 2, 16, 2048, 8, (1, 2, 1)
    bins = [[0, 1, 15, 0], [3, 3, 8, 2]]
    taps, shift = channel_lowpass(128, 0.4 / K, 1)
    shift -= 4
    src = synth.fm_iq_u8(nsrc, sum(runs) * L // 2, fs=2.4e6, dev_hz=30e3, amplitude=55.0, seed=321)
    src[:, L:2 * L] = 127
    cfg = make_cfg(dict(BACK["fmfast_squelch"], downsample=D), L, 2)
    seen = []
    for again in (False, True):
        with bank_handle(cfg, nsrc, K, bins[0], taps, shift, 0) as g:
            g.set_channel_bins(bins)
            d, b0, out = to_device(src), 0, []
            for nb in runs:
                if again:
                    g.set_channel_bins(bins)
                rows, _ = run_once(g, d, L, b0, nb)
                out.append((rows, g.levels_all()[:, :nb].copy(), bytes(g.state_get_all()), g.channels_tell()))
                b0 += nb
            seen.append(out)
    for r, (a, b) in enumerate(zip(*seen, strict=True)):
        assert_rows(b[0], a[0], f"run {r}")
        assert np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3], r


# ------------------------------------------------------------------------ 4. the ring ----

def test_runs_already_queued_use_the_old_bins():
    """Over the source ring: run, set_channel_bins, run - nothing fetched or waited for in between.  The first run's rows are
    the old bins', the second's the new."""
    nsrc, K, per, L, D = 2, 16, 2, 16384, 10
    old, new = [[1, 2], [3, 4]], [[9, 2], [0, 15]]
    taps, shift = random_taps(K, 200, 331)
    src = full_scale(nsrc, 2 * L, 332)
    model = bm.BankModel(K, taps, shift, D, nsrc, bins=old[0])
    want = [model_run(model, src[:, :L], old)[0], model_run(model, src[:, L:], new)[0]]
    with bank_handle(raw_cfg(D, L, 1), nsrc, K, old[0], taps, shift, 0, source_ring=1) as g:
        g.set_channel_bins(old)
        for r in range(2):
            for a in range(nsrc):
                g.push(src[a, r * L:(r + 1) * L], a)
            g.run()
            if r == 0:
                g.set_channel_bins(new)
        out, lens = g.fetch_all_prev()
        assert_rows([out[s, :lens[s]] for s in range(g.nstreams)], raw_rows(*want[0]), "the queued run: the old bins")
        out, lens = g.fetch_all()
        assert_rows([out[s, :lens[s]] for s in range(g.nstreams)], raw_rows(*want[1]), "the run after the call: the new bins")


# -------------------------------------------------------------------- 5. the refusals ----

def test_every_refusal_changes_nothing():
    nsrc, K, per, L, D = 2, 16, 2, 2048, 10
    good = np.array([[5, 6], [7, 5]], dtype=np.int32)
    taps, shift = random_taps(K, 77, 341)
    bad = [np.array([[5, 6], [7, K]], dtype=np.int32), np.array([[-1, 6], [7, 5]], dtype=np.int32), None]
    src = full_scale(nsrc, (len(bad) + 2) * L, 342)
    model = bm.BankModel(K, taps, shift, D, nsrc, bins=[0, 1])
    with demod(raw_cfg(D, L, 1), nsrc * per, source_ring=1) as g:
        # without channels, and with channels but without a bank: -EINVAL
        assert g.lib.rtlfm_gpu_set_channel_bins(g._h, good.ctypes.data) == -errno.EINVAL
        g.set_channels(per, steps=steps_for(nsrc * per))
        assert g.lib.rtlfm_gpu_set_channel_bins(g._h, good.ctypes.data) == -errno.EINVAL
        out = np.zeros(nsrc * per, dtype=np.int32)
        assert g.lib.rtlfm_gpu_get_channel_bins(g._h, out.ctypes.data, out.size) == -errno.EINVAL
        g.set_channel_bank(K, taps, shift, bins=[0, 1])
        g.set_channel_bins(good)
        d = to_device(src)
        for b, bins in enumerate(bad):
            assert g.lib.rtlfm_gpu_set_channel_bins(g._h, None if bins is None else bins.ctypes.data) == -errno.EINVAL, b
            assert np.array_equal(g.channel_bins(), good)
            (I, Q), _, _ = model_run(model, src[:, b * L:(b + 1) * L], good)
            rows, _ = run_once(g, d, L, b, 1)
            assert_rows(rows, raw_rows(I, Q), f"after refusal {b}")
        assert g.lib.rtlfm_gpu_get_channel_bins(g._h, out.ctypes.data, out.size - 1) == -errno.ENOBUFS
        # -EBUSY while a run is begun and not ended (the source ring), then that run and the next still equal the model
        other = np.array([[1, 1], [2, 2]], dtype=np.int32)
        b = len(bad)
        for a in range(nsrc):
            g.push(src[a, b * L:(b + 1) * L], a)
        assert g.run_begin() == 1
        assert g.lib.rtlfm_gpu_set_channel_bins(g._h, other.ctypes.data) == -errno.EBUSY
        g.run_end()
        assert np.array_equal(g.channel_bins(), good)
        (I, Q), _, _ = model_run(model, src[:, b * L:(b + 1) * L], good)
        o, lens = g.fetch_all()
        assert_rows([o[s, :lens[s]] for s in range(g.nstreams)], raw_rows(I, Q), "the run the refused call fell into")
        (I, Q), _, _ = model_run(model, src[:, (b + 1) * L:], good)
        rows, _ = run_once(g, d, L, b + 1, 1)
        assert_rows(rows, raw_rows(I, Q), "after -EBUSY")
        # set_channels drops the per-source bins with the bank
        g.set_channels(per, steps=steps_for(nsrc * per))
        assert g.get_channel_bank()[0] == 0
        g.set_channel_bank(K, taps, shift, bins=[0, 1])
        assert g.channel_bins().tolist() == [[0, 1]] * nsrc


# ------------------------------------------------------------------------ 6. the loop ----

def test_the_loop_follows_the_carriers():
    """K = 16, 2 slots, 3 sources, 8 runs: carriers keyed on and off per run - one of them on a masked bin, one source with
    three at once for its two slots.  run -> bank_survey -> SlotAllocator.step -> set_channel_bins: the survey of every run
    equals the model's, the bins of every run equal those of slots_model.py fed the numpy survey, and the -M raw rows are the
    model's for those bins."""
    from rtlsdr_amd.slots import SlotAllocator
    nsrc, K, slots, L, D, nruns = 3, 16, 2, 4096, 8, 8
    park, mask = 8, [1] + [0] * 15
    # per source: {bin: the runs it is keyed in}
    plan = [{3: range(1, 4), 12: range(2, 7)},
            {0: range(0, 8), 5: range(3, 5)},            # bin 0 is masked: never bound
            {2: range(1, 6), 7: range(1, 3), 9: range(1, 8)}]
    amp = {2: 30.0, 7: 20.0, 9: 40.0}
    n = np.arange(nruns * L // 2, dtype=np.float64)
    src = np.empty((nsrc, nruns * L), dtype=np.uint8)
    rng = np.random.default_rng(351)
    for a in range(nsrc):
        sig = rng.normal(0, 1.0, n.size) + 1j * rng.normal(0, 1.0, n.size)
        for k, on in plan[a].items():
            gate = np.repeat(np.isin(np.arange(nruns), list(on)), L // 2)
            sig = sig + gate * amp.get(k, 35.0) * np.exp(2j * np.pi * k * n / K)
        src[a, 0::2] = np.rint(127 + sig.real).astype(np.uint8)
        src[a, 1::2] = np.rint(127 + sig.imag).astype(np.uint8)
    taps, shift = channel_lowpass(128, 0.4 / K, 1)
    shift -= 4
    # a carrier of amplitude A leaves A^2 per frame in its bin (DC gain 1); noise and leakage stay below 20
    kw = dict(open_level=200, close_level=100, hang=1, park=park, mask=mask)
    model = bm.BankModel(K, taps, shift, D, nsrc, bins=[park] * slots)
    rules = SlotsModel(nsrc, K, slots, **kw)
    history = []
    with bank_handle(raw_cfg(D, L, 1), nsrc, K, [park] * slots, taps, shift, 0, bank_survey=1) as g, \
            SlotAllocator(nsrc, K, slots, **kw) as alloc:
        d = to_device(src)
        bins = np.full((nsrc, slots), park, dtype=np.int32)
        for r in range(nruns):
            (I, Q), power, frames = model_run(model, src[:, r * L:(r + 1) * L], bins)
            rows, _ = run_once(g, d, L, r, 1)
            assert_rows(rows, raw_rows(I, Q), f"run {r}")
            got = g.bank_survey()
            assert_survey(got, power, frames, f"run {r}")
            alloc.step(*got)
            rules.step(power, frames)
            bins = alloc.bins()
            assert bins.tolist() == rules.bins() and alloc.events() == rules.events, r
            g.set_channel_bins(bins)
            history.append(bins.tolist())
    # what the rules had to do with this plan (from the plan alone: a run's survey binds for the NEXT run)
    assert history[0] == [[park, park]] * 3                        # run 0: only the masked carrier is on
    assert history[1] == [[3, park], [park, park], [9, 2]]         # three at once: the two loudest, the loudest first
    assert history[2][0] == [3, 12] and history[3][1] == [5, park]
    assert history[5][0] == [park, 12]                             # 3 went off after run 3: quiet in 4 and 5, freed by hang = 1
    assert all(0 not in row for h in history for row in h)         # the masked bin was never bound
    assert history[7] == [[park, 12], [park, park], [9, park]]     # 12 went off in run 7: one quiet run, still held
