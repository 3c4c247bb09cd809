"""Handles give back what they took (csrc/device_own.h): rtlfm_debug_live's three counters - device allocations,
pinned allocations, events - around every family of runs, on the smallest shapes each feature accepts.  After destroy
the counters are what they were before create; a ragged run's views and rtlpower_gpu_scan's view add nothing that
stays.  The runs' outputs are checked against what the neighbouring tests check them against, with their helpers.
(The counters, not hipMemGetInfo: the device is shared and its free memory moves under other people's work.)"""
import gc

import numpy as np
import pytest

import channel_bank_model as bm
import golden_util as gu
import health_model as hm
import monitor_model as mm
import test_scan_gpu as scan
from bank_survey_common import assert_survey, model_run
from cases import case, make_cfg
from channel_common import (assert_rows, demod, full_scale, make_steps_special, random_bank_taps, random_fir_taps, raw_cfg,
                            run_once, to_device)
from channel_fir_model import FirModel, raw_rows
from rtlsdr_amd import capi, synth
from rtlsdr_amd.capi import RtlfmCfg, RtlpowerCfg
from test_channel_ring_gpu import fetch_rows, push_run
from test_packed_gpu import assert_packed
from test_parity_gpu import _oracle_ragged, assert_parity
from test_power_report_gpu import _check_report, _plan

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def live():
    lib = capi.load()
    return tuple(int(lib.rtlfm_debug_live(k)) for k in range(3))


def baseline():
    gc.collect()  # (a handle an earlier test left to the collector goes now, not between two readings)
    return live()


def plus(c, dev=0, pinned=0, events=0):
    return (c[0] + dev, c[1] + pinned, c[2] + events)


# What run_ragged creates once, in front of its first view, where no batched run of the handle has needed them: the staged
# path's two work buffers and the audio tail's four (a front end that writes PCM itself, -M raw: no batched run takes either)
PATHS_NOT_TAKEN = 6


def test_kinds():
    assert capi.load().rtlfm_debug_live(3) == -22 and capi.load().rtlfm_debug_live(-1) == -22


# ---------------------------------------------------------------- 1. batched runs ----

def test_batched_ring_ragged_and_the_options(oracle_lib):
    """-M wbfm (deemph + low_pass_real: the one-pass tail's scratch), 3 streams, buffers of 16384, two a run: run_device on
    both paths, the ring, a ragged ring run, packed results, verify_twice, the clock probe - one stream of runs against the
    oracle buffer by buffer."""
    ov, sig = case("wbfm_preset")
    L, depth, ns = 16384, 2, 3
    cfg = make_cfg(ov, L, depth)
    nb = 10
    iq = synth.fm_iq_u8(ns, L // 2 * nb, seed=4242, **sig)
    lens = np.full((ns, nb), L, dtype=np.int64)
    lens[2, 6] = 8192  # the ragged run: two streams push 16384 bytes and one 8192
    blocks = [[iq[s, b * L:b * L + lens[s, b]] for b in range(nb)] for s in range(ns)]
    want, wst = _oracle_ragged(oracle_lib, cfg, blocks)
    per_block = [[_oracle_ragged(oracle_lib, cfg, [blocks[s][:b + 1]])[0][0].size for b in range(nb)] for s in range(ns)]
    base = baseline()
    got = [[] for _ in range(ns)]
    with demod(cfg, ns, input_stats=1) as g:
        assert live()[0] > base[0]

        def device(b0, n, path):
            g.set_path(path)
            rows, p = run_once(g, to_device(iq), L, b0, n)
            assert p == path or path == 2, (p, path)
            for s in range(ns):
                got[s].append(rows[s])

        def ring(b0, n):
            for b in range(b0, b0 + n):
                for s in range(ns):
                    g.rtlsdr_callback(blocks[s][b], s)
            g.full_demod()
            rows = fetch_rows(g)
            for s in range(ns):
                assert rows[s].size == per_block[s][b0 + n - 1] - (per_block[s][b0 - 1] if b0 else 0), (b0, s)
                got[s].append(rows[s])
            return rows

        device(0, 2, 1)
        g.timing_enable(True)
        device(2, 2, 2)
        g.timing_read()
        g.timing_enable(False)
        g.set_path(0)
        ring(4, 2)
        batched = live()
        ring(6, 1)
        assert live() == plus(batched, dev=2), "a ragged run: d_tmp and d_tmp_len once, and nothing for its views"
        stats = g.input_stats_all()  # stats_nblocks: the ragged run's one buffer, each stream's record over its own length
        assert stats.shape == (ns, 1) and all(stats[s, 0] == mm.records(blocks[s][6]) for s in range(ns))
        g.set_option("pack_results", 1)
        rows = ring(7, 1)
        assert_packed(g.fetch_packed(), rows, None, "packed")
        packed = live()
        assert packed[0] > batched[0] + 2
        g.set_option("pack_results", 0)
        assert live()[0] < packed[0]
        g.set_option("verify_twice", 1)
        ring(8, 1)
        assert g.get_option("verify_runs") == 1 and g.get_option("verify_mismatches") == 0
        g.set_option("verify_twice", 0)
        g.clock_probe(True)
        ring(9, 1)
        g.clock_probe(False)
        before = live()
        ring_again = [g.fetch(s) for s in range(ns)]  # (the pinned mirror of the per-stream fetch)
        assert live() == plus(before, pinned=2)
        sts = [g.state_get(s) for s in range(ns)]
        assert live()[0] > base[0]
    assert live() == base
    for s in range(ns):
        assert np.array_equal(ring_again[s], got[s][-1])
        assert_parity(np.concatenate(got[s]), want[s], cfg, f"stream {s}")
        assert gu.state_dict(sts[s], False) == gu.state_dict(wst[s], False), s


def test_a_ragged_run_with_the_clock_probe_on(oracle_lib):
    """k_fused (four fifth_order passes), every wave leaving its clock stamps: the stamp buffer a view needs - the most
    waves a one-buffer launch of any of its lengths can have - is there before the first view, which cannot grow it."""
    ov, sig = case("c2_p4_std")
    L, ns = 16384, 3
    cfg = make_cfg(ov, L, 2)
    iq = synth.fm_iq_u8(ns, L // 2 * 3, seed=77, **sig)
    blocks = [[iq[s, :L], iq[s, L:2 * L], iq[s, 2 * L:2 * L + (8192 if s == 1 else L)]] for s in range(ns)]
    want, _ = _oracle_ragged(oracle_lib, cfg, blocks)
    base = baseline()
    got = [[] for _ in range(ns)]
    with demod(cfg, ns, fused_tiles_per_seg=1) as g:  # (a wave per tile: as many waves as a launch can have)
        g.clock_probe(True)
        for run in ([0, 1], [2]):
            for b in run:
                for s in range(ns):
                    g.rtlsdr_callback(blocks[s][b], s)
            g.full_demod()
            rows = fetch_rows(g)
            assert g.last_path == 2 and g.clock_read() is not None
            for s in range(ns):
                got[s].append(rows[s])
        g.clock_probe(False)
    assert live() == base
    for s in range(ns):
        assert_parity(np.concatenate(got[s]), want[s], cfg, f"stream {s}")


def test_stats_health_and_gate_over_a_ragged_run(oracle_lib):
    """input_stats, input_health and squelch_gate on test_scan_gpu's boxcar configuration: a batched run, then a run whose
    last buffer is 512 bytes on streams 1 and 3 and a third with 1024 bytes on stream 2 - records, PCM and squelch_hits
    equal the models'.  The first ragged run creates what any path of a view may need, once (the work buffers of paths the
    batched run did not take among it): no pinned memory, no event, and the second ragged run nothing at all."""
    nb, conseq, L, S = 3, 1, scan.L, scan.S
    cfg = RtlfmCfg.default(block_len=L, max_blocks=nb, squelch_level=scan.LEVEL, **scan.CONFIGS["box7_fm"])
    loud = scan.pattern(nb, conseq, 78)
    loud[1, 2 * nb - 1] = True
    bufs = scan.make_input(loud, 78)
    for s in (1, 3):
        bufs[s][2 * nb - 1] = bufs[s][2 * nb - 1][:512]
    bufs[2][3 * nb - 1] = bufs[2][3 * nb - 1][:1024]
    want = scan.model_runs(oracle_lib, cfg, conseq, bufs, nb)
    base = baseline()
    with demod(cfg, S, squelch_gate=1, conseq_squelch=conseq, input_stats=1, input_health=1) as g:
        scan.run_case(oracle_lib, g, cfg, conseq, bufs, nb, want[:1])
        first = np.stack([np.stack(bufs[s][:nb]) for s in range(S)])
        assert np.array_equal(g.input_stats_all(), mm.records(first))
        assert np.array_equal(g.input_health_all(), hm.records(first))
        batched = live()
        scan.run_case(oracle_lib, g, cfg, conseq, [b[nb:] for b in bufs], nb, want[1:2], check_state=False)
        ragged = live()
        assert ragged == plus(batched, dev=2 + PATHS_NOT_TAKEN), "d_tmp, d_tmp_len and the buffers of the paths not taken so far"
        stats, health = g.input_stats_all(), g.input_health_all()
        assert stats.shape == (S, nb) and health.shape == (S, nb)
        for s in range(S):
            assert g.state_get(s).squelch_hits == want[1][2][s], s
            for b in range(nb):
                assert stats[s, b] == mm.records(bufs[s][nb + b]), (s, b)
        scan.run_case(oracle_lib, g, cfg, conseq, [b[2 * nb:] for b in bufs], nb, want[2:3])
        assert live() == ragged
    assert live() == base


# --------------------------------------------------------------------- 2. channels ----

def test_channels_filter_bank_bins_survey_and_the_source_ring(oracle_lib):
    """2 sources x 2 channels, -M raw /10 on full-scale bytes: the filter, the bank with K = 4, per-source bins, the survey
    on for two runs and off, the source ring with a ragged run (one view of the whole handle per buffer), and set_channels
    with another per_source, which rebuilds the ring's input side."""
    nsrc, per, D, L, cap, K = 2, 2, 10, 4096, 3, 4
    cfg = raw_cfg(D, L, cap)
    steps = make_steps_special(nsrc * per, 9)
    ftaps, fshift = random_fir_taps(33, 5)
    btaps, bshift = random_bank_taps(K, 24, 6)
    bins, bins_ps = [1, 3], [[1, 3], [2, 0]]
    src = full_scale(nsrc, 12 * L, 31)
    base = baseline()
    with demod(cfg, nsrc * per) as g:
        d = to_device(src)
        g.set_channels(per, steps=steps)
        g.set_channel_filter(ftaps, fshift)
        fir = FirModel(steps, per, D, ftaps, fshift, nsrc)
        rows, _ = run_once(g, d, L, 0, 2)
        assert_rows(rows, raw_rows(*fir.run(src[:, :2 * L])), "filter")
        g.reset()  # (pos and every stream's prev_index back to 0: the bank's model starts like a fresh handle)
        g.set_channel_bank(K, btaps, bshift, bins=bins)
        bank = bm.BankModel(K, btaps, bshift, D, nsrc, bins=bins)
        rows, _ = run_once(g, d, L, 2, 1)
        assert_rows(rows, raw_rows(*bank.run(src[:, 2 * L:3 * L])), "bank")
        g.set_channel_bins(np.array(bins_ps, dtype=np.int32).ravel())
        with_bins = live()
        g.set_option("bank_survey", 1)
        for r in range(2):
            (I, Q), power, frames = model_run(bank, src[:, (3 + r) * L:(4 + r) * L], bins_ps)
            rows, _ = run_once(g, d, L, 3 + r, 1)
            assert_survey(g.bank_survey(), power, frames, f"survey run {r}")
            assert_rows(rows, raw_rows(I, Q), f"per-source bins, run {r}")
        assert live()[0] > with_bins[0]
        g.set_option("bank_survey", 0)
        assert live() == with_bins, "the survey's sets, its partial sums and its events go with the option"
        # the source ring: a batched run, then one with a short last buffer on both sources
        g.set_option("source_ring", 1)
        at = 5 * L
        push_run(g, src, [(at, L), (at + L, L)])
        g.full_demod()
        (I, Q), _, _ = model_run(bank, src[:, at:at + 2 * L], bins_ps)
        assert_rows(fetch_rows(g), raw_rows(I, Q), "ring, full buffers")
        at += 2 * L
        batched = live()
        push_run(g, src, [(at, L), (at + L, 1536)])
        g.full_demod()
        (I, Q), _, _ = model_run(bank, src[:, at:at + L + 1536], bins_ps)
        assert_rows(fetch_rows(g), raw_rows(I, Q), "ring, a short last buffer")
        ragged = live()
        # (this handle's runs so far were the filter's and the bank's: the boxcar front end's emit buffer and dummy tile too)
        assert ragged == plus(batched, dev=2 + PATHS_NOT_TAKEN + 2), "d_tmp, d_tmp_len and the buffers of the paths not taken so far"
        assert g.channels_tell() == (at + L + 1536 - 2 * L) // 2
        at += L + 1536
        push_run(g, src, [(at, 512), (at + 512, L)])
        g.full_demod()
        (I, Q), _, _ = model_run(bank, src[:, at:at + 512 + L], bins_ps)
        assert_rows(fetch_rows(g), raw_rows(I, Q), "ring, a short first buffer")
        assert live() == ragged, "a second ragged run: nothing more"
        # another per_source: one source of four channels, the filter again (set_channels drops the bank)
        rebuilt = live()
        steps4 = make_steps_special(4, 10)
        g.set_channels(4, steps=steps4)
        assert g.sources == 1 and live() == rebuilt, "the input side is rebuilt, not added to"
        g.reset()
        fir4 = FirModel(steps4, 4, D, ftaps, fshift, 1)
        at = 11 * L
        push_run(g, src[:1], [(at, L)])
        g.full_demod()
        assert_rows(fetch_rows(g), raw_rows(*fir4.run(src[:1, at:at + L])), "one source of four")
    assert live() == base


# -------------------------------------------------------------------- 3. rtl_power ----

@pytest.mark.parametrize("kw", [dict(bin_e=10, window=1, buf_len=16384),
                                dict(bin_e=9, window=4, downsample=4, downsample_passes=2, boxcar=0, comp_fir_size=9, buf_len=16384)],
                         ids=["frames", "decimated"])
def test_power_scan_view_report_and_probe(oracle_lib, kw):
    """rtlpower_gpu_scan - a one-stream view of the handle whose work buffers (the decimated scan's) are its own and go
    with it - on two streams, then scan_device, the report and the clock probe."""
    from rtlsdr_amd.power import GpuPower
    cfg = RtlpowerCfg.default(**kw)
    L, ns = int(cfg.buf_len), 2
    iq = synth.fm_iq_u8(ns, L // 2 * 2, fs=2.048e6, seed=5)
    want, wn = oracle_lib.power_scan_batch(cfg, iq, nthreads=1)
    base = baseline()
    with GpuPower(cfg, ns, 0) as g:
        created = live()
        assert created[0] > base[0]
        g.scanner(iq[0, :L], 0)
        assert live() == plus(created, dev=1), "d_one on the first call; what the view allocated went with it"
        g.scanner(iq[1, :L], 1)
        assert live() == plus(created, dev=1)
        g.clock_probe(True)
        g.scan_torch(torch.from_numpy(np.ascontiguousarray(iq[:, L:])).cuda())
        g.clock_probe(False)
        g.sync()
        accs = [g.fetch(s) for s in range(ns)]
        for s in range(ns):
            assert accs[s][1] == wn[s] and np.array_equal(accs[s][0], want[s]), s
        scanned = live()
        _check_report(g, _plan(cfg, 2048000, 0.0), accs, True, "report")
        assert live() == plus(scanned, dev=2, pinned=1, events=1)
        assert g.fetch(0)[1] == 0
    assert live() == base
