"""The scanner's device side on the GPU: the squelch gate (k_scan_gate) and the hop mute (k_scan_mute) through
push / run / fetch against the model of tests/scan_model.py - the reference's rule around the oracle - EXACTLY: integer
modes and -A fast, no tolerance.  PCM, per-stream counts, gate records and the carried squelch_hits, over consecutive runs
so that carried hits and carried mutes cross runs; the same under verify_twice; and nothing changes while the option is off."""
import numpy as np
import pytest

import monitor_model as mm
import scan_model as sm
from rtlsdr_amd import capi
from rtlsdr_amd.capi import ATAN_FAST, MODE_AM, MODE_FM, MODE_RAW, RESAMPLE_LOW_PASS_REAL, RtlfmCfg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

L, S, RUNS, LEVEL = 2048, 5, 3, 60
# The squelch level sits between the two kinds of buffer: +-1 noise has an rms() of about 1 behind every decimator used
# here (fifth_order has unit noise gain per pass, a boxcar of D about sqrt(D) <= 4; the one output a boxcar that does not divide
# the buffer carries over from a tone adds up to 35 behind /7), a tone of amplitude 100 one of 70 (-M raw /1) and more.

CONFIGS = {
    "box7_fm": dict(mode=MODE_FM, downsample=7, custom_atan=ATAN_FAST),                          # does not divide the buffer
    "fifth4_fm": dict(mode=MODE_FM, downsample=16, downsample_passes=4, custom_atan=ATAN_FAST),
    "box10_am_dc": dict(mode=MODE_AM, downsample=10, output_scale=25, dc_block_audio=1),
    "fifth2_deemph": dict(mode=MODE_FM, downsample=4, downsample_passes=2, custom_atan=ATAN_FAST, deemph=1, deemph_a=9, rate_out=256000),
    "raw1": dict(mode=MODE_RAW, downsample=1),
}


def demod(cfg, ns=S, **options):
    from rtlsdr_amd.demod import GpuDemod
    return GpuDemod(cfg, ns, 0, options=options)


def pattern(nb, conseq, seed):
    """loud[s][k] for the RUNS * nb buffers of every stream: stream 0 never closes, stream 1 never opens, streams 2 and 3
    to 4
    open for one buffer and stay closed long enough to be held (conseq + 3 buffers), one buffer apart each, with a few
    seeded flips."""
    n = RUNS * nb
    rng = np.random.default_rng(seed)
    loud = np.zeros((S, n), dtype=bool)
    loud[0] = True
    period = conseq + 4  # (+ 1: behind fifth_order passes a tone's filter tail keeps the next short buffer open)
    loud[2] = (np.arange(n) % period) == 0
    loud[3] = ((np.arange(n) + 1) % period) == 0
    loud[4] = ((np.arange(n) + 2) % period) == 0
    flip = rng.random(n) < 0.2  # ... and a little disorder in the three
    loud[2:] ^= flip
    return loud


def make_input(loud, seed):
    rng = np.random.default_rng(seed + 1)
    return [[sm.tone_or_noise(rng, L, bool(loud[s][k])) for k in range(loud.shape[1])] for s in range(loud.shape[0])]


def model_runs(po, cfg, conseq, bufs, nb, mutes=None):
    """Per run: (pcm per stream, records [S, nb], hits per stream).  mutes[(run, stream)] = bytes, set before that run."""
    models = [sm.StreamModel(po, cfg, conseq) for _ in range(len(bufs))]
    out = []
    for r in range(len(bufs[0]) // nb):
        for (rr, s), m in (mutes or {}).items():
            if rr == r:
                models[s].mute = m
        res = [models[s].run(bufs[s][r * nb:(r + 1) * nb]) for s in range(len(bufs))]
        out.append(([x[0] for x in res], np.stack([x[1] for x in res]), [int(m.state.squelch_hits) for m in models]))
    return out


def assert_coverage(runs, nb, conseq):
    """The coverage the pattern owes a case, on the model's records alone."""
    recs = np.concatenate([r[1] for r in runs], axis=1)
    held, opened = recs["emit"] == 0, recs["hits_after"] == 0
    quiet_emitted = (recs["emit"] == 1) & (recs["hits_after"] > 0)
    assert held.any() and opened.any()
    # a closed squelch that still emits needs 0 < hits <= conseq: with conseq == 0 the rule leaves no such buffer
    assert quiet_emitted.any() == (conseq > 0)
    assert (~held).all(axis=1).any(), "a stream with nothing held"
    assert any((r[1]["emit"] == 0).all(axis=1).any() for r in runs), "a stream with a whole run held (count 0)"
    per_run = np.stack([r[1]["emit"] == 0 for r in runs])  # [run, stream, buffer]
    # ... first, middle and last in a run, in runs that also emit (with one buffer per run the three are one)
    mixed = per_run.any(axis=2) & ~per_run.all(axis=2) if nb > 1 else per_run.any(axis=2)
    assert (per_run[:, :, 0] & mixed).any() and (per_run[:, :, -1] & mixed).any(), "held first / last in a run"
    if nb >= 3:
        assert (per_run[:, :, 1:-1].any(axis=2) & mixed).any(), "held in the middle of a run"


def find_case(po, cfg, nb, conseq):
    """The first seed whose pattern gives the case its coverage - judged on the model on the CPU, never on the device."""
    for seed in range(64):
        bufs = make_input(pattern(nb, conseq, seed), seed)
        want = model_runs(po, cfg, conseq, bufs, nb)
        try:
            assert_coverage(want, nb, conseq)
        except AssertionError:
            continue
        return bufs, want
    raise AssertionError("no seed covers the case")


def run_case(po, g, cfg, conseq, bufs, nb, want, check_state=True):
    for r, (pcm, recs, hits) in enumerate(want):
        for s in range(len(bufs)):
            for buf in bufs[s][r * nb:(r + 1) * nb]:
                g.push(buf, s)
        g.run()
        out, lens = g.fetch_all()
        got_recs = g.gate()
        assert got_recs.shape == recs.shape
        assert np.array_equal(got_recs, recs), (r, got_recs, recs)
        assert [int(n) for n in lens] == [p.size for p in pcm], r
        for s in range(len(bufs)):
            assert np.array_equal(out[s, :lens[s]], pcm[s]), (r, s)
            assert np.array_equal(g.gate(s), recs[s])
            if check_state:
                assert g.state_get(s).squelch_hits == hits[s], (r, s)
        assert np.array_equal(g.fetch(2), pcm[2])


@pytest.mark.parametrize("verify", [0, 1])
@pytest.mark.parametrize("nb", [1, 3, 6])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_gate_equals_model(oracle_lib, name, nb, verify):
    for conseq in (0, 1, 2):
        cfg = RtlfmCfg.default(block_len=L, max_blocks=nb, squelch_level=LEVEL, **CONFIGS[name])
        bufs, want = find_case(oracle_lib, cfg, nb, conseq)
        with demod(cfg, squelch_gate=0, conseq_squelch=conseq) as g:
            g.set_option("squelch_gate", 1)
            if verify:
                g.set_option("verify_twice", 1)
            run_case(oracle_lib, g, cfg, conseq, bufs, nb, want)
            if verify:
                assert g.get_option("verify_runs") == RUNS and g.get_option("verify_mismatches") == 0


@pytest.mark.parametrize("conseq", [0, 1, 2])
def test_gate_ragged_run(oracle_lib, conseq):
    """One ragged run: the last buffer of the second run is 512 bytes for streams 1 and 3 (and whole for the others)."""
    nb = 3
    cfg = RtlfmCfg.default(block_len=L, max_blocks=nb, squelch_level=LEVEL, **CONFIGS["box7_fm"])
    loud = pattern(nb, conseq, 77 + conseq)
    loud[1, 2 * nb - 1] = True  # the short buffer of the stream that never opens otherwise: 512 bytes of tone
    bufs = make_input(loud, 77 + conseq)
    for s in (1, 3):
        bufs[s][2 * nb - 1] = bufs[s][2 * nb - 1][:512]
    want = model_runs(oracle_lib, cfg, conseq, bufs, nb)
    assert (want[1][1]["emit"][1] == [0, 0, 1]).all()  # the short buffer opens stream 1 and is emitted alone
    assert want[1][0][1].size == 256 // 7 or want[1][0][1].size == 256 // 7 + 1
    with demod(cfg, squelch_gate=1, conseq_squelch=conseq) as g:
        run_case(oracle_lib, g, cfg, conseq, bufs, nb, want)


def test_gate_off_changes_nothing_and_launch_counts(oracle_lib):
    """squelch_gate = 0: output, state and the launch count of a handle that never heard of the option; on: one launch more
    per run, and one more in a run with a mute pending."""
    nb, conseq = 3, 1
    cfg = RtlfmCfg.default(block_len=L, max_blocks=nb, squelch_level=LEVEL, **CONFIGS["box7_fm"])
    bufs = make_input(pattern(nb, conseq, 5), 5)
    res = {}
    for kind in ("never", "off", "on"):
        with demod(cfg) as g:
            if kind == "off":
                g.set_option("conseq_squelch", conseq)
                g.set_option("squelch_gate", 0)
            if kind == "on":
                g.set_option("conseq_squelch", conseq)
                g.set_option("squelch_gate", 1)
            g.timing_enable(True)
            g.timing_read()
            rows = []
            for r in range(RUNS):
                if r == 2:
                    g.mute(1, 100)
                for s in range(S):
                    for buf in bufs[s][r * nb:(r + 1) * nb]:
                        g.push(buf, s)
                g.run()
                out, lens = g.fetch_all()
                _, launches = g.timing_read()
                rows.append(([out[s, :lens[s]].copy() for s in range(S)], [g.state_get(s).as_dict() for s in range(S)], launches))
            res[kind] = rows
            if kind != "on":
                with pytest.raises(capi.RtlfmError) as e:
                    g.gate()
                assert e.value.code == -61  # -ENODATA
    for r in range(RUNS):
        a, b, c = res["never"][r], res["off"][r], res["on"][r]
        assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0], strict=True)) and a[1] == b[1] and a[2] == b[2]
        assert c[2] == a[2] + 1
    assert res["never"][2][2] == res["never"][1][2] + 1  # the run with the mute pending
    assert res["on"][2][2] == res["on"][1][2] + 1


def test_option_errors(oracle_lib):
    cfg = RtlfmCfg.default(block_len=L, max_blocks=2, **CONFIGS["box7_fm"])  # no squelch level
    with demod(cfg) as g:
        for name, v in (("squelch_gate", 2), ("squelch_gate", -1), ("conseq_squelch", -1), ("squelch_gate", 1)):
            with pytest.raises(capi.RtlfmError) as e:
                g.set_option(name, v)
            assert e.value.code == -22
        assert g.get_option("squelch_gate") == 0 and g.get_option("conseq_squelch") == 10
    # a resampler behind the demodulator: the gate is not built for it, and the handle stays usable
    cfg = RtlfmCfg.default(block_len=L, max_blocks=2, squelch_level=LEVEL, mode=MODE_FM, downsample=6, custom_atan=ATAN_FAST,
                           rate_out=170000, rate_out2=32000, resampler=RESAMPLE_LOW_PASS_REAL)
    rng = np.random.default_rng(3)
    bufs = [sm.tone_or_noise(rng, L, True) for _ in range(2)]
    with demod(cfg, 1) as g:
        with pytest.raises(capi.RtlfmError) as e:
            g.set_option("squelch_gate", 1)
        assert e.value.code == -95 and "squelch_gate" in str(e.value)  # -ENOTSUP
        assert g.get_option("squelch_gate") == 0
        for b in bufs:
            g.push(b, 0)
        g.run()
        want, _ = oracle_lib.run_stream(cfg, np.concatenate(bufs))
        assert np.array_equal(g.fetch(0), want)


MUTES = [0, 1, 15, 16, 17, 2047, 2048, 2049, 3 * 2048 + 5]


def test_mute_equals_oracle_on_muted_input(oracle_lib):
    """Every count, on streams 0, 2 and 4 at once with different counts, two runs of two buffers each (the largest spills into
    the second run); with input_stats on the records are those of the muted bytes; the caller's buffers stay as they were."""
    nb = 2
    cfg = RtlfmCfg.default(block_len=L, max_blocks=nb, **CONFIGS["box7_fm"])
    rng = np.random.default_rng(11)
    with demod(cfg, input_stats=1) as g:
        models = [sm.StreamModel(oracle_lib, cfg, 1 << 30) for _ in range(S)]
        for i in range(len(MUTES)):
            bufs = [[sm.tone_or_noise(rng, L, True) for _ in range(2 * nb)] for _ in range(S)]
            keep = [[b.copy() for b in row] for row in bufs]
            for k, s in enumerate((0, 2, 4)):
                m = MUTES[(i + 3 * k) % len(MUTES)]
                g.mute(s, 5)  # replaced by the call below
                g.mute(s, m)
                models[s].mute = m
            for r in range(2):
                muted = [[sm.apply_mute(b, 0)[0] for b in row[r * nb:(r + 1) * nb]] for row in bufs]
                for s in range(S):
                    left = models[s].mute
                    for j in range(nb):
                        muted[s][j], left = sm.apply_mute(muted[s][j], left)
                want = [models[s].run(bufs[s][r * nb:(r + 1) * nb])[0] for s in range(S)]
                for s in range(S):
                    for b in bufs[s][r * nb:(r + 1) * nb]:
                        g.push(b, s)
                g.run()
                out, lens = g.fetch_all()
                for s in range(S):
                    assert np.array_equal(out[s, :lens[s]], want[s]), (i, r, s)
                assert np.array_equal(g.input_stats_all(), mm.records(np.stack([np.stack(row) for row in muted]))), (i, r)
            assert all(m.mute == 0 for m in models)
            assert all(np.array_equal(a, b) for ra, rb in zip(keep, bufs, strict=True) for a, b in zip(ra, rb, strict=True))


def test_mute_device_and_run_device_busy(oracle_lib):
    lib = capi.load()
    stride, rows, row_bytes = 2048 + 7, 6, 2040  # a stride that is no multiple of 16: every row starts at another alignment
    rng = np.random.default_rng(2)
    host = rng.integers(0, 256, rows * stride + 64, dtype=np.uint8)
    counts = np.array([0, 1, 17, 2039, 2040, 5000], dtype=np.uint32)
    for off in (0, 3):  # and a base that is not aligned either
        d = torch.from_numpy(host).cuda()
        assert lib.rtlfm_gpu_mute_device(0, d.data_ptr() + off, stride, rows, row_bytes, counts.ctypes.data, None) == 0
        want = host.copy()
        for s in range(rows):
            want[off + s * stride: off + s * stride + min(int(counts[s]), row_bytes)] = 127
        assert np.array_equal(d.cpu().numpy(), want), off
    assert lib.rtlfm_gpu_mute_device(0, None, stride, rows, row_bytes, counts.ctypes.data, None) == -22
    assert lib.rtlfm_gpu_mute_device(0, d.data_ptr(), 16, rows, row_bytes, counts.ctypes.data, None) == -22  # rows overlap
    # rtlfm_gpu_run_device never mutes: -EBUSY while a count is pending, and fine again once it is gone
    cfg = RtlfmCfg.default(block_len=L, max_blocks=1, **CONFIGS["box7_fm"])
    with demod(cfg, 2) as g:
        iq = torch.from_numpy(np.stack([sm.tone_or_noise(rng, L, True) for _ in range(2)])).cuda()
        g.mute(1, 16)
        with pytest.raises(capi.RtlfmError) as e:
            g.run_torch(iq)
        assert e.value.code == -16
        g.mute(1, 0)
        out, n = g.run_torch(iq)
        g.sync()
        want, _ = oracle_lib.run_stream(cfg, iq[1].cpu().numpy())
        assert np.array_equal(out[1, :int(n[1])].cpu().numpy(), want)
