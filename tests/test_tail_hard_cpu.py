"""The audio tail on full-scale audio and at the edges of the resampling ratios, without a GPU: the inputs of
tests/golden/tail_hard.json are what they were; on them the counting model (tests/tail_hard.py), the oracle and the
reference's own full_demod() agree in every sample and carried field; every stage has a recorded case whose stores wrap
there, every division form of deemph_filter one with |x - avg| > 49152, every ratio class one behind a front with uniform
counts and one behind a boxcar that does not divide the buffer; and the suite's other inputs wrap nowhere behind the
demodulator - the reason these exist."""
import numpy as np
import pytest

import golden_util as gu
import tail_hard as th
from rtlsdr_amd import capi, synth

RECORD = th.load()
NAMES = [c["name"] for c in th.CASES]


def _oracle(po, c):
    cfg, iq, st = th.build(po, c)
    return cfg, iq, po.run_batch(cfg, iq, states=th.copy_states(st) if st else None, nthreads=4)


def test_the_record_has_the_table():
    assert sorted(RECORD["cases"]) == sorted(NAMES) and len(set(NAMES)) == len(NAMES)
    assert RECORD["flag_cap"] == th.FLAG_CAP == 0.05
    for c in th.CASES:
        assert c["L"] in (8192, 16384) or (c["L"] == 262144 and c["nb"] == 1 and len(c["streams"]) == 1), c["name"]
        # (2 - 4 buffers; five for the one row whose front shows its long count with the fifth, see the table)
        assert (c["nb"] <= 4 or c["name"] == "arb_plus1_box68_am" and c["nb"] == 5) and (c["streams"] == th.FM_STREAMS or len(c["streams"]) <= 8), c["name"]
    assert sum(c["L"] == 262144 for c in th.CASES) == 2


@pytest.mark.parametrize("name", NAMES)
def test_bytes_match_the_record(oracle_lib, name):
    c, rec = th.case(name), RECORD["cases"][name]
    cfg, iq, _ = th.build(oracle_lib, c)
    assert [th.sha(row) for row in iq] == rec["stream_sha256"], name
    assert int(cfg.output_scale) == rec["output_scale"] and (rec["klass"], rec["uniform"]) == (c["klass"], c["uniform"])
    assert rec["stream_set"] == th.stream_set_name(c) and RECORD["stream_sets"] == th.STREAM_SETS


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_oracle(oracle_lib, name):
    """Every sample, every output length and every field the tail carries; the model's counts are the recorded ones, and
    the oracle's output and state the recorded digests."""
    c, rec = th.case(name), RECORD["cases"][name]
    cfg, iq, (want, want_len, wst) = _oracle(oracle_lib, c)
    res = th.model_case(oracle_lib, c, cfg, iq)
    for s, (out, mst, _, _, lens) in enumerate(res):
        assert sum(lens) == want_len[s], (name, s, lens, int(want_len[s]))
        bad = np.flatnonzero(out != want[s, :want_len[s]])
        assert bad.size == 0, (name, s, bad.size, bad[:8])
        got = wst[s].as_dict()
        assert {f: got[f] for f in th.TAIL_STATE} == mst, (name, s)
    t = th.totals(res)
    assert {k: int(t[k]) for k in rec["wraps"]} == rec["wraps"], name
    assert (int(t["max_d"]), int(t["peak"]), int(t["outputs"]), int(t["flagged"])) == (rec["max_d"], rec["peak"], rec["outputs"], rec["flagged"])
    assert [r[4] for r in res] == th.record_lens(rec), name
    assert th.sha(np.concatenate([want[s, :want_len[s]] for s in range(len(iq))])) == rec["out_sha256"], name
    assert th.sha(np.frombuffer(b"".join(bytes(wst[s]) for s in range(len(iq))), dtype=np.uint8)) == rec["state_sha256"], name


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_live_reference(oracle_lib, name):
    """The oracle against the reference's own rtlsdr_callback() + full_demod(), compiled in place: every stream of every
    row from a fresh state (the harness cannot inject one; deemph_filter's function-static avg is out of its reach, so a
    fresh copy of the reference per stream and no comparison of that field, as in test_oracle_golden.py)."""
    if not oracle_lib.have_reference():
        pytest.skip("oracle/_ref is not built: no live reference here")
    cfg, iq, _ = th.build(oracle_lib, th.case(name))
    for s, row in enumerate(iq):
        ref = oracle_lib.Reference()
        try:
            want, rst = ref.run_stream(cfg, row)
        finally:
            ref.close()
        got, st = oracle_lib.run_stream(cfg, row)
        assert got.shape == want.shape, (name, s, got.shape, want.shape)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (name, s, bad.size, bad[:8])
        assert gu.state_dict(st) == gu.state_dict(rst), (name, s)


# ---- conditions on the record: what the table promises to reach ----

def _cases(pred):
    return [n for n in NAMES if pred(th.case(n), RECORD["cases"][n])]


@pytest.mark.parametrize("stage", th.WRAPS)
def test_every_stage_has_a_case_that_wraps_there(stage):
    """low_pass_simple's sum, dc_block_audio_filter's result - mean, low_pass_real's (int16_t)(now_lpr / div) and its int32
    now_lpr, arbitrary_downsample's inner cast and its int16 accumulator."""
    assert _cases(lambda c, r: r["wraps"][stage] > 0), stage


def test_the_int32_accumulator_wraps_by_its_samples_alone():
    assert RECORD["cases"]["lpr_wrap32_am"]["wraps"]["lpr32"] > 0 and not th.case("lpr_wrap32_am")["inject"]


@pytest.mark.parametrize("form,pred", [("MAGIC 0", lambda a: a > 32768), ("MAGIC 1", lambda a: 2 < a <= 32768 and a & (a - 1)),
                                       ("MAGIC 2", lambda a: 2 < a <= 32768 and not a & (a - 1)), ("a == 2", lambda a: a == 2)])
def test_every_division_form_of_deemph_sees_numerators_beyond_49152(form, pred):
    """deemph_form() (rtlfm_hip.hip): a division beyond 32768, a multiply-high, a shift, and a == 2's mean of the two."""
    hit = _cases(lambda c, r: c["cfg"].get("deemph") and pred(c["cfg"]["deemph_a"]) and r["max_d"] > th.BIG_D)
    assert hit, form
    # ... and where the time-parallel forms apply, on runs long enough for them (deemph_scans: 2048 samples per stream)
    if form != "MAGIC 0":
        assert any(sum(th.record_lens(RECORD["cases"][n])[0]) >= 2048 or th.case(n)["cfg"].get("rate_out2") for n in hit), form


def test_no_store_of_deemph_wraps_from_a_state_inside_int16():
    """avg moves towards x and never past it: (int16_t)avg cannot wrap unless the state came in from outside."""
    for n, r in RECORD["cases"].items():
        inside = all(-32768 <= v <= 32767 for v in th.case(n)["inject"].get("deemph_avg", []))
        assert (r["wraps"]["deemph_store"] == 0) == inside, n


@pytest.mark.parametrize("klass", th.CLASSES_BOTH_FRONTS + ("mixed down and up",))
def test_every_ratio_class_has_a_case(klass):
    rows = _cases(lambda c, r: c["klass"] == klass)
    fronts = {th.case(n)["uniform"] for n in rows}
    assert fronts == ({True, False} if klass in th.CLASSES_BOTH_FRONTS else {False}), (klass, rows)
    for n in rows:
        cfg, lens = th.case(n)["cfg"], th.record_lens(RECORD["cases"][n])
        n1 = lambda s, b: _len1(th.case(n), s, b)  # noqa: E731
        pairs = {(n1(s, b), l2) for s, row in enumerate(lens) for b, l2 in enumerate(row)}
        ok = {"len2 == len1": lambda a, b: a == b, "len2 == len1 + 1": lambda a, b: b == a + 1, "len2 == len1 - 1": lambda a, b: b == a - 1,
              "len2 == 0": lambda a, b: b == 0, "len2 == 1": lambda a, b: b == 1, "len1 in (2, 3)": lambda a, b: a in (2, 3),
              "x 10": lambda a, b: 10 * a <= b < 10 * a + a // 50 + 2}.get(klass)
        if ok:
            assert all(ok(a, b) for a, b in pairs), (n, sorted(pairs))
        else:  # one run with buffers that are downsampled and buffers that are upsampled
            assert any(a >= b for a, b in pairs) and any(a < b for a, b in pairs), (n, sorted(pairs))
        assert cfg["resampler"] == capi.RESAMPLE_ARBITRARY
    if klass == "len2 == len1":  # rate_out2 == rate_out, and one above it where the floor still gives equality
        assert {th.case(n)["cfg"]["rate_out2"] - th.case(n)["cfg"]["rate_out"] for n in rows} == {0, 1}


_LEN1 = {}


def _len1(c, s, b):
    """Samples buffer b of stream s hands the resampler: the record's lengths give len2 only."""
    if c["name"] not in _LEN1:
        from oracle import pyoracle as po
        cfg, iq, _ = th.build(po, c)
        _LEN1[c["name"]] = [[len(x) // max(1, int(cfg.post_downsample)) for x in th.demodulated(po, cfg, row)] for row in iq]
    return _LEN1[c["name"]][s][b]


def test_low_pass_real_classes():
    cf = lambda n: th.case(n)["cfg"]  # noqa: E731
    lpr = _cases(lambda c, r: c["cfg"].get("rate_out2", 0) > 0 and c["cfg"]["resampler"] == capi.RESAMPLE_LOW_PASS_REAL)
    for what, pred in (("div == 1", lambda c: c["rate_out"] // c["rate_out2"] == 1 and c["rate_out"] != c["rate_out2"]),
                       ("equal rates", lambda c: c["rate_out"] == c["rate_out2"]), ("rate_out2 == 1", lambda c: c["rate_out2"] == 1)):
        assert {th.case(n)["uniform"] for n in lpr if pred(cf(n))} == {True, False}, what  # at both kinds of front
    # the injected phases also in front of the kernels that run low_pass_real behind deemph_filter
    assert any(cf(n).get("deemph") for n in _cases(lambda c, r: c["klass"] == "lpr phase outside"))
    for n in _cases(lambda c, r: c["klass"] == "lpr phase outside"):
        fast, inj = cf(n)["rate_out"], th.case(n)["inject"]
        assert {-5 * fast, -1, fast, 3 * fast + 7} <= set(inj["prev_lpr_index"])
        assert any(0 < th.I32[1] - v <= 10 for v in inj["now_lpr"]) and any(0 < v - th.I32[0] <= 10 for v in inj["now_lpr"])
    assert {th.case(n)["uniform"] for n in _cases(lambda c, r: c["klass"] == "lpr phase outside")} == {True, False}
    assert {40000, -40000} <= set(th.case("adc_usb")["inject"]["dc_avg"])


def test_the_wide_index_case_is_wide():
    """k_arb_upsample's 64-bit branch: (nlo + 1) len2 >= 2^31."""
    lens = th.record_lens(RECORD["cases"]["arb_up64_usb"])[0]
    assert (131072 + 1) * lens[0] >= 1 << 31 and lens[0] > 131072


def test_flagged_share_of_every_resampler_case_is_within_the_cap():
    for n, r in RECORD["cases"].items():
        assert r["flagged"] <= th.FLAG_CAP * r["outputs"], (n, r["flagged"], r["outputs"])
        assert r["flagged_share"] == round(r["flagged"] / r["outputs"], 6) if r["outputs"] else r["flagged_share"] == 0


def test_the_fm_controls_wrap_nowhere():
    ctl = _cases(lambda c, r: c["streams"] == th.FM_STREAMS)
    assert {th.case(n)["klass"] for n in ctl} >= {"post", "deemph", "adc", "lpr", "down"}
    for n in ctl:
        r = RECORD["cases"][n]
        assert not any(r["wraps"].values()) and r["max_d"] < th.BIG_D, n


# ---- the finding: the suite's other inputs wrap nowhere behind the demodulator ----

def _tail_inputs_wrap_nowhere(po, cfg, iq, what, streams=None):
    """Where the configuration has a tail stage: the audio mode_demod hands the tail stays within 16384 (FM: atan2 / pi *
    16384 cannot exceed it) or below it (the rest), and by the model no store of a tail stage wraps and deemph_filter divides
    nothing beyond 49152 - with the one exception the finding names: low_pass_simple's sum of two to four FM samples, which
    noise at the rails of the discriminator can carry past int16 by accident.  Returns (the input's peak, those accidents)."""
    fm = cfg.mode == capi.MODE_FM
    if not (cfg.post_downsample > 1 or cfg.deemph or cfg.dc_block_audio or cfg.rate_out2 > 0):
        return 0, 0  # no tail stage: nothing is fed one
    peak = accidents = 0
    for s in range(len(iq)) if streams is None else streams:
        blocks = th.demodulated(po, cfg, iq[s])
        peak = max([peak] + [int(np.abs(x).max()) for x in blocks if len(x)])
        info = th.model_tail(cfg, blocks)[2]
        if fm:
            accidents += info["post"]
            info["post"] = 0
        assert not any(info[k] for k in th.WRAPS + ("deemph_store",)), (what, s, dict(info))
        assert info["max_d"] < th.BIG_D, (what, s, info["max_d"])
    assert peak <= 16384 if fm else peak < 16384, (what, peak)
    return peak, accidents


def _gpu_test_module(name):
    """A GPU test module, for what it draws: importing it needs torch, and its absence is a failure here, not a skip."""
    try:
        return __import__(name)
    except pytest.skip.Exception as e:
        pytest.fail(f"{name} cannot be imported: {e}")


ACCIDENTS = {"vs_oracle": 3, "any_buffer_size": 0}  # FM noise whose sum of `step` samples left int16 in low_pass_simple: all there is


@pytest.mark.parametrize("sweep", ["vs_oracle", "any_buffer_size"])
def test_the_sweeps_inputs_wrap_nowhere_in_the_tail(oracle_lib, sweep):
    """test_random_configurations_vs_oracle's 48 seeds and test_random_configurations_any_buffer_size's 24, with their own
    inputs: no store of a tail stage wraps, FM stays within 16384 and the rest below it.  It fails, and is brought up to
    date, the day someone widens the sweeps."""
    tp = _gpu_test_module("test_parity_gpu")
    any_size = sweep == "any_buffer_size"
    assert (tp.SWEEP_SEEDS, tp.SWEEP_W_SEEDS) == (48, 24)  # (the pinned counts below are of these seeds)
    loud = accidents = 0
    for seed in range(tp.SWEEP_W_SEEDS if any_size else tp.SWEEP_SEEDS):
        ov, L, nb, ns, cfg, _ = tp.sweep_draw(seed, any_size)
        if capi.load().rtlfm_cfg_validate(cfg) < 0 or ov["mode"] == capi.MODE_RAW:
            continue
        iq = tp.sweep_input(ov, L, nb, ns, seed, any_size)
        try:
            oracle_lib.run_batch(cfg, iq[:1], nthreads=1)
        except RuntimeError:
            continue  # outside the reference's domain: the sweep skips it too
        peak, acc = _tail_inputs_wrap_nowhere(oracle_lib, cfg, iq, (sweep, seed))
        accidents += acc
        if cfg.mode != capi.MODE_FM:
            loud = max(loud, peak)
    print(f"{sweep}: the loudest AM / USB / LSB audio handed to a tail stage: {loud}; sums of FM samples that wrapped in low_pass_simple: {accidents}")
    assert 0 < loud < 16384
    assert accidents == ACCIDENTS[sweep]


def test_the_long_runs_inputs_wrap_nowhere_in_the_tail(oracle_lib):
    """test_tail_long_runs_gpu.py's default seeds (all FM): the audio they hand the tail, from a fresh state (the states
    that test injects from outside int16 are its own subject: the plain form of the filter)."""
    tl = _gpu_test_module("test_tail_long_runs_gpu")
    assert tl.NSEEDS == 10
    for seed in range(tl.NSEEDS):
        ov, L, nb, ns, cfg, iq, _ = tl.long_run_draw(seed)
        if capi.load().rtlfm_cfg_validate(cfg) < 0:
            continue
        assert cfg.mode == capi.MODE_FM
        peak, acc = _tail_inputs_wrap_nowhere(oracle_lib, cfg, iq, ("long runs", seed), streams=(0, ns - 1))  # (the model walks a sample at a time)
        assert acc == 0, seed
