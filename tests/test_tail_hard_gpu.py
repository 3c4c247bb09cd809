"""The audio tail on a real MI355X on full-scale audio and at the edges of the resampling ratios: every row of
tests/tail_hard.py's case table against the oracle - outputs, lengths and every carried field - through each form of the
tail its configuration has: the automatic plan (as it ships, and again with tail_sync = 1), deemph_sequential = 1,
deemph_four_pass = 1, lpr_separate = 1, rtlfm_gpu_set_path(1), one run split into two launches, and the one-pass kernels
with lpr_chunk = 256 / arb_waves = 1.  Which form ran is asserted: last_route / last_rest / last_path against the plan and
the front end the path names, and the tail's kernels by the lines tail_sync = 1 prints, against what deemph_route() and
run_tail() (rtlfm_hip.hip) lead to for the run's geometry.

The bar: integer-only chains bit-exact.  Behind an arbitrary resampler every output the model (tail_hard.py) does not flag
is bit-exact; a flagged one - its exact value is an integer, so one rounding of a double or a contracted multiply-add can
change the truncation - may instead be the other truncation pushed through the rest of the stage, and a case in which any
does differ is reported in the test's output.  A configuration the library refuses fails: the oracle runs all of them."""
import functools
import re
import time

import numpy as np
import pytest

import golden_util as gu
import tail_hard as th
from rtlsdr_amd import capi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NAMES = [c["name"] for c in th.CASES]
LINE = re.compile(r"rtlfm_hip\[tail\]: (.+) done \((.+)\)")
KGAP = 62  # kDeemphGap (run_plan.h)
_T0 = time.time()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(cfg, iq, injected states or None, the oracle's (out, lens, states), per stream the model's flagged alternatives)."""
    from oracle import pyoracle as po
    po.build()
    c = th.case(name)
    cfg, iq, st = th.build(po, c)
    want = po.run_batch(cfg, iq, states=th.copy_states(st) if st else None, nthreads=4)
    arb = cfg.rate_out2 > 0 and cfg.resampler == capi.RESAMPLE_ARBITRARY
    alts = [r[3] for r in th.model_case(po, c, cfg, iq)] if arb else [{} for _ in iq]
    iq.setflags(write=False)
    return cfg, iq, st, want, alts


def _scans(cfg, opts, T):
    return T >= 2048 and 2 <= cfg.deemph_a <= (KGAP - 2) // 2 and not opts.get("deemph_sequential")


def _expected_lines(cfg, opts, plan, nblocks, uniform):
    """The lines of one launch, in order: run_tail() for this geometry (plan: rtlfm_run_route's, for the stages and the
    out-of-place one-pass filter its bit 32 promises)."""
    lines = []
    lpr = cfg.rate_out2 > 0 and cfg.resampler == capi.RESAMPLE_LOW_PASS_REAL
    arb = cfg.rate_out2 > 0 and cfg.resampler == capi.RESAMPLE_ARBITRARY
    assert plan.tail & 31 == (cfg.post_downsample > 1) | 2 * bool(cfg.deemph) | 4 * bool(cfg.dc_block_audio) | 8 * lpr | 16 * arb, plan.as_dict()
    T, Nblk = plan.T, plan.Nblk
    if cfg.post_downsample > 1:
        lines.append("post")
        T //= cfg.post_downsample
        Nblk = T // nblocks
    resampled = False
    if cfg.deemph:
        assert uniform and cfg.deemph_a != 1, "the table keeps deemph_filter behind fronts with uniform counts"
        if plan.tail & 32:
            lines.append("one pass (deemph)" if _scans(cfg, opts, T) else "sequential")
        elif not _scans(cfg, opts, T):
            lines.append("sequential")
        else:
            one_pass = cfg.post_downsample == 1 and not cfg.dc_block_audio and not opts.get("deemph_four_pass")
            l2 = Nblk * cfg.rate_out2 // cfg.rate_out if arb else 0
            ws = (16 * cfg.deemph_a + 64 + 63) // 64 * 64
            if one_pass and lpr and not opts.get("lpr_separate"):
                lines.append("one pass (lpr)"); resampled = True
            elif one_pass and arb and Nblk >= 2 and l2 > Nblk and (Nblk + 1) * l2 < 1 << 31 and ws <= 256:
                lines.append("one pass (arb)"); resampled = True
            else:
                lines += ["a1", "a2", "b", "c"]
                resampled = lpr and not cfg.dc_block_audio and not opts.get("lpr_separate")  # k_deemph_scan_c_lpr
    if cfg.dc_block_audio:
        lines.append("adc")
    if lpr and not resampled:
        lines.append("lpr")
    if arb and not resampled:
        nlo = plan.Nblk // plan.D if cfg.post_downsample == 1 else Nblk
        nhi = nlo + 1 if cfg.post_downsample == 1 and plan.Nblk % plan.D else nlo
        up = [n < n * cfg.rate_out2 // cfg.rate_out for n in (nlo, nhi)]
        lines += ["arb up"] * any(up) + ["arb down"] * (not all(up))
    return lines


def _forms(name):
    """(form, options, path, split) of a row: every form of the tail its configuration has."""
    c = th.case(name)
    cfg = _case(name)[0]
    nb = c["nb"]
    forms = [("plain", {}, 0, False), ("auto", dict(tail_sync=1), 0, False), ("staged", dict(tail_sync=1), 1, False)]
    if nb > 1:
        forms.append(("split", dict(tail_sync=1), 0, True))
    if cfg.deemph:
        forms.append(("sequential", dict(tail_sync=1, deemph_sequential=1), 0, False))
        forms.append(("four_pass", dict(tail_sync=1, deemph_four_pass=1), 0, False))
        if cfg.rate_out2 > 0 and cfg.resampler == capi.RESAMPLE_LOW_PASS_REAL:
            forms.append(("lpr_separate", dict(tail_sync=1, lpr_separate=1), 0, False))
            forms.append(("four_pass_lpr_separate", dict(tail_sync=1, deemph_four_pass=1, lpr_separate=1), 0, False))
        forms.append(("chunk256", dict(tail_sync=1, lpr_chunk=256), 0, False))
        if cfg.rate_out2 > 0 and cfg.resampler == capi.RESAMPLE_ARBITRARY:
            forms.append(("arb_waves1", dict(tail_sync=1, arb_waves=1), 0, False))
    return forms


ONE_PASS = ("one pass (deemph)", "one pass (lpr)", "one pass (arb)")


def _run_form(name, form, opts, path, split, capfd):
    from rtlsdr_amd.demod import GpuDemod
    c = th.case(name)
    cfg, iq, st, (want, want_len, wst), alts = _case(name)
    ns, L, nb = len(iq), c["L"], c["nb"]
    d = torch.from_numpy(np.array(iq)).cuda()
    outs, seen = [[] for _ in range(ns)], []
    capfd.readouterr()
    with GpuDemod(cfg, ns, 0, options=opts) as g:   # a refusal raises: the oracle runs every row
        g.set_path(path)
        for s in range(ns):
            if st is not None:
                g.state_set(s, capi.RtlfmStreamState.from_buffer_copy(bytes(st[s])))
        for b0, b1 in ((0, 1), (1, nb)) if split else ((0, nb),):
            part = d[:, b0 * L:b1 * L].contiguous()
            out = torch.empty((ns, g.result_cap(b1 - b0)), dtype=torch.int16, device="cuda")
            n = torch.zeros(ns, dtype=torch.int32, device="cuda")
            plan = g.run_route(b1 - b0, out.data_ptr(), out.stride(0))
            try:
                g.run_torch(part, out=out, out_len=n)
                g.sync()
            except capi.RtlfmError as e:
                if e.code in (-5, -14):  # -EIO / -EFAULT: a HIP error or a routing bug - nothing more is started on this GPU
                    pytest.exit(f"{name} / {form}: {e}", returncode=3)
                raise
            assert (g.last_route, g.last_rest, g.last_path) == (plan.route, plan.rest, plan.last_path), (name, form, plan.as_dict())
            front = capi.ROUTE_STAGED if path == 1 else capi.ROUTE_FUSED if cfg.downsample_passes else capi.ROUTE_BOXCAR
            assert (g.last_route, g.last_path) == (front, 1 if path == 1 else 2), (name, form, g.last_route, g.last_path)
            assert g.last_rest == (capi.REST_BACK_HALF if path == 1 else capi.REST_TAIL), (name, form, g.last_rest)
            got = LINE.findall(capfd.readouterr().err)
            if opts.get("tail_sync"):
                if any(status != "no error" for _, status in got):
                    pytest.exit(f"{name} / {form}: a kernel of the tail faulted: {got}", returncode=3)
                lines = [what for what, _ in got]
                assert lines == _expected_lines(cfg, opts, plan, b1 - b0, c["uniform"]), (name, form, (b0, b1), lines)
                seen += lines
            else:
                assert not got
            o, n = out.cpu().numpy(), n.cpu().numpy()
            assert (n >= 0).all() and (n <= out.shape[1]).all(), (name, form, n)
            for s in range(ns):
                outs[s].append(o[s, :n[s]].copy())
        sts = [g.state_get(s) for s in range(ns)]
    differ = 0
    for s in range(ns):
        got_s, want_s = np.concatenate(outs[s]), want[s, :want_len[s]]
        assert got_s.shape[0] == want_len[s], (name, form, s, got_s.shape[0], int(want_len[s]))
        bad = np.flatnonzero(got_s != want_s)
        for i in bad:  # only a flagged output may differ, and only by the other truncation of its exact value
            assert int(i) in alts[s] and int(got_s[i]) in alts[s][int(i)], \
                (name, form, s, f"{bad.size} of {got_s.size} differ, first at {bad[:8].tolist()}: got {got_s[bad[:8]].tolist()}, "
                                f"oracle {want_s[bad[:8]].tolist()}, flagged there: {[sorted(alts[s].get(int(k), [])) for k in bad[:8]]}")
        differ += bad.size
        assert gu.state_dict(sts[s], False) == gu.state_dict(wst[s], False), (name, form, s)
    if differ:
        print(f"{name} / {form}: {differ} flagged outputs of {sum(len(a) for a in alts)} took the other truncation of an integer value")
    return seen, plan.T // max(1, cfg.post_downsample)


@pytest.mark.parametrize("name", NAMES)
def test_every_form_of_the_tail_on_the_hard_cases(name, capfd):
    cfg = _case(name)[0]
    ran, T = {}, 0
    for form, opts, path, split in _forms(name):
        ran[form], t = _run_form(name, form, opts, path, split, capfd)
        T = t if form == "auto" else T
    # the forms that were asked for did run, where the row's geometry has them
    if cfg.deemph:
        assert "sequential" in ran["sequential"], (name, ran["sequential"])
        if _scans(cfg, {}, T):
            assert [w for w in ran["four_pass"] if w in ("a1", "a2", "b", "c")] == ["a1", "a2", "b", "c"], (name, ran["four_pass"])
            one = [w for w in ran["auto"] if w in ONE_PASS]
            if cfg.post_downsample == 1 and not cfg.dc_block_audio and (cfg.rate_out2 <= 0 or cfg.resampler == capi.RESAMPLE_LOW_PASS_REAL):
                assert one, (name, ran["auto"])                      # the one-pass kernels are the automatic plan there ...
            if one:
                assert ran["chunk256"] == ran["auto"]                # ... and ran again with chunks of 256 / one wave per stream
                assert ran.get("arb_waves1", ran["auto"]) == ran["auto"]
        if "lpr_separate" in ran:
            assert ran["lpr_separate"][-1] == "lpr" and ran["four_pass_lpr_separate"][-1] == "lpr", (name, ran)
            assert "lpr" not in ran["four_pass"] or cfg.dc_block_audio, (name, ran["four_pass"])  # k_deemph_scan_c_lpr took it
    print(f"{name}: {[(f, ran[f]) for f in ran if f != 'plain']}; {time.time() - _T0:.1f} s into the file")


def test_the_table_reaches_every_kernel_of_the_tail(capfd):
    """The automatic plan alone, on ten rows of the table, takes each of the three one-pass kernels, the four passes, the
    sequential filter and every other stage's own kernel."""
    seen = set()
    for name in ("post4_usb", "deemph13_usb", "deemph40000_usb181", "deemph13_lpr_usb", "deemph2_arb_up_usb181", "deemph13_arb_up_lsb",
                 "deemph13_adc_usb", "lpr_div1_usb", "arb_down_usb181", "post2_deemph4_adc_arb_usb"):
        seen |= set(_run_form(name, "auto", dict(tail_sync=1), 0, False, capfd)[0])
    assert seen >= {"post", "sequential", "one pass (deemph)", "one pass (lpr)", "one pass (arb)", "a1", "a2", "b", "c", "adc", "lpr", "arb up",
                    "arb down"}, sorted(seen)
