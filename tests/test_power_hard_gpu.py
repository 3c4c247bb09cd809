"""Every rtl_power route on a real MI355X against the oracle on inputs that make fix_fft's int16 stores wrap
(tests/golden/power_hard.json: hard-limited tones, rails 0 / 254), on the bytes at the rails themselves and on one stream
of random bytes: avg[] identical, samples equal, last_kernel the intended route.  The model (tests/power_hard.py) says on the
host that the streams of a case still wrap in every stage the record promises for its size - a case whose inputs stopped
wrapping fails.  Each case at the smallest shape that takes its route, sum and peak hold, in one launch and in two.

Not here: k_power_fft_gl<3>, which first runs at 2^18 bins (stages 14 .. 16 of 18; up to 2^17 the last pass,
k_power_fft_gl_acc<1 | 2 | 3>, takes every stage beyond 13) - the model needs a quarter of a second per frame there."""
import functools

import numpy as np
import pytest

import power_hard as ph
from rtlsdr_amd import synth
from rtlsdr_amd.capi import RtlpowerCfg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

K_GENERAL, K_BIG, K_FRAMES, K_DECIMATED, K_STAGED, K_STAGED_FAST = 1, 2, 3, 4, 5, 6
RECORD = ph.load()
NR = RECORD["reads"]
MAX_STREAMS = 8  # per handle

# (route, recorded case whose sets are the streams, what differs from the case's cfg, options, rows 8 bytes longer than their reads)
ROUTES = [
    (K_GENERAL, "b3", dict(bin_e=1), dict(scan_frames=0), False),  # one stage: nothing can wrap; the rails and the window fold
    (K_GENERAL, "b6", {}, dict(scan_frames=0), False),
    (K_GENERAL, "b10", {}, dict(scan_frames=0), False),
    (K_GENERAL, "b13", {}, {}, True),
    (K_GENERAL, "b6", dict(window=5), dict(scan_frames=0), False),
    (K_FRAMES, "b3", {}, {}, False),
    (K_FRAMES, "b7", {}, {}, False),
    (K_FRAMES, "b12", {}, {}, False),
    (K_FRAMES, "b12", dict(buf_len=32768), {}, False),  # k_power_scan_frames<14>: reads of 16384 points
    (K_FRAMES, "b7", dict(window=7, buf_len=32768), {}, False),
    (K_BIG, "b13", {}, {}, False),                # (eight streams or fewer: every read has a workgroup of its own, the
    (K_BIG, "b14", {}, {}, False),                #  partial accumulators meet through the atomics)
    (K_BIG, "b14", {}, dict(groups=2), False),    # ... and two workgroups per stream, two reads and one
    (K_BIG, "b13", dict(window=1), {}, False),
    (K_STAGED_FAST, "b15", {}, {}, False),        # k_power_fft_gl_acc<1>
    (K_STAGED_FAST, "b16", {}, {}, False),        # <2>
    (K_STAGED_FAST, "b17", {}, {}, False),        # <3>
    (K_STAGED_FAST, "b15", dict(window=1), {}, False),
    (K_STAGED, "b15", {}, dict(staged_fast=0), False),
    (K_STAGED, "b16", {}, dict(staged_fast=0), False),
    (K_STAGED, "b17", {}, dict(staged_fast=0), False),
    (K_STAGED, "b15", dict(window=6), dict(staged_fast=0), False),
    (K_STAGED, "b10", dict(buf_len=65536), {}, False),  # reads beyond one workgroup's LDS: k_power_fft_lds + k_power_accum,
    (K_STAGED, "b14", dict(buf_len=65536), {}, False),  # 32 frames a read and two
    (K_DECIMATED, "b10_box4", {}, {}, False),
    (K_DECIMATED, "b9_fifth2_fir9", {}, {}, False),
    (K_DECIMATED, "b10_box4", dict(window=1), {}, False),
    (K_DECIMATED, "b9_fifth2_fir9", dict(window=4), {}, False),
    (K_GENERAL, "b10_box4", {}, dict(dec_fast=0), False),
    (K_GENERAL, "b9_fifth2_fir9", {}, dict(dec_fast=0), False),
]


def _id(v):
    return "-".join(f"{k[:3]}{x}" for k, x in v.items()) or "-" if isinstance(v, dict) else str(v)


@functools.lru_cache(maxsize=None)
def _inputs(case, L):
    """(the recorded sets' streams, those + the rail streams + one of random bytes) for NR reads of L bytes."""
    c = RECORD["cases"][case]
    hard = np.stack([ph.stream(rec, L // 2 * NR) for rec in c["sets"]])
    every = np.concatenate([hard, ph.rail_streams(L * NR), synth.random_u8(1, L * NR, seed=1000 + c["cfg"]["bin_e"])])
    hard.setflags(write=False); every.setflags(write=False)
    return hard, every


@functools.lru_cache(maxsize=None)
def _driven(case, L):
    """Stores that wrap per stage, by the model, over the case's streams under the rectangle window."""
    cfg = RtlpowerCfg.default(**{**RECORD["cases"][case]["cfg"], "window": 0, "buf_len": L})
    return sum(ph.model_scan(cfg, row)[2] for row in _inputs(case, L)[0])


@functools.lru_cache(maxsize=None)
def _want(case, diff, peak):
    from oracle import pyoracle as po
    po.build()
    cfg = RtlpowerCfg.default(**{**RECORD["cases"][case]["cfg"], "window": 0, **dict(diff), "peak_hold": peak})
    return po.power_scan_batch(cfg, _inputs(case, int(cfg.buf_len))[1], nthreads=4)


@pytest.mark.parametrize("peak", [0, 1], ids=["sum", "peak"])
@pytest.mark.parametrize("route,case,diff,opts,wide", ROUTES, ids=_id)
def test_route_on_wrapping_streams(route, case, diff, opts, wide, peak):
    from rtlsdr_amd.power import GpuPower
    c = RECORD["cases"][case]
    kw = {**c["cfg"], "window": 0, **diff, "peak_hold": peak}
    cfg = RtlpowerCfg.default(**kw)
    L = int(cfg.buf_len)
    iq = _inputs(case, L)[1]
    if kw["window"] == 0 and kw["bin_e"] == c["cfg"]["bin_e"]:
        # the inputs still do what they are here for (in reads longer than the recorded ones remove_dc's average is another:
        # the counts differ, the stages must not)
        driven = _driven(case, L)
        print(f"{case}: stores that wrap per stage {[int(w) for w in driven]}")
        assert L != c["cfg"]["buf_len"] or [int(w) for w in driven] == c["total_wraps"], (case, driven)
        assert driven[0] == 0 and driven[1] == 0
        for s in c["stages"]:
            assert driven[int(s)] > 0, (case, s)
        assert len(c["stages"]) + len(c["missing"]) == max(0, kw["bin_e"] - 2)
    want, wn = _want(case, tuple(sorted(diff.items())), peak)
    for s0 in range(0, len(iq), MAX_STREAMS):
        rows = iq[s0:s0 + MAX_STREAMS]
        ns = len(rows)
        d = torch.zeros((ns, L * NR + (8 if wide else 0)), dtype=torch.uint8, device="cuda")
        d[:, :L * NR] = torch.from_numpy(np.array(rows)).cuda()  # (a copy: the shared inputs are read-only)
        for split in (None, 1):
            with GpuPower(cfg, ns, 0) as g:
                for k, v in opts.items():
                    g.set_option(k, v)
                for r0, nr in ((0, NR),) if split is None else ((0, split), (split, NR - split)):
                    g.scan_device(d.data_ptr() + r0 * L, d.stride(0), nr)
                    g.sync()
                    assert g.last_kernel == route, (kw, opts, split, g.last_kernel)
                for s in range(ns):
                    avg, n = g.fetch(s)
                    assert n == wn[s0 + s], (kw, opts, split, s0 + s)
                    bad = np.flatnonzero(avg != want[s0 + s])
                    assert bad.size == 0, (kw, opts, split, s0 + s, bad.size, bad[:8], avg[bad[:4]], want[s0 + s][bad[:4]])
