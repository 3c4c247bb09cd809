"""The route a run took against the route its plan names: for every row of tests/fm_route_rows.py that a handle can be
brought to, a run of two buffers of three streams (channels: 2 sources x 2 channels) - or of one buffer where the row
says so - must leave in last_route / last_rest / last_path what rtlfm_run_route predicts for the handle's configuration,
options and output rows, which is what the row expects; and the rows, lengths and state records must equal the same run
under rtlfm_gpu_set_path(1) in every bit wherever both exist.  One ragged ring run: last_route is the last view's."""
import ctypes as C

import numpy as np
import pytest

import row_geometry as rg
from cases import make_cfg
from channel_common import random_bank_taps, random_fir_taps, steps_for
from fm_route_rows import ENOTSUP, PLACES, ROWS, STREAMS, out_stride
from rtlsdr_amd import capi, synth
from rtlsdr_amd.capi import CHANNELS_BANK, CHANNELS_FILTER, RtlfmRouteOpts
from rtlsdr_amd.demod import GpuDemod, run_route

pytestmark = pytest.mark.gpu

GPU_ROWS = [r for r in ROWS if r["gpu"]]
_inputs, _staged = {}, {}


def _input(rows, L):
    """uint8 [rows, 2 L]: an FM signal, the last row full-scale random bytes (made once per shape)."""
    if (rows, L) not in _inputs:
        iq = synth.fm_iq_u8(rows, L, seed=5300 + rows, fs=1.024e6, dev_hz=3e3)
        iq[rows - 1] = synth.random_u8(1, 2 * L, seed=5301)[0]
        _inputs[rows, L] = iq
    return _inputs[rows, L]


def _open(r, path):
    """A handle in row r's state with rtlfm_gpu_set_path(path).  (apart_budget_gb = 0: no placement search for rows of a
    few KiB - the option is no input of the plan.)"""
    cfg = make_cfg(r["ov"], r["L"], 2)
    g = GpuDemod(cfg, 4 if r["chan"] else STREAMS, 0, options=dict(apart_budget_gb=0))
    g.set_path(path)  # (in front of the options: set_path(2) puts pass0_engine back to the compiled default)
    for k, v in r["opts"].items():
        g.set_option(k, v)
    if r["chan"]:
        g.set_channels(2, steps=steps_for(4))
        if r["chan"] == CHANNELS_FILTER:
            g.set_channel_filter(*random_fir_taps(33, 5))
        if r["chan"] == CHANNELS_BANK:
            K = 16
            taps, shift = random_bank_taps(K, 8 * K, 77)
            g.set_channel_bank(K, taps, shift, bins=[1, 5])
    return g


def _run(r, path, predict=False):
    """One run of row r's buffers into rows at the row's place.  Returns (r of rtlfm_gpu_run_device, per stream rows,
    lengths, state records, (last_route, last_rest, last_path), the plan predicted for exactly these rows or its error)."""
    with _open(r, path) as g:
        L, nb, S = r["L"], r["nb"], g.nstreams
        iq = _input(2 if r["chan"] else STREAMS, L)[:, :nb * L]
        off = PLACES[r["place"]][0]
        cap = capi.load().rtlfm_result_cap(C.byref(g.cfg)) * nb
        din = rg.DeviceInput(iq, 0, 0)
        dout = rg.DeviceOutput(S, cap, off, out_stride(r, cap))
        plan = None
        if predict:
            try:
                plan = g.run_route(nb, dout.ptr, dout.stride)
            except capi.RtlfmError as e:
                plan = e.code
        rc = g.lib.rtlfm_gpu_run_device(g._h, din.ptr, din.stride, nb, dout.ptr, dout.stride, dout.len.data_ptr())
        g.sync()
        if rc < 0:
            return rc, None, None, None, None, plan
        rows, n, stray = dout.read()
        assert stray.size == 0, (r["name"], path, rg.describe_stray(stray, dout.plan))
        return rc, rows, n, bytes(g.state_get_all()), (g.last_route, g.last_rest, g.last_path), plan


def _staged_twin(r):
    """The same run under rtlfm_gpu_set_path(1): once per (configuration, options, channels, place, buffers)."""
    key = (tuple(sorted(r["ov"].items())), r["L"], tuple(sorted(r["opts"].items())), r["chan"], r["place"], r["nb"])
    if key not in _staged:
        _staged[key] = _run(r, 1)
    return _staged[key]


@pytest.mark.parametrize("r", GPU_ROWS, ids=lambda r: r["name"])
def test_the_run_takes_the_route_its_plan_names(r):
    rc, rows, n, state, last, plan = _run(r, r["path"], predict=True)
    print(f"{r['name']}: run {rc}, last (route, rest, path) {last}, predicted {plan if isinstance(plan, int) else (plan.route, plan.rest, plan.last_path)}")
    if r["want"] < 0:
        assert rc == r["want"] == plan == ENOTSUP, (r, rc, plan)
        return
    assert rc == 0, (r, rc)
    assert last == (plan.route, plan.rest, plan.last_path), (r, last, plan.as_dict())
    assert last[:2] == (r["want"], r["rest"]), (r, last)
    rc1, rows1, n1, state1, last1, _ = _staged_twin(r)
    assert rc1 == 0 and last1[2] == 1, (r, rc1, last1)
    assert np.array_equal(n, n1), (r["name"], n.tolist(), n1.tolist())
    for s, (a, b) in enumerate(zip(rows, rows1, strict=True)):
        if not np.array_equal(a, b):
            d = np.flatnonzero(a != b)
            raise AssertionError(f"{r['name']} stream {s}: {d.size} of {a.size} samples differ from path 1, first at {d[:8].tolist()}")
    assert state == state1, f"{r['name']}: the state records differ from path 1's"


def test_a_fresh_handles_options_are_the_planners_defaults():
    d = RtlfmRouteOpts.default()
    with GpuDemod(make_cfg({}, 16384, 1), 1, 0) as g:
        for name in ("pass0_engine", "squelch_fused", "deep_rest", "deemph_four_pass", "deemph_sequential", "arb_serial"):
            assert g.get_option(name) == getattr(d, name), name
        assert (g.last_route, g.last_rest, g.last_path) == (0, 0, 0)
        g.set_path(3)
        assert g.get_option("pass0_engine") == 0


def test_a_ragged_ring_run_leaves_the_last_views_route():
    """The squelch behind the boxcar over the ring, buffers of two lengths: streams of 16384 bytes take k_boxcar_scan's SQ
    form, a stream of 8192 bytes its emit mode - each range of streams is a view that plans for its own length, and the
    handle reads what the last one took."""
    ov = dict(downsample=84, rate_out=12000, squelch_level=50, custom_atan=capi.ATAN_FAST)
    L = 16384
    cfg = make_cfg(ov, L, 1)
    iq = _input(STREAMS, L)
    for short, want in ((2, (capi.ROUTE_BOXCAR_EMIT, capi.REST_BACK_HALF, 2)), (0, (capi.ROUTE_BOXCAR, capi.REST_TAIL, 2))):
        with GpuDemod(cfg, STREAMS, 0, options=dict(apart_budget_gb=0)) as g:
            for s in range(STREAMS):
                g.rtlsdr_callback(iq[s, :L // 2 if s == short else L], s)
            g.full_demod()
            g.sync()
            assert (g.last_route, g.last_rest, g.last_path) == want, short
            # the last view: the streams behind the short one (or the short one itself), one buffer of its own length
            last_len = L // 2 if short == STREAMS - 1 else L
            view_cfg = make_cfg(ov, last_len, 1)
            p = run_route(view_cfg, 1 if short == STREAMS - 1 else STREAMS - 1 - short, 1, no_deemph_scan=1)
            assert (p.route, p.rest, p.last_path) == want, (short, p.as_dict())
