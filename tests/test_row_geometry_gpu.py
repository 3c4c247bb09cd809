"""rtl_fm and the channel front ends on rows of every alignment the C ABI accepts (include/rtlfm_hip.h,
rtlfm_gpu_run_device): any d_iq on a 16-byte boundary, any stream_stride that is a multiple of 16, any d_out on a 4-byte
boundary, any even out_stride - "any d_out / out_stride gives the same samples".

Every other GPU test hands the library rows that start on 128-byte lines (GpuDemod.run_torch, .contiguous()).  Here the
rows come from tests/row_geometry.py: the named geometries `line` (that one), `piece` (16-byte aligned, all eight phases
of a line), `dword` and `dword6` (4-byte aligned output rows), the output rows exactly as long as the header promises
(rtlfm_result_cap() * nblocks) inside an allocation full of a sentinel, the input rows inside an allocation filled with
0x00 and then with 0xFF.  Per case, geometry and path:

  1. the project's parity bar against the oracle (test_parity_gpu.assert_parity), and the oracle's state records;
  2. output, lengths and the bytes of rtlfm_gpu_state_get_all() equal to the `line` geometry's on the same path, bit for bit;
  3. no element outside a row's window written;
  4. nothing changes with the bytes around the input rows;
  5. the route that ran (last_path of every run) is in every message."""
import ctypes as C
import errno
from collections import namedtuple

import numpy as np
import pytest

import channel_bank_model as bm
import channel_fir_model as fm
import channel_model as cm
import golden_util as gu
import row_geometry as rg
from cases import CASES, case, make_cfg
from channel_common import full_scale, make_steps, model_runs, random_bank_taps, random_fir_taps, raw_cfg, steps_for
from rtlsdr_amd import capi, synth
from rtlsdr_amd.capi import ATAN_LUT, MODE_RAW, RtlfmCfg
from test_channel_bank_gpu import bins_of
from test_parity_gpu import assert_parity

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

Run = namedtuple("Run", "outs lens state paths stray")
PATHS = [pytest.param(0, id="auto"), pytest.param(1, id="staged")]

# ------------------------------------------------------------------------ cases ----

SLOW_NB = dict(fs=1.024e6, dev_hz=300.0)
DEEMPH_ALONE = dict(downsample=8, downsample_passes=3, deemph=1, deemph_a=8, rate_out=128000, custom_atan=ATAN_LUT)

# name -> (cfg overrides, signal, block_len, runs, streams)
FM_CASES = {n: (ov, sig, 16384, (2, 1), rg.STREAMS) for n, ov, sig in CASES}
for L_ in (1536, 2560):  # buffers that nine and ten passes do not divide: k_fifth_irregular
    FM_CASES[f"p9_L{L_}"] = (dict(downsample=512, downsample_passes=9, rate_out=2000), SLOW_NB, L_, (2, 1), rg.STREAMS)
    FM_CASES[f"p10fir_L{L_}"] = (dict(downsample=1024, downsample_passes=10, comp_fir_size=9, rate_out=2000), SLOW_NB, L_, (2, 1),
                                rg.STREAMS)
for n_ in ("c2_p4_std", "c1_boxcar10_fast", "wbfm_preset", "p4_rdc"):  # a partial tile behind every buffer's whole ones
    FM_CASES[f"{n_}_L11776"] = (*case(n_), 512 * 23, (2, 1), rg.STREAMS)
# at least 16384 samples per stream in one launch: the time-parallel deemph forms
FM_CASES["wbfm_preset_long"] = (*case("wbfm_preset"), 65536, (3,), 5)
FM_CASES["box10_deemph_arb_down96000_long"] = (*case("box10_deemph_arb_down96000"), 65536, (3,), 5)
FM_CASES["p3_deemph_alone_long"] = (DEEMPH_ALONE, dict(fs=1.024e6, dev_hz=60e3), 65536, (3,), 5)
# ... and -E dc behind it, in place in the caller's rows
FM_CASES["p4_deemph_dc_long"] = (dict(downsample=16, downsample_passes=4, dc_block_audio=1, deemph=1, deemph_a=12),
                                 dict(fs=1.024e6, dev_hz=3e3), 65536, (3,), 5)

_inputs, _oracle, _runs = {}, {}, {}


def fm_inputs(name):
    """(cfg, iq [streams, nb * L]): the case's own FM signal, the last stream full-scale random bytes."""
    if name not in _inputs:
        ov, sig, L, runs, ns = FM_CASES[name]
        nb = sum(runs)
        iq = synth.fm_iq_u8(ns, L // 2 * nb, seed=6100 + len(name), **sig)
        iq[ns - 1] = synth.random_u8(1, L * nb, seed=6200 + len(name))[0]
        _inputs[name] = (make_cfg(ov, L, max(runs)), iq)
    return _inputs[name]


def fm_oracle(oracle_lib, name):
    if name not in _oracle:
        cfg, iq = fm_inputs(name)
        _oracle[name] = oracle_lib.run_batch(cfg, iq, nthreads=4)
    return _oracle[name]


def run_rows(cfg, iq, runs, geom, path, fill, nstreams=None, setup=None, options=None):
    """The runs of `runs[k]` buffers of the input rows iq through rtlfm_gpu_run_device, input and output rows of every run
    at the named geometry, the output rows of the capacity the header promises."""
    from rtlsdr_amd.demod import GpuDemod
    g_ = rg.GEOMETRIES[geom]
    L = int(cfg.block_len)
    S = nstreams or iq.shape[0]
    cfg = RtlfmCfg.from_buffer_copy(bytes(cfg))
    cfg.max_blocks = max(runs)
    per_block = capi.load().rtlfm_result_cap(C.byref(cfg))
    outs, lens, paths, bad = [[] for _ in range(S)], [], [], []
    with GpuDemod(cfg, S, 0, options=options) as g:
        g.set_path(path)
        if setup:
            setup(g)
        b0 = 0
        for nb in runs:
            din = rg.DeviceInput(iq[:, b0 * L:(b0 + nb) * L], g_["in_off"], g_["in_pad"], fill)
            cap = per_block * nb
            dout = rg.DeviceOutput(S, cap, g_["out_off"], rg.out_stride(geom, cap))
            g.run_device(din.ptr, din.stride, nb, dout.ptr, dout.stride, dout.len.data_ptr())
            g.sync()
            rows, n, stray = dout.read()
            for s in range(S):
                outs[s].append(rows[s])
            lens.append(n)
            paths.append(g.last_path)
            bad.append(rg.describe_stray(stray, dout.plan) + [int(stray.size)] if stray.size else [])
            b0 += nb
        state = bytes(g.state_get_all())
    return Run([np.concatenate(x) for x in outs], np.stack(lens), state, paths, bad)


def fm_run(name, geom, path, fill=0x00):
    key = (name, geom, path, fill)
    if key not in _runs:
        cfg, iq = fm_inputs(name)
        _runs[key] = run_rows(cfg, iq, FM_CASES[name][3], geom, path, fill)
    return _runs[key]


def assert_same(a, b, what):
    """Two runs: rows, lengths and state records equal in every bit."""
    assert np.array_equal(a.lens, b.lens), f"{what}: lengths {a.lens.tolist()} for {b.lens.tolist()}"
    for s, (x, y) in enumerate(zip(a.outs, b.outs, strict=True)):
        if not np.array_equal(x, y):
            d = np.flatnonzero(x != y)
            raise AssertionError(f"{what}: stream {s}: {d.size} of {x.size} samples differ, first at {d[:8].tolist()}: "
                                 f"{x[d[:4]].tolist()} for {y[d[:4]].tolist()}")
    if a.state != b.state:
        n = len(a.state) // len(a.outs)
        diff = [s for s in range(len(a.outs)) if a.state[s * n:(s + 1) * n] != b.state[s * n:(s + 1) * n]]
        raise AssertionError(f"{what}: the state records of streams {diff} differ")


def assert_clean(r, what):
    assert not any(r.stray), f"{what}: elements outside the rows' windows were written; per run (row, offset from its start) ... count: {r.stray}"


def check_geometry(run, name, geom, path, compare):
    """Assertions 2 - 5 for one case, geometry and path; `compare(got, what)` is assertion 1."""
    got, gotF, line = run(name, geom, path, 0x00), run(name, geom, path, 0xFF), run(name, "line", path, 0x00)
    what = f"{name} {geom} path={path} last_path={got.paths}"
    assert_clean(got, what)
    assert_clean(gotF, what + " (0xFF around the input)")
    compare(got, what)
    assert got.paths == line.paths or geom in ("dword", "dword6"), f"{what}: line took {line.paths}"
    assert_same(got, line, what + f" against line ({line.paths})")
    assert gotF.paths == got.paths, what
    assert_same(gotF, got, what + ": 0xFF around the input rows against 0x00")


# ------------------------------------------------------------------------ rtl_fm ----

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("geom", list(rg.GEOMETRIES))
@pytest.mark.parametrize("name", list(FM_CASES))
def test_rtlfm_rows_of_any_accepted_alignment(oracle_lib, name, geom, path):
    cfg, _ = fm_inputs(name)
    want, want_len, wst = fm_oracle(oracle_lib, name)
    states = (capi.RtlfmStreamState * len(want_len))

    def compare(got, what):
        st = states.from_buffer_copy(got.state)
        for s in range(len(want_len)):
            assert_parity(got.outs[s], want[s, :want_len[s]], cfg, f"{what} stream {s}")
            assert gu.state_dict(st[s], False) == gu.state_dict(wst[s], False), f"{what} stream {s}: state"

    check_geometry(fm_run, name, geom, path, compare)
    got = fm_run(name, geom, path)
    if path == 1:
        assert got.paths == [1] * len(got.paths), (name, geom, got.paths)


FORMS = [
    # the store forms that large launches take by themselves: whole 128-byte lines, non-temporal (k_boxcar_scan finds the
    # lines from the row's address bits and keeps the rest of a tile's last line in LDS)
    ("c1_boxcar10_fast", dict(box_store=1)), ("raw_box10", dict(box_store=1)), ("box256_std", dict(box_store=1)),
    ("p3_lut", dict(fused_store=1)),
    # the four-pass deemph_filter, in place in the caller's rows: its chunks begin at a row's first 16-byte boundary
    ("p3_deemph_alone_long", dict(deemph_four_pass=1)), ("p4_deemph_dc_long", dict(deemph_four_pass=1)),
    # ... and in front of low_pass_real; the resampler's other store forms
    ("wbfm_preset_long", dict(deemph_four_pass=1)), ("wbfm_preset_long", dict(lpr_separate=1)),
    ("wbfm_preset_long", dict(lpr_ring=0)), ("wbfm_preset_long", dict(lpr_scalar_stores=1)),
]


@pytest.mark.parametrize("geom", list(rg.GEOMETRIES))
@pytest.mark.parametrize("name,options", FORMS, ids=[f"{n}-{k}" for n, o in FORMS for k in o])
def test_store_and_tail_forms_on_rows_of_any_accepted_alignment(name, options, geom):
    """The forms a handle takes only by size or by option (none changes a result): the same samples, lengths and state as
    the default forms on line-aligned rows, and nothing outside a row's window."""
    cfg, iq = fm_inputs(name)
    runs = FM_CASES[name][3]
    want = fm_run(name, "line", 0)
    for fill in (0x00, 0xFF):
        got = run_rows(cfg, iq, runs, geom, 0, fill, options=options)
        what = f"{name} {options} {geom} last_path={got.paths} fill={fill:#x}"
        assert_clean(got, what)
        assert_same(got, want, what + " against the default forms on line")


def test_routes_change_where_the_code_says():
    """The decisions rtlfm_hip.hip takes from d_out & 15 and out_stride & 7, seen through last_path: an FM chain without an
    audio tail stores 16-byte vectors straight into the caller's rows and so leaves the one-launch front end for rows that
    are only 4-byte aligned (can_fuse = false); -M raw writes the caller's rows from the front end on 16-byte aligned rows
    (raw_direct) and goes through the handle's own buffer otherwise - one launch either way, and the same samples."""
    paths = {g: fm_run("c2_p4_std", g, 0).paths for g in ("line", "piece", "dword")}
    assert paths["line"] == [2, 2] and paths["piece"] == [2, 2], paths
    assert paths["dword"] == [1, 1], paths
    for name in ("raw_box10", "raw_p2"):
        a, b = fm_run(name, "piece", 0), fm_run(name, "dword", 0)
        assert a.paths == [2, 2] and b.paths == [2, 2], (name, a.paths, b.paths)
        assert_same(a, b, f"{name}: piece (raw_direct) against dword")
    # where an out-of-place stage of the audio tail writes the caller's rows (low_pass_simple, a resampler), and behind the
    # boxcar, whose stores find their own alignment, the front end stays the one-launch kernel
    for name in ("p4_post4", "c3_p6_fir9_deemph_up22050", "c1_boxcar10_fast"):
        assert fm_run(name, "dword", 0).paths == [2, 2], name


def test_refusals_move_nothing(oracle_lib):
    """What the header does not accept is -EINVAL, and the handle is as it was: the correct call behind every refusal
    gives the oracle's output and state."""
    from rtlsdr_amd.demod import GpuDemod
    ov, sig = case("c2_p4_std")
    L, nb, ns = 16384, 3, 2
    cfg = make_cfg(ov, L, nb)
    iq = synth.fm_iq_u8(ns, L // 2 * nb, seed=99, **sig)
    want, want_len, wst = oracle_lib.run_batch(cfg, iq, nthreads=2)
    cap = capi.load().rtlfm_result_cap(C.byref(cfg)) * nb
    st = rg.out_stride("line", cap)
    refused = [("d_iq + 8", dict(iq=8)), ("stream_stride + 8", dict(stride=8)), ("stream_stride - 16", dict(stride=-16)),
               ("d_out + 1 element", dict(out=2)), ("odd out_stride", dict(ostride=1))]
    for what, d in refused:
        with GpuDemod(cfg, ns, 0) as g:
            din = rg.DeviceInput(iq, 0, 32)   # (room for a longer stride)
            dout = rg.DeviceOutput(ns, cap, 0, st + 2)
            r = g.lib.rtlfm_gpu_run_device(g._h, din.ptr + d.get("iq", 0), nb * L + d.get("stride", 0), nb,
                                           dout.ptr + d.get("out", 0), st + d.get("ostride", 0), dout.len.data_ptr())
            assert r == -errno.EINVAL, (what, r)
            g.sync()
            _, n, stray = dout.read()
            assert not n.any() and stray.size == 0 and (dout.t.cpu().numpy() == rg.SENTINEL).all(), what
            g.run_device(din.ptr, din.stride, nb, dout.ptr, dout.stride, dout.len.data_ptr())
            g.sync()
            rows, n, stray = dout.read()
            states = g.state_get_all()
            assert stray.size == 0, what
            for s in range(ns):
                assert_parity(rows[s], want[s, :want_len[s]], cfg, f"behind the refusal of {what}, stream {s}")
                assert gu.state_dict(states[s], False) == gu.state_dict(wst[s], False), what


def test_host_fetch_into_rows_of_an_odd_stride(oracle_lib):
    """rtlfm_gpu_fetch_all / _fetch_all_prev into host rows cap + 1 apart: every row equals fetch(s), and nothing but
    [row, row + lens[s]) is touched."""
    from rtlsdr_amd.demod import GpuDemod
    ov, sig = case("c1_boxcar10_fast")
    L, ns = 16384, 3
    cfg = make_cfg(ov, L, 2)
    iq = synth.fm_iq_u8(ns, L // 2 * 3, seed=98, **sig)
    cap = capi.load().rtlfm_result_cap(C.byref(cfg)) * 2
    stride = cap + 1
    assert stride % 2 == 1

    def fetch_rows(g, fn):
        buf = np.full(ns * stride + 64, rg.SENTINEL, dtype=np.int16)
        lens = np.zeros(ns, dtype=np.int32)
        capi.check(fn(g._h, buf[32:].ctypes.data, stride, lens.ctypes.data), "fetch_all")
        touched = buf != rg.SENTINEL
        rows = []
        for s in range(ns):
            a = 32 + s * stride
            rows.append(buf[a:a + lens[s]].copy())
            touched[a:a + lens[s]] = False
        assert not touched.any(), np.flatnonzero(touched)[:8].tolist()
        return rows

    with GpuDemod(cfg, ns, 0) as g:
        for s in range(ns):
            g.push(iq[s, :L], s)
            g.push(iq[s, L:2 * L], s)
        g.run()
        first = [g.fetch(s) for s in range(ns)]
        rows = fetch_rows(g, g.lib.rtlfm_gpu_fetch_all)
        for s in range(ns):
            assert first[s].size > 0 and np.array_equal(rows[s], first[s]), s
        for s in range(ns):
            g.push(iq[s, 2 * L:], s)
        g.run()
        prev = fetch_rows(g, g.lib.rtlfm_gpu_fetch_all_prev)
        second = [g.fetch(s) for s in range(ns)]
        rows = fetch_rows(g, g.lib.rtlfm_gpu_fetch_all)
        for s in range(ns):
            assert np.array_equal(prev[s], first[s]), s
            assert np.array_equal(rows[s], second[s]), s
    want, want_len, _ = oracle_lib.run_batch(make_cfg(ov, L, 3), iq, nthreads=2)
    for s in range(ns):
        assert_parity(np.concatenate([first[s], second[s]]), want[s, :want_len[s]], cfg, f"push / run / fetch_all stream {s}")


# ---------------------------------------------------------------------- channels ----

CH_RUNS = (1, 2)
CH_L, CH_D, CH_NSRC = 2048, 10, 3
_ch = {}


def channel_case(front):
    """(cfg, source bytes, streams, setup(g), the model's rows, the model's prev_index) of one front end: -M raw on
    full-scale bytes."""
    if front in _ch:
        return _ch[front]
    src = full_scale(CH_NSRC, sum(CH_RUNS) * CH_L, 4100 + len(front))
    cfg = raw_cfg(CH_D, CH_L, nb=max(CH_RUNS))
    if front == "bank":
        K = 16
        bins = bins_of("subset", K, 3)
        taps, shift = random_bank_taps(K, 8 * K, 77)
        S = CH_NSRC * len(bins)
        model = bm.BankModel(K, taps, shift, CH_D, CH_NSRC, bins=bins)
        want, _ = model_runs(model, src, CH_L, CH_RUNS)
        p0 = list(model.p0)

        def setup(g):
            g.set_channels(len(bins), steps=steps_for(S))
            g.set_channel_bank(K, taps, shift, bins=bins)
    else:
        per = 5
        S = CH_NSRC * per
        steps = make_steps(S, 21)
        if front == "fir":
            taps, shift = random_fir_taps(80, 78)
            model = fm.FirModel(steps, per, CH_D, taps, shift, CH_NSRC)
            want, _ = model_runs(model, src, CH_L, CH_RUNS)
            p0 = list(model.p0)
        else:
            rows, state, b0 = [[] for _ in range(S)], None, 0
            for nb in CH_RUNS:
                r, state = cm.model_raw_boxcar(src[:, b0 * CH_L:(b0 + nb) * CH_L], steps, CH_D, state, per_source=per, pos=b0 * CH_L // 2)
                for s in range(S):
                    rows[s].append(r[s])
                b0 += nb
            want = [np.concatenate(x) for x in rows]
            p0 = [state[s]["prev_index"] for s in range(S)]
            taps = None

        def setup(g):
            g.set_channels(per, steps=steps)
            if taps is not None:
                g.set_channel_filter(taps, shift)
    _ch[front] = (cfg, src, S, setup, want, p0)
    return _ch[front]


def channel_run(front, geom, path, fill=0x00):
    key = ("channels", front, geom, path, fill)
    if key not in _runs:
        cfg, src, S, setup, _, _ = channel_case(front)
        _runs[key] = run_rows(cfg, src, CH_RUNS, geom, path, fill, nstreams=S, setup=setup)
    return _runs[key]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("geom", ["line", "piece", "dword"])
@pytest.mark.parametrize("front", ["boxcar", "fir", "bank"])
def test_channel_front_ends_on_rows_of_any_accepted_alignment(front, geom, path):
    """k_channel_boxcar, k_channel_fir and k_channel_bank (path 0) and their staged cross-checks (path 1): the source rows at
    the input geometry, the stream rows at the output geometry, against the models."""
    cfg, src, S, _, want, p0 = channel_case(front)
    states = (capi.RtlfmStreamState * S)

    def compare(got, what):
        for s in range(S):
            assert got.outs[s].shape == want[s].shape, (what, s, got.outs[s].shape, want[s].shape)
            if not np.array_equal(got.outs[s], want[s]):
                d = np.flatnonzero(got.outs[s] != want[s])
                raise AssertionError(f"{what} stream {s}: {d.size} of {want[s].size} differ from the model, first at {d[:8].tolist()}")
        st = states.from_buffer_copy(got.state)
        assert [st[s].prev_index for s in range(S)] == p0, what

    check_geometry(channel_run, front, geom, path, compare)
    assert channel_run(front, geom, path).paths == [2 if path == 0 else 1] * len(CH_RUNS)
