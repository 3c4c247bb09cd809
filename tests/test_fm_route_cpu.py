"""The plan of an rtl_fm run without a GPU: rtlfm_run_route (include/rtlfm_hip.h) - the planner the run itself calls,
csrc/run_plan.h - must name, for the rows of tests/fm_route_rows.py, the route and the rest the GPU suite finds in
last_route / last_rest afterwards (tests/test_fm_route_gpu.py).  The same rows go through tools/fm_route_check.cpp, the
planner as a program of its own under AddressSanitizer + UBSan."""
import ctypes as C
import os
import subprocess

import pytest

from cases import make_cfg
from fm_route_rows import ENOTSUP, LAUNCH_OPTIONS, ROWS, STREAMS, out_low_bits, out_stride
from rtlsdr_amd import capi
from rtlsdr_amd.capi import RtlfmCfg, RtlfmRouteOpts, RtlfmRoutePlan
from rtlsdr_amd.demod import run_route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(r):
    """(cfg, nstreams, nblocks, out_low_bits, out_stride, options) of row r: rows of the capacity the header promises."""
    cfg = make_cfg(r["ov"], r["L"], 2)
    ns = 4 if r["chan"] else STREAMS
    cap = capi.load().rtlfm_result_cap(C.byref(cfg)) * r["nb"]
    return cfg, ns, r["nb"], out_low_bits(r), out_stride(r, cap), dict(r["opts"], path=r["path"], channels=r["chan"])


def _plan(r, **more):
    cfg, ns, nb, low, stride, o = _args(r)
    return run_route(cfg, ns, nb, low, stride, **dict(o, **more))


def test_every_route_and_every_rest_is_in_the_table():
    assert {r["want"] for r in ROWS} == set(range(1, 12)) | {ENOTSUP}
    assert {r["rest"] for r in ROWS} == set(range(7)) | {None}
    assert {r["path"] for r in ROWS} == {0, 1, 2} and len(ROWS) > 150


@pytest.mark.parametrize("r", ROWS, ids=lambda r: r["name"])
def test_route_of_the_shapes_the_gpu_suite_runs(r):
    if r["want"] < 0:
        with pytest.raises(capi.RtlfmError) as e:
            _plan(r)
        assert e.value.code == r["want"], r
        return
    p = _plan(r)
    assert (p.route, p.rest) == (r["want"], r["rest"]), (r, p.as_dict())
    staged = p.route in (capi.ROUTE_STAGED, capi.ROUTE_CHAN_MIX, capi.ROUTE_CHAN_FIR_PLAIN, capi.ROUTE_CHAN_BANK_PLAIN)
    assert p.last_path == (1 if staged else 2), (r, p.as_dict())
    assert p.copy_state == int(staged or r["chan"] != 0), (r, p.as_dict())
    levels = bool(r["ov"].get("squelch_level") or r["ov"].get("report_levels"))
    assert p.sq_front == int(levels and p.route in (capi.ROUTE_FUSED, capi.ROUTE_BOXCAR)), (r, p.as_dict())


def test_the_geometry_is_the_runs():
    """N0, Nblk, D, T, varcnt, level, first_irr of a few rows, by hand."""
    by = {r["name"]: r for r in ROWS}
    for name, want in (("p4", dict(N0=8192, Nblk=512, D=1, T=1024, varcnt=0, level=4, first_irr=4, tail=0)),
                       ("box84_squelch_16384", dict(N0=8192, Nblk=8192, D=84, T=196, varcnt=1, level=0, first_irr=0)),
                       ("box10_dword", dict(N0=8192, Nblk=8192, D=10, T=1639, varcnt=1)),
                       ("chan_mix_box8_path0", dict(N0=8192, Nblk=8192, D=8, T=2048, varcnt=0)),
                       ("p10_fir9", dict(N0=32768, Nblk=32, D=1, T=64, level=6, first_irr=10)),
                       ("p9_irregular", dict(N0=768, Nblk=1, T=2, level=6, first_irr=8)),
                       ("p6_c3_tail", dict(tail=2 | 16, tail_follows=1)), ("wbfm", dict(tail=2 | 8, tail_follows=1)),
                       ("p3_deemph_dword_2048", dict(tail=2 | 32, T=2048)), ("p3_deemph_line_1024", dict(tail=2, T=1024)),
                       ("raw_p2", dict(tail_follows=0)), ("raw_p2_dword", dict(tail_follows=1)), ("p4_squelch", dict(tail_follows=1, sq_front=1))):
        got = _plan(by[name]).as_dict()
        assert {k: got[k] for k in want} == want, (name, got)


@pytest.mark.parametrize("want", range(1, 12))
def test_route_does_not_depend_on_the_launch_options(want):
    """fused_waves, fused_min_tiles, fused_tiles_per_seg, box_store, fused_store, lpr_*, arb_waves shape launches; the planner
    does not take them: rtlfm_route_opts has no such field, and a handle's other options cannot reach it."""
    fields = {n for n, _ in RtlfmRouteOpts._fields_}
    assert not fields & set(LAUNCH_OPTIONS) and fields == {"path", "pass0_engine", "squelch_fused", "deep_rest", "deemph_four_pass",
                                                            "deemph_sequential", "arb_serial", "no_deemph_scan", "channels"}
    r = next(r for r in ROWS if r["want"] == want)
    for k, v in LAUNCH_OPTIONS.items():
        with pytest.raises(AttributeError):
            _plan(r, **{k: v})


def test_default_options_are_a_fresh_handles():
    """opts == NULL plans with the values a fresh handle has (the handle's own defaults are kRouteDefaults' fields:
    tests/test_fm_route_gpu.py reads them back from one)."""
    lib = capi.load()
    n = 0
    for r in ROWS:
        if not r["opts"] and r["path"] == 0 and not r["chan"]:
            cfg, ns, nb, low, stride, _ = _args(r)
            a, b = RtlfmRoutePlan(), RtlfmRoutePlan()
            ra = lib.rtlfm_run_route(C.byref(cfg), ns, nb, low, stride, None, C.byref(a))
            rb = lib.rtlfm_run_route(C.byref(cfg), ns, nb, low, stride, C.byref(RtlfmRouteOpts.default()), C.byref(b))
            assert ra == rb == r["want"] and a.as_dict() == b.as_dict(), r
            n += 1
    assert n > 40


def test_arb_serial_and_the_stream_count_only_move_tail_follows():
    """Config 3's tail in line (from 2048 streams on, or arb_serial = 1) leaves the front end a launch that nothing follows."""
    r = next(r for r in ROWS if r["name"] == "p6_c3_tail")
    cfg, _, nb, low, stride, _ = _args(r)
    for ns, serial, follows in ((3, -1, 1), (2047, -1, 1), (2048, -1, 0), (3, 1, 0), (4096, 0, 1)):
        p = run_route(cfg, ns, nb, low, stride, arb_serial=serial)
        assert (p.route, p.rest, p.tail_follows) == (capi.ROUTE_FUSED, capi.REST_TAIL, follows), (ns, serial, p.as_dict())


def test_a_views_flag_keeps_deemph_sequential():
    by = {r["name"]: r for r in ROWS}
    p = _plan(by["p3_deemph_dword_2048"], no_deemph_scan=1)
    assert (p.route, p.tail) == (capi.ROUTE_STAGED, 2), p.as_dict()


def test_what_the_run_refuses_has_no_route():
    lib = capi.load()
    for bad in (dict(block_len=16386), dict(block_len=256), dict(downsample_passes=11), dict(downsample=0), dict(downsample=20000),
                dict(comp_fir_size=5), dict(max_blocks=0), dict(post_downsample=17), dict(deemph=1, deemph_a=0), dict(mode=5),
                dict(block_len=262144, max_blocks=16384)):
        cfg = RtlfmCfg.default(**bad)
        v = lib.rtlfm_cfg_validate(C.byref(cfg))
        assert v < 0, bad
        assert lib.rtlfm_run_route(C.byref(cfg), 3, 1, 0, 1 << 20, None, None) == v, bad
    cfg = RtlfmCfg.default(max_blocks=2)
    ok = lambda *a, **o: lib.rtlfm_run_route(C.byref(cfg), *a, C.byref(RtlfmRouteOpts.default(**o)), None)  # noqa: E731
    assert ok(3, 2, 0, 1 << 20) == capi.ROUTE_BOXCAR
    assert ok(0, 2, 0, 1 << 20) == -22 and ok(3, 0, 0, 1 << 20) == -22
    assert ok(3, 3, 0, 1 << 20) == -7                                      # more buffers than max_blocks: -E2BIG
    assert ok(3, 2, 2, 1 << 20) == -22 and ok(3, 2, 0, (1 << 20) + 1) == -22  # rows off a dword, an odd stride
    assert ok(3, 2, 4, (1 << 20) + 2) == capi.ROUTE_BOXCAR
    for o in (dict(path=3), dict(path=-1), dict(pass0_engine=2), dict(arb_serial=2), dict(channels=4), dict(channels=-1)):
        assert ok(3, 2, 0, 1 << 20, **o) == -22, o
    assert lib.rtlfm_run_route(None, 3, 2, 0, 1 << 20, None, None) == -22
    cfg = RtlfmCfg.default(max_blocks=2, dc_block_raw=1)
    assert ok(4, 2, 0, 1 << 20, channels=capi.CHANNELS_MIXER) == ENOTSUP  # rtlfm_gpu_set_channels refuses -E rdc


def test_fm_route_check_under_the_sanitizers(tmp_path):
    """tools/fm_route_check.cpp with csrc/run_plan.h, under AddressSanitizer + UBSan, over the rows above and over its own
    sweep of configurations (refused ones too), options, alignments and buffer counts."""
    exe = str(tmp_path / "fm_route_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tools", "fm_route_check.cpp")])
    lines = []
    for r in ROWS:
        cfg, ns, nb, low, stride, o = _args(r)
        o = RtlfmRouteOpts.default(**o)
        fields = [getattr(cfg, n) for n, _ in cfg._fields_] + [ns, nb, low, stride] + [getattr(o, n) for n, _ in o._fields_]
        lines.append(" ".join(str(int(v)) for v in fields + [r["want"], r["rest"] if r["rest"] is not None else -1]))
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stdout.startswith(f"fm_route_check: ok, {len(ROWS)} rows"), p.stdout
