"""The plan of an rtl_power scan without a GPU: rtlpower_scan_route (include/rtlpower_hip.h) - the planner the scan
itself calls - must name, for the shapes the GPU suite scans, the transform that suite finds in last_kernel afterwards.
The same rows go through tools/route_check.cpp, the planner as a program of its own under AddressSanitizer + UBSan."""
import ctypes as C
import os
import subprocess

import pytest

from rtlsdr_amd import build as hipbuild
from rtlsdr_amd import capi
from rtlsdr_amd.capi import RtlpowerCfg, RtlpowerRouteOpts
from rtlsdr_amd.power import scan_route
from test_power_gpu import _decimated_cases
from test_power_report_gpu import FAMILIES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_NONE, K_GENERAL, K_BIG, K_FRAMES, K_DECIMATED, K_STAGED, K_STAGED_FAST = range(7)  # enum rtlpower_kernel
MAX_POINTS = 16384  # what one workgroup's LDS holds (power_kernels.h, kMaxPoints)


def _row(want, kw, opts=None, ns=4, nr=3, pad=0, addr=0):
    """One scan: nr reads of ns streams, rows `pad` bytes longer than their reads, the first at an address whose low
    bits are `addr`."""
    return dict(want=want, kw=kw, opts=dict(opts or {}), ns=ns, nr=nr, pad=pad, addr=addr)


def route_rows():
    rows = [_row(family, kw, opts) for family, kw, opts in FAMILIES]
    for kw in _decimated_cases():
        L, ds, N = kw["buf_len"], kw["downsample"], 1 << kw["bin_e"]
        per = (L // ds) // 2
        fast_expected = 512 <= per <= 8192 and per & (per - 1) == 0 and (L // 2) % ds == 0 and N <= per  # test_power_decimated_scans
        chunks = -(-(L // ds) // (2 * N))
        slow = K_STAGED if chunks * N > MAX_POINTS else K_GENERAL
        for dec_fast in (1, 0):
            rows.append(_row(K_DECIMATED if fast_expected and dec_fast else slow, kw, dict(dec_fast=dec_fast), ns=3, nr=5))
    for bin_e in range(15, 22):  # one frame per read beyond 16384 points
        kw = dict(bin_e=bin_e, buf_len=2 << bin_e)
        rows += [_row(K_STAGED_FAST, kw), _row(K_STAGED, kw, dict(staged_fast=0)), _row(K_STAGED, kw, pad=8), _row(K_STAGED, kw, addr=8)]
    for bin_e in (13, 14):
        kw = dict(bin_e=bin_e, buf_len=2 << bin_e)
        rows += [_row(K_BIG, kw), _row(K_GENERAL, kw, pad=8), _row(K_GENERAL, kw, addr=8)]
    for L in (16384, 32768):  # several frames per read
        for bin_e in range(3, 13):
            if (2 << bin_e) < L:
                kw = dict(bin_e=bin_e, buf_len=L)
                rows += [_row(K_FRAMES, kw), _row(K_GENERAL, kw, dict(scan_frames=0))]
    rows.append(_row(K_NONE, dict(bin_e=0, buf_len=16384)))
    return rows


ROWS = route_rows()


def _route(r, **more):
    cfg = RtlpowerCfg.default(**r["kw"])
    return scan_route(cfg, r["ns"], r["nr"], r["nr"] * int(cfg.buf_len) + r["pad"], r["addr"], **dict(r["opts"], **more))


def test_every_family_is_in_the_table():
    assert {r["want"] for r in ROWS} == set(range(7))
    assert len(FAMILIES) == 10 and len(_decimated_cases()) > 50


@pytest.mark.parametrize("r", ROWS, ids=lambda r: "-".join(f"{k[:3]}{v}" for k, v in {**r["kw"], **r["opts"], "pad": r["pad"], "addr": r["addr"]}.items()
                                                          if k in ("bin_e", "downsample", "boxcar", "buf_len", "pad", "addr") or k in r["opts"]))
def test_route_of_the_shapes_the_gpu_suite_scans(r):
    assert _route(r) == r["want"], r


@pytest.mark.parametrize("family", range(1, 7))
def test_route_does_not_depend_on_the_launch_options(family):
    r = next(r for r in ROWS if r["want"] == family)
    for groups in (0, 1, 3, 1000):
        for staged_batch in (0, 1, 2):
            for staged_pipe in (0, 1, 2):
                assert _route(r, groups=groups, staged_batch=staged_batch, staged_pipe=staged_pipe) == family, (r, groups, staged_batch, staged_pipe)


def test_default_options_are_the_handles():
    """opts == NULL plans with the defaults a fresh handle has."""
    lib = capi.load()
    for r in ROWS:
        if not r["opts"]:
            cfg = RtlpowerCfg.default(**r["kw"])
            assert lib.rtlpower_scan_route(C.byref(cfg), r["ns"], r["nr"], r["nr"] * int(cfg.buf_len) + r["pad"], r["addr"], None) == r["want"], r


def test_what_the_scan_refuses_has_no_route():
    lib = capi.load()
    o = RtlpowerRouteOpts.default()
    for bad in (dict(bin_e=22), dict(buf_len=16386), dict(window=8), dict(bin_e=14, buf_len=16384, downsample=4, downsample_passes=2, boxcar=0),
                dict(bin_e=5, buf_len=16384, downsample=16384, boxcar=1)):
        cfg = RtlpowerCfg.default(**bad)
        assert lib.rtlpower_cfg_validate(C.byref(cfg)) < 0, bad
        assert lib.rtlpower_scan_route(C.byref(cfg), 4, 3, 3 * int(cfg.buf_len), 0, C.byref(o)) < 0, bad
        with pytest.raises(capi.RtlfmError):
            scan_route(cfg, 4, 3)
    cfg = RtlpowerCfg.default()
    assert lib.rtlpower_scan_route(C.byref(cfg), 4, 3, 3 * 16384 - 4, 0, None) == -22  # rows shorter than their reads
    assert lib.rtlpower_scan_route(C.byref(cfg), 0, 3, 3 * 16384, 0, None) == -22
    assert lib.rtlpower_scan_route(C.byref(cfg), 4, 0, 3 * 16384, 0, None) == -22
    assert lib.rtlpower_scan_route(None, 4, 3, 3 * 16384, 0, None) == -22


def test_route_check_under_the_sanitizers(tmp_path):
    """tools/route_check.cpp with the unit that holds plan_scan, host code under AddressSanitizer + UBSan, over the rows
    above and over its own sweep of configurations, strides and options."""
    exe = str(tmp_path / "route_check")
    subprocess.check_call([hipbuild._hipcc(), f"--offload-arch={hipbuild.ARCH}", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe, os.path.join(hipbuild.CSRC, "rtlpower_hip.hip"),
                           os.path.join(ROOT, "tools", "route_check.cpp")])
    lines = []
    for r in ROWS:
        cfg, o = RtlpowerCfg.default(**r["kw"]), RtlpowerRouteOpts.default(**r["opts"])
        fields = [getattr(cfg, n) for n, _ in cfg._fields_] + [r["ns"], r["nr"], r["nr"] * int(cfg.buf_len) + r["pad"], r["addr"]]
        fields += [getattr(o, n) for n, _ in o._fields_] + [r["want"]]
        lines.append(" ".join(str(int(v)) for v in fields))
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stdout.startswith(f"route_check: ok, {len(ROWS)} rows"), p.stdout
