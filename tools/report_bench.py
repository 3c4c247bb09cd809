#!/usr/bin/env python3
"""What one rtl_power report costs: rtlpower_gpu_report against the path it replaces.  A tool, not a test.

    python tools/report_bench.py [--rounds 5] [--shapes 1024x14,4096x10] [--out FILE]

For every shape (streams x 2^bin_e bins; 1024 x 2^14 is BASELINE configs[3]'s) the handle scans one read of noise per
stream, then ONE report is timed on a host clock, from the call to the point named, three legs alternating round by
round in the same process:

    old      rtlpower_gpu_fetch + rtlpower_csv_dbm for every stream, then rtlpower_gpu_clear and a synchronise
             (what rtl_power_hip does without -N)
    values   rtlpower_gpu_report(clear = 1) + rtlpower_gpu_report_fetch_all: every value in host memory
    lines    the same, then rtlpower_csv_report for every stream: every CSV line in host memory

The scan in front of each leg is not timed (every leg starts synchronised, on the same accumulators: a report resets
them).  Prints one JSON line: per shape and leg the median / min / max in ms, the bins the report left to the host, and
whether the lines of `old` and `lines` were the same bytes.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bench_shape(streams, bin_e, rounds):
    import numpy as np
    import torch
    from rtlsdr_amd import capi
    from rtlsdr_amd.capi import RtlpowerCfg
    from rtlsdr_amd.power import GpuPower
    lib = capi.load()
    bins = 1 << bin_e
    L = max(16384, 2 << bin_e)
    cfg = RtlpowerCfg.default(bin_e=bin_e, window=1, buf_len=L)
    rate = 2_800_000
    plan = capi.RtlpowerPlan(lower=100_000_000, upper=100_000_000 + rate, max_size=1, tune_count=1, bw_seen=rate, rate=rate,
                             bin_e=bin_e, downsample=1, downsample_passes=0, buf_len=L, crop=0.0, bin_size=rate / bins)
    gen = torch.Generator(device="cuda").manual_seed(7)
    iq = torch.randint(0, 256, (streams, L), dtype=torch.uint8, device="cuda", generator=gen)
    avg = np.zeros(bins, dtype=np.int64)
    samples = C.c_int32()
    line = C.create_string_buffer(bins * 16 + 512)
    width = bins + 1
    centi = np.zeros((streams, width), dtype=np.int32)
    lens = np.zeros(streams, dtype=np.int32)
    nsamp = np.zeros(streams, dtype=np.int32)
    with GpuPower(cfg, streams, 0) as g:
        h = g._h

        def scan():
            g.scan_torch(iq)
            g.sync()
            torch.cuda.synchronize()

        def old(keep=None):
            t0 = time.perf_counter()
            for s in range(streams):
                assert lib.rtlpower_gpu_fetch(h, s, avg.ctypes.data, C.byref(samples)) == 0
                n = lib.rtlpower_csv_dbm(C.byref(plan), 0, avg.ctypes.data, samples.value, line, len(line))
                assert n > 0
                if keep is not None:
                    keep.append(line.raw[:n])
            assert lib.rtlpower_gpu_clear(h) == 0 and lib.rtlpower_gpu_sync(h) == 0
            return (time.perf_counter() - t0) * 1e3

        def new(lines, keep=None):
            t0 = time.perf_counter()
            assert lib.rtlpower_gpu_report(h, float(rate), 0.0, 1) == 0
            assert lib.rtlpower_gpu_report_fetch_all(h, centi.ctypes.data, width, lens.ctypes.data, nsamp.ctypes.data) == 0
            if lines:
                for s in range(streams):
                    n = lib.rtlpower_csv_report(C.byref(plan), 0, centi[s].ctypes.data, int(lens[s]), int(nsamp[s]), line, len(line))
                    assert n > 0
                    if keep is not None:
                        keep.append(line.raw[:n])
            return (time.perf_counter() - t0) * 1e3

        # warm-up of every leg (the first report allocates its device and pinned blocks), and the bytes compared once
        a, b = [], []
        scan(); old(a)
        scan(); new(True, b)
        scan(); new(False)
        same = a == b
        ms = {"old": [], "values": [], "lines": []}
        doubts = []
        for _ in range(rounds):
            scan(); ms["old"].append(old())
            scan(); ms["values"].append(new(False)); doubts.append(g.report_doubts)
            scan(); ms["lines"].append(new(True))
    res = {"streams": streams, "bins": bins, "values_per_report": streams * width, "lines_identical": same, "doubts": doubts}
    for k, v in ms.items():
        res[k] = {"ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)}
    res["old_over_values"] = round(res["old"]["ms_median"] / res["values"]["ms_median"], 2)
    res["old_over_lines"] = round(res["old"]["ms_median"] / res["lines"]["ms_median"], 2)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="1024x14,4096x10")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("report_bench.py measures on a GPU; there is none here")
    res = {"tool": "report_bench", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "shapes": []}
    for sh in a.shapes.split(","):
        s, e = sh.split("x")
        res["shapes"].append(bench_shape(int(s), int(e), a.rounds))
    text = json.dumps(res)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
