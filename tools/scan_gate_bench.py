#!/usr/bin/env python3
"""What the scanner's squelch gate (k_scan_gate, option "squelch_gate") costs, next to what it replaces.  A tool, not a test.

    python tools/scan_gate_bench.py [--rounds 5 --runs 20]

On the scanner shape -M fm -s 12k -l 50 (a boxcar of 84, 16384-byte buffers), 4096 streams x 1 buffer and 256 streams x 16
buffers, device-resident input, half of the (stream, buffer) pairs a tone and half noise.  Alternating round by round in
one session, wall time per call after warm-up (the device idle before and after):
    off      rtlfm_gpu_run_device with the gate off                                   (a)
    on       the same with the gate on                                                (b)
    records  rtlfm_gpu_gate_all: every stream's records in one copy                   (c)
    loops    rtlfm_gpu_state_get + rtlfm_gpu_state_set for every stream after a run   (d): the tool's way before the gate
and prints one JSON line per shape with the medians in microseconds, on - off and (on - off + records) / loops.
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("scan_gate_bench.py measures on a GPU; there is none here")
    from rtlsdr_amd import capi
    from rtlsdr_amd.capi import RtlfmCfg
    from rtlsdr_amd.demod import GpuDemod, optimal_settings
    L = 16384
    for S, NB in ((4096, 1), (256, 16)):
        cfg = RtlfmCfg.default(block_len=L, max_blocks=NB, squelch_level=50, rate_out=12000)
        optimal_settings(cfg, 100_000_000, 12000)
        rng = np.random.default_rng(1)
        n = L // 2
        ph = 2 * np.pi * 0.254 * np.arange(n)
        tone = np.clip(np.rint(np.stack([127.4 + 100 * np.cos(ph), 127.4 + 100 * np.sin(ph)], axis=1)), 0, 255).astype(np.uint8).ravel()
        iq = (127 + rng.integers(-1, 2, (S, NB, L))).astype(np.uint8)
        iq[rng.random((S, NB)) < 0.5] = tone
        d_iq = torch.from_numpy(iq.reshape(S, NB * L)).cuda()
        handles = {"off": GpuDemod(cfg, S), "on": GpuDemod(cfg, S, squelch_gate=True, conseq_squelch=1)}
        outs = {k: (torch.empty((S, g.result_cap(NB)), dtype=torch.int16, device="cuda"), torch.zeros(S, dtype=torch.int32, device="cuda"))
                for k, g in handles.items()}

        def run(kind):
            g = handles[kind]
            g.run_torch(d_iq, *outs[kind])

        def timed(fn, reps):
            torch.cuda.synchronize()
            for g in handles.values():
                g.sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            for g in handles.values():
                g.sync()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / reps * 1e6

        def loops():
            g = handles["off"]
            st = capi.RtlfmStreamState()
            for s in range(S):
                g.lib.rtlfm_gpu_state_get(g._h, s, C.byref(st))
                if st.squelch_hits > 1:
                    st.squelch_hits = 2
                g.lib.rtlfm_gpu_state_set(g._h, s, C.byref(st))

        for kind in handles:  # warm-up: allocations, first launches
            for _ in range(3):
                run(kind)
        handles["on"].gate()
        res = {k: [] for k in ("off", "on", "records", "loops")}
        for _ in range(a.rounds):
            res["off"].append(timed(lambda: run("off"), a.runs))
            res["on"].append(timed(lambda: run("on"), a.runs))
            res["records"].append(timed(lambda: handles["on"].gate(), a.runs))
            res["loops"].append(timed(loops, 1))
        med = {k: statistics.median(v) for k, v in res.items()}
        held = int((handles["on"].gate()["emit"] == 0).sum())
        print(json.dumps({"streams": S, "buffers": NB, "held_last_run": held, "off_us": round(med["off"], 1), "on_us": round(med["on"], 1),
                          "records_us": round(med["records"], 1), "loops_us": round(med["loops"], 1),
                          "gate_us": round(med["on"] - med["off"], 1),
                          "gate_plus_records_over_loops": round((med["on"] - med["off"] + med["records"]) / med["loops"], 4),
                          "all_us": {k: [round(x, 1) for x in v] for k, v in res.items()}}))
        for g in handles.values():
            g.close()


if __name__ == "__main__":
    main()
