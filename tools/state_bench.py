#!/usr/bin/env python3
"""What moving the carried state of many streams costs, one stream at a time and all at once.  A tool, not a test.

    python tools/state_bench.py [--rounds 5]

On handles of 256 and 4096 streams (the shape does not matter: a record is 328 bytes whatever the configuration), wall
time per call after warm-up, the handle idle before and after, alternating round by round in one session:
    loop     rtlfm_gpu_state_get + rtlfm_gpu_state_set for every stream        (a): all there was before
    bulk     rtlfm_gpu_state_get_all + rtlfm_gpu_state_set_all                 (b)
    move     one rtlfm_gpu_state_move in place (the identity map)              (c)
and what the tool's shrink() does when half of the sources have ended - a new handle of S / 2 streams exists already in
both forms, so that only the regroup is timed:
    shrink_old   state_get from the old + state_set into the new handle for every staying stream
    shrink_new   one rtlfm_gpu_state_move with map = every second stream
One JSON line per stream count with the medians of the rounds in microseconds and loop / bulk, loop / move.
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
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("state_bench.py measures on a GPU; there is none here")
    from rtlsdr_amd import capi
    from rtlsdr_amd.capi import RtlfmCfg
    from rtlsdr_amd.demod import GpuDemod
    cfg = RtlfmCfg.default(block_len=2048, max_blocks=1, downsample=7, custom_atan=capi.ATAN_FAST)
    for S in (256, 4096):
        with GpuDemod(cfg, S) as g, GpuDemod(cfg, S // 2) as half:
            ident = np.arange(S, dtype=np.int32)
            every_second = np.arange(0, S, 2, dtype=np.int32)
            st = capi.RtlfmStreamState()

            def loop():
                for s in range(S):
                    g.lib.rtlfm_gpu_state_get(g._h, s, C.byref(st))
                    g.lib.rtlfm_gpu_state_set(g._h, s, C.byref(st))

            def bulk():
                g.state_set_all(g.state_get_all())

            def move():
                g.move_from(g, ident)

            def shrink_old():
                for k, s in enumerate(every_second):
                    g.lib.rtlfm_gpu_state_get(g._h, int(s), C.byref(st))
                    half.lib.rtlfm_gpu_state_set(half._h, k, C.byref(st))

            def shrink_new():
                half.move_from(g, every_second)

            forms = {"loop": loop, "bulk": bulk, "move": move, "shrink_old": shrink_old, "shrink_new": shrink_new}

            def timed(fn):
                g.sync()
                half.sync()
                t0 = time.perf_counter()
                fn()
                return (time.perf_counter() - t0) * 1e6
            for fn in (bulk, move, shrink_new):  # warm-up: first calls allocate (the map's device array)
                fn()
            res = {k: [] for k in forms}
            for _ in range(a.rounds):
                for k, fn in forms.items():
                    res[k].append(timed(fn))
            med = {k: statistics.median(v) for k, v in res.items()}
            print(json.dumps({"streams": S, **{k + "_us": round(v, 1) for k, v in med.items()},
                              "loop_over_bulk": round(med["loop"] / med["bulk"], 1), "loop_over_move": round(med["loop"] / med["move"], 1),
                              "shrink_old_over_new": round(med["shrink_old"] / med["shrink_new"], 1),
                              "all_us": {k: [round(x, 1) for x in v] for k, v in res.items()}}))


if __name__ == "__main__":
    main()
