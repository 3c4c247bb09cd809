#!/usr/bin/env python3
"""What regrouping a handle with channels on costs: on the device in one launch, and through the host.  A tool, not a test.

    python tools/channel_move_bench.py [--rounds 7] [--sources 64] [--per 64]

One handle of 64 sources x 64 channels (4096 streams; 1.3 MB of records, 0.5 MB of history) with a 33-tap channel filter
set, so that a history is carried.  Wall time per call after warm-up, the handle idle before and after, the forms
alternating round by round in one session:
    move     one rtlfm_gpu_channels_move in place, the sources reversed            (k_source_move: records, history, pos)
    host     the same regroup through the host: rtlfm_gpu_state_get_all + rtlfm_gpu_channels_history_get, the permutation
             in numpy, rtlfm_gpu_state_set_all + rtlfm_gpu_channels_history_set    (the route between devices)
and, with the option source_dc on (the bias words travel too), the same two again.  One JSON line per setting with the
medians of the rounds in microseconds and host / move; every round's figures beside them.
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sources", type=int, default=64)
    ap.add_argument("--per", type=int, default=64)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("channel_move_bench.py measures on a GPU; there is none here")
    from rtlsdr_amd import capi
    from rtlsdr_amd.capi import RtlfmCfg, RtlfmStreamState
    from rtlsdr_amd.demod import GpuDemod, channel_lowpass
    nsrc, per = a.sources, a.per
    S = nsrc * per
    cfg = RtlfmCfg.default(block_len=2048, max_blocks=1, downsample=10, custom_atan=capi.ATAN_FAST, rate_out=240000)
    taps, shift = channel_lowpass(33, 0.04, 1)
    rec = C.sizeof(RtlfmStreamState)
    for dc in (0, 1):
        with GpuDemod(cfg, S) as g:
            g.set_channels(per, steps=np.arange(S, dtype=np.uint32) * 12345)
            g.set_channel_filter(taps, shift)
            g.set_option("source_dc", dc)
            # one run, so that what moves is not all silence
            iq = torch.randint(0, 256, (nsrc, 2048), dtype=torch.uint8, device="cuda")
            g.run_torch(iq)
            g.sync()
            rev = np.arange(nsrc - 1, -1, -1, dtype=np.int32)

            def move():
                g.channels_move_from(g, rev)

            def host():
                st = np.frombuffer(g.state_get_all(), dtype=np.uint8).reshape(nsrc, per * rec)
                hist, words = g.channels_history()
                g.set_channels_history(hist[rev], None if words is None else words[rev])
                moved = np.ascontiguousarray(st[rev])  # (held in a name: the call below gets its address only)
                g.lib.rtlfm_gpu_state_set_all(g._h, moved.ctypes.data, S)

            forms = {"move": move, "host": host}

            def timed(fn):
                g.sync()
                t0 = time.perf_counter()
                fn()
                return (time.perf_counter() - t0) * 1e6
            # both forms undo each other in pairs: after an even number of calls the handle is where it was
            before = bytes(g.state_get_all()), g.channels_history()[0].tobytes()
            for fn in (move, host):  # warm-up: the first move allocates the map's device array
                fn()
            assert (bytes(g.state_get_all()), g.channels_history()[0].tobytes()) == before, "move and host disagree"
            res = {k: [] for k in forms}
            for _ in range(a.rounds):
                for k, fn in forms.items():
                    res[k].append(timed(fn))
            med = {k: statistics.median(v) for k, v in res.items()}
            print(json.dumps({"sources": nsrc, "per_source": per, "streams": S, "source_dc": dc, "record_bytes": S * rec, "history_bytes": nsrc * 8192,
                              **{k + "_us": round(v, 1) for k, v in med.items()}, "host_over_move": round(med["host"] / med["move"], 1),
                              "all_us": {k: [round(x, 1) for x in v] for k, v in res.items()}}))


if __name__ == "__main__":
    main()
