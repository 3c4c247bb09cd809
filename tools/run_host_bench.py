#!/usr/bin/env python3
"""Host time of a run where the device has next to nothing to do (LAB.md I.53): what rtlfm_gpu_run_device costs the
calling thread per call - the plan, the launches - on a few routes, and a ring run of short buffers (push, run, fetch:
every range of streams a view that plans for itself).  (GPU box)

    python tools/run_host_bench.py [--calls 2000] [--repeat 3]

Prints one line per shape: microseconds per call, `repeat` times (the device is waited for every 50 calls, outside the
clock only at the end: the queue never runs dry, so this is enqueue time)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtlsdr_amd import synth  # noqa: E402
from rtlsdr_amd.capi import ATAN_FAST, RtlfmCfg  # noqa: E402
from rtlsdr_amd.demod import GpuDemod  # noqa: E402

S, L = 8, 16384
SHAPES = [
    ("k_fused p4", dict(downsample=16, downsample_passes=4), 0, 0),
    ("k_fused p4 squelch", dict(downsample=16, downsample_passes=4, squelch_level=50), 0, 0),
    ("k_fused emit p7 + k_deep_rest", dict(downsample=128, downsample_passes=7), 0, 0),
    ("k_boxcar_scan /6 + wbfm tail", dict(downsample=6, deemph=1, deemph_a=13, rate_out=170000, rate_out2=32000), 0, 0),
    ("staged p4 (path 1)", dict(downsample=16, downsample_passes=4), 1, 0),
    ("k_channel_boxcar /8, 4 x 2", dict(downsample=8), 0, 2),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    iq = synth.fm_iq_u8_torch(S, L // 2, dev, fs=1.024e6, dev_hz=3e3)
    for name, ov, path, per in SHAPES:
        cfg = RtlfmCfg.default(block_len=L, max_blocks=1, custom_atan=ATAN_FAST, **ov)
        with GpuDemod(cfg, S, 0, options=dict(apart_budget_gb=0)) as g:
            g.set_path(path)
            if per:
                g.set_channels(per, steps=[1000 * k for k in range(S)])
            rows = iq[:S // per] if per else iq
            out = torch.empty((S, g.result_cap(1)), dtype=torch.int16, device=dev)
            n = torch.zeros(S, dtype=torch.int32, device=dev)

            def burst(k):
                t = 0.0
                for b0 in range(0, k, 50):
                    t0 = time.perf_counter()
                    for _ in range(min(50, k - b0)):
                        g.run_device(rows.data_ptr(), rows.stride(0), 1, out.data_ptr(), out.stride(0), n.data_ptr())
                    t += time.perf_counter() - t0
                    g.sync()
                return t * 1e6 / k
            burst(200)
            print(f"{name:34s} " + " ".join(f"{burst(a.calls):7.2f}" for _ in range(a.repeat)) + " us per rtlfm_gpu_run_device", flush=True)
    # the ring, buffers of two lengths: two views per run
    cfg = RtlfmCfg.default(block_len=L, max_blocks=1, custom_atan=ATAN_FAST, downsample=16, downsample_passes=4)
    host = iq.cpu().numpy()
    with GpuDemod(cfg, S, 0, options=dict(apart_budget_gb=0)) as g:
        def cycle(k):
            t0 = time.perf_counter()
            for _ in range(k):
                for s in range(S):
                    g.push(host[s, :L // 2 if s >= S // 2 else L], s)
                g.run()
                g.fetch_all()
            return (time.perf_counter() - t0) * 1e6 / k
        cycle(50)
        print(f"{'ring, 8 streams, 16384 / 8192 B':34s} " + " ".join(f"{cycle(a.calls // 10):7.2f}" for _ in range(a.repeat)) + " us per push x 8, run, fetch_all",
              flush=True)


if __name__ == "__main__":
    main()
