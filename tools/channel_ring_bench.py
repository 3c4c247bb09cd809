#!/usr/bin/env python3
"""The channelizer through the callback boundary: 64 sources x 64 channels = 4096 streams, 4 x 262144 B per source and
step, config c1's chain (low_pass /10, -A fast) behind k_channel_boxcar, fed over the source-indexed ring (option
source_ring; include/rtlfm_hip.h, "The ring and channels").

Timed in ONE session on one GPU, alternating, after a warm-up of each:
  ring     the steady state of rtlfm_gpu_push x (sources x blocks) -> rtlfm_gpu_run -> rtlfm_gpu_fetch_all_prev into
           pinned host rows: the whole step by the host clock, and its three parts (push, run, fetch) each by the host
           clock around its calls - run only queues work, so the parts say where the HOST waits, not what the device does
  device   the same handle through rtlfm_gpu_run_device on input that already lies in device memory, results left there
  h2d      one step's input (sources x blocks x block_len bytes) from pinned host memory to the device, alone
  d2h      one step's results (streams rows of PCM) from the device to pinned host memory, alone
Prints one JSON line.  There is no pass mark: the figures say what bounds the step."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sources", type=int, default=64)
    ap.add_argument("--per-source", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--block-len", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=20, help="runs per timed window")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3, help="timed windows per variant, alternating")
    a = ap.parse_args()

    import torch

    from rtlsdr_amd import build as hipbuild
    from rtlsdr_amd.capi import ATAN_FAST, RtlfmCfg, check
    from rtlsdr_amd.demod import GpuDemod
    hipbuild.build()
    if not torch.cuda.is_available():
        sys.exit("channel_ring_bench: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    dev = torch.device("cuda", 0)
    nsrc, per = a.sources, a.per_source
    S = nsrc * per
    L, NB = a.block_len, a.blocks
    cfg = RtlfmCfg.default(downsample=10, custom_atan=ATAN_FAST, rate_out=240000, block_len=L, max_blocks=NB)
    rng = np.random.default_rng(20261020)
    host_in = torch.from_numpy(rng.integers(38, 217, size=(nsrc, NB * L), dtype=np.uint8)).pin_memory()
    src = host_in.numpy()
    steps = rng.integers(0, 1 << 32, size=S, dtype=np.uint64).astype(np.uint32)

    g = GpuDemod(cfg, S, 0, options=dict(source_ring=1))
    g.set_channels(per, steps=steps)
    assert g.sources == nsrc
    lib, h = g.lib, g._h
    cap = lib.rtlfm_result_cap(C.byref(cfg)) * NB + 16
    host_out = torch.empty((S, cap), dtype=torch.int16).pin_memory()
    lens = np.zeros(S, dtype=np.int32)
    d_in = host_in.to(dev)
    d_out = torch.empty((S, g.result_cap(NB)), dtype=torch.int16, device=dev)
    d_len = torch.zeros(S, dtype=torch.int32, device=dev)
    ptrs = [[src[i, j * L:(j + 1) * L].ctypes.data for j in range(NB)] for i in range(nsrc)]

    def ring(n):
        """n steady-state steps (one run is in flight when the window opens): ms per step - whole, push, run, fetch."""
        for i in range(nsrc):
            for p in ptrs[i]:
                check(lib.rtlfm_gpu_push(h, i, p, L), "push")
        check(lib.rtlfm_gpu_run(h), "run")
        g.sync()
        tp = tr = tf = 0.0
        t00 = time.perf_counter()
        for _ in range(n):
            t0 = time.perf_counter()
            for i in range(nsrc):
                for p in ptrs[i]:
                    check(lib.rtlfm_gpu_push(h, i, p, L), "push")
            t1 = time.perf_counter()
            check(lib.rtlfm_gpu_run(h), "run")
            t2 = time.perf_counter()
            check(lib.rtlfm_gpu_fetch_all_prev(h, host_out.data_ptr(), cap, lens.ctypes.data), "fetch_all_prev")
            t3 = time.perf_counter()
            tp += t1 - t0
            tr += t2 - t1
            tf += t3 - t2
        whole = time.perf_counter() - t00
        g.sync()
        return dict(step_ms=whole * 1e3 / n, push_ms=tp * 1e3 / n, run_ms=tr * 1e3 / n, fetch_ms=tf * 1e3 / n)

    def device(n):
        g.sync()
        t0 = time.perf_counter()
        for _ in range(n):
            g.run_device(d_in.data_ptr(), d_in.stride(0), NB, d_out.data_ptr(), d_out.stride(0), d_len.data_ptr())
        g.sync()
        return dict(step_ms=(time.perf_counter() - t0) * 1e3 / n)

    def h2d(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            d_in.copy_(host_in, non_blocking=True)
        torch.cuda.synchronize()
        return dict(step_ms=(time.perf_counter() - t0) * 1e3 / n)

    def d2h(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            host_out.copy_(d_out[:, :cap], non_blocking=True)
        torch.cuda.synchronize()
        return dict(step_ms=(time.perf_counter() - t0) * 1e3 / n)

    variants = dict(ring=ring, device=device, h2d=h2d, d2h=d2h)
    for f in variants.values():
        f(a.warmup)
    assert g.last_path == 2
    mx = int(lens.max())
    res = {k: [] for k in variants}
    for _ in range(a.repeats):
        for k, f in variants.items():
            res[k].append(f(a.steps))
    out = dict(tool="channel_ring_bench", gpu=torch.cuda.get_device_name(0), sources=nsrc, per_source=per, streams=S, blocks=NB,
               block_len=L, steps=a.steps, repeats=a.repeats, input_bytes_per_step=nsrc * NB * L,
               result_bytes_per_step=S * mx * 2, pinned_input_bytes=2 * nsrc * NB * L,
               stream_samples_per_step=S * NB * (L // 2))
    for k, rows in res.items():
        med = {name: float(np.median([r[name] for r in rows])) for name in rows[0]}
        med["step_ms_min"] = float(min(r["step_ms"] for r in rows))
        med["step_ms_max"] = float(max(r["step_ms"] for r in rows))
        out[k] = med
    out["ring"]["gsamples_per_s"] = out["stream_samples_per_step"] / out["ring"]["step_ms"] / 1e6
    out["device"]["gsamples_per_s"] = out["stream_samples_per_step"] / out["device"]["step_ms"] / 1e6
    out["h2d"]["gbytes_per_s"] = out["input_bytes_per_step"] / out["h2d"]["step_ms"] / 1e6
    out["d2h"]["gbytes_per_s"] = S * cap * 2 / out["d2h"]["step_ms"] / 1e6
    g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
