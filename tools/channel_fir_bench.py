#!/usr/bin/env python3
"""The channel filter at scale: tools/channel_bench.py's shape - 64 sources x 64 channels = 4096 streams, 4 x 262144 B per
source and step, low_pass /10's place, -A fast - with a filter set (include/rtlfm_hip.h, rtlfm_gpu_set_channel_filter).

Timed in ONE session on one GPU, alternating, after a warm-up of each:
  boxcar       no filter: k_channel_boxcar + the back half (the yardstick the filter replaces)
  fir<N>_p2    N = 4 D and 8 D taps of rtlfm_channel_lowpass(N, 0.4 / D, D) on path 2: k_channel_fir, one launch
  fir<N>_p1    the same on path 1: k_channel_mix over the history's end and the run, k_channel_fir_plain, k_source_history
each as the front end alone (the handle's event timing) and as the whole step (host clock around --steps runs that end in
a synchronise).  The outputs of the two paths are compared for every N (they must be equal).  Prints one JSON line.
"""
import argparse
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
    ap.add_argument("--downsample", type=int, default=10)
    ap.add_argument("--taps", type=int, nargs="*", default=None, help="filter lengths (default: 4 D and 8 D)")
    ap.add_argument("--steps", type=int, default=20, help="runs per timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per variant, alternating")
    ap.add_argument("--no-path1", action="store_true", help="skip path 1 (a capture-rate work buffer: 8.6 GB at the default shape)")
    a = ap.parse_args()

    import torch

    from rtlsdr_amd import build as hipbuild
    from rtlsdr_amd.capi import ATAN_FAST, RtlfmCfg
    from rtlsdr_amd.demod import GpuDemod, channel_lowpass
    hipbuild.build()
    if not torch.cuda.is_available():
        sys.exit("channel_fir_bench: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    dev = torch.device("cuda", 0)
    S = a.sources * a.per_source
    L, NB, D = a.block_len, a.blocks, a.downsample
    lengths = a.taps or [4 * D, 8 * D]
    cfg = RtlfmCfg.default(downsample=D, custom_atan=ATAN_FAST, rate_out=2400000 // D, block_len=L, max_blocks=NB)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20261019)
    src = torch.randint(38, 217, (a.sources, NB * L), dtype=torch.uint8, device=dev, generator=gen)
    rng = np.random.default_rng(1)
    steps = rng.integers(0, 1 << 32, size=S, dtype=np.uint64).astype(np.uint32)

    chan = GpuDemod(cfg, S, 0)
    chan.set_channels(a.per_source, steps=steps)
    out = torch.empty((S, chan.result_cap(NB)), dtype=torch.int16, device=dev)
    out_len = torch.zeros(S, dtype=torch.int32, device=dev)
    filters = {n: channel_lowpass(n, 0.4 / D, D) for n in lengths}
    current = [None]

    def select(ntaps, path):
        """(set_channel_filter waits for the handle and clears the history: only when the filter really changes)"""
        if current[0] != ntaps:
            if ntaps:
                chan.set_channel_filter(*filters[ntaps])
            else:
                chan.set_channel_filter(None)
            current[0] = ntaps
        chan.set_path(path)
        chan.channels_seek(0)

    def window(n, front=False):
        if front:
            chan.timing_enable(True)
            chan.timing_read()
        chan.sync()
        t0 = time.perf_counter()
        for _ in range(n):
            chan.run_device(src.data_ptr(), src.stride(0), NB, out.data_ptr(), out.stride(0), out_len.data_ptr())
        chan.sync()
        ms = (time.perf_counter() - t0) * 1e3 / n
        fms = None
        if front:
            tot, k = chan.timing_read()
            chan.timing_enable(False)
            fms = tot / max(1, k)
        return ms, fms

    def variant(ntaps, path):
        def f(n, front=False):
            select(ntaps, path)
            r = window(n, front)
            assert chan.last_path == (1 if path == 1 else 2)
            return r
        return f

    variants = {"boxcar": variant(0, 0)}
    for n in lengths:
        variants[f"fir{n}_p2"] = variant(n, 0)
        if not a.no_path1:
            variants[f"fir{n}_p1"] = variant(n, 1)

    # the same input from the same state through both paths: equal, or the timing compares two different things
    equal = {}
    if not a.no_path1:
        for n in lengths:
            chan.reset(); variants[f"fir{n}_p2"](1); a_out, a_len = out.clone(), out_len.clone()
            chan.reset(); variants[f"fir{n}_p1"](1)
            equal[str(n)] = bool(torch.equal(a_len, out_len)) and all(
                bool(torch.equal(a_out[s, :int(a_len[s])], out[s, :int(a_len[s])])) for s in range(0, S, max(1, S // 64)))
        chan.reset()

    for f in variants.values():
        f(a.warmup)
    res = {k: dict(step_ms=[], front_ms=[]) for k in variants}
    for _ in range(a.repeats):
        for k, f in variants.items():
            ms, _ = f(a.steps)
            res[k]["step_ms"].append(ms)
        for k, f in variants.items():  # the event pairs cost a little: the front end in windows of its own
            _, fms = f(a.steps, True)
            res[k]["front_ms"].append(fms)
    samples = S * NB * (L // 2)
    line = {
        "tool": "channel_fir_bench", "gpu": torch.cuda.get_device_name(0), "sources": a.sources, "per_source": a.per_source,
        "streams": S, "blocks": NB, "block_len": L, "downsample": D, "steps": a.steps, "repeats": a.repeats,
        "paths_equal": equal, "stream_samples_per_step": samples,
    }
    for k, r in res.items():
        med = float(np.median(r["step_ms"]))
        line[k] = dict(step_ms=med, step_ms_min=float(min(r["step_ms"])), step_ms_max=float(max(r["step_ms"])),
                       front_ms=float(np.median(r["front_ms"])), gsamples_per_s=samples / med / 1e6)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
