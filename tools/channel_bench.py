#!/usr/bin/env python3
"""Channels at scale: 64 sources x 64 channels = 4096 streams, 4 x 262144 B per source and step, config c1's chain
(low_pass /10, -A fast) behind the NCO front end (include/rtlfm_hip.h, rtlfm_gpu_set_channels).

Three things are timed in ONE session on one GPU, alternating, after a warm-up of each:
  fused    k_channel_boxcar + the back half (rtlfm_gpu_last_path 2): the front-end kernel alone (the handle's event
           timing) and the whole step (host clock around --steps runs that end in a synchronise)
  staged   the same handle forced to path 1: k_channel_mix + k_boxcar + the back half
  c1       the yardstick: the same chain on 4096 INDEPENDENT streams of 4 x 262144 B each (k_boxcar_scan), which reads
           64 times the input bytes and mixes nothing
and the fused and staged outputs are compared (they must be equal).  Prints one JSON line.
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
    ap.add_argument("--steps", type=int, default=50, help="runs per timed window")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per variant, alternating")
    ap.add_argument("--no-yardstick", action="store_true", help="skip c1 (4 GiB of input at the default shape)")
    ap.add_argument("--no-staged", action="store_true", help="skip path 1 (two capture-rate work buffers: 17 GB at the default shape)")
    a = ap.parse_args()

    import torch

    from rtlsdr_amd import build as hipbuild
    from rtlsdr_amd.capi import ATAN_FAST, RtlfmCfg
    from rtlsdr_amd.demod import GpuDemod
    hipbuild.build()
    if not torch.cuda.is_available():
        sys.exit("channel_bench: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    dev = torch.device("cuda", 0)
    S = a.sources * a.per_source
    L, NB = a.block_len, a.blocks
    cfg = RtlfmCfg.default(downsample=10, custom_atan=ATAN_FAST, rate_out=240000, block_len=L, max_blocks=NB)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20261019)
    src = torch.randint(38, 217, (a.sources, NB * L), dtype=torch.uint8, device=dev, generator=gen)
    rng = np.random.default_rng(1)
    steps = rng.integers(0, 1 << 32, size=S, dtype=np.uint64).astype(np.uint32)

    chan = GpuDemod(cfg, S, 0)
    chan.set_channels(a.per_source, steps=steps)
    out = torch.empty((S, chan.result_cap(NB)), dtype=torch.int16, device=dev)
    out_len = torch.zeros(S, dtype=torch.int32, device=dev)

    def window(g, iq, n, front=False):
        """(ms per step by the host clock around n runs and a synchronise, ms per step of the front-end kernel alone)"""
        if front:
            g.timing_enable(True)
            g.timing_read()
        g.sync()
        t0 = time.perf_counter()
        for _ in range(n):
            g.run_device(iq.data_ptr(), iq.stride(0), NB, out.data_ptr(), out.stride(0), out_len.data_ptr())
        g.sync()
        ms = (time.perf_counter() - t0) * 1e3 / n
        fms = None
        if front:
            tot, k = g.timing_read()
            g.timing_enable(False)
            fms = tot / max(1, k)
        return ms, fms

    torch.cuda.synchronize()
    variants = {}

    def fused(n, front=False):
        chan.set_path(0)
        chan.channels_seek(0)
        r = window(chan, src, n, front)
        assert chan.last_path == 2
        return r

    def staged(n, front=False):
        chan.set_path(1)
        chan.channels_seek(0)
        r = window(chan, src, n, front)
        assert chan.last_path == 1
        return r
    variants["fused"] = fused
    if not a.no_staged:
        variants["staged"] = staged
    if not a.no_yardstick:
        plain = GpuDemod(cfg, S, 0)
        iq = torch.randint(0, 256, (S, NB * L), dtype=torch.uint8, device=dev, generator=gen)
        variants["c1"] = lambda n, front=False: window(plain, iq, n, front)

    # the same input from the same state through both channel paths: equal, or the timing compares two different things
    equal = None
    if "staged" in variants:
        chan.reset(); fused(1); a_out, a_len = out.clone(), out_len.clone()
        chan.reset(); staged(1)
        equal = bool(torch.equal(a_len, out_len)) and all(
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
        "tool": "channel_bench", "gpu": torch.cuda.get_device_name(0), "sources": a.sources, "per_source": a.per_source,
        "streams": S, "blocks": NB, "block_len": L, "steps": a.steps, "repeats": a.repeats, "paths_equal": equal,
        "stream_samples_per_step": samples,
    }
    for k, r in res.items():
        med = float(np.median(r["step_ms"]))
        line[k] = dict(step_ms=med, step_ms_min=float(min(r["step_ms"])), step_ms_max=float(max(r["step_ms"])),
                       front_ms=float(np.median(r["front_ms"])), gsamples_per_s=samples / med / 1e6)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
