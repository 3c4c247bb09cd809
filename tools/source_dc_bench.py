#!/usr/bin/env python3
"""What the option source_dc costs, in tools/channel_bank_bench.py's shape: 64 sources x 64 channels, 4 x 262144 B per source
and step, -A fast.  Front ends:
  boxcar10     k_channel_boxcar at / 10
  fir80        k_channel_fir with 80 taps of rtlfm_channel_lowpass(80, 0.4 / 10, 10) at / 10
  bank64_10    k_channel_bank at K = 64, 512 taps, / 10
  bank64_32    the same at / 32

Timed in ONE session on one GPU and, per front end, on ONE handle, the option alternating 0 / 1 window by window after a
warm-up of each: the front end's timed pair (HIP events; with the option on the pre-pass rides inside it) and the whole
step by the host clock.  The pre-pass alone - the sums over the source rows and k_source_dc_smooth, two launches - is timed
as a pair of its own through rtlfm_gpu_source_dc_prepass.  Prints one JSON line.
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
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--block-len", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=10, help="runs per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per variant, alternating")
    a = ap.parse_args()

    import torch

    from rtlsdr_amd import build as hipbuild
    from rtlsdr_amd.capi import ATAN_FAST, RtlfmCfg, check
    from rtlsdr_amd.demod import GpuDemod, channel_lowpass
    hipbuild.build()
    if not torch.cuda.is_available():
        sys.exit("source_dc_bench: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    dev = torch.device("cuda", 0)
    nsrc, per, L, NB = a.sources, a.channels, a.block_len, a.blocks
    gen = torch.Generator(device=dev)
    gen.manual_seed(20261021)
    src = torch.randint(38, 217, (nsrc, NB * L), dtype=torch.uint8, device=dev, generator=gen)
    line = {"tool": "source_dc_bench", "gpu": torch.cuda.get_device_name(0), "sources": nsrc, "channels": per, "blocks": NB,
            "block_len": L, "steps": a.steps, "repeats": a.repeats}
    rng = np.random.default_rng(1)
    steps = rng.integers(0, 1 << 32, size=nsrc * per, dtype=np.uint64).astype(np.uint32)

    def front(g, name, D):
        if name == "fir80":
            g.set_channel_filter(*channel_lowpass(80, 0.4 / D, D))
        if name.startswith("bank"):
            taps, shift = channel_lowpass(512, 0.4 / per, D)
            g.set_channel_bank(per, taps, shift - (per.bit_length() - 1))

    for name, D in (("boxcar10", 10), ("fir80", 10), ("bank64_10", 10), ("bank64_32", 32)):
        cfg = RtlfmCfg.default(downsample=D, custom_atan=ATAN_FAST, rate_out=2400000 // D, block_len=L, max_blocks=NB)
        g = GpuDemod(cfg, nsrc * per, 0)
        g.set_channels(per, steps=steps)
        front(g, name, D)
        out = torch.empty((g.nstreams, g.result_cap(cfg.max_blocks)), dtype=torch.int16, device=dev)
        out_len = torch.zeros(g.nstreams, dtype=torch.int32, device=dev)

        def run():
            g.run_device(src.data_ptr(), src.stride(0), NB, out.data_ptr(), out.stride(0), out_len.data_ptr())

        def prepass():
            check(g.lib.rtlfm_gpu_source_dc_prepass(g._h, src.data_ptr(), src.stride(0), NB), "rtlfm_gpu_source_dc_prepass")

        def window(fn, n, timed):
            if timed:
                g.timing_enable(True)
                g.timing_read()
            g.sync()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            g.sync()
            ms = (time.perf_counter() - t0) * 1e3 / n
            fms = None
            if timed:
                tot, k = g.timing_read()
                g.timing_enable(False)
                fms = tot / max(1, k)
            return ms, fms

        def variant(on, fn=run):
            def f(n, timed=False):
                if g.get_option("source_dc") != on:
                    g.set_option("source_dc", on)  # (outside the window: it waits for the handle and clears the history)
                return window(fn, n, timed)
            return f

        variants = {"off": variant(0), "on": variant(1)}
        for f in variants.values():
            f(a.warmup)
        res = {k: dict(step_ms=[], front_ms=[]) for k in variants}
        pre = []
        for _ in range(a.repeats):
            for k, f in variants.items():
                res[k]["step_ms"].append(f(a.steps)[0])
            for k, f in variants.items():  # the event pairs cost a little: the front end in windows of its own
                res[k]["front_ms"].append(f(a.steps, True)[1])
            pre.append(variant(1, prepass)(a.steps, True)[1])
        leg = {}
        for k, r in res.items():
            leg[k] = dict(step_ms=float(np.median(r["step_ms"])), step_ms_min=float(min(r["step_ms"])), step_ms_max=float(max(r["step_ms"])),
                          front_ms=float(np.median(r["front_ms"])), front_ms_min=float(min(r["front_ms"])),
                          front_ms_max=float(max(r["front_ms"])))
        leg["prepass_ms"] = dict(median=float(np.median(pre)), min=float(min(pre)), max=float(max(pre)))
        leg["front_on_minus_off_ms"] = leg["on"]["front_ms"] - leg["off"]["front_ms"]
        leg["front_on_over_off"] = leg["on"]["front_ms"] / leg["off"]["front_ms"]
        line[name] = leg
        g.close()
        del out, out_len
        torch.cuda.empty_cache()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
