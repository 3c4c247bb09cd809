#!/usr/bin/env python3
"""What the options source_stats / source_health cost, in tools/channel_bench.py's shape: 4 x 262144 B per source and
step, / 10, -A fast, the boxcar front end.  Two shapes:
  64 sources x 64 channels     the front end is bound by its 4096 streams: a read of the source rows is noise
  1024 sources x 4 channels    the front end is bound by the source bytes: every extra read of them is a share of the step

Variants, all on ONE handle per shape in ONE process, alternating window by window after a warm-up of each:
  off            nothing on
  dc             source_dc alone (k_rdc_sums_wide + k_source_dc_smooth in front of the front end)
  dc_rec         source_dc + both record options: k_source_prepass, one read of the source rows for all of it
  rec            both record options without source_dc (k_input_health with the statistics)
(The A/B of LAB.md had a sixth, source_dc + the records as two launches - k_rdc_sums_wide, then k_input_health - behind an
internal option; it lost at 1024 x 4 and went with the option.)

Timed: the front end's timed pair (HIP events; the pre-pass and the readers ride inside it) and the whole step by the host
clock.  Prints one JSON line: per variant the median over the repeats and their spread (min, max).
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
    ap.add_argument("--shapes", default="64x64,1024x4", help="sources x channels, comma separated")
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--block-len", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=10, help="runs per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per variant, alternating")
    a = ap.parse_args()

    import torch

    from rtlsdr_amd import build as hipbuild
    from rtlsdr_amd.capi import ATAN_FAST, RtlfmCfg
    from rtlsdr_amd.demod import GpuDemod
    hipbuild.build()
    if not torch.cuda.is_available():
        sys.exit("source_health_bench: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    dev = torch.device("cuda", 0)
    L, NB, D = a.block_len, a.blocks, 10
    line = {"tool": "source_health_bench", "gpu": torch.cuda.get_device_name(0), "blocks": NB, "block_len": L, "steps": a.steps,
            "repeats": a.repeats}
    variants = {"off": (0, 0), "dc": (1, 0), "dc_rec": (1, 1), "rec": (0, 1)}  # (source_dc, records)
    for shape in a.shapes.split(","):
        nsrc, per = (int(v) for v in shape.split("x"))
        gen = torch.Generator(device=dev)
        gen.manual_seed(20261021)
        src = torch.randint(38, 217, (nsrc, NB * L), dtype=torch.uint8, device=dev, generator=gen)
        steps = np.random.default_rng(1).integers(0, 1 << 32, size=nsrc * per, dtype=np.uint64).astype(np.uint32)
        cfg = RtlfmCfg.default(downsample=D, custom_atan=ATAN_FAST, rate_out=2400000 // D, block_len=L, max_blocks=NB)
        g = GpuDemod(cfg, nsrc * per, 0)
        g.set_channels(per, steps=steps)
        out = torch.empty((g.nstreams, g.result_cap(cfg.max_blocks)), dtype=torch.int16, device=dev)
        out_len = torch.zeros(g.nstreams, dtype=torch.int32, device=dev)

        def window(n, timed):
            if timed:
                g.timing_enable(True)
                g.timing_read()
            g.sync()
            t0 = time.perf_counter()
            for _ in range(n):
                g.run_device(src.data_ptr(), src.stride(0), NB, out.data_ptr(), out.stride(0), out_len.data_ptr())
            g.sync()
            ms = (time.perf_counter() - t0) * 1e3 / n
            fms = None
            if timed:
                tot, k = g.timing_read()
                g.timing_enable(False)
                fms = tot / max(1, k)
            return ms, fms

        def select(dc, rec):
            # (outside the window: source_dc waits for the handle and clears the history)
            for name, v in (("source_dc", dc), ("source_stats", rec), ("source_health", rec)):
                if g.get_option(name) != v:
                    g.set_option(name, v)

        for v in variants.values():
            select(*v)
            window(a.warmup, False)
        res = {k: dict(step_ms=[], front_ms=[]) for k in variants}
        for _ in range(a.repeats):
            for k, v in variants.items():
                select(*v)
                res[k]["step_ms"].append(window(a.steps, False)[0])
            for k, v in variants.items():  # the event pairs cost a little: the front end in windows of its own
                select(*v)
                res[k]["front_ms"].append(window(a.steps, True)[1])
        leg = {}
        for k, r in res.items():
            leg[k] = {m: dict(median=float(np.median(r[m])), min=float(min(r[m])), max=float(max(r[m]))) for m in ("step_ms", "front_ms")}
        line[shape] = leg
        g.close()
        del out, out_len, src
        torch.cuda.empty_cache()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
