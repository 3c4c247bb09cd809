#!/usr/bin/env python3
"""What the option source_iq costs, in tools/source_health_bench.py's shape: 4 x 262144 B per source and step, / 10,
-A fast, the boxcar front end.  Two shapes:
  64 sources x 64 channels     the front end is bound by its 4096 streams: k_source_iq moves 128 MiB beside it
  1024 sources x 4 channels    the front end is bound by the source bytes: k_source_iq moves 2 GiB, as much again as it reads

Variants, on ONE handle per shape in ONE process, alternating window by window after a warm-up of each:
  off            the option at 0
  iq             the option at 1 with coefficients near the identity (k_source_iq in front of the front end, which then
                 reads the handle's corrected rows)
Timed: the front end's timed pair (HIP events; k_source_iq rides inside it) and the whole step by the host clock.  Beside
them `copy_ms`: a bare device-to-device copy of the same source bytes (one read + one write of them, nothing else) by HIP
events, and the library's streaming probe (rtlfm_gpu_bw_probe: read only, and read + 1/8 written).  `iq_ms` = the timed
pair with the option on minus the pair with it off: what the pass adds, the front end's changed input included.
Prints one JSON line: per variant the median over the repeats and their spread (min, max).
"""
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
    ap.add_argument("--shapes", default="64x64,1024x4", help="sources x channels, comma separated")
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--block-len", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=10, help="runs per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per variant, alternating")
    ap.add_argument("--nt", type=int, default=1, help="k_source_iq's loads non-temporal (option input_stats_nt)")
    a = ap.parse_args()

    import torch

    from rtlsdr_amd import build as hipbuild
    from rtlsdr_amd import capi
    from rtlsdr_amd.capi import ATAN_FAST, RtlfmCfg
    from rtlsdr_amd.demod import GpuDemod
    hipbuild.build()
    if not torch.cuda.is_available():
        sys.exit("source_iq_bench: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    dev = torch.device("cuda", 0)
    L, NB, D = a.block_len, a.blocks, 10
    line = {"tool": "source_iq_bench", "gpu": torch.cuda.get_device_name(0), "blocks": NB, "block_len": L, "steps": a.steps,
            "repeats": a.repeats, "nt": a.nt}
    rd, rw, rwc, wf = C.c_double(), C.c_double(), C.c_double(), C.c_double()
    capi.check(capi.load().rtlfm_gpu_bw_probe(0, 1 << 30, 8, 5, C.byref(rd), C.byref(rw), C.byref(rwc), C.byref(wf)), "rtlfm_gpu_bw_probe")
    line["probe"] = {"read_gbs": round(rd.value, 1), "rw_gbs": round(rw.value, 1), "write_fraction": wf.value}
    for shape in a.shapes.split(","):
        nsrc, per = (int(v) for v in shape.split("x"))
        gen = torch.Generator(device=dev)
        gen.manual_seed(20261021)
        src = torch.randint(38, 217, (nsrc, NB * L), dtype=torch.uint8, device=dev, generator=gen)
        steps = np.random.default_rng(1).integers(0, 1 << 32, size=nsrc * per, dtype=np.uint64).astype(np.uint32)
        cfg = RtlfmCfg.default(downsample=D, custom_atan=ATAN_FAST, rate_out=2400000 // D, block_len=L, max_blocks=NB)
        g = GpuDemod(cfg, nsrc * per, 0, options=dict(input_stats_nt=a.nt))
        g.set_channels(per, steps=steps)
        coef = np.tile(np.array([13000, 0, -2200, 16384], dtype=np.int16), (nsrc, 1))
        g.set_source_iq(coef)
        out = torch.empty((g.nstreams, g.result_cap(cfg.max_blocks)), dtype=torch.int16, device=dev)
        out_len = torch.zeros(g.nstreams, dtype=torch.int32, device=dev)
        dst = torch.empty_like(src)

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

        def copy_window(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(n):
                dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / n

        def select(on):
            if g.get_option("source_iq") != on:
                g.set_option("source_iq", on)  # (outside the window: it waits for the handle)

        variants = {"off": 0, "iq": 1}
        for v in variants.values():
            select(v)
            window(a.warmup, False)
        copy_window(a.warmup)
        res = {k: dict(step_ms=[], front_ms=[]) for k in variants}
        copies = []
        for _ in range(a.repeats):
            for k, v in variants.items():
                select(v)
                res[k]["step_ms"].append(window(a.steps, False)[0])
            for k, v in variants.items():  # the event pairs cost a little: the front end in windows of its own
                select(v)
                res[k]["front_ms"].append(window(a.steps, True)[1])
            copies.append(copy_window(a.steps))
        leg = {}
        for k, r in res.items():
            leg[k] = {m: dict(median=float(np.median(r[m])), min=float(min(r[m])), max=float(max(r[m]))) for m in ("step_ms", "front_ms")}
        leg["copy_ms"] = dict(median=float(np.median(copies)), min=float(min(copies)), max=float(max(copies)))
        leg["iq_ms"] = leg["iq"]["front_ms"]["median"] - leg["off"]["front_ms"]["median"]
        leg["moved_mib"] = 2 * nsrc * NB * L / (1 << 20)
        line[shape] = leg
        g.close()
        del out, out_len, src, dst
        torch.cuda.empty_cache()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
