#!/usr/bin/env python3
"""The channel bank's survey and slots at scale, in tools/channel_bank_bench.py's shape: 64 sources, K = 256 bins, 4 x 262144 B
per source and step, 512 taps of rtlfm_channel_lowpass(512, 0.4 / K, D) with shift 14 - log2 K, -A fast, at / 10 and / 32.

Timed in ONE session on one GPU, per D, alternating, after a warm-up of each:
  bank            per_source 16, option bank_survey 0: k_channel_bank (the front end's event timing) and the whole step
  bank_survey     the same handle with the option at 1: k_channel_bank_survey + k_bank_survey_reduce, and the whole step
  fetch_us        rtlfm_gpu_bank_survey of a finished run: host clock, the device idle (64 x 256 uint64 and 64 int32)
  set_bins_us     one rtlfm_gpu_set_channel_bins call: host clock (it waits for nothing: a pinned copy is queued)
  loop            the whole step with 16 slots: run -> bank_survey -> SlotAllocator.step -> set_channel_bins
  wide            the handle a caller needs today to see all 256 bins: per_source 256, option off, the whole step
The survey is compared with numpy's sum of the wide handle's -M raw rows' squares once, on a small run (they must be
equal).  Prints one JSON line.
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
    ap.add_argument("--K", type=int, default=256)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--block-len", type=int, default=262144)
    ap.add_argument("--downsample", type=int, nargs="*", default=[10, 32])
    ap.add_argument("--bank-taps", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10, help="runs per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per variant, alternating")
    ap.add_argument("--no-wide", action="store_true", help="skip the per_source = K handle (sources x K streams of back half)")
    a = ap.parse_args()

    import torch

    from rtlsdr_amd import build as hipbuild
    from rtlsdr_amd.capi import ATAN_FAST, MODE_RAW, RtlfmCfg
    from rtlsdr_amd.demod import GpuDemod, channel_lowpass
    from rtlsdr_amd.slots import SlotAllocator
    hipbuild.build()
    if not torch.cuda.is_available():
        sys.exit("bank_survey_bench: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    dev = torch.device("cuda", 0)
    K, per, nsrc = a.K, a.slots, a.sources
    m = K.bit_length() - 1
    L, NB = a.block_len, a.blocks
    gen = torch.Generator(device=dev)
    gen.manual_seed(20261020)
    src = torch.randint(38, 217, (nsrc, NB * L), dtype=torch.uint8, device=dev, generator=gen)
    line = {"tool": "bank_survey_bench", "gpu": torch.cuda.get_device_name(0), "sources": nsrc, "K": K, "slots": per, "blocks": NB,
            "block_len": L, "bank_taps": a.bank_taps, "steps": a.steps, "repeats": a.repeats}

    def handle(cfg, per_source, bins):
        g = GpuDemod(cfg, nsrc * per_source, 0)
        g.set_channels(per_source, steps=np.zeros(nsrc * per_source, dtype=np.uint32))
        taps, shift = channel_lowpass(a.bank_taps, 0.4 / K, cfg.downsample)
        g.set_channel_bank(K, taps, shift - m, bins=bins)
        out = torch.empty((g.nstreams, g.result_cap(cfg.max_blocks)), dtype=torch.int16, device=dev)
        out_len = torch.zeros(g.nstreams, dtype=torch.int32, device=dev)
        return g, out, out_len

    def run(g, out, out_len, rows=src, nb=NB):
        g.run_device(rows.data_ptr(), rows.stride(0), nb, out.data_ptr(), out.stride(0), out_len.data_ptr())

    for D in a.downsample:
        leg = {}
        # the survey against the rows it sums, once, small: -M raw, one buffer of 16384 B, per_source = K
        small = RtlfmCfg.default(mode=MODE_RAW, downsample=D, block_len=16384, max_blocks=1)
        g, out, out_len = handle(small, K, None)
        g.set_option("bank_survey", 1)
        run(g, out, out_len, src[:, :16384].contiguous(), 1)
        power, frames = g.bank_survey()
        rows = out.cpu().numpy().astype(np.int64)
        n = int(out_len[0]) // 2
        want = (rows[:, 0:2 * n:2] ** 2 + rows[:, 1:2 * n:2] ** 2).sum(axis=1).astype(np.uint64).reshape(nsrc, K)
        leg["survey_equals_rows"] = bool(np.array_equal(power, want)) and frames.tolist() == [n] * nsrc
        g.close()
        del out, out_len

        cfg = RtlfmCfg.default(downsample=D, custom_atan=ATAN_FAST, rate_out=2400000 // D, block_len=L, max_blocks=NB)
        bins0 = [(7 + 13 * c) % K for c in range(per)]
        g, out, out_len = handle(cfg, per, bins0)
        wide = None if a.no_wide else handle(cfg, K, None)
        alloc = SlotAllocator(nsrc, K, per, open_level=1 << 40, close_level=1 << 39, hang=2, park=K // 2)
        all_bins = np.tile(np.array(bins0, dtype=np.int32), (nsrc, 1))

        def window(fn, n, sync, timed=None):
            if timed is not None:
                timed.timing_enable(True)
                timed.timing_read()
            sync()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            sync()
            ms = (time.perf_counter() - t0) * 1e3 / n
            fms = None
            if timed is not None:
                tot, k = timed.timing_read()
                timed.timing_enable(False)
                fms = tot / max(1, k)
            return ms, fms

        def plain(on):
            def f(n, front=False):
                if g.get_option("bank_survey") != on:
                    g.set_option("bank_survey", on)  # (outside the window; 1 -> 0 waits and frees)
                return window(lambda: run(g, out, out_len), n, g.sync, g if front else None)
            return f

        def loop_step():
            run(g, out, out_len)
            alloc.step(*g.bank_survey())
            g.set_channel_bins(alloc.bins())

        def loop(n, front=False):
            g.set_option("bank_survey", 1)
            return window(loop_step, n, g.sync, g if front else None)

        variants = {"bank": plain(0), "bank_survey": plain(1), "loop": loop}
        if wide is not None:
            variants["wide"] = lambda n, front=False: window(lambda: run(*wide), n, wide[0].sync, wide[0] if front else None)
        for f in variants.values():
            f(a.warmup)
        res = {k: dict(step_ms=[], front_ms=[]) for k in variants}
        host = dict(fetch_us=[], set_bins_us=[])
        for _ in range(a.repeats):
            for k, f in variants.items():
                res[k]["step_ms"].append(f(a.steps)[0])
            for k, f in variants.items():  # the event pairs cost a little: the front end in windows of its own
                res[k]["front_ms"].append(f(a.steps, True)[1])
            g.set_option("bank_survey", 1)
            run(g, out, out_len)
            g.sync()
            t0 = time.perf_counter()
            for _ in range(20):
                g.bank_survey()
            host["fetch_us"].append((time.perf_counter() - t0) * 1e6 / 20)
            t0 = time.perf_counter()
            for _ in range(20):
                g.set_channel_bins(all_bins)
            host["set_bins_us"].append((time.perf_counter() - t0) * 1e6 / 20)
            g.sync()
        for k, r in res.items():
            leg[k] = dict(step_ms=float(np.median(r["step_ms"])), step_ms_min=float(min(r["step_ms"])), step_ms_max=float(max(r["step_ms"])),
                          front_ms=float(np.median(r["front_ms"])), front_ms_min=float(min(r["front_ms"])),
                          front_ms_max=float(max(r["front_ms"])))
        for k, v in host.items():
            leg[k] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
        leg["survey_front_over_bank"] = leg["bank_survey"]["front_ms"] / leg["bank"]["front_ms"]
        line["D%d" % D] = leg
        alloc.close()
        g.close()
        if wide is not None:
            wide[0].close()
        del out, out_len, wide
        torch.cuda.empty_cache()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
