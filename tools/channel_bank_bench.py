#!/usr/bin/env python3
"""The channel bank at scale: tools/channel_fir_bench.py's shape - 64 sources x 64 channels = 4096 streams, 4 x 262144 B per
source and step, -A fast - with the channels uniformly spaced, steps[k] = k 2^32 / K, so that the mixer paths and the bank
(include/rtlfm_hip.h, rtlfm_gpu_set_channel_bank) cut out the same channels.

Timed in ONE session on one GPU, per D (default 10, the existing legs' D, and 32, the 2x oversampled bank), alternating,
after a warm-up of each:
  boxcar      k_channel_boxcar + the back half
  fir80_p2    80 taps of rtlfm_channel_lowpass(80, 0.4 / D, D) on path 2: k_channel_fir, one NCO mixer per channel
  bank_p2     512 taps of rtlfm_channel_lowpass(512, 0.4 / K, D), shift 14 - log2 K, on path 2: k_channel_bank, one launch
  bank_p1     the same on path 1: the plain cross-check
each as the front end alone (the handle's event timing) and as the whole step (host clock around --steps runs that end in
a synchronise).  The outputs of the bank's two paths are compared (they must be equal).  Prints one JSON line.
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
    ap.add_argument("--K", type=int, default=64, help="channels per source = bins of the bank")
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--block-len", type=int, default=262144)
    ap.add_argument("--downsample", type=int, nargs="*", default=[10, 32])
    ap.add_argument("--bank-taps", type=int, default=512)
    ap.add_argument("--fir-taps", type=int, default=80)
    ap.add_argument("--steps", type=int, default=20, help="runs per timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per variant, alternating")
    ap.add_argument("--no-path1", action="store_true", help="skip the bank's path 1 (a work buffer of K dwords per source and output)")
    a = ap.parse_args()

    import torch

    from rtlsdr_amd import build as hipbuild
    from rtlsdr_amd.capi import ATAN_FAST, RtlfmCfg
    from rtlsdr_amd.demod import GpuDemod, channel_lowpass
    hipbuild.build()
    if not torch.cuda.is_available():
        sys.exit("channel_bank_bench: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    dev = torch.device("cuda", 0)
    K = a.K
    m = K.bit_length() - 1
    S = a.sources * K
    L, NB = a.block_len, a.blocks
    gen = torch.Generator(device=dev)
    gen.manual_seed(20261019)
    src = torch.randint(38, 217, (a.sources, NB * L), dtype=torch.uint8, device=dev, generator=gen)
    steps = np.tile(np.array([(k << 32) // K for k in range(K)], dtype=np.uint32), a.sources)
    samples = S * NB * (L // 2)
    line = {"tool": "channel_bank_bench", "gpu": torch.cuda.get_device_name(0), "sources": a.sources, "K": K, "streams": S,
            "blocks": NB, "block_len": L, "bank_taps": a.bank_taps, "fir_taps": a.fir_taps, "steps": a.steps, "repeats": a.repeats,
            "stream_samples_per_step": samples}

    for D in a.downsample:
        cfg = RtlfmCfg.default(downsample=D, custom_atan=ATAN_FAST, rate_out=2400000 // D, block_len=L, max_blocks=NB)
        chan = GpuDemod(cfg, S, 0)
        chan.set_channels(K, steps=steps)
        out = torch.empty((S, chan.result_cap(NB)), dtype=torch.int16, device=dev)
        out_len = torch.zeros(S, dtype=torch.int32, device=dev)
        fir = channel_lowpass(a.fir_taps, 0.4 / D, D)
        bank_taps, bank_shift = channel_lowpass(a.bank_taps, 0.4 / K, D)
        bank_shift -= m
        current = [None]

        def select(kind, path):
            """(the setters wait for the handle and clear the history: only when the front end really changes)"""
            if current[0] != kind:
                chan.set_channel_bank(0)
                chan.set_channel_filter(None)
                if kind == "fir":
                    chan.set_channel_filter(*fir)
                elif kind == "bank":
                    chan.set_channel_bank(K, bank_taps, bank_shift)
                current[0] = kind
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

        def variant(kind, path):
            def f(n, front=False):
                select(kind, path)
                r = window(n, front)
                assert chan.last_path == (1 if path == 1 else 2)
                return r
            return f

        variants = {"boxcar": variant("boxcar", 0), "fir%d_p2" % a.fir_taps: variant("fir", 0), "bank_p2": variant("bank", 0)}
        if not a.no_path1:
            variants["bank_p1"] = variant("bank", 1)

        # the same input from the same state through both paths of the bank: equal, or the timing compares two different things
        equal = None
        if not a.no_path1:
            chan.reset(); variants["bank_p2"](1); a_out, a_len = out.clone(), out_len.clone()
            chan.reset(); variants["bank_p1"](1)
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
        leg = {"paths_equal": equal}
        for k, r in res.items():
            med = float(np.median(r["step_ms"]))
            leg[k] = dict(step_ms=med, step_ms_min=float(min(r["step_ms"])), step_ms_max=float(max(r["step_ms"])),
                          front_ms=float(np.median(r["front_ms"])), front_ms_min=float(min(r["front_ms"])),
                          front_ms_max=float(max(r["front_ms"])), gsamples_per_s=samples / med / 1e6)
        line["D%d" % D] = leg
        chan.close()
        del out, out_len
        torch.cuda.empty_cache()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
