#!/usr/bin/env python3
"""What the ADC statistics of the raw input (k_input_stats, option "input_stats") cost.  A tool, not a test.

    python tools/input_stats_bench.py kernel [--rounds 5 --launches 20]
        k_input_stats alone on the ns4096 shape (4096 streams x 4 x 262144 B = 4 GiB): HIP-event time per launch and
        achieved read rate, non-temporal and plain loads alternating round by round, next to rtlfm_gpu_bw_probe's
        read_gbs of the same process (the library's own ceiling probe)
    python tools/input_stats_bench.py steps [--workloads ns4096,c1,c3 --rounds 5 --steps 20 --parent LIB]
        the ns4096 / c1 / c3 steps (bench.py's shapes) with the option off and on, alternating round by round; with
        --parent <another build of librtlfm_hip.so> that build's step as a third leg (option off must equal it)
    python tools/input_stats_bench.py trace
        a few launches of everything, for `rocprofv3 --kernel-trace --stats -- python tools/input_stats_bench.py trace`

Every mode prints one JSON line.  Input and output are plain allocations (wherever the allocator puts them: the
"co-located" figures of bench.py, not its placed ones) - the same for every leg, which is what a difference needs.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    # bench.py's WORKLOADS
    "ns4096": dict(streams=4096, blocks=4, block_len=262144, passes=4, boxcar=0, fir9=0, atan="std", fs=2.4e6, tail=""),
    "c1": dict(streams=256, blocks=64, block_len=262144, passes=0, boxcar=10, fir9=0, atan="fast", fs=2.4e6, tail=""),
    "c3": dict(streams=4096, blocks=4, block_len=262144, passes=6, boxcar=0, fir9=1, atan="std", fs=1.024e6, tail="c3"),
}


def make_cfg(w):
    from rtlsdr_amd.capi import ATAN_FAST, ATAN_STD, RESAMPLE_ARBITRARY, RtlfmCfg, load
    d = w["boxcar"] if w["boxcar"] else 1 << w["passes"]
    kw = dict(downsample=d, downsample_passes=w["passes"], comp_fir_size=9 if w["fir9"] else 0,
              custom_atan=ATAN_FAST if w["atan"] == "fast" else ATAN_STD, rate_out=int(w["fs"] / d), block_len=w["block_len"],
              max_blocks=w["blocks"])
    if w["tail"] == "c3":
        kw.update(rate_out=16000, deemph=1, deemph_a=load().rtlfm_deemph_a(16000, 75), rate_out2=22050, resampler=RESAMPLE_ARBITRARY)
    return RtlfmCfg.default(**kw)


def kernel_mode(a):
    import ctypes as C

    import torch
    from rtlsdr_amd import capi
    lib = capi.load()
    S, NB, L = 4096, 4, 262144
    dev = torch.device("cuda", 0)
    iq = torch.randint(0, 256, (S, NB * L), dtype=torch.uint8, device=dev)
    out = torch.zeros((S * NB, 4), dtype=torch.int32, device=dev)
    nbytes = S * NB * L

    def launch(nt):
        r = lib.rtlfm_gpu_input_stats_device(0, iq.data_ptr(), iq.stride(0), L, NB, S, out.data_ptr(), nt,
                                             torch.cuda.current_stream().cuda_stream or None)
        assert r == 0, r

    def timed(nt, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            launch(nt)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    for nt in (1, 0):
        timed(nt, 5)
    ms = {1: [], 0: []}
    for _ in range(a.rounds):
        for nt in (1, 0):
            ms[nt].append(timed(nt, a.launches))
    rd, rw, rwc, wf = C.c_double(), C.c_double(), C.c_double(), C.c_double()
    r = lib.rtlfm_gpu_bw_probe(0, nbytes, 16, 20, C.byref(rd), C.byref(rw), C.byref(rwc), C.byref(wf))
    res = {"mode": "kernel", "shape": [S, NB, L], "bytes": nbytes, "rounds": a.rounds, "launches": a.launches, "bw_probe_rc": r,
           "bw_probe_read_gbs": round(rd.value, 1)}
    for nt, name in ((1, "nontemporal"), (0, "plain")):
        med = statistics.median(ms[nt])
        res[name] = {"ms_median": round(med, 4), "ms_min": round(min(ms[nt]), 4), "ms_max": round(max(ms[nt]), 4),
                     "read_gbs": round(nbytes / med / 1e6, 1),
                     "of_bw_probe_read": round(nbytes / med / 1e6 / rd.value, 4) if rd.value > 0 else None}
    print(json.dumps(res))


class Leg:
    def __init__(self, name, w, iq, lib_path, options):
        import torch
        from rtlsdr_amd.demod import GpuDemod
        self.name, self.w, self.iq = name, w, iq
        self.g = GpuDemod(make_cfg(w), w["streams"], 0, lib_path=lib_path, options=options)
        cap = self.g.result_cap(w["blocks"])
        self.out = torch.empty((w["streams"], cap), dtype=torch.int16, device=iq.device)
        self.n = torch.zeros(w["streams"], dtype=torch.int32, device=iq.device)
        self.ms = []

    def step(self):
        self.g.run_device(self.iq.data_ptr(), self.iq.stride(0), self.w["blocks"], self.out.data_ptr(), self.out.stride(0), self.n.data_ptr())

    def timed(self, n):
        """wall ms per step of n steps back to back, ending in a synchronise (front end + tail, as a caller sees it)"""
        self.g.sync()
        t0 = time.perf_counter()
        for _ in range(n):
            self.step()
        self.g.sync()
        return (time.perf_counter() - t0) * 1e3 / n


def steps_mode(a, trace=False):
    import torch
    from rtlsdr_amd import synth
    res = {"mode": "trace" if trace else "steps", "rounds": a.rounds, "steps": a.steps, "workloads": {}}
    for name in a.workloads.split(","):
        w = SHAPES[name]
        dev = torch.device("cuda", 0)
        iq = synth.fm_iq_u8_torch(w["streams"], w["blocks"] * w["block_len"] // 2, dev, fs=w["fs"],
                                  dev_hz=75e3 if w["fs"] > 2e6 else 5e3, amplitude=40.0 if w["atan"] == "fast" else 60.0)
        torch.cuda.synchronize()
        legs = [Leg("off", w, iq, None, None), Leg("on", w, iq, None, {"input_stats": 1})]
        if a.parent:
            legs.append(Leg("parent", w, iq, a.parent, None))
        for leg in legs:
            leg.timed(3 if trace else 10)
        if not trace:
            for _ in range(a.rounds):
                for leg in legs:
                    leg.ms.append(leg.timed(a.steps))
            nbytes = w["streams"] * w["blocks"] * w["block_len"]
            e = {"bytes": nbytes}
            for leg in legs:
                e[leg.name] = {"ms_median": round(statistics.median(leg.ms), 4), "ms_min": round(min(leg.ms), 4),
                               "ms_max": round(max(leg.ms), 4)}
            e["on_minus_off_ms"] = round(e["on"]["ms_median"] - e["off"]["ms_median"], 4)
            if a.parent:
                e["off_over_parent"] = round(e["off"]["ms_median"] / e["parent"]["ms_median"], 4)
            res["workloads"][name] = e
        for leg in legs:
            leg.g.close()
        del legs, iq
        torch.cuda.empty_cache()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["kernel", "steps", "trace"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--workloads", default="ns4096,c1,c3")
    ap.add_argument("--parent", default=None, help="another build of librtlfm_hip.so (an earlier revision) as a third leg")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("input_stats_bench.py measures on a GPU; there is none here")
    if a.mode == "kernel":
        kernel_mode(a)
    elif a.mode == "steps":
        steps_mode(a)
    else:
        a.rounds, a.launches = 1, 3
        kernel_mode(a)
        steps_mode(a, trace=True)


if __name__ == "__main__":
    main()
