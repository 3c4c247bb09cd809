#!/usr/bin/env python3
"""What the input-health records of the raw input (k_input_health, option "input_health") cost next to the ADC
statistics (k_input_stats).  A tool, not a test.

    python tools/input_health_bench.py [--rounds 5 --launches 20]

On the ns4096 shape (4096 streams x 4 x 262144 B = 4 GiB) it times, alternating round by round in one session, HIP-event
time per launch after warm-up:
    health     k_input_health alone            (rtlfm_gpu_input_health_device)
    stats      k_input_stats alone             (rtlfm_gpu_input_stats_device)
    combined   one launch writing both arrays  (rtlfm_gpu_input_health_stats_device: what a handle with both options runs)
and prints one JSON line with the medians, the read rates, health / stats and combined / (health + stats).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--plain", action="store_true", help="plain loads instead of non-temporal ones")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("input_health_bench.py measures on a GPU; there is none here")
    from rtlsdr_amd import capi
    lib = capi.load()
    S, NB, L = a.streams, 4, 262144
    nt = 0 if a.plain else 1
    dev = torch.device("cuda", 0)
    iq = torch.randint(0, 256, (S, NB * L), dtype=torch.uint8, device=dev)
    health = torch.zeros((S * NB, 4), dtype=torch.int32, device=dev)
    stats = torch.zeros((S * NB, 4), dtype=torch.int32, device=dev)
    nbytes = S * NB * L
    q = torch.cuda.current_stream().cuda_stream or None
    args = (0, iq.data_ptr(), iq.stride(0), L, NB, S)

    def go(name):
        if name == "health":
            r = lib.rtlfm_gpu_input_health_device(*args, health.data_ptr(), nt, q)
        elif name == "stats":
            r = lib.rtlfm_gpu_input_stats_device(*args, stats.data_ptr(), nt, q)
        else:
            r = lib.rtlfm_gpu_input_health_stats_device(*args, health.data_ptr(), stats.data_ptr(), nt, q)
        assert r == 0, (name, r)

    def timed(name, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            go(name)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    legs = ("health", "stats", "combined")
    for name in legs:
        timed(name, 5)
    ms = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name in legs:
            ms[name].append(timed(name, a.launches))
    res = {"shape": [S, NB, L], "bytes": nbytes, "rounds": a.rounds, "launches": a.launches, "nontemporal": nt}
    med = {}
    for name in legs:
        med[name] = statistics.median(ms[name])
        res[name] = {"ms_median": round(med[name], 4), "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4),
                     "read_gbs": round(nbytes / med[name] / 1e6, 1)}
    res["health_over_stats"] = round(med["health"] / med["stats"], 4)
    res["combined_over_sum"] = round(med["combined"] / (med["health"] + med["stats"]), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
