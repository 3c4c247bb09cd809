#!/usr/bin/env python3
"""What packed results save on the way back to the host: the channelizer's ring shape of tools/channel_ring_bench.py -
64 sources x 64 channels = 4096 streams, 4 x 262144 B per source and step, config c1's chain (low_pass /10, -A fast)
behind k_channel_boxcar over the source-indexed ring - with the squelch set (-l), and sources in which a stated number
of every source's 64 channels carry a carrier: 64, 16, 4, 1, 0.

How a channel is made open or closed.  At /10 the 64 channels of a source overlap - the boxcar passes everything within
a few percent of the sample rate - so a carrier cannot be kept out of its neighbours by spacing.  The k open channels
are tuned 2^-10 of the sample rate beside k carriers that lie close together around one frequency (2^-14 of the sample
rate apart, amplitude 5 each, random phases; beside, because rms() takes the mean out and an unmodulated carrier at rest
would not count); the 64 - k closed ones are tuned a whole multiple of a tenth of the sample rate away from it, where the
boxcar of 10 has its zeros: what they see of the carriers is a fiftieth, below the squelch, beside noise of one LSB.
tests/scan_model.tone_or_noise shows the two kinds of buffer for one stream.  The open rows are counted from the index
and reported; the input of every step is the same bytes, so that after the warm-up the closed channels stay closed
(conseq_squelch, 10, has long run out) and the held count is every buffer of every closed channel.

Timed in ONE session on one GPU and ONE handle per occupancy, alternating windows after a warm-up of each:
  all      option pack_results 0: rtlfm_gpu_push x (sources x blocks) -> rtlfm_gpu_run -> rtlfm_gpu_fetch_all_prev into pinned rows
  packed   option pack_results 2: the same with rtlfm_gpu_fetch_packed_prev into a pinned buffer
each the whole step by the host clock and its three parts (push, run, fetch) by the host clock around their calls - run only
queues work, so the parts say where the HOST waits.  The two pack launches alone by events around them (option pack_us,
rtlfm_gpu_timing_enable), in a window of its own that waits for every run.  Bytes copied back per step: the rectangle
max(lens) x streams and the lengths, against the packed total and the index.
Prints a table and one JSON line.  There is no pass mark."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SQUELCH = 15
CARRIER = 5.0
OFF_TUNE = 1.0 / 1024  # an open channel sits this far (cycles per capture sample) beside its carrier: rms() takes the mean
                       # out (src/rtl_fm.c:1083-1112), an unmodulated carrier at rest would not count


def make_sources(rng, nsrc, nbytes, k):
    """uint8 [nsrc, nbytes]: k carriers 2^-14 of the sample rate apart around 0, one waveform turned by a phase of its
    own for every source, and noise of one LSB."""
    n = np.arange(nbytes // 2, dtype=np.float64)
    base = np.zeros(n.size, dtype=np.complex128)
    for c in range(k):
        base += CARRIER * np.exp(1j * 2 * np.pi * (carrier_cycles(c, k) * n + rng.random()))
    out = np.empty((nsrc, nbytes), dtype=np.uint8)
    for i in range(nsrc):
        sig = base * np.exp(2j * np.pi * rng.random())
        out[i, 0::2] = np.clip(np.rint(127 + sig.real + rng.integers(-1, 2, n.size)), 0, 255)
        out[i, 1::2] = np.clip(np.rint(127 + sig.imag + rng.integers(-1, 2, n.size)), 0, 255)
    return out


def carrier_cycles(c, k):
    """carrier c of k, in cycles per capture sample"""
    return (c - k // 2) / 16384.0


def channel_steps(nsrc, per, k):
    """uint32 [nsrc * per]: channel c < k of every source beside carrier c; the others on the boxcar's zeros around the cluster"""
    st = np.zeros((nsrc, per), dtype=np.uint64)
    for c in range(per):
        cyc = carrier_cycles(c, k) - OFF_TUNE if c < k else (1 + (c - k) % 9) / 10.0
        st[:, c] = int(round(cyc * (1 << 32))) & 0xFFFFFFFF
    return st.reshape(-1).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sources", type=int, default=64)
    ap.add_argument("--per-source", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--block-len", type=int, default=262144)
    ap.add_argument("--open", type=int, nargs="*", default=None, help="open channels per source (default 64 16 4 1 0)")
    ap.add_argument("--steps", type=int, default=10, help="runs per timed window")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3, help="timed windows per variant, alternating")
    a = ap.parse_args()

    import torch

    from rtlsdr_amd import build as hipbuild
    from rtlsdr_amd.capi import ATAN_FAST, PACKED_ROW, RtlfmCfg, check
    from rtlsdr_amd.demod import GpuDemod
    hipbuild.build()
    if not torch.cuda.is_available():
        sys.exit("packed_fetch_bench: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    nsrc, per = a.sources, a.per_source
    S = nsrc * per
    L, NB = a.block_len, a.blocks
    opens = a.open if a.open else [k for k in (64, 16, 4, 1, 0) if k <= per]
    cfg = RtlfmCfg.default(downsample=10, custom_atan=ATAN_FAST, rate_out=240000, block_len=L, max_blocks=NB, squelch_level=SQUELCH)
    rng = np.random.default_rng(20261020)
    host_in = torch.empty((nsrc, NB * L), dtype=torch.uint8).pin_memory()
    src = host_in.numpy()
    ptrs = [[src[i, j * L:(j + 1) * L].ctypes.data for j in range(NB)] for i in range(nsrc)]

    g = GpuDemod(cfg, S, 0, options=dict(source_ring=1))
    lib, h = g.lib, g._h
    cap = lib.rtlfm_result_cap(C.byref(cfg)) * NB + 16
    host_out = torch.empty((S, cap), dtype=torch.int16).pin_memory()
    host_packed = torch.empty(S * ((cap + 7) & ~7), dtype=torch.int16).pin_memory()
    lens = np.zeros(S, dtype=np.int32)
    index = np.zeros(S, dtype=PACKED_ROW)
    total = C.c_size_t()

    def push():
        for i in range(nsrc):
            for p in ptrs[i]:
                check(lib.rtlfm_gpu_push(h, i, p, L), "push")

    def fetch_all():
        check(lib.rtlfm_gpu_fetch_all_prev(h, host_out.data_ptr(), cap, lens.ctypes.data), "fetch_all_prev")

    def fetch_packed():
        check(lib.rtlfm_gpu_fetch_packed_prev(h, host_packed.data_ptr(), host_packed.numel(), index.ctypes.data, C.byref(total)),
              "fetch_packed_prev")

    def window(mode, fetch, n):
        """n steady-state steps with option pack_results at `mode` (one run is in flight when the window opens)"""
        g.set_option("pack_results", mode)
        for _ in range(2):
            push()
            check(lib.rtlfm_gpu_run(h), "run")
        g.sync()
        tp = tr = tf = 0.0
        t00 = time.perf_counter()
        for _ in range(n):
            t0 = time.perf_counter()
            push()
            t1 = time.perf_counter()
            check(lib.rtlfm_gpu_run(h), "run")
            t2 = time.perf_counter()
            fetch()
            t3 = time.perf_counter()
            tp += t1 - t0
            tr += t2 - t1
            tf += t3 - t2
        whole = time.perf_counter() - t00
        g.sync()
        return dict(step_ms=whole * 1e3 / n, push_ms=tp * 1e3 / n, run_ms=tr * 1e3 / n, fetch_ms=tf * 1e3 / n)

    def pack_alone(n):
        """the two launches by their own events: every run waited for"""
        g.set_option("pack_results", 2)
        g.timing_enable(True)
        us = []
        for _ in range(n + 1):
            push()
            check(lib.rtlfm_gpu_run(h), "run")
            us.append(g.get_option("pack_us"))
        g.timing_enable(False)
        g.timing_read()
        return float(np.median(us[1:]))

    rows = []
    for k in opens:
        src[:] = make_sources(rng, nsrc, NB * L, k)
        g.set_option("pack_results", 0)
        g.reset()
        g.set_channels(per, steps=channel_steps(nsrc, per, k))
        for _ in range(a.warmup):  # conseq_squelch runs out: from here on every closed channel is held
            push()
            check(lib.rtlfm_gpu_run(h), "run")
        res = dict(all=[], packed=[])
        for _ in range(a.repeats):
            res["all"].append(window(0, fetch_all, a.steps))
            res["packed"].append(window(2, fetch_packed, a.steps))
        assert g.last_path == 2
        row = dict(open_per_source=k, open_rows=int((index["len"] > 0).sum()), held_buffers=int(index["held"].sum()),
                   all_bytes=int(S * int(lens.max()) * 2 + S * 4), packed_bytes=int(total.value * 2 + S * 16),
                   pack_launches_us=pack_alone(a.steps))
        for name, ws in res.items():
            row[name] = {f: float(np.median([w[f] for w in ws])) for f in ws[0]}
        rows.append(row)
        print(f"open {k:2d} of {per}: rows open {row['open_rows']:5d} of {S}, held {row['held_buffers']:6d}; "
              f"fetch_all_prev step {row['all']['step_ms']:7.3f} ms (push {row['all']['push_ms']:.3f} run {row['all']['run_ms']:.3f} "
              f"fetch {row['all']['fetch_ms']:.3f}) {row['all_bytes'] / 1e6:8.2f} MB | fetch_packed_prev step {row['packed']['step_ms']:7.3f} ms "
              f"(push {row['packed']['push_ms']:.3f} run {row['packed']['run_ms']:.3f} fetch {row['packed']['fetch_ms']:.3f}) "
              f"{row['packed_bytes'] / 1e6:8.2f} MB | pack launches {row['pack_launches_us']:.0f} us", flush=True)
    out = dict(tool="packed_fetch_bench", gpu=torch.cuda.get_device_name(0), sources=nsrc, per_source=per, streams=S, blocks=NB,
               block_len=L, squelch_level=SQUELCH, steps=a.steps, repeats=a.repeats, input_bytes_per_step=nsrc * NB * L, rows=rows)
    g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
