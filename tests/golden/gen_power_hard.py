#!/usr/bin/env python3
"""Write tests/golden/power_hard.json: parameters of hard-limited tones (tests/power_hard.py, square_iq) on which fix_fft's
int16 stores wrap, per transform case of tests/test_power_hard_gpu.py - parameters, the model's counts and a digest of the
bytes, no bytes.

A seeded, bounded search per case over (inc, phase, rails): random increments, bin-centred ones (k << (32 - bin_e)) and
coarse ones (k << 26), each judged by the model on one read; for a stage none of them reached, candidates found at the
size at which that stage is the last (lifted(), below).  Of the candidates a greedy cover keeps, up to 2^14 points for the
bin-centred ones and for the others separately, the few that together wrap in every stage 2 .. bin_e - 1; a stage no
candidate reached is named in "missing".  The kept sets are then run through the model as the tests use them (READS reads) and recorded with
their per-stage counts.  A frame with a bin of |X|^2 > 2^31 - 1 - which is re = im = -32768, exactly 2^31, and nothing
else - is recorded where the search meets one; "over_2_31" is null where it did not.

    python tests/golden/gen_power_hard.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import power_hard as ph  # noqa: E402
from rtlsdr_amd.capi import RtlpowerCfg  # noqa: E402

SEED = 20261021

# case -> (cfg, candidates).  The decimated cases: ds = what the tone's increment is multiplied by in front of the FFT;
# their rails are 127 +- a with the decimated samples at +-124 .. +-127 (boxcar / 4: a = 31; two fifth_order passes and
# the FIR have a gain of about 4.35 and overshoot: a from 24 to 31), where the window product stays a coherent +-32 k square
CASES = {
    "b3": (dict(bin_e=3, buf_len=16384), 300),
    "b6": (dict(bin_e=6, buf_len=16384), 600),
    "b7": (dict(bin_e=7, buf_len=16384), 600),
    "b10": (dict(bin_e=10, buf_len=16384), 900),
    "b12": (dict(bin_e=12, buf_len=16384), 900),
    "b13": (dict(bin_e=13, buf_len=16384), 900),
    "b14": (dict(bin_e=14, buf_len=32768), 900),
    "b15": (dict(bin_e=15, buf_len=65536), 400),
    "b16": (dict(bin_e=16, buf_len=131072), 300),
    "b17": (dict(bin_e=17, buf_len=262144), 200),
    "b10_box4": (dict(bin_e=10, downsample=4, boxcar=1, buf_len=16384), 900),
    "b9_fifth2_fir9": (dict(bin_e=9, downsample=4, downsample_passes=2, boxcar=0, comp_fir_size=9, buf_len=16384), 900),
}


def candidate(rng, k, kw):
    bin_e, ds = kw["bin_e"], kw.get("downsample", 1)
    kind = ("random", "centred", "coarse")[k % 3]
    if ds == 1:
        inc = (int(rng.integers(0, 1 << 32)) if kind == "random" else int(rng.integers(1, 1 << bin_e)) << (32 - bin_e) if kind == "centred"
               else int(rng.integers(1, 64)) << 26)
        lo, hi = ph.RAILS[0] if k % 4 else ph.RAILS[1 + (k // 4) % 2]  # three in four on the pair that wraps
    else:
        # a tone inside the decimated band: the increment behind the decimator is inc * ds
        e = (int(rng.integers(0, 1 << 31)) if kind == "random" else int(rng.integers(1, 1 << (bin_e - 1))) << (32 - bin_e) if kind == "centred"
             else int(rng.integers(1, 32)) << 26)
        inc = (e // ds) if k % 2 else ((1 << 32) - e // ds)
        a = 31 if kw.get("boxcar") else int(rng.integers(24, 32))
        lo, hi = 127 - a, 127 + a
    return dict(inc=inc & 0xFFFFFFFF, phase=int(rng.integers(0, 1 << 32)), lo=lo, hi=hi, kind=kind)


def centred(rec, kw):
    return (rec["inc"] * kw.get("downsample", 1)) % (1 << (32 - kw["bin_e"])) == 0


def lifted(rng, kw, s, tries=3000, most=6):
    """Candidates for a stage s the search above did not reach.  Stage s of a transform of 2^E points is the last stage of
    2^(E - s - 1) transforms of 2^(s + 1) points, each over every 2^(E - s - 1)-th sample: of the tone (inc << (E - s - 1),
    phase + o inc) for its offset o.  So the search runs at 2^(s + 1) points, where it costs little, over increments that
    are multiples of 2^(E - s - 1), and what wraps in the last stage there is shifted back (offset 0; the bits shifted out
    at the top are free).  Only remove_dc's average differs between the two, so the caller's model decides."""
    E, sh = kw["bin_e"], kw["bin_e"] - s - 1
    small = RtlpowerCfg.default(window=0, bin_e=s + 1, buf_len=2 << (s + 1))
    found = []
    for k in range(tries):
        inc = (int(rng.integers(1, 1 << (s + 1))) << (31 - s), int(rng.integers(0, 1 << (32 - sh))) << sh, int(rng.integers(1, 64)) << 26)[k % 3]
        rec = dict(inc=inc & 0xFFFFFFFF, phase=int(rng.integers(0, 1 << 32)), lo=0, hi=254, kind="lifted")
        n = int(ph.model_scan(small, ph.stream(rec, 1 << (s + 1)))[2][s])
        if n:
            found.append((n, k, rec))
    out = []
    for n, _, rec in sorted(found, key=lambda f: (-f[0], f[1]))[:most]:
        out.append(dict(rec, inc=(rec["inc"] >> sh) | (int(rng.integers(0, 1 << sh)) << (32 - sh)) if sh else rec["inc"]))
    return out


def cover(cands, wraps, stages):
    """Greedy: the candidate that wraps in the most stages not yet covered, until none adds one."""
    left, kept = set(stages), []
    while left:
        gain = [(len([s for s in left if wraps[i][s] > 0]), int(min([wraps[i][s] for s in left if wraps[i][s] > 0], default=0)), -i) for i in cands]
        n, _, neg = max(gain, default=(0, 0, 0))
        if n == 0:
            break
        kept.append(-neg)
        left -= {s for s in left if wraps[-neg][s] > 0}
    return kept, left


def main():
    out = {"seed": SEED, "reads": ph.READS, "cases": {}}
    for name, (kw, ncand) in CASES.items():
        rng = np.random.default_rng([SEED, len(out["cases"])])
        cfg = RtlpowerCfg.default(window=0, **kw)
        L, bin_e = int(cfg.buf_len), int(cfg.bin_e)
        recs = [candidate(rng, k, kw) for k in range(ncand)]
        wraps, big = [], None
        for i, rec in enumerate(recs):
            m = ph.model_scan(cfg, ph.stream(rec, L // 2))
            wraps.append(m[2])
            if m.big_bins and big is None:
                big = i
        stages = range(2, bin_e)
        for s in [s for s in stages if not any(w[s] for w in wraps)]:
            for rec in lifted(rng, kw, s):
                recs.append(rec)
                wraps.append(ph.model_scan(cfg, ph.stream(rec, L // 2))[2])
        ncand = len(recs)
        is_c = [centred(r, kw) for r in recs]
        if bin_e <= 14:
            keep_c, left_c = cover([i for i in range(ncand) if is_c[i]], wraps, stages)
            keep_o, left_o = cover([i for i in range(ncand) if not is_c[i]], wraps, stages)
        else:  # (the model takes a second per set there: one cover of all candidates)
            keep_c, left_c = cover(range(ncand), wraps, stages)
            keep_o, left_o = [], left_c
        keep = keep_c + [i for i in keep_o if i not in keep_c]
        if big is not None and big not in keep:
            keep.append(big)
        sets = []
        for i in keep:
            iq = ph.stream(recs[i], L // 2 * ph.READS)
            m = ph.model_scan(cfg, iq)
            sets.append(dict(recs[i], centred=bool(is_c[i]), wraps=[int(w) for w in m[2]], window_wraps=m.window_wraps,
                             big_bins=m.big_bins, sha256=ph.sha(iq)))
        hit = {s: [k for k, st in enumerate(sets) if st["wraps"][s] > 0] for s in stages}
        case = dict(cfg=kw, candidates=ncand, sets=sets, stages={str(s): hit[s] for s in stages if hit[s]},
                    missing=[s for s in stages if not hit[s]], missing_centred=sorted(left_c), missing_not_centred=sorted(left_o),
                    total_wraps=[int(sum(st["wraps"][s] for st in sets)) for s in range(bin_e)],
                    over_2_31=next((k for k, st in enumerate(sets) if st["big_bins"]), None))
        out["cases"][name] = case
        print(f"{name}: {len(sets)} sets ({len(keep_c)} centred), total wraps per stage {case['total_wraps']}, missing {case['missing']}, "
              f"centred miss {case['missing_centred']}, others miss {case['missing_not_centred']}, over 2^31 - 1: {case['over_2_31']}", flush=True)
    found = [name for name, c in out["cases"].items() if c["over_2_31"] is not None]
    out["over_2_31_found"] = found
    out["over_2_31_note"] = ("sets with a bin of |X|^2 > 2^31 - 1 (exactly 2^31: re = im = -32768): "
                             + (", ".join(found) if found else f"none among the {sum(n for _, n in CASES.values())} candidates and the lifted ones"))
    with open(ph.FIXTURE, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"{ph.FIXTURE}: {os.path.getsize(ph.FIXTURE)} bytes")


if __name__ == "__main__":
    main()
