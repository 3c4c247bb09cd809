#!/usr/bin/env python3
"""Write tests/golden/tail_hard.json: per row of tests/tail_hard.py's case table the stream parameters and a digest of
their bytes, the configuration as the planner completed it, what the counting model saw - stores outside the stored type per
stage, the largest |x - avg| deemph_filter divided, the peak, the share of flagged resampler outputs, the output length of every
buffer - and a digest of the oracle's output and of the state it carried.  Records, no samples.

A row is written only if the model equals the oracle on it in every sample and carried field and at most
tail_hard.FLAG_CAP of its resampled outputs are flagged: a row over the cap is replaced in the table by another ratio of
its class, not recorded.

    python tests/golden/gen_tail_hard.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tail_hard as th  # noqa: E402
from oracle import pyoracle as po  # noqa: E402


def record(c):
    cfg, iq, st = th.build(po, c)
    want, want_len, wst = po.run_batch(cfg, iq, states=th.copy_states(st) if st else None, nthreads=4)
    res = th.model_case(po, c, cfg, iq)
    for s, (out, mst, _, _, lens) in enumerate(res):
        assert sum(lens) == want_len[s] and np.array_equal(out, want[s, :want_len[s]]), (c["name"], s)
        got = wst[s].as_dict()
        assert all(got[f] == mst[f] for f in th.TAIL_STATE), (c["name"], s, got, mst)
    t = th.totals(res)
    share = t["flagged"] / t["outputs"] if t["outputs"] else 0.0
    assert share <= th.FLAG_CAP, (c["name"], share)
    lens = [r[4] for r in res]
    rows = [list(x) for x in dict.fromkeys(tuple(l) for l in lens)]
    return dict(klass=c["klass"], uniform=c["uniform"], output_scale=int(cfg.output_scale), streams=len(iq),
                stream_set=th.stream_set_name(c), stream_sha256=[th.sha(row) for row in iq],
                wraps={k: int(t[k]) for k in th.WRAPS + ("deemph_store",)}, max_d=int(t["max_d"]), peak=int(t["peak"]),
                outputs=int(t["outputs"]), flagged=int(t["flagged"]), flagged_share=round(share, 6),
                lens=dict(rows=rows, of_stream=[rows.index(list(l)) for l in lens]),
                out_sha256=th.sha(np.concatenate([want[s, :want_len[s]] for s in range(len(iq))])),
                state_sha256=th.sha(np.frombuffer(b"".join(bytes(wst[s]) for s in range(len(iq))), dtype=np.uint8)))


def dumps(obj, depth=0):
    """json with the innermost containers - lists of scalars, small dicts of scalars - on one line."""
    pad = " " * (depth + 1)
    flat = lambda v: not isinstance(v, (list, dict))  # noqa: E731
    if isinstance(obj, dict) and not all(flat(v) for v in obj.values()) or isinstance(obj, dict) and depth < 2:
        return "{\n" + ",\n".join(f"{pad}{json.dumps(k)}: {dumps(v, depth + 1)}" for k, v in obj.items()) + "\n" + " " * depth + "}"
    if isinstance(obj, list) and not all(flat(v) for v in obj):
        return "[\n" + ",\n".join(pad + dumps(v, depth + 1) for v in obj) + "\n" + " " * depth + "]"
    return json.dumps(obj)


def main():
    po.build()
    out = {"flag_cap": th.FLAG_CAP, "stream_sets": th.STREAM_SETS, "cases": {}}
    for c in th.CASES:
        out["cases"][c["name"]] = r = record(c)
        print(f"{c['name']:28s} {r['klass']:18s} scale {r['output_scale']:3d} wraps {dict((k, v) for k, v in r['wraps'].items() if v)} max_d {r['max_d']} "
              f"peak {r['peak']} flagged {r['flagged']}/{r['outputs']} lens {r['lens']['rows'][0]}", flush=True)
    with open(th.FIXTURE, "w") as f:
        f.write(dumps(out) + "\n")
    print(f"{th.FIXTURE}: {os.path.getsize(th.FIXTURE)} bytes")


if __name__ == "__main__":
    main()
