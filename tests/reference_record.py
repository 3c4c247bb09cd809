"""The reference's own results for the tests that compare against it.

Where oracle/_ref is built (the reference compiled in place, oracle/Makefile) a test asks the live reference.  Everywhere
else it reads what the live reference returned for the same case from tests/golden/reference/results.npz, which
tests/golden/gen_reference_results.py writes by running those tests against the live reference.  Every test input comes
from a fixed seed; the record keeps a digest of the inputs of each case, so a case whose input is not the recorded one
fails instead of being compared with another input's result."""
import hashlib
import os

import numpy as np

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference", "results.npz")
RECORD_DIR_ENV = "RTLFM_RECORD_REFERENCE"  # set by gen_reference_results.py: where the live results of a run are collected

_record = None


def digest(*inputs) -> str:
    h = hashlib.sha256()
    for x in inputs:
        h.update(np.ascontiguousarray(x).tobytes() if isinstance(x, np.ndarray) else repr(x).encode())
    return h.hexdigest()


def _slot(key: str) -> str:
    return hashlib.sha256(key.encode()).hexdigest()[:20]


def result(live: bool, key: str, compute, inputs=()) -> dict:
    """`compute()` -> {name: array} from the live reference when `live`, else the recorded result of case `key`
    (fed the same `inputs`)."""
    global _record
    d = digest(*inputs)
    if live:
        res = {k: np.asarray(v) for k, v in compute().items()}
        out_dir = os.environ.get(RECORD_DIR_ENV)
        if out_dir:
            np.savez(os.path.join(out_dir, _slot(key) + ".npz"), **{f"{_slot(key)}.{k}": v for k, v in res.items()},
                     **{f"{_slot(key)}.__inputs__": np.array(d)})
        return res
    if _record is None:
        _record = np.load(RECORD)
    s = _slot(key)
    assert f"{s}.__inputs__" in _record.files, f"{key}: no result of the reference recorded (tests/golden/gen_reference_results.py)"
    assert str(_record[f"{s}.__inputs__"]) == d, f"{key}: the inputs differ from those the recorded result was computed from"
    return {n[len(s) + 1:]: _record[n] for n in _record.files if n.startswith(s + ".") and not n.endswith(".__inputs__")}
