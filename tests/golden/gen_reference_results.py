#!/usr/bin/env python3
"""Write tests/golden/reference/results.npz: what the live reference returned for every case of the tests that compare
against it (tests/reference_record.py), so that those tests run where oracle/_ref cannot be built.

Needs oracle/_ref (oracle/Makefile builds it where the reference's sources are).  Runs those test modules against the
live reference with RTLFM_RECORD_REFERENCE pointing at a temporary directory, then merges what they wrote.  The
record is data only: outputs, carried states, planner answers and digests of the inputs, no reference source text.

    python tests/golden/gen_reference_results.py
"""
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import reference_record as rr  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

MODULES = ["tests/test_oracle_golden.py", "tests/test_power_oracle.py", "tests/test_capi_symbols.py", "tests/test_device_shim.py",
           "tests/test_power_hard_cpu.py"]


def main():
    po.build()
    assert po.have_reference() and po.have_power_reference(), "oracle/_ref not built (the reference's sources are not here)"
    with tempfile.TemporaryDirectory() as d:
        env = dict(os.environ, **{rr.RECORD_DIR_ENV: d})
        subprocess.check_call([sys.executable, "-m", "pytest", "-q", "-m", "not gpu", "-p", "no:cacheprovider"] + MODULES,
                              cwd=ROOT, env=env)
        merged = {}
        for f in sorted(glob.glob(os.path.join(d, "*.npz"))):
            with np.load(f) as z:
                merged.update({k: z[k] for k in z.files})
    np.savez_compressed(rr.RECORD, **merged)
    print(f"{rr.RECORD}: {sum(k.endswith('.__inputs__') for k in merged)} cases, {os.path.getsize(rr.RECORD)} bytes")


if __name__ == "__main__":
    main()
