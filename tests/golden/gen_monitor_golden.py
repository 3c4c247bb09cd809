#!/usr/bin/env python3
"""Writes tests/golden/monitor/accumulators.npz: the reference's own callback / full_demod accumulators (sampleMax,
samplePowSum, samplePowCount, levelSum, numSummed) for the inputs of tests/test_monitor_cpu.py, from the LIVE
reference (oracle/_ref must be built), with a digest of those inputs - as tests/reference_record.py keeps one - so that
a test whose inputs are not the recorded ones fails instead of being compared with another input's result.

    python tests/golden/gen_monitor_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import monitor_model as mm
    import test_monitor_cpu as t
    from oracle import pyoracle as po
    po.build()
    if not po.have_reference():
        raise SystemExit("oracle/_ref is not built: no live reference to record from")
    acc = t.live_accumulators(po)
    os.makedirs(os.path.dirname(mm.GOLDEN), exist_ok=True)
    np.savez(mm.GOLDEN, accumulators=acc, inputs=np.array(t.input_digest()), lengths=np.array(mm.ACC_LENGTHS))
    print(f"{mm.GOLDEN}: {acc.shape[0]} block lengths")


if __name__ == "__main__":
    main()
