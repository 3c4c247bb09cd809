"""The input-health model without a GPU: the vectorised twin (tests/health_model.py) against the literal loops, and the
split of underrun_test() into per-buffer records plus the engine's junction term against one call per buffer with the
static counter carried."""
import numpy as np
import pytest

import health_model as hm
from rtlsdr_amd import synth


def inputs(L, seed):
    rng = np.random.default_rng(seed)
    cnt = hm.counter((1, L), start=int(rng.integers(0, 256)))
    return {
        "random": synth.random_u8(1, L, seed=seed)[0],
        "fm": synth.fm_iq_u8(1, L // 2, amplitude=100.0, seed=seed)[0],
        "counter": cnt[0],
        "gaps": hm.plant_gaps(cnt, L)[0],
        "values": hm.plant_values(np.full((1, L), 127, dtype=np.uint8), L)[0],
        "all0": np.zeros(L, dtype=np.uint8),
        "all255": np.full(L, 255, dtype=np.uint8),
        "all127": np.full(L, 127, dtype=np.uint8),
    }


@pytest.mark.parametrize("L", [512, 7680, 8192, 16896, 262144])
def test_twin_equals_loops(L):
    for kind, buf in inputs(L, seed=L).items():
        if L == 262144 and kind not in ("random", "gaps"):
            continue  # the loops are slow: the long buffer on the two inputs that stress every term
        got = hm.records(buf)
        assert tuple(got.tolist()) == hm.record_loop(buf), kind
        assert hm.detect_overload_loop(buf) == (8000 * int(got["overload"]) >= L), kind
    assert int(hm.records(inputs(L, 1)["counter"])["lost"]) == 0
    z = hm.records(np.zeros(L, dtype=np.uint8))
    assert (int(z["overload"]), int(z["high"]), int(z["lost"])) == (L, L, L - 1)  # every byte overloads; 0 after 0 loses 1


def test_wrap_is_continuity():
    assert int(hm.records(np.array([254, 255, 0, 1], dtype=np.uint8))["lost"]) == 0
    assert int(hm.records(np.array([255, 1], dtype=np.uint8))["lost"]) == 1
    assert int(hm.records(np.array([0, 255], dtype=np.uint8))["lost"]) == 254
    assert hm.record_loop(np.array([0, 255], dtype=np.uint8))[2] == 254


@pytest.mark.parametrize("kind", ["random", "gaps", "counter"])
def test_every_split_into_buffers(kind):
    """For EVERY split of a byte sequence into buffers: records + junction terms == one underrun_test call per buffer."""
    n = 9
    seq = {"random": synth.random_u8(1, n, seed=3)[0], "counter": hm.counter((1, n), 250)[0],
           "gaps": np.array([250, 251, 253, 254, 255, 0, 0, 2, 1], dtype=np.uint8)}[kind]
    for mask in range(1 << (n - 1)):  # bit i set: a buffer boundary after byte i
        cuts = [0] + [i + 1 for i in range(n - 1) if mask >> i & 1] + [n]
        bufs = [seq[a:b] for a, b in zip(cuts, cuts[1:])]
        ref = hm.Underrun()
        per_call = [ref.call(b) for b in bufs]
        eng = hm.StreamModel(0, 4)
        before = 0
        for b, want in zip(bufs, per_call):
            eng.feed(hm.records(b), len(b))
            assert eng.dropped_samples - before == want, (mask, cuts)
            before = eng.dropped_samples
        assert (eng.total_samples, eng.dropped_samples) == (ref.total_samples, ref.dropped_samples)


def test_longer_random_splits():
    rng = np.random.default_rng(11)
    seq = hm.plant_gaps(hm.counter((1, 4096), 200), 4096)[0]
    seq[1000:1100] = rng.integers(0, 256, 100)
    for _ in range(50):
        cuts = [0] + sorted(set(rng.integers(1, 4096, rng.integers(1, 12)).tolist())) + [4096]
        ref, eng = hm.Underrun(), hm.StreamModel(0, 4)
        for a, b in zip(cuts, cuts[1:]):
            ref.call(seq[a:b])
            eng.feed(hm.records(seq[a:b]), b - a)
        assert eng.dropped_samples == ref.dropped_samples
