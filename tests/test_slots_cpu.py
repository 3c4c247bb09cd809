"""The channel bank's slot allocator (include/rtlfm_slots.h, csrc/slots.cpp, rtlsdr_amd/slots.py) against
tests/slots_model.py: host code, integers only, no GPU.  Seeded random power sequences, then the rules one by one; and
tools/slots_check.cpp, the same engine as a stand-alone program under AddressSanitizer + UBSan."""
import ctypes as C
import errno
import os
import shutil
import subprocess

import numpy as np
import pytest

from rtlsdr_amd import build as hipbuild
from rtlsdr_amd import capi
from slots_model import SlotsModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    hipbuild.build()
    return capi.load()


def both(lib, nsources, K, slots, **kw):
    from rtlsdr_amd.slots import SlotAllocator
    return SlotAllocator(nsources, K, slots, **kw), SlotsModel(nsources, K, slots, **kw)


def assert_same(eng, model, what):
    assert eng.bins().tolist() == model.bins(), what
    assert eng.idle().tolist() == model.idle(), what
    assert eng.events() == model.events, what


def step_both(eng, model, power, frames, what=""):
    eng.step(np.asarray(power, dtype=np.uint64), np.asarray(frames, dtype=np.int32))
    model.step(power, frames)
    assert_same(eng, model, what)


@pytest.mark.parametrize("seed", range(12))
def test_random_sequences_equal_the_model(lib, seed):
    rng = np.random.default_rng(4800 + seed)
    N, K, S = int(rng.integers(1, 5)), int(rng.integers(1, 40)), int(rng.integers(1, 7))
    open_level = int(rng.integers(1, 2000))
    close_level = int(rng.integers(0, open_level + 1))
    kw = dict(open_level=open_level, close_level=close_level, hang=int(rng.integers(0, 4)), park=int(rng.integers(0, K)),
              mask=(rng.integers(0, 5, size=K) == 0).astype(np.uint8) if seed % 3 else None)
    eng, model = both(lib, N, K, S, **kw)
    changes = 0
    with eng:
        assert_same(eng, model, "fresh")
        for st in range(60):
            frames = np.where(rng.integers(0, 6, size=N) == 0, 0, rng.integers(1, 300, size=N)).astype(np.int32)
            fr = np.maximum(frames, 1)[:, None].astype(np.uint64)
            kind = rng.integers(0, 8, size=(N, K)) * (rng.integers(0, 3, size=(N, 1)) > 0)  # (a source in three: all quiet)
            quiet = (rng.integers(0, 1 << 62, size=(N, K)).astype(np.uint64)) % (np.uint64(close_level) * fr + np.uint64(1))
            power = np.where(kind < 3, quiet, np.where(kind == 3, np.uint64(open_level) * fr, np.where(
                kind == 4, np.uint64(close_level) * fr, np.uint64(open_level) * fr + rng.integers(0, 3, size=(N, K)).astype(np.uint64))))
            step_both(eng, model, power.astype(np.uint64), frames, (seed, st))
            changes += len(model.events)
    assert changes >= 4, changes  # (the generator's own check: the sequence did bind and free slots)


def test_a_tie_in_power_goes_to_the_lower_bin(lib):
    eng, model = both(lib, 1, 8, 2, open_level=10, close_level=5)
    with eng:
        step_both(eng, model, [[0, 0, 50, 70, 70, 50, 70, 0]], [1])
        assert eng.bins().tolist() == [[3, 4]]
        assert eng.events() == [dict(source=0, slot=0, old_bin=-1, new_bin=3), dict(source=0, slot=1, old_bin=-1, new_bin=4)]


def test_a_bound_slot_is_never_moved_by_a_louder_candidate(lib):
    eng, model = both(lib, 1, 8, 2, open_level=10, close_level=5)
    with eng:
        step_both(eng, model, [[0, 20, 0, 30, 0, 0, 0, 0]], [1])
        assert eng.bins().tolist() == [[3, 1]]
        step_both(eng, model, [[0, 20, 9000, 30, 0, 9000, 0, 0]], [1])
        assert eng.bins().tolist() == [[3, 1]] and eng.events() == []


@pytest.mark.parametrize("hang", [0, 1, 3])
def test_release_happens_exactly_after_hang_plus_one_quiet_runs(lib, hang):
    eng, model = both(lib, 1, 4, 1, open_level=100, close_level=40, hang=hang, park=2)
    loud, between, quiet = [[0, 100, 0, 0]], [[0, 40, 0, 0]], [[0, 39, 0, 0]]
    with eng:
        step_both(eng, model, loud, [1])
        assert eng.bins().tolist() == [[1]]
        for _ in range(hang):  # quiet runs that an at-or-above-close run interrupts do not add up
            step_both(eng, model, quiet, [1])
        step_both(eng, model, between, [1])
        for k in range(hang + 1):
            assert eng.bins().tolist() == [[1]] and not eng.idle().any(), k
            step_both(eng, model, quiet, [1])
        assert eng.idle().tolist() == [[True]] and eng.bins().tolist() == [[2]]  # (park)
        assert eng.events() == [dict(source=0, slot=0, old_bin=1, new_bin=-1)]


def test_frames_zero_freezes_a_source(lib):
    eng, model = both(lib, 2, 4, 1, open_level=10, close_level=10, hang=0)
    with eng:
        step_both(eng, model, [[0, 50, 0, 0], [0, 0, 50, 0]], [2, 2])
        assert eng.bins().tolist() == [[1], [2]]
        # source 0 delivers nothing: neither its silence frees the slot nor its loud bin 3 could bind; source 1 lives on
        step_both(eng, model, [[0, 0, 0, 9999], [0, 0, 0, 0]], [0, 2])
        assert eng.bins().tolist() == [[1], [0]] and eng.idle().tolist() == [[False], [True]]
        assert eng.events() == [dict(source=1, slot=0, old_bin=2, new_bin=-1)]


def test_a_freed_slot_is_bound_again_in_the_same_step_as_one_change(lib):
    eng, model = both(lib, 1, 4, 1, open_level=10, close_level=10, hang=0)
    with eng:
        step_both(eng, model, [[0, 50, 0, 0]], [1])
        step_both(eng, model, [[0, 0, 0, 60]], [1])
        assert eng.events() == [dict(source=0, slot=0, old_bin=1, new_bin=3)]


def test_masked_bins_are_never_assigned(lib):
    eng, model = both(lib, 1, 4, 2, open_level=10, close_level=5, mask=[1, 0, 0, 1], park=0)
    with eng:
        step_both(eng, model, [[9999, 20, 0, 9999]], [1])
        assert eng.bins().tolist() == [[1, 0]] and eng.idle().tolist() == [[False, True]]


def test_refusals(lib):
    def create(n, K, s, **kw):
        cfg = capi.RtlfmSlotsCfg(kw.get("open_level", 10), kw.get("close_level", 5), kw.get("hang", 0), kw.get("park", 0), None)
        a = C.c_void_p()
        r = lib.rtlfm_slots_create(n, K, s, C.byref(cfg), C.byref(a))
        if r == 0:
            lib.rtlfm_slots_destroy(a)
        else:
            assert a.value is None
        return r
    assert create(1, 4, 1) == 0
    assert create(1, 4, 1, close_level=11) == -errno.EINVAL
    assert create(1, 4, 1, close_level=10) == 0  # (close == open is allowed)
    for bad in (dict(park=4), dict(park=-1), dict(hang=-1)):
        assert create(1, 4, 1, **bad) == -errno.EINVAL, bad
    for n, K, s in ((0, 4, 1), (1, 0, 1), (1, 4, 0), (-1, 4, 1), (1, -4, 1), (1, 4, -1)):
        assert create(n, K, s) == -errno.EINVAL, (n, K, s)
    a = C.c_void_p()
    assert lib.rtlfm_slots_create(1, 4, 1, None, C.byref(a)) == -errno.EINVAL
    eng, model = both(lib, 1, 4, 1, open_level=10, close_level=5)
    with eng:
        step_both(eng, model, [[0, 50, 0, 0]], [1])
        p = np.zeros(4, dtype=np.uint64)
        f = np.array([-1], dtype=np.int32)
        assert lib.rtlfm_slots_step(eng._a, p.ctypes.data, f.ctypes.data) == -errno.EINVAL
        assert lib.rtlfm_slots_step(eng._a, None, f.ctypes.data) == -errno.EINVAL
        assert_same(eng, model, "after the refused steps")  # (nothing changed, the last step's events included)
        n = C.c_int()
        assert lib.rtlfm_slots_events(eng._a, None, 0, C.byref(n)) == -errno.ENOBUFS and n.value == 1


def test_levels_near_two_to_the_63_do_not_overflow_the_comparison(lib):
    """open * frames passes 2^64 here: a comparison in 64 bits would wrap and find every bin loud."""
    top = (1 << 63) - 1
    eng, model = both(lib, 1, 4, 2, open_level=top, close_level=top - 1, hang=0)
    with eng:
        step_both(eng, model, [[top, top - 1, (1 << 64) - 1, 5]], [1])
        assert eng.bins().tolist() == [[2, 0]]
        # two frames: level * frames = 2^64 - 2 and 2^64 - 4 - bin 2 at 2^64 - 1 stays, bin 0 at 2^63 - 1 is far below close
        step_both(eng, model, [[top, 5, (1 << 64) - 1, (1 << 64) - 3]], [2])
        assert eng.bins().tolist() == [[2, 0]] and eng.idle().tolist() == [[False, True]]
        # three frames: 3 (2^63 - 2) > 2^64 - no uint64 reaches it
        step_both(eng, model, [[(1 << 64) - 1] * 4], [3])
        assert eng.idle().all()


def test_slots_symbols_are_exported(lib):
    for name in capi.DECLARED_SLOTS_SYMBOLS:
        assert hasattr(lib, name), name
    text = open(os.path.join(ROOT, "include", "rtlfm_slots.h")).read()
    for name in capi.DECLARED_SLOTS_SYMBOLS:
        assert name + "(" in text, name


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not on PATH")
def test_slots_check_under_the_sanitizers(tmp_path):
    """tools/slots_check.cpp with csrc/slots.cpp, AddressSanitizer + UBSan, as a program of its own on the CPU."""
    exe = str(tmp_path / "slots_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tools", "slots_check.cpp"),
                           os.path.join(hipbuild.CSRC, "slots.cpp")])
    r = subprocess.run([exe, "7", "200"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("slots_check: ok"), r.stdout
