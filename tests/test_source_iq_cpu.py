"""IQ balance per source on the CPU: the engine of include/rtlfm_iq.h (csrc/iq.cpp, rtlsdr_amd/iq.py) against
tests/source_iq_model.py - int16 coefficients equal, not close - every rule of it, what the correction is worth on a
mismatched front end, the exported symbols, and tools/iq_check.cpp under the sanitizers.  No GPU: the device half is
tests/test_source_iq_gpu.py."""
import ctypes as C
import errno
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import source_iq_model as model
from rtlsdr_amd import build as hipbuild
from rtlsdr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def iq():
    hipbuild.build()
    from rtlsdr_amd import iq as mod
    return mod


def record_of(total):
    r = np.zeros((), dtype=capi.IQ_SUMS_DTYPE)
    for k in ("n", "si", "sq", "sii", "sqq", "siq"):
        r[k] = total[k]
    return r


def random_buffer(rng, n, spread, g, s, dc=(0.0, 0.0)):
    """n samples: independent x, y0 uniform in +-spread, y = g (y0 + s x), bytes with the offsets dc."""
    x = rng.integers(-spread, spread + 1, size=n).astype(np.float64)
    y0 = rng.integers(-spread, spread + 1, size=n).astype(np.float64)
    y = g * (y0 + s * x)
    out = np.empty(2 * n)
    out[0::2] = np.rint(x + 127 + dc[0])
    out[1::2] = np.rint(y + 127 + dc[1])
    return np.clip(out, 0, 255).astype(np.uint8)


def test_the_model_and_the_header_agree_on_the_record():
    assert model.SUMS_DTYPE == capi.IQ_SUMS_DTYPE and np.dtype(capi.IQ_SUMS_DTYPE).itemsize == 48
    assert C.sizeof(capi.RtlfmIqEvent) == 32
    assert (model.OK, model.WEAK, model.REJECTED) == (capi.IQ_OK, capi.IQ_WEAK, capi.IQ_REJECTED)
    assert (model.CHANGED, model.REJECTED_EVENT) == (capi.IQ_EVENT_CHANGED, capi.IQ_EVENT_REJECTED)


def test_model_apply_identity_and_clamp():
    rng = np.random.default_rng(1)
    b = rng.integers(0, 256, size=(3, 4096), dtype=np.uint8)
    out, clipped = model.apply(b, model.IDENTITY)
    assert np.array_equal(out, b) and not clipped.any()
    # q = 20480 (1.25) on full-scale bytes: Q = 255 -> 128 * 1.25 + 127 = 287, Q = 0 -> -159 + 127 < 0; I untouched
    fs = np.zeros(1024, dtype=np.uint8)
    fs[1::4] = 255
    fs[0::2] = 127
    out, clipped = model.apply(fs, (16384, 0, 0, 20480))
    assert np.array_equal(out[0::2], fs[0::2]) and clipped == 512 and set(out[1::2].tolist()) == {0, 255}
    # one set of coefficients per row
    two, _ = model.apply(b[:2], [(16384, 0, 0, 16384), (8192, 0, 0, 16384)])
    assert np.array_equal(two[0], b[0]) and not np.array_equal(two[1], b[1])
    s = model.sums(b)
    assert s.shape == (3,) and (s["n"] == 2048).all() and int(s["si"][0]) == int(b[0, 0::2].astype(np.int64).sum())


def test_compute_equals_the_model_on_random_totals(iq):
    """Seeded random windows over the whole range of gain and skew (the rejected and the weak among them), with DC offsets:
    verdict, int16 coefficients and the Q14 estimates are equal."""
    rng = np.random.default_rng(2024)
    seen = {model.OK: 0, model.WEAK: 0, model.REJECTED: 0}
    identities = 0
    for k in range(400):
        g, s = rng.uniform(0.3, 2.6), rng.uniform(-0.8, 0.8)
        if k % 5 == 0:
            g, s = 1.0 + rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02)  # around the deadband
        spread = int(rng.choice([0, 1, 2, 3, 10, 40, 100]))
        n = int(rng.integers(1, 40)) * 256
        buf = random_buffer(rng, n, spread, g, s, dc=(rng.uniform(-3, 3), rng.uniform(-3, 3)))
        t = model.total_of(model.sums(buf))
        deadband, min_rms = int(rng.choice([0, 164, 400])), int(rng.choice([0, 2, 5]))
        want = model.compute(t, deadband, min_rms)
        got = iq.compute(record_of(t), deadband, min_rms)
        seen[want[0]] += 1
        identities += want[1] == model.IDENTITY
        if want[0] == model.WEAK:
            assert got[0] == capi.IQ_WEAK, (k, t)
        else:
            assert got == want, (k, g, s, t, got, want)
    assert min(seen.values()) > 10 and identities > 10, (seen, identities)


def test_compute_on_totals_at_the_edge_of_the_integers(iq):
    """Totals as large as a window of 4096 longest buffers leaves them: A passes 2^64, so a 64-bit product would wrap."""
    n = 1 << 29
    t = dict(n=n, si=127 * n, sq=130 * n, sii=(127 * 127 + 900) * n, sqq=(130 * 130 + 625) * n, siq=(127 * 130 + 75) * n)
    assert n * t["sii"] - t["si"] ** 2 > 1 << 64
    want = model.compute(t)
    assert want[0] == model.OK and want[1] != model.IDENTITY
    assert iq.compute(record_of(t)) == want


def test_every_rule_of_compute(iq):
    rng = np.random.default_rng(3)
    # weak: one of the two branches below min_rms (spread 1: rms < 1), and no samples at all
    quiet = model.total_of(model.sums(random_buffer(rng, 4096, 1, 1.0, 0.0)))
    assert model.compute(quiet)[0] == model.WEAK and iq.compute(record_of(quiet))[0] == capi.IQ_WEAK
    assert model.compute(quiet, min_rms=0)[0] == model.OK and iq.compute(record_of(quiet), min_rms=0)[0] == capi.IQ_OK
    empty = dict.fromkeys(("n", "si", "sq", "sii", "sqq", "siq"), 0)
    assert iq.compute(record_of(empty), min_rms=0)[0] == capi.IQ_WEAK
    # rejected: g outside [0.5, 2], |s| > 0.5 - the estimates are reported, the coefficients are not
    for g, s in ((0.4, 0.0), (2.4, 0.0), (1.0, 0.9), (1.0, -0.9)):
        t = model.total_of(model.sums(random_buffer(rng, 8192, 40, g, s)))
        want = model.compute(t)
        assert want[0] == model.REJECTED and want[1] is None and want[2] is not None, (g, s)
        assert iq.compute(record_of(t)) == want
    # the deadband turns a balanced front end into the identity; without it the estimate is a few counts off
    t = model.total_of(model.sums(random_buffer(rng, 65536, 60, 1.0, 0.0)))
    assert iq.compute(record_of(t)) == model.compute(t) and model.compute(t)[1] == model.IDENTITY
    near = model.compute(t, deadband=0)[1]
    assert near != model.IDENTITY and max(abs(a - b) for a, b in zip(near, model.IDENTITY)) < 164
    assert iq.compute(record_of(t), deadband=0)[1] == near
    # both branches: gc < 1 scales I down, gc >= 1 scales Q down; b = 0 and nothing is amplified
    for g, s in ((0.8, 0.17), (1.25, -0.12)):
        coef = model.compute(model.total_of(model.sums(random_buffer(rng, 65536, 60, g, s))))[1]
        assert coef[1] == 0 and max(coef[0], coef[3]) == 16384 and min(coef[0], coef[3]) < 16384 - 164, (g, coef)
        assert (coef[0] < 16384) == (g < 1), (g, coef)
    # refusals
    lib = capi.load()
    out = np.zeros(4, dtype=np.int16)
    r = record_of(t)
    assert lib.rtlfm_iq_compute(None, 164, 2, out.ctypes.data, None, None) == -errno.EINVAL
    assert lib.rtlfm_iq_compute(r.ctypes.data, 164, 2, None, None, None) == -errno.EINVAL
    assert lib.rtlfm_iq_compute(r.ctypes.data, -1, 2, out.ctypes.data, None, None) == -errno.EINVAL
    assert lib.rtlfm_iq_compute(r.ctypes.data, 164, 129, out.ctypes.data, None, None) == -errno.EINVAL
    assert lib.rtlfm_iq_compute(r.ctypes.data, 164, 2, out.ctypes.data, None, None) == 0  # (g_q14 / s_q14 may be NULL)


def drifting_records(rng, nsrc, nbuf, L=4096):
    """Per source a sequence of buffers whose mismatch moves in steps, with quiet and absurd stretches and short buffers
    mixed in: records [nsrc] lists."""
    out = []
    for a in range(nsrc):
        recs, g, s = [], 1.0, 0.0
        for b in range(nbuf):
            if b % 7 == 0:
                g, s = float(rng.choice([1.0, 0.8, 0.805, 1.25, 0.45, 1.001])), float(rng.choice([0.0, 0.17, -0.12, 0.174, 0.8]))
            spread = 1 if (b // 5) % 4 == 3 else 50
            n = (512 if b % 3 == 1 else L) // 2
            recs.append(model.sums(random_buffer(rng, n, spread, g, s, dc=(0.4 * a, -0.4))))
        out.append(np.array(recs, dtype=capi.IQ_SUMS_DTYPE))
    return out


@pytest.mark.parametrize("params", [dict(), dict(window=3, deadband=100, min_rms=1, min_step=0), dict(window=1, min_step=300),
                                    dict(window=5, deadband=0, min_rms=0, min_step=8)], ids=["defaults", "w3", "w1-step300", "w5-open"])
def test_engine_equals_the_model_on_sequences(iq, params):
    """Records fed in pieces of every size: events (kind, coefficients, estimates, window number) and the coefficients after
    every piece are the model's.  The sequences hold weak and rejected windows, changes below min_step and short buffers."""
    rng = np.random.default_rng(77)
    nsrc, nbuf = 3, 140
    recs = drifting_records(rng, nsrc, nbuf)
    m = model.Engine(nsrc, **params)
    kinds = set()
    with iq.IqBalance(nsrc, **params) as e:
        assert np.array_equal(e.coeffs(), m.coeffs())
        at = 0
        while at < nbuf:
            k = int(rng.integers(1, 9))
            for a in range(nsrc):
                e.feed(a, recs[a][at:at + k])
                m.feed(a, recs[a][at:at + k])
            at += k
            got, want = e.poll(), m.poll()
            assert got == want, (at, got, want)
            kinds |= {ev["kind"] for ev in want}
            assert np.array_equal(e.coeffs(), m.coeffs()), at
    assert kinds == {model.CHANGED, model.REJECTED_EVENT}, kinds


def test_min_step_and_window_rules(iq):
    rng = np.random.default_rng(9)
    a = model.sums(random_buffer(rng, 32768, 60, 0.8, 0.17))
    b = a.copy()
    b["sqq"] += np.uint64(32768 // 2)  # the same front end a little later (Q's variance up by 0.5 of about 800): below min_step
    ca, cb = model.compute(model.total_of(a))[1], model.compute(model.total_of(b))[1]
    assert ca != cb and max(abs(x - y) for x, y in zip(ca, cb)) <= 8, (ca, cb)
    with iq.IqBalance(1, window=2) as e:
        e.feed(0, [a])
        assert e.poll() == [] and e.coeffs().tolist() == [list(model.IDENTITY)]  # half a window decides nothing
        e.feed(0, [a])
        ev = e.poll()
        assert len(ev) == 1 and ev[0]["kind"] == capi.IQ_EVENT_CHANGED and ev[0]["window_serial"] == 0
        first = e.coeffs().tolist()
        e.feed(0, [b, b])
        assert e.poll() == [] and e.coeffs().tolist() == first  # within min_step: the old coefficients stay, no event
        e.set_params(window=2, min_step=0)
        e.feed(0, [b, b])
        ev = e.poll()
        assert len(ev) == 1 and ev[0]["window_serial"] == 2 and e.coeffs().tolist() != first
        # set_params starts windows over: one buffer fed before it does not count
        e.feed(0, [a])
        e.set_params(window=2, min_step=0)
        e.feed(0, [a])
        assert e.poll() == []
        # refusals change nothing
        lib = capi.load()
        for bad in ((0, 164, 2, 8), (4097, 164, 2, 8), (2, -1, 2, 8), (2, 164, -1, 8), (2, 164, 129, 8), (2, 164, 2, -1)):
            assert lib.rtlfm_iq_set_params(e._e, *bad) == -errno.EINVAL, bad
        e.feed(0, [a])
        assert len(e.poll()) == 1
        z = np.zeros(1, dtype=capi.IQ_SUMS_DTYPE)
        assert lib.rtlfm_iq_feed(e._e, 0, z.ctypes.data, 1) == -errno.EINVAL       # n == 0
        assert lib.rtlfm_iq_feed(e._e, 1, a.reshape(1).ctypes.data, 1) == -errno.EINVAL
        assert lib.rtlfm_iq_update(e._e, None) == -errno.EINVAL
    h = C.c_void_p()
    assert capi.load().rtlfm_iq_create(0, C.byref(h)) == -errno.EINVAL and h.value is None


IMAGE_CASES = [  # (g, phi, samples, before dB, after dB) as this model gives them with seed 5
    (0.8, 10.0, 131072, 17.0, 42.7),
    (1.25, -7.0, 131072, 17.9, 42.8),
    (0.8, 10.0, 2048, 17.1, 45.2),
]


@pytest.mark.parametrize("g, phi, n, before_want, after_want", IMAGE_CASES, ids=["g0.8-phi10", "g1.25-phi-7", "2048-samples"])
def test_image_rejection(iq, g, phi, n, before_want, after_want):
    """A carrier of amplitude 60 at bin 37 of 256 with noise of sigma 4 through a front end with gain g and phase error phi
    on Q, bytes rint(v + 127.4): the ratio of bin 37 to its mirror bin 219 over Hann-windowed 256-point frames.

    This model, seed 5: g = 0.8, phi = 10 deg: coefficients (12912, 0, -2284, 16384), 17.0 dB before and 42.7 dB after;
    g = 1.25, phi = -7 deg: (16384, 0, 2001, 13203), 17.9 -> 42.8 dB; 2048 samples: (12915, 0, -2238, 16384), 17.1 -> 45.2 dB.  Asserted: after >= before + 20 dB, and both
    figures within 5 dB below what is written here (seeds move the noise in the image bin by a few dB)."""
    buf = model.image_signal(n=n, g=g, phi_deg=phi, seed=5)
    before = model.image_ratio_db(buf)
    t = model.total_of(model.sums(buf.reshape(-1, 512)))
    verdict, coef, _, _ = iq.compute(record_of(t))
    assert verdict == capi.IQ_OK and coef == model.compute(t)[1]
    out, clipped = model.apply(buf, coef)
    after = model.image_ratio_db(out)
    print(f"g={g} phi={phi} n={n}: coef {coef}, image ratio {before:.1f} dB -> {after:.1f} dB, clipped {int(clipped)}")
    if (g, phi, n) == (0.8, 10.0, 131072):
        assert coef == (12912, 0, -2284, 16384)
    assert clipped == 0
    assert after >= before + 20.0, (before, after)
    assert abs(before - before_want) < 1.0 and after >= after_want - 5.0, (before, after)


def test_a_balanced_front_end_is_left_alone(iq):
    """g = 1, phi = 0: the estimate is (16384, 0, -10, 16381) with seed 5 - the rounding of a carrier that repeats every 256
    samples does not average out -, far inside the deadband of 164, which makes it the identity; the image ratio stays
    where the noise puts it (42.8 dB with seed 5)."""
    buf = model.image_signal(g=1.0, phi_deg=0.0, seed=5)
    t = model.total_of(model.sums(buf))
    near = iq.compute(record_of(t), deadband=0)[1]
    assert max(abs(a - b) for a, b in zip(near, model.IDENTITY)) < 164 // 4, near
    assert iq.compute(record_of(t))[1] == model.IDENTITY
    assert model.image_ratio_db(buf) >= 42.8 - 5.0


def test_iq_symbols_are_exported_and_declared(iq):
    lib = capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtlfm_iq.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rtlfm_iq_[a-z_0-9]+)\s*\(", text)))
    assert declared == sorted(capi.DECLARED_IQ_SYMBOLS) and len(declared) == 8
    for name in declared + ["rtlfm_gpu_set_source_iq", "rtlfm_gpu_get_source_iq", "rtlfm_gpu_source_iq_sums", "rtlfm_gpu_source_iq_sums_all"]:
        assert hasattr(lib, name), name
    assert "iq.cpp" in hipbuild.SOURCES


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not on PATH")
def test_iq_check_under_the_sanitizers(tmp_path):
    """tools/iq_check.cpp with csrc/iq.cpp, AddressSanitizer + UBSan, as a program of its own on the CPU."""
    exe = str(tmp_path / "iq_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tools", "iq_check.cpp"),
                           os.path.join(hipbuild.CSRC, "iq.cpp")])
    r = subprocess.run([exe, "7", "200"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("iq_check: ok"), r.stdout
