"""The worst-case fixture of the Q14 discriminator (tests/golden/atan2_hard.npz) on the CPU: that it holds what it
claims, and that the reference's own chain - (int)(atan2(y, x) / 3.14159 * 16384) on the host libm, which the oracle
shares - gives the exact truncation on every row further than atan2_hard.THRESHOLD from a boundary.  Only then is
`want` a fair demand on the kernels (tests/test_atan2_hard_gpu.py)."""
import math
import os

import numpy as np
import pytest

import atan2_hard as ah
import reference_record as rr
from cases import make_cfg


@pytest.fixture(scope="module")
def fx():
    return ah.load()


def test_fixture_decades_and_size(fx):
    nb, npr = len(fx["b_d"]), len(fx["p_d"])
    assert fx["b_yx"].shape == (nb, 2) and fx["b_yx"].dtype == np.int32 and fx["b_want"].shape == fx["b_near"].shape == (nb,)
    assert fx["p_ab"].shape == (npr, 4) and fx["p_ab"].dtype == np.int16 and fx["p_want"].shape == fx["p_near"].shape == (npr,)
    b = ah.decade_counts(fx["b_d"], ah.BOUNDARY_DECADES)
    p = ah.decade_counts(fx["p_d"], ah.PRODUCT_DECADES)
    assert min(b.values()) >= 500, b
    assert min(p.values()) >= 20, p
    assert os.path.getsize(ah.FIXTURE) <= os.path.getsize(rr.RECORD)
    # what the tests lean on: y > 0, operands a boxcar of 255 bytes can produce, products within int32
    yx = fx["b_yx"].astype(np.int64)
    assert yx[:, 0].min() > 0 and 1000 <= np.abs(yx).max(axis=1).min() and np.abs(yx).max() <= (1 << 31) - 1
    assert np.abs(fx["p_ab"].astype(np.int64)).max() <= 127 * ah.BOXCAR
    cj, cr = ah.products(fx["p_ab"])
    assert cj.min() > 0 and max(np.abs(cj).max(), np.abs(cr).max()) <= (1 << 31) - 1
    assert fx["p_d"].max() < 1e-8 and int((fx["p_d"] < 1e-9).sum()) >= 1000
    for k in ("b", "p"):
        w, n = fx[k + "_want"], fx[k + "_near"]
        assert ((w == n) | (w == n - 1)).all() and (fx[k + "_d"] <= 0.5).all() and (fx[k + "_d"] > 0).all()


def _host_chain(y, x):
    return int(math.atan2(float(y), float(x)) / 3.14159 * 16384.0)  # C's (int) truncates toward zero, as int() does


def test_host_libm_chain_on_boundary_rows(fx):
    """math.atan2 is the host libm's: equal to `want` beyond the threshold, never past the nearest boundary; y and -y."""
    yx = fx["b_yx"].tolist()
    for sign in (1, -1):
        got = np.array([_host_chain(sign * y, x) for y, x in yx])
        worst = ah.check(got, fx["b_want"], fx["b_near"], fx["b_d"], f"host chain, y * {sign}", sign)
        print(f"host libm chain, boundary rows, y * {sign}: closest disagreement at d = {worst:.3g}")
        assert int((np.abs(got * sign - fx["b_want"]) > 1).sum()) == 0


def test_oracle_polar_discriminant_on_product_rows(oracle_lib, fx):
    """orc_polar_discriminant (the oracle's restatement, same libm) on the int16 operands; conjugating both mirrors it."""
    f = oracle_lib.oracle().orc_polar_discriminant
    ab = fx["p_ab"].astype(np.int64)
    for sign in (1, -1):
        got = np.array([f(ar, sign * aj, br, sign * bj) for ar, aj, br, bj in ab.tolist()])
        worst = ah.check(got, fx["p_want"], fx["p_near"], fx["p_d"], f"orc_polar_discriminant, conj {sign}", sign)
        print(f"orc_polar_discriminant, product rows, sign {sign}: closest disagreement at d = {worst:.3g}")
        assert int((np.abs(got * sign - fx["p_want"]) > 1).sum()) == 0


def test_product_streams_realise_the_rows(oracle_lib, fx):
    """The byte streams the GPU tests feed: through the oracle (boxcar 255, offset tuning, -A std) output 2m + 1 of a
    stream is the discriminator of its row m."""
    ns, L = 12, 16384
    iq, row, sign = ah.product_streams(fx["p_ab"], ns, L, seed=255)
    assert iq.shape[1] % L == 0 and int((row >= 0).sum()) == len(fx["p_ab"])
    cfg = make_cfg(dict(downsample=ah.BOXCAR, offset_tuning=1, custom_atan=0), L, iq.shape[1] // L)
    out, out_len, _ = oracle_lib.run_batch(cfg, iq, nthreads=4)
    direct = oracle_lib.oracle().orc_polar_discriminant
    ab = fx["p_ab"].astype(np.int64)
    for s in range(ns):
        m = int((row[s] >= 0).sum())
        assert out_len[s] >= 2 * m
        r = row[s, :m]
        got = out[s, 1:2 * m:2]
        ah.check(got, fx["p_want"][r], fx["p_near"][r], fx["p_d"][r], f"stream {s}", sign[s, :m])
        want = [direct(a[0], g * a[1], a[2], g * a[3]) for a, g in zip(ab[r].tolist(), sign[s, :m].tolist())]
        assert np.array_equal(got, np.array(want, np.int16))


def test_fixture_sample_recomputed(fx):
    """200 seeded rows again at 300 bits."""
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    old = mp.prec
    mp.prec = 300
    try:
        rng = np.random.default_rng(7)
        cj, cr = ah.products(fx["p_ab"])
        rows = [(int(fx["b_yx"][i, 0]), int(fx["b_yx"][i, 1]), fx["b_d"][i], fx["b_want"][i], fx["b_near"][i])
                for i in rng.choice(len(fx["b_d"]), 100, replace=False)]
        rows += [(int(cj[i]), int(cr[i]), fx["p_d"][i], fx["p_want"][i], fx["p_near"][i])
                 for i in rng.choice(len(fx["p_d"]), 100, replace=False)]
        for y, x, d, want, near in rows:
            v = mp.atan2(mp.mpf(y), mp.mpf(x)) * (16384 * 100000) / 314159
            n = mp.nint(v)
            assert int(mp.floor(v)) == want and int(n) == near
            assert float(abs(v - n)) == d
    finally:
        mp.prec = old
