#!/usr/bin/env python3
"""Write tests/golden/atan2_hard.npz: integer pairs whose Q14 angle lies as close to an integer as 32-bit operands allow.

polar_discriminant (src/rtl_fm.c:842-849) ends in (int)(atan2(cj, cr) / 3.14159 * 16384): trunc(theta * K) with
K = 16384 / 3.14159, the literal read as the exact rational 314159/100000.  Truncation turns an error of any size into a
whole LSB once theta * K sits that close to an integer k, so the pairs that can tell a good atan2 from a nearly good one
are the rational approximations of tan(k / K).  Random pairs never come closer than about 1e-7 LSB; these go down to 1e-15.

  boundary pairs  (y, x) int32: for every k = 1 .. 16383 the convergents of |tan(k / K)| and the semiconvergents with
                  coefficients a - 1 and ceil(a / 2) of every level, 1000 <= max(y, |x|) <= 2^31 - 1; x < 0 where the
                  tangent is negative.  y > 0 throughout: the tests mirror y.
  product pairs   (ar, aj, br, bj) int16, components within 127 * 255 = 32385 (what a boxcar of 255 full-scale bytes can
                  hold), chosen so that a * conj(b) - all a kernel's discriminator ever sees - points along k / K:
                  for a seeded b and every k, the best convergent of the direction k / K + arg b within the bound,
                  scaled up to it.  Screened in float64, confirmed here.  The first N_B_ALL values of b keep every
                  product with d < 1e-8; the rest (more draws for the decades where 600 give too few) only d < 1e-10.

Per row: the pair, d = |theta * K - nearest integer| (float64), want = trunc(theta * K) (int32) and that nearest integer
(int32: which side of it the angle lies on is what `want` alone does not say), all from 300-bit arithmetic.  The tests
read the file with numpy alone.

CPU only, needs mpmath; about a minute of CPU time, spread over up to 16 processes:

    python tests/golden/gen_atan2_hard.py
"""
import math
import os
import sys
from multiprocessing import Pool

import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "atan2_hard.npz")
SIZE_CAP_FILE = os.path.join(HERE, "reference", "results.npz")

PREC = 300
K_NUM, K_DEN = 16384 * 100000, 314159  # K = 16384 / 3.14159
INT32_MAX = (1 << 31) - 1
BOUND16 = 127 * 255
N_B_ALL, N_B = 600, 2400
BOUNDARY_DECADES = range(-14, -6)  # [1e-14, 1e-13) ... [1e-7, 1e-6)
PRODUCT_DECADES = range(-12, -8)   # [1e-12, 1e-11) ... [1e-9, 1e-8)
# boundary rows kept per decade of d, floor(log10 d) -> rows (the last convergents below 2^31 alone give some 37 000 rows
# under 1e-14); most where the tests' threshold of 1e-10 lies; KEEP_BELOW for each decade under 1e-16, none from 1e-3 up
KEEP = {-16: 800, -15: 1500, -14: 1500, -13: 1500, -12: 2000, -11: 2500, -10: 2500, -9: 1200, -8: 800, -7: 600,
        -6: 200, -5: 200, -4: 200}
KEEP_BELOW = 200


def exact(y: int, x: int):
    """(d, want, nearest integer) of one pair with y > 0 at PREC bits."""
    mp.prec = PREC
    v = mp.atan2(mpf(y), mpf(x)) * K_NUM / K_DEN
    n = mp.nint(v)
    return float(abs(v - n)), int(mp.floor(v)), int(n)


def boundary_pairs_of(k: int):
    """Convergents and a few semiconvergents of |tan(k / K)| as (y, x), x signed."""
    mp.prec = PREC
    t = mp.tan(mpf(k * K_DEN) / K_NUM)
    sign = -1 if t < 0 else 1
    man, exp = abs(t).man, abs(t).exp
    num, den = (int(man) << exp, 1) if exp >= 0 else (int(man), 1 << -exp)
    h2, h1, k2, k1 = 0, 1, 1, 0
    out = []
    while den and max(h1, k1) <= INT32_MAX:
        a, r = divmod(num, den)
        for c in sorted({a, a - 1, (a + 1) // 2}):
            if c < 1:
                continue
            y, x = h2 + c * h1, k2 + c * k1
            if 1000 <= max(y, x) <= INT32_MAX and y > 0 and x > 0:
                out.append((y, sign * x))
        h2, h1, k2, k1 = h1, h2 + a * h1, k1, k2 + a * k1
        num, den = den, r
    return sorted(set(out))


def boundary_rows(ks):
    rows = []
    for k in ks:
        for y, x in boundary_pairs_of(k):
            rows.append((y, x) + exact(y, x))
    return rows


def product_candidates(b, theta):
    """For one b and every boundary angle: a = the best convergent of the direction theta + arg b with components
    within BOUND16, scaled up to the bound; returns the rows whose float64 distance is below 2e-8."""
    br, bj = int(b[0]), int(b[1])
    phi = theta + math.atan2(bj, br)
    s, c = np.sin(phi), np.cos(phi)
    u, v = np.abs(s), np.abs(c)
    steep = u > v
    r = np.where(steep, v, u) / np.where(steep, u, v)
    # continued fraction of r in [0, 1], frozen at the last convergent whose denominator fits
    x = r.copy()
    h2 = np.zeros(r.shape, np.int64); h1 = np.ones(r.shape, np.int64)
    k2 = np.ones(r.shape, np.int64); k1 = np.zeros(r.shape, np.int64)
    live = np.ones(r.shape, bool)
    for _ in range(40):
        a = np.floor(x).astype(np.int64)
        h, k = a * h1 + h2, a * k1 + k2
        ok = live & (k <= BOUND16)
        h2 = np.where(ok, h1, h2); k2 = np.where(ok, k1, k2)
        h1 = np.where(ok, h, h1); k1 = np.where(ok, k, k1)
        frac = x - a
        live = ok & (frac > 1e-12)
        x = np.where(live, 1.0 / np.where(live, frac, 1.0), 0.0)
        if not live.any():
            break
    p, q = h1, np.maximum(k1, 1)
    m = BOUND16 // q
    p, q = p * m, q * m
    ar = np.where(steep, p, q) * np.where(c < 0, -1, 1)
    aj = np.where(steep, q, p) * np.where(s < 0, -1, 1)
    cr = ar * br + aj * bj
    cj = aj * br - ar * bj
    val = np.arctan2(cj.astype(np.float64), cr.astype(np.float64)) * (K_NUM / K_DEN)
    d = np.abs(val - np.rint(val))
    hit = np.flatnonzero((d < 2e-8) & (cj > 0))
    return [(int(ar[i]), int(aj[i]), br, bj) for i in hit]


def product_rows(args):
    first, bs = args
    theta = np.arange(1, 16384, dtype=np.float64) * (K_DEN / K_NUM)
    rows = []
    for n, b in enumerate(bs):
        limit = 1e-8 if first + n < N_B_ALL else 1e-10
        for ar, aj, br, bj in product_candidates(b, theta):
            e = exact(aj * br - ar * bj, ar * br + aj * bj)
            if e[0] < limit:
                rows.append((ar, aj, br, bj) + e)
    return rows


def decade(d):
    return np.floor(np.log10(np.maximum(d, 1e-300))).astype(np.int64)


def thin(rows):
    """Deterministic: within each decade of d the rows in (y, x) order, every n-th kept."""
    rows = sorted(set(rows))
    d = np.array([r[2] for r in rows])
    dec = decade(d)
    keep = np.zeros(len(rows), bool)
    for e in np.unique(dec):
        idx = np.flatnonzero(dec == e)
        cap = KEEP.get(int(e), KEEP_BELOW if e < -16 else 0)
        if len(idx) <= cap:
            keep[idx] = True
        elif cap:
            keep[idx[np.unique(np.linspace(0, len(idx) - 1, cap).astype(np.int64))]] = True
    return [r for r, k in zip(rows, keep) if k]


def main():
    workers = min(16, os.cpu_count() or 1)
    rng = np.random.default_rng(20240607)
    bs = rng.integers(8000, BOUND16 + 1, size=(N_B, 2)) * rng.choice([-1, 1], size=(N_B, 2))
    with Pool(workers) as pool:
        ks = list(range(1, 16384))
        chunks = [ks[i::workers * 8] for i in range(workers * 8)]
        brow = [r for part in pool.map(boundary_rows, chunks) for r in part]
        print(f"boundary candidates: {len(brow)}", file=sys.stderr)
        step = 10
        prow = [r for part in pool.map(product_rows, [(i, bs[i:i + step]) for i in range(0, N_B, step)]) for r in part]
        print(f"product rows: {len(prow)}", file=sys.stderr)
    brow = thin(brow)
    prow = sorted(set(prow))
    b = dict(b_yx=np.array([r[:2] for r in brow], np.int32), b_d=np.array([r[2] for r in brow], np.float64),
             b_want=np.array([r[3] for r in brow], np.int32), b_near=np.array([r[4] for r in brow], np.int32))
    p = dict(p_ab=np.array([r[:4] for r in prow], np.int16), p_d=np.array([r[4] for r in prow], np.float64),
             p_want=np.array([r[5] for r in prow], np.int32), p_near=np.array([r[6] for r in prow], np.int32))
    bdec, pdec = decade(b["b_d"]), decade(p["p_d"])
    for e in BOUNDARY_DECADES:
        n = int((bdec == e).sum())
        print(f"boundary rows in [1e{e}, 1e{e + 1}): {n}")
        assert n >= 500, (e, n)
    for e in PRODUCT_DECADES:
        n = int((pdec == e).sum())
        print(f"product rows in [1e{e}, 1e{e + 1}): {n}")
        assert n >= 20, (e, n)
    assert np.abs(p["p_ab"].astype(np.int64)).max() <= BOUND16
    np.savez_compressed(OUT, **b, **p)
    size, cap = os.path.getsize(OUT), os.path.getsize(SIZE_CAP_FILE)
    print(f"{OUT}: {len(brow)} boundary rows (closest {b['b_d'].min():.3g}), {len(prow)} product rows "
          f"(closest {p['p_d'].min():.3g}), {size} bytes (cap {cap})")
    assert size <= cap, (size, cap)


if __name__ == "__main__":
    main()
