"""tests/golden/atan2_hard.npz (tests/golden/gen_atan2_hard.py) for the tests that read it: operands of the Q14
discriminator whose angle theta * K lies within d of an integer, with the exact truncation `want` and that integer, `near`.

THRESHOLD is the distance from which every float64 evaluation has to give `want`.  It comes from the bound that
rtlsdr_amd/csrc/dsp_device.h states for atan2_q14, not from a measurement: 2e-11 (truncated series) + 2e-13 (one Newton
step) + a few roundings of 1.8e-12 at magnitudes up to 16384 is about 2.5e-11, times four for what v_rcp_f64 may add."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "atan2_hard.npz")
THRESHOLD = 1e-10
BOUNDARY_DECADES = range(-14, -6)  # [1e-14, 1e-13) ... [1e-7, 1e-6): >= 500 boundary rows each
PRODUCT_DECADES = range(-12, -8)   # [1e-12, 1e-11) ... [1e-9, 1e-8): >= 20 product rows each
BOXCAR = 255                       # the product rows' components stay within 127 * BOXCAR


def load():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def decade_counts(d, decades):
    e = np.floor(np.log10(d)).astype(np.int64)
    return {int(k): int((e == k).sum()) for k in decades}


def products(p_ab):
    """(cj, cr) of a * conj(b) for rows (ar, aj, br, bj): multiply(ar, aj, br, -bj), src/rtl_fm.c:836-846."""
    ar, aj, br, bj = (p_ab[:, i].astype(np.int64) for i in range(4))
    return aj * br - ar * bj, ar * br + aj * bj


def other_side(want, near):
    """The integer on the other side of the row's nearest boundary (rows with y > 0, so the angle is positive): with
    the angle just above `near` the truncation is `near` and the other side near - 1, just below it they swap."""
    return np.where(want == near, np.maximum(near - 1, 0), near)


def check(got, want, near, d, what, sign=1):
    """`got` against the exact truncation of the fixture's rows (y > 0; sign = -1, a number or one per row, where
    y was negated: truncation toward zero is odd): equal from THRESHOLD on; below it `want` or the integer across the
    nearest boundary, nothing further.  Returns the largest d at which got != want (0.0 where all agree)."""
    got = got.astype(np.int64) * sign; want = want.astype(np.int64)
    other = other_side(want, near.astype(np.int64))
    wrong = got != want
    worst = float(d[wrong].max()) if wrong.any() else 0.0
    far = np.flatnonzero(wrong & (got != other))
    assert far.size == 0, f"{what}: {far.size} rows beyond the nearest boundary, first {far[:5]}: got {got[far[:5]]}, want {want[far[:5]]}"
    bad = np.flatnonzero(wrong & (d > THRESHOLD))
    assert bad.size == 0, (f"{what}: {bad.size} rows with d > {THRESHOLD} off by one, largest d {worst:.3g}; first {bad[:5]}: "
                           f"got {got[bad[:5]]}, want {want[bad[:5]]}, d {d[bad[:5]]}")
    return worst


def product_streams(p_ab, ns, L, seed):
    """Byte streams whose boxcar of BOXCAR samples (offset tuning: no fs/4 rotation) decimates to z[2m] = b_m,
    z[2m + 1] = a_m, so that fm_demod's output 2m + 1 is the discriminator of row m's product.  Row r goes to stream
    r % ns at m = r // ns; odd m are conjugated (a, b -> conj a, conj b: the product's angle changes sign).  A component
    T = 255 q + r is spread over the window as r samples of q + 1 and 255 - r of q in shuffled order, byte = sample + 127;
    the tail is random bytes up to whole buffers of L.
    Returns (iq uint8 [ns, nb * L], row int [ns, M] with -1 where a stream has no row m, sign int [ns, M])."""
    rng = np.random.default_rng(seed)
    n = len(p_ab)
    M = -(-n // ns)
    row = np.full((ns, M), -1, np.int64)
    row.T.flat[:n] = np.arange(n)  # row r -> [r % ns, r // ns]
    sign = np.where(np.arange(M) % 2 == 1, -1, 1)[None, :].repeat(ns, 0)
    nb = -(-(M * 2 * BOXCAR * 2) // L)
    iq = rng.integers(0, 256, size=(ns, nb * L), dtype=np.uint8)
    for s in range(ns):
        m = int((row[s] >= 0).sum())
        ab = p_ab[row[s, :m]].astype(np.int64)
        ab[:, 1] *= sign[s, :m]; ab[:, 3] *= sign[s, :m]
        z = np.empty((2 * m, 2), np.int64)  # decimated samples (I, Q)
        z[0::2] = ab[:, 2:4]
        z[1::2] = ab[:, 0:2]
        q, r = np.divmod(z, BOXCAR)
        order = rng.random((2 * m, 2, BOXCAR)).argsort(axis=-1)
        samples = q[..., None] + (order < r[..., None])
        assert samples.min() >= -127 and samples.max() <= 128 and np.array_equal(samples.sum(-1), z)
        iq[s, :2 * m * BOXCAR * 2] = (samples.transpose(0, 2, 1) + 127).astype(np.uint8).ravel()
    return iq, row, sign
