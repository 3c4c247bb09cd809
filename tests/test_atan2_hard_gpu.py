"""The `-A std` discriminator where it can go wrong: atan2_q14 (rtlsdr_amd/csrc/dsp_device.h) on the operands of
tests/golden/atan2_hard.npz, whose angles lie between 1e-3 and 1e-15 LSB from a Q14 boundary, against the exact
truncation - as a function (rtlfm_gpu_selftest_atan2: the constant-memory node table, and the device libm chain next
to it) and inside the production kernels that read the node table from LDS: k_boxcar_scan (one launch) and the staged
k_fm_demod, on byte streams whose boxcar sums are the fixture's product rows.

k_fused is not driven to designed operands: its decimated samples come through truncating fifth_order passes with
carried history, and nobody steers those to a chosen 31-bit product.  It shares the inline function and the LDS node
table with k_boxcar_scan.

The bound (atan2_hard.THRESHOLD) is the code's stated one with a margin, not a measurement; what the device measures is
printed (pytest -s) and recorded in LAB.md."""
import numpy as np
import pytest

import atan2_hard as ah
import golden_util as gu
from cases import case, make_cfg
from rtlsdr_amd import capi
from test_parity_gpu import gpu_run

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def fx():
    return ah.load()


def test_atan2_q14_and_device_libm_on_worst_case_rows(fx):
    """Every boundary row and the (cj, cr) of every product row, with y and -y: from d > 1e-10 on both device chains
    give the exact truncation; closer they give it or the integer across that boundary.  No row is exempt."""
    lib = capi.load()
    cj, cr = ah.products(fx["p_ab"])
    yx = np.concatenate([fx["b_yx"].astype(np.int64), np.stack([cj, cr], axis=1)])
    want = np.concatenate([fx["b_want"], fx["p_want"]])
    near = np.concatenate([fx["b_near"], fx["p_near"]])
    d = np.concatenate([fx["b_d"], fx["p_d"]])
    n = len(yx)
    both = np.ascontiguousarray(np.concatenate([yx, yx * np.array([-1, 1])]).astype(np.int32))
    q14 = np.full(2 * n, 1 << 20, np.int32); q14_libm = np.full(2 * n, 1 << 20, np.int32)
    assert lib.rtlfm_gpu_selftest_atan2(0, both.ctypes.data, 2 * n, q14.ctypes.data, q14_libm.ctypes.data) == 0
    worst = {}
    for name, got in (("atan2_q14", q14), ("device libm chain", q14_libm)):
        for sign, part in ((1, got[:n]), (-1, got[n:])):
            wrong = part.astype(np.int64) * sign != want
            worst[name, sign] = float(d[wrong].max()) if wrong.any() else 0.0
            print(f"{name}, y * {sign}: {int(wrong.sum())} of {n} rows differ from the exact truncation, "
                  f"closest disagreement at d = {worst[name, sign]:.3g}")
    for name, got in (("atan2_q14", q14), ("device libm chain", q14_libm)):
        for sign, part in ((1, got[:n]), (-1, got[n:])):
            assert ah.check(part, want, near, d, f"{name}, y * {sign}", sign) == worst[name, sign]


@pytest.fixture(scope="module")
def streams(oracle_lib, fx):
    """The product rows as 12 byte streams of buffers of 16384, and the oracle's run of them (shared, not changed)."""
    ns, L = 12, 16384
    iq, row, sign = ah.product_streams(fx["p_ab"], ns, L, seed=255)
    cfg = make_cfg(dict(downsample=ah.BOXCAR, offset_tuning=1, custom_atan=0, mode=capi.MODE_FM), L, iq.shape[1] // L)
    want, want_len, wst = oracle_lib.run_batch(cfg, iq, nthreads=4)
    return cfg, iq, row, sign, want, want_len, wst


@pytest.mark.parametrize("path", [2, 1], ids=["k_boxcar_scan", "staged_k_fm_demod"])
def test_production_kernels_on_designed_products(fx, streams, path):
    """Output 2m + 1 of a stream is the discriminator of product row m: with d > 1e-10 bit-equal to the oracle and to the
    exact truncation, closer within the nearest boundary; every other output within 1 LSB of the oracle; the carried
    state the oracle's."""
    cfg, iq, row, sign, want, want_len, wst = streams
    ns = iq.shape[0]
    outs, sts, used = gpu_run(cfg, iq, path=path)
    assert used == path
    hard, worst = 0, 0.0
    for s in range(ns):
        o = want[s, :want_len[s]]
        assert outs[s].shape == o.shape, (s, outs[s].shape, o.shape)
        m = int((row[s] >= 0).sum())
        r = row[s, :m]
        got = outs[s][1:2 * m:2]
        d = fx["p_d"][r]
        clear = d > ah.THRESHOLD
        assert np.array_equal(got[clear], o[1:2 * m:2][clear]), f"stream {s}: designed outputs differ from the oracle"
        worst = max(worst, ah.check(got, fx["p_want"][r], fx["p_near"][r], d, f"stream {s}, path {path}", sign[s, :m]))
        diff = np.abs(outs[s].astype(np.int32) - o.astype(np.int32))
        assert diff.max() <= 1, f"stream {s}: output {int(diff.argmax())} is {int(diff.max())} from the oracle"
        assert gu.state_dict(sts[s], False) == gu.state_dict(wst[s], False), s
        hard += int((d < 1e-9).sum())
    print(f"path {path}: {hard} designed outputs with d < 1e-9, closest disagreement with the exact truncation at d = {worst:.3g}")
    assert hard >= 1000


def _carriers(ns, nsamples):
    """Unmodulated carriers around fs / 4 (where rtl_fm tunes the wanted signal), one constant phase step per stream:
    behind the discriminator the audio is flat but for some 10 LSB of jitter from the quantised bytes and the passes'
    truncation, and deemph_filter's avg += (d +- a / 2) / a does not move for |d| < a / 2 - with a = 50 runs of equal
    samples."""
    n = np.arange(nsamples, dtype=np.float64)
    iq = np.empty((ns, 2 * nsamples), np.uint8)
    for s in range(ns):
        ph = 2 * np.pi * n * (0.25 + (s - ns // 2) / (64 * 19.0)) + 0.3 * s
        iq[s, 0::2] = (127 + np.rint(100.0 * np.cos(ph))).astype(np.uint8)
        iq[s, 1::2] = (127 + np.rint(100.0 * np.sin(ph))).astype(np.uint8)
    return iq


@pytest.mark.parametrize("kind", ["carrier", "squelched"])
def test_arbitrary_upsample_of_equal_neighbours(oracle_lib, kind):
    """arbitrary_upsample (src/rtl_fm.c) interpolates a * (1 - frac) + b * frac in double and truncates; with a == b the
    sum is a only as long as product and sum round separately - the one expression of the tail whose result changes if
    the build ever contracts it into an fma.  Flat audio (constant-phase-step carriers, a de-emphasis constant long
    enough to hold it still) and silence (squelch closed) through config 3's stages with the 16000 -> 22050 resampler,
    bit-exact against the oracle."""
    ov, _ = case("c3_p6_fir9_deemph_up22050")
    ov = dict(ov, squelch_level=30000) if kind == "squelched" else dict(ov, deemph_a=50)
    L, nb, ns = 16384, 4, 8
    cfg = make_cfg(ov, L, nb)
    iq = _carriers(ns, L // 2 * nb)
    before, before_len, _ = oracle_lib.run_batch(make_cfg(dict(ov, rate_out2=-1), L, nb), iq, nthreads=2)
    flat = sum(int(((a[1:] == a[:-1]) & ((a[1:] != 0) | (kind == "squelched"))).sum())
               for a in (before[s, :before_len[s]] for s in range(ns)))
    assert flat >= 1000, f"the resampler's input has only {flat} pairs of equal neighbours"
    if kind == "squelched":
        assert not before[:, :before_len[0]][:, -L // 128:].any()
    want, want_len, wst = oracle_lib.run_batch(cfg, iq, nthreads=2)
    for splits in (None, [(0, 1), (1, nb)]):
        outs, sts, _ = gpu_run(cfg, iq, splits=splits)
        for s in range(ns):
            assert np.array_equal(outs[s], want[s, :want_len[s]]), (kind, splits, s)
            assert gu.state_dict(sts[s], False) == gu.state_dict(wst[s], False)
