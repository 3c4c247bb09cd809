"""The channel bank's host side without a GPU (include/rtlfm_hip.h, rtlfm_gpu_set_channel_bank): the symbols, the check's
edges, the numpy model (tests/channel_bank_model.py) against hand-computed sums, and the model against the mixer + channel
filter model it stands in for."""
import errno

import numpy as np
import pytest

import channel_bank_model as bm
import channel_fir_model as fm
from rtlsdr_amd import build as hipbuild
from rtlsdr_amd import capi


@pytest.fixture(scope="module")
def lib():
    hipbuild.build()
    return capi.load()


BANK_SYMBOLS = ("rtlfm_channel_bank_check", "rtlfm_gpu_set_channel_bank", "rtlfm_gpu_get_channel_bank")


def test_bank_symbols_are_exported_and_declared(lib):
    for name in BANK_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.DECLARED_SYMBOLS, name
    assert capi.BANK_MAX_TAPS == bm.MAX_TAPS == 4096


def check(lib, K, taps, shift, ntaps=None):
    t = np.ascontiguousarray(taps, dtype=np.int16)
    return lib.rtlfm_channel_bank_check(K, t.ctypes.data, t.size if ntaps is None else ntaps, shift)


def filter_check(lib, taps, shift):
    t = np.ascontiguousarray(taps, dtype=np.int16)
    return lib.rtlfm_channel_filter_check(t.ctypes.data, t.size, shift)


def test_bank_check_edges(lib):
    one = [1]
    for K in (4, 8, 16, 32, 64, 128, 256):
        assert check(lib, K, one, 0) == 0 and check(lib, K, one, 30) == 0, K
    for K in (-4, 0, 1, 2, 3, 6, 48, 255, 257, 512, 1 << 20):
        assert check(lib, K, one, 0) == -errno.EINVAL, K
    assert check(lib, 4, one, -1) == -errno.EINVAL and check(lib, 4, one, 31) == -errno.EINVAL
    assert check(lib, 4, one, 0, ntaps=0) == -errno.EINVAL and check(lib, 4, one, 0, ntaps=-3) == -errno.EINVAL
    assert lib.rtlfm_channel_bank_check(4, None, 1, 0) == -errno.EINVAL
    assert check(lib, 4, [1] * 4096, 0) == 0
    assert check(lib, 4, [1] * 4097, 0) == -errno.EINVAL
    # 128 max_b sum_q |taps[b + q K]| + rnd <= 2^31 - 1: the largest BRANCH counts, not the filter
    most = ((1 << 31) - 1) // 128  # = 2^24 - 1, the largest branch sum at shift 0
    assert most == (1 << 24) - 1
    q = most // 32767 + 1  # taps of 32767 in one branch that pass it
    assert check(lib, 4, [32767] * 4096, 0) == -errno.ERANGE    # 1024 per branch
    assert check(lib, 256, [32767] * 4096, 0) == 0              # 16 per branch
    assert check(lib, 256, [-32768] * 4096, 0) == 0
    K = 4
    taps = np.zeros(K * q, dtype=np.int64)
    taps[1::K] = 32767                                           # branch 1 alone
    taps[1 + K * (q - 1)] = most - 32767 * (q - 1)
    assert taps[1::K].sum() == most and check(lib, K, taps, 0) == 0
    neg = taps.copy()
    neg[1 + K * (q - 1)] = -(neg[1 + K * (q - 1)] + 1)            # one more, and negative: magnitudes count
    assert check(lib, K, neg, 0) == -errno.ERANGE
    other = taps.copy()
    other[2::K] = 32767                                          # another branch as full: still the largest one that counts
    other[2 + K * (q - 1)] = taps[1 + K * (q - 1)]
    assert check(lib, K, other, 0) == 0
    # ... and the rounding constant belongs to the sum: 128 most = 2^31 - 128, which leaves room for rnd <= 127
    assert check(lib, K, taps, 7) == 0 and check(lib, K, taps, 8) == -errno.ERANGE
    # the package's wrapper
    import rtlsdr_amd
    assert rtlsdr_amd.channel_bank_check(K, taps, 7) == 0 and rtlsdr_amd.channel_bank_check(K, taps, 8) == -errno.ERANGE
    assert rtlsdr_amd.channel_bank_check(5, taps, 0) == -errno.EINVAL


def test_bank_check_and_filter_check_differ(lib):
    """The two checks bound different sums.  128 max_b(...) <= 182 sum(...): on taps alone whatever the channel filter's check
    lets through, the bank's lets through for every K - so a set that passes there fails here only through what the bank
    adds, K; the reverse holds for taps the filter has no room for, in length or in magnitude."""
    ok_filter = [32767] * 64
    assert filter_check(lib, ok_filter, 0) == 0
    assert check(lib, 6, ok_filter, 0) == -errno.EINVAL and check(lib, 512, ok_filter, 0) == -errno.EINVAL
    for K in (4, 64, 256):
        assert check(lib, K, ok_filter, 0) == 0
    rng = np.random.default_rng(3)
    for _ in range(50):  # the implication, on random sets around the filter's limit
        n = int(rng.integers(1, 1025))
        t = rng.integers(-32768, 32768, size=n)
        sh = int(rng.integers(0, 31))
        if filter_check(lib, t, sh) == 0:
            assert check(lib, 4, t, sh) == 0
    long_set = [100] * 4096                     # too long for the filter
    assert filter_check(lib, long_set, 0) == -errno.EINVAL and check(lib, 64, long_set, 0) == 0
    big = [32767] * 1024                        # 182 * 1024 * 32767 > 2^31 - 1, but 16 per branch of 64
    assert filter_check(lib, big, 0) == -errno.ERANGE and check(lib, 64, big, 0) == 0
    assert check(lib, 4, big, 0) == 0 and check(lib, 4, big * 3, 0) == -errno.ERANGE   # 256 and 768 per branch of 4


def test_model_bins_are_fix_fft_of_hand_computed_sums():
    """K = 4, 11 taps, D = 3, pos = 5: every frame's sums by the definition, term by term in Python integers, then the
    oracle's fix_fft of them - the model's bins, in order, permuted and duplicated."""
    from oracle import pyoracle as po
    lib = po._power_lib()
    K, m, D, shift, pos, T = 4, 2, 3, 3, 5, 64
    rng = np.random.default_rng(1)
    taps = [int(v) for v in rng.integers(-300, 300, size=11)]
    src = rng.integers(0, 256, size=(1, 2 * T), dtype=np.uint8)
    src[0, :8] = (0, 255, 255, 0, 0, 0, 255, 255)
    bins = [2, 0, 3, 3, 1]
    model = bm.BankModel(K, taps, shift, D, 1, bins=bins)
    model.seek(pos)
    I, Q = model.run(src)
    x = [(int(src[0, 2 * n]) - 127, int(src[0, 2 * n + 1]) - 127) for n in range(T)]
    sine = lib.orcp_sine_table(m)
    E = T // D
    assert all(a.size == E for a in I) and model.p0 == [T - E * D] * len(bins)
    for k in range(E):
        e = (k + 1) * D - 1
        u = [[0, 0] for _ in range(K)]
        for j, tap in enumerate(taps):
            if e - j >= 0:  # (x = 0 before the clear)
                r = (pos + e - j) % K
                u[r][0] += tap * x[e - j][0]
                u[r][1] += tap * x[e - j][1]
        v = np.array([[max(-32768, min(32767, (c + 4) >> 3)) for c in ur] for ur in u], dtype=np.int16).reshape(-1)
        assert lib.orcp_fix_fft(v.ctypes.data, m, sine, m) == 0
        for c, b in enumerate(bins):
            assert (int(I[c][k]), int(Q[c][k])) == (int(v[2 * b]), int(v[2 * b + 1])), (k, c, b)


def two_carriers(K, k1, k2, amp, n, seed):
    """Two carriers a little off the centres of bins k1 and k2 (k2 a negative shift) plus noise, as source bytes."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    sig = amp * np.exp(2j * np.pi * (k1 / K + 0.11 / K) * t) + 0.7 * amp * np.exp(2j * np.pi * (k2 / K - 0.07 / K) * t + 1.0j)
    sig += rng.normal(0, 2.0, n) + 1j * rng.normal(0, 2.0, n)
    src = np.empty((1, 2 * n), dtype=np.uint8)
    src[0, 0::2] = np.clip(np.rint(127 + sig.real), 0, 255).astype(np.uint8)
    src[0, 1::2] = np.clip(np.rint(127 + sig.imag), 0, 255).astype(np.uint8)
    return src


# The worst |bank - (mixer + filter)| over all bins, frames and both components on this test's own inputs, measured once
# on the two CPU models (LAB.md I.40); the test asserts twice that.  The margin covers the mixer's table rounding and one
# FIX_MPY per stage, which vary with the input.
MEASURED_WORST = {16: 4, 64: 5}


@pytest.mark.parametrize("K,D,ntaps,amp", [(16, 10, 128, 40.0), (64, 32, 512, 50.0)])
def test_bank_agrees_with_mixer_and_filter_model(lib, K, D, ntaps, amp):
    """BankModel with shift = 14 - m against FirModel with steps[k] = k 2^32 / K and shift 14, the same Hamming sinc at the
    boxcar's gain D (8 taps per branch): amplitudes of 400 and 1600 at the output."""
    import ctypes as C
    m = K.bit_length() - 1
    taps = np.zeros(ntaps, dtype=np.int16)
    sh = C.c_int()
    assert lib.rtlfm_channel_lowpass(ntaps, 0.4 / K, D, taps.ctypes.data, C.byref(sh)) == 0 and sh.value == 14
    assert check(lib, K, taps, 14 - m) == 0
    n = 4096
    src = two_carriers(K, 5, K - 3, amp, n, 20261019 + K)
    bank = bm.BankModel(K, taps, 14 - m, D, 1)
    fir = fm.FirModel([(k << 32) // K for k in range(K)], K, D, taps, 14, 1)
    worst, peak = 0, 0
    for part in (src[:, :2 * 1536], src[:, 2 * 1536:]):  # two runs: the histories of both models are carried
        bi, bq = bank.run(part)
        fi, fq = fir.run(part)
        for k in range(K):
            assert bi[k].shape == fi[k].shape
            worst = max(worst, int(np.abs(bi[k] - fi[k]).max()), int(np.abs(bq[k] - fq[k]).max()))
            peak = max(peak, int(np.abs(fi[k]).max()))
    print(f"K={K} D={D} ntaps={ntaps}: worst difference {worst} LSB, peak {peak}")
    assert 0.8 * amp * D <= peak <= 1.3 * amp * D, peak  # the carrier came through at the boxcar's gain
    assert worst <= 2 * MEASURED_WORST[K], (worst, MEASURED_WORST[K])
