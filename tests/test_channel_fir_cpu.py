"""The channel filter's host side without a GPU (include/rtlfm_hip.h, rtlfm_gpu_set_channel_filter): the symbols, the
check's edges, rtlfm_channel_lowpass by its properties, the numpy model (tests/channel_fir_model.py) against the boxcar
model it must contain, and what the filter is for - the neighbour 1.5 channel spacings away - on the model."""
import errno

import numpy as np
import pytest

import channel_fir_model as fm
import channel_model as cm
from rtlsdr_amd import build as hipbuild
from rtlsdr_amd import capi


@pytest.fixture(scope="module")
def lib():
    hipbuild.build()
    return capi.load()


FILTER_SYMBOLS = ("rtlfm_channel_filter_check", "rtlfm_channel_lowpass", "rtlfm_gpu_set_channel_filter",
                  "rtlfm_gpu_get_channel_filter")


def test_filter_symbols_are_exported_and_declared(lib):
    for name in FILTER_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.DECLARED_SYMBOLS, name
    assert capi.CHANNEL_MAX_TAPS == fm.MAX_TAPS == 1024


def check(lib, taps, shift, ntaps=None):
    t = np.ascontiguousarray(taps, dtype=np.int16)
    return lib.rtlfm_channel_filter_check(t.ctypes.data, t.size if ntaps is None else ntaps, shift)


def test_filter_check_edges(lib):
    one = [1]
    assert check(lib, one, 0) == 0 and check(lib, one, 30) == 0
    assert check(lib, one, -1) == -errno.EINVAL and check(lib, one, 31) == -errno.EINVAL
    assert check(lib, one, 0, ntaps=0) == -errno.EINVAL and check(lib, one, 0, ntaps=-3) == -errno.EINVAL
    assert lib.rtlfm_channel_filter_check(None, 1, 0) == -errno.EINVAL
    assert check(lib, [1] * 1024, 0) == 0
    assert check(lib, [1] * 1025, 0) == -errno.EINVAL
    # 182 sum|taps| + r <= 2^31 - 1
    assert check(lib, [32767] * 1024, 0) == -errno.ERANGE
    assert check(lib, [32767] * 64, 0) == 0
    assert check(lib, [-32768] * 64, 0) == 0
    most = ((1 << 31) - 1) // 182  # the largest sum of magnitudes at shift 0
    taps = [32767] * (most // 32767) + [most % 32767]
    assert sum(taps) == most and check(lib, taps, 0) == 0
    assert check(lib, taps[:-1] + [-(taps[-1] + 1)], 0) == -errno.ERANGE  # one more, and negative: magnitudes count
    # ... and the rounding constant belongs to the sum: 182 most + 2^(shift - 1) passes 2^31 - 1 from shift 8 on
    room = (1 << 31) - 1 - 182 * most
    assert 0 <= room < 182
    assert check(lib, taps, 7) == (0 if 64 <= room else -errno.ERANGE)
    assert check(lib, taps, 9) == -errno.ERANGE


def lowpass(lib, ntaps, cutoff, D):
    import ctypes as C
    t = np.zeros(max(ntaps, 1), dtype=np.int16)
    sh = C.c_int(-1)
    r = lib.rtlfm_channel_lowpass(ntaps, cutoff, D, t.ctypes.data, C.byref(sh))
    return r, t, sh.value


def test_channel_lowpass_by_its_properties(lib):
    for ntaps, cutoff, D in ((80, 0.04, 10), (81, 0.04, 10), (40, 0.05, 10), (16, 0.1, 4), (512, 0.4 / 64, 64), (1, 0.25, 1), (1024, 0.01, 25)):
        r, t, sh = lowpass(lib, ntaps, cutoff, D)
        assert r == 0 and sh == 14, (ntaps, cutoff, D, r)
        assert np.array_equal(t, t[::-1]), (ntaps, cutoff, D)
        assert abs(int(t.astype(np.int64).sum()) - D * (1 << 14)) <= ntaps, (ntaps, cutoff, D, int(t.sum()))
        assert check(lib, t, sh) == 0
    # the stopband: ntaps = 8 D, cutoff = 0.4 / D, D = 10 - beyond 0.6 / D at least 40 dB below DC
    r, t, _ = lowpass(lib, 80, 0.04, 10)
    H = np.abs(np.fft.rfft(t.astype(np.float64), 1 << 16))
    f = np.arange(H.size) / float(1 << 16)
    att = 20 * np.log10(H[0] / H[f >= 0.06].max())
    assert att >= 40.0, att
    # the package's wrapper hands out the same taps
    import rtlsdr_amd
    t2, sh2 = rtlsdr_amd.channel_lowpass(80, 0.04, 10)
    assert sh2 == 14 and np.array_equal(t2, t)
    # refusals
    for bad in ((0, 0.1, 4), (1025, 0.1, 4), (8, 0.0, 4), (8, 0.5, 4), (8, -0.1, 4), (8, float("nan"), 4), (8, 0.1, 0)):
        assert lowpass(lib, *bad)[0] == -errno.EINVAL, bad
    assert lowpass(lib, 1, 0.25, 2)[0] == -errno.ERANGE    # one tap of 2 * 2^14 does not fit an int16
    assert lowpass(lib, 4, 0.45, 64)[0] == -errno.ERANGE


def test_model_with_ones_is_the_boxcar_model():
    """Taps of D ones with shift 0 are low_pass(): the model of the filter contains model_raw_boxcar, over runs that
    leave a partial sum behind (256 k % D != 0), at general steps, on full-scale bytes."""
    rng = np.random.default_rng(7)
    nsrc, per = 2, 3
    steps = [int(v) for v in rng.integers(0, 1 << 32, size=nsrc * per, dtype=np.uint64)]
    for D in (7, 10):
        src = rng.integers(0, 256, size=(nsrc, 2 * 256 * 6), dtype=np.uint8)
        model = fm.FirModel(steps, per, D, [1] * D, 0, nsrc)
        state, n0 = None, 0
        for n in (256, 768, 512):
            part = src[:, 2 * n0:2 * (n0 + n)]
            want, state = cm.model_raw_boxcar(part, steps, D, state, per_source=per, pos=n0)
            got = fm.raw_rows(*model.run(part))
            for s in range(nsrc * per):
                assert np.array_equal(got[s], want[s]), (D, n0, s)
                assert model.p0[s] == state[s]["prev_index"]
            n0 += n


def tone_bytes(freq, n, amplitude=50.0):
    ph = 2 * np.pi * freq * np.arange(n)
    src = np.empty((1, 2 * n), dtype=np.uint8)
    src[0, 0::2] = np.rint(127 + amplitude * np.cos(ph)).astype(np.uint8)
    src[0, 1::2] = np.rint(127 + amplitude * np.sin(ph)).astype(np.uint8)
    return src


def mean_power(I, Q, skip):
    i, q = I[0][skip:].astype(np.float64), Q[0][skip:].astype(np.float64)
    return float((i * i + q * q).mean())


def test_the_adjacent_channel_is_gone_and_the_wanted_one_stays(lib):
    """A tone of amplitude 50 at 1.5 / D (step 0, D = 10): the boxcar passes it 13 dB down, 80 taps of
    rtlfm_channel_lowpass(80, 0.04, 10) at most a thousandth of that; a tone at 0.1 / D keeps its power within 10 % of
    (50 D)^2.  Powers are means over the outputs behind the first eight, whose windows still reach into the silence
    the history starts from."""
    D, n = 10, 1 << 14
    r, taps, shift = lowpass(lib, 80, 0.04, D)
    assert r == 0
    skip = 80 // D
    src = tone_bytes(1.5 / D, n)
    box = mean_power(*fm.FirModel([0], 1, D, [1] * D, 0, 1).run(src), skip)
    fir = mean_power(*fm.FirModel([0], 1, D, taps, shift, 1).run(src), skip)
    assert 10000 < box < 14000, box  # (12 104 on the continuous tone)
    assert fir <= box / 1000, (fir, box)
    wanted = mean_power(*fm.FirModel([0], 1, D, taps, shift, 1).run(tone_bytes(0.1 / D, n)), skip)
    assert abs(wanted / (50.0 * D) ** 2 - 1.0) <= 0.10, wanted
