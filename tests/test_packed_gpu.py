"""Packed results on the GPU (include/rtlfm_hip.h, rtlfm_gpu_fetch_packed; csrc/pack_kernel.h).

The operator (rtlfm_gpu_pack_device) against tests/packed_model.py in every byte; mode 1 through the ring against the
same run's rtlfm_gpu_fetch_all; mode 2 - under channels over the source-indexed ring, where squelch_gate is refused, and
without channels - against (a) a twin handle that is fed the same bytes with the option off, its rows and levels gated in
numpy by packed_model's rule with a carried counter, (b) on the boxcar FM front the oracle buffer by buffer with the demod
thread's rule on its state as tests/scan_model.py applies it, and without channels a twin's squelch_gate output.
Everything is equality of bits: -A std is not used on the oracle's side."""
import ctypes as C
import errno

import numpy as np
import pytest

import channel_model as cm
import packed_model as pm
import scan_model as sm
from cases import case, make_cfg
from channel_common import (bounded, demod, full_scale, make_steps_special, random_bank_taps, random_fir_taps, raw_cfg)
from rtlsdr_amd import capi
from rtlsdr_amd.capi import ATAN_FAST, MODE_FM, MODE_RAW, RESAMPLE_LOW_PASS_REAL, RtlfmCfg
from rtlsdr_amd.demod import pack_device

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0x5A5A
GUARD = 64


# ------------------------------------------------------------------ 1. the operator ----

def run_operator(rows, lens, stride, base, cap, twice=False):
    """rows: int16 [S, stride] on the host, placed on the device `base` int16 behind an aligned address.  Returns
    (packed [cap + GUARD] as the launch left it, index, total)."""
    S = len(lens)
    d_rows = torch.full((S * stride + base + 8,), 0x1111, dtype=torch.int16, device="cuda")
    d_rows[base:base + S * stride] = torch.from_numpy(rows.reshape(-1)).cuda()
    d_lens = torch.from_numpy(np.asarray(lens, dtype=np.int32)).cuda()
    out = []
    for _ in range(2 if twice else 1):
        d_packed = torch.full((cap + GUARD,), SENTINEL, dtype=torch.int16, device="cuda")
        d_index = torch.full((S * 16,), 0xEE, dtype=torch.uint8, device="cuda")
        d_total = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        assert d_packed.data_ptr() % 16 == 0 and (d_rows.data_ptr() + 2 * base) % 16 == (2 * base) % 16
        pack_device(d_rows.data_ptr() + 2 * base, stride, d_lens.data_ptr(), S, d_packed.data_ptr(), cap, d_index.data_ptr(),
                    d_total.data_ptr())
        torch.cuda.synchronize()
        out.append((d_packed.cpu().numpy(), d_index.cpu().numpy().view(capi.PACKED_ROW), int(d_total.cpu()[0])))
    if twice:
        assert all(np.array_equal(a, b) for a, b in zip(out[0][:2], out[1][:2])) and out[0][2] == out[1][2]
    return out[0]


def check_operator(lens, stride, base, seed, cap=None, twice=False):
    S = len(lens)
    rng = np.random.default_rng(seed)
    rows = (rng.integers(-32768, 32768, size=(S, stride)).astype(np.int16) | 1)  # no sample is 0: the padding shows
    want, want_idx = pm.pack([rows[s, :lens[s]] for s in range(S)])
    need = want.size
    if cap is None:
        cap = need
    packed, idx, total = run_operator(rows, lens, stride, base, cap, twice)
    what = (S, stride, base, list(lens[:12]))
    assert total == need, what
    assert np.array_equal(idx, want_idx), what
    n = min(cap, need)
    assert np.array_equal(packed[:n], want[:n]), (what, np.flatnonzero(packed[:n] != want[:n])[:8])
    assert (packed[n:] == SENTINEL).all(), (what, "written beyond the total or at / beyond cap")


WIDTH = 4160  # a row's capacity: 65 * 64 int16, two steps of a copy workgroup and a bit
LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, WIDTH]


@pytest.mark.parametrize("stride,base", [(WIDTH, 0), (WIDTH + 1, 1)])
@pytest.mark.parametrize("S", [1, 3])
def test_operator_small_lengths(S, stride, base):
    """Every length of the set in every position; stride a multiple of 64, and odd with the base moved by one int16 (rows
    at every int16 alignment against their 16-byte aligned places)."""
    for k in range(len(LENGTHS)):
        lens = [LENGTHS[(k + 4 * i) % len(LENGTHS)] for i in range(S)]
        check_operator(lens, stride, base, 100 * S + k, twice=(k == 0))


@pytest.mark.parametrize("stride,base", [(24, 0), (64, 0), (25, 1)])
def test_operator_more_streams_than_a_scan_chunk(stride, base):
    S = 9001
    lens = [(7 * s + s // 1000) % 18 for s in range(S)]
    assert set(lens) == set(range(18))
    check_operator(lens, stride, base, 9001, twice=True)


def test_operator_all_empty_and_cap_one_short():
    for S in (1, 3, 2500):
        rows = np.ones((S, 64), dtype=np.int16)
        packed, idx, total = run_operator(rows, [0] * S, 64, 0, 16)
        assert total == 0 and not idx["offset"].any() and not idx["len"].any() and not idx["held"].any()
        assert (packed == SENTINEL).all()
    # one short of the need: the total says so, and nothing lands at or beyond cap
    for lens, stride, base in (([65, 9, WIDTH], WIDTH + 1, 1), ([8], WIDTH, 0), ([5, 3], 64, 0), ([WIDTH, 2048 + 64], WIDTH, 0)):
        need = sum(pm.round8(n) for n in lens)
        check_operator(lens, stride, base, 5, cap=need - 1)
    check_operator([3000, 3000, 3000], WIDTH, 0, 6, cap=4003)  # cap inside the second row, not a multiple of 8
    lib = capi.load()
    d = torch.zeros(64, dtype=torch.int16, device="cuda")
    p = d.data_ptr()
    assert lib.rtlfm_gpu_pack_device(0, p, 8, p, 1, p + 2, 8, p, p, None) == -errno.EINVAL  # d_packed not 16-byte aligned
    assert lib.rtlfm_gpu_pack_device(0, p, 8, p, 0, p, 8, p, p, None) == -errno.EINVAL
    assert lib.rtlfm_gpu_pack_device(99, p, 8, p, 1, p, 8, p, p, None) == -errno.ENODEV


# ------------------------------------------------------------------ the ring's helpers ----

L = 2048
RUNS = (1, 3, 2)
CAP = 3
CONSEQ = 1


def fetch_rows(g):
    o, n = g.fetch_all()
    return [o[s, :n[s]].copy() for s in range(g.nstreams)]


def push_buffers(g, bufs, b0, nb):
    """bufs[row][k]: buffer k of ring row `row`."""
    for i, row in enumerate(bufs):
        for buf in row[b0:b0 + nb]:
            g.push(buf, i)


def assert_packed(got, rows, held, what):
    """got = fetch_packed()'s pair against the rows and held counts it should hold, in every byte."""
    packed, idx = got
    want, want_idx = pm.pack(rows, held)
    assert np.array_equal(idx, want_idx), (what, idx, want_idx)
    assert np.array_equal(packed, want), (what, np.flatnonzero(packed != want)[:8] if packed.size == want.size else (packed.size, want.size))


def fails(g, name, value, code):
    before = g.get_option(name)
    with pytest.raises(capi.RtlfmError) as e:
        g.set_option(name, value)
    assert e.value.code == code, (name, value, e.value.code)
    assert g.get_option(name) == before


# ------------------------------------------------------ 2. mode 1 through the ring ----

def keyed_buffers(S, n, seed):
    """Loud and quiet buffers: stream 0 always loud, stream 1 never, the others keyed."""
    rng = np.random.default_rng(seed)
    loud = np.zeros((S, n), dtype=bool)
    loud[0] = True
    loud[2] = [True, True, False, False, False, True, True, False][:n]
    loud[3] = [False, False, False, True, False, False, False, False][:n]
    loud[4:] = rng.random((S - 4, n)) < 0.5
    return [[sm.tone_or_noise(rng, L, bool(loud[s][k])) for k in range(n)] for s in range(S)]


@pytest.mark.parametrize("ragged", [False, True])
def test_mode1_equals_fetch_all(ragged):
    """box84_fm_squelch50-style behind the squelch gate: some rows empty, some partial, some full - the packed rows are
    fetch_all's of the same run, held is 0; the same on a run whose last buffer is 512 bytes for one stream."""
    S = 5
    cfg = make_cfg(case("box84_fm_squelch50")[0], L, CAP)
    bufs = keyed_buffers(S, sum(RUNS), 21)
    if ragged:
        bufs[3][3] = bufs[3][3][:512]  # the last buffer of the second run
    kinds = set()
    with demod(cfg, S, conseq_squelch=CONSEQ, squelch_gate=1, pack_results=1) as g:
        b0 = 0
        for nb in RUNS:
            push_buffers(g, bufs, b0, nb)
            g.run()
            rows = fetch_rows(g)
            assert_packed(g.fetch_packed(), rows, None, ("mode 1", ragged, b0))
            full = max(len(r) for r in rows)
            kinds |= {"empty" if len(r) == 0 else "full" if len(r) == full else "partial" for r in rows}
            b0 += nb
    assert kinds == {"empty", "partial", "full"}


def test_mode1_under_channels_and_verify_twice():
    """Mode 1 needs nothing of the configuration: channels on, no squelch, -M raw rows of a boxcar that does not divide
    the buffer; under verify_twice the pack runs once, behind the comparison."""
    nsrc, per = 2, 3
    cfg = raw_cfg(7, L, CAP)
    steps = make_steps_special(nsrc * per, 3)
    src = full_scale(nsrc, sum(RUNS) * L, 31)
    bufs = [[src[i, k * L:(k + 1) * L] for k in range(sum(RUNS))] for i in range(nsrc)]
    for verify in (0, 1):
        with demod(cfg, nsrc * per, source_ring=1, pack_results=1, verify_twice=verify) as g:
            g.set_channels(per, steps=steps)
            b0 = 0
            for nb in RUNS:
                push_buffers(g, bufs, b0, nb)
                g.run()
                assert_packed(g.fetch_packed(), fetch_rows(g), None, ("channels mode 1", verify, b0))
                b0 += nb
            if verify:
                assert g.get_option("verify_runs") == len(RUNS) and g.get_option("verify_mismatches") == 0


# ----------------------------------------------- 3. mode 2 under channels, source ring ----

BOUND = 89
FIR_TAPS, FIR_SHIFT = random_fir_taps(33, 5)
BANK_K = 4
BANK_TAPS, BANK_SHIFT = random_bank_taps(BANK_K, 24, 6)
FRONTS = ("box10_fm", "box7_raw", "fir33", "bank4")
# loud[source][buffer] over runs of 1, 3 and 2 buffers, conseq 1 (held from the second quiet buffer in a row on):
#   source 0: the hold begins with the LAST buffer of the second run, lasts into the third and ends inside it
#   source 1: held from the start (squelch_hits starts at 11, far above conseq + 1), open again in the middle of the second run
#   source 2: the hold begins in the MIDDLE of the second run and lasts to the end
LOUD = np.array([[1, 1, 0, 0, 0, 1],
                 [0, 0, 0, 1, 1, 0],
                 [1, 0, 0, 0, 0, 0]], dtype=bool)
WANT_HELD = np.array([[0, 0, 0, 1, 1, 0],
                      [1, 1, 1, 0, 0, 0],
                      [0, 0, 1, 1, 1, 1]], dtype=bool)


def front_cfg(front, level):
    if front == "box10_fm":
        return make_cfg(dict(case("c1_boxcar10_fast")[0], squelch_level=level), L, CAP)
    return raw_cfg(7 if front == "box7_raw" else 10, L, CAP, squelch_level=level)


def open_front(front, cfg, nsrc, per, steps, path, **options):
    g = demod(cfg, nsrc * per, source_ring=1, conseq_squelch=CONSEQ, **options)
    try:
        g.set_path(path)
        g.set_channels(per, steps=steps)
        if front == "fir33":
            g.set_channel_filter(FIR_TAPS, FIR_SHIFT)
        if front == "bank4":
            g.set_channel_bank(BANK_K, BANK_TAPS, BANK_SHIFT, bins=[(3 * c + 1) % BANK_K for c in range(per)])
    except BaseException:
        g.close()
        raise
    return g


def channel_sources(front, nsrc, seed):
    """Loud buffers: bounded where the oracle reads the mixed samples as bytes, full scale behind the -M raw boxcar, and
    +-20 behind the filter and the bank - their random taps have a gain of about a hundred, and rms()'s uint32 sum of
    squares (src/rtl_fm.c:1093-1098) wraps on full-scale input: the levels would say nothing.  Quiet ones: 127 +- 1."""
    n = sum(RUNS)
    loud = (bounded(nsrc, n * L, seed, BOUND) if front == "box10_fm" else full_scale(nsrc, n * L, seed) if front == "box7_raw"
            else bounded(nsrc, n * L, seed, 20))
    quiet = bounded(nsrc, n * L, seed + 1, 1)
    src = quiet.copy()
    for i in range(nsrc):
        for k in range(n):
            if LOUD[i][k]:
                src[i, k * L:(k + 1) * L] = loud[i, k * L:(k + 1) * L]
    return src


def ring_runs(g, src, collect):
    bufs = [[src[i, k * L:(k + 1) * L] for k in range(sum(RUNS))] for i in range(src.shape[0])]
    out, b0 = [], 0
    for nb in RUNS:
        push_buffers(g, bufs, b0, nb)
        g.run()
        out.append(collect(g))
        b0 += nb
    return out


def pick_level(front, nsrc, per, steps, path, src):
    """The squelch level between the two kinds of buffer, from the levels themselves (they do not depend on it): a handle
    with the squelch at 1, so that nothing is below it.  A quiet buffer behind a loud one carries the filter's tail and
    is the loudest of the quiet ones."""
    with open_front(front, front_cfg(front, 1), nsrc, per, steps, path) as g:
        lv = np.concatenate(ring_runs(g, src, lambda g: g.levels_all()), axis=1)
    loud = np.repeat(LOUD[:nsrc], per, axis=0)
    lo, hi = int(lv[~loud].max()), int(lv[loud].min())
    assert 0 <= lo and 2 * (lo + 1) < hi, (front, lo, hi)
    return int(np.sqrt((lo + 1) * hi))


def oracle_runs(cfg, src, steps, per):
    """(b): the mixed bytes through the oracle buffer by buffer, the demod thread's rule on its state after each
    (scan_model.StreamModel's lines).  Per run (rows, held)."""
    states, out, k = None, [], 0
    S = len(steps)
    for nb in RUNS:
        rows, held = [[] for _ in range(S)], [0] * S
        for _ in range(nb):
            o, n, states = cm.model_via_oracle(cfg, src[:, k * L:(k + 1) * L], steps, per, k * (L // 2), states)
            for s in range(S):
                if states[s].squelch_hits > CONSEQ:       # src/rtl_fm.c:1366
                    states[s].squelch_hits = CONSEQ + 1   # :1368
                    held[s] += 1
                else:
                    rows[s].append(o[s, :n[s]].copy())
            k += 1
        out.append(([np.concatenate(r) if r else np.zeros(0, dtype=np.int16) for r in rows], held))
    return out


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("nsrc", [1, 3])
@pytest.mark.parametrize("front", FRONTS)
def test_mode2_under_channels(oracle_lib, front, nsrc, path):
    per = 4
    seed = 10 * FRONTS.index(front) + nsrc
    steps = make_steps_special(nsrc * per, seed)
    src = channel_sources(front, nsrc, seed)
    level = 60 if front == "box10_fm" else pick_level(front, nsrc, per, steps, path, src)
    cfg = front_cfg(front, level)
    # (a) the twin: the option off
    with open_front(front, cfg, nsrc, per, steps, path) as g:
        twin = ring_runs(g, src, lambda g: (fetch_rows(g), g.levels_all(), g.last_path))
        twin_state = bytes(g.state_get_all())
    gate = pm.Gate(nsrc * per, L // 2, int(cfg.downsample), 2 if cfg.mode == MODE_RAW else 1, level, CONSEQ)
    want = [gate.run(rows, lv) for rows, lv, _ in twin]
    held = np.concatenate([np.array([[sr < level for sr in row] for row in lv]) for _, lv, _ in twin], axis=1)
    assert np.array_equal(held, np.repeat(~LOUD[:nsrc], per, axis=0)), "the buffers are not as loud and quiet as arranged"
    assert [sum(h[s] for _, h in want) for s in range(nsrc * per)] == np.repeat(WANT_HELD[:nsrc].sum(axis=1), per).tolist()
    assert [h[0] for _, h in want] == [0, 1, 1], "source 0: a hold that begins in one run and ends inside the next"
    with open_front(front, cfg, nsrc, per, steps, path, pack_results=2) as g:
        fails(g, "squelch_gate", 1, -errno.ENOTSUP)  # channels are on
        got = ring_runs(g, src, lambda g: (g.fetch_packed(), fetch_rows(g), g.last_path))
        state = bytes(g.state_get_all())
    for r, ((packed, rows, p), (w_rows, w_held)) in enumerate(zip(got, want)):
        assert p == twin[r][2] == (1 if path == 1 else 2)
        assert_packed(packed, w_rows, w_held, (front, nsrc, path, "run", r))
        for s, (a, b) in enumerate(zip(rows, twin[r][0], strict=True)):
            assert np.array_equal(a, b), ("fetch_all beside the packed form", r, s)
    assert state == twin_state, "the pack wrote to the carried state"
    if front == "box10_fm":
        for r, ((packed, _, _), (o_rows, o_held)) in enumerate(zip(got, oracle_runs(cfg, src, steps, per))):
            assert_packed(packed, o_rows, o_held, (front, nsrc, path, "oracle, run", r))


# ------------------------------------------------------- 4. mode 2 without channels ----

BOX7 = dict(mode=MODE_FM, downsample=7, custom_atan=ATAN_FAST)
LEVEL = 60  # between +-1 noise and a tone of amplitude 100 behind /7 (tests/test_scan_gpu.py)


def plain_case(S=5):
    cfg = RtlfmCfg.default(block_len=L, max_blocks=CAP, squelch_level=LEVEL, **BOX7)
    return cfg, keyed_buffers(S, sum(RUNS), 41)


def twin_gate_runs(cfg, bufs):
    """A twin handle's squelch_gate output per run: (rows, held per stream)."""
    out, b0 = [], 0
    with demod(cfg, len(bufs), conseq_squelch=CONSEQ, squelch_gate=1) as g:
        for nb in RUNS:
            push_buffers(g, bufs, b0, nb)
            g.run()
            out.append((fetch_rows(g), (g.gate()["emit"] == 0).sum(axis=1).tolist()))
            b0 += nb
    return out


def test_mode2_equals_a_twins_squelch_gate():
    cfg, bufs = plain_case()
    want = twin_gate_runs(cfg, bufs)
    assert any(any(h) for _, h in want) and any(len(r) == 0 for rows, _ in want for r in rows)
    with demod(cfg, len(bufs), conseq_squelch=CONSEQ, pack_results=2) as g:
        b0 = 0
        for r, nb in enumerate(RUNS):
            push_buffers(g, bufs, b0, nb)
            g.run()
            assert_packed(g.fetch_packed(), want[r][0], want[r][1], ("mode 2, no channels, run", r))
            b0 += nb


def test_prev_fetches_the_run_before():
    cfg, bufs = plain_case()
    want = twin_gate_runs(cfg, bufs)
    lib = capi.load()
    idx = np.zeros(len(bufs), dtype=capi.PACKED_ROW)
    total = C.c_size_t()
    with demod(cfg, len(bufs), conseq_squelch=CONSEQ, pack_results=2) as g:
        out = np.zeros(1 << 16, dtype=np.int16)
        assert lib.rtlfm_gpu_fetch_packed(g._h, out.ctypes.data, out.size, idx.ctypes.data, C.byref(total)) == -errno.EAGAIN
        push_buffers(g, bufs, 0, 1)
        g.run()
        assert lib.rtlfm_gpu_fetch_packed_prev(g._h, out.ctypes.data, out.size, idx.ctypes.data, C.byref(total)) == -errno.EAGAIN
        push_buffers(g, bufs, 1, 3)
        g.run()
        assert_packed(g.fetch_packed(prev=True), want[0][0], want[0][1], "prev: run 0")
        assert_packed(g.fetch_packed(), want[1][0], want[1][1], "last: run 1")
        push_buffers(g, bufs, 4, 2)
        g.run()
        assert_packed(g.fetch_packed(prev=True), want[1][0], want[1][1], "prev: run 1")
        # too small: the need is reported, out is untouched
        out[:] = 77
        need = sum(pm.round8(len(r)) for r in want[2][0])
        assert need > 8
        assert lib.rtlfm_gpu_fetch_packed(g._h, out.ctypes.data, need - 1, idx.ctypes.data, C.byref(total)) == -errno.ENOBUFS
        assert total.value == need and (out == 77).all()
        assert_packed(g.fetch_packed(), want[2][0], want[2][1], "last: run 2")


# --------------------------------------------------------- 5. refusals, off is off ----

def run_and_compare(g, cfg, bufs, what):
    """A run of the handle equals the same run of a handle that has seen none of this."""
    push_buffers(g, bufs, 0, len(bufs[0]))
    g.run()
    got = fetch_rows(g)
    with demod(cfg, len(bufs)) as twin:
        push_buffers(twin, bufs, 0, len(bufs[0]))
        twin.run()
        want = fetch_rows(twin)
    for s, (a, b) in enumerate(zip(got, want, strict=True)):
        assert np.array_equal(a, b), (what, s)


def test_refusals_change_nothing():
    rng = np.random.default_rng(9)
    two = lambda n, S=2: [[sm.tone_or_noise(rng, n, bool((s + k) % 2)) for k in range(2)] for s in range(S)]  # noqa: E731
    # no squelch: -EINVAL; other values: -EINVAL
    cfg = RtlfmCfg.default(block_len=L, max_blocks=2, **BOX7)
    with demod(cfg, 2) as g:
        for v in (2, 3, -1):
            fails(g, "pack_results", v, -errno.EINVAL)
        run_and_compare(g, cfg, two(L), "no squelch")
    # a resampler, low_pass_simple, passes that do not divide the buffer: -ENOTSUP
    for kw, n in ((dict(mode=MODE_FM, downsample=6, custom_atan=ATAN_FAST, rate_out=170000, rate_out2=32000,
                        resampler=RESAMPLE_LOW_PASS_REAL), L),
                  (dict(mode=MODE_FM, downsample=8, custom_atan=ATAN_FAST, post_downsample=2), L),
                  (dict(mode=MODE_FM, downsample=512, downsample_passes=9, custom_atan=ATAN_FAST), 1536)):
        cfg = RtlfmCfg.default(block_len=n, max_blocks=2, squelch_level=LEVEL, **kw)
        with demod(cfg, 2) as g:
            fails(g, "pack_results", 2, -errno.ENOTSUP)
            g.set_option("pack_results", 1)  # mode 1 takes every configuration
            g.set_option("pack_results", 0)
            run_and_compare(g, cfg, two(n), kw)
    # the gate and mode 2 exclude each other, either way round
    cfg = RtlfmCfg.default(block_len=L, max_blocks=2, squelch_level=LEVEL, **BOX7)
    with demod(cfg, 2, squelch_gate=1) as g:
        fails(g, "pack_results", 2, -errno.EINVAL)
        g.set_option("squelch_gate", 0)
        run_and_compare(g, cfg, two(L), "gate first")
    with demod(cfg, 2, pack_results=2) as g:
        fails(g, "squelch_gate", 1, -errno.EINVAL)
        assert g.get_option("pack_results") == 2
        run_and_compare(g, cfg, two(L), "mode 2 first")
        # while a run is begun: -EBUSY
        push_buffers(g, two(L), 0, 2)
        assert g.run_begin() == 2
        for v in (0, 1):
            fails(g, "pack_results", v, -errno.EBUSY)
        g.run_end()
        g.fetch_packed()
    # a ragged run in mode 2: -ENOTSUP from run_begin, nothing is taken; reset empties the ring
    with demod(cfg, 2, pack_results=2) as g:
        bufs = two(L)
        bufs[1][1] = bufs[1][1][:512]
        push_buffers(g, bufs, 0, 2)
        assert g.lib.rtlfm_gpu_run_begin(g._h, None) == -errno.ENOTSUP
        assert g.lib.rtlfm_gpu_run_begin(g._h, None) == -errno.ENOTSUP  # still there
        assert g.get_option("pack_results") == 2
        g.reset()
        run_and_compare(g, cfg, two(L), "behind the refused ragged run")
        g.fetch_packed()


def test_off_is_off():
    """pack_results 0: -ENODATA, and results, state and timing_read's launch count are those of a handle that never heard
    of the option - also after it was on and went back to 0."""
    cfg, bufs = plain_case()
    res = {}
    for kind in ("never", "off", "on_then_off"):
        with demod(cfg, len(bufs), conseq_squelch=CONSEQ) as g:
            if kind == "off":
                g.set_option("pack_results", 0)
            g.timing_enable(True)
            g.timing_read()
            if kind == "on_then_off":
                g.set_option("pack_results", 2)
                push_buffers(g, bufs, 0, 1)
                g.run()
                g.fetch_packed()
                assert g.get_option("pack_us") >= 0
                g.set_option("pack_results", 0)
                g.reset()
                g.timing_read()
            rows, b0 = [], 0
            for nb in RUNS:
                push_buffers(g, bufs, b0, nb)
                g.run()
                r = fetch_rows(g)
                with pytest.raises(capi.RtlfmError) as e:
                    g.fetch_packed()
                assert e.value.code == -errno.ENODATA
                assert g.get_option("pack_us") == -1
                rows.append((r, bytes(g.state_get_all()), g.timing_read()[1]))
                b0 += nb
            res[kind] = rows
    for kind in ("off", "on_then_off"):
        for a, b in zip(res["never"], res[kind], strict=True):
            assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0], strict=True)) and a[1] == b[1] and a[2] == b[2], kind
