"""The source-indexed ring (option source_ring; include/rtlfm_hip.h, "The ring and channels"): with channels on, push /
acquire / commit take the SOURCE's index, a run copies one row per source and demodulates every channel of it, and the
results come back per stream.  Everything here goes through rtlfm_gpu_push ... rtlfm_gpu_fetch*, against the models of
tests/channel_model.py, channel_fir_model.py and channel_bank_model.py and against a second handle that is fed the same
bytes through rtlfm_gpu_run_device.

Comparison: equality of every bit (channel_common.assert_rows) - between the two handles always, and against the model
on the integer paths; -M fm with -A std (p2_fir9) gets assert_row_cfg's stated tolerance against the oracle only.

Inputs for the oracle-backed models keep |I - 127|, |Q - 127| <= 89 (the mixed samples must fit the bytes the oracle
reads); the filter and the bank run -M raw on full-scale bytes."""
import ctypes as C
import errno
import threading

import numpy as np
import pytest

import channel_model as cm
from cases import case, make_cfg
from channel_bank_model import BankModel
from channel_common import (assert_row_cfg, assert_rows, bounded, demod, full_scale, make_steps_special,
                            random_bank_taps, random_fir_taps, raw_cfg, run_gpu_per_run, to_device)
from channel_fir_model import FirModel, raw_rows
from rtlsdr_amd import synth
from rtlsdr_amd.capi import MODE_RAW

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BOUND = 89
RUNS = (1, 3, 2)  # 1, cap and 2 buffers
CAP = 3
D = 10
FIR_TAPS, FIR_SHIFT = random_fir_taps(33, 5)
BANK_K = 4
BANK_TAPS, BANK_SHIFT = random_bank_taps(BANK_K, 24, 6)
FRONTS = ("boxcar", "fir33", "bank4", "p2_fir9")


def bank_bins(per):
    """A subset of the four bins, in an order of its own; more channels than bins repeat one."""
    return [(3 * c + 1) % BANK_K for c in range(per)]


def front_cfg(front, L, nb=CAP, **ov):
    if front == "boxcar":
        return make_cfg(dict(case("c1_boxcar10_fast")[0], **ov), L, nb)
    if front == "p2_fir9":
        return make_cfg(dict(case("p2_fir9")[0], **ov), L, nb)
    return raw_cfg(D, L, nb, **ov)


def source_bytes(front, nsrc, nbytes, seed):
    return bounded(nsrc, nbytes, seed, BOUND) if front in ("boxcar", "p2_fir9") else full_scale(nsrc, nbytes, seed)


def open_handle(front, cfg, nsrc, per, steps, source_ring=1, **options):
    g = demod(cfg, nsrc * per, **options)
    try:
        if source_ring:
            g.set_option("source_ring", 1)
        g.set_channels(per, steps=steps)
        if front == "fir33":
            g.set_channel_filter(FIR_TAPS, FIR_SHIFT)
        if front == "bank4":
            g.set_channel_bank(BANK_K, BANK_TAPS, BANK_SHIFT, bins=bank_bins(per))
    except BaseException:
        g.close()
        raise
    return g


class Model:
    """The front end's model over consecutive runs of whole source bytes: rows per stream, and what it knows of the state
    (the oracle: the whole record; the filter's and the bank's models: prev_index)."""

    def __init__(self, front, cfg, nsrc, per, steps):
        self.front, self.cfg, self.nsrc, self.per, self.steps = front, cfg, nsrc, per, steps
        self.pos, self.states = 0, None
        self.box = None  # model_raw_boxcar's carried state (-M raw behind the boxcar)
        if front == "fir33":
            self.m = FirModel(steps, per, int(cfg.downsample), FIR_TAPS, FIR_SHIFT, nsrc)
        if front == "bank4":
            self.m = BankModel(BANK_K, BANK_TAPS, BANK_SHIFT, int(cfg.downsample), nsrc, bins=bank_bins(per))

    def run(self, src):
        """src: uint8 [sources, bytes of the run].  Per stream the run's rows."""
        if self.front in ("fir33", "bank4"):
            return raw_rows(*self.m.run(src))
        if self.cfg.mode == MODE_RAW:  # -M raw behind the boxcar: any number of bytes, full scale
            rows, self.box = cm.model_raw_boxcar(src, self.steps, int(self.cfg.downsample), self.box, per_source=self.per, pos=self.pos)
            self.pos += src.shape[1] // 2
            return rows
        out, n, self.states = cm.model_via_oracle(self.cfg, src, self.steps, self.per, self.pos, self.states)
        self.pos += src.shape[1] // 2
        return [out[s, :n[s]].copy() for s in range(self.nsrc * self.per)]

    def check_state(self, st, what):
        for s in range(self.nsrc * self.per):
            if self.front in ("fir33", "bank4"):
                assert st[s].prev_index == self.m.p0[s], (what, s)
            elif self.box is not None:
                assert {k: getattr(st[s], k) for k in ("now_r", "now_j", "prev_index")} == self.box[s], (what, s)
            else:
                assert st[s].as_dict() == self.states[s].as_dict(), (what, s)


def push_run(g, src, pieces, how="push"):
    """One run's buffers into the ring: pieces = (offset, length) of every buffer, the same for all sources."""
    for i in range(src.shape[0]):
        for at, n in pieces:
            if how == "push":
                g.rtlsdr_callback(src[i, at:at + n], stream=i)
            else:
                acquire_commit(g, i, src[i, at:at + n])


def acquire_commit(g, i, buf):
    p, cap = C.c_void_p(), C.c_uint32()
    assert g.lib.rtlfm_gpu_acquire(g._h, i, C.byref(p), C.byref(cap)) == 0
    assert cap.value == g.cfg.block_len
    b = np.ascontiguousarray(buf)
    C.memmove(p.value, b.ctypes.data, b.size)
    assert g.lib.rtlfm_gpu_commit(g._h, i, b.size) == 0


def fetch_rows(g):
    o, n = g.fetch_all()
    return [o[s, :n[s]].copy() for s in range(g.nstreams)]


def ring_runs(g, src, L, runs, how="push"):
    """Consecutive full-length runs over the ring: (per run per stream rows, last_path of every run)."""
    per_run, paths, b0 = [], [], 0
    for nb in runs:
        push_run(g, src, [((b0 + j) * L, L) for j in range(nb)], how)
        g.full_demod()
        per_run.append(fetch_rows(g))
        paths.append(g.last_path)
        b0 += nb
    return per_run, paths


def joined(per_run):
    return [np.concatenate([r[s] for r in per_run]) for s in range(len(per_run[0]))]


def compare_model(front, cfg, got, want, what):
    if front == "p2_fir9":
        for s, (a, b) in enumerate(zip(got, want, strict=True)):
            assert_row_cfg(a, b, cfg, f"{what} stream {s}")
    else:
        assert_rows(got, want, what)


# ------------------------------------------------ 1. the ring, run_device, the model ----

@pytest.mark.parametrize("L", [512, 16384])
@pytest.mark.parametrize("per", [1, 4, 5])
@pytest.mark.parametrize("nsrc", [1, 3])
@pytest.mark.parametrize("front", FRONTS)
def test_ring_equals_run_device_and_the_model(oracle_lib, front, nsrc, per, L):
    """Runs of 1, 3 (the ring's capacity) and 2 buffers pushed per SOURCE: PCM, lengths and state records of every stream
    equal the model and, in every bit, a second handle fed the same bytes through rtlfm_gpu_run_device; last_path too."""
    seed = FRONTS.index(front) * 100 + nsrc * 10 + per + L
    cfg = front_cfg(front, L)
    steps = make_steps_special(nsrc * per, seed)
    src = source_bytes(front, nsrc, sum(RUNS) * L, seed)
    model = Model(front, cfg, nsrc, per, steps)
    b0, want = 0, []
    for nb in RUNS:
        want.append(model.run(src[:, b0 * L:(b0 + nb) * L]))
        b0 += nb
    with open_handle(front, cfg, nsrc, per, steps) as g:
        assert g.get_option("source_ring") == 1 and g.sources == nsrc
        got, paths = ring_runs(g, src, L, RUNS)
        st = g.state_get_all()
        got_st = bytes(st)
        assert g.channels_tell() == sum(RUNS) * L // 2
    with open_handle(front, cfg, nsrc, per, steps, source_ring=0) as g:
        assert g.sources == nsrc * per
        _, dev, dev_paths = run_gpu_per_run(g, src, L, RUNS)
        dev_st = bytes(g.state_get_all())
    assert paths == dev_paths == [1 if front == "p2_fir9" else 2] * len(RUNS), (paths, dev_paths)
    for r in range(len(RUNS)):
        assert_rows(got[r], dev[r], f"{front} run {r} ring / run_device")
    assert got_st == dev_st
    compare_model(front, cfg, joined(got), joined(want), front)
    model.check_state(st, front)


# ------------------------------------------------------------ 2. acquire / commit ----

def test_acquire_commit_equal_push_and_an_open_slot_holds_the_run(oracle_lib):
    nsrc, per, L = 3, 4, 2048
    cfg = front_cfg("boxcar", L)
    steps = make_steps_special(nsrc * per, 2)
    src = source_bytes("boxcar", nsrc, sum(RUNS) * L, 2)
    model = Model("boxcar", cfg, nsrc, per, steps)
    want = model.run(src)
    with open_handle("boxcar", cfg, nsrc, per, steps) as g:
        got, paths = ring_runs(g, src, L, RUNS, how="acquire")
        st = g.state_get_all()
        # a slot of source 1 out between acquire and commit: the run waits (-EAGAIN, nothing taken), then goes
        tail = source_bytes("boxcar", nsrc, L, 3)
        for i in (0, 2):
            g.rtlsdr_callback(tail[i], stream=i)
        p, cap = C.c_void_p(), C.c_uint32()
        assert g.lib.rtlfm_gpu_acquire(g._h, 1, C.byref(p), C.byref(cap)) == 0
        assert g.lib.rtlfm_gpu_run_begin(g._h, None) == -errno.EAGAIN
        assert g.lib.rtlfm_gpu_acquire(g._h, 1, C.byref(p), C.byref(cap)) == -errno.EBUSY
        C.memmove(p.value, tail[1].ctypes.data, L)
        assert g.lib.rtlfm_gpu_commit(g._h, 1, L) == 0
        g.full_demod()
        last = fetch_rows(g)
    assert paths == [2] * len(RUNS)
    assert_rows(joined(got), want, "acquire / commit")
    model.check_state(st, "acquire / commit")
    assert_rows(last, model.run(tail), "the run behind the open slot")


# ------------------------------------------------------------------------ 3. pos ----

@pytest.mark.parametrize("front", ["boxcar", "fir33", "bank4"])
def test_ring_and_run_device_alternate_at_one_pos(oracle_lib, front):
    """ring, run_device, ring, run_device on ONE handle: channels_tell counts both, the history (filter, bank) changes
    over once per run of either kind, and the output is the model's at one continuous pos."""
    nsrc, per, L = 2, 4, 2048
    kinds = ("ring", "device", "ring", "device", "ring")
    nbs = (2, 1, 3, 2, 1)
    cfg = front_cfg(front, L)
    steps = make_steps_special(nsrc * per, 7)
    src = source_bytes(front, nsrc, sum(nbs) * L, 70 + len(front))
    model = Model(front, cfg, nsrc, per, steps)
    with open_handle(front, cfg, nsrc, per, steps) as g:
        d = to_device(src)
        b0 = 0
        for kind, nb in zip(kinds, nbs):
            if kind == "ring":
                push_run(g, src, [((b0 + j) * L, L) for j in range(nb)])
                g.full_demod()
                got = fetch_rows(g)
            else:
                o, n = g.run_torch(d[:, b0 * L:(b0 + nb) * L].contiguous())
                g.sync()
                o, n = o.cpu().numpy(), n.cpu().numpy()
                got = [o[s, :n[s]].copy() for s in range(g.nstreams)]
            b0 += nb
            assert g.channels_tell() == b0 * L // 2, (kind, b0)
            assert_rows(got, model.run(src[:, (b0 - nb) * L:b0 * L]), f"{front} {kind} run up to buffer {b0}")
        model.check_state(g.state_get_all(), front)


@pytest.mark.parametrize("front", ["boxcar", "fir33"])
def test_verify_twice_over_the_ring(oracle_lib, front):
    """Both executions of a ring run see one pos and one history, and pos moves on once."""
    nsrc, per, L = 2, 3, 2048
    cfg = front_cfg(front, L)
    steps = make_steps_special(nsrc * per, 8)
    src = source_bytes(front, nsrc, 4 * L, 80)
    model = Model(front, cfg, nsrc, per, steps)
    want = [model.run(src[:, :2 * L]), model.run(src[:, 2 * L:])]
    with open_handle(front, cfg, nsrc, per, steps, verify_twice=1) as g:
        got, _ = ring_runs(g, src, L, (2, 2))
        assert g.channels_tell() == 4 * L // 2
        assert g.get_option("verify_runs") == 2 and g.get_option("verify_mismatches") == 0
    assert_rows(joined(got), joined(want), f"{front} verify_twice")


# --------------------------------------------------------------- 4. short buffers ----

SHORT_L = 4096


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("short", [512, 1536, SHORT_L - 512])
@pytest.mark.parametrize("front", ["boxcar", "fir33", "bank4"])
def test_short_last_buffer_equals_the_model_on_the_concatenated_bytes(oracle_lib, front, short, path):
    """A run of 3 buffers whose last is short on BOTH sources, -M raw on full-scale bytes: what comes out is the model's
    on the bytes as one piece; a full-length run behind it continues it - history and pos intact -, and so does a run
    that is short buffers only."""
    nsrc, per, L = 2, 3, SHORT_L
    cfg = raw_cfg(D, L, CAP)
    steps = make_steps_special(nsrc * per, short)
    n1 = 2 * L + short
    src = full_scale(nsrc, n1 + 2 * L + short + 512, short + len(front))
    model = Model(front, cfg, nsrc, per, steps)
    with open_handle(front, cfg, nsrc, per, steps) as g:
        g.set_path(path)
        at = 0
        for pieces in ([L, L, short], [L, L], [short, 512]):
            push_run(g, src, [(at + sum(pieces[:j]), n) for j, n in enumerate(pieces)])
            g.full_demod()
            got = fetch_rows(g)
            assert g.last_path == (1 if path == 1 else 2)
            assert_rows(got, model.run(src[:, at:at + sum(pieces)]), f"{front} path {path} buffers of {pieces}")
            at += sum(pieces)
            assert g.channels_tell() == at // 2
        model.check_state(g.state_get_all(), front)


def test_short_buffer_behind_fifth_order_passes_goes_staged(oracle_lib):
    """p2_fir9 (path 1 behind k_channel_mix): a short last buffer the passes divide.  The reference's generic_fir starts
    every buffer anew, so the expectation is the oracle on buffers of these very lengths: two of L, two of L / 2."""
    nsrc, per, L = 2, 2, SHORT_L
    cfg = front_cfg("p2_fir9", L)
    steps = make_steps_special(nsrc * per, 4)
    src = bounded(nsrc, 3 * L, 44, BOUND)
    w0, n0, carried = cm.model_via_oracle(cfg, src[:, :2 * L], steps, per, 0)
    w1, n1, _ = cm.model_via_oracle(cm.copy_cfg(cfg, block_len=L // 2), src[:, 2 * L:], steps, per, L, carried)
    with open_handle("p2_fir9", cfg, nsrc, per, steps) as g:
        push_run(g, src, [(0, L), (L, L), (2 * L, L // 2)])
        g.full_demod()
        a = fetch_rows(g)
        push_run(g, src, [(2 * L + L // 2, L // 2)])
        g.full_demod()
        b = fetch_rows(g)
        assert g.last_path == 1 and g.channels_tell() == 3 * L // 2
    for s in range(nsrc * per):
        assert_row_cfg(np.concatenate([a[s], b[s]]), np.concatenate([w0[s, :n0[s]], w1[s, :n1[s]]]), cfg, f"p2_fir9 stream {s}")


@pytest.mark.parametrize("front", ["boxcar", "fir33"])
def test_lengths_that_differ_between_sources_are_refused(oracle_lib, front):
    """pos is one counter per handle: -ERANGE, nothing taken, pos unchanged; rtlfm_gpu_reset empties the ring and the
    handle runs from pos 0."""
    nsrc, per, L = 2, 3, SHORT_L
    cfg = raw_cfg(D, L, CAP)
    steps = make_steps_special(nsrc * per, 17)
    src = full_scale(nsrc, 3 * L, 18)
    with open_handle(front, cfg, nsrc, per, steps) as g:
        push_run(g, src, [(0, L)])
        g.full_demod()
        fetch_rows(g)
        g.rtlsdr_callback(src[0, L:2 * L], stream=0)
        g.rtlsdr_callback(src[0, 2 * L:2 * L + 512], stream=0)
        g.rtlsdr_callback(src[1, L:2 * L], stream=1)
        g.rtlsdr_callback(src[1, 2 * L:2 * L + 1024], stream=1)
        taken = C.c_int(-1)
        for _ in range(2):
            assert g.lib.rtlfm_gpu_run_begin(g._h, C.byref(taken)) == -errno.ERANGE
            assert taken.value == -1 and g.channels_tell() == L // 2
        assert g.lib.rtlfm_gpu_run_end(g._h) == -errno.EINVAL  # nothing was begun
        # the buffers are still there: a third one for source 0 is one too many for equal counts
        g.rtlsdr_callback(src[0, :L], stream=0)
        assert g.lib.rtlfm_gpu_run_begin(g._h, None) == -errno.EAGAIN
        g.reset()
        assert g.channels_tell() == 0
        model = Model(front, cfg, nsrc, per, steps)
        push_run(g, src, [(L, L), (2 * L, 1024)])
        g.full_demod()
        assert_rows(fetch_rows(g), model.run(src[:, L:2 * L + 1024]), f"{front} behind the reset")


# ------------------------------------------------------------------------ 5. rows ----

def test_rows_follow_the_sources(oracle_lib):
    nsrc, per, L = 3, 2, 2048
    cfg = front_cfg("boxcar", L)
    steps = make_steps_special(nsrc * per, 23)
    src = source_bytes("boxcar", nsrc, 4 * L, 23)
    buf = src[0, :L]
    with open_handle("boxcar", cfg, nsrc, per, steps) as g:
        lib, h = g.lib, g._h
        p, cap = C.c_void_p(), C.c_uint32()
        for bad in (nsrc, nsrc * per - 1, -1):
            assert lib.rtlfm_gpu_push(h, bad, buf.ctypes.data, L) == -errno.EINVAL
            assert lib.rtlfm_gpu_acquire(h, bad, C.byref(p), C.byref(cap)) == -errno.EINVAL
            assert lib.rtlfm_gpu_commit(h, bad, L) == -errno.EINVAL
        for v in (2, -1):
            assert lib.rtlfm_gpu_set_option(h, b"source_ring", v) == -errno.EINVAL
        # a buffer queued: neither the row count nor the option may change, and the buffer still runs
        model = Model("boxcar", cfg, nsrc, per, steps)
        g.rtlsdr_callback(src[0, :L], stream=0)
        st6 = (C.c_uint32 * (nsrc * per))(*steps)
        assert lib.rtlfm_gpu_set_channels(h, 3, st6) == -errno.EBUSY
        assert lib.rtlfm_gpu_set_channels(h, 0, None) == -errno.EBUSY
        assert lib.rtlfm_gpu_set_option(h, b"source_ring", 0) == -errno.EBUSY
        assert g.get_option("source_ring") == 1 and g.sources == nsrc
        for i in (1, 2):
            g.rtlsdr_callback(src[i, :L], stream=i)
        g.full_demod()
        assert_rows(fetch_rows(g), model.run(src[:, :L]), "the queued buffer behind the refusals")
        # an open slot, a begun run: the option stays
        assert lib.rtlfm_gpu_acquire(h, 0, C.byref(p), C.byref(cap)) == 0
        assert lib.rtlfm_gpu_set_option(h, b"source_ring", 0) == -errno.EBUSY
        assert lib.rtlfm_gpu_commit(h, 0, 0) == 0  # (the slot given back)
        push_run(g, src, [(L, L)])
        assert g.run_begin() == 1
        assert lib.rtlfm_gpu_set_option(h, b"source_ring", 0) == -errno.EBUSY
        assert lib.rtlfm_gpu_set_channels(h, 3, st6) == -errno.EBUSY
        g.run_end()
        assert_rows(fetch_rows(g), model.run(src[:, L:2 * L]), "the begun run")
        # per_source 2 -> 3 on the idle ring: two sources now, the earlier run stays fetchable, the next run is the model's
        # (set_channels puts pos back to 0 and leaves the streams' records as they are: the model carries them on)
        kept = fetch_rows(g)
        g.set_channels(3, steps=steps)
        assert g.sources == 2 and g.channels_tell() == 0
        assert_rows(fetch_rows(g), kept, "the results of the run before set_channels")
        assert lib.rtlfm_gpu_push(h, 2, buf.ctypes.data, L) == -errno.EINVAL
        model = Model("boxcar", cfg, 2, 3, steps)
        model.states = g.state_get_all()
        for r in range(2):
            push_run(g, src[:2], [((2 + r) * L, L)])
            g.full_demod()
            assert_rows(fetch_rows(g), model.run(src[:2, (2 + r) * L:(3 + r) * L]), f"run {r} with 2 sources x 3 channels")
        # the option off and on again on the idle ring: per-stream rows are refused rows again, then the sources' are back
        g.set_option("source_ring", 0)
        assert g.sources == nsrc * per and lib.rtlfm_gpu_push(h, 0, buf.ctypes.data, L) == -errno.ENOTSUP
        g.set_option("source_ring", 1)
        pos, carried = g.channels_tell(), g.state_get_all()
        assert pos == 2 * L // 2
        push_run(g, src[:2], [(0, L)])
        g.full_demod()
        got = fetch_rows(g)
    want, wn, _ = cm.model_via_oracle(cfg, src[:2, :L], steps, 3, pos, carried)
    assert_rows(got, [want[s, :wn[s]] for s in range(6)], "behind source_ring 0 -> 1")


# ------------------------------------------------------------------ 6. off is off ----

def test_source_ring_with_channels_off_changes_nothing(oracle_lib):
    ov, sig = case("c1_boxcar10_fast")
    S, L = 3, 2048
    cfg = make_cfg(ov, L, CAP)
    iq = synth.random_u8(S, sum(RUNS) * L, seed=61)
    rows = {}
    for opt in (0, 1):
        with demod(cfg, S, source_ring=opt) as g:
            assert g.sources == S
            per_run, b0 = [], 0
            for nb in RUNS:
                for s in range(S):
                    for j in range(nb):
                        g.rtlsdr_callback(iq[s, (b0 + j) * L:(b0 + j + 1) * L], stream=s)
                g.full_demod()
                per_run.append(fetch_rows(g))
                b0 += nb
            rows[opt] = (joined(per_run), bytes(g.state_get_all()), g.last_path)
    assert_rows(rows[1][0], rows[0][0], "source_ring 1 / 0, channels off")
    assert rows[1][1:] == rows[0][1:]
    want, wn, _ = oracle_lib.run_batch(cfg, iq)
    assert_rows(rows[1][0], [want[s, :wn[s]] for s in range(S)], "source_ring 1, channels off, the oracle")


def test_without_the_option_the_ring_stays_refused(oracle_lib):
    """tests/test_channels_gpu.py::test_refusals_change_nothing's statement, once more: source_ring 0 is today's handle."""
    nsrc, per, L = 1, 2, 2048
    cfg = front_cfg("boxcar", L, 1)
    buf = np.full(L, 127, dtype=np.uint8)
    with open_handle("boxcar", cfg, nsrc, per, [1, 2], source_ring=0) as g:
        lib, h = g.lib, g._h
        p, cap, taken = C.c_void_p(), C.c_uint32(), C.c_int()
        assert g.get_option("source_ring") == 0
        assert lib.rtlfm_gpu_push(h, 0, buf.ctypes.data, L) == -errno.ENOTSUP
        assert lib.rtlfm_gpu_acquire(h, 0, C.byref(p), C.byref(cap)) == -errno.ENOTSUP
        assert lib.rtlfm_gpu_commit(h, 0, L) == -errno.ENOTSUP
        assert lib.rtlfm_gpu_run(h) == -errno.ENOTSUP
        assert lib.rtlfm_gpu_run_begin(h, C.byref(taken)) == -errno.ENOTSUP


def test_what_stays_refused_with_the_option(oracle_lib, tmp_path):
    nsrc, per, L = 1, 2, 2048
    cfg = make_cfg(dict(case("c1_boxcar10_fast")[0], squelch_level=1), L, 1)
    steps = [12345678, (1 << 32) - 987654321]
    src = bounded(nsrc, 6 * L, 31, BOUND)
    model = Model("boxcar", cfg, nsrc, per, steps)
    with open_handle("boxcar", cfg, nsrc, per, steps) as g:
        lib, h = g.lib, g._h
        refused = [
            ("input_stats", lambda: lib.rtlfm_gpu_set_option(h, b"input_stats", 1)),
            ("input_health", lambda: lib.rtlfm_gpu_set_option(h, b"input_health", 1)),
            ("squelch_gate", lambda: lib.rtlfm_gpu_set_option(h, b"squelch_gate", 1)),
            ("mute", lambda: lib.rtlfm_gpu_mute(h, 0, 4096)),
            ("save", lambda: lib.rtlfm_gpu_save(h, str(tmp_path / "no.snap").encode())),
        ]
        for b, (what, call) in enumerate(refused):
            assert call() == -errno.ENOTSUP, what
            push_run(g, src, [(b * L, L)])
            g.full_demod()
            assert_rows(fetch_rows(g), model.run(src[:, b * L:(b + 1) * L]), f"the run behind {what}")
        assert not (tmp_path / "no.snap").exists()
        for name in ("input_stats", "input_health", "squelch_gate"):
            assert g.get_option(name) == 0
    # set_channels itself, on a handle with one of them on, with the option set
    for opts in (dict(input_stats=1), dict(input_health=1)):
        with demod(front_cfg("boxcar", L, 1), 2, source_ring=1, **opts) as g:
            assert g.lib.rtlfm_gpu_set_channels(g._h, 2, (C.c_uint32 * 2)(1, 2)) == -errno.ENOTSUP
            assert g.sources == 2


# ------------------------------------------------------- 7. producers beside runs ----

def test_producers_push_beside_runs(oracle_lib):
    """Three sources pushed from three threads, each its own, while the main thread starts runs and collects them one
    run late (fetch_all_prev): a producer pushes the buffers of run k + 1 while run k's transfer and kernels are in
    flight and run k - 1 is fetched.  Six runs; every channel's PCM equals the model."""
    nsrc, per, L, depth, runs = 3, 4, 2048, 2, 6
    cfg = front_cfg("boxcar", L, depth)
    steps = make_steps_special(nsrc * per, 90)
    src = source_bytes("boxcar", nsrc, runs * depth * L, 91)
    want, wn, want_st = cm.model_via_oracle(cfg, src, steps, per, 0)
    filled = threading.Barrier(nsrc + 1)   # the producers have pushed run k
    flipped = threading.Barrier(nsrc + 1)  # ... and the main thread has started it: the ring's other half is theirs
    errors = []

    def producer(g, i):
        try:
            for k in range(runs):
                for b in range(k * depth, (k + 1) * depth):
                    g.rtlsdr_callback(src[i, b * L:(b + 1) * L], stream=i)
                filled.wait(60)
                flipped.wait(60)
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)
            filled.abort()
            flipped.abort()

    got = [[] for _ in range(nsrc * per)]

    def collect(rows_lens):
        o, n = rows_lens
        for s in range(nsrc * per):
            got[s].append(o[s, :n[s]].copy())

    with open_handle("boxcar", cfg, nsrc, per, steps) as g:
        th = [threading.Thread(target=producer, args=(g, i)) for i in range(nsrc)]
        for t in th:
            t.start()
        try:
            for k in range(runs):
                filled.wait(60)
                g.full_demod()
                flipped.wait(60)
                if k:
                    collect(g.fetch_all_prev())
        except BaseException:
            filled.abort()  # (the producers must not wait for a main thread that has given up)
            flipped.abort()
            raise
        finally:
            for t in th:
                t.join(60)
        assert not errors, errors
        collect(g.fetch_all())
        st = g.state_get_all()
        assert g.channels_tell() == runs * depth * L // 2
    assert_rows([np.concatenate(r) for r in got], [want[s, :wn[s]] for s in range(nsrc * per)], "producers beside runs")
    for s in range(nsrc * per):
        assert st[s].as_dict() == want_st[s].as_dict(), s
