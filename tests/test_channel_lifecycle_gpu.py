"""The channel lifecycle (include/rtlfm_hip.h, "The channel lifecycle"; include/rtlfm_chansnap.h): what a handle with channels
on carries beyond the records - pos, the source history, its bias pieces - saved, loaded, read, written and regrouped by
source.  Integer modes only (-M fm -A fast), every bit equal to the multi-run models of tests/channel_model.py,
channel_fir_model.py, channel_bank_model.py and source_dc_model.py, none of which knows the code under test.

The common shape: 3 sources, buffers of 2048 bytes = 1024 samples, boxcar / 10 (102.4 outputs per buffer: prev_index is not
zero at any cut), runs of 1, 3 and 5 buffers - the first shorter than the history of 4096 samples, so that what is carried
holds silence and samples together, the last longer."""
import ctypes as C
import errno
import functools
import os

import numpy as np
import pytest

import channel_bank_model as bm
import channel_fir_model as fm
import channel_model as cm
import source_dc_model as sdm
from cases import case, make_cfg
from channel_common import assert_rows, make_steps, run_once, to_device
from rtlsdr_amd import capi
from rtlsdr_amd.capi import RESAMPLE_LOW_PASS_REAL, RtlfmStreamState

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NSRC, L, D = 3, 2048, 10
RUNS = (1, 3, 5)
NB = sum(RUNS)
HIST = 4096
BASE = case("c1_boxcar10_fast")[0]
TAIL = dict(BASE, deemph=1, deemph_a=19, rate_out2=48000, resampler=RESAMPLE_LOW_PASS_REAL)


def cfg_of(ov=BASE):
    cfg = make_cfg(ov, L, max(RUNS))
    assert cfg.downsample == D
    return cfg


@functools.lru_cache(maxsize=None)
def fronts():
    from rtlsdr_amd.demod import channel_lowpass
    ft, fs = channel_lowpass(33, 0.04, 1)
    t4, s4 = channel_lowpass(16, 0.4 / 4, 1)
    t16, s16 = channel_lowpass(40, 0.4 / 16, 1)
    return {
        "boxcar": dict(per=2, fir=None, K=0),
        "fir33": dict(per=2, fir=(ft, fs), K=0),
        "bank4": dict(per=4, fir=None, K=4, bins=None, bank=(t4, s4 - 2)),
        "bank16": dict(per=5, fir=None, K=16, bins=[3, 0, 9, 3, 15], bank=(t16, s16 - 4)),  # 5 selected bins, one twice
    }


FRONTS = ["boxcar", "fir33", "bank4", "bank16"]


def source_bytes(nsrc=NSRC, nb=NB, seed=1):
    """Bytes whose mixed and filtered samples stay inside a byte (the models assert it), each source with its own offset,
    which option source_dc then has something to take off."""
    rng = np.random.default_rng(seed)
    src = rng.integers(-40, 41, size=(nsrc, nb * L)) + 127
    src += np.array([-30, 14, 41, 5])[:nsrc, None]
    return src.astype(np.uint8)


def steps_of(front, nsrc=NSRC, seed=5):
    return np.array(make_steps(nsrc * fronts()[front]["per"], seed), dtype=np.uint32)


def open_handle(front, dc, path=0, nsrc=NSRC, steps=None, ov=BASE, **options):
    """A handle set up in the documented order: set_channels, the filter or the bank, source_dc."""
    from rtlsdr_amd.demod import GpuDemod
    fr = fronts()[front]
    g = GpuDemod(cfg_of(ov), nsrc * fr["per"], 0, options=options)
    g.set_path(path)
    g.set_channels(fr["per"], steps=steps_of(front, nsrc) if steps is None else steps)
    if fr["fir"]:
        g.set_channel_filter(*fr["fir"])
    if fr["K"]:
        g.set_channel_bank(fr["K"], fr["bank"][0], fr["bank"][1], bins=fr["bins"])
    if dc:
        g.set_option("source_dc", 1)
    return g


class Model:
    """One front end's model and the oracle's back half behind it, run by run: pcm() is every stream's PCM of all runs so
    far.  Behind the boxcar the oracle takes the mixed bytes buffer by buffer and carries its own states; behind a filter
    or a bank the oracle's fm_demod takes every buffer's filtered samples (buffers here hold 102 or 103 of them)."""

    def __init__(self, front, dc, steps, nsrc, pos=0, ov=BASE):
        fr = fronts()[front]
        self.fr, self.dc, self.steps, self.nsrc, self.per, self.cfg = fr, dc, [int(v) for v in steps], nsrc, fr["per"], cfg_of(ov)
        self.pos, self.states, self.out, self.iq = pos, None, [], []
        self.p0_before, self.samples = [], []
        self.m = None
        if fr["K"]:
            self.m = (sdm.DcBankModel if dc else bm.BankModel)(fr["K"], fr["bank"][0], fr["bank"][1], D, nsrc, bins=fr["bins"])
        elif fr["fir"]:
            self.m = (sdm.DcFirModel if dc else fm.FirModel)(self.steps, self.per, D, fr["fir"][0], fr["fir"][1], nsrc)
        elif dc:
            self.m = sdm.DcBoxModel(self.steps, self.per, D, nsrc)
        if self.m is not None:
            self.m.seek(pos)

    def run(self, src):
        from oracle import pyoracle as po
        if self.fr["K"] or self.fr["fir"]:
            self.p0_before.append(list(self.m.p0))
            self.samples.append(src.shape[1] // 2)
            self.iq.append(self.m.run(src, L) if self.dc else self.m.run(src))
        else:
            by = self.m.mixed_bytes(src, L) if self.dc else cm.mixed_bytes(src, self.steps, self.per, self.pos)
            out, n, self.states = po.run_batch(cm.copy_cfg(self.cfg, offset_tuning=1), by, self.states, nthreads=4)
            self.out.append([out[s, :n[s]].copy() for s in range(len(self.steps))])
        self.pos += src.shape[1] // 2

    def pcm(self):
        if not (self.fr["K"] or self.fr["fir"]):
            return [np.concatenate([r[s] for r in self.out]) for s in range(len(self.out[0]))]
        # fm_demod() buffer by buffer, as full_demod() calls it: a buffer's first output is always polar_discriminant's,
        # whatever -A says (src/rtl_fm.c:932-959), so the buffers' bounds show in the PCM.  Buffer j of a run that began at
        # prev_index p0 holds the outputs due in its N0 samples.
        from oracle import pyoracle as po
        lib = po.oracle()
        lib.orc_fm_demod.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        lib.orc_fm_demod.restype = C.c_int
        assert self.cfg.mode == capi.MODE_FM and not self.cfg.deemph and self.cfg.rate_out2 < 0 and not self.cfg.squelch_level
        N0, rows = L // 2, []
        for s in range(len(self.iq[0][0])):
            pre_r, pre_j, out = C.c_int32(0), C.c_int32(0), []
            for (I, Q), p0s, T in zip(self.iq, self.p0_before, self.samples, strict=True):
                k = 0
                for j in range(T // N0):
                    cnt = (p0s[s] + (j + 1) * N0) // D - (p0s[s] + j * N0) // D
                    lp = np.empty(2 * cnt, dtype=np.int16)
                    lp[0::2], lp[1::2] = I[s][k:k + cnt], Q[s][k:k + cnt]
                    res = np.zeros(cnt, dtype=np.int16)
                    assert lib.orc_fm_demod(lp.ctypes.data, lp.size, res.ctypes.data, int(self.cfg.custom_atan), C.byref(pre_r), C.byref(pre_j)) == cnt
                    out.append(res)
                    k += cnt
                assert k == I[s].size
            rows.append(np.concatenate(out))
        return rows

    def prev_index(self):
        return [int(self.states[s].prev_index) for s in range(len(self.steps))] if self.m is None or not hasattr(self.m, "p0") else list(self.m.p0)


def model_over(front, dc, steps, src, runs, pos=0, ov=BASE):
    m = Model(front, dc, steps, src.shape[0], pos, ov)
    b0 = 0
    for nb in runs:
        m.run(src[:, b0 * L:(b0 + nb) * L])
        b0 += nb
    return m


@functools.lru_cache(maxsize=None)
def whole(front, dc, tail=False):
    """The model over the whole input, and the input."""
    src = source_bytes()
    m = model_over(front, dc, steps_of(front), src, RUNS, ov=TAIL if tail else BASE)
    return src, m.pcm(), m


def cat(per_run):
    return [np.concatenate([r[s] for r in per_run]) for s in range(len(per_run[0]))]


def state_bytes(g):
    return bytes(g.state_get_all())


def assert_state_fields(g, model, what):
    """What the models know of the records: prev_index of every stream - and behind the boxcar without source_dc, where the
    oracle carries whole records, every field."""
    st = g.state_get_all()
    assert [int(s.prev_index) for s in st] == model.prev_index(), what
    if model.m is None:
        for s in range(len(st)):
            assert st[s].as_dict() == model.states[s].as_dict(), (what, s)


# ------------------------------------------------------------------ 1. resume equals uninterrupted ----

def resumed(tmp_path, front, dc, paths, ov=BASE, via=None):
    """Every run on a handle of its own: set up, load what the one before saved, run, save.  Returns (per run rows, per
    run last_path, (state bytes, pos) at the end).  via: another way from handle to handle."""
    d = to_device(source_bytes())
    snap = str(tmp_path / "keep.chn")
    per_run, seen, b0 = [], [], 0
    carry = None
    for r, nb in enumerate(RUNS):
        with open_handle(front, dc, paths[r], ov=ov) as g:
            if r:
                if via is None:
                    g.channels_load(snap)
                else:
                    via(g, carry)
            rows, p = run_once(g, d, L, b0, nb)
            per_run.append(rows)
            seen.append(p)
            b0 += nb
            if via is None:
                g.channels_save(snap)
                assert sorted(os.listdir(tmp_path)) == ["keep.chn"]
            else:
                fr = fronts()[front]
                carry = (g.channels_tell(), g.state_get_all(), g.channels_history() if fr["fir"] or fr["K"] else None)
            last = (state_bytes(g), g.channels_tell())
    return per_run, seen, last


def uninterrupted(front, dc, paths, ov=BASE):
    d = to_device(source_bytes())
    per_run, b0 = [], 0
    with open_handle(front, dc, ov=ov) as g:
        for r, nb in enumerate(RUNS):
            g.set_path(paths[r])
            per_run.append(run_once(g, d, L, b0, nb)[0])
            b0 += nb
        return per_run, (state_bytes(g), g.channels_tell()), g


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("dc", [0, 1])
@pytest.mark.parametrize("front", FRONTS)
def test_resume_equals_uninterrupted(oracle_lib, tmp_path, front, dc, path):
    _, want, model = whole(front, dc)
    paths = (path,) * len(RUNS)
    never, never_end, _ = uninterrupted(front, dc, paths)
    got, seen, end = resumed(tmp_path, front, dc, paths)
    assert seen == [2 if path == 0 else 1] * len(RUNS)
    for r in range(len(RUNS)):
        assert_rows(got[r], never[r], f"{front} dc {dc} path {path} run {r} against the handle that never stopped")
    assert_rows(cat(got), want, f"{front} dc {dc} path {path} against the model")
    assert end == never_end and end[1] == model.pos == NB * L // 2
    with open_handle(front, dc, path) as g:  # ... and the records the last file holds are the model's
        g.channels_load(str(tmp_path / "keep.chn"))
        assert_state_fields(g, model, f"{front} dc {dc}")
        assert g.channels_tell() == model.pos


@pytest.mark.parametrize("paths", [(1, 0, 1), (0, 1, 0)], ids=["1-2-1", "2-1-2"])
@pytest.mark.parametrize("front,dc", [("boxcar", 1), ("fir33", 0), ("bank16", 1)])
def test_saved_on_one_path_loaded_on_the_other(oracle_lib, tmp_path, front, dc, paths):
    _, want, _ = whole(front, dc)
    got, seen, end = resumed(tmp_path, front, dc, paths)
    assert seen == [2 if p == 0 else 1 for p in paths]
    assert_rows(cat(got), want, f"{front} dc {dc} paths {paths}")
    assert end[1] == NB * L // 2


@pytest.mark.parametrize("path", [0, 1])
def test_resume_with_an_audio_tail(oracle_lib, tmp_path, path):
    """deemph + low_pass_real behind the boxcar: the tail's fields of the record (deemph_avg, now_lpr, prev_lpr_index)
    travel through the file."""
    _, want, model = whole("boxcar", 0, tail=True)
    paths = (path,) * len(RUNS)
    never, never_end, _ = uninterrupted("boxcar", 0, paths, ov=TAIL)
    got, _, end = resumed(tmp_path, "boxcar", 0, paths, ov=TAIL)
    for r in range(len(RUNS)):
        assert_rows(got[r], never[r], f"tail path {path} run {r}")
    assert_rows(cat(got), want, f"tail path {path} against the model")
    assert end == never_end
    last = RtlfmStreamState.from_buffer_copy(end[0][:C.sizeof(RtlfmStreamState)])
    assert last.as_dict() == model.states[0].as_dict()


# ------------------------------------------------------------------------- 2. the history accessors ----

@pytest.mark.parametrize("front,dc", [("fir33", 0), ("fir33", 1), ("bank4", 1), ("bank16", 0)])
def test_history_accessors(oracle_lib, front, dc):
    src = source_bytes()
    d = to_device(src)
    dcm = Model(front, 1, steps_of(front), NSRC) if dc else None
    with open_handle(front, dc) as g:
        hist, words = g.channels_history()
        assert (hist == 127).all() and hist.shape == (NSRC, 2 * HIST) and ((words is None) if not dc else (words == capi.CHANSNAP_DC_NONE).all())
        run_once(g, d, L, 0, 1)
        hist, words = g.channels_history()
        assert (hist[:, :2 * (HIST - L // 2)] == 127).all()          # 3072 leading pairs of silence
        assert np.array_equal(hist[:, 2 * (HIST - L // 2):], src[:, :L])  # ... and the run's 1024
        if dc:
            dcm.run(src[:, :L])
            want = np.full((NSRC, 16), capi.CHANSNAP_DC_NONE, dtype=np.uint32)
            for a in range(NSRC):
                ai, aq = dcm.m.last_avgs[a][0]
                want[a, 12:] = ((127 + ai) & 0xFFFF) | (((127 + aq) & 0xFFFF) << 16)  # one buffer = 4 pieces of 256 samples
            assert np.array_equal(words, want) and (want[:, 12:] != capi.CHANSNAP_DC_NONE).any()
        run_once(g, d, L, 1, 3)
        run_once(g, d, L, 4, 5)
        hist, words = g.channels_history()
        assert np.array_equal(hist, src[:, NB * L - 2 * HIST:])       # the input's last 8192 bytes per source
        if dc:
            dcm.run(src[:, L:4 * L])
            dcm.run(src[:, 4 * L:])
            want = np.array([[((127 + ai) & 0xFFFF) | (((127 + aq) & 0xFFFF) << 16) for ai, aq in dcm.m.last_avgs[a][1:] for _ in range(4)]
                             for a in range(NSRC)], dtype=np.uint32)
            assert np.array_equal(words, want)
        # set, then get: what was set
        rng = np.random.default_rng(77)
        h2 = rng.integers(0, 256, size=hist.shape, dtype=np.uint8)
        w2 = rng.integers(0, 1 << 32, size=(NSRC, 16), dtype=np.uint64).astype(np.uint32) if dc else None
        g.set_channels_history(h2, w2)
        h3, w3 = g.channels_history()
        assert np.array_equal(h3, h2) and (w3 is None if not dc else np.array_equal(w3, w2))
        if dc:  # no biases given: none subtracted
            g.set_channels_history(h2)
            assert (g.channels_history()[1] == capi.CHANSNAP_DC_NONE).all()
        # the caps: one byte or one word short, and the count is written anyway
        n = C.c_int(-1)
        out = np.zeros(hist.size, np.uint8)
        wd = np.zeros(NSRC * 16, np.uint32)
        assert g.lib.rtlfm_gpu_channels_history_get(g._h, out.ctypes.data, out.size - 1, wd.ctypes.data, wd.size, C.byref(n)) == -errno.ENOBUFS
        assert n.value == NSRC
        if dc:
            assert g.lib.rtlfm_gpu_channels_history_get(g._h, out.ctypes.data, out.size, wd.ctypes.data, wd.size - 1, C.byref(n)) == -errno.ENOBUFS
        assert g.lib.rtlfm_gpu_channels_history_set(g._h, out.ctypes.data, None, NSRC - 1) == -errno.EINVAL


@pytest.mark.parametrize("front,dc", [("boxcar", 0), ("fir33", 1), ("bank4", 0)])
def test_seek_history_set_state_set_resumes_like_a_load(oracle_lib, tmp_path, front, dc):
    """The route between devices: tell + state_get_all + channels_history on one handle, seek (which clears the history)
    THEN set_channels_history and state_set_all on the next."""
    def via(g, carry):
        pos, states, hist = carry
        g.channels_seek(pos)
        if hist is not None:
            g.set_channels_history(*hist)
        g.state_set_all(states)
    _, want, model = whole(front, dc)
    got, _, end = resumed(tmp_path, front, dc, (0, 1, 0), via=via)
    assert_rows(cat(got), want, f"{front} dc {dc}")
    assert end[1] == model.pos


def test_history_of_a_boxcar_handle_is_no_data(oracle_lib):
    with open_handle("boxcar", 0) as g:
        n = C.c_int(-1)
        out = np.zeros(NSRC * 2 * HIST, np.uint8)
        assert g.lib.rtlfm_gpu_channels_history_get(g._h, out.ctypes.data, out.size, None, 0, C.byref(n)) == -errno.ENODATA
        assert n.value == NSRC
        g.set_channels(0)
        assert g.lib.rtlfm_gpu_channels_history_get(g._h, out.ctypes.data, out.size, None, 0, C.byref(n)) == -errno.ENOTSUP
        assert g.lib.rtlfm_gpu_channels_history_set(g._h, out.ctypes.data, None, NSRC) == -errno.ENOTSUP


# ------------------------------------------------------------------------------------- 3. the move ----
# The steps do not move (the caller sets them), so the handles of these tests give every source the same per-channel steps:
# a source's records then mean the same at every position.

def same_steps(front, nsrc=NSRC):
    return np.tile(np.array(make_steps(fronts()[front]["per"], 6), dtype=np.uint32), nsrc)


def mapped_want(front, dc, smap, src, feed):
    """What run 2 (3 buffers) gives behind run 1 (1 buffer) and a move by `smap`: per dst source the model of source
    smap[a] over both runs with `feed[a]` as run 2's bytes - or, for -1, a model that starts from silence at run 2's pos.
    Returns (rows of run 2 per dst stream, prev_index per dst stream, pos)."""
    per = fronts()[front]["per"]
    rows, p0 = [], []
    for a, m in enumerate(smap):
        if m < 0:
            md = Model(front, dc, same_steps(front, 1), 1, pos=L // 2)
            md.run(feed[a][None, :])
            rows += md.pcm()
        else:
            md = Model(front, dc, same_steps(front, 1), 1)
            md.run(src[m][None, :L])
            k = [r.size for r in md.pcm()]
            md.run(feed[a][None, :])
            rows += [r[n:] for r, n in zip(md.pcm(), k, strict=True)]
        p0 += md.prev_index()
        assert md.pos == 2 * L and len(rows) == (a + 1) * per
    return rows, p0, 2 * L


def assert_after_move(g, got, want, what):
    rows, p0, pos = want
    assert_rows(got, rows, what)
    assert g.channels_tell() == pos, what
    assert [int(s.prev_index) for s in g.state_get_all()] == p0, what


@pytest.mark.parametrize("front,dc", [("fir33", 1), ("bank4", 0), ("boxcar", 0)])
def test_move_to_a_handle_of_fewer_sources(oracle_lib, front, dc):
    """Run 1 on A (sources 0, 1, 2), B takes sources (2, 0), run 2 on B with their continuing bytes: the model of those two
    over both runs.  Behind the boxcar the records and pos move and there is no history to move.  A is left as it was."""
    src = source_bytes()
    sel = [2, 0]
    with open_handle(front, dc, steps=same_steps(front)) as A, open_handle(front, dc, nsrc=2, steps=same_steps(front, 2)) as B:
        run_once(A, to_device(src), L, 0, 1)
        before = state_bytes(A), A.channels_tell()
        B.channels_move_from(A, sel)
        assert (state_bytes(A), A.channels_tell()) == before and B.channels_tell() == L // 2
        got, _ = run_once(B, to_device(src[sel]), L, 1, 3)
        assert_after_move(B, got, mapped_want(front, dc, sel, src, src[sel][:, L:4 * L]), f"{front} dc {dc}")
        gotA, _ = run_once(A, to_device(src), L, 1, 3)
        assert_after_move(A, gotA, mapped_want(front, dc, [0, 1, 2], src, src[:, L:4 * L]), f"{front} dc {dc}: the move's source goes on")


@pytest.mark.parametrize("front,dc,smap", [("fir33", 0, [2, 0, 1]), ("bank4", 1, [2, 0, 1]), ("fir33", 1, [1, 1, 0]), ("bank4", 0, [1, 1, 0]),
                                           ("fir33", 1, [-1, 0, 1]), ("bank4", 1, [-1, 0, 1]), ("boxcar", 1, [-1, 2, 2])])
def test_move_in_place(oracle_lib, front, dc, smap):
    """A permutation, a fan-out and a source that joins from silence, on the handle itself: run 2 equals the models of the
    mapped sources; the joining source equals a model that starts from silence at the handle's pos."""
    src = source_bytes()
    per = fronts()[front]["per"]
    feed = np.stack([src[m if m >= 0 else 2, L:4 * L] for m in smap])
    if smap[0] == smap[1]:
        feed[1] = feed[0]  # the fan-out's two copies hear the same bytes: two equal sets of rows
    with open_handle(front, dc, steps=same_steps(front)) as A:
        run_once(A, to_device(src), L, 0, 1)
        A.channels_move_from(A, smap)
        assert A.channels_tell() == L // 2
        got, _ = run_once(A, to_device(np.concatenate((src[:, :L], feed), axis=1)), L, 1, 3)
        assert_after_move(A, got, mapped_want(front, dc, smap, src, feed), f"{front} dc {dc} map {smap}")
        if smap[0] == smap[1]:
            assert_rows(got[:per], got[per:2 * per], "the fan-out's two copies")


# ------------------------------------------------------------------------------------- 4. the ring ----

def ring_run(g, src, b0, nb):
    for b in range(b0, b0 + nb):
        for a in range(src.shape[0]):
            g.push(src[a, b * L:(b + 1) * L], a)
    g.run()
    o, n = g.fetch_all()
    return [o[s, :n[s]].copy() for s in range(g.nstreams)]


@pytest.mark.parametrize("dc", [0, 1])
def test_ring_saved_between_two_runs(oracle_lib, tmp_path, dc):
    src, want, model = whole("fir33", dc)
    snap = str(tmp_path / "ring.chn")
    with open_handle("fir33", dc, source_ring=1) as g:
        got = [ring_run(g, src, 0, 1), ring_run(g, src, 1, 3)]
        g.channels_save(snap)
    with open_handle("fir33", dc, source_ring=1) as g:
        g.channels_load(snap)
        got.append(ring_run(g, src, 4, 5))
        assert g.channels_tell() == model.pos
        assert_state_fields(g, model, "ring")
    assert_rows(cat(got), want, f"ring dc {dc}")


# ------------------------------------------------------------------------ 5. refusals change nothing ----

def test_refusals_change_nothing(oracle_lib, tmp_path):
    """Every refusal, then the whole of runs 2 and 3 on the handle that refused: still the model's bits."""
    src, want, model = whole("fir33", 1)
    d = to_device(src)
    n1 = [r.size for r in model_over("fir33", 1, steps_of("fir33"), src, (1,)).pcm()]
    good, other = str(tmp_path / "good.chn"), str(tmp_path / "other.chn")
    snp = str(tmp_path / "streams.snap")
    E = errno
    ft, fs = fronts()["fir33"]["fir"]
    with open_handle("fir33", 1) as g:
        run_once(g, d, L, 0, 1)
        g.channels_save(good)
        lib, h = g.lib, g._h
        kept = state_bytes(g), g.channels_tell(), g.channels_history()[0].tobytes(), g.channels_history()[1].tobytes()

        def unchanged(what):
            now = state_bytes(g), g.channels_tell(), g.channels_history()[0].tobytes(), g.channels_history()[1].tobytes()
            assert now == kept, what

        smap = (C.c_int32 * 3)(0, 1, 2)
        # channels off on either side of a move; the old calls' files and handles
        with open_handle("fir33", 1) as off:
            off.set_channels(0)
            assert lib.rtlfm_gpu_channels_move(h, off._h, smap, 3) == -E.ENOTSUP
            assert lib.rtlfm_gpu_channels_move(off._h, h, smap, 3) == -E.ENOTSUP
            assert lib.rtlfm_gpu_channels_load(off._h, os.fsencode(good)) == -E.ENOTSUP
            assert lib.rtlfm_gpu_channels_save(off._h, os.fsencode(other)) == -E.ENOTSUP and not os.path.exists(other)
            assert lib.rtlfm_gpu_load(off._h, os.fsencode(good)) == -E.EILSEQ        # an RTLFMCHN file to the old reader
            assert lib.rtlfm_gpu_save(off._h, os.fsencode(snp)) == 0
        unchanged("channels off")
        assert lib.rtlfm_gpu_channels_load(h, os.fsencode(snp)) == -E.EILSEQ           # an RTLFMSNP file to the new one
        assert lib.rtlfm_gpu_channels_load(h, os.fsencode(tmp_path / "nothing.chn")) == -E.ENOENT
        assert lib.rtlfm_gpu_save(h, os.fsencode(other)) == -E.ENOTSUP and not os.path.exists(other)  # (the old refusal stays)
        unchanged("the other kind's file")
        # the two sides do not carry the same things: taps, shift, filter against bank, K, per_source, source_dc, the cfg
        t2 = ft.copy()
        t2[5] += 1
        fr4 = fronts()["bank4"]
        variants = [
            ("taps", lambda o: o.set_channel_filter(t2, fs)),
            ("shift", lambda o: o.set_channel_filter(ft, fs + 1)),
            ("ntaps", lambda o: o.set_channel_filter(ft[:31], fs)),
            ("no filter", lambda o: o.set_channel_filter(None)),
            ("source_dc", lambda o: o.set_option("source_dc", 0)),
            ("per_source", lambda o: (o.set_channels(3, steps=steps_of("fir33")), o.set_channel_filter(ft, fs), o.set_option("source_dc", 1))),
            ("a bank as well", lambda o: o.set_channel_bank(4, fr4["bank"][0], fr4["bank"][1], bins=[0, 1])),
        ]
        for name, change in variants:
            with open_handle("fir33", 1) as o:
                change(o)
                pmap = (C.c_int32 * 3)(0, 1, 0) if name != "per_source" else (C.c_int32 * 2)(0, 1)
                assert lib.rtlfm_gpu_channels_move(o._h, h, pmap, len(pmap)) == -E.EMEDIUMTYPE, name
                assert lib.rtlfm_gpu_channels_move(h, o._h, (C.c_int32 * 3)(0, 1, 0), 3) == -E.EMEDIUMTYPE, name
                assert lib.rtlfm_gpu_channels_load(o._h, os.fsencode(good)) == -E.EMEDIUMTYPE, name
                o.channels_save(other)
                assert lib.rtlfm_gpu_channels_load(h, os.fsencode(other)) == -E.EMEDIUMTYPE, name
                os.remove(other)
            unchanged(name)
        with open_handle("bank4", 0) as b4, open_handle("bank4", 0) as b8:
            b8.set_channel_bank(8, fr4["bank"][0], fr4["bank"][1], bins=[0, 1, 2, 3])
            assert lib.rtlfm_gpu_channels_move(b4._h, b8._h, smap, 3) == -E.EMEDIUMTYPE  # two banks that differ in K alone
            b8.channels_save(other)
            assert lib.rtlfm_gpu_channels_load(b4._h, os.fsencode(other)) == -E.EMEDIUMTYPE
            os.remove(other)
        with open_handle("fir33", 1, ov=dict(BASE, squelch_level=3)) as o:
            assert lib.rtlfm_gpu_channels_move(h, o._h, smap, 3) == -E.EMEDIUMTYPE
            assert lib.rtlfm_gpu_channels_load(o._h, os.fsencode(good)) == -E.EMEDIUMTYPE
        # another stream count
        with open_handle("fir33", 1, nsrc=2) as o:
            assert lib.rtlfm_gpu_channels_load(o._h, os.fsencode(good)) == -E.ERANGE
            assert lib.rtlfm_gpu_channels_move(h, o._h, (C.c_int32 * 3)(0, 1, 2), 3) == -E.EINVAL   # 2 is no source of o
        # a bad map, a bad count, NULL
        for bad, n in (((C.c_int32 * 3)(0, 1, 3), 3), ((C.c_int32 * 3)(0, -2, 1), 3), (smap, 2), (smap, 4), (None, 3)):
            assert lib.rtlfm_gpu_channels_move(h, h, bad, n) == -E.EINVAL
        assert lib.rtlfm_gpu_channels_move(None, h, smap, 3) == -E.EINVAL and lib.rtlfm_gpu_channels_save(h, None) == -E.EINVAL
        # a damaged file
        raw = bytearray(open(good, "rb").read())
        raw[len(raw) // 2] ^= 1
        open(other, "wb").write(bytes(raw))
        assert lib.rtlfm_gpu_channels_load(h, os.fsencode(other)) == -E.EILSEQ
        os.remove(other)
        # a save that cannot be written leaves no file
        assert lib.rtlfm_gpu_channels_save(h, os.fsencode(tmp_path / "no_such_dir" / "x.chn")) == -E.ENOENT
        assert sorted(os.listdir(tmp_path)) == ["good.chn", "streams.snap"]
        unchanged("maps, counts and files")
        got = [run_once(g, d, L, 1, 3)[0], run_once(g, d, L, 4, 5)[0]]
        assert g.channels_tell() == model.pos
    assert_rows(cat(got), [w[k:] for w, k in zip(want, n1, strict=True)], "behind every refusal")


def test_busy_handles_refuse(oracle_lib, tmp_path):
    """A run begun, a ring slot open, buffers queued: -EBUSY, and the run that follows is the model's."""
    src, want, model = whole("fir33", 0)
    E = errno
    good = str(tmp_path / "good.chn")
    smap = (C.c_int32 * 3)(0, 1, 2)
    with open_handle("fir33", 0, source_ring=1) as g, open_handle("fir33", 0) as idle:
        lib, h = g.lib, g._h
        g.channels_save(good)
        hist = np.full((NSRC, 2 * HIST), 127, np.uint8)

        def all_busy(what, save_too):
            assert lib.rtlfm_gpu_channels_load(h, os.fsencode(good)) == -E.EBUSY, what
            assert lib.rtlfm_gpu_channels_history_set(h, hist.ctypes.data, None, NSRC) == -E.EBUSY, what
            for dst, s in ((h, h), (h, idle._h), (idle._h, h)):
                assert lib.rtlfm_gpu_channels_move(dst, s, smap, 3) == -E.EBUSY, what
            if save_too:
                assert lib.rtlfm_gpu_channels_save(h, os.fsencode(tmp_path / "busy.chn")) == -E.EBUSY, what
                assert not os.path.exists(tmp_path / "busy.chn")

        g.push(src[0, :L], 0)
        all_busy("buffers queued", True)
        buf, cap = C.c_void_p(), C.c_uint32()
        assert lib.rtlfm_gpu_acquire(h, 1, C.byref(buf), C.byref(cap)) == 0
        all_busy("a ring slot open", True)
        C.memmove(buf, src[1, :L].ctypes.data, L)
        assert lib.rtlfm_gpu_commit(h, 1, L) == 0
        g.push(src[2, :L], 2)
        assert g.run_begin() == 1
        all_busy("a run begun", True)
        g.run_end()
        o, n = g.fetch_all()
        got = [[o[s, :n[s]].copy() for s in range(g.nstreams)], ring_run(g, src, 1, 3), ring_run(g, src, 4, 5)]
        assert idle.channels_tell() == 0
    assert_rows(cat(got), want, "behind -EBUSY")
