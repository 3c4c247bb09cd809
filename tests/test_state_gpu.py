"""The stream lifecycle on the GPU: rtlfm_gpu_state_get_all / _set_all, rtlfm_gpu_state_move (k_state_move) and
rtlfm_gpu_save / _load against the oracle, EXACTLY: integer stages and -A fast (amplitude 30 behind four passes), so every
comparison is for equality.  Two configurations between them carry every field of the record:

  fifth4_fir_deemph_lpr   four fifth_order passes (lp_i/q_hist), generic_fir (droop_i/q_hist), fm_demod (pre_r, pre_j),
                          deemph_filter (deemph_avg), low_pass_real 170000 -> 32000 (now_lpr, prev_lpr_index)
  box7_rdc_adc_sq         a boxcar of 7, which does not divide the 1024-sample buffer (now_r, now_j, prev_index),
                          dc_block_raw (dc_avgI, dc_avgQ), dc_block_audio (dc_avg), the squelch (squelch_hits)

with block_len = 2048, 5 or 7 streams and runs of 1 and 3 buffers."""
import ctypes as C
import errno
import os
import time

import numpy as np
import pytest

import scan_model as sm
from rtlsdr_amd import capi, synth
from rtlsdr_amd.capi import ATAN_FAST, MODE_FM, RESAMPLE_LOW_PASS_REAL, RtlfmCfg, RtlfmStreamState

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

L, LEVEL = 2048, 60
REC = C.sizeof(RtlfmStreamState)
CONFIGS = {
    "fifth4_fir_deemph_lpr": dict(mode=MODE_FM, downsample=16, downsample_passes=4, comp_fir_size=9, custom_atan=ATAN_FAST,
                                  deemph=1, deemph_a=9, rate_out=170000, rate_out2=32000, resampler=RESAMPLE_LOW_PASS_REAL),
    "box7_rdc_adc_sq": dict(mode=MODE_FM, downsample=7, custom_atan=ATAN_FAST, dc_block_raw=1, dc_block_audio=1,
                            squelch_level=LEVEL),
}
NAMES = list(CONFIGS)


def make_cfg(name, nb, **ov):
    return RtlfmCfg.default(block_len=L, max_blocks=nb, **{**CONFIGS[name], **ov})


def demod(cfg, ns, **options):
    from rtlsdr_amd.demod import GpuDemod
    return GpuDemod(cfg, ns, 0, options=options)


def sources(name, ns, nbuf, seed):
    """rows[s][b] = buffer b of source s.  Behind four passes an FM signal of amplitude 30; for the squelch configuration
    tone and +-1 noise buffers in a seeded order, so that squelch_hits moves both ways."""
    if name.startswith("fifth4"):
        iq = synth.fm_iq_u8(ns, L // 2 * nbuf, fs=1.02e6, dev_hz=5e3, amplitude=30.0, seed=seed)
        return [[iq[s, b * L:(b + 1) * L].copy() for b in range(nbuf)] for s in range(ns)]
    rng = np.random.default_rng(seed)
    return [[sm.tone_or_noise(rng, L, bool(rng.random() < 0.6)) for _ in range(nbuf)] for _ in range(ns)]


def copy_state(st):
    return RtlfmStreamState.from_buffer_copy(bytes(st))


def oracle_on(po, cfg, bufs, state=None):
    """(pcm, state behind it) of one source's buffers, from `state` (not changed) or from demod_init()."""
    return po.run_stream(cfg, np.concatenate(bufs), copy_state(state) if state is not None else None)


def feed(g, rows):
    """One run: rows[k] = the buffers stream k of the handle gets.  Returns each stream's PCM."""
    for k, bufs in enumerate(rows):
        for b in bufs:
            g.push(b, k)
    g.run()
    out, lens = g.fetch_all()
    return [out[k, :lens[k]].copy() for k in range(len(rows))]


def table(states):
    """A ctypes array of records as uint8 [n, REC]."""
    return np.frombuffer(bytes(states), dtype=np.uint8).reshape(-1, REC)


def assert_states(g, want, what=""):
    got = g.state_get_all()
    for k, w in enumerate(want):
        assert got[k].as_dict() == w.as_dict(), (what, k)


def fresh_record(cfg):
    with demod(cfg, 1) as g:
        return bytes(g.state_get(0))


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("name", NAMES)
def test_bulk_equals_per_stream_and_the_oracle(oracle_lib, name, nb):
    S = 5
    cfg = make_cfg(name, nb)
    rows = sources(name, S, 4 * nb, 11)
    whole = [oracle_on(oracle_lib, cfg, rows[s]) for s in range(S)]
    half = [oracle_on(oracle_lib, cfg, rows[s][:2 * nb]) for s in range(S)]
    got = [[] for _ in range(S)]
    with demod(cfg, S) as g:
        for r in range(2):
            for s, p in enumerate(feed(g, [rows[s][r * nb:(r + 1) * nb] for s in range(S)])):
                got[s].append(p)
        states = g.state_get_all()
        assert bytes(states) == b"".join(bytes(g.state_get(s)) for s in range(S))  # byte for byte
        for s in range(S):
            assert states[s].as_dict() == half[s][1].as_dict(), s
    with demod(cfg, S) as g2:
        g2.state_set_all(states)
        assert bytes(g2.state_get_all()) == bytes(states)
        for r in range(2, 4):
            for s, p in enumerate(feed(g2, [rows[s][r * nb:(r + 1) * nb] for s in range(S)])):
                got[s].append(p)
        assert_states(g2, [w[1] for w in whole])
        # the wrong count is refused and changes nothing
        for bad in (S - 1, S + 1, 0):
            arr = (RtlfmStreamState * max(bad, 1))()
            assert g2.lib.rtlfm_gpu_state_set_all(g2._h, arr, bad) == -errno.EINVAL
        n = C.c_int()
        assert g2.lib.rtlfm_gpu_state_get_all(g2._h, (RtlfmStreamState * (S - 1))(), S - 1, C.byref(n)) == -errno.ENOBUFS
        assert n.value == S
        assert_states(g2, [w[1] for w in whole])
    for s in range(S):
        assert np.array_equal(np.concatenate(got[s]), whole[s][0]), s


def test_move_kernel_alone_against_a_numpy_gather():
    """No demodulation: 300 records of random bytes gathered into handles of 1, 5, 64, 65 and 300 streams - one lane's
    worth, less than a wave of dwords, exactly and one more than 64 records, and several workgroups - through maps with
    duplicates, -1 entries and the identity."""
    cfg = make_cfg("box7_rdc_adc_sq", 1)
    N = 300
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 256, N * REC, dtype=np.uint8)
    init = np.frombuffer(fresh_record(cfg), dtype=np.uint8)
    with demod(cfg, N) as src:
        src.state_set_all((RtlfmStreamState * N).from_buffer_copy(raw.tobytes()))
        tab = raw.reshape(N, REC)
        for n in (1, 5, 64, 65, 300):
            maps = [np.arange(n), rng.integers(-1, N, n), rng.integers(0, 3, n) * 149, np.full(n, -1), np.full(n, N - 1),
                    np.arange(N - n, N)[::-1]]
            maps[1][0] = -1
            with demod(cfg, n) as dst:
                for m in maps:
                    m = m.astype(np.int32)
                    dst.move_from(src, m)
                    want = np.where((m < 0)[:, None], init[None, :], tab[np.maximum(m, 0)])
                    assert np.array_equal(table(dst.state_get_all()), want), (n, m[:8])
                    if n <= 5:
                        assert b"".join(bytes(dst.state_get(k)) for k in range(n)) == want.tobytes()
        assert np.array_equal(table(src.state_get_all()), tab)  # the source is left as it was


@pytest.mark.parametrize("name", NAMES)
def test_in_place_permutation_rotation_and_fan_out(oracle_lib, name):
    S, nb = 7, 3
    cfg = make_cfg(name, nb)
    rows = sources(name, S, 4 * nb, 23)
    with demod(cfg, S) as g:
        for r in range(2):
            feed(g, [rows[s][r * nb:(r + 1) * nb] for s in range(S)])
        want = [oracle_on(oracle_lib, cfg, rows[s][:2 * nb])[1] for s in range(S)]
        assert_states(g, want, "before")
        for m in ([6, 5, 4, 3, 2, 1, 0], [2, 3, 4, 5, 6, 0, 1], [0, 0, 2, 0, 4, 5, 0]):
            before = table(g.state_get_all()).copy()
            g.move_from(g, m)
            assert np.array_equal(table(g.state_get_all()), before[m]), m
            want = [want[k] for k in m]
            assert_states(g, want, m)
        # what each stream now carries goes on with THAT stream's next buffers
        got = [[] for _ in range(S)]
        for r in range(2, 4):
            for k, p in enumerate(feed(g, [rows[k][r * nb:(r + 1) * nb] for k in range(S)])):
                got[k].append(p)
        for k in range(S):
            pcm, st = oracle_on(oracle_lib, cfg, rows[k][2 * nb:], want[k])
            assert np.array_equal(np.concatenate(got[k]), pcm), k
            assert g.state_get(k).as_dict() == st.as_dict(), k


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("name", NAMES)
def test_continuity_across_a_regroup(oracle_lib, name, nb):
    """Sources 6, 0 and 3 of a 7-stream handle go on in a 4-stream handle beside a source that joins: every PCM row and
    every state is the oracle's on that source's WHOLE input."""
    S = 7
    cfg = make_cfg(name, nb)
    rows = sources(name, S + 1, 4 * nb, 31)  # source 7 is the one that joins
    m = [6, 0, 3, -1]
    who = [6, 0, 3, 7]
    got = {i: [] for i in who}
    with demod(cfg, S) as src, demod(cfg, len(m)) as dst:
        for r in range(2):
            pcm = feed(src, [rows[s][r * nb:(r + 1) * nb] for s in range(S)])
            for i in who[:3]:
                got[i].append(pcm[i])
        dst.move_from(src, m)
        for r in range(2):
            new = slice(r * nb, (r + 1) * nb)
            old = slice((2 + r) * nb, (3 + r) * nb)
            pcm = feed(dst, [rows[i][old] for i in who[:3]] + [rows[7][new]])
            for k, i in enumerate(who):
                got[i].append(pcm[k])
        for k, i in enumerate(who):
            want, st = oracle_on(oracle_lib, cfg, rows[i] if i != 7 else rows[7][:2 * nb])
            assert np.array_equal(np.concatenate(got[i]), want), (k, i)
            assert dst.state_get(k).as_dict() == st.as_dict(), (k, i)
        # ... and the old handle still holds what it held
        assert_states(src, [oracle_on(oracle_lib, cfg, rows[s][:2 * nb])[1] for s in range(S)])


def test_the_owed_mute_travels(oracle_lib):
    """rtlfm_gpu_mute(s, 3 * 2048 + 5), one buffer run on src, then the move: the other 2 * 2048 + 5 bytes are muted on
    dst - and on src, which is left as it was.  The oracle on the muted input, as test_mute_equals_oracle_on_muted_input."""
    S, nb = 5, 2
    cfg = make_cfg("box7_rdc_adc_sq", nb)
    rng = np.random.default_rng(41)
    rows = [[sm.tone_or_noise(rng, L, True) for _ in range(6)] for _ in range(S + 1)]
    models = [sm.StreamModel(oracle_lib, cfg, 1 << 30) for _ in range(S + 1)]

    def clone(mo):
        c = sm.StreamModel(oracle_lib, cfg, 1 << 30)
        c.state, c.mute = copy_state(mo.state), mo.mute
        return c
    m = [4, 2, -1, 0, 2]
    with demod(cfg, S) as src, demod(cfg, len(m)) as dst:
        for s, count in ((0, 3 * L + 5), (2, 3 * L + 5), (4, 100)):
            src.mute(s, count)
            models[s].mute = count
        pcm = feed(src, [[rows[s][0]] for s in range(S)])
        for s in range(S):
            assert np.array_equal(pcm[s], models[s].run([rows[s][0]])[0]), s
        assert [mo.mute for mo in models[:S]] == [2 * L + 5, 0, 2 * L + 5, 0, 0]
        dst.mute(2, 77)  # replaced by the move: a stream that starts afresh is owed nothing
        dst.move_from(src, m)
        dmodels = [clone(models[i]) if i >= 0 else models[S] for i in m]
        for r, (lo, hi) in enumerate(((1, 3), (3, 4), (4, 6))):
            pcm = feed(dst, [rows[i if i >= 0 else S][lo:hi] for i in m])
            for k, i in enumerate(m):
                assert np.array_equal(pcm[k], dmodels[k].run(rows[i if i >= 0 else S][lo:hi])[0]), (r, k)
            pcm = feed(src, [rows[s][lo:hi] for s in range(S)])
            for s in range(S):
                assert np.array_equal(pcm[s], models[s].run(rows[s][lo:hi])[0]), (r, s)
        assert all(mo.mute == 0 for mo in dmodels + models)
        for k in range(len(m)):
            assert dst.state_get(k).as_dict() == dmodels[k].state.as_dict(), k


def _both_go_on(po, cfg, src, dst, rows, at, nb, want_src, want_dst):
    """One more run on each handle; want_*: the oracle states the streams carry (updated in place)."""
    for g, want in ((src, want_src), (dst, want_dst)):
        pcm = feed(g, [rows[k][at:at + nb] for k in range(len(want))])
        for k in range(len(want)):
            w, want[k] = oracle_on(po, cfg, rows[k][at:at + nb], want[k])
            assert np.array_equal(pcm[k], w), k
        assert_states(g, want)


def test_move_errors_leave_both_handles_as_they_were(oracle_lib):
    name, nb = "box7_rdc_adc_sq", 1
    cfg = make_cfg(name, nb)
    rows = sources(name, 7, 8, 53)
    lib = capi.load()
    with demod(cfg, 7) as src, demod(cfg, 4) as dst:
        want_src = [None] * 7
        want_dst = [None] * 4
        _both_go_on(oracle_lib, cfg, src, dst, rows, 0, nb, want_src, want_dst)
        at = 1

        def refused(code, m, a=dst, b=src):
            m = np.asarray(m, dtype=np.int32)
            assert lib.rtlfm_gpu_state_move(a._h, b._h, m.ctypes.data, m.size) == code, m
        refused(-errno.EINVAL, [0, 1, 2])            # n != dst's streams
        refused(-errno.EINVAL, [0, 1, 2, 3, 4])
        refused(-errno.EINVAL, [0, 1, 2, 7])         # an entry out of range
        refused(-errno.EINVAL, [0, -2, 2, 3])
        refused(-errno.EINVAL, [0, 1, 2, 4], a=dst, b=dst)  # in place, the range is the handle's own
        assert lib.rtlfm_gpu_state_move(dst._h, src._h, None, 4) == -errno.EINVAL
        assert lib.rtlfm_gpu_state_move(None, src._h, None, 4) == -errno.EINVAL
        _both_go_on(oracle_lib, cfg, src, dst, rows, at, nb, want_src, want_dst)
        at += 1
        # a begun run, on either side
        for busy, want in ((src, want_src), (dst, want_dst)):
            ns = busy.nstreams
            for k in range(ns):
                busy.push(rows[k][at], k)
            assert busy.run_begin() == 1
            refused(-errno.EBUSY, [0, 1, 2, 3])
            refused(-errno.EBUSY, list(range(ns)), a=busy, b=busy)
            busy.run_end()
            out, lens = busy.fetch_all()
            for k in range(ns):
                w, want[k] = oracle_on(oracle_lib, cfg, [rows[k][at]], want[k])
                assert np.array_equal(out[k, :lens[k]], w), k
            assert_states(busy, want)
            # (the other handle takes the same buffer, so that both stand at the same place again)
            other, owant = (dst, want_dst) if busy is src else (src, want_src)
            pcm = feed(other, [[rows[k][at]] for k in range(other.nstreams)])
            for k in range(other.nstreams):
                w, owant[k] = oracle_on(oracle_lib, cfg, [rows[k][at]], owant[k])
                assert np.array_equal(pcm[k], w), k
            at += 1
        # an open slot between acquire and commit
        buf, cap = C.c_void_p(), C.c_uint32()
        assert lib.rtlfm_gpu_acquire(src._h, 3, C.byref(buf), C.byref(cap)) == 0 and cap.value == L
        refused(-errno.EBUSY, [0, 1, 2, 3])
        assert lib.rtlfm_gpu_commit(src._h, 3, 0) == 0  # the slot goes back unused
        refused(0, [0, 1, 2, 3])                     # ... and now it moves
        want_dst[:] = [copy_state(w) for w in want_src[:4]]
        assert_states(dst, want_dst)
        _both_go_on(oracle_lib, cfg, src, dst, rows, at, nb, want_src, want_dst)


def test_move_between_devices_is_exdev(oracle_lib):
    if torch.cuda.device_count() < 2:
        pytest.skip("test_move_between_devices_is_exdev: one device visible, -EXDEV needs two")
    from rtlsdr_amd.demod import GpuDemod
    cfg = make_cfg("box7_rdc_adc_sq", 1)
    rows = sources("box7_rdc_adc_sq", 2, 2, 3)
    with GpuDemod(cfg, 2, 0) as a, GpuDemod(cfg, 2, 1) as b:
        want_a, want_b = [None] * 2, [None] * 2
        _both_go_on(oracle_lib, cfg, a, b, rows, 0, 1, want_a, want_b)
        m = np.array([1, 0], dtype=np.int32)
        assert a.lib.rtlfm_gpu_state_move(b._h, a._h, m.ctypes.data, 2) == -errno.EXDEV
        assert a.lib.rtlfm_gpu_state_move(a._h, b._h, m.ctypes.data, 2) == -errno.EXDEV
        _both_go_on(oracle_lib, cfg, a, b, rows, 1, 1, want_a, want_b)
        b.state_set_all(a.state_get_all())  # the way across devices
        assert bytes(b.state_get_all()) == bytes(a.state_get_all())


@pytest.mark.parametrize("name", NAMES)
def test_save_destroy_create_load_continue(oracle_lib, tmp_path, name):
    """Two runs, save, a new handle, load, two more runs = the uninterrupted run - with a mute that is still owed when the
    file is written.  Files that do not fit are refused with their own code and change nothing; max_blocks may differ."""
    S, nb = 5, 3
    cfg = make_cfg(name, nb)
    rows = sources(name, S, 4 * nb, 61)
    owed = 2 * nb * L + 700  # stream 1: 700 bytes of it reach into the second half
    whole = []
    for s in range(S):
        x = np.concatenate(rows[s])
        if s == 1:
            x[:owed] = 127
        whole.append(oracle_lib.run_stream(cfg, x))
    got = [[] for _ in range(S)]
    path = tmp_path / "handle.snap"
    with demod(cfg, S) as g:
        g.mute(1, owed)
        for r in range(2):
            for s, p in enumerate(feed(g, [rows[s][r * nb:(r + 1) * nb] for s in range(S)])):
                got[s].append(p)
        g.save(path)
        saved = bytes(g.state_get_all())
    scfg, sn = capi.snapshot_info(path)
    assert sn == S and bytes(scfg) == bytes(cfg)
    # three files that must not load: another stream count, another downsample, a damaged one
    lib = capi.load()
    recs = (RtlfmStreamState * S).from_buffer_copy(saved)
    other_n, other_cfg, damaged = tmp_path / "n.snap", tmp_path / "cfg.snap", tmp_path / "bad.snap"
    assert lib.rtlfm_snapshot_write(os.fsencode(other_n), C.byref(cfg), S - 1, recs, None) == 0
    c2 = make_cfg(name, nb, downsample=cfg.downsample + 1)
    assert lib.rtlfm_snapshot_write(os.fsencode(other_cfg), C.byref(c2), S, recs, None) == 0
    b = bytearray(path.read_bytes())
    b[len(b) // 2] ^= 0x10
    damaged.write_bytes(bytes(b))
    cfg2 = make_cfg(name, nb + 1)  # differs in max_blocks only: loads
    with demod(cfg2, S) as g:
        g.load(path)
        assert bytes(g.state_get_all()) == saved
        for p, code in ((other_n, -errno.ERANGE), (other_cfg, -errno.EMEDIUMTYPE), (damaged, -errno.EILSEQ),
                        (tmp_path / "missing.snap", -errno.ENOENT)):
            with pytest.raises(capi.RtlfmError) as e:
                g.load(p)
            assert e.value.code == code, p
        assert bytes(g.state_get_all()) == saved
        for r in range(2, 4):
            for s, p in enumerate(feed(g, [rows[s][r * nb:(r + 1) * nb] for s in range(S)])):
                got[s].append(p)
        assert_states(g, [w[1] for w in whole])
    for s in range(S):
        assert np.array_equal(np.concatenate(got[s]), whole[s][0]), s


def test_nothing_is_added_to_a_run(oracle_lib, tmp_path):
    """The launch count of a run (rtlfm_gpu_timing_read) is the same before and after every new call."""
    name, S, nb = "fifth4_fir_deemph_lpr", 5, 3
    cfg = make_cfg(name, nb)
    rows = sources(name, S, 3 * nb, 71)
    with demod(cfg, S) as g, demod(cfg, S) as other:
        g.timing_enable(True)
        g.timing_read()
        counts = []
        for r in range(3):
            feed(g, [rows[s][r * nb:(r + 1) * nb] for s in range(S)])
            counts.append(g.timing_read()[1])
            if r == 0:
                g.state_set_all(g.state_get_all())
                g.move_from(g, list(range(S)))
                other.move_from(g, list(range(S)))
                g.move_from(other, list(range(S)))
                g.save(tmp_path / "t.snap")
                g.load(tmp_path / "t.snap")
                assert g.timing_read()[1] == 0  # none of them is counted as a front-end launch either
        assert counts[0] > 0 and counts == [counts[0]] * 3, counts
        assert_states(g, [oracle_on(oracle_lib, cfg, rows[s])[1] for s in range(S)])


def test_cost_at_4096_streams():
    """One copy instead of 8192 synchronising copies: the bulk pair and one move must each take less than a tenth of the
    per-stream loop (the loop uses only entry points the library had before; the expected gap is two to three orders of
    magnitude, the factor of ten is the margin for a busy shared box)."""
    N = 4096
    cfg = make_cfg("box7_rdc_adc_sq", 1)
    with demod(cfg, N) as g:
        ident = np.arange(N, dtype=np.int32)
        g.state_set_all(g.state_get_all())  # (first calls: allocations, the map's device array)
        g.move_from(g, ident)
        g.state_set(0, g.state_get(0))
        t0 = time.perf_counter()
        for s in range(N):
            g.state_set(s, g.state_get(s))
        t_loop = time.perf_counter() - t0
        t_bulk, t_move = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            g.state_set_all(g.state_get_all())
            t_bulk.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            g.move_from(g, ident)
            t_move.append(time.perf_counter() - t0)
        t_bulk, t_move = max(t_bulk), max(t_move)  # the WORST of three against the one loop
        print(f"\n4096 streams: state_get + state_set loop {t_loop * 1e6:.0f} us, state_get_all + state_set_all "
              f"{t_bulk * 1e6:.0f} us, one state_move {t_move * 1e6:.0f} us")
        assert t_bulk < t_loop / 10, (t_bulk, t_loop)
        assert t_move < t_loop / 10, (t_move, t_loop)
