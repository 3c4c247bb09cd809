"""Options source_stats / source_health on the GPU (include/rtlfm_hip.h, "source_stats"): the ADC statistics and the input
health per SOURCE of a handle with channels on - the records bit for bit against tests/health_model.py and a numpy
restatement of the statistics' four lines, with source_dc off (the stream readers' kernels over the source rows) and on
(k_source_prepass: the sums, the statistics and the health from one read); the same records whatever front end follows;
PCM, lengths, state records and the sample counter untouched; the ring, short buffers, verify_twice, the calls' contract
and the soft AGC per source.

Shapes: 512 bytes is the wave-per-buffer form, 7680 its upper edge, 8192 the workgroup form's lower edge, 16384 the
workgroup form with a remainder loop, 32768 the first length whose statistics skip bytes (step 4, masks from LDS), 262144 the
largest; 1 and 3 sources, 1, 4 and 5 channels, runs of 1 and 3 buffers (the wave form packs four (source, buffer) pairs into
a workgroup: 3 x 3 = 9 pairs leave one workgroup with a single wave)."""
import ctypes as C
import errno

import numpy as np
import pytest

import health_model as hm
from channel_common import assert_rows, demod, make_steps, random_bank_taps, random_fir_taps, raw_cfg, run_once, steps_for, to_device
from rtlsdr_amd import capi, synth

pytestmark = pytest.mark.gpu

D = 10
LENGTHS = (512, 7680, 8192, 16384, 32768, 262144)
SHAPES = [(1, 1, 1), (3, 4, 3), (3, 5, 1), (1, 5, 3), (3, 1, 3), (1, 4, 1)]  # (sources, per_source, nblocks)
RECORDS = [(1, 0), (0, 1), (1, 1)]  # (source_stats, source_health)


def stats_model(buffers):
    """uint8 [..., L] -> capi.INPUT_STAT_DTYPE [...]: max, step, pow_sum, pow_count as include/rtlfm_hip.h states them."""
    a = np.ascontiguousarray(buffers, dtype=np.uint8)
    L = a.shape[-1]
    step = 2
    while L >= 16384 * step:
        step += 2
    i = np.arange(0, L, step)
    x = a.astype(np.int64) - 127
    out = np.zeros(a.shape[:-1], dtype=capi.INPUT_STAT_DTYPE)
    out["pow_sum"] = (x[..., i] ** 2 + x[..., i + 1] ** 2).sum(axis=-1)
    out["pow_count"] = i.size
    out["max"] = a.max(axis=-1)
    out["step"] = step
    return out


def planted(nsrc, L, nb):
    """A byte counter with a gap or a threshold value at every unit, wave and workgroup boundary (health_model.py)."""
    return hm.plant_values(hm.plant_gaps(hm.counter((nsrc, nb * L), start=3), L), L)


def full_scale(nsrc, L, nb, seed):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, size=(nsrc, nb * L), dtype=np.uint8)
    src[0, : L // 2] = rng.integers(0, 2, size=L // 2).astype(np.uint8) * 255
    return src


def want_records(src, L):
    b = src.reshape(src.shape[0], -1, L)
    return stats_model(b), hm.records(b)


def assert_recs(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)[:4].tolist()
        raise AssertionError(f"{what}: records differ at {bad}: {[got[tuple(i)] for i in bad]} for {[want[tuple(i)] for i in bad]}")


def chan_handle(cfg, nsrc, per, path=0, **options):
    g = demod(cfg, nsrc * per, **options)
    g.set_path(path)
    g.set_channels(per, steps=make_steps(nsrc * per, 5 + per))
    return g


def fresh_run(g, d, L, nb, stats, health, dc):
    """reset(), the options, one run of buffers 0 .. nb of d.  Returns everything a run leaves: (PCM rows, the state
    records' bytes, channels_tell(), statistics or None, health or None)."""
    g.reset()
    g.set_option("source_dc", dc)
    g.set_option("source_stats", stats)
    g.set_option("source_health", health)
    rows, _ = run_once(g, d, L, 0, nb)
    return (rows, bytes(g.state_get_all()), g.channels_tell(), g.source_stats_all() if stats else None,
            g.source_health_all() if health else None)


def assert_same_run(a, b, what):
    assert_rows(a[0], b[0], what)  # (lengths with them)
    assert a[1] == b[1], f"{what}: the state records differ"
    assert a[2] == b[2], (what, a[2], b[2])


# ------------------------------------------------------------ records against the model ----

@pytest.mark.parametrize("nsrc, per, nb", SHAPES, ids=[f"{s}x{p}x{n}" for s, p, n in SHAPES])
@pytest.mark.parametrize("L", LENGTHS)
def test_records_equal_the_model(L, nsrc, per, nb):
    """Each option alone and both together, with source_dc off and on, on the planted counter (health) and on full-scale
    random bytes (statistics) - both records are checked on both inputs.  The PCM, the state and the counter of every run
    equal those of the run with both record options off."""
    cfg = raw_cfg(D, L, nb)
    with chan_handle(cfg, nsrc, per) as g:
        for name, src in (("planted", planted(nsrc, L, nb)), ("full scale", full_scale(nsrc, L, nb, L + nsrc))):
            want_s, want_h = want_records(src, L)
            d = to_device(src)
            for dc in (0, 1):
                plain = fresh_run(g, d, L, nb, 0, 0, dc)
                for stats, health in RECORDS:
                    what = f"{name} dc={dc} stats={stats} health={health}"
                    got = fresh_run(g, d, L, nb, stats, health, dc)
                    if stats:
                        assert_recs(got[3], want_s, what + ": statistics")
                    if health:
                        assert_recs(got[4], want_h, what + ": health")
                    assert_same_run(got, plain, what)


@pytest.mark.parametrize("L", LENGTHS)
def test_records_equal_the_standalone_operators(L):
    """The handle's records with source_dc on - k_source_prepass - against rtlfm_gpu_input_health_stats_device, the stream
    readers' launch without a handle, on the same device rows: what the two-launch form of the A/B (LAB.md) left.  (Its
    sums against k_rdc_sums_wide's: the PCM of test_records_equal_the_model, whose plain runs take those.)"""
    import torch
    nsrc, per, nb = 3, 4, 3
    src = full_scale(nsrc, L, nb, 7 + L)
    d = to_device(src)
    h_out = torch.zeros(nsrc * nb * 16, dtype=torch.uint8, device="cuda")
    s_out = torch.zeros(nsrc * nb * 16, dtype=torch.uint8, device="cuda")
    lib = capi.load()
    capi.check(lib.rtlfm_gpu_input_health_stats_device(0, d.data_ptr(), d.stride(0), L, nb, nsrc, h_out.data_ptr(), s_out.data_ptr(), 1, None),
               "rtlfm_gpu_input_health_stats_device")
    torch.cuda.synchronize()
    want_h = h_out.cpu().numpy().view(capi.INPUT_HEALTH_DTYPE).reshape(nsrc, nb)
    want_s = s_out.cpu().numpy().view(capi.INPUT_STAT_DTYPE).reshape(nsrc, nb)
    with chan_handle(raw_cfg(D, L, nb), nsrc, per) as g:
        got = fresh_run(g, d, L, nb, 1, 1, 1)
    assert_recs(got[3], want_s, "statistics")
    assert_recs(got[4], want_h, "health")


# ------------------------------------------------------------ every front end ----

FRONTS = [("mix", 0), ("mix", 1), ("fir", 0), ("fir", 1), ("bank", 0), ("bank", 1)]


def front_handle(front, path, cfg, nsrc, **options):
    if front == "bank":
        g = demod(cfg, nsrc * 8, **options)
        g.set_path(path)
        g.set_channels(8, steps=steps_for(nsrc * 8))
        g.set_channel_bank(8, *random_bank_taps(8, 64, 17))
        return g
    g = chan_handle(cfg, nsrc, 4, path, **options)
    if front == "fir":
        g.set_channel_filter(*random_fir_taps(33, 19))
    return g


@pytest.mark.parametrize("front, path", FRONTS, ids=[f"{f}-path{p}" for f, p in FRONTS])
def test_same_records_and_untouched_pcm_on_every_front_end(front, path):
    """Mixer path 2 and path 1, the channel filter and the bank (K = 8) on both paths: the records do not depend on what
    follows, and with source_dc off and on PCM, lengths, state records and channels_tell() equal the run without them."""
    nsrc, L, nb = 3, 2048, 3
    src = full_scale(nsrc, L, nb, 23)
    want_s, want_h = want_records(src, L)
    with front_handle(front, path, raw_cfg(D, L, nb), nsrc) as g:
        d = to_device(src)
        for dc in (0, 1):
            plain = fresh_run(g, d, L, nb, 0, 0, dc)
            assert plain[2] == nb * L // 2
            got = fresh_run(g, d, L, nb, 1, 1, dc)
            what = f"{front} path {path} dc={dc}"
            assert_recs(got[3], want_s, what + ": statistics")
            assert_recs(got[4], want_h, what + ": health")
            assert_same_run(got, plain, what)


# ------------------------------------------------------------ the ring ----

def push_run(g, src, pieces):
    for i in range(src.shape[0]):
        for at, n in pieces:
            g.rtlsdr_callback(src[i, at:at + n], stream=i)


@pytest.mark.parametrize("dc", [0, 1])
def test_source_ring_equals_run_device(dc):
    """push -> run -> fetch over the source ring: the records of the handle's device copy equal run_device's on the same
    bytes (and the model)."""
    nsrc, per, L, nb = 3, 4, 8192, 3
    src = planted(nsrc, L, nb)
    want_s, want_h = want_records(src, L)
    with chan_handle(raw_cfg(D, L, nb), nsrc, per) as g:
        direct = fresh_run(g, to_device(src), L, nb, 1, 1, dc)
    with chan_handle(raw_cfg(D, L, nb), nsrc, per, source_ring=1, source_dc=dc, source_stats=1, source_health=1) as g:
        push_run(g, src, [(j * L, L) for j in range(nb)])
        g.full_demod()
        o, n = g.fetch_all()
        assert_rows([o[s, :n[s]] for s in range(g.nstreams)], direct[0], "the ring's PCM")
        got_s, got_h = g.source_stats_all(), g.source_health_all()
        for a in range(nsrc):
            assert np.array_equal(g.source_stats(a), got_s[a]) and np.array_equal(g.source_health(a), got_h[a]), a
    for got, want, what in ((got_s, want_s, "statistics"), (got_h, want_h, "health")):
        assert_recs(got, want, what)
    assert_recs(got_s, direct[3], "statistics against run_device")
    assert_recs(got_h, direct[4], "health against run_device")


@pytest.mark.parametrize("dc", [0, 1])
def test_ring_run_with_short_buffers_files_each_record_over_its_own_length(dc):
    nsrc, per, L = 3, 4, 16384
    pieces = [(0, 16384), (16384, 16384), (32768, 1536)]
    src = hm.plant_values(hm.plant_gaps(hm.counter((nsrc, 3 * L), start=9), 512), 512)
    want_s = np.stack([stats_model(src[:, at:at + n]) for at, n in pieces], axis=1)
    want_h = np.stack([hm.records(src[:, at:at + n]) for at, n in pieces], axis=1)
    with chan_handle(raw_cfg(D, L, 3), nsrc, per, source_ring=1, source_dc=dc, source_stats=1, source_health=1) as g:
        push_run(g, src, pieces)
        g.full_demod()
        assert_recs(g.source_stats_all(), want_s, "statistics")
        assert_recs(g.source_health_all(), want_h, "health")
        # a run of whole buffers behind it: the rows are the run's again
        push_run(g, src, pieces[:2])
        g.full_demod()
        assert_recs(g.source_health_all(), want_h[:, :2], "health of the run behind")


@pytest.mark.parametrize("dc", [0, 1])
def test_verify_twice_leaves_one_executions_records(dc):
    nsrc, per, L, nb = 3, 4, 2048, 3
    src = full_scale(nsrc, L, nb, 29)
    want_s, want_h = want_records(src, L)
    with chan_handle(raw_cfg(D, L, nb), nsrc, per, verify_twice=1) as g:
        got = fresh_run(g, to_device(src), L, nb, 1, 1, dc)
        assert g.get_option("verify_runs") == 1 and g.get_option("verify_mismatches") == 0
    assert_recs(got[3], want_s, "statistics")
    assert_recs(got[4], want_h, "health")


# ------------------------------------------------------------ the contract ----

def fetch_codes(g, source=0, cap=8):
    """The four fetch calls' return codes and the *n each wrote (-1: not written)."""
    lib, out = g.lib, np.zeros(64 * cap * 16, dtype=np.uint8)
    codes = []
    for fn, one in ((lib.rtlfm_gpu_source_stats, True), (lib.rtlfm_gpu_source_stats_all, False),
                    (lib.rtlfm_gpu_source_health, True), (lib.rtlfm_gpu_source_health_all, False)):
        n = C.c_int(-1)
        r = fn(g._h, source, out.ctypes.data, cap, C.byref(n)) if one else fn(g._h, out.ctypes.data, cap, C.byref(n))
        codes.append((r, n.value))
    return codes


def test_contract():
    nsrc, per, L, nb = 3, 2, 2048, 3
    S = nsrc * per
    src = full_scale(S, L, nb, 31)
    want_s, want_h = want_records(src, L)
    cfg = raw_cfg(D, L, nb)
    with chan_handle(cfg, nsrc, per, source_ring=1) as g:
        d = to_device(src)
        # -ENODATA: the options off; on, before the first run
        run_once(g, d[:nsrc], L, 0, nb)
        assert [c for c, _ in fetch_codes(g)] == [-errno.ENODATA] * 4
        g.set_option("source_stats", 1)
        g.set_option("source_health", 1)
        assert [c for c, _ in fetch_codes(g)] == [-errno.ENODATA] * 4
        run_once(g, d[:nsrc], L, 0, nb)
        assert fetch_codes(g) == [(0, nb)] * 4
        # -ENOBUFS with *n written; -EINVAL for a source outside [0, sources) and for null pointers
        assert fetch_codes(g, cap=nb - 1) == [(-errno.ENOBUFS, nb)] * 4
        for bad in (-1, nsrc):
            codes = fetch_codes(g, source=bad)
            assert codes[0][0] == codes[2][0] == -errno.EINVAL, bad
        n = C.c_int()
        assert g.lib.rtlfm_gpu_source_health(g._h, 0, None, 8, C.byref(n)) == -errno.EINVAL
        assert g.lib.rtlfm_gpu_source_stats_all(g._h, np.zeros(1024, np.uint8).ctypes.data, 8, None) == -errno.EINVAL
        # -EINVAL for a value of 2, -EBUSY inside run_begin / run_end: a refused call changes nothing
        for name in (b"source_stats", b"source_health"):
            assert g.lib.rtlfm_gpu_set_option(g._h, name, 2) == -errno.EINVAL
            assert g.lib.rtlfm_gpu_set_option(g._h, name, -1) == -errno.EINVAL
        push_run(g, src[:nsrc], [(0, L)])
        assert g.run_begin() == 1
        for name in (b"source_stats", b"source_health"):
            assert g.lib.rtlfm_gpu_set_option(g._h, name, 0) == -errno.EBUSY
        g.run_end()
        assert g.get_option("source_stats") == 1 and g.get_option("source_health") == 1
        assert_recs(g.source_health_all(), want_h[:nsrc, :1], "the ring's run behind -EBUSY")
        # the per-stream options stay refused while channels are on, and set_channels stays refused while one of them is on
        for name in (b"input_stats", b"input_health"):
            assert g.lib.rtlfm_gpu_set_option(g._h, name, 1) == -errno.ENOTSUP
        # set_channels from 3 sources to 1 and back: records of the right shape each time, none in between
        for per_now in (S, per):
            g.set_channels(per_now, steps=make_steps(S, 3))
            assert [c for c, _ in fetch_codes(g)] == [-errno.ENODATA] * 4
            rows = S // per_now
            run_once(g, d[:rows], L, 0, nb)
            assert_recs(g.source_stats_all(), want_s[:rows], f"{rows} sources: statistics")
            assert_recs(g.source_health_all(), want_h[:rows], f"{rows} sources: health")
            assert fetch_codes(g, source=rows)[0][0] == -errno.EINVAL
        # -ENODATA after a run with channels off; the options stay set and act again once channels are back on
        g.set_channels(0)
        run_once(g, d, L, 0, nb)
        assert [c for c, _ in fetch_codes(g)] == [-errno.ENODATA] * 4
        assert g.get_option("source_stats") == 1
        g.set_channels(per, steps=make_steps(S, 3))
        run_once(g, d[:nsrc], L, 0, 1)
        assert_recs(g.source_health_all(), want_h[:nsrc, :1], "channels back on")
    # the options may be set with channels off and act on nothing there; with per-stream options on set_channels is refused
    with demod(cfg, S, source_stats=1, source_health=1, input_health=1) as g, demod(cfg, S, input_health=1) as twin:
        a, _ = run_once(g, to_device(src), L, 0, nb)
        b, _ = run_once(twin, to_device(src), L, 0, nb)
        assert_rows(a, b, "channels off")
        assert np.array_equal(g.input_health_all(), twin.input_health_all())
        st = np.ascontiguousarray(make_steps(S, 3), dtype=np.uint32)
        assert g.lib.rtlfm_gpu_set_channels(g._h, per, st.ctypes.data) == -errno.ENOTSUP


def test_options_at_0_leave_the_launch_count_alone():
    """rtlfm_gpu_timing_read's count for a channel run: the options never touched, set and put back, and on (the launches
    sit inside the front end's timed pair)."""
    nsrc, per, L, nb = 2, 2, 2048, 2
    src = full_scale(nsrc, L, nb, 37)
    counts = {}
    for kind in ("never", "back", "on"):
        for dc in (0, 1):
            with chan_handle(raw_cfg(D, L, nb), nsrc, per, source_dc=dc) as g:
                if kind != "never":
                    g.set_option("source_stats", 1)
                    g.set_option("source_health", 1)
                if kind == "back":
                    g.set_option("source_stats", 0)
                    g.set_option("source_health", 0)
                g.timing_enable(True)
                g.timing_read()
                run_once(g, to_device(src), L, 0, nb)
                counts[kind, dc] = g.timing_read()[1]
    for dc in (0, 1):
        assert counts["never", dc] == counts["back", dc] == counts["on", dc], counts


# ------------------------------------------------------------ the engine ----

def loudness_sources(L, nbuf):
    """Four sources: quiet (amplitude 5), middling (60), clipped (127 and more) and one that alternates buffer by buffer
    (those of tests/test_agc_gpu.py)."""
    quiet = synth.fm_iq_u8(1, nbuf * L // 2, amplitude=5.0, first_stream=0)[0]
    mid = synth.fm_iq_u8(1, nbuf * L // 2, amplitude=60.0, first_stream=1)[0]
    loud = synth.fm_iq_u8(1, nbuf * L // 2, amplitude=127.0, first_stream=2)[0]
    alt = quiet.copy()
    for b in range(0, nbuf, 2):
        alt[b * L:(b + 1) * L] = loud[b * L:(b + 1) * L]
    return np.stack([quiet, mid, loud, alt])


@pytest.mark.parametrize("settle", [0, 4])
def test_soft_agc_update_feeds_source_i_to_input_i(settle):
    from rtlsdr_amd.agc import SoftAgc
    nsrc, per, L, nb, runs = 4, 2, 16384, 4, 6
    gain_counts = [29, 29, 5, 3]
    iq = loudness_sources(L, nb * runs)
    want = hm.records(iq.reshape(nsrc, nb * runs, L))
    assert (8000 * want["overload"][2].astype(np.int64) >= L).all() and not want["overload"][0].any()  # clipped / quiet for real
    models = [hm.StreamModel(a, gain_counts[a], settle=settle) for a in range(nsrc)]
    with chan_handle(raw_cfg(D, L, nb), nsrc, per, source_health=1, source_dc=1) as g, SoftAgc(gain_counts) as a:
        a.set_settle(settle)
        a.set_index(2, 4)
        models[2].index = 4
        got, d = [], to_device(iq)
        for r in range(runs):
            run_once(g, d, L, r * nb, nb)
            a.update(g)
            for i in range(nsrc):
                models[i].feed(want[i, r * nb:(r + 1) * nb], L)
            got += a.poll()
            assert [a.state(i) for i in range(nsrc)] == [m.state() for m in models], r
        for i in range(nsrc):
            assert [e for e in got if e["stream"] == i] == models[i].events, i
        # an engine with an input per STREAM does not fit a handle that reports per source
        with SoftAgc([3] * (nsrc * per)) as wrong, pytest.raises(ValueError):
            wrong.update(g)
    assert models[0].events and models[2].events and models[3].events
    assert models[2].index == 0 and models[0].index > 0
