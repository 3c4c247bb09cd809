"""Option source_iq on the GPU (include/rtlfm_hip.h, "source_iq"): k_source_iq's records bit for bit against
tests/source_iq_model.py, and everything behind it - PCM, lengths, state records, levels, the sample counter - bit for bit
against a TWIN handle with the option off that is fed ``model.apply(bytes, coefficients of that run)``: on the boxcar, a
33-tap channel filter, the bank at K = 4 and a fifth_order configuration (RTLFM_ROUTE_CHAN_MIX), on both paths, with
coefficients that differ per source and change between runs; beside source_dc / source_stats / source_health, over the
source ring with a short last buffer, under verify_twice and pack_results 2; every refusal; and the loop with the engine.

Shapes: 512 bytes is the wave-per-buffer form, 7680 its upper edge, 8192 the workgroup form's lower edge, 16384 the
workgroup form with a remainder loop, 262144 the largest (sii passes 2^32 there); 1 and 3 sources, 1, 4 and 5 channels, runs
of 1, 3 and 17 buffers (the wave form packs four (source, buffer) pairs into a workgroup: 3 x 3 and 3 x 17 leave one
workgroup short)."""
import ctypes as C
import errno

import numpy as np
import pytest

import source_iq_model as model
from cases import case, make_cfg
from channel_common import assert_rows, demod, full_scale, make_steps, random_bank_taps, random_fir_taps, raw_cfg, run_once, to_device
from rtlsdr_amd import capi

pytestmark = pytest.mark.gpu

D = 10
LENGTHS = (512, 7680, 8192, 16384)
SHAPES = [(1, 1, 1), (3, 4, 3), (3, 5, 17), (1, 5, 3), (3, 1, 1), (1, 4, 17)]  # (sources, per_source, nblocks)
FRONTS = [("box", 0), ("box", 1), ("fir", 0), ("fir", 1), ("bank", 0), ("bank", 1), ("fifth", 0), ("fifth", 1)]
FRONT_IDS = [f"{f}-path{p}" for f, p in FRONTS]


def random_coef(nsrc, seed):
    """int16 [nsrc, 4] over the whole range, the extremes among them."""
    rng = np.random.default_rng(seed)
    c = rng.integers(-32768, 32768, size=(nsrc, 4)).astype(np.int16)
    c[0] = (32767, -32768, -32768, 32767)
    return c


def mild_coef(nsrc, seed):
    """Coefficients as the engine makes them - near the identity - different per source."""
    rng = np.random.default_rng(seed)
    c = np.zeros((nsrc, 4), dtype=np.int16)
    c[:, 0] = 16384 - rng.integers(0, 4000, size=nsrc)
    c[:, 1] = rng.integers(-300, 300, size=nsrc)
    c[:, 2] = rng.integers(-3000, 3000, size=nsrc)
    c[:, 3] = 16384 - rng.integers(0, 4000, size=nsrc)
    return c


def corrected(src, coef, L):
    """[nsrc, nb * L] raw bytes -> what k_source_iq leaves of them with coef [nsrc, 4]."""
    nsrc = src.shape[0]
    out, _ = model.apply(src.reshape(nsrc, -1, L), np.asarray(coef)[:, None, :])
    return out.reshape(nsrc, -1)


def want_sums(src, coef, L):
    nsrc = src.shape[0]
    return model.sums(src.reshape(nsrc, -1, L), np.asarray(coef)[:, None, :])


def assert_recs(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)[:4].tolist()
        raise AssertionError(f"{what}: records differ at {bad}: {[got[tuple(i)] for i in bad]} for {[want[tuple(i)] for i in bad]}")


def front_cfg(front, L, nb, **ov):
    if front == "fifth":
        return make_cfg(dict(case("p2_fir9")[0], **ov), L, nb)
    return raw_cfg(D, L, nb, report_levels=1, **ov)


def front_handle(front, path, cfg, nsrc, per=4, **options):
    g = demod(cfg, nsrc * per, **options)
    g.set_path(path)
    g.set_channels(per, steps=make_steps(nsrc * per, 5 + per))
    if front == "fir":
        g.set_channel_filter(*random_fir_taps(33, 19))
    if front == "bank":
        g.set_channel_bank(4, *random_bank_taps(4, 32, 17), bins=list(range(per)))
    return g


def everything(g, d, L, b0, nb):
    """One run and all it leaves: (PCM rows with their lengths, state records, channels_tell(), levels or None)."""
    rows, _ = run_once(g, d, L, b0, nb)
    levels = g.levels_all() if g.cfg.report_levels or g.cfg.squelch_level else None
    return rows, bytes(g.state_get_all()), g.channels_tell(), levels


def assert_same(a, b, what):
    assert_rows(a[0], b[0], what)
    assert a[1] == b[1], f"{what}: the state records differ"
    assert a[2] == b[2], (what, a[2], b[2])
    assert (a[3] is None and b[3] is None) or np.array_equal(a[3], b[3]), f"{what}: the levels differ"


# ------------------------------------------------------------ the records ----

@pytest.mark.parametrize("nsrc, per, nb", SHAPES, ids=[f"{s}x{p}x{n}" for s, p, n in SHAPES])
@pytest.mark.parametrize("L", LENGTHS)
def test_sums_and_rows_equal_the_model(L, nsrc, per, nb):
    """Random bytes, all 0 and all 255 with coefficients over the whole int16 range: the records (``clipped`` with them) are
    the model's, and the PCM is the twin's on the model's corrected bytes."""
    cfg = raw_cfg(D, L, nb)
    coef = random_coef(nsrc, L + nsrc)
    with front_handle("box", 0, cfg, nsrc, per, source_iq=1) as g, front_handle("box", 0, cfg, nsrc, per) as twin:
        g.set_source_iq(coef)
        assert np.array_equal(g.get_source_iq(), coef)
        for name, src in (("random", full_scale(nsrc, nb * L, L + nb)), ("zeros", np.zeros((nsrc, nb * L), np.uint8)),
                          ("255", np.full((nsrc, nb * L), 255, np.uint8))):
            g.reset()
            twin.reset()
            got = everything(g, to_device(src), L, 0, nb)
            assert_recs(g.source_iq_sums_all(), want_sums(src, coef, L), name)
            for a in range(nsrc):
                assert np.array_equal(g.source_iq_sums(a), g.source_iq_sums_all()[a]), (name, a)
            assert_same(got, everything(twin, to_device(corrected(src, coef, L)), L, 0, nb), name)


def test_sums_pass_2_to_the_32_at_the_longest_buffer():
    L = 262144
    cfg = raw_cfg(D, L, 1)
    with front_handle("box", 0, cfg, 1, 1, source_iq=1) as g:
        for name, src in (("255", np.full((1, L), 255, np.uint8)), ("random", full_scale(1, L, 3)), ("zeros", np.zeros((1, L), np.uint8))):
            run_once(g, to_device(src), L, 0, 1)
            got, want = g.source_iq_sums_all(), want_sums(src, [model.IDENTITY], L)
            assert_recs(got, want, name)
        assert int(want_sums(np.full((1, L), 255, np.uint8), [model.IDENTITY], L)["sii"][0, 0]) == 131072 * 65025 > 1 << 32


@pytest.mark.parametrize("L", [512, 16384])
def test_clipped_counts_the_bytes_the_clamp_changed(L):
    """Full-scale bytes with q = 20480 (1.25): every Q byte beyond +-102 of 127 is clamped, no I byte is."""
    nsrc, nb = 3, 3
    src = full_scale(nsrc, nb * L, 11)
    coef = np.tile(np.array([16384, 0, 0, 20480], dtype=np.int16), (nsrc, 1))
    with front_handle("box", 0, raw_cfg(D, L, nb), nsrc, 4, source_iq=1) as g:
        g.set_source_iq(coef)
        run_once(g, to_device(src), L, 0, nb)
        got = g.source_iq_sums_all()
    q = src.reshape(nsrc, nb, L)[..., 1::2].astype(np.int64) - 127
    want = ((((20480 * q + 8192) >> 14) + 127 > 255) | (((20480 * q + 8192) >> 14) + 127 < 0)).sum(axis=-1)
    assert np.array_equal(got["clipped"], want) and want.min() > 0
    assert_recs(got, want_sums(src, coef, L), "the whole record")


# ------------------------------------------------------------ the identity ----

@pytest.mark.parametrize("front, path", FRONTS, ids=FRONT_IDS)
def test_identity_changes_nothing(front, path):
    """The option on with the coefficients a fresh handle has: PCM, lengths, state records, channels_tell and levels equal
    the twin's with the option off, over two runs (the filter's and the bank's history goes through the handle's rows)."""
    nsrc, L, runs = 3, 2048, (3, 2)
    cfg = front_cfg(front, L, 3)
    src = full_scale(nsrc, sum(runs) * L, 23)
    with front_handle(front, path, cfg, nsrc, source_iq=1) as g, front_handle(front, path, cfg, nsrc) as twin:
        assert g.get_source_iq().tolist() == [list(model.IDENTITY)] * nsrc
        d, b0 = to_device(src), 0
        for nb in runs:
            a, b = everything(g, d, L, b0, nb), everything(twin, d, L, b0, nb)
            assert_same(a, b, f"{front} path {path} run at {b0}")
            assert g.get_option("last_route") == twin.get_option("last_route")
            if front == "fifth":
                assert g.get_option("last_route") == capi.ROUTE_CHAN_MIX
            assert_recs(g.source_iq_sums_all(), want_sums(src[:, b0 * L:(b0 + nb) * L], [model.IDENTITY] * nsrc, L), f"run at {b0}")
            b0 += nb


# ------------------------------------------------------------ general coefficients ----

@pytest.mark.parametrize("front, path", FRONTS, ids=FRONT_IDS)
def test_general_coefficients_equal_the_twin_on_corrected_bytes(front, path):
    """Three runs, coefficients different per source and changed between the runs (the second set over the whole int16
    range): the handle fed raw bytes equals the twin fed the model's corrected bytes - PCM, lengths, state records, levels.
    The filter's and the bank's history crosses both changes: it holds the bytes as they were consumed."""
    nsrc, L, runs = 3, 2048, (2, 3, 1)
    cfg = front_cfg(front, L, 3)
    src = full_scale(nsrc, sum(runs) * L, 29)
    coefs = [mild_coef(nsrc, 1), random_coef(nsrc, 2), mild_coef(nsrc, 3)]
    with front_handle(front, path, cfg, nsrc, source_iq=1) as g, front_handle(front, path, cfg, nsrc) as twin:
        d, b0 = to_device(src), 0
        for nb, coef in zip(runs, coefs):
            g.set_source_iq(coef)
            part = src[:, b0 * L:(b0 + nb) * L]
            a = everything(g, d, L, b0, nb)
            b = everything(twin, to_device(corrected(part, coef, L)), L, 0, nb)
            assert_same(a, b, f"{front} path {path} run at {b0}")
            assert_recs(g.source_iq_sums_all(), want_sums(part, coef, L), f"run at {b0}")
            assert np.array_equal(g.get_source_iq(), coef)
            b0 += nb


def test_queued_runs_keep_their_coefficients():
    """set_source_iq waits for nothing: five runs queued back to back, the coefficients changed in front of each (more
    changes than the setter has staging buffers), fetched only at the end - every run used the set that ruled when it was
    queued."""
    import torch
    nsrc, per, L, nb = 2, 2, 8192, 2
    cfg = raw_cfg(D, L, nb)
    src = full_scale(nsrc, 5 * nb * L, 31)
    coefs = [mild_coef(nsrc, 10 + k) for k in range(5)]
    with front_handle("box", 0, cfg, nsrc, per, source_iq=1) as g, front_handle("box", 0, cfg, nsrc, per) as twin:
        d, outs = to_device(src), []
        for k in range(5):
            g.set_source_iq(coefs[k])
            outs.append(g.run_torch(d[:, k * nb * L:(k + 1) * nb * L].contiguous()))
        torch.cuda.synchronize()
        g.sync()
        for k in range(5):
            o, n = outs[k][0].cpu().numpy(), outs[k][1].cpu().numpy()
            want, _ = run_once(twin, to_device(corrected(src[:, k * nb * L:(k + 1) * nb * L], coefs[k], L)), L, 0, nb)
            assert_rows([o[s, :n[s]] for s in range(nsrc * per)], want, f"run {k}")


# ------------------------------------------------------------ beside the other source options ----

@pytest.mark.parametrize("front, path", [("box", 0), ("box", 1), ("fir", 0), ("bank", 0)], ids=["box-path0", "box-path1", "fir", "bank"])
def test_dc_stats_and_health_beside_it(front, path):
    """source_dc, source_stats and source_health all on: the statistics and health records are those of the RAW bytes (a
    twin with the option off, fed raw), the DC averages (state records) and the PCM those of the corrected bytes (a twin fed
    corrected), over two runs with a change of coefficients."""
    nsrc, L, runs = 3, 2048, (3, 2)
    cfg = front_cfg(front, L, 3)
    src = full_scale(nsrc, sum(runs) * L, 37)
    on = dict(source_dc=1, source_stats=1, source_health=1)
    with front_handle(front, path, cfg, nsrc, source_iq=1, **on) as g, front_handle(front, path, cfg, nsrc, **on) as raw_twin, \
            front_handle(front, path, cfg, nsrc, **on) as twin:
        d, b0 = to_device(src), 0
        for k, nb in enumerate(runs):
            coef = mild_coef(nsrc, 40 + k) if k else random_coef(nsrc, 40)
            g.set_source_iq(coef)
            part = src[:, b0 * L:(b0 + nb) * L]
            a = everything(g, d, L, b0, nb)
            everything(raw_twin, d, L, b0, nb)
            b = everything(twin, to_device(corrected(part, coef, L)), L, 0, nb)
            assert_same(a, b, f"{front} path {path} run at {b0}")
            assert_recs(g.source_stats_all(), raw_twin.source_stats_all(), "statistics of the raw bytes")
            assert_recs(g.source_health_all(), raw_twin.source_health_all(), "health of the raw bytes")
            assert not np.array_equal(g.source_stats_all(), twin.source_stats_all())  # (the corrected bytes' differ)
            assert_recs(g.source_iq_sums_all(), want_sums(part, coef, L), f"run at {b0}")
            b0 += nb


# ------------------------------------------------------------ the ring, verify_twice, packed results ----

def push_run(g, src, pieces):
    for i in range(src.shape[0]):
        for at, n in pieces:
            g.rtlsdr_callback(src[i, at:at + n], stream=i)


def fetch_rows(g, prev=False):
    o, n = g.fetch_all_prev() if prev else g.fetch_all()
    return [o[s, :n[s]].copy() for s in range(g.nstreams)]


@pytest.mark.parametrize("front", ["box", "fir", "bank"])
def test_source_ring_with_a_short_last_buffer_and_prev(front):
    """push -> run -> fetch over the source ring: a run whose last buffer is short (every buffer's record over its own
    length), a run of whole buffers behind it with other coefficients, and the first run again through _prev."""
    nsrc, L = 3, 8192
    run_a = [(0, L), (L, L), (2 * L, 1536)]
    run_b = [(3 * L, L), (4 * L, L)]
    src = full_scale(nsrc, 5 * L, 41)
    ca, cb = mild_coef(nsrc, 50), random_coef(nsrc, 51)
    cfg = front_cfg(front, L, 3)

    def fixed(pieces, coef):
        out = src.copy()
        for at, n in pieces:
            out[:, at:at + n] = corrected(src[:, at:at + n], coef, n)
        return out
    with front_handle(front, 0, cfg, nsrc, source_ring=1, source_iq=1) as g, front_handle(front, 0, cfg, nsrc, source_ring=1) as twin:
        g.set_source_iq(ca)
        push_run(g, src, run_a)
        push_run(twin, fixed(run_a, ca), run_a)
        g.full_demod()
        twin.full_demod()
        first = fetch_rows(twin)
        assert_rows(fetch_rows(g), first, f"{front}: the run with the short buffer")
        want = np.stack([want_sums(src[:, at:at + n], ca, n)[:, 0] for at, n in run_a], axis=1)
        assert_recs(g.source_iq_sums_all(), want, "each record over its own length")
        g.set_source_iq(cb)
        push_run(g, src, run_b)
        push_run(twin, fixed(run_b, cb), run_b)
        g.full_demod()
        twin.full_demod()
        assert_rows(fetch_rows(g, prev=True), first, f"{front}: the same through _prev")
        assert_rows(fetch_rows(g), fetch_rows(twin), f"{front}: the run behind it")
        assert_recs(g.source_iq_sums_all(), want_sums(src[:, 3 * L:], cb, L), "the run behind it")
        assert bytes(g.state_get_all()) == bytes(twin.state_get_all()) and g.channels_tell() == twin.channels_tell()


@pytest.mark.parametrize("front, path", [("box", 0), ("box", 1), ("fir", 0), ("bank", 1)], ids=["box-path0", "box-path1", "fir", "bank-path1"])
def test_verify_twice_sees_no_difference(front, path):
    nsrc, L, nb = 3, 2048, 3
    cfg = front_cfg(front, L, nb)
    src = full_scale(nsrc, 2 * nb * L, 43)
    with front_handle(front, path, cfg, nsrc, source_iq=1, verify_twice=1) as g, front_handle(front, path, cfg, nsrc) as twin:
        d = to_device(src)
        for k in range(2):
            coef = random_coef(nsrc, 60 + k)
            g.set_source_iq(coef)
            part = src[:, k * nb * L:(k + 1) * nb * L]
            a = everything(g, d, L, k * nb, nb)
            assert_same(a, everything(twin, to_device(corrected(part, coef, L)), L, 0, nb), f"run {k}")
            assert_recs(g.source_iq_sums_all(), want_sums(part, coef, L), f"run {k}")
        assert g.get_option("verify_runs") == 2 and g.get_option("verify_mismatches") == 0


def test_pack_results_2_on_top():
    """-M fm with a squelch over the source ring with pack_results 2: the packed rows and their index are the twin's."""
    nsrc, per, L, runs = 2, 2, 2048, (1, 3)
    cfg = make_cfg(dict(case("c1_boxcar10_fast")[0], squelch_level=30), L, 3)
    src = full_scale(nsrc, sum(runs) * L, 47)
    src[1] = 127 + (src[1] % 3)  # a quiet source: its channels are held back
    coef = mild_coef(nsrc, 70)
    with front_handle("box", 0, cfg, nsrc, per, source_ring=1, pack_results=2, source_iq=1) as g, \
            front_handle("box", 0, cfg, nsrc, per, source_ring=1, pack_results=2) as twin:
        g.set_source_iq(coef)
        b0 = 0
        for nb in runs:
            pieces = [((b0 + j) * L, L) for j in range(nb)]
            push_run(g, src, pieces)
            push_run(twin, corrected(src, coef, L), pieces)
            g.full_demod()
            twin.full_demod()
            (pa, ia), (pb, ib) = g.fetch_packed(), twin.fetch_packed()
            assert np.array_equal(ia, ib) and np.array_equal(pa, pb), b0
            b0 += nb


# ------------------------------------------------------------ the contract ----

def sums_codes(g, source=0, cap=8):
    out = np.zeros(64 * cap * 48, dtype=np.uint8)
    codes = []
    for one in (True, False):
        n = C.c_int(-1)
        r = (g.lib.rtlfm_gpu_source_iq_sums(g._h, source, out.ctypes.data, cap, C.byref(n)) if one
             else g.lib.rtlfm_gpu_source_iq_sums_all(g._h, out.ctypes.data, cap, C.byref(n)))
        codes.append((r, n.value))
    return codes


def test_contract():
    """Every refusal and every -ENODATA case, each followed by a run that still equals the model."""
    nsrc, per, L, nb = 3, 2, 2048, 3
    S = nsrc * per
    src = full_scale(S, nb * L, 53)
    cfg = raw_cfg(D, L, nb)
    lib = capi.load()
    coef = mild_coef(S, 80)
    buf = np.zeros(S * 4, dtype=np.int16)
    with front_handle("box", 0, cfg, nsrc, per, source_ring=1) as g, demod(cfg, S) as plain:
        d = to_device(src)

        def run_equals_model(rows, c, what):
            g.reset()  # (the sample counter and the records back to the start: the coefficients and the options stay)
            got, _ = run_once(g, d[:rows], L, 0, nb)
            plain.set_channels(S // rows, steps=make_steps(S, 5 + per))
            plain.reset()
            want, _ = run_once(plain, to_device(corrected(src[:rows], c[:rows], L)), L, 0, nb)
            assert_rows(got, want, what)
            if g.get_option("source_iq"):
                assert_recs(g.source_iq_sums_all(), want_sums(src[:rows], c[:rows], L), what)
        ident = np.tile(np.array(model.IDENTITY, dtype=np.int16), (S, 1))
        # -ENODATA: the option off (the coefficients may be set all the same and rule once it is on); on, before the first run
        g.set_source_iq(coef[:nsrc])
        run_equals_model(nsrc, ident, "option off: the coefficients act on nothing")
        assert [c for c, _ in sums_codes(g)] == [-errno.ENODATA] * 2
        g.set_option("source_iq", 1)
        assert [c for c, _ in sums_codes(g)] == [-errno.ENODATA] * 2
        run_equals_model(nsrc, coef, "option on")
        assert sums_codes(g) == [(0, nb)] * 2
        # -ENOBUFS with *n written; -EINVAL for a source outside [0, sources) and for null pointers
        assert sums_codes(g, cap=nb - 1) == [(-errno.ENOBUFS, nb)] * 2
        for bad in (-1, nsrc):
            assert sums_codes(g, source=bad)[0][0] == -errno.EINVAL
        n = C.c_int()
        assert lib.rtlfm_gpu_source_iq_sums(g._h, 0, None, 8, C.byref(n)) == -errno.EINVAL
        assert lib.rtlfm_gpu_source_iq_sums_all(g._h, np.zeros(4096, np.uint8).ctypes.data, 8, None) == -errno.EINVAL
        # the option: -EINVAL for any value but 0 / 1; the coefficients: -EINVAL for NULL, -ENOBUFS for a short buffer
        for v in (2, -1):
            assert lib.rtlfm_gpu_set_option(g._h, b"source_iq", v) == -errno.EINVAL
        assert lib.rtlfm_gpu_set_source_iq(g._h, None) == -errno.EINVAL
        assert lib.rtlfm_gpu_get_source_iq(g._h, None, 64) == -errno.EINVAL
        assert lib.rtlfm_gpu_get_source_iq(g._h, buf.ctypes.data, nsrc * 4 - 1) == -errno.ENOBUFS
        assert g.get_option("source_iq") == 1 and np.array_equal(g.get_source_iq(), coef[:nsrc])
        run_equals_model(nsrc, coef, "behind the refused calls")
        # -EBUSY inside run_begin / run_end, for the option and the coefficients, and for the option while buffers are queued
        push_run(g, src[:nsrc], [(0, L)])
        assert lib.rtlfm_gpu_set_option(g._h, b"source_iq", 0) == -errno.EBUSY  # (source_ring: buffers are queued)
        assert g.run_begin() == 1
        assert lib.rtlfm_gpu_set_option(g._h, b"source_iq", 0) == -errno.EBUSY
        assert lib.rtlfm_gpu_set_source_iq(g._h, ident.ctypes.data) == -errno.EBUSY
        g.run_end()
        assert g.get_option("source_iq") == 1 and np.array_equal(g.get_source_iq(), coef[:nsrc])
        assert_recs(g.source_iq_sums_all(), want_sums(src[:nsrc, :L], coef[:nsrc], L), "the ring's run behind -EBUSY")
        # set_channels resets every source to the identity and leaves no records; more sources than before: the rows regrow
        for per_now in (1, per):
            g.set_channels(per_now, steps=make_steps(S, 5 + per))
            rows = S // per_now
            assert [c for c, _ in sums_codes(g)] == [-errno.ENODATA] * 2
            assert np.array_equal(g.get_source_iq(), ident[:rows])
            run_equals_model(rows, ident, f"{rows} sources: the identity")
            g.set_source_iq(coef[:rows])
            run_equals_model(rows, coef, f"{rows} sources")
            assert sums_codes(g, source=rows)[0][0] == -errno.EINVAL
        # channels off: -ENOTSUP for the coefficients, -ENODATA after a run; the option stays set and acts again later
        g.set_channels(0)
        assert lib.rtlfm_gpu_set_source_iq(g._h, ident.ctypes.data) == -errno.ENOTSUP
        assert lib.rtlfm_gpu_get_source_iq(g._h, buf.ctypes.data, buf.size) == -errno.ENOTSUP
        run_once(g, d, L, 0, nb)
        assert [c for c, _ in sums_codes(g)] == [-errno.ENODATA] * 2
        assert g.get_option("source_iq") == 1
        g.set_channels(per, steps=make_steps(S, 5 + per))
        g.set_source_iq(coef[:nsrc])
        run_equals_model(nsrc, coef, "channels back on")
        # back to 0: the rows and records go, the coefficients stay, nothing is corrected; on again: they rule again
        g.set_option("source_iq", 0)
        assert [c for c, _ in sums_codes(g)] == [-errno.ENODATA] * 2
        run_equals_model(nsrc, ident, "option back to 0")
        g.set_option("source_iq", 1)
        assert np.array_equal(g.get_source_iq(), coef[:nsrc])
        run_equals_model(nsrc, coef, "option on again")
    # the option may be set with channels off and acts on nothing there
    with demod(cfg, S, source_iq=1) as g, demod(cfg, S) as twin:
        a, _ = run_once(g, to_device(src), L, 0, nb)
        b, _ = run_once(twin, to_device(src), L, 0, nb)
        assert_rows(a, b, "channels off")
        assert [c for c, _ in sums_codes(g)] == [-errno.ENODATA] * 2


def test_switching_does_not_clear_the_history():
    """A filter's history crosses the option being switched on and off: the twin never switches and sees the same bytes."""
    nsrc, L = 2, 2048
    cfg = front_cfg("fir", L, 1)
    src = full_scale(nsrc, 3 * L, 59)
    with front_handle("fir", 0, cfg, nsrc) as g, front_handle("fir", 0, cfg, nsrc) as twin:
        d = to_device(src)
        for k in range(3):
            g.set_option("source_iq", k % 2)
            assert_same(everything(g, d, L, k, 1), everything(twin, d, L, k, 1), f"run {k}")


def test_option_at_0_leaves_the_launch_count_alone():
    """rtlfm_gpu_timing_read's count for a channel run: the option never touched, and set and put back."""
    nsrc, per, L, nb = 2, 2, 2048, 2
    src = full_scale(nsrc, nb * L, 61)
    counts = {}
    for kind in ("never", "back"):
        with front_handle("box", 0, raw_cfg(D, L, nb), nsrc, per) as g:
            if kind == "back":
                g.set_option("source_iq", 1)
                run_once(g, to_device(src), L, 0, nb)
                g.set_option("source_iq", 0)
                g.reset()
            g.timing_enable(True)
            g.timing_read()
            run_once(g, to_device(src), L, 0, nb)
            counts[kind] = g.timing_read()[1]
    assert counts["never"] == counts["back"], counts


# ------------------------------------------------------------ end to end ----

def test_engine_loop_end_to_end(capsys):
    """The image-test signal (tests/test_source_iq_cpu.py) through two -M raw boxcar channels at +-37/256 fs: run 1 measures,
    the engine decides, run 2 is corrected with its coefficients - and equals the twin's on the model's bytes bit for bit.
    The power ratio of the two channels (wanted over mirror) goes into the log."""
    from rtlsdr_amd.iq import IqBalance
    L, nb = 16384, 4
    n = nb * L // 2
    buf = model.image_signal(n=2 * n, g=0.8, phi_deg=10.0, seed=5).reshape(1, -1)
    step = round(37 / 256 * (1 << 32))
    steps = [step, (1 << 32) - step]
    cfg = raw_cfg(32, L, nb)

    def handle(**options):
        g = demod(cfg, 2, **options)
        g.set_channels(2, steps=steps)
        return g

    def ratio_db(rows):
        p = [float((r.astype(np.float64) ** 2).sum()) for r in rows]
        return 10.0 * np.log10(max(p) / min(p))
    with handle(source_iq=1) as g, handle() as twin, IqBalance(1, window=nb) as e:
        d = to_device(buf)
        first, _ = run_once(g, d, L, 0, nb)
        e.update(g)
        ev = e.poll()
        t = model.total_of(model.sums(buf[:, :nb * L].reshape(1, nb, L)))
        want = model.compute(t)[1]
        assert len(ev) == 1 and ev[0]["kind"] == capi.IQ_EVENT_CHANGED and ev[0]["coef"] == want, (ev, want)
        g.set_source_iq(e.coeffs())
        second, _ = run_once(g, d, L, nb, nb)
        run_once(twin, d, L, 0, nb)
        wanted, _ = run_once(twin, to_device(corrected(buf[:, nb * L:], e.coeffs(), L)), L, 0, nb)
        assert_rows(second, wanted, "run 2 with the engine's coefficients")
        before, after = ratio_db(first), ratio_db(second)
        with capsys.disabled():
            print(f"\nsource_iq end to end: coefficients {want}, channel power ratio {before:.1f} dB -> {after:.1f} dB")
        assert after > before  # (the bound on the image is the CPU test's; this is the log's sanity)
