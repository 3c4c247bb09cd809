"""Channels on the GPU: K channels per wideband source through the NCO front end (include/rtlfm_hip.h,
rtlfm_gpu_set_channels; csrc/channel_kernel.h) against tests/channel_model.py, which hands the mixed samples to the
existing oracle.  Equality everywhere; only -M fm with -A std gets the project's stated tolerance (<= 1 LSB on <= 1e-4 of
the samples: the fp64 atan2).

Inputs for model_via_oracle keep |I - 127|, |Q - 127| <= 89, so that the mixed samples fit the bytes the oracle reads
(89 sqrt(2) (1 + 2^-14) + 1/2 < 127; the model asserts it).  Full-scale inputs go through model_raw_boxcar in -M raw.

The general-step test meets every number of sources, channels per source and block length the feature was specified
with, and every boxcar x mode configuration on both paths; the configurations go round the shapes, three per shape, so
that the suite stays quick - every configuration meets at least three shapes, not all twenty-four.

(box1000_std_squelch has no case at block_len 512: a boxcar longer than the buffer is outside the reference's domain,
and rtlfm_gpu_create says -EDOM.)"""
import ctypes as C
import errno
import functools

import numpy as np
import pytest

import channel_model as cm
from cases import case, make_cfg
from channel_common import assert_row_cfg as assert_rows
from channel_common import bounded, demod
from channel_common import make_steps_special as make_steps
from channel_common import run_gpu_levels as run_gpu
from rtlsdr_amd import synth
from rtlsdr_amd.capi import ATAN_FAST, ATAN_LUT, MODE_AM, MODE_FM, MODE_RAW, MODE_USB

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

Q = 1 << 30
BOUND = 89


def bounded_bytes(rows, nbytes, seed):
    return bounded(rows, nbytes, seed, BOUND)


# ---------------------------------------------------------------- 1. the anchor ----

ANCHOR = ["c1_boxcar10_fast", "box7_std_lpr", "raw_box1", "usb_box8", "box256_std", "box1000_std_squelch", "box84_am_dc",
          "wbfm_preset", "c2_p4_lut", "p2_fir9", "p4_squelch"]
ANCHOR_PARAMS = [(n, L) for n in ANCHOR for L in (512, 16384)
                 if not (case(n)[0].get("downsample_passes", 0) == 0 and case(n)[0]["downsample"] > L // 2)]


@pytest.mark.parametrize("name,L", ANCHOR_PARAMS)
def test_anchor_quarter_rate_and_zero_are_todays_paths(name, L):
    """per_source = 1 with every step 2^30 is the handle with channels off, and step 0 the handle with offset_tuning:
    PCM, lengths and the state records, on full-scale bytes, over two runs of 2 and 3 buffers."""
    S, runs = 3, (2, 3)
    ov, _ = case(name)
    cfg = make_cfg(ov, L, 3)
    src = synth.random_u8(S, 5 * L, seed=len(name) * 1000 + L)
    for step, off in ((Q, 0), (0, 1)):
        with demod(cfg, S) as g:
            g.set_channels(1, steps=[step] * S)
            got, _, paths = run_gpu(g, src, L, runs)
            got_st = bytes(g.state_get_all())
            assert g.channels_tell() == 5 * L // 2
        assert paths == [2 if cfg.downsample_passes == 0 else 1] * 2, paths
        plain = cm.copy_cfg(cfg, offset_tuning=off)
        with demod(plain, S) as g:
            want, _, _ = run_gpu(g, src, L, runs)
            want_st = bytes(g.state_get_all())
        for s in range(S):
            assert_rows(got[s], want[s], cfg, f"{name} L={L} step={step} stream {s}")
        assert got_st == want_st, (name, L, step)


# ------------------------------------------------- 2. general steps, the model ----

BOX_D = (1, 7, 10, 256, 1000)
BOX_MODES = {
    "fmfast": dict(mode=MODE_FM, custom_atan=ATAN_FAST),
    "am": dict(mode=MODE_AM, output_scale=3),
    "usb": dict(mode=MODE_USB, output_scale=2),
    "raw": dict(mode=MODE_RAW),
}
BOX_CFGS = [(f"box{D}_{m}", dict(BOX_MODES[m], downsample=D)) for D in BOX_D for m in BOX_MODES]
BOX_CFGS += [("box10_fmfast_squelch", dict(mode=MODE_FM, custom_atan=ATAN_FAST, downsample=10, squelch_level=50)),
             ("box7_raw_squelch", dict(mode=MODE_RAW, downsample=7, squelch_level=50))]
STAGED_CFGS = [("p3_lut", dict(case("p3_lut")[0], custom_atan=ATAN_LUT)),
               ("c2_p4_fir9_lut", dict(case("c2_p4_fir9_std")[0], custom_atan=ATAN_LUT))]
GEOMS = [(nsrc, per, L) for nsrc in (1, 3) for per in (1, 4, 5, 67) for L in (512, 16384, 16896)]
RUNS = (1, 3, 2)  # 1, cap and 2 buffers: the boxcar's state and pos are carried twice


def general_params():
    out = []
    for gi, (nsrc, per, L) in enumerate(GEOMS):
        ok = [c for c in BOX_CFGS if c[1]["downsample"] <= L // 2]
        for j in range(3):  # three configurations per shape, in rotation: every one of them meets several shapes
            name, ov = ok[(gi * 3 + j) % len(ok)]
            out.append(pytest.param(gi, name, id=f"{nsrc}x{per}_L{L}_{name}"))
    big = len(GEOMS)  # 262144 once, 1 source x 5
    out.append(pytest.param(big, "box10_fmfast", id="1x5_L262144_box10_fmfast"))
    for gi in (4, 20, 9):
        for name, _ in STAGED_CFGS:
            nsrc, per, L = GEOMS[gi]
            out.append(pytest.param(gi, name, id=f"{nsrc}x{per}_L{L}_{name}"))
    return out


@functools.lru_cache(maxsize=2)
def geometry(gi):
    """(nsrc, per, L, source bytes, steps) of shape gi: bounded random bytes, or an FM signal at an amplitude that keeps
    the bound; in both, buffer 1 of every source is silent, for the squelch."""
    nsrc, per, L = GEOMS[gi] if gi < len(GEOMS) else (1, 5, 262144)
    nbuf = sum(RUNS)
    if gi % 2:
        src = synth.fm_iq_u8(nsrc, nbuf * L // 2, fs=2.4e6, dev_hz=50e3, amplitude=84.0, seed=900 + gi)
    else:
        src = bounded_bytes(nsrc, nbuf * L, 100 + gi)
    src[:, L:2 * L] = 127
    assert np.abs(src.astype(np.int32) - 127).max() <= BOUND
    return nsrc, per, L, src, make_steps(nsrc * per, gi)


@pytest.mark.parametrize("gi,name", general_params())
def test_general_steps_equal_the_model(oracle_lib, gi, name):
    nsrc, per, L, src, steps = geometry(gi)
    S = nsrc * per
    ov = dict(BOX_CFGS + STAGED_CFGS)[name]
    cfg = make_cfg(ov, L, max(RUNS))
    boxed = cfg.downsample_passes == 0
    want, want_len, want_st = cm.model_via_oracle(cfg, src, steps, per, 0)
    want_lv = cm.model_levels(cfg, src, steps, per, 0) if cfg.squelch_level else None
    got = {}
    for path in ((0, 1) if boxed else (1,)):
        with demod(cfg, S) as g:
            g.set_path(path)
            g.set_channels(per, steps=steps)
            rows, lv, paths = run_gpu(g, src, L, RUNS, levels=bool(cfg.squelch_level))
            st = g.state_get_all()
            assert g.channels_tell() == sum(RUNS) * L // 2
        assert paths == [2 if path == 0 else 1] * len(RUNS), (path, paths)
        for s in range(S):
            assert_rows(rows[s], want[s, :want_len[s]], cfg, f"{name} path {path} stream {s} step {steps[s]}")
            assert st[s].as_dict() == want_st[s].as_dict(), (name, path, s)
        if want_lv is not None:
            assert np.array_equal(lv, want_lv), (name, path)
        got[path] = rows
    if boxed:
        for s in range(S):
            assert np.array_equal(got[0][s], got[1][s]), (name, s)


def test_segments_with_a_warm_up_tile_equal_one_segment(oracle_lib):
    """The same run cut into segments of one and of two 8 KiB tiles (each but a stream's first re-runs the tile in front
    of it) and as a single segment: the boxcar that does not divide a tile, and the longest one a warm-up tile covers."""
    nsrc, per, L = 2, 5, 16896
    src = bounded_bytes(nsrc, 6 * L, 77)
    steps = make_steps(nsrc * per, 3)
    for D in (7, 1000, 4096):
        cfg = make_cfg(dict(mode=MODE_RAW, downsample=D), L, 3)
        want, want_len, want_st = cm.model_via_oracle(cfg, src, steps, per, 0)
        for tps in (1, 2, 0):
            with demod(cfg, nsrc * per, fused_tiles_per_seg=tps) as g:
                g.set_channels(per, steps=steps)
                rows, _, paths = run_gpu(g, src, L, RUNS)
                st = g.state_get_all()
            assert paths == [2] * 3
            for s in range(nsrc * per):
                assert np.array_equal(rows[s], want[s, :want_len[s]]), (D, tps, s)
                assert st[s].as_dict() == want_st[s].as_dict(), (D, tps, s)


# ---------------------------------------------------------------- 3. full scale ----

@pytest.mark.parametrize("D", [1, 10, 256])
def test_full_scale_raw_equals_the_boxcar_model(D):
    """Bytes from {0, 255} and random ones: |I'|, |Q'| reach 182, the sums wrap as the reference's int16 stores do."""
    nsrc, per, L = 2, 5, 16896
    rng = np.random.default_rng(D)
    src = rng.integers(0, 256, size=(nsrc, 6 * L), dtype=np.uint8)
    src[0] = rng.integers(0, 2, size=6 * L).astype(np.uint8) * 255
    steps = make_steps(nsrc * per, 11 + D)
    cfg = make_cfg(dict(mode=MODE_RAW, downsample=D), L, 3)
    want, state, b0 = [[] for _ in range(nsrc * per)], None, 0
    for nb in RUNS:
        rows, state = cm.model_raw_boxcar(src[:, b0 * L:(b0 + nb) * L], steps, D, state, per_source=per, pos=b0 * L // 2)
        for s, r in enumerate(rows):
            want[s].append(r)
        b0 += nb
    for path in (0, 1):
        with demod(cfg, nsrc * per) as g:
            g.set_path(path)
            g.set_channels(per, steps=steps)
            got, _, paths = run_gpu(g, src, L, RUNS)
            st = g.state_get_all()
        assert paths == [2 if path == 0 else 1] * 3
        for s in range(nsrc * per):
            assert np.array_equal(got[s], np.concatenate(want[s])), (D, path, s)
            assert {k: getattr(st[s], k) for k in ("now_r", "now_j", "prev_index")} == state[s], (D, path, s)


# ------------------------------------------------------------------ 4. pos wraps ----

@pytest.mark.parametrize("path", [0, 1])
def test_pos_wraps_at_two_to_the_32(oracle_lib, path):
    nsrc, per, L, nb = 2, 4, 16384, 2
    pos = (1 << 32) - 1000
    cfg = make_cfg(case("c1_boxcar10_fast")[0], L, nb)
    src = bounded_bytes(nsrc, nb * L, 5)
    steps = make_steps(nsrc * per, 21)
    want, want_len, _ = cm.model_via_oracle(cfg, src, steps, per, pos)
    with demod(cfg, nsrc * per) as g:
        g.set_path(path)
        g.set_channels(per, steps=steps)
        g.channels_seek(pos)
        assert g.channels_tell() == pos
        got, _, _ = run_gpu(g, src, L, (nb,))
        assert g.channels_tell() == pos + nb * L // 2  # the counter itself is 64 bits wide
        g.reset()
        assert g.channels_tell() == 0
    for s in range(nsrc * per):
        assert np.array_equal(got[s], want[s, :want_len[s]]), s


@pytest.mark.parametrize("path", [0, 1])
def test_verify_twice_runs_both_executions_at_one_pos(oracle_lib, path):
    """Under the debugging option verify_twice a run is executed twice: both at the same pos, which moves on once."""
    nsrc, per, L = 1, 4, 4096
    cfg = make_cfg(case("c1_boxcar10_fast")[0], L, 2)
    src = bounded_bytes(nsrc, 4 * L, 12)
    steps = make_steps(nsrc * per, 9)
    want, want_len, _ = cm.model_via_oracle(cfg, src, steps, per, 0)
    with demod(cfg, nsrc * per, verify_twice=1) as g:
        g.set_path(path)
        g.set_channels(per, steps=steps)
        got, _, _ = run_gpu(g, src, L, (2, 2))
        assert g.channels_tell() == 4 * L // 2
        assert g.get_option("verify_runs") == 2 and g.get_option("verify_mismatches") == 0
    for s in range(nsrc * per):
        assert np.array_equal(got[s], want[s, :want_len[s]]), s


# -------------------------------------------------------------------- 5. it tunes ----

def strongest_hz(pcm, rate):
    x = pcm.astype(np.float64)
    spec = np.abs(np.fft.rfft((x - x.mean()) * np.hanning(x.size)))
    return np.argmax(spec) * rate / x.size


def test_two_carriers_of_one_source_come_out_as_two_channels():
    """One source carries FM carriers at +200 kHz and -300 kHz from its centre, modulated with 2 kHz and 5 kHz.  Two
    channels with shifts_hz = channel_freq - capture_freq through the API, /10, -A fast: each demodulates its own tone;
    with the signs of the shifts swapped neither does."""
    fs, L, nb = 2_400_000, 16384, 4
    offs, tones = (200_000, -300_000), (2000.0, 5000.0)
    n = np.arange(nb * L // 2, dtype=np.float64)
    sig = np.zeros(n.size, dtype=np.complex128)
    for f, tone in zip(offs, tones):
        sig += 40.0 * np.exp(1j * (2 * np.pi * f * n / fs + (30e3 / tone) * np.sin(2 * np.pi * tone * n / fs)))
    src = np.empty((1, nb * L), dtype=np.uint8)
    src[0, 0::2] = np.rint(127 + sig.real).astype(np.uint8)
    src[0, 1::2] = np.rint(127 + sig.imag).astype(np.uint8)
    assert np.abs(src.astype(np.int32) - 127).max() <= BOUND
    cfg = make_cfg(case("c1_boxcar10_fast")[0], L, nb)

    def heard(shifts):
        with demod(cfg, 2) as g:
            g.set_channels(2, shifts_hz=shifts, capture_rate=fs)
            rows, _, _ = run_gpu(g, src, L, (nb,))
        return [strongest_hz(r, fs / 10) for r in rows]
    res = 2 * (fs / 10) / (nb * L // 2 // 10)  # two bins of the spectrum
    got = heard(offs)
    assert abs(got[0] - tones[0]) <= res and abs(got[1] - tones[1]) <= res, got
    swapped = heard([-f for f in offs])
    assert abs(swapped[0] - tones[0]) > res and abs(swapped[1] - tones[1]) > res, swapped


# ------------------------------------------------------------------ 6. refusals ----

def test_refusals_change_nothing(oracle_lib, tmp_path):
    """Everything on the -ENOTSUP list while channels are on, each followed by a run that still equals the model."""
    nsrc, per, L = 1, 2, 2048
    S = nsrc * per
    cfg = make_cfg(dict(case("c1_boxcar10_fast")[0], squelch_level=1), L, 1)
    steps = [12345678, (1 << 32) - 987654321]
    NREF = 13  # entries of the list below: one buffer is run behind each
    src = bounded_bytes(nsrc, NREF * L, 31)
    want, want_len, _ = cm.model_via_oracle(cfg, src, steps, per, 0)
    snap = str(tmp_path / "chan.snap")
    buf = np.full(L, 127, dtype=np.uint8)
    with demod(cfg, S) as g, demod(cfg, S) as other:
        lib, h = g.lib, g._h
        other.save(snap)
        g.set_channels(per, steps=steps)
        p, cap, taken = C.c_void_p(), C.c_uint32(), C.c_int()
        refused = [
            ("push", lambda: lib.rtlfm_gpu_push(h, 0, buf.ctypes.data, L)),
            ("acquire", lambda: lib.rtlfm_gpu_acquire(h, 0, C.byref(p), C.byref(cap))),
            ("commit", lambda: lib.rtlfm_gpu_commit(h, 0, L)),
            ("run", lambda: lib.rtlfm_gpu_run(h)),
            ("run_begin", lambda: lib.rtlfm_gpu_run_begin(h, C.byref(taken))),
            ("input_stats", lambda: lib.rtlfm_gpu_set_option(h, b"input_stats", 1)),
            ("input_health", lambda: lib.rtlfm_gpu_set_option(h, b"input_health", 1)),
            ("squelch_gate", lambda: lib.rtlfm_gpu_set_option(h, b"squelch_gate", 1)),
            ("mute", lambda: lib.rtlfm_gpu_mute(h, 1, 4096)),
            ("save", lambda: lib.rtlfm_gpu_save(h, str(tmp_path / "no.snap").encode())),
            ("load", lambda: lib.rtlfm_gpu_load(h, snap.encode())),
            ("state_move into", lambda: lib.rtlfm_gpu_state_move(h, other._h, (C.c_int32 * S)(0, 1), S)),
            ("state_move out of", lambda: lib.rtlfm_gpu_state_move(other._h, h, (C.c_int32 * S)(0, 1), S)),
        ]
        d = torch.from_numpy(src).cuda()
        got = [[] for _ in range(S)]
        for b, (what, call) in enumerate(refused):
            assert call() == -errno.ENOTSUP, what
            assert g.channels_tell() == b * L // 2, what
            o, n = g.run_torch(d[:, b * L:(b + 1) * L].contiguous())
            g.sync()
            o, n = o.cpu().numpy(), n.cpu().numpy()
            for s in range(S):
                got[s].append(o[s, :n[s]].copy())
        assert not (tmp_path / "no.snap").exists()
        for name in ("input_stats", "input_health", "squelch_gate"):
            assert g.get_option(name) == 0
        assert len(refused) == NREF
        for s in range(S):
            assert np.array_equal(np.concatenate(got[s]), want[s, :want_len[s]]), s


def test_refusals_of_set_channels_and_of_the_fused_path(oracle_lib):
    L = 2048
    # cfg.dc_block_raw, and the options that read per-stream rows: set_channels itself says no, the handle stays as it was
    src = bounded_bytes(2, 2 * L, 8)
    for ov, opts in ((dict(case("c1_boxcar10_fast")[0], dc_block_raw=1), {}),
                     (case("c1_boxcar10_fast")[0], dict(input_stats=1)),
                     (case("c1_boxcar10_fast")[0], dict(input_health=1)),
                     (dict(case("c1_boxcar10_fast")[0], squelch_level=1), dict(squelch_gate=1))):
        cfg = make_cfg(ov, L, 2)
        with demod(cfg, 2, **opts) as g:
            steps = (C.c_uint32 * 2)(1, 2)
            assert g.lib.rtlfm_gpu_set_channels(g._h, 1, steps) == -errno.ENOTSUP, (ov, opts)
            assert g.lib.rtlfm_gpu_set_channels(g._h, 2, steps) == -errno.ENOTSUP
            got, _, _ = run_gpu(g, src, L, (2,))  # two rows: channels are off
        want, want_len, _ = oracle_lib.run_batch(cfg, src)
        for s in range(2):
            assert np.array_equal(got[s], want[s, :want_len[s]]), (ov, opts, s)
    # bad arguments
    cfg = make_cfg(case("c1_boxcar10_fast")[0], L, 2)
    with demod(cfg, 6) as g:
        steps = (C.c_uint32 * 6)()
        assert g.lib.rtlfm_gpu_set_channels(g._h, 4, steps) == -errno.EINVAL  # 4 does not divide 6
        assert g.lib.rtlfm_gpu_set_channels(g._h, -1, steps) == -errno.EINVAL
        assert g.lib.rtlfm_gpu_set_channels(g._h, 3, None) == -errno.EINVAL
        assert g.lib.rtlfm_gpu_set_channels(g._h, 0, None) == 0
    # path 2 with fifth_order passes has no fused channel front end: -ENOTSUP at the run, pos and state stay
    cfg = make_cfg(case("p2_fir9")[0], L, 2)
    steps = [7 << 20, 3 << 29, 1, 0]
    src = bounded_bytes(2, 2 * L, 9)
    want, want_len, _ = cm.model_via_oracle(cfg, src, steps, 2, 0)
    with demod(cfg, 4) as g:
        g.set_channels(2, steps=steps)
        g.set_path(2)
        d = torch.from_numpy(src).cuda()
        out = torch.empty((4, g.result_cap(2)), dtype=torch.int16, device="cuda")
        assert g.lib.rtlfm_gpu_run_device(g._h, d.data_ptr(), d.stride(0), 2, out.data_ptr(), out.stride(0), None) == -errno.ENOTSUP
        assert g.channels_tell() == 0
        g.set_path(0)
        got, _, paths = run_gpu(g, src, L, (2,))
        assert paths == [1]
    for s in range(4):
        assert_rows(got[s], want[s, :want_len[s]], cfg, f"p2_fir9 after the refusal, stream {s}")


# ------------------------------------------------------------------ 7. off is off ----

@pytest.mark.parametrize("offset_tuning", [0, 1])
def test_off_is_off(oracle_lib, offset_tuning):
    """set_channels(0) after use: per-stream rows again, offset_tuning honoured again, the carried state goes on."""
    nsrc, per, L = 2, 3, 4096
    S = nsrc * per
    cfg = make_cfg(dict(case("box7_std_lpr")[0], custom_atan=ATAN_FAST, offset_tuning=offset_tuning), L, 2)
    steps = make_steps(S, 5)
    src = bounded_bytes(nsrc, 2 * L, 41)
    rows = synth.random_u8(S, 2 * L, seed=42)
    with demod(cfg, S) as g:
        g.set_channels(per, steps=steps)
        run_gpu(g, src, L, (2,))
        g.set_channels(0)
        assert g.channels_tell() == 0
        carried = g.state_get_all()
        got, _, _ = run_gpu(g, rows, L, (2,))
        st = g.state_get_all()
    want, want_len, want_st = oracle_lib.run_batch(cfg, rows, carried)
    for s in range(S):
        assert np.array_equal(got[s], want[s, :want_len[s]]), s
        assert st[s].as_dict() == want_st[s].as_dict(), s
