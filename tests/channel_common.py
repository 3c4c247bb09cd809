"""What the channel tests on the GPU share (test_channels_gpu.py, test_channel_fir_gpu.py, test_channel_bank_gpu.py,
test_channel_history_gpu.py): handles, runs, inputs and comparisons.  A plain module, like cases.py.

Where the files' own copies differed, both are here under two names."""
import numpy as np

from cases import make_cfg
from channel_fir_model import raw_rows
from rtlsdr_amd.capi import ATAN_FAST, ATAN_STD, MODE_AM, MODE_FM, MODE_RAW

SPECIAL_STEPS = [0, 1, 1 << 30, 1 << 31, (1 << 32) - 1]

# the back half behind a filter or a bank
BACK = {
    "fmfast": dict(mode=MODE_FM, custom_atan=ATAN_FAST),
    "am": dict(mode=MODE_AM, output_scale=3),
    "fmfast_squelch": dict(mode=MODE_FM, custom_atan=ATAN_FAST, squelch_level=20),
    "raw_levels": dict(mode=MODE_RAW, report_levels=1),
}


def demod(cfg, ns, **options):
    from rtlsdr_amd.demod import GpuDemod
    return GpuDemod(cfg, ns, 0, options=options)


def raw_cfg(D, L, nb=3, **ov):
    return make_cfg(dict(mode=MODE_RAW, downsample=D, **ov), L, nb)


def steps_for(S):
    return np.arange(S, dtype=np.uint32) * 12345  # (kept and not used while the bank is on)


def bank_handle(cfg, nsrc, K, bins, taps, shift, path=0, **options):
    per = K if bins is None else len(bins)
    g = demod(cfg, nsrc * per, **options)
    g.set_path(path)
    g.set_channels(per, steps=steps_for(nsrc * per))
    g.set_channel_bank(K, taps, shift, bins=bins)
    return g


def to_device(rows_u8):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rows_u8)).cuda()


def run_once(g, d, L, b0, nb):
    """One run of buffers b0 .. b0 + nb of the device rows d: (per stream PCM, last_path)."""
    o, n = g.run_torch(d[:, b0 * L:(b0 + nb) * L].contiguous())
    g.sync()
    o, n = o.cpu().numpy(), n.cpu().numpy()
    return [o[s, :n[s]].copy() for s in range(g.nstreams)], g.last_path


def run_gpu_per_run(g, rows_u8, L, runs, paths=None):
    """Consecutive runs; paths: set_path() in front of each.  Returns (per stream PCM of all runs, per run per stream PCM,
    last_path of every run)."""
    d = to_device(rows_u8)
    per_run, seen, b0 = [], [], 0
    for r, nb in enumerate(runs):
        if paths is not None:
            g.set_path(paths[r])
        rows, p = run_once(g, d, L, b0, nb)
        per_run.append(rows)
        seen.append(p)
        b0 += nb
    return [np.concatenate([pr[s] for pr in per_run]) for s in range(g.nstreams)], per_run, seen


def run_gpu(g, rows_u8, L, runs, paths=None):
    """run_gpu_per_run without the per-run rows: (per stream PCM of all runs, last_path of every run)."""
    rows, _, seen = run_gpu_per_run(g, rows_u8, L, runs, paths)
    return rows, seen


def run_gpu_levels(g, rows_u8, L, runs, levels=False):
    """Consecutive runs of runs[k] buffers from rows_u8 [rows, buffers * L].  Returns (every stream's PCM of all runs,
    levels_all() of all runs side by side or None, last_path of every run)."""
    d = to_device(rows_u8)
    outs = [[] for _ in range(g.nstreams)]
    lv, paths, b0 = [], [], 0
    for nb in runs:
        rows, p = run_once(g, d, L, b0, nb)
        for s in range(g.nstreams):
            outs[s].append(rows[s])
        if levels:
            lv.append(g.levels_all())
        paths.append(p)
        b0 += nb
    return [np.concatenate(x) for x in outs], (np.concatenate(lv, axis=1) if levels else None), paths


def model_runs(model, src, L, runs):
    """The model (FirModel, BankModel) over the same runs: (per stream raw rows of all runs, per run (I, Q))."""
    per_run, b0 = [], 0
    for nb in runs:
        per_run.append(model.run(src[:, b0 * L:(b0 + nb) * L]))
        b0 += nb
    rows = [np.concatenate([raw_rows(I, Q)[s] for I, Q in per_run]) for s in range(model.S)]
    return rows, per_run


def make_steps(n, seed):
    rng = np.random.default_rng(seed)
    st = [int(v) for v in rng.integers(0, 1 << 32, size=n, dtype=np.uint64)]
    for i, v in enumerate((0, 1 << 30, (1 << 32) - 1)[:n]):
        st[(i * 2) % n] = v
    return st


def make_steps_special(n, seed):
    """Random steps with SPECIAL_STEPS among them, in an order that goes round with the seed."""
    rng = np.random.default_rng(seed)
    st = [int(v) for v in rng.integers(0, 1 << 32, size=n, dtype=np.uint64)]
    k = seed % len(SPECIAL_STEPS)
    sp = SPECIAL_STEPS[k:] + SPECIAL_STEPS[:k]
    for i in range(min(n, len(sp))):
        st[(i * 3) % n if n >= 15 else i] = sp[i]
    return st


def random_fir_taps(ntaps, seed, small=False):
    """int16 taps and a shift that keeps most outputs of full-scale input inside an int16 and lets some saturate."""
    rng = np.random.default_rng(seed)
    if small:
        return rng.integers(-8, 9, size=ntaps).astype(np.int16), 0
    return rng.integers(-2000, 2001, size=ntaps).astype(np.int16), int(np.log2(ntaps)) // 2 + 4


def random_bank_taps(K, ntaps, seed):
    """int16 taps and a shift that keeps most sums of full-scale input inside an int16 and lets some saturate."""
    rng = np.random.default_rng(seed)
    Q = (ntaps + K - 1) // K
    return rng.integers(-2000, 2001, size=ntaps).astype(np.int16), int(np.log2(Q)) // 2 + 3


def full_scale(rows, nbytes, seed):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, size=(rows, nbytes), dtype=np.uint8)
    src[0, : nbytes // 2] = rng.integers(0, 2, size=nbytes // 2).astype(np.uint8) * 255
    return src


def bounded(rows, nbytes, seed, bound):
    rng = np.random.default_rng(seed)
    return (rng.integers(-bound, bound + 1, size=(rows, nbytes)) + 127).astype(np.uint8)


def assert_rows(got, want, what):
    """Every stream's row, equal in every bit."""
    for s, (a, b) in enumerate(zip(got, want, strict=True)):
        assert a.shape == b.shape, (what, s, a.shape, b.shape)
        if not np.array_equal(a, b):
            bad = np.flatnonzero(a != b)
            raise AssertionError(f"{what} stream {s}: {bad.size} of {a.size} differ, first at {bad[:8].tolist()}: "
                                 f"{a[bad[:4]].tolist()} for {b[bad[:4]].tolist()}")


def std_fm(cfg):
    return cfg.mode == MODE_FM and cfg.custom_atan == ATAN_STD


def assert_row_cfg(got, want, cfg, what):
    """One stream's row: equal, or - -M fm with -A std alone - within the project's stated tolerance."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    nbad = int((diff != 0).sum())
    where = np.flatnonzero(diff)[:8].tolist()
    assert std_fm(cfg), f"{what}: {nbad} of {got.size} differ, first at {where}"
    assert diff.max() <= 1 and nbad <= max(1, int(1e-4 * got.size)), f"{what}: {nbad} of {got.size} differ, max {diff.max()}"


def tone_fit(pcm, tone_hz, rate, skip):
    """(RMS of what is left of the audio after the best fit of a tone at tone_hz and a constant, the tone's amplitude)."""
    y = pcm[skip:].astype(np.float64)
    t = (np.arange(y.size) + skip) / rate
    A = np.stack([np.sin(2 * np.pi * tone_hz * t), np.cos(2 * np.pi * tone_hz * t), np.ones(y.size)], axis=1)
    coef, *_ = np.linalg.lstsq(A, y, rcond=None)
    return float(np.sqrt(np.mean((y - A @ coef) ** 2))), float(np.hypot(coef[0], coef[1]))


SEEK_TO = 123456789


def assert_call_clears_the_history(new_model, open_handle, calls, what, src, L, label):
    """A run, the call calls[what](g), a run: the second run equals the model with the history cleared by the call - and
    differs from the model that kept it, so a call that does not clear fails here.  ("set_channels" and "reset" put pos
    back to 0, "channels_seek" moves it to SEEK_TO.)"""
    cleared, kept = new_model(), new_model()
    for m in (cleared, kept):
        m.run(src[:, :L])
    if what in ("set_channels", "reset"):
        cleared.pos = kept.pos = 0
    if what == "channels_seek":
        cleared.pos = kept.pos = SEEK_TO
    cleared.clear()
    want = raw_rows(*cleared.run(src[:, L:]))
    unwanted = raw_rows(*kept.run(src[:, L:]))
    assert not any(np.array_equal(a, b) for a, b in zip(want, unwanted, strict=True))
    with open_handle() as g:
        d = to_device(src)
        run_once(g, d, L, 0, 1)
        calls[what](g)
        got, _ = run_once(g, d, L, 1, 1)
    assert_rows(got, want, label)
