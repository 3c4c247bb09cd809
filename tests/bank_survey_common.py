"""What test_bank_survey_gpu.py and test_bank_bins_gpu.py share: the survey and per-source, per-run bins taken from
tests/channel_bank_model.py used as it is (BankModel.frames() returns Y of all K bins).  A plain module, like
channel_common.py."""
import numpy as np


def survey_of(frames):
    """frames: BankModel.frames()'s list per source.  (power uint64 [sources, K], frames int32 [sources])."""
    power = np.stack([(yi * yi + yq * yq).astype(np.uint64).sum(axis=0, dtype=np.uint64) for _, _, yi, yq in frames])
    return power, np.array([yi.shape[0] for _, _, yi, _ in frames], dtype=np.int32)


def pick(frames, bins_ps):
    """(I, Q) per stream, as BankModel.run returns them, for bins_ps [sources][per_source]."""
    I, Q = [], []
    for (_, _, yi, yq), bins in zip(frames, bins_ps, strict=True):
        for b in bins:
            I.append(yi[:, int(b)].copy())
            Q.append(yq[:, int(b)].copy())
    return I, Q


def model_run(model, src, bins_ps=None):
    """One run of the model: ((I, Q) for bins_ps - the model's own shared list where None -, power, frames)."""
    fr = model.frames(src)
    I, Q = pick(fr, [model.bins] * model.nsrc if bins_ps is None else bins_ps)
    power, n = survey_of(fr)
    return (I, Q), power, n


def assert_survey(got, power, frames, what):
    gp, gf = got
    assert gf.tolist() == frames.tolist(), (what, gf.tolist(), frames.tolist())
    assert gp.dtype == np.uint64 and gp.shape == power.shape, (what, gp.shape, power.shape)
    if not np.array_equal(gp, power):
        bad = np.argwhere(gp != power)
        raise AssertionError(f"{what}: {len(bad)} of {power.size} sums differ, first at (source, bin) {bad[:4].tolist()}: "
                             f"{[int(gp[tuple(b)]) for b in bad[:4]]} for {[int(power[tuple(b)]) for b in bad[:4]]}")
