"""k_input_stats on the GPU: the ADC statistics of the raw input bytes (rtlsdr_callback, reference src/rtl_fm.c:1302-1324)
equal the restatement of tests/monitor_model.py EXACTLY - integers, order-independent - for every block length, stream
count, buffer count, entry point and path, and switching the option on changes no existing result."""
import numpy as np
import pytest

import monitor_model as mm
from cases import case, make_cfg
from rtlsdr_amd import synth
from rtlsdr_amd.capi import RtlfmCfg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

C2 = dict(downsample=16, downsample_passes=4, rate_out=150000)


def demod(cfg, ns, **options):
    from rtlsdr_amd.demod import GpuDemod
    return GpuDemod(cfg, ns, 0, options=options)


def planted(iq, L):
    """A single 255 / 0 at the first and last byte of a buffer and at bytes the strided sum skips (2 and 3 when
    step > 2), another variant per (stream, buffer)."""
    out = iq.copy()
    S, nb = out.shape[0], out.shape[1] // L
    spots = [(0, 255), (L - 1, 255), (L - 1, 0), (2, 255), (3, 0), (0, 0)]
    for s in range(S):
        for b in range(nb):
            at, v = spots[(s + b) % len(spots)]
            out[s, b * L + at] = v
    return out


def inputs(S, L, nb):
    fm = synth.fm_iq_u8(S, nb * L // 2, amplitude=60.0)
    return {"fm": fm, "random": synth.random_u8(S, nb * L, seed=L + S), "all127": np.full((S, nb * L), 127, dtype=np.uint8),
            "planted": planted(fm, L)}


@pytest.mark.parametrize("S", [1, 3, 256])
@pytest.mark.parametrize("L", [512, 16384, 16896, 32768, 65536, 262144])
def test_records_equal_model(L, S):
    cap = 4 if L >= 65536 else 6
    cfg = RtlfmCfg.default(block_len=L, max_blocks=cap, **C2)
    with demod(cfg, S, input_stats=1) as g:
        assert g.get_option("input_stats") == 1
        ins = inputs(S, L, cap)
        for kind, iq in ins.items():
            want = mm.records(iq.reshape(S, cap, L))
            if kind == "planted":
                assert (want["max"] == 255).any() and (want != mm.records(ins["fm"].reshape(S, cap, L))).any()
            d = torch.from_numpy(iq).cuda()
            for nb in range(1, cap + 1):  # 1 ... cap_blocks buffers: a run is the first nb buffers of every stream
                g.run_torch(d[:, :nb * L].contiguous())
                got = g.input_stats_all()
                assert got.shape == (S, nb)
                assert np.array_equal(got, want[:, :nb]), (kind, nb, got[got != want[:, :nb]][:4], want[:, :nb][got != want[:, :nb]][:4])
            for s in {0, S // 2, S - 1}:
                assert np.array_equal(g.input_stats(s), want[s])


def test_option_is_range_checked_and_off_by_default():
    from rtlsdr_amd.capi import RtlfmError
    cfg = RtlfmCfg.default(block_len=16384, max_blocks=2, **C2)
    iq = torch.from_numpy(synth.fm_iq_u8(2, 16384)).cuda()
    with demod(cfg, 2) as g:
        assert g.get_option("input_stats") == 0 and g.get_option("input_stats_nt") == 1
        g.run_torch(iq)
        with pytest.raises(RtlfmError) as e:
            g.input_stats(0)
        assert e.value.code == -61  # -ENODATA while the option is off
        for bad in (-1, 2):
            with pytest.raises(RtlfmError) as e:
                g.set_option("input_stats", bad)
            assert e.value.code == -22
        g.set_option("input_stats", 1)
        assert g.input_stats(0).size == 0  # on, but the last run took none
        g.run_torch(iq)
        assert np.array_equal(g.input_stats_all(), mm.records(iq.cpu().numpy().reshape(2, 2, 16384)))
        g.set_option("input_stats_nt", 0)  # plain loads: the same records
        g.run_torch(iq)
        assert np.array_equal(g.input_stats_all(), mm.records(iq.cpu().numpy().reshape(2, 2, 16384)))


@pytest.mark.parametrize("L", [16384, 65536])
def test_through_the_callback_boundary(L):
    """push + run and run_begin / run_end, full runs and shorter ones."""
    S, cap = 3, 4
    cfg = RtlfmCfg.default(block_len=L, max_blocks=cap, **C2)
    iq = planted(synth.fm_iq_u8(S, 2 * cap * L // 2), L)
    want = mm.records(iq.reshape(S, 2 * cap, L))
    with demod(cfg, S, input_stats=1) as g:
        at = 0
        for nb, two_step in ((cap, False), (1, True), (3, False)):
            for b in range(nb):
                for s in range(S):
                    g.push(iq[s, (at + b) * L:(at + b + 1) * L], s)
            if two_step:
                assert g.run_begin() == nb
                g.run_end()
            else:
                g.run()
            g.fetch_all()
            assert np.array_equal(g.input_stats_all(), want[:, at:at + nb])
            for s in range(S):
                assert np.array_equal(g.input_stats(s), want[s, at:at + nb])
            at += nb


def test_short_callback_buffers():
    """A ragged run (short buffers, another length per range of streams): each buffer's record over its own length."""
    S, L, nb = 4, 16384, 3
    cfg = RtlfmCfg.default(block_len=L, max_blocks=nb, **C2)
    iq = synth.random_u8(S, nb * L, seed=5)
    lens = [[L, 512, L], [L, 512, 8192], [4096, L, 8192], [4096, L, L]]
    with demod(cfg, S, input_stats=1) as g:
        for b in range(nb):
            for s in range(S):
                g.push(iq[s, b * L:b * L + lens[s][b]], s)
        g.run()
        g.fetch_all()
        got = g.input_stats_all()
        for s in range(S):
            for b in range(nb):
                assert got[s, b] == mm.records(iq[s, b * L:b * L + lens[s][b]]), (s, b)


def test_run_device_never_reads_the_stride_padding():
    """stream_stride larger than the run, the padding filled with 255: a kernel that read it would report max 255."""
    S, L, nb, cap = 5, 32768, 3, 4
    cfg = RtlfmCfg.default(block_len=L, max_blocks=cap, **C2)
    iq = synth.fm_iq_u8(S, nb * L // 2, amplitude=60.0)
    want = mm.records(iq.reshape(S, nb, L))
    assert want["max"].max() < 255
    stride = cap * L + 4096
    buf = torch.full((S + 1, stride), 255, dtype=torch.uint8, device="cuda")
    buf[:S, :nb * L] = torch.from_numpy(iq).cuda()
    with demod(cfg, S, input_stats=1) as g:
        out = torch.empty((S, g.result_cap(nb)), dtype=torch.int16, device="cuda")
        n = torch.zeros(S, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        g.run_device(buf.data_ptr(), stride, nb, out.data_ptr(), out.stride(0), n.data_ptr())
        g.sync()
        assert np.array_equal(g.input_stats_all(), want)


PATHS = [("c1_boxcar10_fast", 0, {}), ("c2_p4_std", 0, {}), ("c3_p6_fir9_deemph_up22050", 0, {}), ("wbfm_preset", 0, {}),
         ("raw_p2", 0, {}), ("raw_box10", 0, {}), ("p4_squelch", 0, {}), ("box84_fm_squelch50", 0, {}), ("p7_fir9", 0, {}),
         ("p4_rdc", 0, {}), ("c2_p4_std", 1, {}), ("c1_boxcar10_fast", 1, {}), ("c2_p4_std", 0, {"report_levels": 1})]


@pytest.mark.parametrize("name,path,extra", PATHS, ids=[f"{n}-path{p}{'-L' if e else ''}" for n, p, e in PATHS])
def test_every_path_and_nothing_else_changes(name, path, extra):
    """Boxcar, fused, with a tail, -M raw, squelch, deep, staged: the records equal the model, and PCM, lengths, levels and
    the carried state are byte-identical with the option off and on."""
    import golden_util as gu
    ov, sig = case(name)
    S, L, nb = 5, 16384, 4
    cfg = make_cfg(dict(ov, **extra), L, nb)
    iq = planted(synth.fm_iq_u8(S, 2 * nb * L // 2, **sig), L)
    want = mm.records(iq.reshape(S, 2 * nb, L))
    d = torch.from_numpy(iq).cuda()
    have_levels = bool(cfg.squelch_level or cfg.report_levels)
    res = {}
    for on in (0, 1):
        with demod(cfg, S, input_stats=on) as g:
            g.set_path(path)
            got = []
            for r in range(2):  # two runs: the carried state goes through
                out, n = g.run_torch(d[:, r * nb * L:(r + 1) * nb * L].contiguous())
                g.sync()
                got.append((out.cpu().numpy(), n.cpu().numpy(), g.levels_all() if have_levels else None))
                if on:
                    assert np.array_equal(g.input_stats_all(), want[:, r * nb:(r + 1) * nb]), r
            res[on] = (got, [gu.state_dict(g.state_get(s), False) for s in range(S)], g.last_path)
    assert res[0][2] == res[1][2] and (path != 1 or res[1][2] == 1)
    assert res[0][1] == res[1][1]
    for (o0, n0, l0), (o1, n1, l1) in zip(res[0][0], res[1][0]):
        assert np.array_equal(n0, n1)
        for s in range(S):
            assert np.array_equal(o0[s, :n0[s]], o1[s, :n1[s]])
        assert (l0 is None and l1 is None) or np.array_equal(l0, l1)


@pytest.mark.parametrize("name", ["c2_p4_std", "c1_boxcar10_fast", "c3_p6_fir9_deemph"])
def test_verify_twice_gets_the_same_records(name):
    ov, sig = case(name)
    S, L, nb = 6, 32768, 3
    cfg = make_cfg(ov, L, nb)
    iq = planted(synth.fm_iq_u8(S, nb * L // 2, **sig), L)
    with demod(cfg, S, input_stats=1, verify_twice=1) as g:
        for _ in range(2):
            g.run_torch(torch.from_numpy(iq).cuda())
            g.sync()
            assert np.array_equal(g.input_stats_all(), mm.records(iq.reshape(S, nb, L)))
        assert g.get_option("verify_runs") == 2 and g.get_option("verify_mismatches") == 0


def test_full_size_whole_population():
    """4096 streams x 4 x 262144 B (4 GiB): EVERY record against numpy, in chunks of streams."""
    S, nb, L = 4096, 4, 262144
    cfg = RtlfmCfg.default(block_len=L, max_blocks=nb, **C2)
    iq = synth.fm_iq_u8_torch(S, nb * L // 2, torch.device("cuda", 0))
    # single bytes planted on the device: first / last byte of a buffer and skipped bytes, clipping on some streams
    rows = torch.arange(S, device="cuda")
    for b in range(nb):
        iq[rows[b::7], b * L] = 255
        iq[rows[(b + 1)::11], (b + 1) * L - 1] = 0
        iq[rows[(b + 2)::13], b * L + 2] = 255
        iq[rows[(b + 3)::17], b * L + 3] = 0
    with demod(cfg, S, input_stats=1) as g:
        g.run_torch(iq)
        got = g.input_stats_all()
    assert got.shape == (S, nb)
    for s0 in range(0, S, 128):
        want = mm.records(iq[s0:s0 + 128].cpu().numpy().reshape(-1, nb, L))
        assert np.array_equal(got[s0:s0 + 128], want), s0
    assert (got["max"] == 255).sum() >= S // 7 and (got["step"] == 18).all() and (got["pow_count"] == 14564).all()
