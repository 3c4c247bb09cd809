"""k_input_health on the GPU: the overload / high-level / continuity records of the raw input bytes (softagc,
detect_overload, underrun_test of the reference) equal the restatement of tests/health_model.py EXACTLY - integers,
order-independent - for every block length, stream count, buffer count, entry point and path; with input_stats on as
well one launch writes both record sets; and switching the option on changes no existing result."""
import ctypes as C

import numpy as np
import pytest

import health_model as hm
import monitor_model as mm
from cases import case, make_cfg
from rtlsdr_amd import capi, synth
from rtlsdr_amd.capi import RtlfmCfg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

C2 = dict(downsample=16, downsample_passes=4, rate_out=150000)


def demod(cfg, ns, **options):
    from rtlsdr_amd.demod import GpuDemod
    return GpuDemod(cfg, ns, 0, options=options)


def fm(S, nbytes, **kw):
    """synth.fm_iq_u8, at most eight streams of it: further rows are those rolled (the model takes what it is given)."""
    base = synth.fm_iq_u8(min(S, 8), nbytes // 2, **kw)
    if S <= 8:
        return base
    return np.stack([np.roll(base[s % 8], 2 * (s // 8)) for s in range(S)])


def inputs(S, L, nb):
    cnt = hm.counter((S, nb * L), start=200)
    f = fm(S, nb * L, amplitude=60.0)
    return {"counter": cnt, "gaps": hm.plant_gaps(cnt, L), "random": synth.random_u8(S, nb * L, seed=L + S), "fm": f,
            "all127": np.full((S, nb * L), 127, dtype=np.uint8), "all0": np.zeros((S, nb * L), dtype=np.uint8),
            "all255": np.full((S, nb * L), 255, dtype=np.uint8), "values": hm.plant_values(f, L)}


UNPLANTED = {"gaps": "counter", "values": "fm"}


@pytest.mark.parametrize("S", [1, 3, 256])
@pytest.mark.parametrize("L", [512, 7680, 8192, 16384, 16896, 262144])
def test_records_equal_model(L, S):
    cap = 4
    cfg = RtlfmCfg.default(block_len=L, max_blocks=cap, **C2)
    with demod(cfg, S, input_health=1) as g:
        assert g.get_option("input_health") == 1 and g.get_option("input_stats") == 0
        ins = inputs(S, L, cap)
        wants = {k: hm.records(iq.reshape(S, cap, L)) for k, iq in ins.items()}
        assert not wants["counter"]["lost"].any()                    # a running counter loses nothing
        for k in ("all0", "all255"):                                   # every byte overloads; lost from the model
            assert (wants[k]["overload"] == L).all() and (wants[k]["high"] == L).all()
        assert (wants["all0"]["lost"] == L - 1).all() and (wants["all255"]["lost"] == 255 * (L - 1)).all()
        assert not wants["all127"]["overload"].any() and not wants["all127"]["high"].any()
        for k, base in UNPLANTED.items():                              # a planted input must exercise something
            assert (wants[k] != wants[base]).any(), k
        assert wants["gaps"]["lost"].any()
        for kind, iq in ins.items():
            want = wants[kind]
            d = torch.from_numpy(iq).cuda()
            for nb in range(1, cap + 1):  # 1 ... cap buffers: a run is the first nb buffers of every stream
                g.run_torch(d[:, :nb * L].contiguous())
                got = g.input_health_all()
                assert got.shape == (S, nb)
                bad = got != want[:, :nb]
                assert not bad.any(), (kind, nb, got[bad][:4], want[:, :nb][bad][:4])
                assert not got["pad_"].any()
            for s in {0, S // 2, S - 1}:
                assert np.array_equal(g.input_health(s), want[s])


def test_junctions():
    """A counter through all buffers of a run and across two runs loses 0 in the engine; a gap exactly at a buffer
    boundary is reported by the engine and by no record."""
    from rtlsdr_amd.agc import SoftAgc
    S, L, nb = 3, 8192, 4
    cfg = RtlfmCfg.default(block_len=L, max_blocks=nb, **C2)
    iq = hm.counter((S, 2 * nb * L), start=200)
    gap = iq.copy()
    gap[1, 5 * L:] += np.uint8(9)  # stream 1: between buffers 4 and 5, that is inside the second run
    gap[2, nb * L:] -= np.uint8(3)  # stream 2: between the two runs
    for data, dropped in ((iq, [0, 0, 0]), (gap, [0, 9, 3])):
        with demod(cfg, S, input_health=1) as g, SoftAgc([29] * S) as a:
            for r in range(2):
                g.run_torch(torch.from_numpy(data[:, r * nb * L:(r + 1) * nb * L].copy()).cuda())
                assert not g.input_health_all()["lost"].any()
                a.update(g)
            st = [a.state(s) for s in range(S)]
            assert [x["dropped_samples"] for x in st] == dropped
            assert all(x["total_samples"] == 2 * nb * L for x in st)


def test_option_is_range_checked_and_off_by_default():
    from rtlsdr_amd.agc import SoftAgc
    from rtlsdr_amd.capi import RtlfmError
    L = 16384
    cfg = RtlfmCfg.default(block_len=L, max_blocks=2, **C2)
    host = hm.plant_values(synth.fm_iq_u8(2, L), L)
    want = hm.records(host.reshape(2, 2, L))
    iq = torch.from_numpy(host).cuda()
    with demod(cfg, 2) as g, SoftAgc([5, 5]) as a:
        assert g.get_option("input_health") == 0 and g.get_option("block_len") == L
        g.run_torch(iq)
        with pytest.raises(RtlfmError) as e:
            g.input_health(0)
        assert e.value.code == -61  # -ENODATA while the option is off
        with pytest.raises(RtlfmError) as e:
            g.input_health_all()
        assert e.value.code == -61
        with pytest.raises(RtlfmError) as e:
            a.update(g)
        assert e.value.code == -61
        for bad in (-1, 2):
            with pytest.raises(RtlfmError) as e:
                g.set_option("input_health", bad)
            assert e.value.code == -22
        assert g.get_option("input_health") == 0
        g.set_option("input_health", 1)
        assert g.input_health(0).size == 0  # on, but the last run took none
        g.run_torch(iq)
        assert np.array_equal(g.input_health_all(), want)
        g.set_option("input_stats_nt", 0)  # plain loads: the same records
        g.run_torch(iq)
        assert np.array_equal(g.input_health_all(), want)
    with demod(cfg, 2, input_health=1) as g, SoftAgc([5, 5, 5]) as a3, SoftAgc([5]) as a1:
        g.run_torch(iq)
        for a in (a3, a1):  # a stream-count mismatch either way
            with pytest.raises(RtlfmError) as e:
                a.update(g)
            assert e.value.code == -22
        n = C.c_int()
        out = np.zeros(1, dtype=capi.INPUT_HEALTH_DTYPE)
        assert g.lib.rtlfm_gpu_input_health(g._h, 0, out.ctypes.data, 1, C.byref(n)) == -105 and n.value == 2  # -ENOBUFS
        assert g.lib.rtlfm_gpu_input_health(g._h, 2, out.ctypes.data, 1, C.byref(n)) == -22


@pytest.mark.parametrize("L", [16384, 65536])
def test_through_the_callback_boundary(L):
    """push + run and run_begin / run_end, full runs and shorter ones."""
    S, cap = 3, 4
    cfg = RtlfmCfg.default(block_len=L, max_blocks=cap, **C2)
    iq = hm.plant_gaps(hm.counter((S, 2 * cap * L), start=3), L)
    want = hm.records(iq.reshape(S, 2 * cap, L))
    with demod(cfg, S, input_health=1) as g:
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
            assert np.array_equal(g.input_health_all(), want[:, at:at + nb])
            for s in range(S):
                assert np.array_equal(g.input_health(s), want[s, at:at + nb])
            at += nb


@pytest.mark.parametrize("both", [0, 1])
def test_short_callback_buffers(both):
    """A ragged run (short buffers, another length per range of streams): each buffer's record over its own length."""
    S, L, nb = 4, 16384, 3
    cfg = RtlfmCfg.default(block_len=L, max_blocks=nb, **C2)
    iq = synth.random_u8(S, nb * L, seed=5)
    iq[:, ::3] = 255  # beyond a short buffer's end as well: a record that covered more would count it
    lens = [[L, 512, L], [L, 512, 8192], [4096, L, 8192], [4096, L, L]]
    with demod(cfg, S, input_health=1, input_stats=both) as g:
        for b in range(nb):
            for s in range(S):
                g.push(iq[s, b * L:b * L + lens[s][b]], s)
        g.run()
        g.fetch_all()
        got = g.input_health_all()
        st = g.input_stats_all() if both else None
        for s in range(S):
            for b in range(nb):
                buf = iq[s, b * L:b * L + lens[s][b]]
                assert got[s, b] == hm.records(buf), (s, b)
                if both:
                    assert st[s, b] == mm.records(buf), (s, b)


def test_run_device_never_reads_the_stride_padding():
    """stream_stride larger than the run, the padding filled with 255: a kernel that read it would count it."""
    S, L, nb, cap = 5, 32768, 3, 4
    cfg = RtlfmCfg.default(block_len=L, max_blocks=cap, **C2)
    iq = synth.fm_iq_u8(S, nb * L // 2, amplitude=60.0)
    want = hm.records(iq.reshape(S, nb, L))
    assert not want["overload"].any()
    stride = cap * L + 4096
    buf = torch.full((S + 1, stride), 255, dtype=torch.uint8, device="cuda")
    buf[:S, :nb * L] = torch.from_numpy(iq).cuda()
    with demod(cfg, S, input_health=1) as g:
        out = torch.empty((S, g.result_cap(nb)), dtype=torch.int16, device="cuda")
        n = torch.zeros(S, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        g.run_device(buf.data_ptr(), stride, nb, out.data_ptr(), out.stride(0), n.data_ptr())
        g.sync()
        got = g.input_health_all()
        assert np.array_equal(got["overload"], want["overload"])
        assert np.array_equal(got, want)


# the list of tests/test_input_stats_gpu.py
PATHS = [("c1_boxcar10_fast", 0, {}), ("c2_p4_std", 0, {}), ("c3_p6_fir9_deemph_up22050", 0, {}), ("wbfm_preset", 0, {}),
         ("raw_p2", 0, {}), ("raw_box10", 0, {}), ("p4_squelch", 0, {}), ("box84_fm_squelch50", 0, {}), ("p7_fir9", 0, {}),
         ("p4_rdc", 0, {}), ("c2_p4_std", 1, {}), ("c1_boxcar10_fast", 1, {}), ("c2_p4_std", 0, {"report_levels": 1})]


@pytest.mark.parametrize("name,path,extra", PATHS, ids=[f"{n}-path{p}{'-L' if e else ''}" for n, p, e in PATHS])
def test_every_path_and_nothing_else_changes(name, path, extra):
    """Boxcar, fused, with a tail, -M raw, squelch, deep, staged: the records equal the model; PCM, lengths, levels and
    the carried state are byte-identical with the option off and on; with input_stats on as well both record sets equal
    their models and the statistics are byte-identical to a run with input_stats alone."""
    import golden_util as gu
    ov, sig = case(name)
    S, L, nb = 5, 16384, 4
    cfg = make_cfg(dict(ov, **extra), L, nb)
    iq = hm.plant_values(synth.fm_iq_u8(S, 2 * nb * L // 2, **sig), L)
    want = hm.records(iq.reshape(S, 2 * nb, L))
    want_st = mm.records(iq.reshape(S, 2 * nb, L))
    d = torch.from_numpy(iq).cuda()
    have_levels = bool(cfg.squelch_level or cfg.report_levels)
    res = {}
    for key, opts in (("off", {}), ("on", {"input_health": 1}), ("stats", {"input_stats": 1}), ("both", {"input_health": 1, "input_stats": 1})):
        with demod(cfg, S, **opts) as g:
            g.set_path(path)
            got, stats = [], []
            for r in range(2):  # two runs: the carried state goes through
                out, n = g.run_torch(d[:, r * nb * L:(r + 1) * nb * L].contiguous())
                g.sync()
                got.append((out.cpu().numpy(), n.cpu().numpy(), g.levels_all() if have_levels else None))
                if "input_health" in opts:
                    assert np.array_equal(g.input_health_all(), want[:, r * nb:(r + 1) * nb]), (key, r)
                if "input_stats" in opts:
                    stats.append(g.input_stats_all())
                    assert np.array_equal(stats[-1], want_st[:, r * nb:(r + 1) * nb]), (key, r)
            res[key] = (got, [gu.state_dict(g.state_get(s), False) for s in range(S)], g.last_path, stats)
    for a, b in zip(res["stats"][3], res["both"][3]):
        assert a.tobytes() == b.tobytes()
    for key in ("on", "both"):
        assert res["off"][2] == res[key][2] and (path != 1 or res[key][2] == 1)
        assert res["off"][1] == res[key][1]
        for (o0, n0, l0), (o1, n1, l1) in zip(res["off"][0], res[key][0]):
            assert np.array_equal(n0, n1)
            for s in range(S):
                assert np.array_equal(o0[s, :n0[s]], o1[s, :n1[s]])
            assert (l0 is None and l1 is None) or np.array_equal(l0, l1)


@pytest.mark.parametrize("L", [512, 7680, 8192, 29184, 32768, 65536, 262144])
def test_both_options_one_launch(L):
    """input_stats and input_health together, at the lengths where the statistics' stride masks change (step 2, 2, 4, 6,
    18), and at 7680 and 29184 bytes, where the last wave of a loop of the kernel is half full: both record sets equal their
    models, with the statistics and without."""
    S, nb = 3, 3
    cfg = RtlfmCfg.default(block_len=L, max_blocks=nb, **C2)
    iq = hm.plant_values(synth.random_u8(S, nb * L, seed=L), L)
    with demod(cfg, S, input_health=1, input_stats=1) as g:
        for nt in (1, 0):
            g.set_option("input_stats_nt", nt)
            g.run_torch(torch.from_numpy(iq).cuda())
            assert np.array_equal(g.input_health_all(), hm.records(iq.reshape(S, nb, L)))
            assert np.array_equal(g.input_stats_all(), mm.records(iq.reshape(S, nb, L)))
    with demod(cfg, S, input_health=1) as g:
        g.run_torch(torch.from_numpy(iq).cuda())
        assert np.array_equal(g.input_health_all(), hm.records(iq.reshape(S, nb, L)))


@pytest.mark.parametrize("name", ["c2_p4_std", "c1_boxcar10_fast", "c3_p6_fir9_deemph"])
def test_verify_twice_gets_the_same_records(name):
    ov, sig = case(name)
    S, L, nb = 6, 32768, 3
    cfg = make_cfg(ov, L, nb)
    iq = hm.plant_values(synth.fm_iq_u8(S, nb * L // 2, **sig), L)
    with demod(cfg, S, input_health=1, verify_twice=1) as g:
        for _ in range(2):
            g.run_torch(torch.from_numpy(iq).cuda())
            g.sync()
            assert np.array_equal(g.input_health_all(), hm.records(iq.reshape(S, nb, L)))
        assert g.get_option("verify_runs") == 2 and g.get_option("verify_mismatches") == 0


def test_device_operator_256mib():
    """rtlfm_gpu_input_health_device on 256 x 4 x 262144 B: EVERY record against the twin, with clipping and gaps planted
    on the device at the kernel's boundaries; the combined operator gives the same records and k_input_stats's."""
    S, nb, L = 256, 4, 262144
    lib = capi.load()
    iq = synth.fm_iq_u8_torch(S, nb * L // 2, torch.device("cuda", 0), amplitude=100.0)
    rows = torch.arange(S, device="cuda")
    # a counter on every fourth stream, so that `lost` is small there and a single gap shows
    cnt = (torch.arange(nb * L, device="cuda") % 256).to(torch.uint8)
    iq[rows[::4]] = cnt
    pos = hm.boundary_positions(L)
    for b in range(nb):
        for k, p in enumerate(pos):
            sel = rows[(b + k)::len(pos)]
            if k % 3 == 0:
                iq[sel, b * L + p] = 255 if (k + b) % 2 else 0                 # clipping
            elif k % 3 == 1:
                iq[sel, b * L + p] = iq[sel, b * L + p] + (1, 255, 128)[b % 3]  # a gap of +1, -1, +128 at one byte
            else:
                iq[sel, b * L + p] = (63, 64, 191, 192)[(k + b) % 4]
    out = torch.zeros((S * nb, 16), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    q = torch.cuda.current_stream().cuda_stream or None
    assert lib.rtlfm_gpu_input_health_device(0, iq.data_ptr(), iq.stride(0), L, nb, S, out.data_ptr(), 1, q) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(capi.INPUT_HEALTH_DTYPE).reshape(S, nb)
    host = iq.cpu().numpy()
    want = hm.records(host.reshape(S, nb, L))
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert want["overload"].any() and (want["lost"][::4] > 0).any() and (want["lost"][::4] < 2000).all()
    out2 = torch.zeros_like(out)
    st = torch.zeros((S * nb, 4), dtype=torch.int32, device="cuda")
    for nt in (1, 0):
        assert lib.rtlfm_gpu_input_health_stats_device(0, iq.data_ptr(), iq.stride(0), L, nb, S, out2.data_ptr(), st.data_ptr(), nt, q) == 0
        torch.cuda.synchronize()
        assert np.array_equal(out2.cpu().numpy().view(capi.INPUT_HEALTH_DTYPE).reshape(S, nb), want)
        assert np.array_equal(st.cpu().numpy().view(capi.INPUT_STAT_DTYPE).reshape(S, nb), mm.records(host.reshape(S, nb, L)))
    # the argument checks of rtlfm_gpu_input_stats_device
    assert lib.rtlfm_gpu_input_health_device(0, None, iq.stride(0), L, nb, S, out.data_ptr(), 1, q) == -22
    assert lib.rtlfm_gpu_input_health_device(0, iq.data_ptr(), iq.stride(0), L, nb, S, out.data_ptr() + 4, 1, q) == -22
    assert lib.rtlfm_gpu_input_health_device(0, iq.data_ptr(), iq.stride(0), 500, nb, S, out.data_ptr(), 1, q) == -22
    assert lib.rtlfm_gpu_input_health_device(0, iq.data_ptr(), nb * L - 16, L, nb, S, out.data_ptr(), 1, q) == -22
    assert lib.rtlfm_gpu_input_health_device(0, iq.data_ptr() + 1, iq.stride(0), L, nb, S, out.data_ptr(), 1, q) == -22
    assert lib.rtlfm_gpu_input_health_device(99, iq.data_ptr(), iq.stride(0), L, nb, S, out.data_ptr(), 1, q) == -19
