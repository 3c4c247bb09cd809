"""The route table of an rtl_fm run as rows (tests/test_fm_route_cpu.py, tests/test_fm_route_gpu.py): configuration,
options, path, channels, placement of the output rows and buffer count -> the route and the rest rtlfm_run_route must
name and a run must leave in last_route / last_rest.  A plain module, like cases.py.

The shapes are those the GPU suite runs and reads last_path on (cases.py at 16384 bytes, test_row_geometry_gpu.py's
placements, the channel suites' 2 sources x 2 channels), cut to two buffers of three streams.  Every FM row is -A fast:
the discriminator is no input of the plan, and -A fast is equal in every bit on both paths."""
import errno

from rtlsdr_amd.capi import (ATAN_FAST, CHANNELS_BANK, CHANNELS_FILTER, CHANNELS_MIXER, CHANNELS_OFF, MODE_AM, MODE_RAW,
                             RESAMPLE_ARBITRARY, RESAMPLE_LOW_PASS_REAL, REST_BACK_HALF, REST_DEEP_DEMOD, REST_DEEP_IQ,
                             REST_IRREGULAR, REST_NONE, REST_PER_PASS, REST_TAIL, ROUTE_BOXCAR, ROUTE_BOXCAR_EMIT,
                             ROUTE_CHAN_BANK, ROUTE_CHAN_BANK_PLAIN, ROUTE_CHAN_BOXCAR, ROUTE_CHAN_FIR, ROUTE_CHAN_FIR_PLAIN,
                             ROUTE_CHAN_MIX, ROUTE_FUSED, ROUTE_FUSED_EMIT, ROUTE_STAGED)

ENOTSUP = -errno.ENOTSUP
STREAMS = 3            # channels: 2 sources x 2 channels
# where the output rows lie: (int16 elements from a 128-byte line, stride = capacity rounded up to `rem` modulo `mod`)
PLACES = {"line": (0, 64, 0), "dword": (2, 8, 2), "stride4": (0, 8, 4)}
LAUNCH_OPTIONS = dict(fused_waves=64, fused_min_tiles=1, fused_tiles_per_seg=2, box_store=1, fused_store=1, lpr_chunk=512, lpr_threads=64,
                      lpr_ring=0, lpr_separate=1, lpr_scalar_stores=1, arb_waves=3)


def row(name, want, rest, ov, L=16384, opts=None, path=0, chan=CHANNELS_OFF, place="line", nb=2, gpu=True, stride=None):
    """want: the route, or the negative errno the run answers; stride: int16 between the output rows where the row needs
    another than its place's (CPU only)."""
    ov = dict(ov)
    if ov.get("mode", 0) == 0:
        ov["custom_atan"] = ATAN_FAST
    return dict(name=name, want=want, rest=rest, ov=ov, L=L, opts=dict(opts or {}), path=path, chan=chan, place=place, nb=nb, gpu=gpu,
                stride=stride)


P4 = dict(downsample=16, downsample_passes=4)
SQ = dict(squelch_level=50)
BOX84 = dict(downsample=84, rate_out=12000)
P7 = dict(downsample=128, downsample_passes=7)
DEEMPH_ALONE = dict(downsample=8, downsample_passes=3, deemph=1, deemph_a=5)
C3 = dict(downsample=64, downsample_passes=6, comp_fir_size=9, deemph=1, deemph_a=2, rate_out=16000, rate_out2=22050, resampler=RESAMPLE_ARBITRARY)


def _rows():
    r = [
        # ---- k_fused to PCM, and where it gives way
        row("p4", ROUTE_FUSED, REST_TAIL, P4),
        row("p4_fir9", ROUTE_FUSED, REST_TAIL, dict(P4, comp_fir_size=9)),
        row("p6_c3_tail", ROUTE_FUSED, REST_TAIL, C3),
        row("am_p4", ROUTE_FUSED, REST_TAIL, dict(P4, mode=MODE_AM, output_scale=16)),
        # FM to PCM without an out-of-place tail stage: 16-byte stores straight into the caller's rows
        row("p4_dword", ROUTE_STAGED, REST_BACK_HALF, P4, place="dword"),
        row("p4_stride4", ROUTE_STAGED, REST_BACK_HALF, P4, place="stride4"),
        row("p4_dword_path2", ENOTSUP, None, P4, place="dword", path=2),
        row("p4_stride4_path2", ENOTSUP, None, P4, place="stride4", path=2),
        row("p4_post4_dword", ROUTE_FUSED, REST_TAIL, dict(P4, post_downsample=4), place="dword"),
        row("c3_dword", ROUTE_FUSED, REST_TAIL, C3, place="dword"),
        # ... which the run's length decides where deemph_filter stands alone: from 2048 samples on it is the out-of-place kernel
        row("p3_deemph_dword_2048", ROUTE_FUSED, REST_TAIL, DEEMPH_ALONE, place="dword", nb=2),
        row("p3_deemph_dword_1024", ROUTE_STAGED, REST_BACK_HALF, DEEMPH_ALONE, place="dword", nb=1),
        row("p3_deemph_dword_four_pass", ROUTE_STAGED, REST_BACK_HALF, DEEMPH_ALONE, place="dword", opts=dict(deemph_four_pass=1)),
        row("p3_deemph_dword_sequential", ROUTE_STAGED, REST_BACK_HALF, DEEMPH_ALONE, place="dword", opts=dict(deemph_sequential=1)),
        row("p3_deemph_line_1024", ROUTE_FUSED, REST_TAIL, DEEMPH_ALONE, nb=1),
        # the squelch / -L: rms()'s sums in the front end, or the emit mode
        row("p4_squelch", ROUTE_FUSED, REST_TAIL, dict(P4, **SQ)),
        row("p4_levels", ROUTE_FUSED, REST_TAIL, dict(P4, report_levels=1)),
        row("p4_squelch_unfused", ROUTE_FUSED_EMIT, REST_BACK_HALF, dict(P4, **SQ), opts=dict(squelch_fused=0)),
        row("p4_squelch_dword", ROUTE_FUSED_EMIT, REST_BACK_HALF, dict(P4, **SQ), place="dword"),
        row("p1_squelch_32768", ROUTE_FUSED, REST_TAIL, dict(downsample=2, downsample_passes=1, **SQ), L=65536),
        row("p1_squelch_65536", ROUTE_FUSED_EMIT, REST_BACK_HALF, dict(downsample=2, downsample_passes=1, **SQ), L=131072),
        # -M raw: the emitted IQ is the output
        row("raw_p2", ROUTE_FUSED_EMIT, REST_NONE, dict(mode=MODE_RAW, downsample=4, downsample_passes=2)),
        row("raw_p2_dword", ROUTE_FUSED_EMIT, REST_BACK_HALF, dict(mode=MODE_RAW, downsample=4, downsample_passes=2), place="dword"),
        row("raw_p2_stride4", ROUTE_FUSED_EMIT, REST_BACK_HALF, dict(mode=MODE_RAW, downsample=4, downsample_passes=2), place="stride4"),
        row("raw_p2_squelch", ROUTE_FUSED_EMIT, REST_BACK_HALF, dict(mode=MODE_RAW, downsample=4, downsample_passes=2, **SQ)),
        # the raw DC block and buffers that are no whole tiles: the MFMA pass 0 only
        row("p4_rdc", ROUTE_FUSED, REST_TAIL, dict(P4, dc_block_raw=1)),
        row("p4_rdc_mfma", ROUTE_FUSED, REST_TAIL, dict(P4, dc_block_raw=1), opts=dict(pass0_engine=1)),
        row("p4_rdc_valu", ROUTE_STAGED, REST_BACK_HALF, dict(P4, dc_block_raw=1), opts=dict(pass0_engine=0)),
        row("p4_rdc_valu_path2", ENOTSUP, None, dict(P4, dc_block_raw=1), opts=dict(pass0_engine=0), path=2),
        row("p4_valu", ROUTE_FUSED, REST_TAIL, P4, opts=dict(pass0_engine=0)),
        row("p4_partial_mfma", ROUTE_FUSED, REST_TAIL, P4, L=8704, opts=dict(pass0_engine=1)),
        row("p4_partial_valu", ROUTE_STAGED, REST_BACK_HALF, P4, L=8704, opts=dict(pass0_engine=0)),
        row("p4_partial_squelch_valu", ROUTE_STAGED, REST_BACK_HALF, dict(P4, **SQ), L=8704, opts=dict(pass0_engine=0)),
        row("p7_rdc_valu", ROUTE_STAGED, REST_BACK_HALF, dict(P7, dc_block_raw=1), L=65536, opts=dict(pass0_engine=0)),
        # seven passes and more behind six fused ones
        row("p7", ROUTE_FUSED_EMIT, REST_DEEP_DEMOD, P7, L=65536),
        row("p7_squelch", ROUTE_FUSED_EMIT, REST_DEEP_IQ, dict(P7, **SQ), L=65536),
        row("p7_raw", ROUTE_FUSED_EMIT, REST_DEEP_IQ, dict(P7, mode=MODE_RAW), L=65536),
        row("p7_per_pass", ROUTE_FUSED_EMIT, REST_PER_PASS, P7, L=65536, opts=dict(deep_rest=0)),
        row("p7_squelch_per_pass", ROUTE_FUSED_EMIT, REST_PER_PASS, dict(P7, **SQ), L=65536, opts=dict(deep_rest=0)),
        row("p7_dword", ROUTE_FUSED_EMIT, REST_DEEP_DEMOD, P7, L=65536, place="dword"),
        row("p10_fir9_short", ROUTE_FUSED_EMIT, REST_PER_PASS, dict(downsample=1024, downsample_passes=10, comp_fir_size=9)),  # 128 samples at level 6: the tails are longer
        row("p10_fir9", ROUTE_FUSED_EMIT, REST_DEEP_DEMOD, dict(downsample=1024, downsample_passes=10, comp_fir_size=9), L=65536),
        row("p9_irregular", ROUTE_FUSED_EMIT, REST_IRREGULAR, dict(downsample=512, downsample_passes=9), L=1536),
        row("p9_irregular_valu", ROUTE_STAGED, REST_IRREGULAR, dict(downsample=512, downsample_passes=9), L=1536, opts=dict(pass0_engine=0)),
        row("p9_irregular_raw", ROUTE_FUSED_EMIT, REST_IRREGULAR, dict(downsample=512, downsample_passes=9, mode=MODE_RAW), L=1536),
        # ---- k_boxcar_scan
        row("box10", ROUTE_BOXCAR, REST_TAIL, dict(downsample=10, rate_out=240000)),
        row("box10_dword", ROUTE_BOXCAR, REST_TAIL, dict(downsample=10, rate_out=240000), place="dword"),
        row("box10_rdc_valu", ROUTE_BOXCAR, REST_TAIL, dict(downsample=10, rate_out=240000, dc_block_raw=1), opts=dict(pass0_engine=0)),
        row("wbfm", ROUTE_BOXCAR, REST_TAIL, dict(downsample=6, deemph=1, deemph_a=13, rate_out=170000, rate_out2=32000, resampler=RESAMPLE_LOW_PASS_REAL)),
        row("box84_squelch_16384", ROUTE_BOXCAR, REST_TAIL, dict(BOX84, **SQ)),
        row("box84_squelch_8192", ROUTE_BOXCAR_EMIT, REST_BACK_HALF, dict(BOX84, **SQ), L=8192),
        row("box84_squelch_unfused", ROUTE_BOXCAR_EMIT, REST_BACK_HALF, dict(BOX84, **SQ), opts=dict(squelch_fused=0)),
        row("box1_squelch_65538", ROUTE_BOXCAR_EMIT, REST_BACK_HALF, dict(downsample=1, **SQ), L=65536),  # 2 (32768 / 1 + 1) elements a buffer
        row("box2_squelch_32770", ROUTE_BOXCAR_EMIT, REST_BACK_HALF, dict(downsample=2, **SQ), L=65536),
        row("box3_squelch", ROUTE_BOXCAR, REST_TAIL, dict(downsample=3, **SQ), L=65536),
        row("raw_box10", ROUTE_BOXCAR_EMIT, REST_NONE, dict(mode=MODE_RAW, downsample=10)),
        row("raw_box10_dword", ROUTE_BOXCAR_EMIT, REST_NONE, dict(mode=MODE_RAW, downsample=10), place="dword"),
        row("raw_box10_levels", ROUTE_BOXCAR_EMIT, REST_BACK_HALF, dict(mode=MODE_RAW, downsample=10, report_levels=1)),
        row("box10_fir9", ROUTE_STAGED, REST_BACK_HALF, dict(downsample=10, comp_fir_size=9)),  # (generic_fir behind the boxcar: the staged kernels')
        row("box10_fir9_path2", ENOTSUP, None, dict(downsample=10, comp_fir_size=9), path=2),
    ]
    # rtlfm_gpu_set_path(1) everywhere: the staged kernels, whatever the rest of the row says; (2) where a fused form exists: that form
    for x in list(r):
        if x["path"] == 0 and x["want"] != ENOTSUP:
            irregular = x["rest"] == REST_IRREGULAR
            r.append(dict(x, name=x["name"] + "_path1", path=1, want=ROUTE_STAGED, rest=REST_IRREGULAR if irregular else REST_BACK_HALF))
            if x["want"] != ROUTE_STAGED:
                r.append(dict(x, name=x["name"] + "_path2", path=2))
    # ---- channels x {boxcar, filter, bank} x path {0, 1, 2} x {0, 4 passes}
    box = dict(downsample=8)
    one = {CHANNELS_MIXER: ROUTE_CHAN_BOXCAR, CHANNELS_FILTER: ROUTE_CHAN_FIR, CHANNELS_BANK: ROUTE_CHAN_BANK}
    plain = {CHANNELS_MIXER: ROUTE_CHAN_MIX, CHANNELS_FILTER: ROUTE_CHAN_FIR_PLAIN, CHANNELS_BANK: ROUTE_CHAN_BANK_PLAIN}
    for chan, tag in ((CHANNELS_MIXER, "mix"), (CHANNELS_FILTER, "fir"), (CHANNELS_BANK, "bank")):
        for path in (0, 1, 2):
            r.append(row(f"chan_{tag}_box8_path{path}", plain[chan] if path == 1 else one[chan], REST_BACK_HALF, box, chan=chan, path=path))
            if chan == CHANNELS_MIXER:
                r.append(row(f"chan_mix_p4_path{path}", ENOTSUP if path == 2 else ROUTE_CHAN_MIX, None if path == 2 else REST_BACK_HALF, P4,
                             chan=chan, path=path))
            else:  # rtlfm_gpu_set_channel_filter / _bank refuse a handle with fifth_order passes: no such run
                r.append(row(f"chan_{tag}_p4_path{path}", ENOTSUP, None, P4, chan=chan, path=path, gpu=False))
    r += [
        row("chan_mix_squelch", ROUTE_CHAN_BOXCAR, REST_BACK_HALF, dict(box, **SQ), chan=CHANNELS_MIXER),
        row("chan_mix_raw", ROUTE_CHAN_BOXCAR, REST_NONE, dict(box, mode=MODE_RAW), chan=CHANNELS_MIXER),
        row("chan_mix_raw_dword", ROUTE_CHAN_BOXCAR, REST_NONE, dict(box, mode=MODE_RAW), chan=CHANNELS_MIXER, place="dword"),
        row("chan_mix_raw_levels", ROUTE_CHAN_BOXCAR, REST_BACK_HALF, dict(box, mode=MODE_RAW, report_levels=1), chan=CHANNELS_MIXER),
        row("chan_mix_raw_path1", ROUTE_CHAN_MIX, REST_BACK_HALF, dict(box, mode=MODE_RAW), chan=CHANNELS_MIXER, path=1),
        # a row with no spare dword behind its last possible output (2 x 16384 / 2 / 8 = 2048 samples): through chan_iq
        row("chan_mix_raw_tight_rows", ROUTE_CHAN_BOXCAR, REST_BACK_HALF, dict(box, mode=MODE_RAW), chan=CHANNELS_MIXER, gpu=False, stride=2 * 2048 + 2),
        row("chan_mix_raw_spare_dword", ROUTE_CHAN_BOXCAR, REST_NONE, dict(box, mode=MODE_RAW), chan=CHANNELS_MIXER, gpu=False, stride=2 * 2048 + 4),
        row("chan_fir_raw", ROUTE_CHAN_FIR, REST_BACK_HALF, dict(box, mode=MODE_RAW), chan=CHANNELS_FILTER),
        row("chan_bank_raw", ROUTE_CHAN_BANK, REST_BACK_HALF, dict(box, mode=MODE_RAW), chan=CHANNELS_BANK),
        row("chan_mix_p9_irregular", ROUTE_CHAN_MIX, REST_IRREGULAR, dict(downsample=512, downsample_passes=9), L=1536, chan=CHANNELS_MIXER),
    ]
    names = [x["name"] for x in r]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return r


ROWS = _rows()


def out_stride(r, cap):
    """int16 between the output rows of row r for windows of `cap` elements."""
    if r["stride"] is not None:
        return r["stride"]
    _, mod, rem = PLACES[r["place"]]
    return cap + (rem - cap) % mod


def out_low_bits(r):
    return (2 * PLACES[r["place"]][0]) & 15
