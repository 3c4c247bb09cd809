"""ctypes binding of the C ABI declared in ``include/rtlfm_hip.h``.

The shared library (``rtlsdr_amd/csrc/librtlfm_hip.so``) is the product; this
module only marshals plain pointers and sizes into it.  There is no CPU
fallback: if the library is missing, or it finds no GPU, the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "librtlfm_hip.so")

RTLFM_MAX_PASSES = 10
RTLFM_MAX_BLOCK_LEN = 262144

MODE_FM, MODE_AM, MODE_USB, MODE_LSB, MODE_RAW = range(5)
CHANNEL_MAX_TAPS = 1024  # RTLFM_CHANNEL_MAX_TAPS
BANK_MAX_TAPS = 4096  # RTLFM_BANK_MAX_TAPS
ATAN_STD, ATAN_FAST, ATAN_LUT = range(3)
RESAMPLE_LOW_PASS_REAL, RESAMPLE_ARBITRARY = range(2)
PATH_AUTO, PATH_STAGED, PATH_FUSED = range(3)


class RtlfmCfg(C.Structure):
    """``rtlfm_cfg`` — the demod_state fields that stay constant while
    samples flow (reference: src/rtl_fm.c:172-208)."""

    _fields_ = [
        ("mode", C.c_int32),
        ("downsample", C.c_int32),
        ("downsample_passes", C.c_int32),
        ("comp_fir_size", C.c_int32),
        ("custom_atan", C.c_int32),
        ("post_downsample", C.c_int32),
        ("deemph", C.c_int32),
        ("deemph_a", C.c_int32),
        ("rate_out", C.c_int32),
        ("rate_out2", C.c_int32),
        ("resampler", C.c_int32),
        ("dc_block_audio", C.c_int32),
        ("adc_block_const", C.c_int32),
        ("dc_block_raw", C.c_int32),
        ("rdc_block_const", C.c_int32),
        ("offset_tuning", C.c_int32),
        ("output_scale", C.c_int32),
        ("squelch_level", C.c_int32),
        ("block_len", C.c_uint32),
        ("max_blocks", C.c_int32),
        ("report_levels", C.c_int32),
    ]

    @classmethod
    def from_saved(cls, raw: bytes) -> "RtlfmCfg":
        """A configuration stored by an earlier round's fixture: later fields are zero."""
        return cls.from_buffer_copy(raw.ljust(C.sizeof(cls), b"\0"))

    @classmethod
    def default(cls, **kw) -> "RtlfmCfg":
        """demod_init() defaults (src/rtl_fm.c:1608-1640) plus overrides."""
        c = cls()
        c.mode = MODE_FM
        c.downsample = 1
        c.downsample_passes = 0
        c.comp_fir_size = 0
        c.custom_atan = ATAN_STD
        c.post_downsample = 1
        c.deemph = 0
        c.deemph_a = 0
        c.rate_out = 24000
        c.rate_out2 = -1
        c.resampler = RESAMPLE_LOW_PASS_REAL
        c.dc_block_audio = 0
        c.adc_block_const = 9
        c.dc_block_raw = 0
        c.rdc_block_const = 9
        c.offset_tuning = 0
        c.output_scale = 1
        c.squelch_level = 0
        c.block_len = 16384
        c.max_blocks = 1
        for k, v in kw.items():
            if not hasattr(c, k):
                raise AttributeError(k)
            setattr(c, k, v)
        return c

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class RtlfmStreamState(C.Structure):
    """``rtlfm_stream_state`` — what one stream carries between blocks."""

    _fields_ = [
        ("lp_i_hist", (C.c_int16 * 6) * RTLFM_MAX_PASSES),
        ("lp_q_hist", (C.c_int16 * 6) * RTLFM_MAX_PASSES),
        ("droop_i_hist", C.c_int16 * 9),
        ("droop_q_hist", C.c_int16 * 9),
        ("pad_", C.c_int16 * 2),
        ("now_r", C.c_int32),
        ("now_j", C.c_int32),
        ("prev_index", C.c_int32),
        ("pre_r", C.c_int32),
        ("pre_j", C.c_int32),
        ("now_lpr", C.c_int32),
        ("prev_lpr_index", C.c_int32),
        ("deemph_avg", C.c_int32),
        ("dc_avg", C.c_int32),
        ("dc_avgI", C.c_int32),
        ("dc_avgQ", C.c_int32),
        ("squelch_hits", C.c_int32),
    ]

    def as_dict(self) -> dict:
        d = {}
        for n, _ in self._fields_:
            if n == "pad_":
                continue
            v = getattr(self, n)
            if n in ("lp_i_hist", "lp_q_hist"):
                v = [list(r) for r in v]
            elif hasattr(v, "__len__"):
                v = list(v)
            d[n] = v
        return d


class RtlfmInputStat(C.Structure):
    """``rtlfm_input_stat`` — the ADC statistics of one raw buffer (reference: src/rtl_fm.c:1302-1324)."""

    _fields_ = [("pow_sum", C.c_uint32), ("pow_count", C.c_int32), ("max", C.c_int32), ("step", C.c_int32)]


# the same record as a numpy dtype (GpuDemod.input_stats / .input_stats_all return arrays of it)
INPUT_STAT_DTYPE = [("pow_sum", "<u4"), ("pow_count", "<i4"), ("max", "<i4"), ("step", "<i4")]


class RtlfmInputHealth(C.Structure):
    """``rtlfm_input_health`` — overload / high-level / continuity counts of one raw buffer (include/rtlfm_hip.h)."""

    _fields_ = [("overload", C.c_uint32), ("high", C.c_uint32), ("lost", C.c_uint32), ("first", C.c_uint8), ("last", C.c_uint8),
                ("pad_", C.c_uint16)]


# ... as a numpy dtype (GpuDemod.input_health / .input_health_all return arrays of it)
INPUT_HEALTH_DTYPE = [("overload", "<u4"), ("high", "<u4"), ("lost", "<u4"), ("first", "u1"), ("last", "u1"), ("pad_", "<u2")]


class RtlfmGateRec(C.Structure):
    """``rtlfm_gate_rec`` — what the squelch gate decided for one buffer (include/rtlfm_hip.h)."""

    _fields_ = [("hits_after", C.c_int32), ("emit", C.c_uint8), ("pad", C.c_uint8 * 3)]


# ... as a numpy dtype (GpuDemod.gate / .gate_all return arrays of it)
GATE_REC_DTYPE = [("hits_after", "<i4"), ("emit", "u1"), ("pad", "u1", (3,))]


class RtlfmPackedRow(C.Structure):
    """``rtlfm_packed_row`` — where one stream's row lies in a packed result buffer (include/rtlfm_hip.h)."""

    _fields_ = [("offset", C.c_uint64), ("len", C.c_int32), ("held", C.c_int32)]


# ... as a numpy dtype (GpuDemod.fetch_packed and pack_device return arrays of it)
PACKED_ROW = [("offset", "<u8"), ("len", "<i4"), ("held", "<i4")]


class RtlfmScanEvent(C.Structure):
    """``rtlfm_scan_event`` — one hop of a stream (include/rtlfm_scan.h)."""

    _fields_ = [("stream", C.c_int32), ("from_index", C.c_int32), ("to_index", C.c_int32), ("freq", C.c_uint32),
                ("pad_", C.c_uint32), ("buffer_serial", C.c_int64)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "pad_"}


class RtlfmSlotsCfg(C.Structure):
    """``rtlfm_slots_cfg`` (include/rtlfm_slots.h)."""

    _fields_ = [("open_level", C.c_uint64), ("close_level", C.c_uint64), ("hang", C.c_int32), ("park", C.c_int32),
                ("mask", C.c_void_p)]


class RtlfmSlotsEvent(C.Structure):
    """``rtlfm_slots_event`` — one change of a slot's bin; an idle slot is bin -1 (include/rtlfm_slots.h)."""

    _fields_ = [("source", C.c_int32), ("slot", C.c_int32), ("old_bin", C.c_int32), ("new_bin", C.c_int32)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class RtlfmAgcEvent(C.Structure):
    """``rtlfm_agc_event`` — one change of a stream's gain index (include/rtlfm_agc.h)."""

    _fields_ = [("stream", C.c_int32), ("old_index", C.c_int32), ("new_index", C.c_int32), ("overloaded", C.c_int32),
                ("buffer_serial", C.c_int64)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class RtlfmIqEvent(C.Structure):
    """``rtlfm_iq_event`` — one decision of the IQ-balance engine (include/rtlfm_iq.h)."""

    _fields_ = [("source", C.c_int32), ("kind", C.c_int32), ("coef", C.c_int16 * 4), ("g_q14", C.c_int32), ("s_q14", C.c_int32),
                ("window_serial", C.c_int64)]

    def as_dict(self) -> dict:
        return {n: (tuple(getattr(self, n)) if n == "coef" else getattr(self, n)) for n, _ in self._fields_}


IQ_OK, IQ_WEAK, IQ_REJECTED = range(3)           # rtlfm_iq_compute's verdicts
IQ_EVENT_CHANGED, IQ_EVENT_REJECTED = range(2)   # rtlfm_iq_event.kind
# ``rtlfm_iq_sums`` as a numpy dtype (GpuDemod.source_iq_sums / _all return arrays of it)
IQ_SUMS_DTYPE = [("n", "<u4"), ("clipped", "<u4"), ("si", "<u8"), ("sq", "<u8"), ("sii", "<u8"), ("sqq", "<u8"), ("siq", "<u8")]

MONITOR_AUTO_GAIN = -100
CRIT_IN, CRIT_OUT, CRIT_LT, CRIT_GT = range(4)
CRIT_NAMES = ("in", "out", "<", ">")  # aCritStr, src/rtl_fm.c:116
MONITOR_COMMAND_MAX, MONITOR_ARGS_MAX = 256, 1024


class RtlfmMonitorRule(C.Structure):
    """``rtlfm_monitor_rule`` — one measurement line of the command file (include/rtlfm_monitor.h)."""

    _fields_ = [
        ("freq", C.c_uint32),
        ("gain", C.c_int32),
        ("crit", C.c_int32),
        ("num_meas", C.c_int32),
        ("ref_level", C.c_double),
        ("ref_tol", C.c_double),
        ("num_block_trigger", C.c_int32),
        ("check_adc_max", C.c_int32),
        ("check_adc_rms", C.c_int32),
        ("omit_first", C.c_int32),
        ("command", C.c_char * MONITOR_COMMAND_MAX),
        ("args", C.c_char * MONITOR_ARGS_MAX),
    ]

    @classmethod
    def default(cls, **kw) -> "RtlfmMonitorRule":
        """cmd_init()'s values (rtlfm_monitor_rule_default) plus overrides."""
        r = cls(crit=CRIT_IN, num_meas=10, omit_first=3)
        for k, v in kw.items():
            if not hasattr(r, k):
                raise AttributeError(k)
            setattr(r, k, v.encode() if isinstance(v, str) else v)
        return r

    def as_dict(self) -> dict:
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["command"] = d["command"].decode()
        d["args"] = d["args"].decode()
        return d


class RtlfmMonitorEvent(C.Structure):
    """``rtlfm_monitor_event`` — what one finished cycle of one stream reports."""

    _fields_ = [("stream", C.c_int32), ("cycle", C.c_int32), ("crit_met", C.c_int32), ("fired", C.c_int32),
                ("blocked_for", C.c_int32), ("adc_max", C.c_int32), ("level_db", C.c_double), ("adc_rms", C.c_double)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class RtlfmMonitorStat(C.Structure):
    """``rtlfm_monitor_stat`` — the exit statistics of one line (src/rtl_fm.c:2033-2040)."""

    _fields_ = [("count", C.c_int32), ("min_level", C.c_float), ("max_level", C.c_float), ("sum_levels", C.c_double)]


WIN_RECTANGLE, WIN_HAMMING, WIN_BLACKMAN, WIN_BLACKMAN_HARRIS, WIN_HANN_POISSON, WIN_YOUSSEF, WIN_KAISER, \
    WIN_BARTLETT = range(8)


class RtlpowerCfg(C.Structure):
    """``rtlpower_cfg`` — what scanner() reads (reference src/rtl_power.c:86-120)."""

    _fields_ = [
        ("bin_e", C.c_int32),
        ("window", C.c_int32),
        ("downsample", C.c_int32),
        ("downsample_passes", C.c_int32),
        ("boxcar", C.c_int32),
        ("comp_fir_size", C.c_int32),
        ("peak_hold", C.c_int32),
        ("buf_len", C.c_uint32),
    ]

    @classmethod
    def default(cls, **kw) -> "RtlpowerCfg":
        c = cls(bin_e=10, window=WIN_RECTANGLE, downsample=1, downsample_passes=0, boxcar=1,
                comp_fir_size=0, peak_hold=0, buf_len=16384)
        for k, v in kw.items():
            if not hasattr(c, k):
                raise AttributeError(k)
            setattr(c, k, v)
        return c

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class RtlfmRouteOpts(C.Structure):
    """``rtlfm_route_opts`` - what of a handle steers a run's plan besides its configuration, with a fresh handle's values."""

    _fields_ = [("path", C.c_int32), ("pass0_engine", C.c_int32), ("squelch_fused", C.c_int32), ("deep_rest", C.c_int32),
                ("deemph_four_pass", C.c_int32), ("deemph_sequential", C.c_int32), ("arb_serial", C.c_int32),
                ("no_deemph_scan", C.c_int32), ("channels", C.c_int32)]

    @classmethod
    def default(cls, **kw) -> "RtlfmRouteOpts":
        o = cls(path=0, pass0_engine=-1, squelch_fused=1, deep_rest=1, deemph_four_pass=0, deemph_sequential=0, arb_serial=-1,
                no_deemph_scan=0, channels=0)
        for k, v in kw.items():
            if not hasattr(o, k):
                raise AttributeError(k)
            setattr(o, k, v)
        return o


class RtlfmRoutePlan(C.Structure):
    """``rtlfm_route_plan`` - a run's plan as rtlfm_run_route writes it."""

    _fields_ = [(n, C.c_int32) for n in ("route", "rest", "last_path", "sq_front", "copy_state", "tail_follows", "tail", "N0", "Nblk", "D",
                                         "T", "varcnt", "level", "first_irr")]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


# enum rtlfm_route / rtlfm_rest / rtlfm_channels_kind (include/rtlfm_hip.h)
(ROUTE_STAGED, ROUTE_FUSED, ROUTE_FUSED_EMIT, ROUTE_BOXCAR, ROUTE_BOXCAR_EMIT, ROUTE_CHAN_MIX, ROUTE_CHAN_BOXCAR, ROUTE_CHAN_FIR,
 ROUTE_CHAN_FIR_PLAIN, ROUTE_CHAN_BANK, ROUTE_CHAN_BANK_PLAIN) = range(1, 12)
REST_NONE, REST_DEEP_DEMOD, REST_DEEP_IQ, REST_PER_PASS, REST_IRREGULAR, REST_BACK_HALF, REST_TAIL = range(7)
CHANNELS_OFF, CHANNELS_MIXER, CHANNELS_FILTER, CHANNELS_BANK = range(4)

# Every symbol include/rtlfm_hip.h declares: (name, restype, argtypes)
_P = C.POINTER
_SIGNATURES = [
    ("rtlfm_cfg_default", None, [_P(RtlfmCfg)]),
    ("rtlfm_optimal_settings", C.c_int,
     [_P(RtlfmCfg), C.c_uint32, C.c_int32, C.c_int32, C.c_int, C.c_int,
      _P(C.c_uint32), _P(C.c_uint32)]),
    ("rtlfm_deemph_a", C.c_int32, [C.c_int32, C.c_int32]),
    ("rtlfm_result_len", C.c_int, [_P(RtlfmCfg)]),
    ("rtlfm_result_cap", C.c_int, [_P(RtlfmCfg)]),
    ("rtlfm_cfg_validate", C.c_int, [_P(RtlfmCfg)]),
    ("rtlfm_gpu_create", C.c_int, [_P(RtlfmCfg), C.c_int, C.c_int, _P(C.c_void_p)]),
    ("rtlfm_gpu_destroy", C.c_int, [C.c_void_p]),
    ("rtlfm_gpu_push", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32]),
    ("rtlfm_gpu_acquire", C.c_int, [C.c_void_p, C.c_int, _P(C.c_void_p), _P(C.c_uint32)]),
    ("rtlfm_gpu_commit", C.c_int, [C.c_void_p, C.c_int, C.c_uint32]),
    ("rtlfm_gpu_run", C.c_int, [C.c_void_p]),
    ("rtlfm_gpu_run_begin", C.c_int, [C.c_void_p, _P(C.c_int)]),
    ("rtlfm_gpu_run_end", C.c_int, [C.c_void_p]),
    ("rtlfm_gpu_run_device", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("rtlfm_gpu_fetch", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, _P(C.c_int)]),
    ("rtlfm_gpu_fetch_all", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("rtlfm_gpu_fetch_all_prev", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("rtlfm_gpu_levels", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, _P(C.c_int)]),
    ("rtlfm_gpu_levels_all", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _P(C.c_int)]),
    ("rtlfm_gpu_input_stats", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, _P(C.c_int)]),
    ("rtlfm_gpu_input_stats_all", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _P(C.c_int)]),
    ("rtlfm_gpu_input_stats_device", C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    ("rtlfm_gpu_input_health", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, _P(C.c_int)]),
    ("rtlfm_gpu_input_health_all", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _P(C.c_int)]),
    ("rtlfm_gpu_input_health_device", C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    ("rtlfm_gpu_input_health_stats_device", C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                      C.c_void_p]),
    ("rtlfm_gpu_source_stats", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, _P(C.c_int)]),
    ("rtlfm_gpu_source_stats_all", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _P(C.c_int)]),
    ("rtlfm_gpu_source_health", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, _P(C.c_int)]),
    ("rtlfm_gpu_source_health_all", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _P(C.c_int)]),
    ("rtlfm_gpu_set_source_iq", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rtlfm_gpu_get_source_iq", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("rtlfm_gpu_source_iq_sums", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, _P(C.c_int)]),
    ("rtlfm_gpu_source_iq_sums_all", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _P(C.c_int)]),
    ("rtlfm_gpu_gate", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, _P(C.c_int)]),
    ("rtlfm_gpu_gate_all", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _P(C.c_int)]),
    ("rtlfm_gpu_mute", C.c_int, [C.c_void_p, C.c_int, C.c_uint32]),
    ("rtlfm_gpu_mute_device", C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]),
    ("rtlfm_gpu_fetch_packed", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, _P(C.c_size_t)]),
    ("rtlfm_gpu_fetch_packed_prev", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, _P(C.c_size_t)]),
    ("rtlfm_gpu_pack_device", C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    ("rtlfm_gpu_state_get", C.c_int, [C.c_void_p, C.c_int, _P(RtlfmStreamState)]),
    ("rtlfm_gpu_state_set", C.c_int, [C.c_void_p, C.c_int, _P(RtlfmStreamState)]),
    ("rtlfm_gpu_reset", C.c_int, [C.c_void_p]),
    ("rtlfm_gpu_state_get_all", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _P(C.c_int)]),
    ("rtlfm_gpu_state_set_all", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("rtlfm_gpu_state_move", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    ("rtlfm_gpu_save", C.c_int, [C.c_void_p, C.c_char_p]),
    ("rtlfm_gpu_load", C.c_int, [C.c_void_p, C.c_char_p]),
    ("rtlfm_gpu_channels_history_get", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, _P(C.c_int)]),
    ("rtlfm_gpu_channels_history_set", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    ("rtlfm_gpu_channels_move", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    ("rtlfm_gpu_channels_save", C.c_int, [C.c_void_p, C.c_char_p]),
    ("rtlfm_gpu_channels_load", C.c_int, [C.c_void_p, C.c_char_p]),
    ("rtlfm_channel_step", C.c_uint32, [C.c_int32, C.c_uint32]),
    ("rtlfm_channel_table", C.c_int, [C.c_void_p]),
    ("rtlfm_gpu_set_channels", C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    ("rtlfm_gpu_channels_seek", C.c_int, [C.c_void_p, C.c_uint64]),
    ("rtlfm_gpu_channels_tell", C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    ("rtlfm_channel_filter_check", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("rtlfm_channel_lowpass", C.c_int, [C.c_int, C.c_double, C.c_int, C.c_void_p, _P(C.c_int)]),
    ("rtlfm_gpu_set_channel_filter", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    ("rtlfm_gpu_get_channel_filter", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _P(C.c_int), _P(C.c_int)]),
    ("rtlfm_channel_bank_check", C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int]),
    ("rtlfm_channel_filter_check_dc", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("rtlfm_channel_bank_check_dc", C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int]),
    ("rtlfm_gpu_source_dc_prepass", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    ("rtlfm_gpu_set_channel_bank", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    ("rtlfm_gpu_get_channel_bank", C.c_int,
     [C.c_void_p, _P(C.c_int), C.c_void_p, C.c_int, C.c_void_p, C.c_int, _P(C.c_int), _P(C.c_int)]),
    ("rtlfm_gpu_bank_survey", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, _P(C.c_int)]),
    ("rtlfm_gpu_bank_survey_prev", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, _P(C.c_int)]),
    ("rtlfm_gpu_set_channel_bins", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rtlfm_gpu_get_channel_bins", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("rtlfm_gpu_sync", C.c_int, [C.c_void_p]),
    ("rtlfm_gpu_set_stream", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rtlfm_gpu_wait_for", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rtlfm_gpu_release_to", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rtlfm_gpu_set_path", C.c_int, [C.c_void_p, C.c_int]),
    ("rtlfm_gpu_last_path", C.c_int, [C.c_void_p]),
    ("rtlfm_run_route", C.c_int, [_P(RtlfmCfg), C.c_int, C.c_int, C.c_uint, C.c_size_t, _P(RtlfmRouteOpts), _P(RtlfmRoutePlan)]),
    ("rtlfm_gpu_timing_enable", C.c_int, [C.c_void_p, C.c_int]),
    ("rtlfm_gpu_timing_read", C.c_int, [C.c_void_p, _P(C.c_double), _P(C.c_int)]),
    ("rtlfm_gpu_clock_probe", C.c_int, [C.c_void_p, C.c_int]),
    ("rtlfm_gpu_clock_read", C.c_int, [C.c_void_p, _P(C.c_double), _P(C.c_double)]),
    ("rtlfm_gpu_clock_stamps", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _P(C.c_int)]),
    ("rtlfm_gpu_bw_probe", C.c_int, [C.c_int, C.c_size_t, C.c_int, C.c_int, _P(C.c_double), _P(C.c_double), _P(C.c_double),
                                     _P(C.c_double)]),
    ("rtlfm_gpu_set_option", C.c_int, [C.c_void_p, C.c_char_p, C.c_long]),
    ("rtlfm_gpu_get_option", C.c_int, [C.c_void_p, C.c_char_p, _P(C.c_long)]),
    ("rtlfm_gpu_selftest_atan2", C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    ("rtlfm_gpu_selftest_fast_atan2", C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    ("rtlfm_gpu_selftest_const_div", C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    ("rtlfm_debug_live", C.c_long, [C.c_int]),
    ("rtlfm_gpu_rotate_90_u8", C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("rtlfm_gpu_malloc", C.c_int, [C.c_int, C.c_size_t, _P(C.c_void_p)]),
    ("rtlfm_gpu_malloc_apart", C.c_int, [C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, _P(C.c_void_p), _P(C.c_int)]),
    ("rtlfm_gpu_malloc_apart_ex", C.c_int, [C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, _P(C.c_void_p), _P(C.c_int),
                                            _P(C.c_double), _P(C.c_size_t)]),
    ("rtlfm_gpu_placement_probe", C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, _P(C.c_double), _P(C.c_double)]),
    ("rtlfm_gpu_place_pair", C.c_int, [C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, _P(C.c_void_p), _P(C.c_void_p), _P(C.c_int), _P(C.c_int),
                                       _P(C.c_double), _P(C.c_size_t)]),
    ("rtlfm_gpu_copy", C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]),
    ("rtlfm_gpu_free", C.c_int, [C.c_void_p]),
    ("rtlfm_gpu_device_numa_node", C.c_int, [C.c_int]),
    ("rtlfm_plan_segments", C.c_int, [C.c_int] * 8 + [_P(C.c_int), _P(C.c_int), C.c_int]),
    ("rtlfm_gpu_strerror", C.c_char_p, [C.c_int]),
    ("rtlfm_gpu_version", C.c_int, []),
]

class RtlpowerPlan(C.Structure):
    """``rtlpower_plan`` — frequency_range()'s hop plan (reference src/rtl_power.c:438-540)."""

    _fields_ = [("lower", C.c_int32), ("upper", C.c_int32), ("max_size", C.c_int32), ("tune_count", C.c_int32),
                ("bw_seen", C.c_int32), ("rate", C.c_int32), ("bin_e", C.c_int32), ("downsample", C.c_int32),
                ("downsample_passes", C.c_int32), ("buf_len", C.c_int32), ("crop", C.c_double),
                ("bin_size", C.c_double)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class RtlpowerRouteOpts(C.Structure):
    """``rtlpower_route_opts`` — the options that steer a scan, with their defaults."""

    _fields_ = [("groups", C.c_int32), ("dec_fast", C.c_int32), ("staged_fast", C.c_int32), ("staged_pipe", C.c_int32),
                ("staged_batch", C.c_int32), ("scan_frames", C.c_int32)]

    @classmethod
    def default(cls, **kw) -> "RtlpowerRouteOpts":
        o = cls(groups=0, dec_fast=1, staged_fast=1, staged_pipe=0, staged_batch=0, scan_frames=1)
        for k, v in kw.items():
            if not hasattr(o, k):
                raise AttributeError(k)
            setattr(o, k, v)
        return o


# ... and include/rtlpower_hip.h
_POWER_SIGNATURES = [
    ("rtlpower_frequency_range", C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int, _P(RtlpowerPlan)]),
    ("rtlpower_tune_freq", C.c_int32, [_P(RtlpowerPlan), C.c_int]),
    ("rtlpower_plan_cfg", None, [_P(RtlpowerPlan), C.c_int, C.c_int, C.c_int, C.c_int, _P(RtlpowerCfg)]),
    ("rtlpower_csv_dbm", C.c_int, [_P(RtlpowerPlan), C.c_int, C.c_void_p, C.c_int32, C.c_char_p, C.c_size_t]),
    ("rtlpower_window_coefs", C.c_int, [C.c_int, C.c_int, C.c_void_p]),
    ("rtlpower_cfg_validate", C.c_int, [_P(RtlpowerCfg)]),
    ("rtlpower_gpu_create", C.c_int, [_P(RtlpowerCfg), C.c_int, C.c_int, _P(C.c_void_p)]),
    ("rtlpower_gpu_destroy", C.c_int, [C.c_void_p]),
    ("rtlpower_gpu_scan_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    ("rtlpower_gpu_scan", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32]),
    ("rtlpower_gpu_fetch", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, _P(C.c_int32)]),
    ("rtlpower_gpu_clear", C.c_int, [C.c_void_p]),
    ("rtlpower_gpu_sync", C.c_int, [C.c_void_p]),
    ("rtlpower_gpu_set_stream", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rtlpower_gpu_wait_for", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rtlpower_gpu_release_to", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rtlpower_gpu_set_option", C.c_int, [C.c_void_p, C.c_char_p, C.c_long]),
    ("rtlpower_gpu_get_option", C.c_int, [C.c_void_p, C.c_char_p, _P(C.c_long)]),
    ("rtlpower_gpu_timing_enable", C.c_int, [C.c_void_p, C.c_int]),
    ("rtlpower_gpu_timing_read", C.c_int, [C.c_void_p, _P(C.c_double), _P(C.c_int)]),
    ("rtlpower_gpu_clock_probe", C.c_int, [C.c_void_p, C.c_int]),
    ("rtlpower_gpu_clock_read", C.c_int, [C.c_void_p, _P(C.c_double), _P(C.c_double)]),
    ("rtlpower_report_host", C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_int, C.c_double, C.c_void_p, _P(C.c_int)]),
    ("rtlpower_csv_report", C.c_int, [_P(RtlpowerPlan), C.c_int, C.c_void_p, C.c_int, C.c_int32, C.c_char_p, C.c_size_t]),
    ("rtlpower_gpu_store", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int32]),
    ("rtlpower_gpu_scan_host", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    ("rtlpower_gpu_report", C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_int]),
    ("rtlpower_gpu_report_fetch", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, _P(C.c_int), _P(C.c_int32)]),
    ("rtlpower_gpu_report_fetch_all", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    ("rtlpower_scan_route", C.c_int, [_P(RtlpowerCfg), C.c_int, C.c_int, C.c_size_t, C.c_uint, _P(RtlpowerRouteOpts)]),
]
CENTI_SIGN, CENTI_INF, CENTI_NAN = 0x80000000, 0x7FFFFFFF, 0x7FFFFFFE  # RTLPOWER_CENTI_* (include/rtlpower_hip.h)
_SIGNATURES = _SIGNATURES + _POWER_SIGNATURES

# ... and include/rtlfm_monitor.h (the level monitor: host code inside the same library)
_MONITOR_SIGNATURES = [
    ("rtlfm_monitor_rule_default", None, [_P(RtlfmMonitorRule)]),
    ("rtlfm_monitor_create", C.c_int, [C.c_int, _P(RtlfmMonitorRule), _P(C.c_void_p)]),
    ("rtlfm_monitor_destroy", C.c_int, [C.c_void_p]),
    ("rtlfm_monitor_feed", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    ("rtlfm_monitor_update", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rtlfm_monitor_poll", C.c_int, [C.c_void_p, _P(RtlfmMonitorEvent), C.c_int, _P(C.c_int)]),
    ("rtlfm_monitor_stats", C.c_int, [C.c_void_p, C.c_int, _P(RtlfmMonitorStat)]),
    ("rtlfm_monitor_rule_get", C.c_int, [C.c_void_p, C.c_int, _P(RtlfmMonitorRule)]),
    ("rtlfm_monitor_parse_file", C.c_int, [C.c_char_p, _P(RtlfmMonitorRule), C.c_int, _P(C.c_int), _P(C.c_int), _P(C.c_int)]),
    ("rtlfm_monitor_format_event", C.c_int, [_P(RtlfmMonitorRule), _P(RtlfmMonitorEvent), C.c_char_p, C.c_size_t]),
]
DECLARED_MONITOR_SYMBOLS = [s[0] for s in _MONITOR_SIGNATURES]

# ... and include/rtlfm_agc.h (input health: soft AGC, overload, continuity; host code inside the same library)
_AGC_SIGNATURES = [
    ("rtlfm_agc_create", C.c_int, [C.c_int, C.c_void_p, C.c_void_p, _P(C.c_void_p)]),
    ("rtlfm_agc_destroy", C.c_int, [C.c_void_p]),
    ("rtlfm_agc_feed", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    ("rtlfm_agc_update", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rtlfm_agc_poll", C.c_int, [C.c_void_p, _P(RtlfmAgcEvent), C.c_int, _P(C.c_int)]),
    ("rtlfm_agc_state", C.c_int, [C.c_void_p, C.c_int, _P(C.c_int32), _P(C.c_int32), _P(C.c_uint64), _P(C.c_uint64)]),
    ("rtlfm_agc_set_index", C.c_int, [C.c_void_p, C.c_int, C.c_int32]),
    ("rtlfm_agc_set_settle", C.c_int, [C.c_void_p, C.c_int32]),
]
DECLARED_AGC_SYMBOLS = [s[0] for s in _AGC_SIGNATURES]

# ... and include/rtlfm_iq.h (IQ balance per source: the policy between k_source_iq's records and its coefficients)
_IQ_SIGNATURES = [
    ("rtlfm_iq_compute", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, _P(C.c_int32), _P(C.c_int32)]),
    ("rtlfm_iq_create", C.c_int, [C.c_int, _P(C.c_void_p)]),
    ("rtlfm_iq_destroy", C.c_int, [C.c_void_p]),
    ("rtlfm_iq_feed", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    ("rtlfm_iq_update", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rtlfm_iq_poll", C.c_int, [C.c_void_p, _P(RtlfmIqEvent), C.c_int, _P(C.c_int)]),
    ("rtlfm_iq_coeffs", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rtlfm_iq_set_params", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
]
DECLARED_IQ_SYMBOLS = [s[0] for s in _IQ_SIGNATURES]

# ... and include/rtlfm_scan.h (the scanner's hop engine; host code inside the same library)
_SCAN_SIGNATURES = [
    ("rtlfm_scan_create", C.c_int, [C.c_int, C.c_uint32, C.c_int32, _P(C.c_void_p)]),
    ("rtlfm_scan_destroy", C.c_int, [C.c_void_p]),
    ("rtlfm_scan_set_list", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    ("rtlfm_scan_parse_list", C.c_int, [C.c_char_p, C.c_void_p, C.c_int, _P(C.c_int)]),
    ("rtlfm_scan_feed", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    ("rtlfm_scan_update", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rtlfm_scan_events", C.c_int, [C.c_void_p, _P(RtlfmScanEvent), C.c_int, _P(C.c_int)]),
    ("rtlfm_scan_apply", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rtlfm_scan_take_hopped", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _P(C.c_int)]),
    ("rtlfm_scan_freq", C.c_int, [C.c_void_p, C.c_int, _P(C.c_uint32), _P(C.c_int32), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64)]),
]
DECLARED_SCAN_SYMBOLS = [s[0] for s in _SCAN_SIGNATURES]

# ... and include/rtlfm_slots.h (the channel bank's slot allocator; host code inside the same library)
_SLOTS_SIGNATURES = [
    ("rtlfm_slots_create", C.c_int, [C.c_int, C.c_int, C.c_int, _P(RtlfmSlotsCfg), _P(C.c_void_p)]),
    ("rtlfm_slots_destroy", C.c_int, [C.c_void_p]),
    ("rtlfm_slots_step", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rtlfm_slots_bins", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rtlfm_slots_idle", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rtlfm_slots_events", C.c_int, [C.c_void_p, _P(RtlfmSlotsEvent), C.c_int, _P(C.c_int)]),
]
DECLARED_SLOTS_SYMBOLS = [s[0] for s in _SLOTS_SIGNATURES]

# ... and include/rtlfm_snapshot.h (the snapshot file of rtlfm_gpu_save / _load; host code inside the same library)
_SNAPSHOT_SIGNATURES = [
    ("rtlfm_snapshot_write", C.c_int, [C.c_char_p, _P(RtlfmCfg), C.c_int, C.c_void_p, C.c_void_p]),
    ("rtlfm_snapshot_info", C.c_int, [C.c_char_p, _P(RtlfmCfg), _P(C.c_int)]),
    ("rtlfm_snapshot_read", C.c_int, [C.c_char_p, _P(RtlfmCfg), C.c_void_p, C.c_void_p, C.c_int, _P(C.c_int)]),
]
DECLARED_SNAPSHOT_SYMBOLS = [s[0] for s in _SNAPSHOT_SIGNATURES]

class RtlfmChansnapHdr(C.Structure):
    """``rtlfm_chansnap_hdr`` — the header fields of a channel snapshot (include/rtlfm_chansnap.h)."""

    _fields_ = [("pos", C.c_uint64), ("nstreams", C.c_uint32), ("per_source", C.c_uint32), ("flags", C.c_uint32),
                ("fir_ntaps", C.c_uint32), ("fir_shift", C.c_uint32), ("bank_K", C.c_uint32), ("bank_ntaps", C.c_uint32),
                ("bank_shift", C.c_uint32), ("hist_samples", C.c_uint32), ("dc_pieces", C.c_uint32)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class RtlfmChansnapParts(C.Structure):
    """``rtlfm_chansnap_parts`` — the writer's sections."""

    _fields_ = [(n, C.c_void_p) for n in ("cfg", "steps", "fir_taps", "bank_taps", "bins", "states", "hist", "dc")]


class RtlfmChansnapBufs(C.Structure):
    """``rtlfm_chansnap_bufs`` — where the reader puts each section and how many elements fit there."""

    _fields_ = [("cfg", C.c_void_p)] + [f for n in ("steps", "fir_taps", "bank_taps", "bins", "states", "hist", "dc")
                                        for f in ((n, C.c_void_p), ("cap_" + n, C.c_size_t))]


CHANSNAP_HIST, CHANSNAP_DC_PIECES, CHANSNAP_DC_NONE = 4096, 16, 0x007F007F  # RTLFM_CHANSNAP_*
CHANSNAP_FLAG_SOURCE_DC, CHANSNAP_FLAG_HISTORY = 1, 2

# ... and include/rtlfm_chansnap.h (the file of rtlfm_gpu_channels_save / _load; host code inside the same library)
_CHANSNAP_SIGNATURES = [
    ("rtlfm_chansnap_write", C.c_int, [C.c_char_p, _P(RtlfmChansnapHdr), _P(RtlfmChansnapParts)]),
    ("rtlfm_chansnap_info", C.c_int, [C.c_char_p, _P(RtlfmChansnapHdr), _P(RtlfmCfg)]),
    ("rtlfm_chansnap_read", C.c_int, [C.c_char_p, _P(RtlfmChansnapHdr), _P(RtlfmChansnapBufs)]),
]
DECLARED_CHANSNAP_SYMBOLS = [s[0] for s in _CHANSNAP_SIGNATURES]

DECLARED_SYMBOLS = [s[0] for s in _SIGNATURES]
DECLARED_FM_SYMBOLS = [s[0] for s in _SIGNATURES if s[0].startswith("rtlfm_")]
DECLARED_POWER_SYMBOLS = [s[0] for s in _POWER_SIGNATURES]

_lib = None


class RtlfmError(RuntimeError):
    def __init__(self, code: int, what: str):
        self.code = code
        super().__init__(f"{what}: {code} ({strerror(code)})")


def load(path: str | None = None) -> C.CDLL:
    """Load librtlfm_hip.so (once) and attach the prototypes."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("RTLFM_HIP_LIB") or LIB_PATH  # env override: A/B builds
    if not os.path.exists(p):
        raise FileNotFoundError(
            f"{p} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    # One HIP runtime per process: torch bundles its own libamdhip64.so.7 and
    # libhsa-runtime64 under the same sonames as /opt/rocm's.  If this library
    # is opened first it binds /opt/rocm's copy, torch then brings a second HSA
    # runtime and the device disappears for whoever comes second.  Importing
    # torch first (when it is installed) makes both share torch's copy.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(p)
    for name, res, args in (_SIGNATURES + _MONITOR_SIGNATURES + _AGC_SIGNATURES + _IQ_SIGNATURES + _SCAN_SIGNATURES + _SNAPSHOT_SIGNATURES
                            + _SLOTS_SIGNATURES + _CHANSNAP_SIGNATURES):
        if p != LIB_PATH and not hasattr(lib, name):
            continue  # an explicitly named other build (`path` or RTLFM_HIP_LIB: A/B against an earlier revision) may predate a symbol
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def strerror(code: int) -> str:
    try:
        return load().rtlfm_gpu_strerror(code).decode()
    except Exception:
        return os.strerror(-code) if code < 0 else "ok"


def check(code: int, what: str) -> int:
    if code < 0:
        raise RtlfmError(code, what)
    return code


def snapshot_info(path: str):
    """rtlfm_snapshot_info: (RtlfmCfg, stream count) of a snapshot file that passes every check of its format (the
    checksum included); RtlfmError otherwise (-EILSEQ for a damaged file).  Needs no GPU."""
    cfg, n = RtlfmCfg(), C.c_int()
    check(load().rtlfm_snapshot_info(os.fsencode(path), C.byref(cfg), C.byref(n)), "rtlfm_snapshot_info")
    return cfg, n.value


def chansnap_info(path: str):
    """rtlfm_chansnap_info: (RtlfmChansnapHdr, RtlfmCfg) of a channel snapshot (include/rtlfm_chansnap.h) that passes every
    check of its format, the checksum included; RtlfmError otherwise (-EILSEQ for a damaged file or one of the other
    kind).  Needs no GPU."""
    hdr, cfg = RtlfmChansnapHdr(), RtlfmCfg()
    check(load().rtlfm_chansnap_info(os.fsencode(path), C.byref(hdr), C.byref(cfg)), "rtlfm_chansnap_info")
    return hdr, cfg


def chansnap_read(path: str) -> dict:
    """rtlfm_chansnap_read: the whole file as a dict - ``hdr``, ``cfg``, ``steps`` uint32 [n], ``fir_taps`` / ``bank_taps``
    int16, ``bins`` int32 [sources, per_source] (empty without a bank), ``states`` (a ctypes array of RtlfmStreamState),
    ``hist`` uint8 [sources, 8192] and ``dc`` uint32 [sources, 16] (empty where the file holds none).  Needs no GPU."""
    import numpy as np
    hdr, cfg = chansnap_info(path)
    n, nsrc = hdr.nstreams, hdr.nstreams // hdr.per_source
    hist = bool(hdr.flags & CHANSNAP_FLAG_HISTORY)
    dc = hist and bool(hdr.flags & CHANSNAP_FLAG_SOURCE_DC)
    out = dict(cfg=RtlfmCfg(), steps=np.zeros(n, np.uint32), fir_taps=np.zeros(hdr.fir_ntaps, np.int16),
               bank_taps=np.zeros(hdr.bank_ntaps, np.int16), bins=np.zeros((nsrc if hdr.bank_K else 0, hdr.per_source), np.int32),
               states=(RtlfmStreamState * n)(), hist=np.zeros((nsrc if hist else 0, 2 * CHANSNAP_HIST), np.uint8),
               dc=np.zeros((nsrc if dc else 0, CHANSNAP_DC_PIECES), np.uint32))
    b = RtlfmChansnapBufs(cfg=C.addressof(out["cfg"]), states=C.addressof(out["states"]), cap_states=n)
    for k in ("steps", "fir_taps", "bank_taps", "bins", "hist", "dc"):
        setattr(b, k, out[k].ctypes.data)
        setattr(b, "cap_" + k, out[k].size)
    h2 = RtlfmChansnapHdr()
    check(load().rtlfm_chansnap_read(os.fsencode(path), C.byref(h2), C.byref(b)), "rtlfm_chansnap_read")
    out["hdr"] = h2
    return out


def chansnap_write(path: str, cfg: RtlfmCfg, per_source: int, pos: int, steps, states, fir_taps=None, fir_shift: int = 0, bank_K: int = 0,
                   bank_taps=None, bank_shift: int = 0, bins=None, hist=None, dc=None, source_dc: bool = False):
    """rtlfm_chansnap_write: a channel snapshot from its parts (``states``: a ctypes array of RtlfmStreamState; ``hist`` is
    needed exactly where a filter or a bank is given, ``dc = None`` with ``source_dc`` writes "none subtracted").  The
    file appears whole or not at all.  Needs no GPU."""
    import numpy as np
    st = np.ascontiguousarray(steps, np.uint32)
    ft = np.ascontiguousarray([] if fir_taps is None else fir_taps, np.int16)
    bt = np.ascontiguousarray([] if bank_taps is None else bank_taps, np.int16)
    bn = np.ascontiguousarray([] if bins is None else bins, np.int32)
    hs = np.ascontiguousarray([] if hist is None else hist, np.uint8)
    dw = None if dc is None else np.ascontiguousarray(dc, np.uint32)
    if not isinstance(states, C.Array):
        states = (RtlfmStreamState * len(states))(*states)
    n = len(states)
    has_hist = ft.size > 0 or bank_K > 0
    nsrc = n // per_source if per_source > 0 else 0
    if st.size != n or (bank_K and bn.size != n) or (has_hist and hs.size != nsrc * 2 * CHANSNAP_HIST) or \
            (dw is not None and dw.size != nsrc * CHANSNAP_DC_PIECES):
        raise ValueError("chansnap_write: a section's size does not follow from the header")
    hdr = RtlfmChansnapHdr(pos=pos, nstreams=n, per_source=per_source,
                           flags=(CHANSNAP_FLAG_SOURCE_DC if source_dc else 0) | (CHANSNAP_FLAG_HISTORY if has_hist else 0),
                           fir_ntaps=ft.size, fir_shift=fir_shift, bank_K=bank_K, bank_ntaps=bt.size if bank_K else 0,
                           bank_shift=bank_shift if bank_K else 0)
    parts = RtlfmChansnapParts(cfg=C.addressof(cfg), steps=st.ctypes.data, fir_taps=ft.ctypes.data if ft.size else None,
                               bank_taps=bt.ctypes.data if bt.size else None, bins=bn.ctypes.data if bn.size else None,
                               states=C.addressof(states), hist=hs.ctypes.data if hs.size else None,
                               dc=None if dw is None else dw.ctypes.data)
    check(load().rtlfm_chansnap_write(os.fsencode(path), C.byref(hdr), C.byref(parts)), "rtlfm_chansnap_write")
