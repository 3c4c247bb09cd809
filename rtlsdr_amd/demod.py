"""Host-side mirror of rtl_fm's per-buffer interface over the C ABI.

Names follow the reference (src/rtl_fm.c): ``rtlsdr_callback`` is what
``rtlsdr_read_async`` calls with a u8 IQ buffer (:1274), ``full_demod`` turns
the queued buffers into PCM (:1179), and what the output thread would
``fwrite`` (:1400) comes back from ``fetch``.  All arithmetic happens in the
HIP library; this class only moves pointers.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import capi
from .capi import RtlfmCfg, RtlfmStreamState, check


class GpuDemod:
    """``nstreams`` independent rtl_fm demodulators sharing one configuration."""

    def __init__(self, cfg: RtlfmCfg, nstreams: int = 1, device: int = 0, lib_path: str | None = None,
                 options: dict | None = None, squelch_gate: bool | None = None, conseq_squelch: int | None = None,
                 source_dc: bool | None = None, source_stats: bool | None = None, source_health: bool | None = None,
                 source_iq: bool | None = None):
        self.lib = capi.load(lib_path)  # lib_path: another build of the library (A/B measurements)
        self.cfg = cfg
        self.nstreams = nstreams
        self.device = device
        h = C.c_void_p()
        check(self.lib.rtlfm_gpu_create(C.byref(cfg), nstreams, device, C.byref(h)), "rtlfm_gpu_create")
        self._h = h
        self._per_source = 0  # channels (set_channels): 0 = off
        self._path = 0        # set_path
        for k, v in (options or {}).items():
            self.set_option(k, v)
        # the scanner's squelch gate (include/rtlfm_hip.h, rtlfm_gpu_gate): off unless asked for
        if conseq_squelch is not None:
            self.set_option("conseq_squelch", conseq_squelch)
        if squelch_gate is not None:
            self.set_option("squelch_gate", int(bool(squelch_gate)))
        # the raw DC block per source in front of the channel front ends (include/rtlfm_hip.h, option source_dc)
        if source_dc is not None:
            self.set_option("source_dc", int(bool(source_dc)))
        # the ADC statistics and the input health per source (include/rtlfm_hip.h, options source_stats / source_health)
        if source_stats is not None:
            self.set_option("source_stats", int(bool(source_stats)))
        if source_health is not None:
            self.set_option("source_health", int(bool(source_health)))
        # IQ balance per source, measured and applied on the device (include/rtlfm_hip.h, option source_iq)
        if source_iq is not None:
            self.set_option("source_iq", int(bool(source_iq)))

    # -- lifetime ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self.lib.rtlfm_gpu_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the callback boundary ---------------------------------------------
    @property
    def sources(self) -> int:
        """Rows of the ring's input side - what ``stream`` of ``rtlsdr_callback`` counts: the streams, or, with the option
        ``source_ring`` while channels are on, the wideband sources (``nstreams // per_source``).  Results are per stream
        (= per channel) either way."""
        if self._per_source and self.get_option("source_ring"):
            return self.nstreams // self._per_source
        return self.nstreams

    def rtlsdr_callback(self, buf, stream: int = 0):
        """What rtlsdr_read_async's callback does with (buf, len, ctx).  ``stream`` is the row of the ring: the stream,
        or - channels on, option ``source_ring`` set - the SOURCE in ``range(self.sources)``; ``full_demod`` then turns
        every source's queued buffers into all of its channels, and ``fetch*`` hand back one row per stream.  Every
        source must have delivered the same number of buffers, and buffer k the same length on every source
        (``-ERANGE`` otherwise: the channels share one sample counter).  Without ``source_ring`` the ring is refused
        while channels are on (``-ENOTSUP``)."""
        a = np.ascontiguousarray(buf, dtype=np.uint8)
        check(self.lib.rtlfm_gpu_push(self._h, stream, a.ctypes.data, a.size), "rtlfm_gpu_push")

    push = rtlsdr_callback

    def full_demod(self):
        check(self.lib.rtlfm_gpu_run(self._h), "rtlfm_gpu_run")

    run = full_demod

    def run_begin(self) -> int:
        """rtlfm_gpu_run_begin: take what the ring's filling half holds and flip the halves; returns buffers per stream
        (per source over the source ring) taken."""
        n = C.c_int()
        check(self.lib.rtlfm_gpu_run_begin(self._h, C.byref(n)), "rtlfm_gpu_run_begin")
        return n.value

    def run_end(self):
        """rtlfm_gpu_run_end: the transfer and the kernels of the run that _begin took."""
        check(self.lib.rtlfm_gpu_run_end(self._h), "rtlfm_gpu_run_end")

    def fetch(self, stream: int = 0) -> np.ndarray:
        cap = capi.load().rtlfm_result_cap(C.byref(self.cfg)) * max(1, self.cfg.max_blocks) + 16
        out = np.empty(cap, dtype=np.int16)
        n = C.c_int()
        check(self.lib.rtlfm_gpu_fetch(self._h, stream, out.ctypes.data, cap, C.byref(n)), "rtlfm_gpu_fetch")
        return out[:n.value].copy()

    def fetch_all(self):
        """(out int16 [nstreams, cap], lens int32 [nstreams]) of the last full_demod(): one transfer."""
        cap = capi.load().rtlfm_result_cap(C.byref(self.cfg)) * max(1, self.cfg.max_blocks) + 16
        out = np.empty((self.nstreams, cap), dtype=np.int16)
        lens = np.zeros(self.nstreams, dtype=np.int32)
        check(self.lib.rtlfm_gpu_fetch_all(self._h, out.ctypes.data, cap, lens.ctypes.data), "rtlfm_gpu_fetch_all")
        return out, lens

    def fetch_all_prev(self):
        """The same for the run BEFORE the last one (rtlfm_gpu_fetch_all_prev): does not wait for the run started since."""
        cap = capi.load().rtlfm_result_cap(C.byref(self.cfg)) * max(1, self.cfg.max_blocks) + 16
        out = np.empty((self.nstreams, cap), dtype=np.int16)
        lens = np.zeros(self.nstreams, dtype=np.int32)
        check(self.lib.rtlfm_gpu_fetch_all_prev(self._h, out.ctypes.data, cap, lens.ctypes.data), "rtlfm_gpu_fetch_all_prev")
        return out, lens

    def fetch_packed(self, prev: bool = False):
        """rtlfm_gpu_fetch_packed (``prev``: _fetch_packed_prev): ``(packed int16 [total], index)`` of a run made with the
        option ``pack_results`` at 1 or 2 - ``index`` a record array (``capi.PACKED_ROW``: offset, len, held) per stream,
        stream s's samples ``packed[offset : offset + len]``.  One small copy for the index, one for the samples."""
        fn = self.lib.rtlfm_gpu_fetch_packed_prev if prev else self.lib.rtlfm_gpu_fetch_packed
        index = np.zeros(self.nstreams, dtype=capi.PACKED_ROW)
        total = C.c_size_t()
        # room for the worst case (every row full, rounded up to 8): pages the copy does not reach are never touched
        cap = capi.load().rtlfm_result_cap(C.byref(self.cfg)) * max(1, self.cfg.max_blocks) + 16
        out = np.empty(self.nstreams * ((cap + 7) & ~7), dtype=np.int16)
        check(fn(self._h, out.ctypes.data, out.size, index.ctypes.data, C.byref(total)),
              "rtlfm_gpu_fetch_packed_prev" if prev else "rtlfm_gpu_fetch_packed")
        return out[:total.value], index

    # -- device-resident form ------------------------------------------------
    def result_cap(self, nblocks: int) -> int:
        c = self.lib.rtlfm_result_cap(C.byref(self.cfg)) * nblocks + 16
        return (c + 63) & ~63  # rows start on 128-byte lines: the front end's tile stores then cover whole lines

    def run_device(self, d_iq_ptr: int, stream_stride: int, nblocks: int, d_out_ptr: int,
                   out_stride: int, d_out_len_ptr: int = 0):
        check(self.lib.rtlfm_gpu_run_device(self._h, d_iq_ptr, stream_stride, nblocks, d_out_ptr,
                                            out_stride, d_out_len_ptr or None), "rtlfm_gpu_run_device")

    def run_torch(self, iq, out=None, out_len=None):
        """iq: torch uint8 [nstreams, nblocks*block_len] on this device.
        Returns (out int16 [nstreams, cap], out_len int32 [nstreams]).

        Stream contract: the library launches on the handle's own stream.  This method orders it
        after torch's current stream (whatever produced ``iq`` and allocated / zeroed the outputs)
        and makes torch's current stream wait for the library's kernels before it returns, so the
        results can be used from torch without ``sync()`` and the caching allocator cannot hand
        ``out`` to someone else while the kernels still write it.  ``run_device`` does neither."""
        import torch
        rows = self.nstreams // self._per_source if self._per_source else self.nstreams  # channels on: one row per source
        assert iq.dtype == torch.uint8 and iq.is_cuda and iq.dim() == 2 and iq.shape[0] == rows
        assert iq.stride(1) == 1
        L = int(self.cfg.block_len)
        nb = iq.shape[1] // L
        cap = self.result_cap(nb)
        if out is None:
            out = torch.empty((self.nstreams, cap), dtype=torch.int16, device=iq.device)
        if out_len is None:
            out_len = torch.zeros(self.nstreams, dtype=torch.int32, device=iq.device)
        ts = torch.cuda.current_stream(iq.device).cuda_stream or None
        check(self.lib.rtlfm_gpu_wait_for(self._h, ts), "rtlfm_gpu_wait_for")
        self.run_device(iq.data_ptr(), iq.stride(0), nb, out.data_ptr(), out.stride(0), out_len.data_ptr())
        check(self.lib.rtlfm_gpu_release_to(self._h, ts), "rtlfm_gpu_release_to")
        return out, out_len

    def levels(self, stream: int = 0) -> np.ndarray:
        """rms() of the decimated IQ per buffer of the last run (needs squelch_level or report_levels)."""
        out = np.zeros(max(1, self.cfg.max_blocks), dtype=np.int32)
        n = C.c_int()
        check(self.lib.rtlfm_gpu_levels(self._h, stream, out.ctypes.data, out.size, C.byref(n)), "rtlfm_gpu_levels")
        return out[:n.value].copy()

    def levels_all(self) -> np.ndarray:
        """int32 [nstreams, buffers of the last run]: every stream's levels in one copy."""
        cap = max(1, self.cfg.max_blocks)
        out = np.zeros((self.nstreams, cap), dtype=np.int32)
        n = C.c_int()
        check(self.lib.rtlfm_gpu_levels_all(self._h, out.ctypes.data, cap, C.byref(n)), "rtlfm_gpu_levels_all")
        return out[:, :n.value].copy()

    def input_stats(self, stream: int = 0) -> np.ndarray:
        """The ADC statistics of the raw bytes (src/rtl_fm.c:1302-1324) of every buffer of the last run for ``stream``:
        a record array with pow_sum, pow_count, max, step.  Needs ``set_option("input_stats", 1)`` before the run."""
        out = np.zeros(max(1, self.cfg.max_blocks), dtype=capi.INPUT_STAT_DTYPE)
        n = C.c_int()
        check(self.lib.rtlfm_gpu_input_stats(self._h, stream, out.ctypes.data, out.size, C.byref(n)), "rtlfm_gpu_input_stats")
        return out[:n.value].copy()

    def input_stats_all(self) -> np.ndarray:
        """The same for every stream in one copy: records [nstreams, buffers of the last run]."""
        cap = max(1, self.cfg.max_blocks)
        out = np.zeros((self.nstreams, cap), dtype=capi.INPUT_STAT_DTYPE)
        n = C.c_int()
        check(self.lib.rtlfm_gpu_input_stats_all(self._h, out.ctypes.data, cap, C.byref(n)), "rtlfm_gpu_input_stats_all")
        return out[:, :n.value].copy()

    def input_health(self, stream: int = 0) -> np.ndarray:
        """The overload / high-level / continuity records (include/rtlfm_hip.h) of every buffer of the last run for
        ``stream``: a record array with overload, high, lost, first, last.  Needs ``set_option("input_health", 1)``
        before the run."""
        out = np.zeros(max(1, self.cfg.max_blocks), dtype=capi.INPUT_HEALTH_DTYPE)
        n = C.c_int()
        check(self.lib.rtlfm_gpu_input_health(self._h, stream, out.ctypes.data, out.size, C.byref(n)), "rtlfm_gpu_input_health")
        return out[:n.value].copy()

    def input_health_all(self) -> np.ndarray:
        """The same for every stream in one copy: records [nstreams, buffers of the last run]."""
        cap = max(1, self.cfg.max_blocks)
        out = np.zeros((self.nstreams, cap), dtype=capi.INPUT_HEALTH_DTYPE)
        n = C.c_int()
        check(self.lib.rtlfm_gpu_input_health_all(self._h, out.ctypes.data, cap, C.byref(n)), "rtlfm_gpu_input_health_all")
        return out[:, :n.value].copy()

    def _source_records(self, name: str, dtype, source: int | None) -> np.ndarray:
        cap = max(1, self.cfg.max_blocks)
        n = C.c_int()
        if source is None:
            nsrc = self.nstreams // self._per_source if self._per_source else self.nstreams
            out = np.zeros((nsrc, cap), dtype=dtype)
            check(getattr(self.lib, name + "_all")(self._h, out.ctypes.data, cap, C.byref(n)), name + "_all")
            return out[:, :n.value].copy()
        out = np.zeros(cap, dtype=dtype)
        check(getattr(self.lib, name)(self._h, int(source), out.ctypes.data, cap, C.byref(n)), name)
        return out[:n.value].copy()

    def source_stats(self, source: int = 0) -> np.ndarray:
        """``input_stats``' records for the raw bytes of SOURCE ``source`` of the last run that channels took: needs
        channels on and ``set_option("source_stats", 1)`` before the run (``RtlfmError`` with -ENODATA otherwise)."""
        return self._source_records("rtlfm_gpu_source_stats", capi.INPUT_STAT_DTYPE, source)

    def source_stats_all(self) -> np.ndarray:
        """The same for every source in one copy: records [sources, buffers of the last run]."""
        return self._source_records("rtlfm_gpu_source_stats", capi.INPUT_STAT_DTYPE, None)

    def source_health(self, source: int = 0) -> np.ndarray:
        """``input_health``'s records for the raw bytes of SOURCE ``source`` of the last run that channels took: needs
        channels on and ``set_option("source_health", 1)`` before the run."""
        return self._source_records("rtlfm_gpu_source_health", capi.INPUT_HEALTH_DTYPE, source)

    def source_health_all(self) -> np.ndarray:
        """The same for every source in one copy: records [sources, buffers of the last run]."""
        return self._source_records("rtlfm_gpu_source_health", capi.INPUT_HEALTH_DTYPE, None)

    def source_iq_sums(self, source: int = 0) -> np.ndarray:
        """The second moments of the RAW bytes of SOURCE ``source`` per buffer of the last run that channels took (records of
        ``capi.IQ_SUMS_DTYPE``): needs channels on and ``set_option("source_iq", 1)`` before the run."""
        return self._source_records("rtlfm_gpu_source_iq_sums", capi.IQ_SUMS_DTYPE, source)

    def source_iq_sums_all(self) -> np.ndarray:
        """The same for every source in one copy: records [sources, buffers of the last run]."""
        return self._source_records("rtlfm_gpu_source_iq_sums", capi.IQ_SUMS_DTYPE, None)

    def set_source_iq(self, coef):
        """rtlfm_gpu_set_source_iq: the Q14 coefficients (a, b, p, q) of every source, int16 [sources, 4].  No wait: runs
        already queued use the old coefficients, later runs the new."""
        c = np.ascontiguousarray(coef, dtype=np.int16)
        nsrc = self.nstreams // self._per_source if self._per_source else 0
        if self._per_source and c.size != nsrc * 4:
            raise ValueError(f"four coefficients per source: {nsrc} sources, not {c.shape}")
        check(self.lib.rtlfm_gpu_set_source_iq(self._h, c.ctypes.data), "rtlfm_gpu_set_source_iq")

    def get_source_iq(self) -> np.ndarray:
        """rtlfm_gpu_get_source_iq: the coefficients as they rule now, int16 [sources, 4]."""
        nsrc = self.nstreams // self._per_source if self._per_source else self.nstreams
        out = np.zeros((nsrc, 4), dtype=np.int16)
        check(self.lib.rtlfm_gpu_get_source_iq(self._h, out.ctypes.data, out.size), "rtlfm_gpu_get_source_iq")
        return out

    def gate(self, stream: int | None = None) -> np.ndarray:
        """The squelch gate's records of the last run (``set_option("squelch_gate", 1)`` before it): a record array with
        hits_after and emit per buffer - of ``stream``, or [nstreams, buffers] for every stream in one copy."""
        cap = max(1, self.cfg.max_blocks)
        n = C.c_int()
        if stream is None:
            out = np.zeros((self.nstreams, cap), dtype=capi.GATE_REC_DTYPE)
            check(self.lib.rtlfm_gpu_gate_all(self._h, out.ctypes.data, cap, C.byref(n)), "rtlfm_gpu_gate_all")
            return out[:, :n.value].copy()
        out = np.zeros(cap, dtype=capi.GATE_REC_DTYPE)
        check(self.lib.rtlfm_gpu_gate(self._h, stream, out.ctypes.data, cap, C.byref(n)), "rtlfm_gpu_gate")
        return out[:n.value].copy()

    def mute(self, stream: int, nbytes: int):
        """rtlfm_gpu_mute: the next ``nbytes`` that ``stream`` hands over read as 127 (the callback's mute after a retune)."""
        check(self.lib.rtlfm_gpu_mute(self._h, stream, int(nbytes)), "rtlfm_gpu_mute")

    # -- channels: K channels per wideband source ------------------------------------
    def set_channels(self, per_source: int, steps=None, shifts_hz=None, capture_rate: int | None = None):
        """rtlfm_gpu_set_channels: stream s becomes channel ``s % per_source`` of source ``s // per_source``, mixed down by
        ``steps[s]`` (uint32 phase steps), or by ``channel_step(shifts_hz[s], capture_rate)`` with
        ``shifts_hz[s] = channel_freq - capture_freq`` (how far above the sources' tuned frequency the channel lies).  ``per_source = 0`` switches channels off.  While they are on,
        ``run_torch`` / ``run_device`` take ``nstreams // per_source`` input rows (include/rtlfm_hip.h has the rest)."""
        if per_source == 0:
            check(self.lib.rtlfm_gpu_set_channels(self._h, 0, None), "rtlfm_gpu_set_channels")
            self._per_source = 0
            return
        if steps is None:
            if shifts_hz is None or capture_rate is None:
                raise ValueError("set_channels needs steps, or shifts_hz and capture_rate")
            steps = [channel_step(int(f), int(capture_rate)) for f in shifts_hz]
        st = np.ascontiguousarray(steps, dtype=np.uint32)
        if st.shape != (self.nstreams,):
            raise ValueError(f"one step per stream: {self.nstreams}, not {st.shape}")
        check(self.lib.rtlfm_gpu_set_channels(self._h, int(per_source), st.ctypes.data), "rtlfm_gpu_set_channels")
        self._per_source = int(per_source)

    def channels_seek(self, pos: int):
        """rtlfm_gpu_channels_seek: the complex samples the sources have delivered so far (what the NCO phase counts from)."""
        check(self.lib.rtlfm_gpu_channels_seek(self._h, int(pos)), "rtlfm_gpu_channels_seek")

    def channels_tell(self) -> int:
        pos = C.c_uint64()
        check(self.lib.rtlfm_gpu_channels_tell(self._h, C.byref(pos)), "rtlfm_gpu_channels_tell")
        return pos.value

    def set_channel_filter(self, taps=None, shift: int = 0):
        """rtlfm_gpu_set_channel_filter: int16 ``taps`` and ``shift`` in the boxcar's place while channels are on -
        ``sat16((sum taps[j] m[e - j] + r) >> shift)`` at the samples the boxcar emits at (``channel_lowpass`` makes a
        set).  ``None`` or no taps removes the filter.  Clears the filter's history."""
        t = np.ascontiguousarray([] if taps is None else taps, dtype=np.int16)
        if t.ndim != 1:
            raise ValueError("taps: one dimension")
        check(self.lib.rtlfm_gpu_set_channel_filter(self._h, t.ctypes.data if t.size else None, int(t.size), int(shift) if t.size else 0),
              "rtlfm_gpu_set_channel_filter")

    def channel_filter(self):
        """rtlfm_gpu_get_channel_filter: ``(taps, shift)`` as set; ``(empty, 0)`` without a filter."""
        out = np.zeros(capi.CHANNEL_MAX_TAPS, dtype=np.int16)
        n, sh = C.c_int(), C.c_int()
        check(self.lib.rtlfm_gpu_get_channel_filter(self._h, out.ctypes.data, out.size, C.byref(n), C.byref(sh)), "rtlfm_gpu_get_channel_filter")
        return out[:n.value].copy(), sh.value

    def set_channel_bank(self, K: int, taps=None, shift: int = 0, bins=None):
        """rtlfm_gpu_set_channel_bank: channel ``c`` of every source becomes bin ``bins[c]`` of a ``K``-point fix_fft over
        the ``K`` polyphase sums of int16 ``taps`` (``v_r = sat16((u_r + rnd) >> shift)``), in the mixer paths' place while
        channels are on.  ``bins = None`` is the identity (``per_source == K``).  ``K = 0`` removes the bank.  Clears the
        bank's history."""
        if not K:
            check(self.lib.rtlfm_gpu_set_channel_bank(self._h, 0, None, None, 0, 0), "rtlfm_gpu_set_channel_bank")
            return
        t = np.ascontiguousarray([] if taps is None else taps, dtype=np.int16)
        if t.ndim != 1:
            raise ValueError("taps: one dimension")
        b = None
        if bins is not None:
            b = np.ascontiguousarray(bins, dtype=np.int32)
            if b.shape != (self._per_source,):
                raise ValueError(f"one bin per channel of a source: {self._per_source}, not {b.shape}")
        check(self.lib.rtlfm_gpu_set_channel_bank(self._h, int(K), None if b is None else b.ctypes.data, t.ctypes.data if t.size else None,
                                                  int(t.size), int(shift)), "rtlfm_gpu_set_channel_bank")

    def get_channel_bank(self):
        """rtlfm_gpu_get_channel_bank: ``(K, bins, taps, shift)`` as set; ``(0, empty, empty, 0)`` without a bank."""
        bins = np.zeros(max(self._per_source, 1), dtype=np.int32)
        taps = np.zeros(capi.BANK_MAX_TAPS, dtype=np.int16)
        K, n, sh = C.c_int(), C.c_int(), C.c_int()
        check(self.lib.rtlfm_gpu_get_channel_bank(self._h, C.byref(K), bins.ctypes.data, bins.size, taps.ctypes.data, taps.size, C.byref(n),
                                                  C.byref(sh)), "rtlfm_gpu_get_channel_bank")
        return K.value, (bins[:self._per_source].copy() if K.value else bins[:0].copy()), taps[:n.value].copy(), sh.value

    def bank_survey(self, prev: bool = False):
        """rtlfm_gpu_bank_survey (``prev``: _bank_survey_prev): ``(power uint64 [sources, K], frames int32 [sources])`` of
        a run the bank took with the option ``bank_survey`` at 1 - every bin's summed ``Yi^2 + Yq^2`` over the frames the
        run emitted, selected or not.  ``RtlfmError`` with -ENODATA where that run carried none."""
        fn = self.lib.rtlfm_gpu_bank_survey_prev if prev else self.lib.rtlfm_gpu_bank_survey
        what = "rtlfm_gpu_bank_survey_prev" if prev else "rtlfm_gpu_bank_survey"
        nsrc = self.nstreams // self._per_source if self._per_source else self.nstreams
        K = C.c_int()
        frames = np.zeros(nsrc, dtype=np.int32)
        r = fn(self._h, None, 0, frames.ctypes.data, C.byref(K))  # (the size first: K is written with -ENOBUFS)
        if r < 0 and r != -105:
            check(r, what)
        power = np.zeros((nsrc, max(K.value, 1)), dtype=np.uint64)
        check(fn(self._h, power.ctypes.data, power.size, frames.ctypes.data, C.byref(K)), what)
        return power[:, :K.value], frames

    def set_channel_bins(self, bins):
        """rtlfm_gpu_set_channel_bins: ``bins`` int32 [sources, per_source] - channel c of source a becomes bin
        ``bins[a][c]`` of the bank that is set.  Nothing else changes, nothing is waited for: runs already queued use the
        old bins, later ones the new."""
        b = np.ascontiguousarray(bins, dtype=np.int32)
        if not self._per_source or b.size != self.nstreams:
            raise ValueError(f"bins: [sources, per_source] = {self.nstreams} entries, not {b.shape}")
        check(self.lib.rtlfm_gpu_set_channel_bins(self._h, b.ctypes.data), "rtlfm_gpu_set_channel_bins")

    def channel_bins(self) -> np.ndarray:
        """rtlfm_gpu_get_channel_bins: int32 [sources, per_source] as they rule now."""
        per = max(self._per_source, 1)
        out = np.zeros((self.nstreams // per, per), dtype=np.int32)
        check(self.lib.rtlfm_gpu_get_channel_bins(self._h, out.ctypes.data, out.size), "rtlfm_gpu_get_channel_bins")
        return out

    # -- state & plumbing ------------------------------------------------------
    def state_get(self, stream: int = 0) -> RtlfmStreamState:
        st = RtlfmStreamState()
        check(self.lib.rtlfm_gpu_state_get(self._h, stream, C.byref(st)), "rtlfm_gpu_state_get")
        return st

    def state_set(self, stream: int, st: RtlfmStreamState):
        check(self.lib.rtlfm_gpu_state_set(self._h, stream, C.byref(st)), "rtlfm_gpu_state_set")

    def state_get_all(self):
        """Every stream's record in one wait and one copy: a ctypes array of ``RtlfmStreamState`` [nstreams]."""
        out = (RtlfmStreamState * self.nstreams)()
        n = C.c_int()
        check(self.lib.rtlfm_gpu_state_get_all(self._h, out, self.nstreams, C.byref(n)), "rtlfm_gpu_state_get_all")
        return out

    def state_set_all(self, states):
        """The reverse: ``states`` holds exactly nstreams records (a ctypes array as state_get_all returns, or a sequence
        of ``RtlfmStreamState``)."""
        if not isinstance(states, C.Array):
            states = (RtlfmStreamState * len(states))(*states)
        check(self.lib.rtlfm_gpu_state_set_all(self._h, states, len(states)), "rtlfm_gpu_state_set_all")

    def move_from(self, src: "GpuDemod", map):
        """rtlfm_gpu_state_move: stream k of this handle takes the carried state and the owed mute of stream ``map[k]`` of
        ``src`` (-1: the initial state); ``src`` may be this handle itself.  One kernel launch for all streams."""
        m = np.ascontiguousarray(map, dtype=np.int32)
        check(self.lib.rtlfm_gpu_state_move(self._h, src._h, m.ctypes.data, m.size), "rtlfm_gpu_state_move")

    def save(self, path):
        """rtlfm_gpu_save: every stream's record and owed mute into a snapshot file (include/rtlfm_snapshot.h)."""
        check(self.lib.rtlfm_gpu_save(self._h, os.fsencode(path)), "rtlfm_gpu_save")

    def load(self, path):
        """rtlfm_gpu_load: the reverse, into a handle of the same stream count and configuration (max_blocks and
        report_levels may differ); a file that does not fit or is damaged changes nothing (RtlfmError)."""
        check(self.lib.rtlfm_gpu_load(self._h, os.fsencode(path)), "rtlfm_gpu_load")

    # -- the channel lifecycle: what a handle with channels on carries beyond the records -------------
    def channels_history(self):
        """rtlfm_gpu_channels_history_get: ``(bytes uint8 [sources, 8192], dc)`` - every source's last 4096 complex samples
        as raw bytes, oldest first (bytes 127 where cleared), and with the option ``source_dc`` on the history's bias words,
        uint32 [sources, 16] (else ``None``).  RtlfmError with -ENODATA when neither a filter nor a bank is set."""
        nsrc = self.nstreams // self._per_source if self._per_source else 0
        on = bool(self._per_source and self.get_option("source_dc"))
        out = np.zeros((nsrc, 2 * capi.CHANSNAP_HIST), dtype=np.uint8)
        dc = np.zeros((nsrc, capi.CHANSNAP_DC_PIECES), dtype=np.uint32)
        n = C.c_int()
        check(self.lib.rtlfm_gpu_channels_history_get(self._h, out.ctypes.data, out.size, dc.ctypes.data, dc.size, C.byref(n)),
              "rtlfm_gpu_channels_history_get")
        return out, (dc if on else None)

    def set_channels_history(self, bytes, dc=None):
        """rtlfm_gpu_channels_history_set: the inverse (``dc = None`` with ``source_dc`` on: none subtracted).  Behind
        ``channels_seek``, which clears the history - seek first."""
        b = np.ascontiguousarray(bytes, dtype=np.uint8)
        if b.ndim != 2 or b.shape[1] != 2 * capi.CHANSNAP_HIST:
            raise ValueError(f"history: [sources, {2 * capi.CHANSNAP_HIST}] bytes, not {b.shape}")
        d = None
        if dc is not None:
            d = np.ascontiguousarray(dc, dtype=np.uint32)
            if d.shape != (b.shape[0], capi.CHANSNAP_DC_PIECES):
                raise ValueError(f"dc: [sources, {capi.CHANSNAP_DC_PIECES}] words, not {d.shape}")
        check(self.lib.rtlfm_gpu_channels_history_set(self._h, b.ctypes.data, None if d is None else d.ctypes.data, b.shape[0]),
              "rtlfm_gpu_channels_history_set")

    def channels_move_from(self, src: "GpuDemod", source_map):
        """rtlfm_gpu_channels_move: source a of this handle takes the records, the history and the biases of source
        ``source_map[a]`` of ``src`` (-1: a source that joins from silence), and the handle takes ``src``'s pos; ``src`` may
        be this handle itself.  One kernel launch."""
        m = np.ascontiguousarray(source_map, dtype=np.int32)
        check(self.lib.rtlfm_gpu_channels_move(self._h, src._h, m.ctypes.data, m.size), "rtlfm_gpu_channels_move")

    def channels_save(self, path):
        """rtlfm_gpu_channels_save: records, pos, history and biases into a channel snapshot (include/rtlfm_chansnap.h)."""
        check(self.lib.rtlfm_gpu_channels_save(self._h, os.fsencode(path)), "rtlfm_gpu_channels_save")

    def channels_load(self, path):
        """rtlfm_gpu_channels_load: the reverse, into a handle set up alike (stream count, per_source, filter, bank,
        ``source_dc``, configuration); a file that does not fit or is damaged changes nothing (RtlfmError)."""
        check(self.lib.rtlfm_gpu_channels_load(self._h, os.fsencode(path)), "rtlfm_gpu_channels_load")

    def reset(self):
        check(self.lib.rtlfm_gpu_reset(self._h), "rtlfm_gpu_reset")

    def sync(self):
        check(self.lib.rtlfm_gpu_sync(self._h), "rtlfm_gpu_sync")

    def set_stream(self, hip_stream_ptr: int):
        check(self.lib.rtlfm_gpu_set_stream(self._h, hip_stream_ptr or None), "rtlfm_gpu_set_stream")

    def set_option(self, name: str, value: int):
        """rtlfm_gpu_set_option: tunables and A/B switches by name (include/rtlfm_hip.h)."""
        check(self.lib.rtlfm_gpu_set_option(self._h, name.encode(), int(value)), f"rtlfm_gpu_set_option({name})")

    def get_option(self, name: str) -> int:
        v = C.c_long()
        check(self.lib.rtlfm_gpu_get_option(self._h, name.encode(), C.byref(v)), f"rtlfm_gpu_get_option({name})")
        return v.value

    def clock_stamps(self):
        """uint64 [waves, 4] of the last stamped launch: shader clock first / last, 100 MHz counter first / last."""
        n = C.c_int()
        if self.lib.rtlfm_gpu_clock_stamps(self._h, None, 0, C.byref(n)) < 0:
            return None
        out = np.zeros((n.value, 4), dtype=np.uint64)
        check(self.lib.rtlfm_gpu_clock_stamps(self._h, out.ctypes.data, n.value, C.byref(n)), "rtlfm_gpu_clock_stamps")
        return out

    def set_path(self, path: int):
        check(self.lib.rtlfm_gpu_set_path(self._h, path), "rtlfm_gpu_set_path")
        self._path = min(path, 2)  # (3 / 4: path 2 with the pass-0 engine forced, which the option pass0_engine reads back)

    @property
    def last_path(self) -> int:
        return self.lib.rtlfm_gpu_last_path(self._h)

    @property
    def last_route(self) -> int:
        """Which front end the last run took (``capi.ROUTE_*``, enum rtlfm_route); 0 before the first run."""
        return self.get_option("last_route")

    @property
    def last_rest(self) -> int:
        """What followed it (``capi.REST_*``, enum rtlfm_rest)."""
        return self.get_option("last_rest")

    def run_route(self, nblocks: int, d_out_ptr: int = 0, out_stride: int | None = None, no_deemph_scan: bool = False):
        """The plan a run of ``nblocks`` buffers of this handle into rows at ``d_out_ptr``, ``out_stride`` int16 apart
        (default: ``result_cap(nblocks)``), will take - ``run_route()`` below with the handle's configuration, its stream
        count, its path and options as they are set now, and the channels that are on."""
        o = {k: self.get_option(k) for k in ("pass0_engine", "squelch_fused", "deep_rest", "deemph_four_pass", "deemph_sequential", "arb_serial")}
        channels = capi.CHANNELS_OFF
        if self._per_source:
            channels = (capi.CHANNELS_BANK if self.get_channel_bank()[0] else
                        capi.CHANNELS_FILTER if self.channel_filter()[0].size else capi.CHANNELS_MIXER)
        return run_route(self.cfg, self.nstreams, nblocks, d_out_ptr & 15, self.result_cap(nblocks) if out_stride is None else out_stride,
                         path=self._path, no_deemph_scan=int(no_deemph_scan), channels=channels, **o)

    def timing_enable(self, on: bool = True):
        check(self.lib.rtlfm_gpu_timing_enable(self._h, int(on)), "rtlfm_gpu_timing_enable")

    def clock_probe(self, on: bool = True):
        check(self.lib.rtlfm_gpu_clock_probe(self._h, int(on)), "rtlfm_gpu_clock_probe")

    def clock_read(self):
        """(mean shader MHz, span ms) of the last fused fifth_order launch, or None."""
        mhz, span = C.c_double(), C.c_double()
        r = self.lib.rtlfm_gpu_clock_read(self._h, C.byref(mhz), C.byref(span))
        if r < 0:
            return None
        return mhz.value, span.value

    def timing_read(self):
        ms = C.c_double()
        n = C.c_int()
        check(self.lib.rtlfm_gpu_timing_read(self._h, C.byref(ms), C.byref(n)), "rtlfm_gpu_timing_read")
        return ms.value, n.value


def optimal_settings(cfg: RtlfmCfg, freq: int, rate_in: int, min_capture_rate: int = 1000000,
                     use_fifth_order: bool = False, edge: int = 0):
    """optimal_settings() (src/rtl_fm.c:1407-1445); returns (capture_freq, capture_rate)."""
    cf, cr = C.c_uint32(), C.c_uint32()
    check(capi.load().rtlfm_optimal_settings(C.byref(cfg), freq, rate_in, min_capture_rate,
                                             int(use_fifth_order), edge, C.byref(cf), C.byref(cr)),
          "rtlfm_optimal_settings")
    return cf.value, cr.value


def run_route(cfg: RtlfmCfg, nstreams: int, nblocks: int, out_low_bits: int = 0, out_stride: int | None = None, **options):
    """``rtlfm_run_route``: the plan (``capi.RtlfmRoutePlan``: route, rest, last_path, ...) a run of ``nblocks`` buffers of
    ``nstreams`` streams takes - what ``last_route`` / ``last_rest`` / ``last_path`` read after it -, from the run's own
    planner (no GPU).  ``out_low_bits``: the low four bits of the first row's address; ``out_stride``: int16 between rows
    (default: ``GpuDemod.result_cap``'s).  ``options`` as ``capi.RtlfmRouteOpts``; RtlfmError where the run would be
    refused (-ENOTSUP: ``path=2`` without a fused form)."""
    if out_stride is None:
        out_stride = (capi.load().rtlfm_result_cap(C.byref(cfg)) * nblocks + 16 + 63) & ~63
    plan = capi.RtlfmRoutePlan()
    check(capi.load().rtlfm_run_route(C.byref(cfg), nstreams, nblocks, out_low_bits, out_stride,
                                      C.byref(capi.RtlfmRouteOpts.default(**options)), C.byref(plan)), "rtlfm_run_route")
    return plan


def deemph_a(rate_out: int, time_constant_us: int = 75) -> int:
    return capi.load().rtlfm_deemph_a(rate_out, time_constant_us)


def pack_device(d_rows_ptr: int, stride: int, d_lens_ptr: int, nstreams: int, d_packed_ptr: int, cap: int, d_index_ptr: int,
                d_total_ptr: int, device: int = 0, hip_stream_ptr: int = 0):
    """rtlfm_gpu_pack_device: row s - ``lens[s]`` int16 at ``d_rows + s * stride``, any int16 alignment - behind the rows
    before it in ``d_packed`` (16-byte aligned, ``cap`` int16), each row starting on a multiple of 8; the index
    (``capi.PACKED_ROW`` [nstreams]) and the total need (uint64, also where it exceeds ``cap``) on the device.
    Asynchronous on ``hip_stream_ptr`` (0: the default stream).  All pointers are device addresses."""
    check(capi.load().rtlfm_gpu_pack_device(int(device), d_rows_ptr, int(stride), d_lens_ptr, int(nstreams), d_packed_ptr, int(cap),
                                            d_index_ptr, d_total_ptr, hip_stream_ptr or None), "rtlfm_gpu_pack_device")


def channel_step(shift_hz: int, capture_rate: int) -> int:
    """rtlfm_channel_step: the NCO phase step (uint32) that brings a channel ``shift_hz = channel_freq - capture_freq`` above the tuned frequency to rest at
    ``capture_rate``: round_half_up(shift_hz * 2^32 / capture_rate) modulo 2^32, in integers.  Needs no GPU."""
    return int(capi.load().rtlfm_channel_step(int(shift_hz), int(capture_rate)))


def channel_lowpass(ntaps: int, cutoff: float, D: int):
    """rtlfm_channel_lowpass: ``(taps, shift)`` of a Hamming-windowed sinc with ``cutoff`` in cycles per capture sample and
    the boxcar's DC gain ``D`` (int16 taps, shift 14).  Needs no GPU."""
    out = np.zeros(max(int(ntaps), 1), dtype=np.int16)
    sh = C.c_int()
    check(capi.load().rtlfm_channel_lowpass(int(ntaps), float(cutoff), int(D), out.ctypes.data, C.byref(sh)), "rtlfm_channel_lowpass")
    return out, sh.value


def channel_bank_check(K: int, taps, shift: int) -> int:
    """rtlfm_channel_bank_check: 0, or a negative errno (-EINVAL for a bad K / taps / shift, -ERANGE where a branch's sum
    could overflow an int32).  Needs no GPU."""
    t = np.ascontiguousarray(taps, dtype=np.int16)
    return int(capi.load().rtlfm_channel_bank_check(int(K), t.ctypes.data if t.size else None, int(t.size), int(shift)))


def channel_table() -> np.ndarray:
    """rtlfm_channel_table: the NCO's table, int16 [1024, 2] = (cos, sin) in Q14.  Needs no GPU."""
    out = np.zeros((1024, 2), dtype=np.int16)
    check(capi.load().rtlfm_channel_table(out.ctypes.data), "rtlfm_channel_table")
    return out
