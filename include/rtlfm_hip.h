/*
 * rtlfm_hip.h — C ABI of the MI355X (gfx950) demodulation layer.
 *
 * This is the drop-in boundary for rtl_fm's per-buffer hot path.  It sits
 * exactly where the reference's async callback hands over its uint8 IQ buffer:
 *
 *   reference boundary                       replaced by
 *   ---------------------------------------  -------------------------------
 *   rtlsdr_read_async_cb_t                   rtlfm_gpu_push()
 *     (include/rtl-sdr.h:472)
 *   rtlsdr_callback body from the u8->i16    rtlfm_gpu_push() + rtlfm_gpu_run()
 *     convert on (src/rtl_fm.c:1326-1343)
 *   full_demod(&demod)                       rtlfm_gpu_run() / _run_device()
 *     (src/rtl_fm.c:1179-1272)
 *   memcpy into output_state + fwrite        rtlfm_gpu_fetch()
 *     (src/rtl_fm.c:1382-1388, 1400)
 *   struct demod_state fields that persist   rtlfm_stream_state via
 *     across blocks (src/rtl_fm.c:172-208)     rtlfm_gpu_state_get/_set()
 *   optimal_settings() + deemph_a            rtlfm_optimal_settings(),
 *     (src/rtl_fm.c:1407-1445, 1929-1931)      rtlfm_deemph_a()
 *
 * Conventions follow include/rtl-sdr.h: every entry point returns int,
 * 0 on success and a negative value on error (-errno style).  All pointers
 * are plain C pointers; there are no C++ or torch types in any signature.
 *
 * One handle batches `nstreams` independent IQ streams that share one
 * configuration (one rtl_fm command line) but each own their filter state.
 * Blocks of one stream are processed in order and never dropped; this is a
 * deliberate, documented difference from rtl_fm's lossy thread hand-off
 * (src/rtl_fm.c:1339-1343, 1368-1371).
 */
#ifndef RTLFM_HIP_H
#define RTLFM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTLFM_MAX_PASSES 10          /* lp_i_hist[10][6], src/rtl_fm.c:178 */
#define RTLFM_MAX_BLOCK_LEN 262144u  /* MAXIMUM_BUF_LENGTH, src/rtl_fm.c:88-90 */

/* demod_state.mode_demod (src/rtl_fm.c:200), selected by -M (src/rtl_fm.c:1820-1841) */
enum rtlfm_mode {
	RTLFM_MODE_FM = 0,   /* fm_demod  src/rtl_fm.c:932  */
	RTLFM_MODE_AM = 1,   /* am_demod  src/rtl_fm.c:961  */
	RTLFM_MODE_USB = 2,  /* usb_demod src/rtl_fm.c:978  */
	RTLFM_MODE_LSB = 3,  /* lsb_demod src/rtl_fm.c:990  */
	RTLFM_MODE_RAW = 4   /* raw_demod src/rtl_fm.c:1002 */
};

/* demod_state.custom_atan, selected by -A (src/rtl_fm.c:1811-1819) */
enum rtlfm_atan {
	RTLFM_ATAN_STD = 0,  /* polar_discriminant src/rtl_fm.c:842 */
	RTLFM_ATAN_FAST = 1, /* polar_disc_fast    src/rtl_fm.c:874 */
	RTLFM_ATAN_LUT = 2   /* polar_disc_lut     src/rtl_fm.c:894 */
};

/* What runs when rate_out2 > 0 (src/rtl_fm.c:1268-1271). */
enum rtlfm_resampler {
	RTLFM_RESAMPLE_LOW_PASS_REAL = 0, /* live path, src/rtl_fm.c:755-775 */
	RTLFM_RESAMPLE_ARBITRARY = 1      /* arbitrary_resample, src/rtl_fm.c:1114-1177
	                                     (call site commented out at :1270) */
};

/*
 * Per-handle configuration: the demod_state / dongle_state fields that are
 * constant while samples flow (src/rtl_fm.c:172-208).  Field names are the
 * reference's.
 */
typedef struct rtlfm_cfg {
	int32_t mode;               /* enum rtlfm_mode */
	int32_t downsample;         /* boxcar factor of low_pass() when passes == 0 */
	int32_t downsample_passes;  /* fifth_order() iterations, 0..10 */
	int32_t comp_fir_size;      /* 0 or 9 (generic_fir with cic_9_tables) */
	int32_t custom_atan;        /* enum rtlfm_atan */
	int32_t post_downsample;    /* low_pass_simple() step, 1 = off */
	int32_t deemph;             /* deemph_filter() on/off */
	int32_t deemph_a;           /* its divisor, see rtlfm_deemph_a() */
	int32_t rate_out;           /* "fast" of low_pass_real() */
	int32_t rate_out2;          /* <= 0: no resampler */
	int32_t resampler;          /* enum rtlfm_resampler */
	int32_t dc_block_audio;     /* dc_block_audio_filter() on/off */
	int32_t adc_block_const;    /* default 9 */
	int32_t dc_block_raw;       /* dc_block_raw_filter() on/off */
	int32_t rdc_block_const;    /* default 9 */
	int32_t offset_tuning;      /* 1: skip rotate16_neg90 (src/rtl_fm.c:1336) */
	int32_t output_scale;       /* am/usb/lsb gain from optimal_settings() */
	int32_t squelch_level;      /* 0 = off (src/rtl_fm.c:1204) */
	uint32_t block_len;         /* bytes per callback buffer = lp_len, multiple of 512 */
	int32_t max_blocks;         /* most blocks per stream one run may take */
	int32_t report_levels;      /* 1: keep the per-buffer rms() of the decimated IQ (what -L prints,
	                               src/rtl_fm.c:1217-1237) for rtlfm_gpu_levels() also when the squelch is off */
} rtlfm_cfg;

/*
 * Everything a stream carries from one block to the next
 * (src/rtl_fm.c:178-199 plus deemph_filter's function-static avg, :1013).
 */
typedef struct rtlfm_stream_state {
	int16_t lp_i_hist[RTLFM_MAX_PASSES][6];
	int16_t lp_q_hist[RTLFM_MAX_PASSES][6];
	int16_t droop_i_hist[9];
	int16_t droop_q_hist[9];
	int16_t pad_[2];
	int32_t now_r, now_j, prev_index;   /* low_pass() */
	int32_t pre_r, pre_j;               /* fm_demod() */
	int32_t now_lpr, prev_lpr_index;    /* low_pass_real() */
	int32_t deemph_avg;                 /* static int avg in deemph_filter() */
	int32_t dc_avg;                     /* dc_block_audio_filter() */
	int32_t dc_avgI, dc_avgQ;           /* dc_block_raw_filter() */
	int32_t squelch_hits;               /* src/rtl_fm.c:1208-1213 */
} rtlfm_stream_state;

typedef struct rtlfm_gpu rtlfm_gpu;

/* ---- host-side planner helpers (no GPU needed) -------------------------- */

/* rtlfm_cfg with demod_init()'s defaults (src/rtl_fm.c:1608-1640). */
void rtlfm_cfg_default(rtlfm_cfg *cfg);

/*
 * optimal_settings() (src/rtl_fm.c:1407-1445).  `use_fifth_order` is the
 * truthy downsample_passes placeholder set by -F (src/rtl_fm.c:1807-1810).
 * Writes downsample, downsample_passes, output_scale into cfg; returns the
 * capture rate through *capture_rate and the tuned frequency through
 * *capture_freq (either may be NULL).
 */
int rtlfm_optimal_settings(rtlfm_cfg *cfg, uint32_t freq, int32_t rate_in,
                           int32_t min_capture_rate, int use_fifth_order,
                           int edge, uint32_t *capture_freq,
                           uint32_t *capture_rate);

/* deemph_a = round(1/(1-exp(-1/(rate_out*tc)))) (src/rtl_fm.c:1929-1931). */
int32_t rtlfm_deemph_a(int32_t rate_out, int32_t time_constant_us);

/* Output samples one block yields, or -1 if it depends on carried state. */
int rtlfm_result_len(const rtlfm_cfg *cfg);
/* Upper bound of output samples per block (always defined). */
int rtlfm_result_cap(const rtlfm_cfg *cfg);

/* What rtlfm_gpu_create() accepts, without a GPU: 0, or the error it would return (-EINVAL; -EDOM
 * where the reference itself leaves its domain: see rtlfm_gpu_strerror; -E2BIG where max_blocks buffers of block_len
 * bytes are more than 2^31 - 1 complex samples per stream - a run is counted in int). */
int rtlfm_cfg_validate(const rtlfm_cfg *cfg);

/* ---- the GPU layer ------------------------------------------------------ */

/* Allocates per-stream state (demod_init() values) and work buffers on
 * HIP device `device`.  Fails with -ENODEV if there is no usable GPU: there
 * is no CPU fallback. */
int rtlfm_gpu_create(const rtlfm_cfg *cfg, int nstreams, int device,
                     rtlfm_gpu **out);
int rtlfm_gpu_destroy(rtlfm_gpu *h);

/*
 * The rtlsdr_read_async callback body (rtlsdr_callback, src/rtl_fm.c:1274-1344): append one buffer
 * of interleaved u8 I,Q for `stream`.  `iq` is owned by the caller and may be reused as soon as
 * this returns (the driver resubmits it, src/librtlsdr.c:2705-2707): the bytes are copied into a
 * pinned staging ring.  len is the transfer's actual_length (include/rtl-sdr.h:472): at most
 * cfg.block_len, a multiple of 512; short buffers are demodulated as the reference would (every
 * stage sees that buffer's own length).
 * Callable from the thread that runs rtlsdr_read_async, concurrently for different streams and
 * concurrently with rtlfm_gpu_run(): the ring has two halves, and a callback never waits for a
 * transfer or a kernel.  -ENOSPC when max_blocks buffers are already queued for the stream, -EBUSY while
 * the stream has a slot open between rtlfm_gpu_acquire() and rtlfm_gpu_commit() (one producer per stream).
 *
 * The ring and channels.  The ring's INPUT side - the pinned staging rows, their device copies, the counts - has one row
 * per stream.  While channels are on (rtlfm_gpu_set_channels) every call of the ring is refused with -ENOTSUP, unless the
 * handle's option source_ring is 1 (rtlfm_gpu_set_option; default 0): then the input side has one row per SOURCE,
 * rows = nstreams / per_source, and
 *   - `stream` of rtlfm_gpu_push / _acquire / _commit is the source's index in [0, rows), anything else -EINVAL;
 *   - rtlfm_gpu_run / _run_begin want the same number of buffers from every source (-EAGAIN otherwise) and buffer k of
 *     the run of ONE length on every source: pos is one counter per handle.  Lengths that differ between the sources
 *     are -ERANGE; nothing is taken, and rtlfm_gpu_reset empties the ring.  Short buffers whose lengths agree are run
 *     buffer by buffer through the channel front ends, each of which takes every length the ring accepts;
 *   - a run copies rows rows to the device and is one rtlfm_gpu_run_device on them: pos advances and the source
 *     history changes over once per run, ring runs and rtlfm_gpu_run_device calls may alternate on one handle, and
 *     rtlfm_gpu_channels_tell counts both;
 *   - the RESULT side stays per stream (= per channel): rtlfm_gpu_fetch / _fetch_all / _fetch_all_prev,
 *     rtlfm_gpu_levels*.
 * At 64 sources x 64 channels with 4 x 262144-byte buffers the ring pins 2 x 64 MiB instead of 2 x 4 GiB.  With
 * channels off the option changes nothing: rows = streams.  The option itself: -EINVAL for anything but 0 / 1; -EBUSY,
 * changing nothing, while a run is begun, a slot is open or buffers are queued.  rtlfm_gpu_set_channels with the option
 * on says -EBUSY while buffers are queued; otherwise both rebuild the input side at once for the new number of rows
 * (a failed allocation there is tried again by the next call of the ring).  Results of runs before such a call STAY
 * fetchable: the result side is not touched.  The mute, the statistics, the gate and the snapshots stay refused.
 */
int rtlfm_gpu_push(rtlfm_gpu *h, int stream, const uint8_t *iq, uint32_t len);

/*
 * The same boundary without the copy: the reference's zero-copy mode hands the callback the kernel's own
 * transfer buffers (use_zerocopy, src/librtlsdr.c:2744-2810); here the producer - a file reader, an rtl_tcp
 * receiver, any device layer that can write to a pointer - writes the samples of `stream`'s next buffer
 * straight into the pinned staging ring:
 *   rtlfm_gpu_acquire   *buf = where to write, *cap = cfg.block_len bytes of room; -ENOSPC when max_blocks
 *                       buffers are queued, -EBUSY while this stream's previous slot is still open
 *   rtlfm_gpu_commit    the first len bytes are a buffer (whole 512-byte packets, at most block_len;
 *                       len == 0 gives the slot back unused)
 * One open slot per stream; different streams concurrently, also while a run is in flight.
 * rtlfm_gpu_run() returns -EAGAIN while a slot is open (it sees every buffer whole or not at all).
 * rtlfm_gpu_push() stays for buffers that belong to someone else (librtlsdr's callback argument).
 */
int rtlfm_gpu_acquire(rtlfm_gpu *h, int stream, uint8_t **buf, uint32_t *cap);
int rtlfm_gpu_commit(rtlfm_gpu *h, int stream, uint32_t len);

/*
 * full_demod() for every queued buffer of every stream (all streams must have the same number
 * queued, else -EAGAIN and nothing changes).  Asynchronous: hands the filled half of the ring to
 * the GPU (async H2D on a copy stream, kernels behind it) and returns; callbacks go on filling the
 * other half, the next run's transfer overlaps this run's kernels.  One caller at a time.
 */
int rtlfm_gpu_run(rtlfm_gpu *h);
/*
 * The same in two steps.  _begin takes what the ring's filling half holds and flips the halves (-EAGAIN as above;
 * *taken, may be NULL = buffers per stream taken) - the only part of a run during which the producers must not
 * acquire or push; _end queues the transfer and the kernels (-EINVAL without a begun run; _begin says -EBUSY while one
 * is pending).  A caller that gates its producers itself (one that counts queued buffers: host/rtl_fm_hip.cpp) holds
 * its gate around _begin only, so that a callback waits for a flip, never for a transfer, a first run's allocations or
 * a kernel launch.  rtlfm_gpu_run() is _begin followed by _end.
 * A FAILED _end (a HIP error, -ENOTSUP) loses the buffers _begin took: the producers have been released, the carried state
 * has not moved on, so the stream now has a gap - what the filters carry no longer matches the input position.  The
 * handle stays usable, but the caller must start the streams afresh (rtlfm_gpu_reset, or rtlfm_gpu_state_set per stream)
 * before the next run if continuity matters; results of earlier runs stay fetchable.
 */
int rtlfm_gpu_run_begin(rtlfm_gpu *h, int *taken);
int rtlfm_gpu_run_end(rtlfm_gpu *h);

/*
 * The same on input already resident in device memory.
 *   d_iq        device pointer; stream s, block b starts at
 *               d_iq + s*stream_stride + b*block_len
 *   d_out       device pointer; stream s writes its concatenated block
 *               results at d_out + s*out_stride (int16 elements)
 *   d_out_len   device pointer to nstreams int32 (total samples per stream),
 *               may be NULL
 * Asynchronous on the handle's stream.
 * Any d_out / out_stride gives the same samples.  Rows that start on 128-byte lines (d_out 128-byte
 * aligned, out_stride a multiple of 64) let the front end's tile stores cover whole lines (1 % of the
 * launch); rows that are at least 16-byte aligned (out_stride a multiple of 8) let the resampler of
 * the -M wbfm tail store eight outputs at a time (17 % of that step).
 */
int rtlfm_gpu_run_device(rtlfm_gpu *h, const uint8_t *d_iq,
                         size_t stream_stride, int nblocks, int16_t *d_out,
                         size_t out_stride, int32_t *d_out_len);

/* Copy out what the last rtlfm_gpu_run() produced for `stream` (what the
 * reference fwrite()s, src/rtl_fm.c:1400).  Blocks until the run is done; the first fetch after a
 * run brings every stream's result over in one transfer, the others are host copies.  Results of a
 * run stay valid until the second run after it. */
int rtlfm_gpu_fetch(rtlfm_gpu *h, int stream, int16_t *out, int cap, int *n);
/* The same for all streams at once: stream s gets lens[s] samples at out + s * out_stride (int16
 * elements; rtlfm_result_cap() * max_blocks is always enough).  One device-to-host transfer. */
int rtlfm_gpu_fetch_all(rtlfm_gpu *h, int16_t *out, size_t out_stride, int32_t *lens);
/* The same for the run BEFORE the last one (-EAGAIN until there have been two).  Waits for that run only,
 * not for the one started since: run(k + 1) as soon as its buffers are in, then fetch_all_prev() for run k,
 * keeps consecutive runs' H2D copies back to back on the link. */
int rtlfm_gpu_fetch_all_prev(rtlfm_gpu *h, int16_t *out, size_t out_stride, int32_t *lens);

/*
 * rms() of the decimated IQ (`sr` in full_demod(), src/rtl_fm.c:1204-1237) of every buffer of the
 * last run for `stream`: what the squelch compared with squelch_level and what -L prints.  Needs
 * cfg.squelch_level or cfg.report_levels; a buffer whose rms() came out negative (the wrapped sum
 * of squares, see rms()) reads INT32_MIN as in the reference.  *n = buffers in the last run.
 */
int rtlfm_gpu_levels(rtlfm_gpu *h, int stream, int32_t *rms, int cap, int *n);
/* The same for every stream in one copy: stream s gets its *n levels at rms + s * cap (cap = room per stream). */
int rtlfm_gpu_levels_all(rtlfm_gpu *h, int32_t *rms, int cap, int *n);

/*
 * The ADC statistics rtlsdr_callback keeps on the raw bytes of a buffer BEFORE the byte-to-int16 conversion
 * (src/rtl_fm.c:1302-1324), one record per buffer:
 *   max        largest byte of the buffer (sampleMax, the overload check, :1305-1312)
 *   step       2; while (len >= 16384 * step) step += 2;                                   (:1314-1315)
 *   pow_sum    sum over i = 0, step, 2 step, ... < len of (buf[i]-127)^2 + (buf[i+1]-127)^2 (:1316-1321)
 *   pow_count  number of those i.  The reference adds (double)pow_sum / pow_count to samplePowSum per buffer;
 *              that and everything behind it is host work: include/rtlfm_monitor.h
 * Taken on the GPU over the full-rate input (k_input_stats, csrc/input_stats_kernel.h) by every run while the
 * option "input_stats" is 1 (default 0: nothing is launched, nothing allocated), whatever path the run takes;
 * integer and bit-identical to the reference.  rtlfm_gpu_input_stats: the last run's records of `stream`, the
 * contract of rtlfm_gpu_levels (-ENODATA while the option is off, -ENOBUFS when cap is too small, *n = buffers
 * of the last run that have records); _all: every stream in one copy, stream s at out + s * cap.
 */
typedef struct { uint32_t pow_sum; int32_t pow_count; int32_t max; int32_t step; } rtlfm_input_stat;
int rtlfm_gpu_input_stats(rtlfm_gpu *h, int stream, rtlfm_input_stat *out, int cap, int *n);
int rtlfm_gpu_input_stats_all(rtlfm_gpu *h, rtlfm_input_stat *out, int cap, int *n);
/* The same kernel as a standalone operator (no handle), asynchronous on hip_stream (NULL = the default stream): nstreams
 * rows of nblocks buffers of block_len bytes (a multiple of 512) at d_iq + s * stream_stride (16-byte aligned, a multiple of
 * 16), records [nstreams][nblocks] to device memory d_out (16-byte aligned).  nontemporal: 1 / 0 as input_stats_nt. */
int rtlfm_gpu_input_stats_device(int device, const uint8_t *d_iq, size_t stream_stride, uint32_t block_len, int nblocks,
                                 int nstreams, rtlfm_input_stat *d_out, int nontemporal, void *hip_stream);

/* Input health: what the reference's other three passes over the raw bytes of a transfer count, one record per buffer:
 *   overload   bytes equal to 0 or 255: softagc()'s `overload` (src/librtlsdr.c:3288-3327) and detect_overload()'s
 *              overload_count (src/rtl_tcp.c:235-244)
 *   high       bytes < 64 or > 191: softagc()'s high_level
 *   lost       what underrun_test() (src/rtl_test.c:121-151) adds to `lost` at positions 1 .. len-1 of this buffer; the
 *              term at position 0 needs the previous buffer's last byte and is added by the host engine
 *              (include/rtlfm_agc.h) from `first` and its own carried counter
 *   first,last buf[0] and buf[len-1];  pad_ is always 0
 * Taken on the GPU (k_input_health, csrc/input_health_kernel.h) by every run while the option "input_health" is 1
 * (default 0: nothing is launched, nothing allocated), whatever path the run takes, ragged runs per buffer over its own
 * length; integer and bit-identical to the reference.  With "input_stats" on as well ONE launch reads the input and
 * writes both record arrays.  The functions follow rtlfm_gpu_input_stats / _all / _device.
 */
typedef struct { uint32_t overload, high, lost; uint8_t first, last; uint16_t pad_; } rtlfm_input_health;
int rtlfm_gpu_input_health(rtlfm_gpu *h, int stream, rtlfm_input_health *out, int cap, int *n);
int rtlfm_gpu_input_health_all(rtlfm_gpu *h, rtlfm_input_health *out, int cap, int *n);
int rtlfm_gpu_input_health_device(int device, const uint8_t *d_iq, size_t stream_stride, uint32_t block_len, int nblocks,
                                  int nstreams, rtlfm_input_health *d_out, int nontemporal, void *hip_stream);
/* The launch a handle with both options on makes, without a handle: d_out as above and d_stats as
 * rtlfm_gpu_input_stats_device's d_out, from one read of the input. */
int rtlfm_gpu_input_health_stats_device(int device, const uint8_t *d_iq, size_t stream_stride, uint32_t block_len, int nblocks,
                                        int nstreams, rtlfm_input_health *d_out, rtlfm_input_stat *d_stats, int nontemporal,
                                        void *hip_stream);

/*
 * Scanning, the device side (csrc/scan_kernel.h; the host engine is include/rtlfm_scan.h).
 *
 * The squelch gate: the rule of the reference's demod thread (demod_thread_fn, src/rtl_fm.c:1366-1370) - while
 * squelch_hits > conseq_squelch a buffer is not handed to the output thread and the counter is held at
 * conseq_squelch + 1 - applied to every buffer of a run, for any max_blocks.  With the option "squelch_gate" on, one
 * more kernel (k_scan_gate) runs at the end of every run, whatever path the run takes, ragged runs included: it walks
 * the run's per-buffer rms() (what rtlfm_gpu_levels reads) from the carried squelch_hits, removes the held buffers'
 * results from each stream's PCM row (the emitted ones move down, in order) and writes the CLAMPED counter to the state:
 * rtlfm_gpu_fetch / _fetch_all / _fetch_all_prev and run_device's d_out_len then return exactly the bytes the reference
 * fwrite()s, and rtlfm_gpu_state_get reads what the reference's d->squelch_hits reads.  A held buffer still passes
 * through every filter (its state counts), as in the reference.
 * One record per (stream, buffer) of the last run: rtlfm_gpu_gate / _gate_all, the contract of rtlfm_gpu_levels / _all
 * (-ENODATA while the option is off, -ENOBUFS when cap is too small).
 */
typedef struct { int32_t hits_after; uint8_t emit; uint8_t pad[3]; } rtlfm_gate_rec;
int rtlfm_gpu_gate(rtlfm_gpu *h, int stream, rtlfm_gate_rec *out, int cap, int *n);
int rtlfm_gpu_gate_all(rtlfm_gpu *h, rtlfm_gate_rec *out, int cap, int *n);
/*
 * The hop mute (rtlsdr_callback, src/rtl_fm.c:1289-1296): the next nbytes that `stream` hands over through
 * rtlfm_gpu_push / _acquire + _commit read as 127, across buffers and across runs (the handle keeps what is left per
 * stream; calling again REPLACES the pending count, as `dongle.mute = ...` does).  Applied by the next run(s) to the
 * handle's own device copy of the input behind the transfer (k_scan_mute: one launch, only in runs where a count is
 * pending), in front of the input statistics / health readers and the front end, which see the muted bytes as the
 * reference's callback does.  The caller's buffers and the pinned ring are not written.  Call it from the thread that
 * runs the handle (rtlfm_gpu_run*), not from a producer.
 * rtlfm_gpu_run_device takes const input and never mutes: -EBUSY while a count is pending.
 */
int rtlfm_gpu_mute(rtlfm_gpu *h, int stream, uint32_t nbytes);
/* The same kernel on input that already lives on the device (the caller's own buffer, as rtlfm_gpu_rotate_90_u8): of
 * every row s at d_iq + s * stream_stride (any alignment) the first min(mute_bytes[s], row_bytes) bytes become 127.
 * mute_bytes is HOST memory.  Ordered on hip_stream (NULL = the default stream) and waits for it before it returns. */
int rtlfm_gpu_mute_device(int device, uint8_t *d_iq, size_t stream_stride, int nstreams, size_t row_bytes,
                          const uint32_t *mute_bytes, void *hip_stream);

/*
 * Packed results (csrc/pack_kernel.h): fetch what the streams hold, not max(lens) x nstreams.
 *
 * rtlfm_gpu_fetch_all / _fetch_all_prev copy a rectangle as wide as the longest row.  With the option "pack_results"
 * at 1 or 2 every ring run (rtlfm_gpu_run / _run_end) ends with two more launches on the handle's stream - k_pack_plan
 * and k_pack_copy, behind the run's last kernel, behind its audio tail where it left one and behind the squelch gate
 * where that is on (under verify_twice once, behind the comparison) - which write every stream's row, one behind the
 * other, into a packed buffer of the ring half the run used, and an index of it.  Both are allocated on first use,
 * sized for the worst case, and freed with the handle or when the option goes back to 0.  The pack is read-only towards
 * the run: rows, lengths, levels and the carried state are not written, and rtlfm_gpu_fetch / _fetch_all /
 * _fetch_all_prev return what they return without it.  With 0 (default) nothing is launched and nothing allocated.
 *
 *   rtlfm_packed_row   offset: where the row starts, in int16 from the start of the packed buffer, always a multiple
 *                      of 8 (a 16-byte boundary; an empty row: where the next one starts); len: its samples; held: buffers
 *                      of this run the rule left out (mode 2; 0 in mode 1).  The elements between a row's last sample and
 *                      the next row's start are 0: the packed form of a run is the same byte for byte every time.
 *
 *   mode 1   a row's packed length is its result length (what rtlfm_gpu_fetch_all writes to lens): every
 *            configuration, every path, ragged runs, with or without "squelch_gate", with channels on.
 *   mode 2   additionally every buffer the reference's demod thread would not hand to its output thread is left out
 *            (demod_thread_fn, src/rtl_fm.c:1366-1370: held while squelch_hits > conseq_squelch, the counter then kept at
 *            conseq_squelch + 1).  The counter moves as full_demod() moves it (:1206-1213: a level below the squelch
 *            adds one, any other zeroes it, a negative level changes nothing), so "hits > conseq" holds for exactly the
 *            same buffers whether or not the CARRIED counter was ever clamped: the walk starts from the squelch_hits
 *            the run started from and clamps a local copy only.  It reads the run's levels (rtlfm_gpu_levels),
 *            cfg.squelch_level and the option "conseq_squelch"; buffer b's extent in its row is the one the squelch of
 *            that run used (the gate's).  This is the squelch gate's output without its writes: allowed with channels
 *            on, with every channel front end and on both paths, where "squelch_gate" is refused.
 *            Refused, the option then staying what it was: -EINVAL without a squelch (cfg.squelch_level == 0) and while
 *            "squelch_gate" is on (and "squelch_gate" while mode 2 is on: the rows would already be compacted);
 *            -ENOTSUP behind a resampler, post_downsample > 1 or a buffer the fifth_order passes do not divide (as
 *            "squelch_gate").  A ragged run in mode 2: -ENOTSUP from rtlfm_gpu_run_begin, nothing is taken.
 *   Setting the option: -EBUSY while a run is begun and not ended; -EINVAL for values other than 0, 1, 2.
 *
 * rtlfm_gpu_fetch_packed / _fetch_packed_prev wait exactly as rtlfm_gpu_fetch_all / _fetch_all_prev do (_prev for that
 * run only), copy the index (nstreams records) and then *total int16 in ONE transfer.  *total is the sum of the rows'
 * lengths each rounded up to 8.  -ENODATA when that run was not packed (the option was off when it ran); -ENOBUFS with
 * *total set when cap < *total (out is then untouched; rows has been written); -EAGAIN as their unpacked twins.
 *
 * rtlfm_gpu_pack_device: the mode-1 operator without a handle, as the other *_device entry points asynchronous on
 * hip_stream (NULL = the default stream).  Row s is d_lens[s] (negative: 0) int16 at d_rows + s * stride, any int16
 * alignment; d_packed is 16-byte aligned and holds cap int16; d_index [nstreams]; *d_total is always the full need, also
 * when it exceeds cap - nothing at or beyond cap is then written, and the caller sees the need from the total.
 */
typedef struct { uint64_t offset; int32_t len; int32_t held; } rtlfm_packed_row;   /* 16 bytes */
int rtlfm_gpu_fetch_packed(rtlfm_gpu *h, int16_t *out, size_t cap, rtlfm_packed_row *rows /* [nstreams] */, size_t *total);
int rtlfm_gpu_fetch_packed_prev(rtlfm_gpu *h, int16_t *out, size_t cap, rtlfm_packed_row *rows, size_t *total);
int rtlfm_gpu_pack_device(int device, const int16_t *d_rows, size_t stride, const int32_t *d_lens, int nstreams,
                          int16_t *d_packed, size_t cap, rtlfm_packed_row *d_index, uint64_t *d_total, void *hip_stream);

int rtlfm_gpu_state_get(rtlfm_gpu *h, int stream, rtlfm_stream_state *st);
int rtlfm_gpu_state_set(rtlfm_gpu *h, int stream, const rtlfm_stream_state *st);
/* demod_init() values for every stream. */
int rtlfm_gpu_reset(rtlfm_gpu *h);

/*
 * The stream lifecycle: the carried state of MANY streams in one operation ("Checkpoint /
 * resume": the persisting fields of struct demod_state, src/rtl_fm.c:172-208, are one explicit, copyable record per
 * stream).  rtlfm_gpu_state_get / _set wait for the handle and make one small blocking copy per call; a loop of them
 * over thousands of streams costs thousands of times a run (DESIGN.md sections 8.3, 8.4).
 *
 * rtlfm_gpu_state_get_all / _set_all: every stream's record in one wait and one copy, with the semantics of the
 * per-stream calls.  get_all: *n = the handle's stream count (written even where it does not fit), -ENOBUFS when
 * cap is smaller.  set_all: n must be the handle's stream count (-EINVAL).
 *
 * rtlfm_gpu_state_move: stream k of dst takes the carried state AND the hop mute still owed (rtlfm_gpu_mute) of
 * stream map[k] of src; map[k] == -1 gives it demod_init()'s state and no mute.  n must be dst's stream count and
 * every map[k] must lie in [-1, src's stream count); an entry may occur several times (one stream fans out to
 * several).  dst == src is allowed: a permutation, a fan-out or a reset of single streams in place.  The handles
 * share one configuration by the caller's word - a record means what its handle's configuration makes of it.
 * What a stream carries moves; what describes a run does not: the per-run records (levels, gate, input statistics
 * and health) and the results stay where they are, and buffers queued in src's ring stay with src, which is left
 * exactly as it was (when it is not dst).
 * Blocks like rtlfm_gpu_state_set: waits for everything both handles have queued, then ONE kernel launch
 * (k_state_move, csrc/state_kernel.h) whatever n is - the map travels to the device as one small array - and no
 * call into the HIP runtime per stream.
 *   -EBUSY   either handle has a run begun and not ended (rtlfm_gpu_run_begin) or a ring slot open (rtlfm_gpu_acquire)
 *   -EXDEV   the handles are on different devices: go through rtlfm_gpu_state_get_all / _set_all
 *   -EINVAL  anything out of range; both handles are left as they were (as after every failure)
 *
 * rtlfm_gpu_save / _load: every stream's record and owed mute to / from a file (include/rtlfm_snapshot.h, host-only
 * format: checksummed, written through a temporary file and rename).  save = get_all + the mutes +
 * rtlfm_snapshot_write; load = rtlfm_snapshot_read + set_all + rtlfm_gpu_mute.  load changes nothing and says
 *   -ERANGE       the file holds another number of streams than the handle
 *   -EMEDIUMTYPE  it was saved under another configuration: any rtlfm_cfg field but max_blocks and report_levels
 *                 differs (those two change how much a run takes and what it reports, not what a stream carries)
 *   -EILSEQ       it is damaged or no snapshot at all
 * A restarted service that loads what it saved goes on without a click: its first output sample is the one the
 * uninterrupted run would have produced.
 */
int rtlfm_gpu_state_get_all(rtlfm_gpu *h, rtlfm_stream_state *out, int cap, int *n);
int rtlfm_gpu_state_set_all(rtlfm_gpu *h, const rtlfm_stream_state *in, int n);
int rtlfm_gpu_state_move(rtlfm_gpu *dst, rtlfm_gpu *src, const int32_t *map, int n);
int rtlfm_gpu_save(rtlfm_gpu *h, const char *path);
int rtlfm_gpu_load(rtlfm_gpu *h, const char *path);

/*
 * Channels: K demodulated channels per wideband source through one NCO front end.
 *
 * The reference tunes one dongle to one channel; its only frequency translation is rotate16_neg90 (src/rtl_fm.c:424-434),
 * fs/4 and fixed.  With channels on, stream s of the handle is channel s % per_source of SOURCE s / per_source, and the
 * rotation's place is taken by a mixer with a per-stream step.  Integer and bit-exact everywhere:
 *   table    1024 entries, Q14: c[i] = lround(16384 cos(2 pi i / 1024)), s[i] the same of sin, in double (rtlfm_channel_table)
 *   phase    sample n of a run: (uint32)((pos + n) * step), table index = phase >> 22; pos = complex samples the handle
 *            has consumed since rtlfm_gpu_set_channels / rtlfm_gpu_reset / rtlfm_gpu_channels_seek - one counter per
 *            handle, the streams run in lockstep; all of it modulo 2^32
 *   mixer    x = I - 127, y = Q - 127 (rtlsdr_callback, src/rtl_fm.c:1326-1328):
 *            I' = (x c + y s + 8192) >> 14,  Q' = (y c - x s + 8192) >> 14: multiplication by e^(-j theta).
 *            step = 2^30 is rotate16_neg90's 1, -j, -1, +j to the bit, step = 0 the identity (offset_tuning = 1)
 *   step     rtlfm_channel_step(shift_hz, capture_rate) = (uint32) round_half_up(shift_hz 2^32 / capture_rate), in
 *            integers; 0 for capture_rate == 0.  shift_hz = channel_freq - capture_freq: how far ABOVE the frequency the
 *            source is tuned to the channel lies (a carrier at +shift_hz in the capture comes to rest at 0).  rtl_fm's
 *            own tuning (capture_freq = freq - capture_rate / 4, src/rtl_fm.c:1423-1428, rtlfm_optimal_settings) puts its
 *            one channel at +capture_rate / 4 -> 2^30: the reference's own chain, its sign convention
 * Behind the mixer the chain is the stream's own, unchanged: low_pass or fifth_order (+ generic_fir) on I', Q' with the
 * stream's carried state, then the squelch, -L levels (rtlfm_gpu_levels*), every -M mode and every audio tail;
 * rtlfm_gpu_state_get / _set(_all) and rtlfm_gpu_set_path work per channel as they do per stream.
 *
 * rtlfm_gpu_set_channels: per_source >= 1 must divide the handle's stream count (-EINVAL), steps[nstreams] is copied;
 * per_source == 0 switches channels off (steps may be NULL).  Sets pos = 0.  Waits for what the handle has queued.
 * While channels are on, rtlfm_gpu_run_device
 *   - reads d_iq as nstreams / per_source rows, stream_stride apart: one per source;
 *   - ignores cfg.offset_tuning;
 *   - adds nblocks * block_len / 2 to pos once per successful run (also under verify_twice, whose two executions use
 *     the same pos);
 *   - takes the boxcar (downsample_passes == 0, rtl_fm's default decimator) through ONE launch from source bytes to
 *     every channel's decimated IQ (k_channel_boxcar; rtlfm_gpu_last_path says 2), everything else through the staged
 *     kernels behind k_channel_mix (1); rtlfm_gpu_set_path(1) forces the latter, 2 with fifth_order passes is -ENOTSUP.
 * What reads or owns per-STREAM input rows, or would lose pos, is refused with -ENOTSUP and changes nothing while
 * channels are on: rtlfm_gpu_push / _acquire / _commit / _run / _run_begin (the ring) unless the option source_ring
 * gives the ring a row per source ("The ring and channels" at rtlfm_gpu_push), the options input_stats,
 * input_health and squelch_gate, rtlfm_gpu_mute, rtlfm_gpu_save / _load / _state_move; and rtlfm_gpu_set_channels itself
 * on a handle with cfg.dc_block_raw or one of those options on (-EBUSY with a run begun, a ring slot open or a mute owed,
 * and - option source_ring on - with buffers queued in the ring, whose rows it would change).
 * rtlfm_gpu_channels_seek / _tell: set / read pos (a caller that resumes a recording sets where it is).
 */
uint32_t rtlfm_channel_step(int32_t shift_hz, uint32_t capture_rate);
int rtlfm_channel_table(int16_t *cos_sin /* [1024][2] */);
int rtlfm_gpu_set_channels(rtlfm_gpu *h, int per_source, const uint32_t *steps /* [nstreams] */);
int rtlfm_gpu_channels_seek(rtlfm_gpu *h, uint64_t pos);
int rtlfm_gpu_channels_tell(rtlfm_gpu *h, uint64_t *pos);

/*
 * The channel filter: a caller-supplied FIR in the boxcar's place (csrc/channel_fir_kernel.h).
 *
 * A boxcar /D is a sinc whose first sidelobe lies 13 dB down, and a channel cut out of a wideband capture has no tuner
 * filter in front of it: a neighbour 1.5 channel spacings away folds onto the output at that level.  With a filter set
 * and channels on, low_pass()'s sum (src/rtl_fm.c:461-481) is replaced; everything behind it stays the stream's chain.
 * Integers only, one definition for every path:
 *   m[n]     a channel's mixed I' (or Q') as above, |m| <= 182; n counts the complex samples since the history was last
 *            cleared, m[n] = 0 for n < 0
 *   outputs  are due at exactly the samples e at which low_pass() emits one: where the stream's prev_index reaches D =
 *            cfg.downsample.  prev_index and the count of outputs are kept as the boxcar keeps them; now_r / now_j are
 *            carried along unchanged and not used
 *   value    sat16((sum_{j < ntaps} taps[j] m[e - j] + r) >> shift), r = shift ? 1 << (shift - 1) : 0, the shift
 *            arithmetic, sat16 a clamp to [-32768, 32767].  The sum is an int32 that cannot overflow (the check below),
 *            so every order of summation gives the same bits.  Taps of D ones with shift 0 are the boxcar.
 * rtlfm_channel_filter_check (host only, no GPU): -EINVAL unless 1 <= ntaps <= RTLFM_CHANNEL_MAX_TAPS, 0 <= shift <= 30
 * and taps != NULL; -ERANGE unless 182 sum|taps[j]| + r <= 2^31 - 1.
 * rtlfm_channel_lowpass (host only, no GPU): a Hamming-windowed sinc in double, cutoff in cycles per capture sample
 * (0 < cutoff < 0.5, else -EINVAL; D >= 1), normalised to a sum of 1, taps[j] = floor(h[j] D 2^14 + 0.5), *shift = 14: the
 * boxcar's DC gain D, so squelch levels and every -M mode see the amplitudes they see today.  -ERANGE if a tap does not
 * fit an int16 or the check fails.
 * rtlfm_gpu_set_channel_filter: runs the check first; ntaps == 0 removes the filter (the boxcar is back, bit for bit).
 * -ENOTSUP, changing nothing, on a handle with cfg.downsample_passes > 0 (the filter takes the boxcar's place, not
 * fifth_order's); -EBUSY while a run is begun and not ended.  May be called with channels off: the taps are kept and act
 * only while channels are on.  Waits for what the handle has queued.  One filter and one D for all channels.
 * rtlfm_gpu_get_channel_filter: *ntaps and *shift are always written; the taps are copied if ntaps <= cap, else -ENOBUFS.
 *
 * History, the filter's and the channel bank's (below) alike - there is one: what is carried from run to run is every
 * SOURCE's last 4096 complex samples as raw bytes (the filter reads ntaps - 1 of them, the bank up to ntaps + K), in two
 * device buffers of the handle: a run reads one and writes the other, changed over where pos advances.  Not in
 * rtlfm_stream_state, whose size and snapshot format stay.  The mixer is a pure function of pos and the bytes: a run
 * mixes what it needs of them again.  A run shorter than the history shifts it.  The buffers hold 16 KiB per source - not
 * per stream - and are allocated once channels are on and a filter or a bank is set (grown when rtlfm_gpu_set_channels
 * brings more sources, never shrunk): 2 x 16 KiB x sources, which with a filter alone and fewer than 4 channels per source
 * is more than the 4 KiB per stream the filter would need by itself.  The history is cleared to bytes 127 (mixed zeros,
 * m[n < 0] = 0; x[n < 0] = 0) by
 *   rtlfm_gpu_set_channel_filter   (new taps start from silence; also while the bank is on and the filter rests, and
 *                                   also with ntaps == 0),
 *   rtlfm_gpu_set_channel_bank     (the same; also with K == 0, so the filter that acts again starts from silence),
 *   rtlfm_gpu_set_channels         (other sources, pos = 0),
 *   rtlfm_gpu_reset                (with the state records and pos),
 *   rtlfm_gpu_channels_seek        (the bytes belong to the old position).
 * A call that is refused clears nothing.  Under verify_twice both executions of a run see one pos and one history.
 * Paths: rtlfm_gpu_set_path(0 / 2) - one launch from source bytes to every channel's decimated IQ (k_channel_fir;
 * rtlfm_gpu_last_path says 2), the default; (1) - k_channel_mix over the history and the run, then a plain kernel with
 * one lane per output, and a history kernel (the cross-check).  Both read and write the same history: changing the path
 * between two runs changes no output bit.
 */
#define RTLFM_CHANNEL_MAX_TAPS 1024
int rtlfm_channel_filter_check(const int16_t *taps, int ntaps, int shift);
int rtlfm_channel_lowpass(int ntaps, double cutoff, int D, int16_t *taps, int *shift);
int rtlfm_gpu_set_channel_filter(rtlfm_gpu *h, const int16_t *taps, int ntaps, int shift);
int rtlfm_gpu_get_channel_filter(rtlfm_gpu *h, int16_t *taps, int cap, int *ntaps, int *shift);

/*
 * The channel bank: uniformly spaced channels by polyphase sums and one fix_fft (DESIGN.md section 8.5,
 * csrc/channel_bank_kernel.h).
 *
 * The mixer paths pay for every source sample once per channel.  Where the channels are spaced fs / K apart the mixer
 * bank collapses: group the filter's taps by n mod K - K polyphase sums per output instant - and apply one K-point
 * transform; bin k is the channel at +k fs / K.  The work per source sample no longer grows with K.  The transform is
 * rtl_power's fix_fft (src/rtl_power.c:271-327), which the project already runs bit for bit on the device.  Integers
 * only, one definition for every path:
 *   K, taps  K = 2^m, 2 <= m <= 8; taps[ntaps] int16, 1 <= ntaps <= RTLFM_BANK_MAX_TAPS; 0 <= shift <= 30; D =
 *            cfg.downsample, any D (it need not relate to K)
 *   bins     bins[per_source], each in [0, K), duplicates allowed: channel c of every source is bin bins[c].  NULL is
 *            the identity and needs per_source == K
 *   x[n]     (I - 127, Q - 127) of the source; n is absolute, pos (rtlfm_gpu_channels_tell) + the index within the run;
 *            x = 0 before the point where the history was last cleared
 *   outputs  are due at the samples e at which low_pass() emits one, as for the channel filter - here with ONE schedule per
 *            source, taken from the prev_index of the source's channel 0; a run writes the new prev_index and the count
 *            to every channel of the source.  now_r / now_j are copied, not used
 *   sums     per component, r = 0 .. K - 1: u_r = sum over j < ntaps with (e - j) mod K == r of taps[j] x[e - j]  (K is a
 *            power of two: (pos + i) & (K - 1) is exact across pos wrapping 2^32);
 *            v_r = sat16((u_r + rnd) >> shift), rnd = shift ? 1 << (shift - 1) : 0
 *   Y        = fix_fft(v) exactly as rtl_power defines it with N_WAVE = K: bit reversal, one halving per stage, FIX_MPY
 *            rounding, int16 wrap on every store, sine_table(m).  Channel c's decimated IQ sample is Y[bins[c]].  A
 *            carrier k fs / K ABOVE the tuned frequency comes to rest at 0 in bin k (the sign convention of
 *            rtlfm_channel_step); bins >= K / 2 are the negative shifts
 * Behind it the stream's chain is unchanged: squelch, -L levels, every -M mode, every audio tail.  The steps given to
 * rtlfm_gpu_set_channels are kept and not used while the bank is on.
 * rtlfm_channel_bank_check (host only, no GPU): -EINVAL for a bad K, ntaps or shift or NULL taps; -ERANGE unless
 * 128 max over branches b of sum_q |taps[b + q K]| + rnd <= 2^31 - 1: u_r is an int32 that cannot overflow, so every order
 * of summation gives the same bits.  rtlfm_channel_lowpass(ntaps, cutoff, D) with shift = 14 - m gives the boxcar's DC
 * gain D (the transform halves once per stage: 2^-m).
 * rtlfm_gpu_set_channel_bank: runs the check first; K == 0 removes the bank (the mixer paths are back, bit for bit).
 * -EINVAL with channels off or a bin outside [0, K) (or bins == NULL with per_source != K); -ENOTSUP, changing nothing,
 * with cfg.downsample_passes > 0; -EBUSY while a run is begun and not ended.  Waits for what the handle has queued and
 * clears the history.  While on, the bank takes precedence over a set channel filter: the filter's taps are kept
 * and act again once the bank is removed.  rtlfm_gpu_set_channels removes the bank (bins belongs to the old per_source).
 * rtlfm_gpu_get_channel_bank: *K, *ntaps and *shift are always written (0 without a bank); bins (per_source of them) and
 * taps are copied if both caps suffice, else -ENOBUFS.
 *
 * History: the one described with the channel filter above - its size, its five clearing calls, verify_twice.
 * Paths: rtlfm_gpu_set_path(0 / 2) - k_channel_bank, one launch from source bytes to every selected channel's decimated
 * IQ (rtlfm_gpu_last_path says 2), the default; (1) - the plain cross-check: one lane per (frame, residue) forms v in
 * memory, one lane per frame runs fix_fft in the reference's loop order, a scatter and a history kernel follow.  Both
 * read and write the same history: changing the path between two runs changes no output bit.
 * Everything refused while channels are on stays refused; with the bank off no kernel, path or result changes.
 */
#define RTLFM_BANK_MAX_TAPS 4096
int rtlfm_channel_bank_check(int K, const int16_t *taps, int ntaps, int shift);
int rtlfm_gpu_set_channel_bank(rtlfm_gpu *h, int K, const int32_t *bins /* [per_source] or NULL */, const int16_t *taps, int ntaps,
                               int shift);
int rtlfm_gpu_get_channel_bank(rtlfm_gpu *h, int *K, int32_t *bins, int bins_cap, int16_t *taps, int taps_cap, int *ntaps, int *shift);

/*
 * The bank's survey and per-source bins: a few demodulator SLOTS per source that follow the activity (DESIGN.md section
 * 8.5, "Survey and slots"; include/rtlfm_slots.h has the allocator that turns one into the other).
 *
 * Per output instant the bank computes all K bins of a source and keeps the per_source the caller selected.  With the
 * option "bank_survey" at 1 a run the bank takes also leaves, for source a with E_a the frames the run emitted (the count
 * written to the source's channels),
 *   frames[a]   = E_a
 *   power[a][k] = sum over f < E_a of Yi[f][k]^2 + Yq[f][k]^2        (uint64; one term reaches 2^31)
 * Y being the int16 pair fix_fft leaves for bin k at frame f: all K bins, selected or not, whatever bins says.  Integers,
 * the same on both paths.  Path 2: k_channel_bank_survey - k_channel_bank's body with, per tile, the 256 lanes over (bin,
 * group of frames) adding the results up out of LDS in 64-bit registers, and per segment one [K] partial stored - and
 * k_bank_survey_reduce, which adds the segments and writes frames; both inside the front end's timed pair.  Path 1:
 * k_bank_power_plain, one lane per (source, bin), behind the cross-check's kernels.  No atomics; a run without frames
 * leaves zeros.  Two sets of buffers rotate as the ring's halves do, allocated by the first surveyed run and freed when
 * the option returns to 0 (which waits for the handle) or with the handle.  Under verify_twice a survey is one
 * execution's.  A ring run that holds short buffers is not surveyed.  With the option at 0 (default) no kernel, path,
 * result or allocation differs.  Anything but 0 / 1 -EINVAL; -EBUSY while a run is begun and not ended; it may be set with
 * the bank or channels off and acts only on runs the bank takes.
 * rtlfm_gpu_bank_survey (_prev): power [sources][K] (cap: elements), frames [sources] and *K of the last run (of the run
 * before it), waited for as rtlfm_gpu_fetch_all (_prev) wait - _prev for that run only, not the one started since; for
 * runs through rtlfm_gpu_run_device just the same.  -ENODATA when that run carried no survey (option off, bank off, no
 * run yet); -ENOBUFS when cap is too small, *K written all the same.
 *
 * rtlfm_gpu_set_channel_bins: bins [sources][per_source], each in [0, K) - channel c of source a becomes bin
 * bins[a][c] of the bank that is set.  Nothing else changes: pos, the history, the taps and every stream's carried record
 * stay (as retuning a dongle keeps demod_state).  The call does not wait for the device: the new bins travel through a
 * rotation of pinned buffers on the handle's stream, so runs already queued use the old bins and later runs the new.
 * -EINVAL without a bank, for NULL, or for a bin outside [0, K); -EBUSY while a run is begun and not ended; a refused call
 * changes nothing.  rtlfm_gpu_set_channel_bank afterwards is its shared list again; it and rtlfm_gpu_set_channels drop the
 * per-source bins.  rtlfm_gpu_get_channel_bins: [sources][per_source] as they rule now (the shared list repeated where no
 * per-source bins are set); -ENOBUFS where cap < sources * per_source.  rtlfm_gpu_get_channel_bank keeps returning
 * per_source bins: source 0's.
 *
 * The loop: run r -> rtlfm_gpu_bank_survey -> rtlfm_slots_step -> rtlfm_gpu_set_channel_bins -> run
 * r + 1.  A decision made from run r's survey acts on run r + 1 (r + 2 through _prev): a transmission's first buffer is
 * lost.
 */
int rtlfm_gpu_bank_survey(rtlfm_gpu *h, uint64_t *power, size_t cap, int32_t *frames, int *K);
int rtlfm_gpu_bank_survey_prev(rtlfm_gpu *h, uint64_t *power, size_t cap, int32_t *frames, int *K);
int rtlfm_gpu_set_channel_bins(rtlfm_gpu *h, const int32_t *bins /* [sources][per_source] */);
int rtlfm_gpu_get_channel_bins(rtlfm_gpu *h, int32_t *bins, int cap);

/*
 * Option "source_dc": the raw DC block per SOURCE in front of the mixers and the bank ("Source DC").
 *
 * A capture has a DC spike at the frequency the dongle is tuned to; the reference takes it off with dc_block_raw_filter
 * "BEFORE up-mixing" (src/rtl_fm.c:1043-1065, :1329-1332).  cfg.dc_block_raw stays refused while channels are on (it is a
 * stream's filter); this option is the same recurrence for the source rows.  0 (default) / 1; it acts only on runs that
 * channels take and may be set with channels off.  All of it is integers, one definition for every path:
 *
 * averages     a run has nblocks buffers of L bytes (cfg.block_len, or a ring view's own length: whole 512-byte packets, so
 *              a buffer is a multiple of 256 complex samples).  For source a and buffer b, k = cfg.rdc_block_const:
 *                  mI    = trunc(sum(I - 127) / (L / 2))                     (C division; likewise mQ)
 *                  aI[b] = trunc((mI + aI[b-1] k) / (k + 1))                 (likewise aQ)
 *                  aI[-1] = clamp(dc_avgI, -128, 128) of the record of the source's CHANNEL 0 (stream a * per_source)
 *              - the recurrence of :1055-1058 with the carried value clamped on the way in, so that a broken record moves
 *              values and never breaks a bound (as p0c does for prev_index): |a| <= 128 by induction.
 * subtraction  every sample of buffer b enters every front end as x = I - 127 - aI[b], y = Q - 127 - aQ[b]: |x|, |y| <= 256.
 *              The mixer, the boxcar, the filter and the bank are the existing definitions with this x, y; everything behind
 *              the front end is the stream's chain unchanged (rms() keeps its DC fix: omitDCfix follows cfg.dc_block_raw = 0).
 * record       after a run dc_avgI / dc_avgQ of EVERY channel's record of the source are a[nblocks - 1] (as the bank writes
 *              prev_index); rtlfm_gpu_state_get / _set (_all) see them per channel.  verify_twice: both executions use
 *              one set of averages and one history.
 * history      the filter and the bank re-read up to 4096 samples in front of a run as raw bytes; those keep the x, y they
 *              were consumed with: beside the byte history the handle carries, per source, what was subtracted from each
 *              of its sixteen 256-sample pieces, in two copies that change over with the bytes.  Wherever the history is
 *              cleared these are too (bytes 127 with a = 0: x = 0).  A run shorter than the history shifts whole pieces.
 * switching    in either direction waits for the handle, clears the history (a sixth clearing call) and leaves every
 *              record alone.
 * refusals     each changes nothing.  -EINVAL: a value other than 0 / 1, or - setting 1 - cfg.rdc_block_const outside
 *              0 ... 65535; -ENOTSUP on a handle with cfg.dc_block_raw; -EBUSY while a run is begun, a ring slot is open
 *              or, with source_ring, buffers are queued; -ERANGE: setting 1 while a filter or bank is set that fails the
 *              wider check below.
 * bounds       with the option on |m| <= 362 instead of 182 ((256 (|c| + |s|) + 8192) >> 14 over the table) and the bank
 *              sees |x| <= 256 instead of 128.  rtlfm_channel_filter_check_dc / rtlfm_channel_bank_check_dc (host only) are
 *              the two checks with those factors; rtlfm_gpu_set_channel_filter / _bank apply them while the option is 1
 *              (-ERANGE, nothing changed).  Mixed samples still fit the packed int16 the kernels keep in LDS.
 * kernels      k_rdc_sums_wide / _small on the source rows (one more read of the source bytes) and k_source_dc_smooth,
 *              inside the front end's timed pair, leave one list per source: what comes off the bytes of every 256-sample
 *              piece of the history and of the run.  k_channel_boxcar<STAGE, true>, k_channel_fir<true>, k_channel_bank_dc (_survey_dc)
 *              and, on path 1, k_channel_mix<true> and k_bank_sums<true> are the existing bodies reading it.  With the option at
 *              0 no kernel, path, launch count, result or allocation differs.
 */
int rtlfm_channel_filter_check_dc(const int16_t *taps, int ntaps, int shift);
/* Measurement only (tools/source_dc_bench.py): source_dc's pre-pass alone over d_iq's source rows, as one timed pair of
 * rtlfm_gpu_timing_read.  Waits for the handle first; moves nothing a run carries.  -ENOTSUP with the option or channels
 * off, -EBUSY while a run is begun, -EINVAL / -E2BIG as rtlfm_gpu_run_device. */
int rtlfm_gpu_source_dc_prepass(rtlfm_gpu *h, const uint8_t *d_iq, size_t stream_stride, int nblocks);
int rtlfm_channel_bank_check_dc(int K, const int16_t *taps, int ntaps, int shift);

/*
 * Options "source_stats" and "source_health": the ADC statistics and the input health per SOURCE (DESIGN.md section 8.5,
 * "Source statistics and health").
 *
 * One wideband source feeds K channels, so its gain decides all K at once: an overloaded ADC spoils every channel, too
 * little gain raises every channel's noise.  "input_stats" / "input_health" read per-STREAM input rows and stay refused
 * while channels are on (-ENOTSUP, both ways round); these two are the same records for the source rows.  Each 0 (default)
 * / 1; they act only on runs that channels take and may be set with channels off (as "source_dc").
 *
 * records      one rtlfm_input_stat and / or one rtlfm_input_health per (source, buffer) of the run, with exactly the
 *              definitions at rtlfm_gpu_input_stats / rtlfm_gpu_input_health above (no new type), taken over the source's raw
 *              bytes before anything else touches them: in front of source_dc's subtraction, the mixers, the filter and the
 *              bank.  Integer and order-independent: bit-identical to the reference's loops.  They change no result: PCM,
 *              lengths, state records and rtlfm_gpu_channels_tell are those of the run without them.
 * which runs   rtlfm_gpu_run_device reads the caller's source rows; ring runs over "source_ring" read the handle's device
 *              copy.  A ring run that holds short buffers files each buffer's record over its own length, [source][nb], as
 *              the stream readers do per stream.  Under verify_twice the records are one execution's (both see the same bytes).
 * fetch        rtlfm_gpu_source_stats / _health: the last run's records of `source`; _all: every source in one copy, source
 *              a at out + a * cap.  The contract of rtlfm_gpu_levels / _all with sources for streams: -EINVAL for bad
 *              arguments or a source outside [0, sources); -ENODATA while the option is off, before the first run, after
 *              rtlfm_gpu_set_channels and while the last run was not one that channels took; -ENOBUFS, with *n written, when
 *              cap is too small; *n = buffers of the last run.
 * setting      -EINVAL for any value but 0 / 1, -EBUSY while a run is begun and not ended or a ring slot is open; a refused
 *              call changes nothing.  Setting 0 frees nothing.  The records, [sources][max_blocks], are allocated by the first
 *              run that needs them and regrown when rtlfm_gpu_set_channels makes the sources more.
 * kernels      inside the front end's timed pair (rtlfm_gpu_timing_read shows what they cost).  With "source_dc" on the
 *              source rows are read ONCE for all of it: k_source_prepass (csrc/source_prepass_kernel.h) leaves the sums
 *              k_rdc_sums_wide / _small would and the records, built from the readers' own per-word functions.  With
 *              "source_dc" off k_input_health (which takes the statistics along) or k_input_stats run over the source rows.
 *              Loads as input_stats_nt.  With both options at 0 no kernel, path, launch count, result or allocation differs.
 */
int rtlfm_gpu_source_stats(rtlfm_gpu *h, int source, rtlfm_input_stat *out, int cap, int *n);
int rtlfm_gpu_source_stats_all(rtlfm_gpu *h, rtlfm_input_stat *out, int cap, int *n);
int rtlfm_gpu_source_health(rtlfm_gpu *h, int source, rtlfm_input_health *out, int cap, int *n);
int rtlfm_gpu_source_health_all(rtlfm_gpu *h, rtlfm_input_health *out, int cap, int *n);

/*
 * Option "source_iq": IQ balance per SOURCE, measured and applied on the device ("Source IQ").
 *
 * A wideband source whose I and Q differ in gain or are not in quadrature folds the channel at +f onto the channel at -f:
 * every one of its K demodulators hears its mirror channel.  rtl_tcp -c (iqBalance, src/rtl_tcp.c:211-233) rewrites its
 * uint8 buffer; so does this option (0 default / 1), for runs that channels take.  It may be set with channels off.
 *
 * records      one rtlfm_iq_sums per (source, buffer) of the run over the RAW bytes I, Q in [0, 255]: n = len / 2, si = sum I,
 *              sq = sum Q, sii = sum I^2, sqq = sum Q^2, siq = sum I Q; clipped = output BYTES the clamp below changed.
 *              Integers: any order of summation gives the same bits.
 * rows         with x = I - 127, y = Q - 127 and the source's four int16 Q14 coefficients (a, b, p, q):
 *                I' = (a x + b y + 8192) >> 14,  Q' = (p x + q y + 8192) >> 14    (arithmetic shift, int32)
 *              and each output byte is clamp(v + 127, 0, 255).  The identity (16384, 0, 0, 16384) reproduces every byte.
 *              The rows go into a buffer of the handle's, [sources][max_blocks * block_len], allocated by the first run that
 *              needs it, regrown when rtlfm_gpu_set_channels makes the sources more, freed when the option returns to 0.
 * who reads    everything behind it reads the corrected rows in the caller's place: source_dc's sums, every channel front
 *              end and cross-check, k_channel_mix, and k_source_history - the history keeps the bytes as they were
 *              consumed, so a change of coefficients between runs needs no list per piece.  "source_stats" / "source_health"
 *              describe the ADC and keep reading the RAW rows (k_input_health / k_input_stats as with source_dc off; with
 *              source_dc on its sums come from k_rdc_sums_* on the corrected rows, and k_source_prepass is not used: one
 *              more read).  verify_twice: both executions read the same coefficients and leave the same rows and records.
 * setting      -EINVAL for any value but 0 / 1; -EBUSY while a run is begun, a ring slot is open or, with source_ring,
 *              buffers are queued; a refused call changes nothing.  Either direction waits for the handle and does NOT
 *              clear the history.  With the option at 0 no kernel, launch count, allocation or result differs.
 *
 * rtlfm_gpu_set_source_iq: coef [sources][4] = (a, b, p, q) per source.  No wait: the copy goes through a rotation of pinned
 * buffers on the handle's stream (as rtlfm_gpu_set_channel_bins) - runs already queued use the old coefficients, later
 * runs the new.  -ENOTSUP with channels off, -EINVAL for NULL, -EBUSY in a begun run.  A fresh handle has the identity and
 * rtlfm_gpu_set_channels resets every source to it.  May be called with the option off; the values rule once it is on.
 * rtlfm_gpu_get_source_iq: the coefficients as they rule now, [sources][4]; -ENOBUFS when cap (in int16) is too small,
 * -ENOTSUP with channels off.
 * rtlfm_gpu_source_iq_sums / _all: the contract of rtlfm_gpu_source_stats / _all: -EINVAL for bad arguments or a source
 * outside [0, sources); -ENODATA while the option is off, before the first run, after rtlfm_gpu_set_channels and while the
 * last run was not one that channels took; -ENOBUFS, with *n written, when cap is too small; a ring run that holds short
 * buffers files each buffer's record over its own length, [source][nb].
 *
 * The coefficients belong to the caller: rtlfm_gpu_channels_save / _load / _move and the RTLFMCHN file do not carry them.
 * Whoever resumes or regroups reads them with rtlfm_gpu_get_source_iq and sets them again, as with the soft AGC's indices.
 * The policy that turns records into coefficients is host code: include/rtlfm_iq.h.
 */
typedef struct rtlfm_iq_sums {
	uint32_t n, clipped;
	uint64_t si, sq, sii, sqq, siq;
} rtlfm_iq_sums;  /* 48 bytes */
int rtlfm_gpu_set_source_iq(rtlfm_gpu *h, const int16_t *coef /* [sources][4] */);
int rtlfm_gpu_get_source_iq(rtlfm_gpu *h, int16_t *coef, int cap);
int rtlfm_gpu_source_iq_sums(rtlfm_gpu *h, int source, rtlfm_iq_sums *out, int cap, int *n);
int rtlfm_gpu_source_iq_sums_all(rtlfm_gpu *h, rtlfm_iq_sums *out, int cap, int *n);

/*
 * The channel lifecycle: snapshot, resume and regroup by SOURCE ("Lifecycle").
 *
 * rtlfm_gpu_save / _load / _state_move stay refused while channels are on (-ENOTSUP): a handle with channels on carries
 * three things no rtlfm_stream_state record holds -
 *   pos        the handle's one sample counter (rtlfm_gpu_channels_tell);
 *   history    with a channel filter or a bank set, every source's last 4096 complex samples as raw bytes, which both re-read
 *              in front of every run: 8192 bytes per source, oldest sample first, bytes 127 where it was cleared or where a
 *              run shorter than the history shifted silence in;
 *   biases     with option "source_dc" as well, what was subtracted from each of the history's sixteen 256-sample pieces:
 *              16 words per source as the kernels keep them (0x007f007f where nothing was) -
 * and these calls, beside the old ones, move all of it.  With channels off every one of them is -ENOTSUP and nothing differs.
 *
 * rtlfm_gpu_channels_history_get: waits for the handle; *sources is written always; [sources][8192] bytes of the history
 * and, with "source_dc" on, [sources][16] bias words (dc may be NULL while the option is off).  -ENOTSUP with channels off,
 * -ENODATA when neither a filter nor a bank is set (nothing is carried then), -ENOBUFS when a cap is too small.
 * rtlfm_gpu_channels_history_set: the inverse, in the role rtlfm_gpu_state_set_all plays for the records.  sources must be
 * the handle's (-EINVAL); dc == NULL with "source_dc" on means "none subtracted"; -EBUSY while a run is begun, a ring slot
 * is open or (option source_ring) buffers are queued.  With rtlfm_gpu_state_get_all / _set_all and rtlfm_gpu_channels_tell /
 * _seek these two are the route between devices.  rtlfm_gpu_channels_seek clears the history: to resume, seek FIRST, then
 * history_set.
 *
 * rtlfm_gpu_channels_move: the regroup, by source and on the device.  For a < nsources (= dst's sources), m = source_map[a]:
 * source a of dst receives the per_source records of source m of src (channel c from channel c), its history and its biases;
 * m == -1 gives demod_init()'s records, a history of bytes 127 and no biases - a source that joins from silence.  An entry
 * may occur several times (a fan-out); dst == src is a permutation in place.  dst takes src's pos: one counter per handle.
 * Steps, shared or per-source bins, taps and options do not move - the caller sets them on dst, as it must anyway to switch
 * channels on there, and every call that clears comes before the move:
 *   rtlfm_gpu_set_channels, rtlfm_gpu_set_channel_filter / _set_channel_bank, option "source_dc", rtlfm_gpu_channels_move,
 *   rtlfm_gpu_set_channel_bins.
 * Waits for both handles, then ONE launch (k_source_move, csrc/state_kernel.h) for records, history and biases.
 *   -EINVAL       NULL, nsources not dst's sources, or an entry outside [-1, src's sources)
 *   -ENOTSUP      channels off on either handle
 *   -EXDEV        different devices: go through the accessors above
 *   -EMEDIUMTYPE  the handles do not carry the same things: a rtlfm_cfg field other than max_blocks / report_levels,
 *                 per_source, option "source_dc", the filter (ntaps, shift, taps) or the bank (K, ntaps, shift, taps) differs
 *   -EBUSY        as rtlfm_gpu_channels_history_set, on either handle
 * Every refusal leaves both handles as they were.
 *
 * rtlfm_gpu_channels_save / _load: all of it to / from a file (include/rtlfm_chansnap.h: magic "RTLFMCHN", checksummed,
 * written through a temporary file and rename).  save = state_get_all + channels_history_get + channels_tell, with the
 * steps, the taps and the bins as they rule, + rtlfm_chansnap_write (-EBUSY as rtlfm_gpu_channels_history_set: buffers queued in the ring would be missing from the file).  load
 * checks the whole file first, changes nothing on any failure and says
 *   -ERANGE       the file holds another number of streams than the handle
 *   -EMEDIUMTYPE  the comparison of the move, between the file and the handle
 *   -ENOTSUP      channels are off (RTLFMSNP files and such handles belong to rtlfm_gpu_load)
 *   -EBUSY        as above
 *   -EILSEQ       the file is damaged, or an RTLFMSNP file
 * The file's steps and bins are for the caller: load neither compares nor applies them (a different step after a resume is
 * a retune, which keeps a stream's state in the reference too).  Set the handle up as for a move, then load.
 */
int rtlfm_gpu_channels_history_get(rtlfm_gpu *h, uint8_t *bytes, size_t cap_bytes, uint32_t *dc, size_t cap_dc, int *sources);
int rtlfm_gpu_channels_history_set(rtlfm_gpu *h, const uint8_t *bytes, const uint32_t *dc, int sources);
int rtlfm_gpu_channels_move(rtlfm_gpu *dst, rtlfm_gpu *src, const int32_t *source_map, int nsources);
int rtlfm_gpu_channels_save(rtlfm_gpu *h, const char *path);
int rtlfm_gpu_channels_load(rtlfm_gpu *h, const char *path);

int rtlfm_gpu_sync(rtlfm_gpu *h);
/* Launch on a caller-owned hipStream_t (NULL = the handle's own stream).  On a caller-owned stream
 * EVERYTHING the handle launches is ordered on that stream, the audio tail (deemph, DC block,
 * resamplers) included: work the caller enqueues on it behind rtlfm_gpu_run_device() sees the
 * finished d_out / d_out_len.  (On its own stream the handle runs the audio tail of a step on a
 * second internal stream, overlapped with the next step's front end; rtlfm_gpu_sync /
 * _release_to / _state_get / _fetch* wait for both.) */
int rtlfm_gpu_set_stream(rtlfm_gpu *h, void *hip_stream);
/*
 * Ordering against another HIP stream without a host synchronisation.  The library launches on
 * its own non-blocking stream, which is NOT ordered with the caller's streams by itself:
 *   rtlfm_gpu_wait_for(h, p)    work launched on the handle from now on starts after everything
 *                               already enqueued on p (the producer of d_iq, the allocator of d_out);
 *   rtlfm_gpu_release_to(h, c)  work enqueued on c from now on starts after everything the handle
 *                               has launched so far (the consumer of d_out / d_out_len).
 * NULL names the legacy default stream.  A caller that uses neither must rtlfm_gpu_sync().
 * (The handle's own streams come from a process-wide pool and go back to it when the handle is destroyed; the library
 * never calls hipStreamDestroy.  Not an economy: on the runtime this was written against, a stream that had been ordered
 * against another stream this way and was then destroyed had a freed object of its own released once more, later, in
 * whoever's heap block it had become - csrc/stream_pool.h, LAB.md I.21.  A caller that creates and destroys streams of
 * its own around these calls at a high rate may want to pool them too.)
 */
int rtlfm_gpu_wait_for(rtlfm_gpu *h, void *producer_stream);
int rtlfm_gpu_release_to(rtlfm_gpu *h, void *consumer_stream);

/*
 * Tunables and A/B switches of one handle, by name (none of them changes a result; the parity
 * suite runs under several).  The library reads no environment variable while samples flow:
 * RTLFM_OPTIONS="name=value,name=value" is applied once, inside rtlfm_gpu_create().
 *   fused_waves          waves a front-end launch aims for (default 8192 = twice the GPU's wave slots);
 *                        a stream's run is cut into that many segments / nstreams.  Sets fused_waves_tail too.
 *   fused_waves_tail     the same for configurations with an audio tail behind the front end (deemph, DC block,
 *                        resamplers; default 20480 behind the boxcar, 12288 behind fifth_order passes: shorter
 *                        segments let the tail's waves in sooner)
 *   fused_min_tiles      shortest segment in 8 KiB tiles (default 8: each segment but a stream's first
 *                        re-runs one warm-up tile); not applied while the launch cannot fill the GPU
 *   fused_tiles_per_seg  > 0: exactly this segment length (tests)
 *   pass0_engine         -1 compiled default, 0 v_dot4, 1 int8 MFMA (as rtlfm_gpu_set_path 3 / 4)
 *   tail_serial          1: audio tail on the front end's stream, no overlap with the next step
 *   tail_priority        -1 (default) / 0 / 1: the tail's own stream at the lowest / default / highest HIP priority.  Not a
 *                        scheduling hint: streams of one priority share four hardware queues, and a tail that shares the
 *                        front end's queue runs behind the next step instead of beside it; another priority = another pool
 *   deemph_sequential    1: deemph_filter one lane per stream, never parallel over time
 *   deemph_four_pass     1: no one-pass (speculative) deemph kernels
 *   lpr_separate         1: low_pass_real as a kernel of its own behind deemph_filter
 *   lpr_scalar_stores    1: the resampler's outputs one by one
 *   lpr_chunk            most samples per lane of the one-pass deemph + low_pass_real kernel (default 5440; 256 ... 2^20,
 *                        anything else -EINVAL); shorter runs get shorter chunks so that about 64 K lanes work
 *   lpr_threads          lanes per workgroup of that kernel: 64, 128, 192 or 256 (default; anything else -EINVAL).  A
 *                        workgroup owns whole streams (lpr_threads / chunks of them, or one with a loop over its chunks)
 *   (retired: the options of the slim -M wbfm tail, of the span form of config 3's tail and of the three-kernel -E dc answer -ENOENT)
 *   lpr_ring             1 (default): that kernel's outputs leave through LDS in aligned 64-byte pieces; 0: 16 bytes per lane
 *   squelch_fused        1 (default): rms()'s sums per buffer inside the front end + k_squelch_apply; 0: emit mode + k_squelch_*
 *   box_store            how k_boxcar_scan's outputs leave: -1 (default) by the launch's output size - beyond 192 MiB (what the
 *                        256 MiB Infinity Cache cannot keep anyway) as whole 128-byte lines with non-temporal stores, the
 *                        rest of a tile's last line waiting in LDS for the next tile; below, plain stores -, 0 / 1 = always
 *                        plain / always lines
 *   fused_store          the fifth_order front end's PCM stores with 1-3 passes (4 / 2 / 1 KiB of PCM per 8 KiB tile): -1 (default)
 *                        non-temporal with three passes (whole lines per instruction) when the launch writes more than
 *                        192 MiB, 0 / 1 = never / always (with one or two passes non-temporal stores are slower: tests only)
 *   deep_rest            1 (default): passes 6 ... 9, generic_fir and the demodulator behind k_fused<6>'s emit mode in ONE
 *                        kernel per step (k_deep_rest); 0: one staged kernel per stage
 *   apart_budget_gb      most device memory (GiB, default 16, never more than half of what is free) a placement
 *                        search may hold in candidate allocations; 0 = no search, plain allocations
 *   arb_serial           where deemph_filter + arbitrary_upsample (config 3's tail) runs: 1 = on the front end's stream, behind
 *                        it; 0 = on the tail's own stream beside the next front end, as every other tail; -1 (default) = in
 *                        line from 2048 streams on (1.5 % of config 3's step).  Setting it waits for the handle's work
 *   arb_waves            waves per stream of k_deemph_spec_arb (each takes every arb_waves-th span of 2048 samples): 0
 *                        (default) = as many as make about 16384 waves of all streams, else 1 .. 8; outside -EINVAL
 *   verify_twice         debugging: 1 = every rtlfm_gpu_run_device() executes its run TWICE from the same carried state - into
 *                        shadow rows first, then into the caller's, the device idle in between - and compares rows, lengths and
 *                        the state records on the device; a difference is reported on stderr and counted.  Separates a transient
 *                        fault of the device code from a deterministic one (tests/test_soak_gpu.py).  Twice the time and a
 *                        second set of output rows; ragged runs (short callback buffers) are not verified
 *   input_stats          1: every run also takes the ADC statistics of its raw input bytes (rtlfm_gpu_input_stats; one more
 *                        kernel, k_input_stats, in front of the front end; default 0; anything but 0 / 1 -EINVAL)
 *   input_stats_nt       that kernel's loads non-temporal (1, default) or plain (0): an A/B switch, LAB.md
 *   input_health         1: every run also takes the overload / high-level / continuity records of its raw input bytes
 *                        (rtlfm_gpu_input_health; k_input_health in front of the front end, which with input_stats on takes
 *                        the statistics in the same launch; default 0; anything but 0 / 1 -EINVAL); loads as input_stats_nt
 *   squelch_gate         1: k_scan_gate at the end of every run (see rtlfm_gpu_gate; default 0: nothing is launched, nothing
 *                        allocated; anything but 0 / 1 -EINVAL).  Needs cfg.squelch_level != 0 (-EINVAL); -ENOTSUP with a
 *                        resampler (rate_out2 > 0), post_downsample > 1, or a buffer the fifth_order passes do not divide
 *   conseq_squelch       the demod thread's limit (default 10, demod_init, src/rtl_fm.c:1613; < 0 -EINVAL)
 *   pack_results         0 (default) / 1 / 2: every ring run also leaves its results packed (see rtlfm_gpu_fetch_packed)
 *   bank_survey          0 (default) / 1: every run the channel bank takes also leaves every bin's power (see
 *                        rtlfm_gpu_bank_survey)
 *   source_dc            0 (default) / 1: runs that channels take subtract every source's smoothed buffer averages in front
 *                        of the mixers and the bank (see "source_dc" above)
 *   source_stats         0 (default) / 1: runs that channels take leave the ADC statistics of every source's raw bytes, and
 *   source_health        ... the overload / high-level / continuity records (see "source_stats" above)
 *   source_iq            0 (default) / 1: runs that channels take measure every source's second moments and rewrite its bytes
 *                        with the source's IQ-balance coefficients in front of everything else (see "source_iq" above)
 * Read-only (rtlfm_gpu_get_option):
 *   pack_us              device time of the last run's two pack launches in microseconds (waits for them); -1 when that
 *                        run was not packed or rtlfm_gpu_timing_enable was off
 *   verify_runs         runs executed under verify_twice so far, and
 *   verify_mismatches    ... how many of them differed between their two executions
 *   last_route           which front end the last run took, one of enum rtlfm_route below (0 before the first run; over the ring,
 *                        the last view's of a run with short buffers), and
 *   last_rest            ... what followed it, one of enum rtlfm_rest: the plan rtlfm_run_route() names for that run
 *   block_len            the buffer length the handle was created with
 *   ring_apart           1 / 0: the result buffers behind rtlfm_gpu_push() / _run() are / are not a quarter of the HBM
 *                        away from the ring's device input; -1 before the ring exists (it is built by the first push)
 *   ring_tries           searches the ring's placement took: 2 = the first found every candidate in the input's class and the
 *                        ring's own device inputs were moved once (the handle owns both sides there)
 *   res_apart            the same for the audio tail's work buffers against the first run's input (-1: none yet;
 *                        0 also on a caller-owned stream (rtlfm_gpu_set_stream), where no search is made - the search
 *                        times launches on the null stream and synchronises the device; a caller on its own stream
 *                        places its OWN output with rtlfm_gpu_malloc_apart before the first run: INTEGRATION.md)
 *   deep_apart           the same for the buffer a front end's emit mode writes (-M raw, the squelch, -L, 7-10 passes);
 *                        -1: this configuration has none / not allocated yet
 *   placement_ms         wall time the placement searches of this handle took, in all
 *   placement_walked_mb  most a search held in temporary allocations (MiB)
 *   placement_held_mb    what the handle's placed blocks hold NOW (MiB): a search that finds a place returns the candidate
 *                        itself, which may be a 1, 2 or 4 GiB block for a smaller request (the buffers that belong together
 *                        share one); a search that finds nothing keeps nothing and the block is exactly the request
 *   poison               1 when RTLFM_POISON=1 was in the environment at the library's first allocation: every device
 *                        allocation of both libraries is filled with 0xA5 and every run / scan first leaves 0xA5 in all of
 *                        every CU's LDS, so that nothing read before it is written goes unnoticed (debug_poison.h;
 *                        tests/test_poison_gpu.py runs the parity suites that way)
 *   ring_force_retry     1: the ring's first placement search counts as failed (tests: the path that moves the device inputs)
 *   tail_sync            1: synchronise and report after every tail kernel (debugging)
 *   fused_debug          clock-stamp experiments (2 / 18 / 4, see fused_kernel.h)
 * Returns -ENOENT for an unknown name, -EINVAL for a value out of range.
 */
int rtlfm_gpu_set_option(rtlfm_gpu *h, const char *name, long value);
int rtlfm_gpu_get_option(rtlfm_gpu *h, const char *name, long *value);

/* 0 = automatic, 1 = staged reference kernels, 2 = fused streaming kernel
 * (fails with -ENOTSUP at run time when the configuration has no fused
 * form); 3 / 4 = fused with the first decimation pass forced onto v_dot4 /
 * onto the int8 MFMA pipe (2 takes the compiled default).  For tests and A/B measurement.
 * Which kernels each value leads to for a given configuration: the route table of DESIGN.md 4.6a, rtlfm_run_route below. */
int rtlfm_gpu_set_path(rtlfm_gpu *h, int path);
/* Which path the last run took (1 or 2): 2 where a one-launch front end ran, 1 where the staged kernels decimated.  The
 * read-only options "last_route" and "last_rest" say which front end and what followed it (enum rtlfm_route / rtlfm_rest). */
int rtlfm_gpu_last_path(rtlfm_gpu *h);

/*
 * A run's plan.  rtlfm_gpu_run_device() decides everything it can before its first launch - which front end, what
 * follows it, where the carried state is copied - from the configuration, the buffer count, a handful of options and the
 * alignment of the caller's rows, and from nothing else; rtlfm_run_route() makes the same plan without a handle and
 * without a GPU.  What "last_route" reads (0 before the first run):
 */
enum rtlfm_route {
	RTLFM_ROUTE_STAGED = 1,           /* k_convert, a kernel per pass (k_fifth ... / k_boxcar), the staged back half */
	RTLFM_ROUTE_FUSED = 2,            /* k_fused from the bytes to the PCM */
	RTLFM_ROUTE_FUSED_EMIT = 3,       /* k_fused leaves the decimated IQ (of the first six passes at most) */
	RTLFM_ROUTE_BOXCAR = 4,           /* k_boxcar_scan from the bytes to the PCM */
	RTLFM_ROUTE_BOXCAR_EMIT = 5,      /* k_boxcar_scan leaves the decimated IQ */
	RTLFM_ROUTE_CHAN_MIX = 6,         /* channels: k_channel_mix, then as RTLFM_ROUTE_STAGED */
	RTLFM_ROUTE_CHAN_BOXCAR = 7,      /* channels: k_channel_boxcar */
	RTLFM_ROUTE_CHAN_FIR = 8,         /* channels, a filter set: k_channel_fir */
	RTLFM_ROUTE_CHAN_FIR_PLAIN = 9,   /* ... its cross-check: k_channel_mix x 2, k_channel_fir_plain, k_source_history */
	RTLFM_ROUTE_CHAN_BANK = 10,       /* channels, a bank set: k_channel_bank */
	RTLFM_ROUTE_CHAN_BANK_PLAIN = 11  /* ... its cross-check: k_bank_sums, k_bank_fft, k_bank_scatter, k_source_history */
};
/* What follows the front end ("last_rest"). */
enum rtlfm_rest {
	RTLFM_REST_NONE = 0,        /* nothing: -M raw without a squelch, the front end wrote the caller's rows (and their lengths follow) */
	RTLFM_REST_DEEP_DEMOD = 1,  /* k_deep_rest: passes 6 .., generic_fir and the demodulator in one launch; the audio tail */
	RTLFM_REST_DEEP_IQ = 2,     /* k_deep_rest without the demodulator (a squelch, -L, -M raw); the back half */
	RTLFM_REST_PER_PASS = 3,    /* a k_fifth per pass beyond the sixth, k_fir9; the back half */
	RTLFM_REST_IRREGULAR = 4,   /* buffers the passes do not divide: k_fifth up to the first such pass, k_fifth_irregular; the audio tail */
	RTLFM_REST_BACK_HALF = 5,   /* the back half: k_squelch_*, k_fm_demod / k_simple_demod, the audio tail */
	RTLFM_REST_TAIL = 6         /* the front end demodulated: k_squelch_apply where it took rms()'s sums, the audio tail */
};
enum rtlfm_channels_kind { RTLFM_CHANNELS_OFF = 0, RTLFM_CHANNELS_MIXER = 1, RTLFM_CHANNELS_FILTER = 2, RTLFM_CHANNELS_BANK = 3 };
/* What of a handle steers a run besides its configuration: rtlfm_gpu_set_path's 0 / 1 / 2, the options of these names, the
 * flag of the ring's views of short buffers (they keep to the sequential deemph_filter), and what channels are on.  A
 * fresh handle's values are 0, -1, 1, 1, 0, 0, -1, 0, 0. */
typedef struct rtlfm_route_opts {
	int32_t path, pass0_engine, squelch_fused, deep_rest, deemph_four_pass, deemph_sequential, arb_serial, no_deemph_scan, channels;
} rtlfm_route_opts;
typedef struct rtlfm_route_plan {
	int32_t route, rest;         /* enum rtlfm_route, enum rtlfm_rest */
	int32_t last_path;           /* what rtlfm_gpu_last_path() says afterwards */
	int32_t sq_front;            /* 1: the front end takes rms()'s sums and k_squelch_apply follows it */
	int32_t copy_state;          /* 1: the carried record is copied to the next one in front of the launches (else the front end does) */
	int32_t tail_follows;        /* 1: the front end is cut into segments for a launch that kernels follow */
	int32_t tail;                /* the audio tail's stages: 1 low_pass_simple, 2 deemph_filter, 4 dc_block_audio, 8 low_pass_real,
	                                16 arbitrary_resample, 32 deemph_filter as the out-of-place one-pass kernel */
	int32_t N0, Nblk, D, T;      /* complex samples per buffer; buffer b owns the outputs of Nblk inputs through a boxcar D
	                                (fifth_order passes: Nblk outputs, D = 1); outputs of a stream's run (varcnt: at most) */
	int32_t varcnt;              /* 1: the boxcar does not divide a buffer, per-stream counts */
	int32_t level, first_irr;    /* passes the fused front end runs; the first pass handed a length it does not divide (none: the pass count) */
} rtlfm_route_plan;
/*
 * The plan of a run of `nblocks` buffers on a handle of `nstreams` streams into rows whose first address has the low
 * four bits `out_low_bits` and which lie `out_stride` int16 apart.  opts == NULL: a fresh handle's values.  *plan (may be
 * NULL) is written whenever a route is returned.  Returns the route; -ENOTSUP where rtlfm_gpu_set_path(2) has no fused
 * form to take (and for channels in a state their setters refuse); the error of rtlfm_cfg_validate(); -EINVAL / -E2BIG
 * for arguments rtlfm_gpu_run_device() refuses.  The options that shape launches (fused_waves, fused_min_tiles,
 * fused_tiles_per_seg, box_store, fused_store, lpr_*, arb_waves) are no inputs: they cannot change a route.
 */
int rtlfm_run_route(const rtlfm_cfg *cfg, int nstreams, int nblocks, unsigned out_low_bits, size_t out_stride,
                    const rtlfm_route_opts *opts, rtlfm_route_plan *plan);

/*
 * HIP-event timing of the decimating front-end kernel (the dominant kernel)
 * on the stream it is launched on.  enable(1) starts recording one event pair
 * per run; read() synchronises and returns the summed milliseconds and the
 * number of launches since the last read, then clears them.
 */
int rtlfm_gpu_timing_enable(rtlfm_gpu *h, int on);
int rtlfm_gpu_timing_read(rtlfm_gpu *h, double *front_ms, int *launches);

/*
 * In-kernel clock probe of the fused fifth_order front end: with probe(1) every wave of a launch
 * records the shader clock counter and the 100 MHz real-time counter at its first and last
 * instruction; read() synchronises and returns the mean shader clock (MHz) the waves of the LAST
 * launch ran at and the span from the first wave's start to the last wave's end (ms), or -ENODATA.
 * (The package runs at its power cap on this path: the clock, not the instruction count, is what
 * moves between boxes and over a run.)
 */
int rtlfm_gpu_clock_probe(rtlfm_gpu *h, int on);
int rtlfm_gpu_clock_read(rtlfm_gpu *h, double *shader_mhz, double *span_ms);
/* The raw stamps of that launch: out[4 w .. 4 w + 3] = wave w's shader clock at its first / last
 * instruction and the 100 MHz counter at its first / last instruction.  *waves = waves of the launch
 * (out may be NULL to ask); -ENOBUFS when cap_waves is smaller. */
int rtlfm_gpu_clock_stamps(rtlfm_gpu *h, uint64_t *out, int cap_waves, int *waves);

/*
 * The box's own HBM streaming ceilings (SURVEY.md §8d asks for a measured ceiling next to the
 * nominal 8 TB/s): the front-end kernels' skeleton - one wave per contiguous segment, 8 KiB tiles,
 * non-temporal coalesced 16-byte loads with the next tile in flight, the same LDS footprint - and
 * none of their arithmetic, over `bytes` (>= 256 MiB) of device memory, `reps` launches each:
 *   *read_gbs          read only
 *   *rw_gbs            the same with one byte stored per ~write_div bytes read (16 = the /16 chain's PCM),
 *                      the written bytes a quarter of the HBM away from the read ones (rtlfm_gpu_malloc_apart);
 *                      (bytes read + bytes written) / time
 *   *rw_colocated_gbs  the same with input and output inside one allocation (the same quarter)
 *   *write_fraction    the share actually stored (2, 4, 8 or 16 bytes per lane and tile: 1/64 ... 1/8)
 * Allocates and frees its own buffers; no handle needed.  Returns 1 when the "apart" placement was found,
 * 0 when it was not (then *rw_gbs is another co-located figure), negative on error.
 */
int rtlfm_gpu_bw_probe(int device, size_t bytes, int write_div, int reps, double *read_gbs, double *rw_gbs,
                       double *rw_colocated_gbs, double *write_fraction);

/*
 * Diagnostic: evaluates the kernels' atan2 -> Q14 routine (the arithmetic of
 * polar_discriminant, src/rtl_fm.c:842-849) and the device math library's
 * atan2 chain on n host pairs yx[2k] = y, yx[2k+1] = x.  Either output may be
 * NULL.  Used by the parity tests to pin one against the other.
 */
int rtlfm_gpu_selftest_atan2(int device, const int32_t *yx, int n, int32_t *q14, int32_t *q14_libm);
/* The kernels' fast_atan2 (src/rtl_fm.c:851-872, incl. its 32-bit wrap-around) on n host pairs. */
int rtlfm_gpu_selftest_fast_atan2(int device, const int32_t *yx, int n, int32_t *q14);
/* q[i] = nd[2i] / nd[2i+1] (C's truncating division, divisor >= 1) as the resampler's walk
 * divides by fast / slow (src/rtl_fm.c:769): the magic-number form of staged_kernels.h */
int rtlfm_gpu_selftest_const_div(int device, const int32_t *nd, int n, int32_t *q);

/* What the library's handles hold right now, process-wide (rtlfm_gpu and rtlpower_gpu alike): kind 0 device
 * allocations, 1 pinned host allocations, 2 events; -EINVAL for any other kind.  For leak checks: the figures after
 * destroying a handle equal those from before creating it. */
long rtlfm_debug_live(int kind);

/*
 * rotate_90 on raw u8 IQ (src/rtl_fm.c:437-447, NEG_U8(x) = 255 - x, :375-392): sample n
 * times (+j)^n, in place on device memory, len bytes (a multiple of 8, 16-byte aligned
 * buffer), on hip_stream (NULL = the default stream).  The reference keeps this function
 * but never calls it (its live path rotates the int16 copy by -90 degrees, which the
 * decimating kernels fold into their taps); it is offered as a standalone operator.
 */
int rtlfm_gpu_rotate_90_u8(int device, void *d_buf, size_t len, void *hip_stream);

/*
 * Where the output lives relative to the input matters on MI355X: every allocation belongs to one of (as far as the
 * probes have seen) three classes of its HBM, and a kernel that reads from one class and writes into the SAME class -
 * the PCM is 1/16 of the bytes at /16 - streams 5.6 TB/s where it streams 6.5 TB/s with the writes in another class
 * (read only: 6.9).  Buffers allocated one after the other normally share a class.
 *
 * rtlfm_gpu_malloc_apart: `bytes` of device memory for a write stream that runs beside the read stream
 * of `other` (other_bytes long; only read).  A bounded search: at most eight candidates - the request's own size, then
 * 1, 2, 1, 4, 1, 2, 4 GiB (the driver's allocator serves different sizes from different places) -, each timed against
 * `other` with one short bandwidth probe, never more than 16 GiB (rtlfm_gpu_malloc_apart_ex: budget_bytes) or half of
 * the free device memory held at once, typically 5-30 ms; the step that succeeded on a device is tried first the next
 * time in this process.  A winning candidate larger than the request is kept whole (the library asks for the buffers of
 * one handle that belong together as ONE block; "placement_held_mb" says what a handle's placed blocks hold).  *apart (may
 * be NULL) = 1 when found; otherwise - buffers too small to matter (< 256 MiB streamed), no budget, every candidate in
 * `other`'s class, probe failure - every candidate is freed and a plain allocation of exactly `bytes` is returned with
 * *apart = 0: the result is always usable, nothing of a failed search is kept, and the caller can see which it got.
 * A decision rests on the MEDIAN of three separately timed probe launches per candidate.
 * The library's own result buffers behind rtlfm_gpu_push() / _run() are placed this way.
 * rtlfm_gpu_placement_probe: 1 if existing buffers `in` / `out` are in different classes, 0 if not (or too
 * small to tell); OVERWRITES the first in_bytes / 16 bytes of `out`.
 * rtlfm_gpu_malloc / _free: plain device memory through the library.
 */
int rtlfm_gpu_malloc(int device, size_t bytes, void **out);
int rtlfm_gpu_malloc_apart(int device, size_t bytes, const void *other, size_t other_bytes, void **out, int *apart);
/* The same with the search's cost in the open: budget_bytes = most the search may hold in candidates (0: no search, plain
 * memory; rtlfm_gpu_malloc_apart uses 16 GiB; never more than half of the free device memory is taken),
 * *search_ms = wall time of the call, *walked_bytes = most it held at once (either may be NULL). */
int rtlfm_gpu_malloc_apart_ex(int device, size_t bytes, const void *other, size_t other_bytes, size_t budget_bytes,
                              void **out, int *apart, double *search_ms, size_t *walked_bytes);
int rtlfm_gpu_placement_probe(int device, const void *in, size_t in_bytes, void *out, size_t out_bytes,
                              double *read_ms, double *rw_ms);
/*
 * The caller owns BOTH sides (a service that allocates its own device input and output for rtlfm_gpu_run_device, on its
 * own stream or not): one call that chooses the PAIR.  in_bytes of input memory and out_bytes of output memory in
 * different classes of the HBM: an input is allocated, a bounded search (as rtlfm_gpu_malloc_apart_ex, budget_bytes)
 * looks for its partner; if every candidate shares the input's class the input itself MOVES - a new one is allocated
 * while the old one is still held, so that it comes from somewhere else - and the search runs again, up to max_tries
 * searches (1 ... 8; the library's ring does the same with its own device inputs).  Whatever was only held to push the
 * allocator on is freed before the call returns.  *in is uninitialised device memory for the caller to fill; both
 * pointers are released with rtlfm_gpu_free.  *apart = 1 when a pair was found (0: plain allocations, usable all the
 * same), *tries = searches made, *search_ms / *walked_bytes = wall time and most memory held at once (any may be NULL).
 * Runs probe launches on the null stream and synchronises the device: call it at set-up, not while samples flow.
 */
int rtlfm_gpu_place_pair(int device, size_t in_bytes, size_t out_bytes, size_t budget_bytes, int max_tries,
                         void **in, void **out, int *apart, int *tries, double *search_ms, size_t *walked_bytes);
/* bytes from one device buffer to another on `device` (synchronous), for callers without a HIP runtime at hand. */
int rtlfm_gpu_copy(int device, void *dst, const void *src, size_t bytes);
int rtlfm_gpu_free(void *p);
/* NUMA node of the host the device hangs on (sysfs), or -1 if unknown: where the threads that fill the
 * device's staging ring should run. */
int rtlfm_gpu_device_numa_node(int device);

/*
 * The front-end planner by itself (host only, no GPU): how a launch over `nstreams` streams of `total_tiles` 8 KiB tiles each
 * is cut into segments (one wave per stream and segment).  fifth_order / tail_follows as the run would set them;
 * target_waves, min_tiles, tiles_per_seg, gss_x10: the options of the same names (0 = the library's defaults).
 * *segs = segments per stream, starts[0 .. *segs] their tile boundaries (-ENOBUFS when cap < *segs + 1).
 */
int rtlfm_plan_segments(int nstreams, int total_tiles, int fifth_order, int tail_follows, int target_waves, int min_tiles,
                        int tiles_per_seg, int gss_x10, int *segs, int *starts, int cap);

const char *rtlfm_gpu_strerror(int err);
/* (major<<16)|(minor<<8)|patch */
int rtlfm_gpu_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RTLFM_HIP_H */
