/*
 * rtlfm_agc.h — input health for N streams: the software AGC of gain mode 2 (softagc(), src/librtlsdr.c:3288-3327,
 * enabled at :1545-1548), rtl_tcp's overload report (detect_overload(), src/rtl_tcp.c:235-244) and rtl_test's
 * continuity check (underrun_test(), src/rtl_test.c:121-151).
 *
 * The engine is pure host code fed with records: the per-buffer rtlfm_input_health of the raw input, taken on the GPU
 * (rtlfm_gpu_input_health), each with the buffer's own length `len`.  It needs no GPU itself.
 *
 * Per stream, buffer by buffer in order:
 *   1. continuity (underrun_test): on the stream's first buffer bcnt = first (`uninit`).  The term at the junction is
 *      |first - bcnt| when the two differ, else 0;  lost_buf = junction + rec.lost;  bcnt = (uint8_t)(last + 1);
 *      total_samples += len;  dropped_samples += lost_buf.
 *   2. overload (detect_overload):  overloaded = 8000 * overload >= len.
 *   3. soft AGC (softagc), for a stream that has it enabled:
 *        overloaded                  -> index one down when index > 0
 *        else 8000 * high <= len     -> index one up when index < gain_count - 1
 *      Every change is an event.  index starts at 0, as mode 2 sets it (:1547).
 * 8000 * overload stays below 2^31 at RTLFM_MAX_BLOCK_LEN.
 *
 * Divergences from the reference, all deliberate:
 *   - the reference hands the new index to a worker thread, and dev->gain_index moves only once the tuner took it
 *     (:3231-3249, :1465-1485); while that is pending softagc() decides nothing.  The engine moves the index at once
 *     and is deterministic: the same records give the same indices;
 *   - settle = k (rtlfm_agc_set_settle): after a change the next k buffers of that stream make no AGC decision - they
 *     were captured before the change could act (a run takes several buffers per stream at once).  Continuity and
 *     overload are still taken from them.  The default 0 is the reference's rule;
 *   - no decision is lost when a callback is late: every buffer is counted;
 *   - rtl_tcp's -c level estimate (iqBalance) is not taken: a float one-pole recurrence over every sample has no
 *     exact parallel form.
 *
 * Conventions as include/rtlfm_hip.h: int results, 0 or -errno.
 */
#ifndef RTLFM_AGC_H
#define RTLFM_AGC_H

#include <stdint.h>

#include "rtlfm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One change of a stream's gain index. */
typedef struct rtlfm_agc_event {
	int32_t stream;
	int32_t old_index, new_index;
	int32_t overloaded;      /* 1: stepped down on overload; 0: stepped up on a low level */
	int64_t buffer_serial;   /* this stream's buffer number from 0 on which the decision fell */
} rtlfm_agc_event;

typedef struct rtlfm_agc rtlfm_agc;

/* gain_counts[s] = entries of stream s's gain table (rtlsdr_get_tuner_gains), >= 1; enable[s] != 0: the soft AGC runs
 * for stream s (NULL = for every stream).  Continuity and overload are kept for every stream either way. */
int rtlfm_agc_create(int nstreams, const int32_t *gain_counts, const int32_t *enable, rtlfm_agc **out);
int rtlfm_agc_destroy(rtlfm_agc *a);

/* n consecutive buffers of `stream`: their records and their own lengths in bytes (> 0). */
int rtlfm_agc_feed(rtlfm_agc *a, int stream, const rtlfm_input_health *recs, const uint32_t *lens, int n);
/* Feed every stream from the handle's last run, every buffer with the handle's buffer length (the read-only option
 * "block_len"; a caller whose runs hold shorter buffers knows their lengths and feeds by hand).  -ENODATA unless the
 * handle's option "input_health" is set, -EINVAL when the handle's stream count differs from the engine's.  Call it
 * once per run. */
int rtlfm_agc_update(rtlfm_agc *a, rtlfm_gpu *h);
/* Take up to cap events, oldest first, every stream's in its own order; *n = how many were written. */
int rtlfm_agc_poll(rtlfm_agc *a, rtlfm_agc_event *ev, int cap, int *n);
/* Any of the four outputs may be NULL.  overloaded_last: detect_overload's verdict on the stream's last buffer. */
int rtlfm_agc_state(rtlfm_agc *a, int stream, int32_t *index, int32_t *overloaded_last, uint64_t *total_samples,
                    uint64_t *dropped_samples);
/* Put the stream's index where the caller's tuner is (0 .. gain_count - 1); no event. */
int rtlfm_agc_set_index(rtlfm_agc *a, int stream, int32_t index);
/* settle = k >= 0 for every stream, see above. */
int rtlfm_agc_set_settle(rtlfm_agc *a, int32_t k);

#ifdef __cplusplus
}
#endif
#endif /* RTLFM_AGC_H */
