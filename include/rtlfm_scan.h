/*
 * rtlfm_scan.h — the hop engine of a scanner for N streams: what rtl_fm's controller thread does with several -f
 * ("use multiple -f for scanning (requires squelch)", controller_thread_fn, src/rtl_fm.c:1495-1507), fed with the
 * squelch gate's per-buffer records (rtlfm_gate_rec, rtlfm_gpu_gate, include/rtlfm_hip.h).
 *
 * Pure host code; it needs no GPU itself.  Per stream it holds a frequency list of any length (there is no
 * FREQUENCIES_LIMIT), the index of the frequency the stream is on (freq_now) and counters.
 *
 * One rtlfm_scan_feed() is one run of the stream.  Per stream:
 *   - every buffer is counted (serial 0, 1, 2, ... over the stream's life); a buffer with emit == 0 is a HELD one: the
 *     demod thread did not hand it on and asked the controller for a hop (:1366-1370);
 *   - if the run had at least one held buffer that may request (see settle) and the list has more than one entry, the
 *     stream hops ONCE at the end of the run: freq_now = (freq_now + 1) % len (:1504); an event is queued, and the
 *     stream is marked for rtlfm_scan_apply(), which calls rtlfm_gpu_mute(h, stream, dump_bytes) (:1507);
 *   - a list of one entry never hops (:1500); a stream without a list counts as a list of one.
 *
 * Divergences from the reference, all deliberate:
 *   - the reference signals its controller once per held buffer and the condition variable coalesces signals as timing
 *     has it; here there is AT MOST ONE hop per stream per run: all buffers of a run were captured before a retune
 *     could act.  The result is a deterministic function of the records;
 *   - settle = k: the first k buffers of the stream fed after a hop request no hop (they may have been captured before
 *     the retune acted); they are still counted, and still gated on the device.  settle = 0 is the reference's rule;
 *   - every buffer of every stream is counted, none is dropped when a thread is late.
 *
 * Conventions as include/rtlfm_hip.h: int results, 0 or -errno.
 */
#ifndef RTLFM_SCAN_H
#define RTLFM_SCAN_H

#include <stdint.h>

#include "rtlfm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTLFM_SCAN_DEFAULT_DUMP 4096u  /* DEFAULT_BUFFER_DUMP, src/rtl_fm.c:1507 */

/* One hop of a stream. */
typedef struct rtlfm_scan_event {
	int32_t stream;
	int32_t from_index, to_index;  /* positions in the stream's list */
	uint32_t freq;                 /* the frequency hopped to: list[to_index] */
	uint32_t pad_;
	int64_t buffer_serial;         /* this stream's buffer number from 0: the first held buffer of the run that asked */
} rtlfm_scan_event;

typedef struct rtlfm_scan rtlfm_scan;

/* dump_bytes: what rtlfm_scan_apply mutes after a hop (RTLFM_SCAN_DEFAULT_DUMP is the reference's); settle >= 0. */
int rtlfm_scan_create(int nstreams, uint32_t dump_bytes, int32_t settle, rtlfm_scan **out);
int rtlfm_scan_destroy(rtlfm_scan *sc);
/* The stream's list (n >= 1, copied); freq_now returns to 0. */
int rtlfm_scan_set_list(rtlfm_scan *sc, int stream, const uint32_t *freqs, int n);
/*
 * A list from text, no engine needed: entries separated by blanks, tabs or commas; an entry is one frequency or a
 * range a:b:step, which stands for a, a + step, ... up to and including b (frequency_range(), src/rtl_fm.c:1573-1595);
 * every number may end in k, M or G (atofs()) and is cut to an integer as the reference does.  *n = entries the text
 * stands for; they are written to out when cap is large enough, else -ENOBUFS (out may be NULL with cap 0, to ask).
 * -EINVAL for a malformed text: no entry, something that is no number, a range with one colon or more than two,
 * step <= 0, a > b, a value above 2^32 - 1; -E2BIG for more than 2^24 entries.
 */
int rtlfm_scan_parse_list(const char *text, uint32_t *out, int cap, int *n);
/* One run of `stream`: its n gate records in order. */
int rtlfm_scan_feed(rtlfm_scan *sc, int stream, const rtlfm_gate_rec *recs, int n);
/* Feed every stream from the handle's last run through one rtlfm_gpu_gate_all.  -ENODATA unless the handle's option
 * "squelch_gate" is set, -EINVAL when the handle's stream count differs from the engine's.  Call it once per run. */
int rtlfm_scan_update(rtlfm_scan *sc, rtlfm_gpu *h);
/* Take up to cap events, oldest first; *n = how many were written. */
int rtlfm_scan_events(rtlfm_scan *sc, rtlfm_scan_event *ev, int cap, int *n);
/* rtlfm_gpu_mute(h, stream, dump_bytes) for every stream that has hopped since the last call. */
int rtlfm_scan_apply(rtlfm_scan *sc, rtlfm_gpu *h);
/* The same without a handle: streams[0 .. *n) = the streams that have hopped since the last call (and forgets them). */
int rtlfm_scan_take_hopped(rtlfm_scan *sc, int32_t *streams, int cap, int *n);
/* Where `stream` is; any output may be NULL.  hops, buffers, held: counters over the stream's life. */
int rtlfm_scan_freq(rtlfm_scan *sc, int stream, uint32_t *freq, int32_t *index, uint64_t *hops, uint64_t *buffers,
                    uint64_t *held);

#ifdef __cplusplus
}
#endif
#endif /* RTLFM_SCAN_H */
