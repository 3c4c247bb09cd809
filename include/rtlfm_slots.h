/*
 * rtlfm_slots.h — the slot allocator of the channel bank for N sources: which bins of a source's K the source's few
 * demodulator slots are bound to, decided from the bank's survey (rtlfm_gpu_bank_survey, include/rtlfm_hip.h) and handed
 * back through rtlfm_gpu_set_channel_bins.
 *
 * Pure host code, integers only: it needs no GPU, and its result is a deterministic function of the surveys it was fed.
 * Per source it holds, for each of `slots` slots, the bin the slot is bound to (or that it is idle) and a count of quiet
 * runs.
 *
 * One rtlfm_slots_step() is one run's survey: power [sources][K] and frames [sources].  A bin is AT OR ABOVE a level when
 * power >= level * frames (mean power per frame; compared in 128 bits, no division).  Per source, independently:
 *   1. frames == 0: nothing changes for this source;
 *   2. every bound slot whose bin is below close_level counts one more quiet run; every other bound slot's count returns
 *      to 0;
 *   3. a slot whose count exceeds `hang` becomes idle (so: exactly after hang + 1 quiet runs in a row);
 *   4. the candidates are the bins that are not masked, not bound to a slot, and at or above open_level, ordered by power
 *      descending, ties to the lower bin;
 *   5. the candidates fill the idle slots in ascending slot order (a slot freed in step 3 included);
 *   6. a bound slot is never moved, however loud a candidate is.
 *
 * Latency: a decision made from run r's survey acts on run r + 1 (r + 2 where the survey is fetched through
 * rtlfm_gpu_bank_survey_prev).  A transmission's first buffer is lost.
 *
 * Conventions as include/rtlfm_hip.h: int results, 0 or -errno.
 */
#ifndef RTLFM_SLOTS_H
#define RTLFM_SLOTS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rtlfm_slots_cfg {
	uint64_t open_level;   /* mean power per frame at which an unbound bin becomes a candidate */
	uint64_t close_level;  /* ... below which a bound bin counts as quiet; close_level <= open_level */
	int32_t hang;          /* runs a slot stays bound after its bin fell below close_level; >= 0 */
	int32_t park;          /* the bin an idle slot is bound to, in [0, K) */
	const uint8_t *mask;   /* [K], nonzero: never assigned (bin 0's DC spike, the band edges); NULL: none.  Copied */
} rtlfm_slots_cfg;

/* One change of the last step.  An idle slot is bin -1 here (rtlfm_slots_bins hands out `park` for it). */
typedef struct rtlfm_slots_event {
	int32_t source, slot;
	int32_t old_bin, new_bin;
} rtlfm_slots_event;

typedef struct rtlfm_slots rtlfm_slots;

/* nsources >= 1; K >= 1; 1 <= slots; -EINVAL for any of these, for close_level > open_level, hang < 0, park outside
 * [0, K) or NULL pointers.  Every slot starts idle. */
int rtlfm_slots_create(int nsources, int K, int slots, const rtlfm_slots_cfg *cfg, rtlfm_slots **out);
int rtlfm_slots_destroy(rtlfm_slots *sl);
/* One run's survey: power [nsources][K], frames [nsources] (a negative count is -EINVAL and changes nothing). */
int rtlfm_slots_step(rtlfm_slots *sl, const uint64_t *power, const int32_t *frames);
/* bins [nsources][slots], ready for rtlfm_gpu_set_channel_bins: idle slots carry `park`. */
int rtlfm_slots_bins(rtlfm_slots *sl, int32_t *bins);
/* idle [nsources][slots]: 1 where the slot is idle. */
int rtlfm_slots_idle(rtlfm_slots *sl, uint8_t *idle);
/* The changes of the last step, by source, then slot: *n = how many there are; the first min(cap, *n) are written;
 * -ENOBUFS where cap < *n.  A slot freed and bound again in one step is one change. */
int rtlfm_slots_events(rtlfm_slots *sl, rtlfm_slots_event *ev, int cap, int *n);

#ifdef __cplusplus
}
#endif
#endif /* RTLFM_SLOTS_H */
