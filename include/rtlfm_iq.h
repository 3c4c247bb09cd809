/*
 * rtlfm_iq.h — IQ balance for N wideband sources: the policy between the device's measurement and the device's correction
 * (option "source_iq", include/rtlfm_hip.h; DESIGN.md section 8.5, "Source IQ").  In the place of rtl_tcp -c (iqBalance,
 * src/rtl_tcp.c:211-233), whose float one-pole level estimate over every sample has no exact parallel form: here the
 * estimate is taken from block sums of second moments, which are integers.
 *
 * The engine is pure host code fed with records: the per-buffer rtlfm_iq_sums of a source's RAW bytes, taken on the GPU
 * (rtlfm_gpu_source_iq_sums).  It needs no GPU itself.
 *
 * Per source, every `window` consecutive buffers (default 16; short buffers count as buffers and weigh by their n) form
 * totals N, SI, SQ, SII, SQQ, SIQ, and rtlfm_iq_compute decides:
 *   1. in 128-bit integers  A = N SII - SI^2,  B = N SQQ - SQ^2,  C = N SIQ - SI SQ   (central moments times N^2: the DC
 *      offset of the bytes drops out);
 *   2. A or B below N^2 min_rms^2 (default min_rms = 2), or N = 0: the window is WEAK, nothing changes, no event;
 *   3. otherwise in double, one rounded operation at a time:  g = sqrt(B / A),  s = C / sqrt(A * B);
 *   4. g outside [0.5, 2] or |s| > 0.5: the window is REJECTED - an event, nothing changes;
 *   5. |g - 1| * 16384 < deadband and |s| * 16384 < deadband (default deadband = 164, the reference's 1 %): the identity;
 *   6. else with c = sqrt(1 - s * s) and gc = g * c:
 *        gc >= 1:  a = 1,   p = -(s / c),  q = 1 / gc
 *        else:     a = gc,  p = -(s * g),  q = 1
 *      b = 0 in both, each coefficient floor(v * 16384 + 0.5): neither branch ever amplifies;
 *   7. the new coefficients replace the source's current ones, with a CHANGED event, only where one of the four differs
 *      from its current value by more than min_step (default 8).
 * The estimate is open loop - taken from raw bytes, in front of the correction - so it cannot oscillate.
 * With y = g (Qt cos phi + It sin phi) and x = It:  E[xy] / sqrt(E[x^2] E[y^2]) = sin phi  and  Qt = y / (g c) - x s / c.
 *
 * Conventions as include/rtlfm_hip.h: int results, 0 or -errno.
 */
#ifndef RTLFM_IQ_H
#define RTLFM_IQ_H

#include <stdint.h>

#include "rtlfm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what rtlfm_iq_compute returns (>= 0) */
#define RTLFM_IQ_OK       0  /* coef holds the window's coefficients (the identity inside the deadband) */
#define RTLFM_IQ_WEAK     1  /* too little signal: coef, g_q14, s_q14 untouched */
#define RTLFM_IQ_REJECTED 2  /* g or s outside what a tuner's mismatch can be: coef untouched, g_q14 / s_q14 written */

/* event kinds */
#define RTLFM_IQ_EVENT_CHANGED  0
#define RTLFM_IQ_EVENT_REJECTED 1

typedef struct rtlfm_iq_event {
	int32_t source;
	int32_t kind;            /* RTLFM_IQ_EVENT_* */
	int16_t coef[4];         /* (a, b, p, q) as they rule after the event */
	int32_t g_q14, s_q14;    /* the window's estimates, floor(v * 16384 + 0.5), g_q14 at most 2^30 */
	int64_t window_serial;   /* this source's window number from 0 on which the decision fell */
} rtlfm_iq_event;  /* 32 bytes */

typedef struct rtlfm_iq rtlfm_iq;

/* The rule above on one set of totals; deadband >= 0 (Q14), min_rms in 0 .. 128.  g_q14 / s_q14 may be NULL. */
int rtlfm_iq_compute(const rtlfm_iq_sums *total, int32_t deadband, int32_t min_rms, int16_t coef[4], int32_t *g_q14, int32_t *s_q14);

int rtlfm_iq_create(int nsources, rtlfm_iq **out);
int rtlfm_iq_destroy(rtlfm_iq *e);
/* n consecutive buffers of `source`. */
int rtlfm_iq_feed(rtlfm_iq *e, int source, const rtlfm_iq_sums *recs, int n);
/* Feed every source from the handle's last run.  -ENODATA unless the handle's option "source_iq" is set and its last run
 * was one that channels took, -EINVAL when the handle's source count differs from the engine's.  Call it once per run. */
int rtlfm_iq_update(rtlfm_iq *e, rtlfm_gpu *h);
/* Take up to cap events, oldest first, every source's in its own order; *n = how many were written. */
int rtlfm_iq_poll(rtlfm_iq *e, rtlfm_iq_event *ev, int cap, int *n);
/* The coefficients as they rule now, [nsources][4]: what rtlfm_gpu_set_source_iq takes. */
int rtlfm_iq_coeffs(rtlfm_iq *e, int16_t *out);
/* window 1 .. 4096, deadband >= 0, min_rms 0 .. 128, min_step >= 0 (-EINVAL, nothing changed).  Windows in progress start over. */
int rtlfm_iq_set_params(rtlfm_iq *e, int32_t window, int32_t deadband, int32_t min_rms, int32_t min_step);

#ifdef __cplusplus
}
#endif
#endif /* RTLFM_IQ_H */
