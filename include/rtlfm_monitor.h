/*
 * rtlfm_monitor.h — the level monitor: rtl_fm's command file (-C, README.rtlfm_cmdfile) for N streams.
 *
 * The reference averages rms() of the decimated IQ over #meas buffers, turns the mean into dB, tests it against
 * in / out / lt / gt with a tolerance, holds a trigger off for #blocks, reports the ADC maximum and ADC rms of the
 * raw bytes beside it and starts a command (src/rtl_fm.c:527-736, 1239-1254, 1302-1324, 1375-1380).  One dongle
 * hops through the file's lines there.  Here LINE i OF THE FILE IS WATCHED PERMANENTLY BY STREAM i: no retune.
 *
 * The engine is pure host code fed with records: the per-buffer rms() levels (rtlfm_gpu_levels) and the per-buffer
 * ADC statistics of the raw input (rtlfm_gpu_input_stats, taken on the GPU).  It needs no GPU itself.
 *
 * Per stream, buffer by buffer in order:
 *   1. callback side (:1305-1324), for a buffer that comes with a record:
 *        check_adc_max:  sample_max = max(sample_max, st.max)
 *        check_adc_rms:  pow_sum += (double)st.pow_sum / st.pow_count;  pow_count += 1
 *      (one double division per buffer, accumulated in buffer order: the order is part of the result)
 *   2. full_demod side (:1248-1253): if (num_summed < num_meas && rms >= 0) { level_sum += rms; num_summed++; }
 *      a negative rms() - the wrapped sum of squares, INT32_MIN from rtlfm_gpu_levels - is skipped and the cycle
 *      gets one buffer longer, as in the reference
 *   3. when num_summed >= num_meas the cycle ends (checkTriggerCommand, :652-736): the first omit_first cycles
 *      report nothing.  Otherwise the stream's hold-off counter goes down by num_meas (floor 0),
 *        level_db = 20 log10(1e-10 + level_sum / num_summed),      crit_met = testTrigCrit (:640-650),
 *        statistics (count, sum, float min / max),  adc_max = sample_max - 127,
 *        adc_rms = pow_count > 0 ? sqrt(pow_sum / pow_count) : -1;
 *      with the counter at 0 the event is FIRED when the criterion holds and the counter becomes
 *      num_block_trigger; with the counter above 0 the event says "would trigger" / "does not trigger" and
 *      blocked_for = the counter.  Then what the controller resets on its hop (:1556-1566):
 *      level_sum, num_summed, pow_sum, pow_count, sample_max.
 *
 * Divergences from the reference, all deliberate:
 *   - a stream keeps its line for good: no hop, hence no mute / -B dump and no DC-filter reset between cycles;
 *   - the hold-off counter is per stream and counts that stream's own cycles (the reference lowers every line's
 *     counter on every cycle of the one dongle);
 *   - the engine is lossless and ordered like the rest of the library: every buffer is counted (the reference's
 *     demod thread drops the buffer on which a cycle ends, :1375-1380) and lines are not limited to
 *     FREQUENCIES_LIMIT;
 *   - frequency hopping / scanning stays out of scope.
 *
 * Conventions as include/rtlfm_hip.h: int results, 0 or -errno.
 */
#ifndef RTLFM_MONITOR_H
#define RTLFM_MONITOR_H

#include <stdint.h>

#include "rtlfm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTLFM_MONITOR_AUTO_GAIN (-100)  /* AUTO_GAIN, src/rtl_fm.c:91 */
#define RTLFM_MONITOR_COMMAND_MAX 256
#define RTLFM_MONITOR_ARGS_MAX 1024

/* enum trigExpr and its print names "in", "out", "<", ">" (src/rtl_fm.c:116) */
enum rtlfm_monitor_crit { RTLFM_CRIT_IN = 0, RTLFM_CRIT_OUT = 1, RTLFM_CRIT_LT = 2, RTLFM_CRIT_GT = 3 };

/* One measurement line of the command file (struct cmd_state's per-line fields, src/rtl_fm.c:129-137). */
typedef struct rtlfm_monitor_rule {
	uint32_t freq;              /* Hz */
	int32_t gain;               /* tenths of a dB, or RTLFM_MONITOR_AUTO_GAIN */
	int32_t crit;               /* enum rtlfm_monitor_crit */
	int32_t num_meas;           /* buffers per cycle; <= 0 is taken as 10 (:611) */
	double ref_level;           /* dB */
	double ref_tol;             /* dB */
	int32_t num_block_trigger;  /* hold-off after a fired trigger, in buffers */
	int32_t check_adc_max;      /* keyword lines adc / adcmax */
	int32_t check_adc_rms;      /* keyword line adcrms */
	int32_t omit_first;         /* cycles at the start that report nothing (omitFirstFreqLevels: 3) */
	char command[RTLFM_MONITOR_COMMAND_MAX];  /* "" = none */
	char args[RTLFM_MONITOR_ARGS_MAX];
} rtlfm_monitor_rule;

/* What one finished cycle of one stream reports. */
typedef struct rtlfm_monitor_event {
	int32_t stream;
	int32_t cycle;        /* this stream's cycle number from 0, the omitted ones counted */
	int32_t crit_met;     /* testTrigCrit() */
	int32_t fired;        /* 1: the criterion held and the hold-off counter was 0 ("activates trigger") */
	int32_t blocked_for;  /* > 0: the hold-off counter ("..., blocks for n"); 0: not blocked */
	int32_t adc_max;      /* sample_max - 127 (-127 when no maximum was taken) */
	double level_db;
	double adc_rms;       /* -1 when no power was taken */
} rtlfm_monitor_event;

/* The exit statistics of one line (src/rtl_fm.c:2033-2040): mean = sum_levels / count. */
typedef struct rtlfm_monitor_stat {
	int32_t count;
	float min_level, max_level;
	double sum_levels;
} rtlfm_monitor_stat;

typedef struct rtlfm_monitor rtlfm_monitor;

/* cmd_init()'s values: crit in, 0 +- 0 dB, 10 measurements, no hold-off, omit_first 3, no command. */
void rtlfm_monitor_rule_default(rtlfm_monitor_rule *rule);

/* One rule per stream (copied). */
int rtlfm_monitor_create(int nstreams, const rtlfm_monitor_rule *rules, rtlfm_monitor **out);
int rtlfm_monitor_destroy(rtlfm_monitor *m);

/* nbuffers consecutive buffers of `stream`: their rms() levels and, where taken, their ADC records (st may be NULL). */
int rtlfm_monitor_feed(rtlfm_monitor *m, int stream, const int32_t *rms, const rtlfm_input_stat *st, int nbuffers);
/* Feed every stream from the handle's last run (one copy of the levels, one of the records).  -ENODATA unless the
 * handle has report_levels or squelch_level; without the option "input_stats" the streams are fed without records.
 * -EINVAL when the handle's stream count differs from the monitor's.  Call it once per run. */
int rtlfm_monitor_update(rtlfm_monitor *m, rtlfm_gpu *h);
/* Take up to cap finished events, oldest first, every stream's in its own order; *n = how many were written. */
int rtlfm_monitor_poll(rtlfm_monitor *m, rtlfm_monitor_event *ev, int cap, int *n);
int rtlfm_monitor_stats(rtlfm_monitor *m, int stream, rtlfm_monitor_stat *out);
/* The rule stream `stream` runs under, as the engine took it (num_meas fixed). */
int rtlfm_monitor_rule_get(rtlfm_monitor *m, int stream, rtlfm_monitor_rule *out);

/*
 * The command file's grammar (toNextCmdLine, src/rtl_fm.c:527-638), the whole file once:
 *   freq, gain, crit, level, tolerance, #meas, #blocks [, command [, args]]
 * '#' comments and blank lines are skipped; freq takes k / M / G suffixes; gain is dB or auto / a; crit is
 * in == out != <> lt < gt >; the keyword lines adc / adcmax and adcrms switch the checks on for every rule.
 * A broken line is reported on stderr with the reference's message and skipped.
 * *nrules = measurement lines found (may exceed cap: then -ENOBUFS and the first cap are written).
 * -ENOENT when the file cannot be opened, -ENODATA when it holds no valid line.
 */
int rtlfm_monitor_parse_file(const char *path, rtlfm_monitor_rule *rules, int cap, int *nrules, int *check_adc_max,
                             int *check_adc_rms);

/* The -v line of one event in the reference's wording (:716-718, :731-733), without the newline; returns its length. */
int rtlfm_monitor_format_event(const rtlfm_monitor_rule *rule, const rtlfm_monitor_event *ev, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* RTLFM_MONITOR_H */
