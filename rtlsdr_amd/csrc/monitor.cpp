// monitor.cpp — the trigger engine of include/rtlfm_monitor.h: rtl_fm's command file (-C) for N streams.
//
// Pure host code.  Every step cites the line of the reference (src/rtl_fm.c) whose arithmetic it keeps; the order of
// the floating-point operations is the reference's, so that the dB values are its values.
#include <cctype>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <new>
#include <string>
#include <vector>

#include "../../include/rtlfm_monitor.h"

namespace {

struct StreamMon {
	rtlfm_monitor_rule rule;
	// what the callback accumulates (dongle_state, :167-169)
	double pow_sum = 0.0;
	int pow_count = 0;
	int sample_max = 0;
	// what full_demod accumulates (cmd_state, :138-139)
	double level_sum = 0.0;
	int num_summed = 0;
	int omit_left = 0;  // omitFirstFreqLevels
	int wait = 0;       // waitTrigger[line]
	int cycle = 0;
	rtlfm_monitor_stat stat = {0, 0.0f, 0.0f, 0.0};
};

bool crit_holds(const rtlfm_monitor_rule &r, double level)
{
	// testTrigCrit, :640-650
	const double lo = r.ref_level - r.ref_tol, hi = r.ref_level + r.ref_tol;
	switch (r.crit) {
	case RTLFM_CRIT_IN: return lo <= level && level <= hi;
	case RTLFM_CRIT_OUT: return lo > level || level > hi;
	case RTLFM_CRIT_LT: return level < lo;
	case RTLFM_CRIT_GT: return level > hi;
	}
	return false;
}

}  // namespace

struct rtlfm_monitor {
	std::vector<StreamMon> s;
	std::deque<rtlfm_monitor_event> events;
	std::vector<int32_t> levels;            // rtlfm_monitor_update's copies
	std::vector<rtlfm_input_stat> records;
};

// checkTriggerCommand, :652-736, for one stream's finished cycle
static void end_cycle(rtlfm_monitor *m, int stream)
{
	StreamMon &q = m->s[(size_t)stream];
	const rtlfm_monitor_rule &r = q.rule;
	const int cycle = q.cycle++;
	if (q.omit_left > 0) {
		q.omit_left--;  // :666-670: the first cycles report nothing (and do not touch the counter)
	} else {
		if (q.wait > 0) {  // :673-679
			q.wait -= r.num_meas;
			if (q.wait < 0) q.wait = 0;
		}
		const double level = 20.0 * log10(1E-10 + q.level_sum / q.num_summed);  // :680
		const bool crit = crit_holds(r, level);
		if (q.stat.count == 0) {  // :685-698
			q.stat.count = 1;
			q.stat.sum_levels = level;
			q.stat.min_level = (float)level;
			q.stat.max_level = (float)level;
		} else {
			q.stat.count++;
			q.stat.sum_levels += level;
			if (q.stat.min_level > (float)level) q.stat.min_level = (float)level;
			if (q.stat.max_level < (float)level) q.stat.max_level = (float)level;
		}
		rtlfm_monitor_event ev;
		ev.stream = stream;
		ev.cycle = cycle;
		ev.crit_met = crit ? 1 : 0;
		ev.adc_max = q.sample_max - 127;                                         // :660
		ev.adc_rms = q.pow_count > 0 ? sqrt(q.pow_sum / q.pow_count) : -1.0;     // :703
		ev.level_db = level;
		if (q.wait <= 0) {  // :713-714
			q.wait = crit ? r.num_block_trigger : 0;
			ev.fired = crit ? 1 : 0;
			ev.blocked_for = 0;
		} else {            // :730-733
			ev.fired = 0;
			ev.blocked_for = q.wait;
		}
		m->events.push_back(ev);
	}
	// what the controller resets when it hops (:1556-1566); here the stream stays on its line
	q.level_sum = 0.0;
	q.num_summed = 0;
	q.pow_sum = 0.0;
	q.pow_count = 0;
	q.sample_max = 0;
}

extern "C" void rtlfm_monitor_rule_default(rtlfm_monitor_rule *rule)
{
	if (!rule) return;
	memset(rule, 0, sizeof(*rule));
	rule->crit = RTLFM_CRIT_IN;
	rule->num_meas = 10;
	rule->omit_first = 3;
}

extern "C" int rtlfm_monitor_create(int nstreams, const rtlfm_monitor_rule *rules, rtlfm_monitor **out)
{
	if (!out) return -EINVAL;
	*out = nullptr;
	if (nstreams < 1 || !rules) return -EINVAL;
	for (int i = 0; i < nstreams; i++)
		if (rules[i].crit < RTLFM_CRIT_IN || rules[i].crit > RTLFM_CRIT_GT) return -EINVAL;
	rtlfm_monitor *m = new (std::nothrow) rtlfm_monitor;
	if (!m) return -ENOMEM;
	m->s.resize((size_t)nstreams);
	for (int i = 0; i < nstreams; i++) {
		StreamMon &q = m->s[(size_t)i];
		q.rule = rules[i];
		q.rule.command[RTLFM_MONITOR_COMMAND_MAX - 1] = 0;
		q.rule.args[RTLFM_MONITOR_ARGS_MAX - 1] = 0;
		if (q.rule.num_meas <= 0) q.rule.num_meas = 10;  // :611
		q.omit_left = q.rule.omit_first > 0 ? q.rule.omit_first : 0;
	}
	*out = m;
	return 0;
}

extern "C" int rtlfm_monitor_destroy(rtlfm_monitor *m)
{
	if (!m) return -EINVAL;
	delete m;
	return 0;
}

extern "C" int rtlfm_monitor_feed(rtlfm_monitor *m, int stream, const int32_t *rms, const rtlfm_input_stat *st, int nbuffers)
{
	if (!m || stream < 0 || (size_t)stream >= m->s.size() || nbuffers < 0 || (nbuffers > 0 && !rms)) return -EINVAL;
	StreamMon &q = m->s[(size_t)stream];
	for (int b = 0; b < nbuffers; b++) {
		if (st) {
			if (q.rule.check_adc_max && st[b].max > q.sample_max) q.sample_max = st[b].max;  // :1305-1312
			if (q.rule.check_adc_rms && st[b].pow_count > 0) {                                // :1322-1323
				q.pow_sum += (double)st[b].pow_sum / st[b].pow_count;
				q.pow_count += 1;
			}
		}
		if (q.num_summed < q.rule.num_meas && rms[b] >= 0) {  // :1250-1253
			q.level_sum += rms[b];
			q.num_summed++;
		}
		if (q.num_summed >= q.rule.num_meas) end_cycle(m, stream);  // :1375-1376
	}
	return 0;
}

extern "C" int rtlfm_monitor_update(rtlfm_monitor *m, rtlfm_gpu *h)
{
	if (!m || !h) return -EINVAL;
	const int S = (int)m->s.size();
	// the handle's stream count: a levels copy sized for S streams must not be written by a larger handle
	int32_t probe = 0;
	int n = 0;
	int r = rtlfm_gpu_levels(h, S - 1, &probe, 0, &n);  // -EINVAL: fewer streams; -ENODATA: no levels kept; else *n
	if (r == -EINVAL || r == -ENODATA) return r;
	if (r != -ENOBUFS && r < 0) return r;
	if (rtlfm_gpu_levels(h, S, &probe, 0, &n) != -EINVAL) return -EINVAL;  // the handle has more streams
	if (n <= 0) return 0;
	m->levels.resize((size_t)S * n);
	if ((r = rtlfm_gpu_levels_all(h, m->levels.data(), n, &n)) < 0) return r;
	m->records.resize((size_t)S * n);
	int ns = 0;
	r = rtlfm_gpu_input_stats_all(h, m->records.data(), n, &ns);
	const bool have = r == 0 && ns == n;
	if (r < 0 && r != -ENODATA && r != -ENOBUFS) return r;
	for (int s = 0; s < S; s++)
		if ((r = rtlfm_monitor_feed(m, s, m->levels.data() + (size_t)s * n, have ? m->records.data() + (size_t)s * n : nullptr, n)) < 0)
			return r;
	return 0;
}

extern "C" int rtlfm_monitor_poll(rtlfm_monitor *m, rtlfm_monitor_event *ev, int cap, int *n)
{
	if (!m || !n || cap < 0 || (cap > 0 && !ev)) return -EINVAL;
	int k = 0;
	while (k < cap && !m->events.empty()) {
		ev[k++] = m->events.front();
		m->events.pop_front();
	}
	*n = k;
	return 0;
}

extern "C" int rtlfm_monitor_stats(rtlfm_monitor *m, int stream, rtlfm_monitor_stat *out)
{
	if (!m || !out || stream < 0 || (size_t)stream >= m->s.size()) return -EINVAL;
	*out = m->s[(size_t)stream].stat;
	return 0;
}

extern "C" int rtlfm_monitor_rule_get(rtlfm_monitor *m, int stream, rtlfm_monitor_rule *out)
{
	if (!m || !out || stream < 0 || (size_t)stream >= m->s.size()) return -EINVAL;
	*out = m->s[(size_t)stream].rule;
	return 0;
}

// ---------------------------------------------------------------- the command file ----

static char *trimmed(char *s)
{
	size_t l = strlen(s);
	while (l > 0 && isspace((unsigned char)s[l - 1])) s[--l] = 0;
	while (*s && isspace((unsigned char)*s)) s++;
	return s;
}

// atofs(): a number with an optional k / M / G suffix
static double suffixed(const char *s)
{
	std::string t(s);
	while (t.size() > 1 && isspace((unsigned char)t.back())) t.pop_back();
	if (t.empty()) return 0.0;
	double mul = 1.0;
	switch (t.back()) {
	case 'g': case 'G': mul = 1e9; break;
	case 'm': case 'M': mul = 1e6; break;
	case 'k': case 'K': mul = 1e3; break;
	default: return atof(t.c_str());
	}
	t.pop_back();
	return mul * atof(t.c_str());
}

extern "C" int rtlfm_monitor_parse_file(const char *path, rtlfm_monitor_rule *rules, int cap, int *nrules, int *check_adc_max,
                                        int *check_adc_rms)
{
	if (!path || !nrules || cap < 0 || (cap > 0 && !rules)) return -EINVAL;
	*nrules = 0;
	FILE *f = fopen(path, "r");
	if (!f) return -ENOENT;
	int adc_max = 0, adc_rms = 0, line_no = 0, found = 0;
	char buf[4096];
	while (fgets(buf, sizeof(buf), f)) {
		line_no++;
		char *p = trimmed(buf);
		if (p[0] == '#' || p[0] == 0) continue;
		char *save = nullptr;
		bool first = true;
		auto field = [&]() -> char * {
			char *t = strtok_r(first ? p : nullptr, ",", &save);
			first = false;
			return t;
		};
		auto broken = [&](const char *what) { fprintf(stderr, "error parsing %s in line %d of command file!\n", what, line_no); };
		char *t = field();
		if (!t) { broken("frequency"); continue; }
		t = trimmed(t);
		if (!strcmp(t, "adc") || !strcmp(t, "adcmax")) { adc_max = 1; continue; }
		if (!strcmp(t, "adcrms")) { adc_rms = 1; continue; }
		rtlfm_monitor_rule r;
		rtlfm_monitor_rule_default(&r);
		r.freq = (uint32_t)suffixed(t);
		if (!(t = field())) { broken("gain"); continue; }
		t = trimmed(t);
		r.gain = (!strcmp(t, "auto") || !strcmp(t, "a")) ? RTLFM_MONITOR_AUTO_GAIN : (int)(atof(t) * 10);
		if (!(t = field())) { broken("expr"); continue; }
		t = trimmed(t);
		if (!strcmp(t, "in") || !strcmp(t, "==")) r.crit = RTLFM_CRIT_IN;
		else if (!strcmp(t, "out") || !strcmp(t, "!=") || !strcmp(t, "<>")) r.crit = RTLFM_CRIT_OUT;
		else if (!strcmp(t, "lt") || !strcmp(t, "<")) r.crit = RTLFM_CRIT_LT;
		else if (!strcmp(t, "gt") || !strcmp(t, ">")) r.crit = RTLFM_CRIT_GT;
		else { broken("expr"); continue; }
		if (!(t = field())) { broken("level"); continue; }
		r.ref_level = atof(trimmed(t));
		if (!(t = field())) { broken("tolerance"); continue; }
		r.ref_tol = atof(trimmed(t));
		if (!(t = field())) { broken("#measurements"); continue; }
		r.num_meas = atoi(trimmed(t));
		if (r.num_meas <= 0) {
			fprintf(stderr, "warning: fixed #measurements from %d to 10 in line %d of command file!\n", r.num_meas, line_no);
			r.num_meas = 10;
		}
		if (!(t = field())) { broken("#blockTrigger"); continue; }
		r.num_block_trigger = atoi(trimmed(t));
		// command and arguments may be missing or empty
		if ((t = field())) {
			t = trimmed(t);
			if (strlen(t) >= RTLFM_MONITOR_COMMAND_MAX) { broken("command"); continue; }
			strcpy(r.command, t);
			if ((t = field())) {
				t = trimmed(t);
				if (strlen(t) >= RTLFM_MONITOR_ARGS_MAX) { broken("command"); continue; }
				strcpy(r.args, t);
			}
		}
		if (found < cap) rules[found] = r;
		found++;
	}
	fclose(f);
	*nrules = found;
	if (check_adc_max) *check_adc_max = adc_max;
	if (check_adc_rms) *check_adc_rms = adc_rms;
	if (!found) {
		fprintf(stderr, "error: command file '%s' does not contain any valid lines!\n", path);
		return -ENODATA;
	}
	for (int i = 0; i < found && i < cap; i++) {  // the keywords hold for the whole file
		rules[i].check_adc_max = adc_max;
		rules[i].check_adc_rms = adc_rms;
	}
	return found > cap ? -ENOBUFS : 0;
}

extern "C" int rtlfm_monitor_format_event(const rtlfm_monitor_rule *r, const rtlfm_monitor_event *ev, char *buf, size_t cap)
{
	if (!r || !ev || !buf || !cap) return -EINVAL;
	char adc[128];
	adc[0] = 0;
	const char *mark = ev->adc_max >= 64 ? (ev->adc_max >= 120 ? "!!" : "! ") : "  ";  // :704
	if (r->check_adc_max && r->check_adc_rms) snprintf(adc, sizeof(adc), "adc max %3d%s rms %5.1f ", ev->adc_max, mark, ev->adc_rms);
	else if (r->check_adc_max) snprintf(adc, sizeof(adc), "adc max %3d%s ", ev->adc_max, mark);
	else if (r->check_adc_rms) snprintf(adc, sizeof(adc), "adc rms %5.1f ", ev->adc_rms);
	int n;
	if (ev->blocked_for <= 0)  // :716-718
		n = snprintf(buf, cap, "%.3f kHz: gain %4.1f + level %4.1f dB %s=> %s", (double)r->freq / 1000.0, 0.1 * r->gain, ev->level_db, adc,
		             ev->fired ? "activates trigger" : "does not trigger");
	else                       // :731-733
		n = snprintf(buf, cap, "%.3f kHz: gain %4.1f + level %4.1f dB %s=> %s, blocks for %d", (double)r->freq / 1000.0, 0.1 * r->gain,
		             ev->level_db, adc, ev->crit_met ? "would trigger" : "does not trigger", ev->blocked_for);
	return n;
}
