// iq.cpp — the IQ-balance engine of include/rtlfm_iq.h: from the per-buffer second moments of every source's raw bytes
// (k_source_iq, option source_iq) to the four Q14 coefficients the same kernel applies.  In the place of iqBalance
// (reference src/rtl_tcp.c:211-233).
//
// Pure host code.  The moments and the weak-signal test are integer (128 bits); g, s and the coefficients are double, one
// rounded operation per statement (the build has -ffp-contract=off): tests/source_iq_model.py repeats them in Python and
// the int16 results are equal, not close.
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <deque>
#include <new>
#include <vector>

#include "../../include/rtlfm_iq.h"

namespace {

typedef __int128 i128;

struct SourceIq {
	rtlfm_iq_sums total{};   // the window so far (n is the samples' count; windows of 4096 longest buffers stay below 2^32)
	int32_t buffers = 0;
	int64_t serial = 0;      // windows decided so far
	int16_t coef[4] = {16384, 0, 0, 16384};
};

int16_t q14(double v) { return (int16_t)std::floor(v * 16384.0 + 0.5); }

}  // namespace

struct rtlfm_iq {
	std::vector<SourceIq> s;
	std::deque<rtlfm_iq_event> events;
	int32_t window = 16, deadband = 164, min_rms = 2, min_step = 8;
	std::vector<rtlfm_iq_sums> records;  // rtlfm_iq_update's copy
};

extern "C" int rtlfm_iq_compute(const rtlfm_iq_sums *t, int32_t deadband, int32_t min_rms, int16_t coef[4], int32_t *g_q14, int32_t *s_q14)
{
	if (!t || !coef || deadband < 0 || min_rms < 0 || min_rms > 128) return -EINVAL;
	const i128 N = (i128)t->n;
	const i128 A = N * (i128)t->sii - (i128)t->si * (i128)t->si;
	const i128 B = N * (i128)t->sqq - (i128)t->sq * (i128)t->sq;
	const i128 C = N * (i128)t->siq - (i128)t->si * (i128)t->sq;
	const i128 floor_ = N * N * (i128)min_rms * (i128)min_rms;
	if (N == 0 || A <= 0 || B <= 0 || A < floor_ || B < floor_) return RTLFM_IQ_WEAK;
	const double a_ = (double)A, b_ = (double)B, c_ = (double)C;
	const double ratio = b_ / a_;
	const double g = std::sqrt(ratio);
	const double ab = a_ * b_;
	const double root = std::sqrt(ab);
	const double s = c_ / root;
	if (g_q14) {
		const double gq = std::floor(g * 16384.0 + 0.5);
		*g_q14 = gq > 1073741824.0 ? 1073741824 : (int32_t)gq;
	}
	if (s_q14) *s_q14 = (int32_t)std::floor(s * 16384.0 + 0.5);
	if (g < 0.5 || g > 2.0 || std::fabs(s) > 0.5) return RTLFM_IQ_REJECTED;
	const double dg = std::fabs(g - 1.0) * 16384.0, ds = std::fabs(s) * 16384.0;
	if (dg < (double)deadband && ds < (double)deadband) {
		coef[0] = 16384; coef[1] = 0; coef[2] = 0; coef[3] = 16384;
		return RTLFM_IQ_OK;
	}
	const double ss = s * s;
	const double one_ss = 1.0 - ss;
	const double c = std::sqrt(one_ss);
	const double gc = g * c;
	double a, p, q;
	if (gc >= 1.0) {
		a = 1.0;
		const double sc = s / c;
		p = -sc;
		q = 1.0 / gc;
	} else {
		a = gc;
		const double sg = s * g;
		p = -sg;
		q = 1.0;
	}
	coef[0] = q14(a); coef[1] = 0; coef[2] = q14(p); coef[3] = q14(q);
	return RTLFM_IQ_OK;
}

extern "C" int rtlfm_iq_create(int nsources, rtlfm_iq **out)
{
	if (!out) return -EINVAL;
	*out = nullptr;
	if (nsources < 1) return -EINVAL;
	rtlfm_iq *e = new (std::nothrow) rtlfm_iq;
	if (!e) return -ENOMEM;
	e->s.resize((size_t)nsources);
	*out = e;
	return 0;
}

extern "C" int rtlfm_iq_destroy(rtlfm_iq *e)
{
	if (!e) return -EINVAL;
	delete e;
	return 0;
}

extern "C" int rtlfm_iq_feed(rtlfm_iq *e, int source, const rtlfm_iq_sums *recs, int n)
{
	if (!e || source < 0 || (size_t)source >= e->s.size() || n < 0 || (n > 0 && !recs)) return -EINVAL;
	for (int b = 0; b < n; b++)
		if (recs[b].n == 0 || recs[b].n > RTLFM_MAX_BLOCK_LEN / 2) return -EINVAL;  // before anything is counted
	SourceIq &q = e->s[(size_t)source];
	for (int b = 0; b < n; b++) {
		const rtlfm_iq_sums &r = recs[b];
		q.total.n += r.n; q.total.clipped += r.clipped;
		q.total.si += r.si; q.total.sq += r.sq; q.total.sii += r.sii; q.total.sqq += r.sqq; q.total.siq += r.siq;
		if (++q.buffers < e->window) continue;
		int16_t coef[4];
		int32_t g = 0, s = 0;
		const int verdict = rtlfm_iq_compute(&q.total, e->deadband, e->min_rms, coef, &g, &s);
		q.total = rtlfm_iq_sums{};
		q.buffers = 0;
		const int64_t serial = q.serial++;
		if (verdict < 0) return verdict;
		if (verdict == RTLFM_IQ_WEAK) continue;
		rtlfm_iq_event ev{};
		ev.source = source; ev.g_q14 = g; ev.s_q14 = s; ev.window_serial = serial;
		if (verdict == RTLFM_IQ_REJECTED) {
			ev.kind = RTLFM_IQ_EVENT_REJECTED;
			memcpy(ev.coef, q.coef, sizeof(ev.coef));
			e->events.push_back(ev);
			continue;
		}
		bool moved = false;
		for (int k = 0; k < 4; k++) {
			const int d = (int)coef[k] - (int)q.coef[k];
			if ((d < 0 ? -d : d) > e->min_step) moved = true;
		}
		if (!moved) continue;
		memcpy(q.coef, coef, sizeof(q.coef));
		ev.kind = RTLFM_IQ_EVENT_CHANGED;
		memcpy(ev.coef, q.coef, sizeof(ev.coef));
		e->events.push_back(ev);
	}
	return 0;
}

extern "C" int rtlfm_iq_update(rtlfm_iq *e, rtlfm_gpu *h)
{
	if (!e || !h) return -EINVAL;
	const int S = (int)e->s.size();
	// the handle's source count: a copy sized for S sources must not be written by a larger handle
	rtlfm_iq_sums probe;
	int n = 0;
	int r = rtlfm_gpu_source_iq_sums(h, S - 1, &probe, 0, &n);  // -EINVAL: fewer sources; -ENODATA: option off; else *n
	if (r == -EINVAL || r == -ENODATA) return r;
	if (r != -ENOBUFS && r < 0) return r;
	if (rtlfm_gpu_source_iq_sums(h, S, &probe, 0, &n) != -EINVAL) return -EINVAL;  // the handle has more sources
	if (n <= 0) return 0;
	e->records.resize((size_t)S * n);
	if ((r = rtlfm_gpu_source_iq_sums_all(h, e->records.data(), n, &n)) < 0) return r;
	for (int s = 0; s < S; s++)
		if ((r = rtlfm_iq_feed(e, s, e->records.data() + (size_t)s * n, n)) < 0) return r;
	return 0;
}

extern "C" int rtlfm_iq_poll(rtlfm_iq *e, rtlfm_iq_event *ev, int cap, int *n)
{
	if (!e || !n || cap < 0 || (cap > 0 && !ev)) return -EINVAL;
	int k = 0;
	while (k < cap && !e->events.empty()) {
		ev[k++] = e->events.front();
		e->events.pop_front();
	}
	*n = k;
	return 0;
}

extern "C" int rtlfm_iq_coeffs(rtlfm_iq *e, int16_t *out)
{
	if (!e || !out) return -EINVAL;
	for (size_t s = 0; s < e->s.size(); s++) memcpy(out + s * 4, e->s[s].coef, sizeof(e->s[s].coef));
	return 0;
}

extern "C" int rtlfm_iq_set_params(rtlfm_iq *e, int32_t window, int32_t deadband, int32_t min_rms, int32_t min_step)
{
	if (!e || window < 1 || window > 4096 || deadband < 0 || min_rms < 0 || min_rms > 128 || min_step < 0) return -EINVAL;
	e->window = window; e->deadband = deadband; e->min_rms = min_rms; e->min_step = min_step;
	for (SourceIq &q : e->s) {
		q.total = rtlfm_iq_sums{};
		q.buffers = 0;
	}
	return 0;
}
