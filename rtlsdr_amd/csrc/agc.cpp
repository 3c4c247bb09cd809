// agc.cpp — the input-health engine of include/rtlfm_agc.h: softagc() (src/librtlsdr.c:3288-3327), detect_overload()
// (src/rtl_tcp.c:235-244) and underrun_test() (src/rtl_test.c:121-151) for N streams, fed with per-buffer records.
//
// Pure host code, integer throughout.  Every step cites the line of the reference whose arithmetic it keeps.
#include <cerrno>
#include <cstdint>
#include <deque>
#include <new>
#include <vector>

#include "../../include/rtlfm_agc.h"

namespace {

struct StreamAgc {
	int32_t gain_count = 1;
	bool enabled = true;
	int32_t index = 0;        // dev->gain_index; mode 2 starts at 0 (src/librtlsdr.c:1547)
	int32_t hold = 0;         // buffers left that make no AGC decision (settle)
	bool uninit = true;       // underrun_test's static `uninit`
	uint8_t bcnt = 0;         // ... and its static `bcnt`
	int32_t overloaded = 0;
	int64_t serial = 0;
	uint64_t total = 0, dropped = 0;  // total_samples, dropped_samples (src/rtl_test.c:144-145)
};

}  // namespace

struct rtlfm_agc {
	std::vector<StreamAgc> s;
	std::deque<rtlfm_agc_event> events;
	int32_t settle = 0;
	std::vector<rtlfm_input_health> records;  // rtlfm_agc_update's copy
	std::vector<uint32_t> lens;
};

extern "C" int rtlfm_agc_create(int nstreams, const int32_t *gain_counts, const int32_t *enable, rtlfm_agc **out)
{
	if (!out) return -EINVAL;
	*out = nullptr;
	if (nstreams < 1 || !gain_counts) return -EINVAL;
	for (int i = 0; i < nstreams; i++)
		if (gain_counts[i] < 1) return -EINVAL;
	rtlfm_agc *a = new (std::nothrow) rtlfm_agc;
	if (!a) return -ENOMEM;
	a->s.resize((size_t)nstreams);
	for (int i = 0; i < nstreams; i++) {
		a->s[(size_t)i].gain_count = gain_counts[i];
		a->s[(size_t)i].enabled = enable ? enable[i] != 0 : true;
	}
	*out = a;
	return 0;
}

extern "C" int rtlfm_agc_destroy(rtlfm_agc *a)
{
	if (!a) return -EINVAL;
	delete a;
	return 0;
}

extern "C" int rtlfm_agc_feed(rtlfm_agc *a, int stream, const rtlfm_input_health *recs, const uint32_t *lens, int n)
{
	if (!a || stream < 0 || (size_t)stream >= a->s.size() || n < 0 || (n > 0 && (!recs || !lens))) return -EINVAL;
	for (int b = 0; b < n; b++)
		if (lens[b] == 0 || lens[b] > RTLFM_MAX_BLOCK_LEN) return -EINVAL;  // before anything is counted
	StreamAgc &q = a->s[(size_t)stream];
	for (int b = 0; b < n; b++) {
		const rtlfm_input_health &r = recs[b];
		const int64_t len = (int64_t)lens[b];
		// underrun_test: the term at i = 0, then the record's terms at i = 1 .. len-1
		if (q.uninit) {  // :126-130
			q.bcnt = r.first;
			q.uninit = false;
		}
		uint32_t lost = r.lost;
		if (r.first != q.bcnt)  // :133-138
			lost += r.first > q.bcnt ? (uint32_t)(r.first - q.bcnt) : (uint32_t)(q.bcnt - r.first);
		q.bcnt = (uint8_t)(r.last + 1);  // :139-141 after the last byte
		q.total += (uint64_t)len;        // :144
		q.dropped += lost;               // :145
		// detect_overload, src/rtl_tcp.c:243; softagc tests the same (src/librtlsdr.c:3308)
		q.overloaded = 8000 * (int64_t)r.overload >= len ? 1 : 0;
		const int64_t serial = q.serial++;
		if (!q.enabled) continue;
		if (q.hold > 0) {  // captured before the last change could act
			q.hold--;
			continue;
		}
		int32_t next = q.index;
		if (q.overloaded) {
			if (q.index > 0) next = q.index - 1;  // :3308-3315
		} else if (8000 * (int64_t)r.high <= len) {
			if (q.index < q.gain_count - 1) next = q.index + 1;  // :3317-3324
		}
		if (next != q.index) {
			a->events.push_back({stream, q.index, next, q.overloaded, serial});
			q.index = next;
			q.hold = a->settle;
		}
	}
	return 0;
}

extern "C" int rtlfm_agc_update(rtlfm_agc *a, rtlfm_gpu *h)
{
	if (!a || !h) return -EINVAL;
	const int S = (int)a->s.size();
	// the handle's stream count: a copy sized for S streams must not be written by a larger handle
	rtlfm_input_health probe;
	int n = 0;
	int r = rtlfm_gpu_input_health(h, S - 1, &probe, 0, &n);  // -EINVAL: fewer streams; -ENODATA: option off; else *n
	if (r == -EINVAL || r == -ENODATA) return r;
	if (r != -ENOBUFS && r < 0) return r;
	if (rtlfm_gpu_input_health(h, S, &probe, 0, &n) != -EINVAL) return -EINVAL;  // the handle has more streams
	if (n <= 0) return 0;
	long len = 0;
	if ((r = rtlfm_gpu_get_option(h, "block_len", &len)) < 0) return r;
	a->records.resize((size_t)S * n);
	if ((r = rtlfm_gpu_input_health_all(h, a->records.data(), n, &n)) < 0) return r;
	a->lens.assign((size_t)n, (uint32_t)len);
	for (int s = 0; s < S; s++)
		if ((r = rtlfm_agc_feed(a, s, a->records.data() + (size_t)s * n, a->lens.data(), n)) < 0) return r;
	return 0;
}

extern "C" int rtlfm_agc_poll(rtlfm_agc *a, rtlfm_agc_event *ev, int cap, int *n)
{
	if (!a || !n || cap < 0 || (cap > 0 && !ev)) return -EINVAL;
	int k = 0;
	while (k < cap && !a->events.empty()) {
		ev[k++] = a->events.front();
		a->events.pop_front();
	}
	*n = k;
	return 0;
}

extern "C" int rtlfm_agc_state(rtlfm_agc *a, int stream, int32_t *index, int32_t *overloaded_last, uint64_t *total_samples,
                               uint64_t *dropped_samples)
{
	if (!a || stream < 0 || (size_t)stream >= a->s.size()) return -EINVAL;
	const StreamAgc &q = a->s[(size_t)stream];
	if (index) *index = q.index;
	if (overloaded_last) *overloaded_last = q.overloaded;
	if (total_samples) *total_samples = q.total;
	if (dropped_samples) *dropped_samples = q.dropped;
	return 0;
}

extern "C" int rtlfm_agc_set_index(rtlfm_agc *a, int stream, int32_t index)
{
	if (!a || stream < 0 || (size_t)stream >= a->s.size()) return -EINVAL;
	StreamAgc &q = a->s[(size_t)stream];
	if (index < 0 || index >= q.gain_count) return -EINVAL;
	q.index = index;
	return 0;
}

extern "C" int rtlfm_agc_set_settle(rtlfm_agc *a, int32_t k)
{
	if (!a || k < 0) return -EINVAL;
	a->settle = k;
	return 0;
}
