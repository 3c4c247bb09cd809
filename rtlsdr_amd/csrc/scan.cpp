// scan.cpp — the hop engine of include/rtlfm_scan.h: the controller thread's rule for several -f
// (controller_thread_fn, src/rtl_fm.c:1495-1507) for N streams, fed with the squelch gate's per-buffer records.
//
// Pure host code.  Every step cites the line of the reference whose rule it keeps.
#include <cerrno>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <new>
#include <string>
#include <vector>

#include "../../include/rtlfm_scan.h"

namespace {

struct StreamScan {
	std::vector<uint32_t> freqs;
	int32_t now = 0;       // freq_now
	int32_t hold = 0;      // buffers left that request no hop (settle)
	bool hopped = false;   // since the last rtlfm_scan_apply / _take_hopped
	int64_t serial = 0;
	uint64_t hops = 0, held = 0;
};

// one number with an optional k / M / G at its end (atofs(), convenience.c), cut to an integer; false: no number
bool parse_number(const std::string &t, int64_t *out)
{
	if (t.empty()) return false;
	std::string body = t;
	double mul = 1.0;
	switch (body.back()) {
	case 'g': case 'G': mul = 1e9; body.pop_back(); break;
	case 'm': case 'M': mul = 1e6; body.pop_back(); break;
	case 'k': case 'K': mul = 1e3; body.pop_back(); break;
	default: break;
	}
	if (body.empty()) return false;
	const unsigned char c0 = (unsigned char)body[0];
	if (!(c0 == '.' || c0 == '+' || c0 == '-' || (c0 >= '0' && c0 <= '9'))) return false;  // (strtod would take "inf", "nan", "0x..")
	if (body.find_first_of("xXnN") != std::string::npos) return false;
	char *end = nullptr;
	const double v = strtod(body.c_str(), &end);
	if (end == body.c_str() || *end) return false;
	const double f = v * mul;
	if (!(f > -1e18 && f < 1e18)) return false;
	*out = (int64_t)f;
	return true;
}

}  // namespace

struct rtlfm_scan {
	std::vector<StreamScan> s;
	std::deque<rtlfm_scan_event> events;
	uint32_t dump_bytes = RTLFM_SCAN_DEFAULT_DUMP;
	int32_t settle = 0;
	std::vector<rtlfm_gate_rec> records;  // rtlfm_scan_update's copy
};

extern "C" int rtlfm_scan_create(int nstreams, uint32_t dump_bytes, int32_t settle, rtlfm_scan **out)
{
	if (!out) return -EINVAL;
	*out = nullptr;
	if (nstreams < 1 || settle < 0) return -EINVAL;
	rtlfm_scan *sc = new (std::nothrow) rtlfm_scan;
	if (!sc) return -ENOMEM;
	sc->s.resize((size_t)nstreams);
	sc->dump_bytes = dump_bytes;
	sc->settle = settle;
	*out = sc;
	return 0;
}

extern "C" int rtlfm_scan_destroy(rtlfm_scan *sc)
{
	if (!sc) return -EINVAL;
	delete sc;
	return 0;
}

extern "C" int rtlfm_scan_set_list(rtlfm_scan *sc, int stream, const uint32_t *freqs, int n)
{
	if (!sc || stream < 0 || (size_t)stream >= sc->s.size() || !freqs || n < 1) return -EINVAL;
	StreamScan &q = sc->s[(size_t)stream];
	q.freqs.assign(freqs, freqs + n);
	q.now = 0;
	return 0;
}

extern "C" int rtlfm_scan_parse_list(const char *text, uint32_t *out, int cap, int *n)
{
	if (!text || !n || cap < 0 || (cap > 0 && !out)) return -EINVAL;
	*n = 0;
	const int64_t kMaxEntries = 1 << 24;
	int64_t count = 0;
	const char *p = text;
	while (*p) {
		while (*p == ' ' || *p == '\t' || *p == ',' || *p == '\r' || *p == '\n') p++;
		if (!*p) break;
		const char *e = p;
		while (*e && *e != ' ' && *e != '\t' && *e != ',' && *e != '\r' && *e != '\n') e++;
		const std::string tok(p, e);
		p = e;
		int64_t a = 0, b = 0, step = 1;
		const size_t c1 = tok.find(':');
		if (c1 == std::string::npos) {
			if (!parse_number(tok, &a)) return -EINVAL;
			b = a;
		} else {
			// a:b:step stands for a, a + step, ... <= b (frequency_range(), src/rtl_fm.c:1582)
			const size_t c2 = tok.find(':', c1 + 1);
			if (c2 == std::string::npos || tok.find(':', c2 + 1) != std::string::npos) return -EINVAL;
			if (!parse_number(tok.substr(0, c1), &a) || !parse_number(tok.substr(c1 + 1, c2 - c1 - 1), &b) ||
			    !parse_number(tok.substr(c2 + 1), &step))
				return -EINVAL;
			if (step <= 0 || a > b) return -EINVAL;
		}
		if (a < 0 || b > (int64_t)UINT32_MAX) return -EINVAL;
		const int64_t k = (b - a) / step + 1;
		if (count + k > kMaxEntries) return -E2BIG;
		for (int64_t i = 0; i < k; i++)
			if (count + i < cap) out[count + i] = (uint32_t)(a + i * step);
		count += k;
	}
	if (count == 0) return -EINVAL;
	*n = (int)count;
	return count > cap ? -ENOBUFS : 0;
}

extern "C" int rtlfm_scan_feed(rtlfm_scan *sc, int stream, const rtlfm_gate_rec *recs, int n)
{
	if (!sc || stream < 0 || (size_t)stream >= sc->s.size() || n < 0 || (n > 0 && !recs)) return -EINVAL;
	StreamScan &q = sc->s[(size_t)stream];
	int64_t asked_at = -1;
	for (int b = 0; b < n; b++) {
		const int64_t serial = q.serial++;
		if (!recs[b].emit) q.held++;
		if (q.hold > 0) {  // fed after a hop, maybe captured before it acted: no request
			q.hold--;
			continue;
		}
		if (!recs[b].emit && asked_at < 0) asked_at = serial;  // safe_cond_signal(&controller.hop, ...), :1369
	}
	if (asked_at < 0 || q.freqs.size() <= 1) return 0;  // :1500
	const int32_t from = q.now;
	q.now = (int32_t)((size_t)(q.now + 1) % q.freqs.size());  // :1504
	q.hops++;
	q.hopped = true;  // dongle.mute = DEFAULT_BUFFER_DUMP (:1507) is rtlfm_scan_apply's
	q.hold = sc->settle;
	sc->events.push_back({stream, from, q.now, q.freqs[(size_t)q.now], 0, asked_at});
	return 0;
}

extern "C" int rtlfm_scan_update(rtlfm_scan *sc, rtlfm_gpu *h)
{
	if (!sc || !h) return -EINVAL;
	const int S = (int)sc->s.size();
	// the handle's stream count: a copy sized for S streams must not be written by a larger handle
	rtlfm_gate_rec probe;
	int n = 0;
	int r = rtlfm_gpu_gate(h, S - 1, &probe, 0, &n);  // -EINVAL: fewer streams; -ENODATA: option off; else *n
	if (r == -EINVAL || r == -ENODATA) return r;
	if (r != -ENOBUFS && r < 0) return r;
	if (rtlfm_gpu_gate(h, S, &probe, 0, &n) != -EINVAL) return -EINVAL;  // the handle has more streams
	if (n <= 0) return 0;
	sc->records.resize((size_t)S * n);
	if ((r = rtlfm_gpu_gate_all(h, sc->records.data(), n, &n)) < 0) return r;
	for (int s = 0; s < S; s++)
		if ((r = rtlfm_scan_feed(sc, s, sc->records.data() + (size_t)s * n, n)) < 0) return r;
	return 0;
}

extern "C" int rtlfm_scan_events(rtlfm_scan *sc, rtlfm_scan_event *ev, int cap, int *n)
{
	if (!sc || !n || cap < 0 || (cap > 0 && !ev)) return -EINVAL;
	int k = 0;
	while (k < cap && !sc->events.empty()) {
		ev[k++] = sc->events.front();
		sc->events.pop_front();
	}
	*n = k;
	return 0;
}

extern "C" int rtlfm_scan_take_hopped(rtlfm_scan *sc, int32_t *streams, int cap, int *n)
{
	if (!sc || !n || cap < 0 || (cap > 0 && !streams)) return -EINVAL;
	int k = 0;
	for (size_t s = 0; s < sc->s.size(); s++)
		if (sc->s[s].hopped) k++;
	*n = k;
	if (k > cap) return -ENOBUFS;
	k = 0;
	for (size_t s = 0; s < sc->s.size(); s++)
		if (sc->s[s].hopped) {
			streams[k++] = (int32_t)s;
			sc->s[s].hopped = false;
		}
	return 0;
}

extern "C" int rtlfm_scan_apply(rtlfm_scan *sc, rtlfm_gpu *h)
{
	if (!sc || !h) return -EINVAL;
	for (size_t s = 0; s < sc->s.size(); s++) {
		if (!sc->s[s].hopped) continue;
		const int r = rtlfm_gpu_mute(h, (int)s, sc->dump_bytes);
		if (r < 0) return r;
		sc->s[s].hopped = false;
	}
	return 0;
}

extern "C" int rtlfm_scan_freq(rtlfm_scan *sc, int stream, uint32_t *freq, int32_t *index, uint64_t *hops, uint64_t *buffers,
                               uint64_t *held)
{
	if (!sc || stream < 0 || (size_t)stream >= sc->s.size()) return -EINVAL;
	const StreamScan &q = sc->s[(size_t)stream];
	if (freq) *freq = q.freqs.empty() ? 0 : q.freqs[(size_t)q.now];
	if (index) *index = q.now;
	if (hops) *hops = q.hops;
	if (buffers) *buffers = (uint64_t)q.serial;
	if (held) *held = q.held;
	return 0;
}
