// slots.cpp — the channel bank's slot allocator for N sources (include/rtlfm_slots.h): host code, integers only.
#include <errno.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/rtlfm_slots.h"

struct rtlfm_slots {
	int nsources = 0, K = 0, slots = 0;
	uint64_t open_level = 0, close_level = 0;
	int32_t hang = 0, park = 0;
	std::vector<uint8_t> mask;        // [K]
	std::vector<int32_t> bin;         // [nsources][slots]; -1: idle
	std::vector<int64_t> quiet;       // [nsources][slots]
	std::vector<rtlfm_slots_event> ev;  // of the last step
	std::vector<uint8_t> bound;       // [K] scratch
	std::vector<int32_t> cand;        // scratch
};

// power >= level * frames, frames > 0: the product has up to 95 bits
static inline bool at_or_above(uint64_t power, uint64_t level, int32_t frames)
{
	return (unsigned __int128)power >= (unsigned __int128)level * (unsigned __int128)(uint32_t)frames;
}

extern "C" int rtlfm_slots_create(int nsources, int K, int slots, const rtlfm_slots_cfg *cfg, rtlfm_slots **out)
{
	if (!cfg || !out || nsources < 1 || K < 1 || slots < 1) return -EINVAL;
	if (cfg->close_level > cfg->open_level || cfg->hang < 0 || cfg->park < 0 || cfg->park >= K) return -EINVAL;
	if ((long long)nsources * slots > INT32_MAX || (long long)nsources * K > INT32_MAX) return -EINVAL;
	rtlfm_slots *sl = new (std::nothrow) rtlfm_slots;
	if (!sl) return -ENOMEM;
	try {
		sl->nsources = nsources; sl->K = K; sl->slots = slots;
		sl->open_level = cfg->open_level; sl->close_level = cfg->close_level;
		sl->hang = cfg->hang; sl->park = cfg->park;
		sl->mask.assign((size_t)K, 0);
		for (int k = 0; cfg->mask && k < K; k++) sl->mask[(size_t)k] = cfg->mask[k] ? 1 : 0;
		sl->bin.assign((size_t)nsources * slots, -1);
		sl->quiet.assign((size_t)nsources * slots, 0);
		sl->bound.assign((size_t)K, 0);
		sl->cand.reserve((size_t)K);
	} catch (const std::bad_alloc &) {
		delete sl;
		return -ENOMEM;
	}
	*out = sl;
	return 0;
}

extern "C" int rtlfm_slots_destroy(rtlfm_slots *sl)
{
	if (!sl) return -EINVAL;
	delete sl;
	return 0;
}

extern "C" int rtlfm_slots_step(rtlfm_slots *sl, const uint64_t *power, const int32_t *frames)
{
	if (!sl || !power || !frames) return -EINVAL;
	for (int a = 0; a < sl->nsources; a++)
		if (frames[a] < 0) return -EINVAL;
	sl->ev.clear();
	const int K = sl->K, n = sl->slots;
	for (int a = 0; a < sl->nsources; a++) {
		const int32_t fr = frames[a];
		if (fr == 0) continue;
		const uint64_t *pw = power + (size_t)a * K;
		int32_t *bin = sl->bin.data() + (size_t)a * n;
		int64_t *quiet = sl->quiet.data() + (size_t)a * n;
		const size_t ev0 = sl->ev.size();
		std::fill(sl->bound.begin(), sl->bound.end(), 0);
		int idle = 0;
		for (int s = 0; s < n; s++) {
			if (bin[s] >= 0) {
				if (!at_or_above(pw[bin[s]], sl->close_level, fr)) quiet[s]++;
				else quiet[s] = 0;
				if (quiet[s] > sl->hang) {
					sl->ev.push_back({a, s, bin[s], -1});
					bin[s] = -1;
					quiet[s] = 0;
				}
			}
			if (bin[s] >= 0) sl->bound[(size_t)bin[s]] = 1;
			else idle++;
		}
		if (idle > 0) {
			sl->cand.clear();
			for (int k = 0; k < K; k++)
				if (!sl->mask[(size_t)k] && !sl->bound[(size_t)k] && at_or_above(pw[k], sl->open_level, fr)) sl->cand.push_back(k);
			// power descending, ties to the lower bin: only as many as there are idle slots need be in order
			const size_t take = std::min(sl->cand.size(), (size_t)idle);
			std::partial_sort(sl->cand.begin(), sl->cand.begin() + (ptrdiff_t)take, sl->cand.end(),
			                  [pw](int32_t x, int32_t y) { return pw[x] != pw[y] ? pw[x] > pw[y] : x < y; });
			size_t c = 0;
			for (int s = 0; s < n && c < take; s++) {
				if (bin[s] >= 0) continue;
				bin[s] = sl->cand[c++];
				quiet[s] = 0;
				// a slot freed above and bound again is one change
				size_t e = ev0;
				while (e < sl->ev.size() && sl->ev[e].slot != s) e++;
				if (e < sl->ev.size()) sl->ev[e].new_bin = bin[s];
				else sl->ev.push_back({a, s, -1, bin[s]});
			}
			std::sort(sl->ev.begin() + (ptrdiff_t)ev0, sl->ev.end(),
			          [](const rtlfm_slots_event &x, const rtlfm_slots_event &y) { return x.slot < y.slot; });
		}
	}
	return 0;
}

extern "C" int rtlfm_slots_bins(rtlfm_slots *sl, int32_t *bins)
{
	if (!sl || !bins) return -EINVAL;
	for (size_t i = 0; i < sl->bin.size(); i++) bins[i] = sl->bin[i] >= 0 ? sl->bin[i] : sl->park;
	return 0;
}

extern "C" int rtlfm_slots_idle(rtlfm_slots *sl, uint8_t *idle)
{
	if (!sl || !idle) return -EINVAL;
	for (size_t i = 0; i < sl->bin.size(); i++) idle[i] = sl->bin[i] < 0;
	return 0;
}

extern "C" int rtlfm_slots_events(rtlfm_slots *sl, rtlfm_slots_event *ev, int cap, int *n)
{
	if (!sl || !n || cap < 0 || (cap > 0 && !ev)) return -EINVAL;
	*n = (int)sl->ev.size();
	for (int i = 0; i < cap && i < *n; i++) ev[i] = sl->ev[(size_t)i];
	return cap < *n ? -ENOBUFS : 0;
}
