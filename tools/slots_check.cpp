// tools/slots_check.cpp — the slot allocator (rtlsdr_amd/csrc/slots.cpp) under AddressSanitizer + UBSan.
//
// A stand-alone CPU program: it is compiled TOGETHER with slots.cpp, is never loaded into Python and needs no GPU.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer
//       -o slots_check tools/slots_check.cpp rtlsdr_amd/csrc/slots.cpp     (one command line)
//   ./slots_check [seed] [sequences]
//
// It drives rtlfm_slots_* through what tests/test_slots_cpu.py drives it through - seeded random power sequences over
// random shapes (levels up to 2^63, frames of 0 among them), the refusals - and compares every step's bins, idle flags and
// events with a second, slower implementation of the header's rules written here (per source: sort all candidates, no
// scratch arrays).  Output arrays are allocated to EXACTLY the size the header states, so a write past them is a report.
// Exit status 0 and the line "slots_check: ok ..." when nothing was reported.
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <random>
#include <vector>

#include "../include/rtlfm_slots.h"

static int fail(const char *what, long seq, int step)
{
	fprintf(stderr, "slots_check: FAILED: %s (sequence %ld, step %d)\n", what, seq, step);
	return 1;
}

struct Model {
	int N, K, S;
	uint64_t open, close;
	int hang, park;
	std::vector<uint8_t> mask;
	std::vector<int> bin;
	std::vector<long> quiet;
	std::vector<rtlfm_slots_event> ev;
	static bool ge(uint64_t p, uint64_t lv, int fr) { return (unsigned __int128)p >= (unsigned __int128)lv * (unsigned)fr; }
	void step(const uint64_t *power, const int32_t *frames)
	{
		ev.clear();
		for (int a = 0; a < N; a++) {
			const int fr = frames[a];
			if (!fr) continue;
			const uint64_t *pw = power + (size_t)a * K;
			std::vector<int> before(bin.begin() + (size_t)a * S, bin.begin() + (size_t)(a + 1) * S);
			int *b = bin.data() + (size_t)a * S;
			long *q = quiet.data() + (size_t)a * S;
			for (int s = 0; s < S; s++) {
				if (b[s] < 0) continue;
				q[s] = ge(pw[b[s]], close, fr) ? 0 : q[s] + 1;
				if (q[s] > hang) { b[s] = -1; q[s] = 0; }
			}
			std::vector<int> cand;
			for (int k = 0; k < K; k++)
				if (!mask[k] && std::find(b, b + S, k) == b + S && ge(pw[k], open, fr)) cand.push_back(k);
			std::stable_sort(cand.begin(), cand.end(), [pw](int x, int y) { return pw[x] > pw[y]; });  // (stable: ties stay by bin)
			size_t c = 0;
			for (int s = 0; s < S && c < cand.size(); s++)
				if (b[s] < 0) { b[s] = cand[c++]; q[s] = 0; }
			for (int s = 0; s < S; s++)
				if (b[s] != before[s]) ev.push_back({a, s, before[s], b[s]});
		}
	}
};

int main(int argc, char **argv)
{
	const unsigned seed = argc > 1 ? (unsigned)strtoul(argv[1], nullptr, 0) : 1u;
	const long nseq = argc > 2 ? strtol(argv[2], nullptr, 0) : 300;
	std::mt19937_64 rng(seed);
	long steps = 0, changes = 0;

	// the refusals
	{
		rtlfm_slots *sl = nullptr;
		rtlfm_slots_cfg c{100, 50, 1, 0, nullptr};
		rtlfm_slots_cfg bad = c;
		bad.close_level = 101;
		if (rtlfm_slots_create(1, 4, 1, &bad, &sl) != -EINVAL) return fail("close > open accepted", -1, 0);
		bad = c; bad.park = 4;
		if (rtlfm_slots_create(1, 4, 1, &bad, &sl) != -EINVAL) return fail("park == K accepted", -1, 0);
		bad = c; bad.park = -1;
		if (rtlfm_slots_create(1, 4, 1, &bad, &sl) != -EINVAL) return fail("park < 0 accepted", -1, 0);
		bad = c; bad.hang = -1;
		if (rtlfm_slots_create(1, 4, 1, &bad, &sl) != -EINVAL) return fail("hang < 0 accepted", -1, 0);
		if (rtlfm_slots_create(0, 4, 1, &c, &sl) != -EINVAL || rtlfm_slots_create(1, 0, 1, &c, &sl) != -EINVAL ||
		    rtlfm_slots_create(1, 4, 0, &c, &sl) != -EINVAL || rtlfm_slots_create(1, 4, 1, nullptr, &sl) != -EINVAL ||
		    rtlfm_slots_create(1, 4, 1, &c, nullptr) != -EINVAL)
			return fail("a bad shape or NULL accepted", -1, 0);
		if (sl) return fail("a refused create wrote a handle", -1, 0);
		if (rtlfm_slots_create(1, 4, 1, &c, &sl) != 0) return fail("create", -1, 0);
		std::vector<uint64_t> p(4, 0);
		int32_t f = -1;
		if (rtlfm_slots_step(sl, p.data(), &f) != -EINVAL || rtlfm_slots_step(sl, nullptr, &f) != -EINVAL) return fail("a bad step accepted", -1, 0);
		rtlfm_slots_destroy(sl);
		if (rtlfm_slots_destroy(nullptr) != -EINVAL) return fail("destroy(NULL)", -1, 0);
	}

	for (long seq = 0; seq < nseq; seq++) {
		Model m;
		m.N = 1 + (int)(rng() % 4);
		m.K = 1 + (int)(rng() % (seq % 3 ? 16 : 256));
		m.S = 1 + (int)(rng() % (seq % 5 ? 4 : 20));  // (also more slots than bins)
		const bool huge = seq % 4 == 3;              // levels near 2^63
		m.open = huge ? (1ull << 63) - rng() % 1000 : 1 + rng() % 1000;
		m.close = huge ? m.open - rng() % 1000 : rng() % (m.open + 1);
		m.hang = (int)(rng() % 4);
		m.park = (int)(rng() % (unsigned)m.K);
		m.mask.assign((size_t)m.K, 0);
		for (auto &v : m.mask) v = rng() % 5 == 0;
		m.bin.assign((size_t)m.N * m.S, -1);
		m.quiet.assign((size_t)m.N * m.S, 0);
		rtlfm_slots_cfg cfg{m.open, m.close, m.hang, m.park, seq % 7 == 6 ? nullptr : m.mask.data()};
		if (!cfg.mask) m.mask.assign((size_t)m.K, 0);
		rtlfm_slots *sl = nullptr;
		if (rtlfm_slots_create(m.N, m.K, m.S, &cfg, &sl) != 0) return fail("create", seq, 0);
		std::vector<uint64_t> power((size_t)m.N * m.K);
		std::vector<int32_t> frames((size_t)m.N);
		for (int st = 0; st < 40; st++, steps++) {
			for (int a = 0; a < m.N; a++) frames[(size_t)a] = rng() % 6 == 0 ? 0 : 1 + (int)(rng() % (huge ? 2 : 300));
			for (int a = 0; a < m.N; a++)
				for (int k = 0; k < m.K; k++) {
					const int fr = frames[(size_t)a] ? frames[(size_t)a] : 1;
					const unsigned kind = (unsigned)(rng() % 8);  // quiet, between the levels, loud, exactly on a level, a tie
					uint64_t v;
					if (huge) v = kind < 3 ? rng() : kind < 5 ? m.open * (uint64_t)(fr == 1) + (fr == 1 ? 0 : ~0ull) : m.close - 1;
					else v = kind < 3 ? rng() % (m.close * fr + 1) : kind == 3 ? m.open * fr : kind == 4 ? m.close * fr
					       : kind == 5 ? m.open * fr + 7 : m.open * fr + rng() % 3;
					power[(size_t)a * m.K + k] = v;
				}
			if (rtlfm_slots_step(sl, power.data(), frames.data()) != 0) return fail("step", seq, st);
			m.step(power.data(), frames.data());
			std::vector<int32_t> bins((size_t)m.N * m.S);
			std::vector<uint8_t> idle((size_t)m.N * m.S);
			if (rtlfm_slots_bins(sl, bins.data()) != 0 || rtlfm_slots_idle(sl, idle.data()) != 0) return fail("bins / idle", seq, st);
			for (size_t i = 0; i < bins.size(); i++) {
				if (idle[i] != (m.bin[i] < 0)) return fail("idle flags differ", seq, st);
				if (bins[i] != (m.bin[i] < 0 ? m.park : m.bin[i])) return fail("bins differ", seq, st);
			}
			int n = -1;
			const int want = (int)m.ev.size();
			std::vector<rtlfm_slots_event> ev((size_t)want);
			if (rtlfm_slots_events(sl, ev.data(), want, &n) != 0 || n != want) return fail("event count differs", seq, st);
			for (int i = 0; i < want; i++)
				if (ev[(size_t)i].source != m.ev[(size_t)i].source || ev[(size_t)i].slot != m.ev[(size_t)i].slot ||
				    ev[(size_t)i].old_bin != m.ev[(size_t)i].old_bin || ev[(size_t)i].new_bin != m.ev[(size_t)i].new_bin)
					return fail("events differ", seq, st);
			if (want > 0) {
				std::vector<rtlfm_slots_event> few((size_t)want - 1);
				if (rtlfm_slots_events(sl, few.data(), want - 1, &n) != -ENOBUFS || n != want) return fail("-ENOBUFS of events", seq, st);
			}
			changes += want;
		}
		rtlfm_slots_destroy(sl);
	}
	if (changes < steps / 4) return fail("the sequences hardly changed a slot: the check saw little", nseq, 0);
	printf("slots_check: ok: seed %u, %ld sequences, %ld steps, %ld changes equal to the rules written out again\n", seed, nseq, steps, changes);
	return 0;
}
