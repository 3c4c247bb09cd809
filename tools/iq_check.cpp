// iq_check.cpp — csrc/iq.cpp (include/rtlfm_iq.h) as a program of its own on the CPU, for AddressSanitizer + UBSan
// (tests/test_source_iq_cpu.py builds and runs it): seeded random records through rtlfm_iq_compute and the engine, with the
// invariants of the rule checked on every result and every refusal tried.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/iq_check.cpp rtlsdr_amd/csrc/iq.cpp
//   ./a.out [seed] [rounds]
//
// The engine's only call into the GPU library is rtlfm_iq_update's; it is stubbed here (-ENODATA: the option off).
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../include/rtlfm_iq.h"

extern "C" int rtlfm_gpu_source_iq_sums(rtlfm_gpu *, int, rtlfm_iq_sums *, int, int *) { return -ENODATA; }
extern "C" int rtlfm_gpu_source_iq_sums_all(rtlfm_gpu *, rtlfm_iq_sums *, int, int *) { return -ENODATA; }

#define CHECK(cond)                                                                  \
	do {                                                                             \
		if (!(cond)) {                                                               \
			fprintf(stderr, "iq_check: %s failed (%s:%d)\n", #cond, __FILE__, __LINE__); \
			return 1;                                                                \
		}                                                                            \
	} while (0)

// a buffer of n samples with the given spread, gain and skew, as its record
static rtlfm_iq_sums record(std::mt19937_64 &rng, uint32_t n, int spread, double g, double s)
{
	rtlfm_iq_sums r{};
	r.n = n;
	std::uniform_int_distribution<int> d(-spread, spread);
	for (uint32_t k = 0; k < n; k++) {
		const int x = d(rng), y0 = d(rng);
		double yv = g * (y0 + s * x);
		int I = x + 127, Q = (int)(yv < 0 ? yv - 0.5 : yv + 0.5) + 127;
		I = I < 0 ? 0 : I > 255 ? 255 : I;
		Q = Q < 0 ? 0 : Q > 255 ? 255 : Q;
		r.si += (uint64_t)I; r.sq += (uint64_t)Q;
		r.sii += (uint64_t)(I * I); r.sqq += (uint64_t)(Q * Q); r.siq += (uint64_t)(I * Q);
	}
	return r;
}

int main(int argc, char **argv)
{
	const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 0) : 1;
	const int rounds = argc > 2 ? atoi(argv[2]) : 100;
	std::mt19937_64 rng(seed);
	int16_t coef[4];
	int32_t g = 0, s = 0;
	// refusals
	rtlfm_iq_sums z{};
	CHECK(rtlfm_iq_compute(nullptr, 164, 2, coef, &g, &s) == -EINVAL);
	CHECK(rtlfm_iq_compute(&z, 164, 2, nullptr, &g, &s) == -EINVAL);
	CHECK(rtlfm_iq_compute(&z, -1, 2, coef, &g, &s) == -EINVAL);
	CHECK(rtlfm_iq_compute(&z, 164, 129, coef, &g, &s) == -EINVAL);
	CHECK(rtlfm_iq_compute(&z, 164, 2, coef, nullptr, nullptr) == RTLFM_IQ_WEAK);
	rtlfm_iq *e = nullptr;
	CHECK(rtlfm_iq_create(0, &e) == -EINVAL && e == nullptr);
	CHECK(rtlfm_iq_create(3, nullptr) == -EINVAL);
	CHECK(rtlfm_iq_create(3, &e) == 0 && e);
	CHECK(rtlfm_iq_set_params(e, 0, 164, 2, 8) == -EINVAL);
	CHECK(rtlfm_iq_set_params(e, 4097, 164, 2, 8) == -EINVAL);
	CHECK(rtlfm_iq_set_params(e, 4, -1, 2, 8) == -EINVAL);
	CHECK(rtlfm_iq_set_params(e, 4, 164, 2, -1) == -EINVAL);
	CHECK(rtlfm_iq_feed(e, 3, &z, 1) == -EINVAL);
	CHECK(rtlfm_iq_feed(e, 0, nullptr, 1) == -EINVAL);
	CHECK(rtlfm_iq_feed(e, 0, &z, 1) == -EINVAL);  // n == 0
	CHECK(rtlfm_iq_update(e, nullptr) == -EINVAL);
	CHECK(rtlfm_iq_update(e, reinterpret_cast<rtlfm_gpu *>(e)) == -ENODATA);
	int n = -1;
	CHECK(rtlfm_iq_poll(e, nullptr, 1, &n) == -EINVAL);
	CHECK(rtlfm_iq_poll(e, nullptr, 0, &n) == 0 && n == 0);
	CHECK(rtlfm_iq_coeffs(e, nullptr) == -EINVAL);
	// the largest window of the largest buffers at full scale: nothing overflows (UBSan watches the 128-bit products)
	{
		rtlfm_iq_sums t{};
		t.n = 4096u * 131072u;  // 2^29 (uint32: the engine's windows stay below 2^32 samples)
		t.si = (uint64_t)t.n * 255 / 2; t.sq = (uint64_t)t.n * 255 / 2;
		t.sii = (uint64_t)t.n * 65025 / 2; t.sqq = (uint64_t)t.n * 65025 / 2; t.siq = (uint64_t)t.n * 65025 / 4;
		CHECK(rtlfm_iq_compute(&t, 164, 128, coef, &g, &s) >= 0);
	}
	CHECK(rtlfm_iq_set_params(e, 4, 164, 2, 8) == 0);
	std::uniform_real_distribution<double> ug(0.3, 2.5), us(-0.7, 0.7);
	std::uniform_int_distribution<int> uspread(0, 127), ulen(1, 64);
	long changed = 0, rejected = 0;
	for (int r = 0; r < rounds; r++) {
		for (int src = 0; src < 3; src++) {
			const double gg = ug(rng), sv = us(rng);
			std::vector<rtlfm_iq_sums> recs;
			const int spread = uspread(rng);
			for (int b = 0; b < 4; b++) recs.push_back(record(rng, (uint32_t)ulen(rng) * 256u, spread, gg, sv));
			CHECK(rtlfm_iq_feed(e, src, recs.data(), (int)recs.size()) == 0);
			rtlfm_iq_sums t{};
			for (const auto &q : recs) { t.n += q.n; t.si += q.si; t.sq += q.sq; t.sii += q.sii; t.sqq += q.sqq; t.siq += q.siq; }
			int16_t c2[4] = {1, 2, 3, 4};
			const int v = rtlfm_iq_compute(&t, 164, 2, c2, &g, &s);
			CHECK(v >= 0 && v <= 2);
			if (v == RTLFM_IQ_OK) {
				CHECK(c2[1] == 0 && c2[0] > 0 && c2[0] <= 16384 && c2[3] > 0 && c2[3] <= 16384);  // never amplified
				CHECK(c2[0] == 16384 || c2[3] == 16384);
				CHECK(c2[2] >= -9500 && c2[2] <= 9500);  // |s| <= 0.5: |p| <= 0.5 / sqrt(0.75)
			} else {
				CHECK(c2[0] == 1 && c2[1] == 2 && c2[2] == 3 && c2[3] == 4);  // untouched
			}
		}
		rtlfm_iq_event ev[8];
		do {
			CHECK(rtlfm_iq_poll(e, ev, 8, &n) == 0);
			for (int k = 0; k < n; k++) {
				CHECK(ev[k].source >= 0 && ev[k].source < 3 && ev[k].window_serial == r);
				if (ev[k].kind == RTLFM_IQ_EVENT_CHANGED) changed++;
				else { CHECK(ev[k].kind == RTLFM_IQ_EVENT_REJECTED); rejected++; }
			}
		} while (n == 8);
	}
	int16_t all[12];
	CHECK(rtlfm_iq_coeffs(e, all) == 0);
	for (int src = 0; src < 3; src++) CHECK(all[src * 4 + 1] == 0 && all[src * 4] <= 16384 && all[src * 4 + 3] <= 16384);
	CHECK(rtlfm_iq_destroy(e) == 0);
	CHECK(rtlfm_iq_destroy(nullptr) == -EINVAL);
	CHECK(rounds < 20 || (changed > 0 && rejected > 0));
	printf("iq_check: ok (seed %llu, %d rounds, %ld changes, %ld rejected windows)\n", (unsigned long long)seed, rounds, changed, rejected);
	return 0;
}
