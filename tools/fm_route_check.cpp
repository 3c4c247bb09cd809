// fm_route_check.cpp - the run planner of csrc/run_plan.h (plan_run, through run_route = rtlfm_run_route) as a program of
// its own on the CPU, under AddressSanitizer + UBSan (tests/test_fm_route_cpu.py): the header needs no HIP and no device.
// Standard input holds one row per line - the 21 fields of rtlfm_cfg, then nstreams nblocks out_low_bits out_stride, the
// nine fields of rtlfm_route_opts, and the route and the rest expected - and every row must give them.  Then a sweep of
// its own over configurations (refused ones among them), options, alignments and buffer counts: whatever
// rtlfm_cfg_validate accepts must plan to a route - or to -ENOTSUP under rtlfm_gpu_set_path(2) or for channels their
// setters refuse -, whatever it refuses must return its error, and every plan must be consistent in itself.
#include <cerrno>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../rtlsdr_amd/csrc/run_plan.h"

using namespace rtlfm::plan;

static int fail(const char *what, long row, long got, long want)
{
	fprintf(stderr, "fm_route_check: %s %ld: got %ld, expected %ld\n", what, row, got, want);
	return 1;
}

// what a plan must satisfy whatever the configuration: 0, or the number of the rule it breaks
static int inconsistent(const rtlfm_cfg &c, const rtlfm_route_opts &o, const rtlfm_route_plan &p)
{
	const bool levels = c.squelch_level || c.report_levels;
	const bool staged = p.route == RTLFM_ROUTE_STAGED || p.route == RTLFM_ROUTE_CHAN_MIX;
	const bool plain = p.route == RTLFM_ROUTE_CHAN_FIR_PLAIN || p.route == RTLFM_ROUTE_CHAN_BANK_PLAIN;
	const bool chan = p.route >= RTLFM_ROUTE_CHAN_MIX;
	if (p.route < RTLFM_ROUTE_STAGED || p.route > RTLFM_ROUTE_CHAN_BANK_PLAIN) return 1;
	if (p.rest < RTLFM_REST_NONE || p.rest > RTLFM_REST_TAIL) return 2;
	if (chan != (o.channels != RTLFM_CHANNELS_OFF)) return 3;
	if (p.last_path != ((staged || plain) ? 1 : 2)) return 4;
	if (o.path == 1 && p.last_path != 1) return 5;
	if (o.path == 2 && p.last_path != 2) return 6;
	if (p.copy_state != (staged || chan)) return 7;
	if (p.sq_front && !(levels && (p.route == RTLFM_ROUTE_FUSED || p.route == RTLFM_ROUTE_BOXCAR))) return 8;
	if ((p.route == RTLFM_ROUTE_FUSED || p.route == RTLFM_ROUTE_BOXCAR) && (p.rest != RTLFM_REST_TAIL || p.sq_front != levels)) return 9;
	if (p.rest == RTLFM_REST_TAIL && p.route != RTLFM_ROUTE_FUSED && p.route != RTLFM_ROUTE_BOXCAR) return 10;
	if (p.rest == RTLFM_REST_NONE && (c.mode != RTLFM_MODE_RAW || levels || staged || plain)) return 11;
	if ((p.rest >= RTLFM_REST_DEEP_DEMOD && p.rest <= RTLFM_REST_PER_PASS) && (p.route != RTLFM_ROUTE_FUSED_EMIT || c.downsample_passes <= 6)) return 12;
	if ((p.rest == RTLFM_REST_IRREGULAR) != (p.first_irr < c.downsample_passes && (staged || p.route == RTLFM_ROUTE_FUSED_EMIT))) return 13;
	const bool fifth = p.route == RTLFM_ROUTE_FUSED || p.route == RTLFM_ROUTE_FUSED_EMIT;  // k_fused: fifth_order passes; every other one-launch front end: none
	if (fifth ? c.downsample_passes < 1 : (!staged && c.downsample_passes != 0)) return 14;
	if (c.mode == RTLFM_MODE_RAW && p.tail != 0) return 15;
	if (p.N0 != (int)(c.block_len / 2) || p.T < 0 || p.D < 1 || p.Nblk < 0 || p.level < 0 || p.level > 6 || p.first_irr > c.downsample_passes) return 16;
	if (p.tail_follows && chan) return 17;
	return 0;
}

int main()
{
	long rows = 0;
	for (;; rows++) {
		long v[36];
		int n = 0;
		while (n < 36 && scanf("%ld", &v[n]) == 1) n++;
		if (n == 0) break;
		if (n != 36) return fail("short row", rows, n, 36);
		rtlfm_cfg c;
		int32_t w[21];  // (21 fields of four bytes each, block_len among them)
		static_assert(sizeof(rtlfm_cfg) == sizeof(w), "rtlfm_cfg: 21 fields");
		for (int k = 0; k < 21; k++) w[k] = (int32_t)v[k];
		memcpy(&c, w, sizeof(c));
		const rtlfm_route_opts o = {(int32_t)v[25], (int32_t)v[26], (int32_t)v[27], (int32_t)v[28], (int32_t)v[29],
		                            (int32_t)v[30], (int32_t)v[31], (int32_t)v[32], (int32_t)v[33]};
		rtlfm_route_plan p{};
		const int got = run_route(&c, (int)v[21], (int)v[22], (unsigned)v[23], (size_t)v[24], &o, &p);
		if (got != (int)v[34]) return fail("row's route", rows, got, v[34]);
		if (got >= 0 && p.rest != (int)v[35]) return fail("row's rest", rows, p.rest, v[35]);
		if (got >= 0 && inconsistent(c, o, p)) return fail("row's plan breaks rule", rows, inconsistent(c, o, p), 0);
	}
	long swept = 0, planned = 0, refused = 0, notsup = 0, by_route[12] = {0}, by_rest[7] = {0};
	const int32_t modes[] = {-1, 0, 1, 3, 4, 5};
	const uint32_t lens[] = {0, 500, 512, 1536, 8192, 8704, 16384, 65536, 131072, 262144, 262656};
	const int32_t dec[][3] = {{1, 0, 0}, {0, 0, 0}, {3, 0, 0}, {10, 0, 9}, {2047, 0, 0}, {4096, 0, 0}, {200000, 0, 0}, {2, 1, 0}, {16, 4, 9},
	                          {64, 6, 0}, {0, 7, 9}, {-3, 8, 0}, {512, 9, 9}, {1024, 10, 0}, {1, 11, 0}, {1, -1, 0}, {4, 2, 5}};
	const int32_t deemph_as[] = {0, 1, 5, 30, 31, INT_MAX};
	const int32_t blocks[] = {0, 1, 4, 20000, INT_MAX};
	for (int32_t mode : modes)
		for (uint32_t len : lens)
			for (const auto &d : dec)
				for (int32_t mb : blocks)
					for (int k = 0; k < 1024; k++) {
						rtlfm_cfg c{};
						c.mode = mode; c.downsample = d[0]; c.downsample_passes = d[1]; c.comp_fir_size = d[2];
						c.custom_atan = k % 3; c.post_downsample = (k & 64) ? 2 : (k % 37 == 0 ? 17 : 1);
						c.deemph = k & 1; c.deemph_a = deemph_as[k % 6];
						c.rate_out = (k % 11 == 0) ? 0 : 24000; c.rate_out2 = (k & 2) ? ((k & 4) ? 48000 : 8000) : -1; c.resampler = (k >> 3) % 3;
						c.dc_block_audio = (k >> 5) & 1; c.adc_block_const = 9; c.dc_block_raw = k % 9 == 0; c.rdc_block_const = 9;
						c.offset_tuning = k & 1; c.output_scale = 1; c.squelch_level = (k & 16) ? 50 : 0;
						c.block_len = len; c.max_blocks = mb; c.report_levels = (k >> 8) & 1;
						const rtlfm_route_opts o = {k % 4 - (k % 13 == 0), k % 3 - 1 + 3 * (k % 17 == 0), (k >> 1) & 1, (k >> 2) & 1, (k >> 3) & 1,
						                            (k >> 4) & 1, k % 3 - 1, (k >> 6) & 1, (k >> 9) ? (k % 11 % 5) : 0};
						const int ns = (k & 32) ? 4096 : 3;
						const int nb = k % 7 == 0 ? 0 : k % 7 == 1 ? mb : k % 7 == 2 ? (mb < INT_MAX ? mb + 1 : mb) : 1;
						const unsigned low = (k & 8) ? (k % 16) : 0;
						const size_t stride = (size_t)(k % 5 == 0 ? 8 : k % 5 == 1 ? 4096 + 2 * (k % 8) : k % 5 == 2 ? 1 << 20 : 262144 + 7);
						rtlfm_route_plan p{};
						const int r = run_route(&c, ns, nb, low, stride, (k & 128) && k % 19 ? &o : nullptr, &p);
						const rtlfm_route_opts &eo = (k & 128) && k % 19 ? o : kRouteDefaults;
						swept++;
						const int v = validate_cfg(&c);
						if (v < 0) {
							if (r != v) return fail("refused configuration", swept, r, v);
							refused++;
							continue;
						}
						// the arguments rtlfm_gpu_run_device refuses, the option values the setters refuse, the channel states theirs do
						int want = 0;
						if (nb < 1 || (low & 3) || (stride & 1)) want = -EINVAL;
						else if (nb > mb) want = -E2BIG;
						else if (eo.path < 0 || eo.path > 2 || eo.pass0_engine < -1 || eo.pass0_engine > 1 || eo.channels < 0 || eo.channels > 3) want = -EINVAL;
						else if ((eo.channels && c.dc_block_raw) || (eo.channels >= 2 && c.downsample_passes > 0)) want = -ENOTSUP;
						if (want < 0) {
							if (r != want) return fail("refused arguments", swept, r, want);
							refused++;
							continue;
						}
						if (r == -ENOTSUP && eo.path == 2) { notsup++; continue; }
						if (r < 0) return fail("an accepted configuration has no route", swept, r, 0);
						if (r != p.route) return fail("return value and plan differ", swept, r, p.route);
						if (inconsistent(c, eo, p)) return fail("plan breaks rule", swept, inconsistent(c, eo, p), 0);
						planned++;
						by_route[p.route]++;
						by_rest[p.rest]++;
					}
	if (run_route(nullptr, 1, 1, 0, 8, nullptr, nullptr) != -EINVAL) return fail("null cfg", 0, 0, -EINVAL);
	if (!planned || !notsup || !refused) return fail("the sweep reached nothing of one kind", planned, notsup, refused);
	for (int k = RTLFM_ROUTE_STAGED; k <= RTLFM_ROUTE_CHAN_BANK_PLAIN; k++)
		if (!by_route[k]) return fail("the sweep never took route", k, 0, 1);
	for (int k = RTLFM_REST_NONE; k <= RTLFM_REST_TAIL; k++)
		if (!by_rest[k]) return fail("the sweep never left rest", k, 0, 1);
	printf("fm_route_check: ok, %ld rows, %ld of %ld swept planned, %ld without a fused form under path 2, %ld refused\n", rows, planned, swept,
	       notsup, refused);
	return 0;
}
