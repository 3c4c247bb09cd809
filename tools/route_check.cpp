// route_check.cpp - the scan planner of csrc/rtlpower_hip.hip (plan_scan, through rtlpower_scan_route) as a program of its
// own on the CPU, under AddressSanitizer + UBSan (tests/test_power_route_cpu.py): built together with the unit, host side
// instrumented; it needs no device.  Standard input holds one row per line - the eight fields of rtlpower_cfg, then
// nstreams nreads stream_stride addr_low_bits, the six fields of rtlpower_route_opts, and the route expected - and every
// row must give that route.  Then a sweep of its own over configurations, strides and options: whatever
// rtlpower_cfg_validate accepts must plan to a route, without a finding.
#include <cerrno>
#include <cstdio>
#include <cstdlib>

#include "../include/rtlpower_hip.h"

static int fail(const char *what, long row, int got, int want)
{
	fprintf(stderr, "route_check: %s %ld: route %d, expected %d\n", what, row, got, want);
	return 1;
}

int main()
{
	long rows = 0;
	for (;; rows++) {
		long v[19];
		int n = 0;
		while (n < 19 && scanf("%ld", &v[n]) == 1) n++;
		if (n == 0) break;
		if (n != 19) return fail("short row", rows, n, 19);
		const rtlpower_cfg c = {(int32_t)v[0], (int32_t)v[1], (int32_t)v[2], (int32_t)v[3], (int32_t)v[4], (int32_t)v[5], (int32_t)v[6], (uint32_t)v[7]};
		const rtlpower_route_opts o = {(int32_t)v[12], (int32_t)v[13], (int32_t)v[14], (int32_t)v[15], (int32_t)v[16], (int32_t)v[17]};
		const int got = rtlpower_scan_route(&c, (int)v[8], (int)v[9], (size_t)v[10], (unsigned)v[11], &o);
		if (got != (int)v[18]) return fail("row", rows, got, (int)v[18]);
	}
	long swept = 0, planned = 0;
	const uint32_t lens[] = {16, 48, 4096, 16384, 32768, 49152, 65536, 262144, 1u << 22, 1u << 26};
	const int dec[][3] = {{1, 0, 1}, {1, 0, 0}, {3, 0, 0}, {2, 0, 1}, {7, 0, 1}, {4096, 0, 1}, {2, 1, 0}, {8, 3, 0}, {64, 6, 0}, {1024, 10, 0}};
	for (int bin_e = -1; bin_e <= 22; bin_e++)
		for (uint32_t len : lens)
			for (const auto &d : dec)
				for (int fir = 0; fir <= 9; fir += 9)
					for (int k = 0; k < 64; k++) {
						const rtlpower_cfg c = {bin_e, bin_e & 7, d[0], d[1], d[2], fir, k & 1, len};
						const int nreads = 1 + (k % 5) * 3, ns = k & 2 ? 1 : 1024;
						const size_t stride = (size_t)nreads * len + (k & 4 ? 8 : 0);
						const rtlpower_route_opts o = {k % 3, k >> 3 & 1, k >> 4 & 1, k % 3, k % 4, k >> 5 & 1};
						const int r = rtlpower_scan_route(&c, ns, nreads, stride, k & 8, k & 16 ? &o : nullptr);
						swept++;
						if (rtlpower_cfg_validate(&c) < 0) {
							if (r >= 0) return fail("refused configuration", swept, r, -EINVAL);
							continue;
						}
						if (r < 0 || r > RTLPOWER_KERNEL_STAGED_FAST || (r == RTLPOWER_KERNEL_NONE) != (bin_e == 0)) return fail("sweep", swept, r, 0);
						planned++;
					}
	if (rtlpower_scan_route(nullptr, 1, 1, 16, 0, nullptr) != -EINVAL) return fail("null cfg", 0, 0, -EINVAL);
	printf("route_check: ok, %ld rows, %ld of %ld swept configurations planned\n", rows, planned, swept);
	return 0;
}
