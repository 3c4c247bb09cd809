// power_report_kernel.h — csv_dbm()'s arithmetic (reference src/rtl_power.c:722-765) for every stream of a handle in
// one launch: the DC patch, the half swap and the crop as an index map, 10 log10 of the scaled accumulator reduced to
// what "%.2f" prints, and the reset of avg[] / samples (:761-764) in the same pass.  DESIGN.md section 4.6.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtlpower {

// One reported value: bit 31 = the sign "%.2f" prints ("-0.00" included), bits 0 .. 30 = hundredths of a dB.
// Three magnitudes are reserved; the third never leaves the library.
constexpr uint32_t kCentiSign = 0x80000000u;
constexpr uint32_t kCentiInf = 0x7fffffffu;    // kCentiSign | kCentiInf (-1 as int32) is the "-inf" of an empty bin
constexpr uint32_t kCentiNan = 0x7ffffffeu;
constexpr uint32_t kCentiDoubt = 0x7ffffffdu;  // "decided by the host": patched in before rtlpower_gpu_report_fetch returns

struct ReportDoubt {
	int32_t stream, j;  // output j of the stream; j == outn is the line's trailing value
	long long avg;      // the accumulator that output reads (after the DC patch)
};

struct ReportParams {
	long long *avg;        // [nstreams][len]
	int32_t *samples;      // [nstreams]
	int len;               // 1 << bin_e
	int i1, outn;          // first kept bin of the swapped spectrum, number of kept bins (i2 - i1 + 1)
	int patch;             // bin_e > 0: source bin 0 is read as bin 1
	int clear;             // leave avg[] and samples zero
	int groups, seg;       // workgroups per stream, source bins per workgroup (a multiple of the block size)
	double rate, guard;    // guard: distance of 100 |dBm| from a rounding boundary k + 0.5 below which the host decides
	uint32_t *out;         // [nstreams][outn + 1]: the kept bins, then the trailing value of the line (:755-760)
	int32_t *out_samples;  // [nstreams]
	uint32_t *doubt_count; // zeroed on the stream in front of every launch
	ReportDoubt *doubts;
	uint32_t doubt_cap;
	uint32_t *arrived;     // [nstreams], zero between launches: which workgroup of a stream is the last to have read samples
};

constexpr int kReportThreads = 256;

// 10 log10(x) as "%.2f" prints it, or kCentiDoubt where this arithmetic cannot tell
__device__ inline uint32_t report_centi(double x, double guard)
{
	const double dbm = 10 * log10(x);
	const double t = 100.0 * fabs(dbm), k = floor(t), f = t - k;
	if (t < 1.0e9 && fabs(f - 0.5) >= guard)  // (false for a NaN)
		return (x < 1.0 ? kCentiSign : 0u) | ((uint32_t)k + (f > 0.5 ? 1u : 0u));  // the sign of log10 x, "-0.00" included: from x itself
	return kCentiDoubt;
}

// Every source bin is loaded by exactly one thread, which is also the one that zeroes it: the store follows the load of
// the same address in the same thread.  The one bin that two outputs read - bin 1, which also stands in for bin 0 -
// reaches lane 0 through a lane exchange (bins 0 and 1 always sit in lanes 0 and 1 of one wave), not through a second
// load.  samples is read by thread 0 of every workgroup of a stream; the workgroup that arrives last at the stream's
// counter (acquire / release at device scope) zeroes it.  No zeroing depends on the order workgroups run in.
__global__ __launch_bounds__(kReportThreads) void k_power_report(ReportParams p)
{
	const int s = (int)(blockIdx.x / (unsigned)p.groups), g = (int)(blockIdx.x % (unsigned)p.groups);
	__shared__ int32_t sh_samples;
	if (threadIdx.x == 0) {
		const int32_t n = p.samples[s];
		sh_samples = n;
		if (g == 0) p.out_samples[s] = n;
	}
	__syncthreads();
	const int32_t samples = sh_samples;
	if (samples == 0 && !p.clear) return;  // a stream that was never scanned reports length 0; nothing to reset
	long long *row = p.avg + (size_t)s * p.len;
	uint32_t *orow = p.out + (size_t)s * (p.outn + 1);
	const int b0 = g * p.seg, b1 = b0 + p.seg < p.len ? b0 + p.seg : p.len;
	const double dsamples = (double)samples;
	for (int base = b0; base < b1; base += kReportThreads) {  // the same trip count in every lane: the exchange below runs in all of them
		const int b = base + (int)threadIdx.x;
		const bool live = b < b1;
		long long a = 0;
		if (live) {
			a = row[b];
			if (p.clear) row[b] = 0;
		}
		if (p.patch && base == 0) {  // uniform: only the first round of a stream's workgroup 0 holds bins 0 and 1
			const long long a_next = __shfl(a, 1);  // lane 1's bin: bin 1 where this lane holds bin 0
			if (b == 0) a = a_next;                 // "nuke DC component", :732
		}
		const int j = (b - p.i1 - (p.len >> 1)) & (p.len - 1);  // the half swap (:734-738) and the crop (:746-748)
		if (!live || samples == 0 || j >= p.outn) continue;
		// the bin's own value: two divisions in this order (:749-752); the last kept bin once more as the line's
		// trailing value, which the reference forms with ONE division by rate * samples (:755-758)
		const bool last = j == p.outn - 1;
		uint32_t w = kCentiSign | kCentiInf, wt = w;  // a == 0: 10 log10(+-0) = -inf whatever rate and samples are
		if (a != 0) {
			w = wt = kCentiDoubt;  // (a negative accumulator - a NaN - is the host's to print)
			if (a > 0) {
				double x = (double)a;
				x /= p.rate;
				x /= dsamples;
				w = report_centi(x, p.guard);
				if (last) wt = report_centi((double)a / (p.rate * dsamples), p.guard);
			}
		}
		if (w == kCentiDoubt) {
			const uint32_t at = atomicAdd(p.doubt_count, 1u);
			if (at < p.doubt_cap) p.doubts[at] = ReportDoubt{s, j, a};
		}
		orow[j] = w;
		if (last) {
			if (wt == kCentiDoubt) {
				const uint32_t at = atomicAdd(p.doubt_count, 1u);
				if (at < p.doubt_cap) p.doubts[at] = ReportDoubt{s, p.outn, a};
			}
			orow[p.outn] = wt;
		}
	}
	if (p.clear && threadIdx.x == 0) {
		if (p.groups == 1) {
			p.samples[s] = 0;
		} else if (__hip_atomic_fetch_add(&p.arrived[s], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (uint32_t)p.groups - 1) {
			p.samples[s] = 0;
			p.arrived[s] = 0;
		}
	}
}

}  // namespace rtlpower
