// source_prepass_kernel.h — everything a channel run wants to know about its SOURCE rows before the front end touches them,
// from one read of the bytes: option source_dc's buffer sums (what k_rdc_sums_wide / _small leave in d_sdc_sums), option
// source_health's records (input_health_kernel.h) and option source_stats' records (input_stats_kernel.h).
//
// With source_dc on, the sums alone already cost a read of every source row; the readers behind them would cost a second.
// At many sources x few channels the front end is bound by the source bytes and that second read is a large share of the
// step: here the words a lane holds for the sums also go through ihealth::add16 and istats::add16.  (With source_dc off
// there is nothing to share a read with: ihealth::launch / istats::launch run over the source rows as they are, and no
// instance of this kernel exists for that case - hence no DC switch among the template parameters.)
//
// Nothing here is a new definition.  Per 16-byte unit:
//   sums     v_dot4_u32_u8 against (1, 0, 1, 0) / (0, 1, 0, 1), the -127 per sample taken off at the end (k_rdc_sums_wide)
//   health   ihealth::add16 with the byte to the unit's left (a one-byte load of the line already in flight)
//   stats    istats::add16, masked from 32 KiB on (step >= 4)
// The dots are the compiler's builtins, which keep the hazard distance (tests/test_isa_lint.py reads this unit too).
// All of it is integer and order-independent: the records and the sums are bit-identical to the separate kernels'.
//
// Geometry and loads are k_input_health's: a workgroup per (source, buffer) from 8 KiB up, eight 16-byte loads of a lane
// in flight; a wave per (source, buffer), four to a workgroup, below.  Lanes reduce by shuffles, waves through LDS; no
// atomics; thread 0 (lane 0) stores every result with ordinary vector stores.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/rtlfm_hip.h"
#include "input_health_kernel.h"
#include "input_stats_kernel.h"

namespace rtlfm {
namespace sprepass {

using istats::v4u;

struct Sums {
	unsigned si = 0, sq = 0;  // u8 sums: <= 262144 * 255 / 2 each
};

__device__ __forceinline__ void add16(Sums &d, const v4u &v)
{
	d.si = __builtin_amdgcn_udot4(v.x, 0x00010001u, d.si, false); d.sq = __builtin_amdgcn_udot4(v.x, 0x01000100u, d.sq, false);
	d.si = __builtin_amdgcn_udot4(v.y, 0x00010001u, d.si, false); d.sq = __builtin_amdgcn_udot4(v.y, 0x01000100u, d.sq, false);
	d.si = __builtin_amdgcn_udot4(v.z, 0x00010001u, d.si, false); d.sq = __builtin_amdgcn_udot4(v.z, 0x01000100u, d.sq, false);
	d.si = __builtin_amdgcn_udot4(v.w, 0x00010001u, d.si, false); d.sq = __builtin_amdgcn_udot4(v.w, 0x01000100u, d.sq, false);
}

__device__ __forceinline__ void wave_reduce2(unsigned &x, unsigned &y)
{
	for (int off = 32; off > 0; off >>= 1) {
		x += (unsigned)__shfl_down((int)x, off, 64);
		y += (unsigned)__shfl_down((int)y, off, 64);
	}
}

__device__ __forceinline__ void put_sums(long long *sums, uint32_t L, unsigned si, unsigned sq)
{
	const long long pairs = L / 2;
	sums[0] = (long long)si - 127 * pairs;
	sums[1] = (long long)sq - 127 * pairs;
}

// What one lane accumulates, and the one place a unit enters all three
template <bool HEALTH, bool STATS, bool MASKED>
struct Lane {
	Sums d;
	ihealth::Acc a;
	istats::Acc sa;
	// e_left: ihealth::add16's (unused without HEALTH); m: the unit's mask (unused unless MASKED)
	__device__ __forceinline__ void add(const v4u &v, uint32_t e_left, const uint4 &m)
	{
		add16(d, v);
		if (HEALTH) ihealth::add16(a, v, e_left);
		if (STATS) istats::add16<MASKED>(sa, v, m);
	}
};

// One (source, buffer) by a workgroup of 256: the loop of k_input_health over Lane::add, then the reductions.
template <bool HEALTH, bool STATS, bool MASKED, bool NT>
__device__ __forceinline__ void wide_body(const uint8_t *__restrict__ src, uint32_t L, int step, int count, int period, uint4 *mtab,
                                          uint32_t (*red)[4], long long *__restrict__ sums, rtlfm_input_health *__restrict__ hout,
                                          rtlfm_input_stat *__restrict__ sout)
{
	const v4u *src4 = reinterpret_cast<const v4u *>(src);
	const uint32_t n16 = L / 16;  // L is a multiple of 512
	uint32_t e = 0, de = 0;
	if (STATS && MASKED) {
		istats::fill_masks(mtab, step, period, (int)threadIdx.x);
		__syncthreads();
		e = threadIdx.x % (unsigned)period;
		de = 256u % (unsigned)period;
	}
	Lane<HEALTH, STATS, MASKED> ln;
	const uint4 none = make_uint4(0, 0, 0, 0);
	auto next_mask = [&]() {
		const uint4 m = mtab[e];
		e += de;
		if (e >= (unsigned)period) e -= (unsigned)period;
		return m;
	};
	uint32_t k = threadIdx.x;
	for (; k + 7 * 256 < n16; k += 8 * 256) {
		v4u v[8];
		uint32_t lf[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
		for (int j = 0; j < 8; j++) v[j] = istats::load16<NT>(src4 + k + 256 * j);
		if (HEALTH) {
			lf[0] = src[(size_t)k * 16 - (k ? 1u : 0u)];
#pragma unroll
			for (int j = 1; j < 8; j++) lf[j] = src[(size_t)(k + 256 * j) * 16 - 1];
		}
#pragma unroll
		for (int j = 0; j < 8; j++) {
			const uint32_t el = (j == 0 && k == 0) ? lf[0] : ((lf[j] + 1u) & 0xffu);
			ln.add(v[j], el, (STATS && MASKED) ? next_mask() : none);
		}
	}
	for (; k < n16; k += 256) {
		const v4u v = istats::load16<NT>(src4 + k);
		uint32_t lf = 0;
		if (HEALTH) lf = src[(size_t)k * 16 - (k ? 1u : 0u)];
		ln.add(v, k == 0 ? lf : ((lf + 1u) & 0xffu), (STATS && MASKED) ? next_mask() : none);
	}
	uint32_t ends = 0;
	if (HEALTH && threadIdx.x == 0) ends = (uint32_t)src[0] | (uint32_t)src[L - 1] << 8;
	wave_reduce2(ln.d.si, ln.d.sq);
	if (HEALTH) ihealth::wave_reduce3(ln.a.lost, ln.a.nhigh, ln.a.nover);
	int pow = ln.sa.pow;
	uint32_t mx = 0;
	if (STATS) {
		mx = istats::acc_max(ln.sa);
		istats::wave_reduce(pow, mx);
	}
	const int w = threadIdx.x >> 6;
	if ((threadIdx.x & 63) == 0) {
		red[0][w] = ln.d.si; red[1][w] = ln.d.sq;
		if (HEALTH) { red[2][w] = ln.a.lost; red[3][w] = ln.a.nhigh; red[4][w] = ln.a.nover; }
		if (STATS) { red[5][w] = (uint32_t)pow; red[6][w] = mx; }
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		auto sum4 = [&](int r) { return red[r][0] + red[r][1] + red[r][2] + red[r][3]; };
		put_sums(sums, L, sum4(0), sum4(1));
		if (HEALTH) ihealth::put_record(hout, L, sum4(2), sum4(3), sum4(4), ends, ends >> 8);
		if (STATS) {
			const uint32_t m01 = red[6][0] > red[6][1] ? red[6][0] : red[6][1];
			const uint32_t m23 = red[6][2] > red[6][3] ? red[6][2] : red[6][3];
			istats::put_record(sout, sum4(5), count, m01 > m23 ? m01 : m23, step);
		}
	}
}

// Buffers of at least 8 KiB.  sums: [source][nblocks][2], as k_rdc_sums_wide's; the records of buffer b of source s at
// [s * rec_stride + b] of hout / sout (a ring run of short buffers files single buffers into longer rows).  `period` > 1
// - the statistics skip bytes, step >= 4 - is the same for the whole launch: the branch is uniform.
template <bool HEALTH, bool STATS, bool NT>
__global__ void __launch_bounds__(256)
k_source_prepass(const uint8_t *__restrict__ iq, size_t src_stride, uint32_t L, int nblocks, long long *__restrict__ sums,
                 rtlfm_input_health *__restrict__ hout, rtlfm_input_stat *__restrict__ sout, int rec_stride, int step, int count, int period)
{
	__shared__ uint4 mtab[istats::kMaxPeriod];
	__shared__ uint32_t red[7][4];
	// (source, buffer) folded into grid.x: grid.y stops at 65535
	const size_t s = blockIdx.x / (unsigned)nblocks;
	const int b = (int)(blockIdx.x % (unsigned)nblocks);
	const uint8_t *src = iq + s * src_stride + (size_t)b * L;
	long long *su = sums + (s * (size_t)nblocks + b) * 2;
	rtlfm_input_health *ho = HEALTH ? hout + s * (size_t)rec_stride + b : nullptr;
	rtlfm_input_stat *so = STATS ? sout + s * (size_t)rec_stride + b : nullptr;
	if (STATS && step != 2)
		wide_body<HEALTH, STATS, true, NT>(src, L, step, count, period, mtab, red, su, ho, so);
	else
		wide_body<HEALTH, STATS, false, NT>(src, L, step, count, period, mtab, red, su, ho, so);
}

// Shorter buffers (512 ... 7680 bytes, always step 2): a wave per (source, buffer), four to a workgroup, no barrier.
template <bool HEALTH, bool STATS, bool NT>
__global__ void __launch_bounds__(256)
k_source_prepass_small(const uint8_t *__restrict__ iq, size_t src_stride, uint32_t L, int nblocks, size_t total,
                       long long *__restrict__ sums, rtlfm_input_health *__restrict__ hout, rtlfm_input_stat *__restrict__ sout,
                       int rec_stride, int step, int count)
{
	const size_t sb = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (sb >= total) return;
	const uint32_t lane = threadIdx.x & 63;
	const size_t s = sb / (unsigned)nblocks;
	const int b = (int)(sb % (unsigned)nblocks);
	const uint8_t *src = iq + s * src_stride + (size_t)b * L;
	const v4u *src4 = reinterpret_cast<const v4u *>(src);
	const uint32_t n16 = L / 16;
	Lane<HEALTH, STATS, false> ln;
	const uint4 none = make_uint4(0, 0, 0, 0);
	for (uint32_t k = lane; k < n16; k += 64) {
		const v4u v = istats::load16<NT>(src4 + k);
		uint32_t lf = 0;
		if (HEALTH) lf = src[(size_t)k * 16 - (k ? 1u : 0u)];
		ln.add(v, k == 0 ? lf : ((lf + 1u) & 0xffu), none);
	}
	uint32_t ends = 0;
	if (HEALTH && lane == 0) ends = (uint32_t)src[0] | (uint32_t)src[L - 1] << 8;
	wave_reduce2(ln.d.si, ln.d.sq);
	if (HEALTH) ihealth::wave_reduce3(ln.a.lost, ln.a.nhigh, ln.a.nover);
	int pow = ln.sa.pow;
	uint32_t mx = 0;
	if (STATS) {
		mx = istats::acc_max(ln.sa);
		istats::wave_reduce(pow, mx);
	}
	if (lane == 0) {
		put_sums(sums + sb * 2, L, ln.d.si, ln.d.sq);
		if (HEALTH) ihealth::put_record(hout + s * (size_t)rec_stride + b, L, ln.a.lost, ln.a.nhigh, ln.a.nover, ends, ends >> 8);
		if (STATS) istats::put_record(sout + s * (size_t)rec_stride + b, (uint32_t)pow, count, mx, step);
	}
}

// Queues the pre-pass of S sources x nblocks buffers of L bytes on q: the sums into `sums`, and the records of whichever of
// hout / sout is given (at least one: the sums alone are k_rdc_sums_wide's business).  Returns 0 or -EINVAL.
inline int launch(const uint8_t *d_iq, size_t src_stride, uint32_t L, int nblocks, int S, long long *sums, rtlfm_input_health *hout,
                  rtlfm_input_stat *sout, int rec_stride, bool nontemporal, hipStream_t q)
{
	if (!d_iq || !sums || (!hout && !sout) || S < 1 || nblocks < 1 || L < 512 || (L & 511) || L > RTLFM_MAX_BLOCK_LEN) return -EINVAL;
	if (((uintptr_t)d_iq & 15) || (src_stride & 15) || src_stride < (size_t)nblocks * L || rec_stride < nblocks) return -EINVAL;
	int step, count;
	istats::step_count(L, &step, &count);
	const int period = istats::mask_period(step);
	if (period > istats::kMaxPeriod) return -EINVAL;
	const size_t total = (size_t)S * nblocks;
	if (total > 0x7fffffffu) return -EINVAL;
	const bool small = L < 8192;
	const unsigned grid = small ? (unsigned)((total + 3) / 4) : (unsigned)total;
#define RTLFM_SPREPASS_GO(H, ST, N) \
	do { \
		if (small) k_source_prepass_small<H, ST, N><<<grid, 256, 0, q>>>(d_iq, src_stride, L, nblocks, total, sums, hout, sout, rec_stride, step, count); \
		else k_source_prepass<H, ST, N><<<grid, 256, 0, q>>>(d_iq, src_stride, L, nblocks, sums, hout, sout, rec_stride, step, count, period); \
	} while (0)
	if (hout && sout) { if (nontemporal) RTLFM_SPREPASS_GO(true, true, true); else RTLFM_SPREPASS_GO(true, true, false); }
	else if (hout) { if (nontemporal) RTLFM_SPREPASS_GO(true, false, true); else RTLFM_SPREPASS_GO(true, false, false); }
	else { if (nontemporal) RTLFM_SPREPASS_GO(false, true, true); else RTLFM_SPREPASS_GO(false, true, false); }
#undef RTLFM_SPREPASS_GO
	return 0;
}

}  // namespace sprepass
}  // namespace rtlfm
