// input_health_kernel.h — the three passes the reference makes over the raw bytes of every transfer besides the
// callback's statistics (input_stats_kernel.h), as one reader:
//
//   overload   bytes equal to 0 or 255        softagc()'s `overload` (src/librtlsdr.c:3288-3327) and
//                                             detect_overload()'s overload_count (src/rtl_tcp.c:235-244)
//   high       bytes < 64 or > 191            softagc()'s high_level
//   lost       what underrun_test() (src/rtl_test.c:121-151) adds to `lost` at positions i = 1 .. len-1 of the buffer:
//              after any iteration bcnt == (uint8_t)(buf[i] + 1) whether or not the bytes matched, so the term at i is
//              |buf[i] - e| with e = (uint8_t)(buf[i-1] + 1), on ints in 0 .. 255 (255 -> 0 is continuity, not a loss)
//   first,last buf[0], buf[len-1]: the term at i = 0 needs the previous buffer's last byte and is the host engine's
//              (include/rtlfm_agc.h), which leaves this kernel without carried state or order between workgroups
//
// One 16-byte record per (stream, buffer) of a run, overwritten by every launch.  Integer and order-independent:
// bit-identical to the reference whatever the reduction order.  No count can wrap: lost <= 255 * 262143, the counts
// <= 262144 = RTLFM_MAX_BLOCK_LEN.
//
// Geometry and loads are k_input_stats's.  Per 32-bit word w of four bytes (M7 = 0x7f7f7f7f, M8 = 0x80808080):
//   a = w & M7; E = (a + 0x01010101) ^ (w & M8)     every byte + 1 mod 256, no carry between bytes
//   lost      v_sad_u8(w, (E << 8) | top byte of the E of the word to the left): four |buf[i] - e| into the accumulator.
//             The byte to the left of a lane's 16-byte unit is another lane's: a one-byte load at offset -1 of the
//             unit's own address (an immediate offset of the same address registers, the line already in flight for the
//             neighbour's load) - no VALU; a DPP wave shift costs a v_mov per unit AND the same load for lane 0.
//   high      b + 64 mod 256 has its top bit clear exactly for b < 64 || b > 191: ((a + 0x40404040) ^ w) & M8 has a bit per
//             byte that is NOT high; popcounts accumulate, high = len - sum
//   overload  E & 0xfe == 0 exactly for b = 0, 255: ((E & 0x7e7e7e7e) + M7) | E | M7 is all ones but the top bit of the
//             bytes that overload (the exact zero-byte mask, inverted); popcounts accumulate, overload = 8 len - sum
//
// STATS: the same launch also writes k_input_stats's records (istats::add16 on the words it holds anyway), for a handle
// with both options on: the input is read once.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/rtlfm_hip.h"
#include "input_stats_kernel.h"

namespace rtlfm {
namespace ihealth {

using istats::v4u;

struct Acc {
	uint32_t lost = 0, nhigh = 0, nover = 0;  // nhigh / nover count the bytes that are NOT high / do NOT overload
};

// w: four bytes; pred_low: what underrun_test expects in w's lowest byte (0 .. 255).  Returns E of w.
__device__ __forceinline__ uint32_t add_word(Acc &a, uint32_t w, uint32_t pred_low)
{
	const uint32_t l7 = w & 0x7f7f7f7fu;
	const uint32_t E = (l7 + 0x01010101u) ^ (w & 0x80808080u);
	a.lost = __builtin_amdgcn_sad_u8(w, (E << 8) | pred_low, a.lost);
	a.nhigh += (uint32_t)__popc(((l7 + 0x40404040u) ^ w) & 0x80808080u);
	a.nover += (uint32_t)__popc(((E & 0x7e7e7e7eu) + 0x7f7f7f7fu) | E | 0x7f7f7f7fu);
	return E;
}

// e_left: what underrun_test expects in the unit's first byte ((uint8_t)(byte to its left + 1); the first byte itself
// at the head of a buffer, whose term is the engine's)
__device__ __forceinline__ void add16(Acc &a, const v4u &v, uint32_t e_left)
{
	uint32_t E = add_word(a, v.x, e_left);
	E = add_word(a, v.y, E >> 24);
	E = add_word(a, v.z, E >> 24);
	add_word(a, v.w, E >> 24);
}

__device__ __forceinline__ void wave_reduce3(uint32_t &x, uint32_t &y, uint32_t &z)
{
	for (int off = 32; off > 0; off >>= 1) {
		x += (uint32_t)__shfl_down((int)x, off, 64);
		y += (uint32_t)__shfl_down((int)y, off, 64);
		z += (uint32_t)__shfl_down((int)z, off, 64);
	}
}

__device__ __forceinline__ void put_record(rtlfm_input_health *out, uint32_t L, uint32_t lost, uint32_t nhigh, uint32_t nover,
                                           uint32_t first, uint32_t last)
{
	// one 16-byte vector store; pad_ = 0
	*reinterpret_cast<uint4 *>(out) = make_uint4(8u * L - nover, L - nhigh, lost, (first & 0xffu) | (last & 0xffu) << 8);
}

// Buffers of at least 8 KiB: one workgroup per (stream, buffer), eight 16-byte loads of a lane in flight.
template <bool STATS, bool MASKED, bool NT>
__global__ void __launch_bounds__(256)
k_input_health(const uint8_t *__restrict__ iq, size_t stream_stride, uint32_t L, int nblocks, rtlfm_input_health *__restrict__ out,
               int rec_stride, int step, int count, int period, rtlfm_input_stat *__restrict__ sout)
{
	__shared__ uint4 mtab[istats::kMaxPeriod];
	__shared__ uint32_t red[5][4];
	const size_t s = blockIdx.x / (unsigned)nblocks;
	const int b = (int)(blockIdx.x % (unsigned)nblocks);
	const uint8_t *src = iq + s * stream_stride + (size_t)b * L;
	const v4u *src4 = reinterpret_cast<const v4u *>(src);
	const uint32_t n16 = L / 16;  // L is a multiple of 512
	uint32_t e = 0, de = 0;
	if (STATS && MASKED) {
		istats::fill_masks(mtab, step, period, (int)threadIdx.x);
		__syncthreads();
		e = threadIdx.x % (unsigned)period;
		de = 256u % (unsigned)period;
	}
	Acc a;
	istats::Acc sa;
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
		uint32_t lf[8];
#pragma unroll
		for (int j = 0; j < 8; j++) v[j] = istats::load16<NT>(src4 + k + 256 * j);
		lf[0] = src[(size_t)k * 16 - (k ? 1u : 0u)];
#pragma unroll
		for (int j = 1; j < 8; j++) lf[j] = src[(size_t)(k + 256 * j) * 16 - 1];
#pragma unroll
		for (int j = 0; j < 8; j++) {
			const uint32_t el = (j == 0 && k == 0) ? lf[0] : ((lf[j] + 1u) & 0xffu);
			add16(a, v[j], el);
			if (STATS) istats::add16<MASKED>(sa, v[j], MASKED ? next_mask() : none);
		}
	}
	for (; k < n16; k += 256) {
		const v4u v = istats::load16<NT>(src4 + k);
		const uint32_t lf = src[(size_t)k * 16 - (k ? 1u : 0u)];
		add16(a, v, k == 0 ? lf : ((lf + 1u) & 0xffu));
		if (STATS) istats::add16<MASKED>(sa, v, MASKED ? next_mask() : none);
	}
	uint32_t ends = 0;
	if (threadIdx.x == 0) ends = (uint32_t)src[0] | (uint32_t)src[L - 1] << 8;
	wave_reduce3(a.lost, a.nhigh, a.nover);
	int pow = sa.pow;
	uint32_t mx = 0;
	if (STATS) {
		mx = istats::acc_max(sa);
		istats::wave_reduce(pow, mx);
	}
	const int w = threadIdx.x >> 6;
	if ((threadIdx.x & 63) == 0) {
		red[0][w] = a.lost; red[1][w] = a.nhigh; red[2][w] = a.nover;
		if (STATS) { red[3][w] = (uint32_t)pow; red[4][w] = mx; }
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		put_record(out + s * (size_t)rec_stride + b, L, red[0][0] + red[0][1] + red[0][2] + red[0][3],
		           red[1][0] + red[1][1] + red[1][2] + red[1][3], red[2][0] + red[2][1] + red[2][2] + red[2][3], ends, ends >> 8);
		if (STATS) {
			const uint32_t m01 = red[4][0] > red[4][1] ? red[4][0] : red[4][1];
			const uint32_t m23 = red[4][2] > red[4][3] ? red[4][2] : red[4][3];
			istats::put_record(sout + s * (size_t)rec_stride + b, red[3][0] + red[3][1] + red[3][2] + red[3][3], count,
			                   m01 > m23 ? m01 : m23, step);
		}
	}
}

// Shorter buffers (512 ... 7680 bytes, always step 2): a wave per (stream, buffer), four to a workgroup, no barrier.
template <bool STATS, bool NT>
__global__ void __launch_bounds__(256)
k_input_health_small(const uint8_t *__restrict__ iq, size_t stream_stride, uint32_t L, int nblocks, size_t total,
                     rtlfm_input_health *__restrict__ out, int rec_stride, int step, int count, rtlfm_input_stat *__restrict__ sout)
{
	const size_t sb = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (sb >= total) return;
	const uint32_t lane = threadIdx.x & 63;
	const size_t s = sb / (unsigned)nblocks;
	const int b = (int)(sb % (unsigned)nblocks);
	const uint8_t *src = iq + s * stream_stride + (size_t)b * L;
	const v4u *src4 = reinterpret_cast<const v4u *>(src);
	const uint32_t n16 = L / 16;
	Acc a;
	istats::Acc sa;
	const uint4 none = make_uint4(0, 0, 0, 0);
	for (uint32_t k = lane; k < n16; k += 64) {
		const v4u v = istats::load16<NT>(src4 + k);
		const uint32_t lf = src[(size_t)k * 16 - (k ? 1u : 0u)];
		add16(a, v, k == 0 ? lf : ((lf + 1u) & 0xffu));
		if (STATS) istats::add16<false>(sa, v, none);
	}
	uint32_t ends = 0;
	if (lane == 0) ends = (uint32_t)src[0] | (uint32_t)src[L - 1] << 8;
	wave_reduce3(a.lost, a.nhigh, a.nover);
	int pow = sa.pow;
	uint32_t mx = 0;
	if (STATS) {
		mx = istats::acc_max(sa);
		istats::wave_reduce(pow, mx);
	}
	if (lane == 0) {
		put_record(out + s * (size_t)rec_stride + b, L, a.lost, a.nhigh, a.nover, ends, ends >> 8);
		if (STATS) istats::put_record(sout + s * (size_t)rec_stride + b, (uint32_t)pow, count, mx, step);
	}
}

// Queues the health records of S streams x nblocks buffers of L bytes on q; with `sout` the same launch also writes
// the statistics istats::launch would (records filed alike, rec_stride per stream).  Returns 0 or -EINVAL.
inline int launch(const uint8_t *d_iq, size_t stream_stride, uint32_t L, int nblocks, int S, rtlfm_input_health *out, int rec_stride,
                  bool nontemporal, hipStream_t q, rtlfm_input_stat *sout = nullptr)
{
	if (!d_iq || !out || S < 1 || nblocks < 1 || L < 512 || (L & 511) || L > RTLFM_MAX_BLOCK_LEN) return -EINVAL;
	if (((uintptr_t)d_iq & 15) || (stream_stride & 15) || stream_stride < (size_t)nblocks * L) return -EINVAL;
	int step, count;
	istats::step_count(L, &step, &count);
	const int period = istats::mask_period(step);
	if (period > istats::kMaxPeriod) return -EINVAL;
	const size_t total = (size_t)S * nblocks;
	if (L < 8192) {
		const unsigned grid = (unsigned)((total + 3) / 4);
#define RTLFM_IHEALTH_GO(ST, N) k_input_health_small<ST, N><<<grid, 256, 0, q>>>(d_iq, stream_stride, L, nblocks, total, out, rec_stride, step, count, sout)
		if (sout) { if (nontemporal) RTLFM_IHEALTH_GO(true, true); else RTLFM_IHEALTH_GO(true, false); }
		else { if (nontemporal) RTLFM_IHEALTH_GO(false, true); else RTLFM_IHEALTH_GO(false, false); }
#undef RTLFM_IHEALTH_GO
		return 0;
	}
	const unsigned grid = (unsigned)total;
#define RTLFM_IHEALTH_GO(ST, M, N) k_input_health<ST, M, N><<<grid, 256, 0, q>>>(d_iq, stream_stride, L, nblocks, out, rec_stride, step, count, period, sout)
	if (!sout) { if (nontemporal) RTLFM_IHEALTH_GO(false, false, true); else RTLFM_IHEALTH_GO(false, false, false); }
	else if (step == 2) { if (nontemporal) RTLFM_IHEALTH_GO(true, false, true); else RTLFM_IHEALTH_GO(true, false, false); }
	else { if (nontemporal) RTLFM_IHEALTH_GO(true, true, true); else RTLFM_IHEALTH_GO(true, true, false); }
#undef RTLFM_IHEALTH_GO
	return 0;
}

}  // namespace ihealth
}  // namespace rtlfm
