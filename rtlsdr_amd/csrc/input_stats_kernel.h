// input_stats_kernel.h — the ADC statistics rtlsdr_callback keeps on the raw bytes of every buffer
// (reference src/rtl_fm.c:1302-1324), before the byte-to-int16 conversion:
//
//   max        largest byte of the buffer                                        (:1305-1312)
//   step       2; while (len >= 16384 * step) step += 2;                         (:1314-1315)
//   pow_sum    sum over i = 0, step, 2 step, ... < len of (buf[i]-127)^2 + (buf[i+1]-127)^2   (:1316-1321)
//   pow_count  number of those i
//
// One record per (stream, buffer) of a run, overwritten by every launch (nothing accumulates on the device; the
// host-side monitor does the reference's accumulation over buffers, include/rtlfm_monitor.h).  All of it is
// integer and order-independent: the records are bit-identical to the reference whatever the reduction order.
//
// A pure reader: 16-byte loads, every byte of a buffer once, nothing beyond nblocks * block_len of a row.
//   squares  (int8)(b ^ 0x7f) == 127 - b for every byte, so four squares are one signed v_dot4 of the word
//            with itself (the compiler's builtin: it keeps the hazard distance).  The bytes `step` skips are
//            masked to zero first; the masks repeat every lcm(16, step) bytes = at most nine 16-byte units
//            and sit in LDS.  step == 2 (every buffer below 32 KiB) takes all bytes: no mask, no LDS read.
//   max      v_pk_max_u16 of the word as it is carries the odd bytes' maximum in the high byte of each half,
//            the same of the word shifted left by eight bits the even bytes'.
// pow_sum cannot wrap: pow_count <= 16384 and a term is at most 2 * 128^2.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/rtlfm_hip.h"

namespace rtlfm {
namespace istats {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef unsigned short us2 __attribute__((ext_vector_type(2)));

constexpr int kMaxPeriod = 9;  // lcm(16, step) / 16 for step = 2 ... 18 (block_len <= RTLFM_MAX_BLOCK_LEN)

// step and pow_count of a buffer of len bytes, as the callback computes them
inline void step_count(uint32_t len, int *step, int *count)
{
	int st = 2;
	while (len >= 16384u * (uint32_t)st) st += 2;
	*step = st;
	*count = (int)((len + (uint32_t)st - 1) / (uint32_t)st);
}

// 16-byte units after which the masks repeat
inline int mask_period(int step)
{
	int g = step, b = 16;
	while (b) { const int t = g % b; g = b; b = t; }
	return step / g;
}

struct Acc {
	int pow = 0;
	uint32_t mo = 0, me = 0;  // two u16 each: the high bytes are the running maxima of the odd / even bytes
};

__device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b)
{
	return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}

template <bool MASKED>
__device__ __forceinline__ void add_word(Acc &a, uint32_t w, uint32_t m)
{
	a.mo = pk_max(a.mo, w);
	a.me = pk_max(a.me, w << 8);
	uint32_t x = w ^ 0x7f7f7f7fu;
	if (MASKED) x &= m;
	a.pow = __builtin_amdgcn_sdot4((int)x, (int)x, a.pow, false);
}

template <bool MASKED>
__device__ __forceinline__ void add16(Acc &a, const v4u &v, const uint4 &m)
{
	add_word<MASKED>(a, v.x, m.x);
	add_word<MASKED>(a, v.y, m.y);
	add_word<MASKED>(a, v.z, m.z);
	add_word<MASKED>(a, v.w, m.w);
}

template <bool NT>
__device__ __forceinline__ v4u load16(const v4u *p)
{
	return NT ? __builtin_nontemporal_load(p) : *p;
}

// mtab[e] = which bytes of the 16-byte unit e (mod period) of a buffer the strided sum takes: the pair at buffer
// offset p (even) counts when p % step == 0
__device__ __forceinline__ void fill_masks(uint4 *mtab, int step, int period, int tid)
{
	if (tid < period) {
		uint32_t m[4];
		for (int w = 0; w < 4; w++) {
			const int p = tid * 16 + w * 4;
			m[w] = (p % step == 0 ? 0x0000ffffu : 0u) | ((p + 2) % step == 0 ? 0xffff0000u : 0u);
		}
		mtab[tid] = make_uint4(m[0], m[1], m[2], m[3]);
	}
}

__device__ __forceinline__ void wave_reduce(int &pow, uint32_t &mx)
{
	for (int off = 32; off > 0; off >>= 1) {
		pow += __shfl_down(pow, off, 64);
		const uint32_t o = (uint32_t)__shfl_down((int)mx, off, 64);
		mx = o > mx ? o : mx;
	}
}

__device__ __forceinline__ uint32_t acc_max(const Acc &a)
{
	const uint32_t t = pk_max(a.mo, a.me);  // high byte of each half: odd and even bytes together
	const uint32_t hi = t >> 24, lo = (t >> 8) & 0xffu;
	return hi > lo ? hi : lo;
}

__device__ __forceinline__ void put_record(rtlfm_input_stat *out, uint32_t pow, int count, uint32_t mx, int step)
{
	*reinterpret_cast<uint4 *>(out) = make_uint4(pow, (uint32_t)count, mx, (uint32_t)step);  // one 16-byte vector store
}

// Buffers of at least 8 KiB: one workgroup per (stream, buffer), eight 16-byte loads of a lane in flight.
// rec_stride = records per stream in `out` (the run's nblocks; a ragged run files single buffers into longer rows).
template <bool MASKED, bool NT>
__global__ void __launch_bounds__(256)
k_input_stats(const uint8_t *__restrict__ iq, size_t stream_stride, uint32_t L, int nblocks, int step, int count, int period,
              rtlfm_input_stat *__restrict__ out, int rec_stride)
{
	__shared__ uint4 mtab[kMaxPeriod];
	__shared__ uint32_t red[2][4];
	// (stream, buffer) folded into grid.x: grid.y stops at 65535 streams
	const size_t s = blockIdx.x / (unsigned)nblocks;
	const int b = (int)(blockIdx.x % (unsigned)nblocks);
	const v4u *src4 = reinterpret_cast<const v4u *>(iq + s * stream_stride + (size_t)b * L);
	const uint32_t n16 = L / 16;  // L is a multiple of 512
	uint32_t e = 0, de = 0;
	if (MASKED) {
		fill_masks(mtab, step, period, (int)threadIdx.x);
		__syncthreads();
		e = threadIdx.x % (unsigned)period;
		de = 256u % (unsigned)period;
	}
	Acc a;
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
#pragma unroll
		for (int j = 0; j < 8; j++) v[j] = load16<NT>(src4 + k + 256 * j);
#pragma unroll
		for (int j = 0; j < 8; j++) add16<MASKED>(a, v[j], MASKED ? next_mask() : none);
	}
	for (; k < n16; k += 256) {
		const v4u v = load16<NT>(src4 + k);
		add16<MASKED>(a, v, MASKED ? next_mask() : none);
	}
	int pow = a.pow;
	uint32_t mx = acc_max(a);
	wave_reduce(pow, mx);
	const int w = threadIdx.x >> 6;
	if ((threadIdx.x & 63) == 0) { red[0][w] = (uint32_t)pow; red[1][w] = mx; }
	__syncthreads();
	if (threadIdx.x == 0) {
		const uint32_t m01 = red[1][0] > red[1][1] ? red[1][0] : red[1][1];
		const uint32_t m23 = red[1][2] > red[1][3] ? red[1][2] : red[1][3];
		put_record(out + s * (size_t)rec_stride + b, red[0][0] + red[0][1] + red[0][2] + red[0][3], count, m01 > m23 ? m01 : m23, step);
	}
}

// Shorter buffers (512 ... 7680 bytes, always step 2): a WAVE per (stream, buffer), four to a workgroup, no barrier
// (as k_rdc_sums_small: a workgroup per 512-byte buffer is launch overhead and nothing else).
template <bool NT>
__global__ void __launch_bounds__(256)
k_input_stats_small(const uint8_t *__restrict__ iq, size_t stream_stride, uint32_t L, int nblocks, size_t total, int step, int count,
                    rtlfm_input_stat *__restrict__ out, int rec_stride)
{
	const size_t sb = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (sb >= total) return;
	const int lane = threadIdx.x & 63;
	const size_t s = sb / (unsigned)nblocks;
	const int b = (int)(sb % (unsigned)nblocks);
	const v4u *src4 = reinterpret_cast<const v4u *>(iq + s * stream_stride + (size_t)b * L);
	const uint32_t n16 = L / 16;
	Acc a;
	const uint4 none = make_uint4(0, 0, 0, 0);
	for (uint32_t k = lane; k < n16; k += 64) {
		const v4u v = load16<NT>(src4 + k);
		add16<false>(a, v, none);
	}
	int pow = a.pow;
	uint32_t mx = acc_max(a);
	wave_reduce(pow, mx);
	if (lane == 0) put_record(out + s * (size_t)rec_stride + b, (uint32_t)pow, count, mx, step);
}

// Queues the statistics of S streams x nblocks buffers of L bytes on q.  Returns 0 or -EINVAL.
inline int launch(const uint8_t *d_iq, size_t stream_stride, uint32_t L, int nblocks, int S, rtlfm_input_stat *out, int rec_stride,
                  bool nontemporal, hipStream_t q)
{
	if (!d_iq || !out || S < 1 || nblocks < 1 || L < 512 || (L & 511) || L > RTLFM_MAX_BLOCK_LEN) return -EINVAL;
	if (((uintptr_t)d_iq & 15) || (stream_stride & 15) || stream_stride < (size_t)nblocks * L) return -EINVAL;
	int step, count;
	step_count(L, &step, &count);
	const int period = mask_period(step);
	if (period > kMaxPeriod) return -EINVAL;
	const size_t total = (size_t)S * nblocks;
	if (L < 8192) {
		const unsigned grid = (unsigned)((total + 3) / 4);
		if (nontemporal) k_input_stats_small<true><<<grid, 256, 0, q>>>(d_iq, stream_stride, L, nblocks, total, step, count, out, rec_stride);
		else k_input_stats_small<false><<<grid, 256, 0, q>>>(d_iq, stream_stride, L, nblocks, total, step, count, out, rec_stride);
		return 0;
	}
	const unsigned grid = (unsigned)total;
#define RTLFM_ISTATS_GO(M, N) k_input_stats<M, N><<<grid, 256, 0, q>>>(d_iq, stream_stride, L, nblocks, step, count, period, out, rec_stride)
	if (step == 2) { if (nontemporal) RTLFM_ISTATS_GO(false, true); else RTLFM_ISTATS_GO(false, false); }
	else { if (nontemporal) RTLFM_ISTATS_GO(true, true); else RTLFM_ISTATS_GO(true, false); }
#undef RTLFM_ISTATS_GO
	return 0;
}

}  // namespace istats
}  // namespace rtlfm
