// source_iq_kernel.h — option source_iq: one read of every SOURCE row of a channel run and one write.  What rtl_tcp -c
// (iqBalance, reference src/rtl_tcp.c:211-233) does to its uint8 buffer in one sequential float loop is split here into an
// exact measurement and an exact correction; the policy between them is host code (include/rtlfm_iq.h, csrc/iq.cpp).
//
//   record   per (source, buffer), over the RAW bytes I, Q in [0, 255]: n = L / 2, si = sum I, sq = sum Q, sii = sum I^2,
//            sqq = sum Q^2, siq = sum I Q, and `clipped`, the output BYTES the clamp below changed (rtlfm_iq_sums).
//   rows     with x = I - 127, y = Q - 127 and the source's four int16 Q14 coefficients (a, b, p, q):
//              I' = (a x + b y + 8192) >> 14,  Q' = (p x + q y + 8192) >> 14   (arithmetic shift; |a x + b y| < 2^24)
//            each output byte clamp(v + 127, 0, 255).  (16384, 0, 0, 16384) reproduces every byte.
//
// Per dword (two samples, I0 Q0 I1 Q1): five v_dot4_u32_u8 for the moments - against (1, 0, 1, 0) / (0, 1, 0, 1) and
// against the word's own I bytes, Q bytes and Q bytes moved onto the I positions - and, per sample, v_dot2_i32_i16 of the
// packed (x, y) with (a, b) and with (p, q).  The dots are the compiler's builtins, which keep the hazard distance
// (tests/test_isa_lint.py reads this unit too).  All of it is integer: any order of summation leaves the same bits.
//
// How the grid is cut (k_input_stats' geometry): a workgroup of 256 per (source, buffer) from 8 KiB up, eight 16-byte loads
// of a lane in flight; a wave per (source, buffer), four to a workgroup, below.  A lane's partial sums are uint32 - at most
// 512 samples of a 262144-byte buffer, 512 * 255^2 < 2^25 - and so is a wave's (a quarter of the longest buffer:
// 32768 * 255^2 < 2^31); lanes reduce by shuffles, waves through LDS, and thread 0 adds the four waves in uint64 (sii
// passes 2^32 at 262144 bytes) and stores the record with ordinary vector stores.  No atomics, no float.
//
// Loads may be non-temporal (the raw rows are read again only by the record readers); the stores are plain: every front
// end reads the corrected rows at once.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/rtlfm_hip.h"
#include "input_stats_kernel.h"

namespace rtlfm {
namespace siq {

using istats::v4u;
typedef short s2 __attribute__((ext_vector_type(2)));

static_assert(sizeof(rtlfm_iq_sums) == 48, "rtlfm_iq_sums is three 16-byte stores");
static_assert(RTLFM_MAX_BLOCK_LEN <= 262144u, "a wave's uint32 partial sums are sized for 262144-byte buffers");

struct Acc {
	uint32_t si = 0, sq = 0, sii = 0, sqq = 0, siq = 0, clipped = 0;
};

__device__ __forceinline__ uint32_t clamp_byte(int v, uint32_t &clipped)
{
	const int c = v < 0 ? 0 : v > 255 ? 255 : v;
	clipped += c != v ? 1u : 0u;
	return (uint32_t)c;
}

// one dword, I0 Q0 I1 Q1: the raw bytes' moments into a, the corrected dword back
__device__ __forceinline__ uint32_t word(Acc &a, uint32_t w, s2 ab, s2 pq)
{
	const uint32_t wi = w & 0x00ff00ffu, wq = w & 0xff00ff00u;
	a.si = __builtin_amdgcn_udot4(w, 0x00010001u, a.si, false);
	a.sq = __builtin_amdgcn_udot4(w, 0x01000100u, a.sq, false);
	a.sii = __builtin_amdgcn_udot4(w, wi, a.sii, false);
	a.sqq = __builtin_amdgcn_udot4(w, wq, a.sqq, false);
	a.siq = __builtin_amdgcn_udot4(w, wq >> 8, a.siq, false);
	const s2 k127 = {127, 127};
	const s2 xy0 = __builtin_bit_cast(s2, (w & 0xffu) | ((w << 8) & 0x00ff0000u)) - k127;
	const s2 xy1 = __builtin_bit_cast(s2, ((w >> 16) & 0xffu) | ((w >> 8) & 0x00ff0000u)) - k127;
	const int i0 = (__builtin_amdgcn_sdot2(xy0, ab, 8192, false) >> 14) + 127;
	const int q0 = (__builtin_amdgcn_sdot2(xy0, pq, 8192, false) >> 14) + 127;
	const int i1 = (__builtin_amdgcn_sdot2(xy1, ab, 8192, false) >> 14) + 127;
	const int q1 = (__builtin_amdgcn_sdot2(xy1, pq, 8192, false) >> 14) + 127;
	return clamp_byte(i0, a.clipped) | clamp_byte(q0, a.clipped) << 8 | clamp_byte(i1, a.clipped) << 16 | clamp_byte(q1, a.clipped) << 24;
}

__device__ __forceinline__ v4u unit(Acc &a, const v4u &v, s2 ab, s2 pq)
{
	v4u o;
	o.x = word(a, v.x, ab, pq);
	o.y = word(a, v.y, ab, pq);
	o.z = word(a, v.z, ab, pq);
	o.w = word(a, v.w, ab, pq);
	return o;
}

__device__ __forceinline__ void wave_reduce(Acc &a)
{
	for (int off = 32; off > 0; off >>= 1) {
		a.si += (uint32_t)__shfl_down((int)a.si, off, 64);
		a.sq += (uint32_t)__shfl_down((int)a.sq, off, 64);
		a.sii += (uint32_t)__shfl_down((int)a.sii, off, 64);
		a.sqq += (uint32_t)__shfl_down((int)a.sqq, off, 64);
		a.siq += (uint32_t)__shfl_down((int)a.siq, off, 64);
		a.clipped += (uint32_t)__shfl_down((int)a.clipped, off, 64);
	}
}

__device__ __forceinline__ void put_record(rtlfm_iq_sums *out, uint32_t L, uint32_t clipped, uint64_t si, uint64_t sq, uint64_t sii, uint64_t sqq,
                                           uint64_t siq)
{
	uint4 *o = reinterpret_cast<uint4 *>(out);  // (records are 48 bytes apart in a 256-byte aligned allocation)
	o[0] = make_uint4(L / 2, clipped, (uint32_t)si, (uint32_t)(si >> 32));
	o[1] = make_uint4((uint32_t)sq, (uint32_t)(sq >> 32), (uint32_t)sii, (uint32_t)(sii >> 32));
	o[2] = make_uint4((uint32_t)sqq, (uint32_t)(sqq >> 32), (uint32_t)siq, (uint32_t)(siq >> 32));
}

// the source's (a, b) and (p, q), each a packed pair of int16
__device__ __forceinline__ void load_coef(const int16_t *__restrict__ coef, size_t s, s2 &ab, s2 &pq)
{
	const uint2 c = *reinterpret_cast<const uint2 *>(coef + s * 4);
	ab = __builtin_bit_cast(s2, c.x);
	pq = __builtin_bit_cast(s2, c.y);
}

// Buffers of at least 8 KiB: one workgroup per (source, buffer).  Buffer b of source s is read at iq + s * src_stride + b * L
// and written at out + s * out_stride + b * L; its record goes to recs[s * rec_stride + b] (a ring run of short buffers
// files single buffers into longer rows).
template <bool NT>
__global__ void __launch_bounds__(256)
k_source_iq(const uint8_t *__restrict__ iq, size_t src_stride, uint32_t L, int nblocks, const int16_t *__restrict__ coef,
            uint8_t *__restrict__ out, size_t out_stride, rtlfm_iq_sums *__restrict__ recs, int rec_stride)
{
	__shared__ uint32_t red[6][4];
	// (source, buffer) folded into grid.x: grid.y stops at 65535
	const size_t s = blockIdx.x / (unsigned)nblocks;
	const int b = (int)(blockIdx.x % (unsigned)nblocks);
	const v4u *src4 = reinterpret_cast<const v4u *>(iq + s * src_stride + (size_t)b * L);
	v4u *dst4 = reinterpret_cast<v4u *>(out + s * out_stride + (size_t)b * L);
	const uint32_t n16 = L / 16;  // L is a multiple of 512
	s2 ab, pq;
	load_coef(coef, s, ab, pq);
	Acc a;
	uint32_t k = threadIdx.x;
	for (; k + 7 * 256 < n16; k += 8 * 256) {
		v4u v[8];
#pragma unroll
		for (int j = 0; j < 8; j++) v[j] = istats::load16<NT>(src4 + k + 256 * j);
#pragma unroll
		for (int j = 0; j < 8; j++) dst4[k + 256 * j] = unit(a, v[j], ab, pq);
	}
	for (; k < n16; k += 256) dst4[k] = unit(a, istats::load16<NT>(src4 + k), ab, pq);
	wave_reduce(a);
	const int w = threadIdx.x >> 6;
	if ((threadIdx.x & 63) == 0) {
		red[0][w] = a.si; red[1][w] = a.sq; red[2][w] = a.sii; red[3][w] = a.sqq; red[4][w] = a.siq; red[5][w] = a.clipped;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		auto sum4 = [&](int r) { return (uint64_t)red[r][0] + red[r][1] + red[r][2] + red[r][3]; };
		put_record(recs + s * (size_t)rec_stride + b, L, (uint32_t)sum4(5), sum4(0), sum4(1), sum4(2), sum4(3), sum4(4));
	}
}

// Shorter buffers (512 ... 7680 bytes): a wave per (source, buffer), four to a workgroup, no barrier.
template <bool NT>
__global__ void __launch_bounds__(256)
k_source_iq_small(const uint8_t *__restrict__ iq, size_t src_stride, uint32_t L, int nblocks, size_t total, const int16_t *__restrict__ coef,
                  uint8_t *__restrict__ out, size_t out_stride, rtlfm_iq_sums *__restrict__ recs, int rec_stride)
{
	const size_t sb = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (sb >= total) return;
	const uint32_t lane = threadIdx.x & 63;
	const size_t s = sb / (unsigned)nblocks;
	const int b = (int)(sb % (unsigned)nblocks);
	const v4u *src4 = reinterpret_cast<const v4u *>(iq + s * src_stride + (size_t)b * L);
	v4u *dst4 = reinterpret_cast<v4u *>(out + s * out_stride + (size_t)b * L);
	const uint32_t n16 = L / 16;
	s2 ab, pq;
	load_coef(coef, s, ab, pq);
	Acc a;
	for (uint32_t k = lane; k < n16; k += 64) dst4[k] = unit(a, istats::load16<NT>(src4 + k), ab, pq);
	wave_reduce(a);
	if (lane == 0) put_record(recs + s * (size_t)rec_stride + b, L, a.clipped, a.si, a.sq, a.sii, a.sqq, a.siq);
}

// Queues the pass over S sources x nblocks buffers of L bytes on q.  coef: [S][4] int16 on the device, 8-byte aligned;
// out rows hold nblocks * L bytes at least and start on 16-byte lines.  Returns 0 or -EINVAL.
inline int launch(const uint8_t *d_iq, size_t src_stride, uint32_t L, int nblocks, int S, const int16_t *coef, uint8_t *out, size_t out_stride,
                  rtlfm_iq_sums *recs, int rec_stride, bool nontemporal, hipStream_t q)
{
	if (!d_iq || !coef || !out || !recs || S < 1 || nblocks < 1 || L < 512 || (L & 511) || L > RTLFM_MAX_BLOCK_LEN) return -EINVAL;
	if (((uintptr_t)d_iq & 15) || (src_stride & 15) || src_stride < (size_t)nblocks * L || rec_stride < nblocks) return -EINVAL;
	if (((uintptr_t)out & 15) || (out_stride & 15) || out_stride < (size_t)nblocks * L || ((uintptr_t)coef & 7) || ((uintptr_t)recs & 15)) return -EINVAL;
	const size_t total = (size_t)S * nblocks;
	if (total > 0x7fffffffu) return -EINVAL;
	if (L < 8192) {
		const unsigned grid = (unsigned)((total + 3) / 4);
		if (nontemporal) k_source_iq_small<true><<<grid, 256, 0, q>>>(d_iq, src_stride, L, nblocks, total, coef, out, out_stride, recs, rec_stride);
		else k_source_iq_small<false><<<grid, 256, 0, q>>>(d_iq, src_stride, L, nblocks, total, coef, out, out_stride, recs, rec_stride);
		return 0;
	}
	if (nontemporal) k_source_iq<true><<<(unsigned)total, 256, 0, q>>>(d_iq, src_stride, L, nblocks, coef, out, out_stride, recs, rec_stride);
	else k_source_iq<false><<<(unsigned)total, 256, 0, q>>>(d_iq, src_stride, L, nblocks, coef, out, out_stride, recs, rec_stride);
	return 0;
}

}  // namespace siq
}  // namespace rtlfm
