// pack_kernel.h — the packed form of a run's results (option pack_results, rtlfm_gpu_fetch_packed, rtlfm_gpu_pack_device):
// every stream's row behind the other in ONE buffer, so that the copy back to the host moves what the streams hold and
// not max(lens) x nstreams.  Two launches, both read-only towards the run: they read the rows, the lengths, the levels and
// the state copy the run started from, and write only the packed buffer, its index, the total and (mode 2) a table of
// their own.
//
//   k_pack_plan   ONE workgroup.  Every stream's packed length - mode 1: lens[s]; mode 2: the extents of the buffers the
//                 demod thread's rule (scan::gate_step, src/rtl_fm.c:1366-1370 on :1206-1213) emits, walked from
//                 sin[s].squelch_hits with a LOCAL counter -, rounded up to 8 int16 so that every row starts on a 16-byte
//                 boundary, and the exclusive prefix sum over the streams: kPlanThreads streams at a time, a wave scan by
//                 lane shifts, the waves' totals through LDS, a carried total from chunk to chunk.  No atomics: the index
//                 is the same every time.
//   k_pack_copy   grid (piece, part): a piece is a stream's row (mode 1) or one emitted buffer's extent (mode 2).  The
//                 destination is 16-byte aligned at row starts only, the source at nothing but int16: a piece's elements in
//                 front of its first aligned destination vector and behind its last one go one by one; the vectors in
//                 between are whole 16-byte stores, each from the one or two ALIGNED 16-byte source vectors that hold its
//                 bytes, funnelled by the (piece-uniform, even) byte distance.  Both aligned vectors hold bytes of the
//                 piece, so no load touches a line the piece does not.  The elements behind a row's last sample up to the
//                 next multiple of 8 are written as 0, and nothing at or beyond `cap` is written.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/rtlfm_hip.h"
#include "staged_kernels.h"
#include "scan_kernel.h"

namespace rtlfm {
namespace pack {

constexpr int kPlanThreads = 1024;  // streams per chunk of the scan: 32768 streams are 32 chunks
constexpr int kPlanWaves = kPlanThreads / 64;
constexpr int kCopyThreads = 256;
constexpr int kCopyPart = kCopyThreads * 8;  // int16 per workgroup and step: 16 bytes per lane
constexpr int kCopyMaxParts = 32;

struct PlanParams {
	int mode;                // 1: lens; 2: the rule on levels
	int S;
	const int32_t *lens;     // mode 1
	// mode 2: buffer b of stream s is [mul * dec_block_begin(b), mul * dec_block_begin(b + 1)) of its row (GateParams)
	const int32_t *levels;   // [S][nblocks]
	const state_t *sin;
	int32_t *piece_off;      // [S][nblocks]: where buffer b starts in the stream's PACKED row, -1 when it is held
	int nblocks, N, D, mul;
	int level, conseq;
	rtlfm_packed_row *index;
	unsigned long long *total;
};

struct CopyParams {
	int mode;
	const int16_t *R;        // the rows
	size_t rstride;          // int16 per stream
	int16_t *packed;         // 16-byte aligned
	unsigned long long cap;  // int16
	const rtlfm_packed_row *index;
	const state_t *sin;      // mode 2 (as PlanParams)
	const int32_t *piece_off;
	int nblocks, N, D, mul;
};

__global__ void __launch_bounds__(kPlanThreads) k_pack_plan(PlanParams p)
{
	__shared__ unsigned long long wave_tot[kPlanWaves];
	const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
	unsigned long long carry = 0;  // the same in every lane
	for (int c0 = 0; c0 < p.S; c0 += kPlanThreads) {
		const int s = c0 + tid;
		int len = 0, held = 0;
		if (s < p.S) {
			if (p.mode == 2) {
				int hits = p.sin[s].squelch_hits;  // a local copy: the carried state is the run's to write
				const int p0 = p.D > 1 ? p.sin[s].prev_index : 0;
				for (int b = 0; b < p.nblocks; b++) {
					const size_t at = (size_t)s * p.nblocks + b;
					const int n = p.mul * (dec_block_begin(b + 1, p.N, p.D, p0) - dec_block_begin(b, p.N, p.D, p0));
					if (scan::gate_step(hits, p.levels[at], p.level, p.conseq)) {
						p.piece_off[at] = len;
						len += n;
					} else {
						p.piece_off[at] = -1;
						held++;
					}
				}
			} else {
				len = p.lens[s] > 0 ? p.lens[s] : 0;
			}
		}
		const unsigned long long padded = ((unsigned long long)len + 7) & ~7ull;
		unsigned long long x = padded;  // inclusive scan of the wave
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const unsigned long long y = __shfl_up(x, d);
			if (lane >= d) x += y;
		}
		if (lane == 63) wave_tot[wave] = x;
		__syncthreads();
		unsigned long long base = carry, chunk = 0;
#pragma unroll
		for (int w = 0; w < kPlanWaves; w++) {
			const unsigned long long t = wave_tot[w];
			if (w < wave) base += t;
			chunk += t;
		}
		if (s < p.S) {
			rtlfm_packed_row r;
			r.offset = base + x - padded;
			r.len = len; r.held = held;
			p.index[s] = r;
		}
		carry += chunk;
		__syncthreads();  // the totals have been read
	}
	if (tid == 0) *p.total = carry;
}

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// Destination vector v = source bytes [16 v + SH, 16 v + SH + 16) of the aligned source vectors a[]: SH even, 0 .. 14
template <int SH>
__device__ __forceinline__ void copy_vectors(const v4u *a, v4u *dst, int nv)
{
	constexpr int Q = SH >> 2;
	constexpr bool half = (SH & 2) != 0;
	for (int v = (int)(blockIdx.y * kCopyThreads + threadIdx.x); v < nv; v += (int)gridDim.y * kCopyThreads) {
		const v4u lo = a[v];
		v4u out = lo;
		if (SH != 0) {
			const v4u hi = a[v + 1];  // holds the vector's last bytes: SH > 0
			const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
			uint32_t o[4];
#pragma unroll
			for (int i = 0; i < 4; i++) o[i] = half ? (w[Q + i] >> 16) | (w[Q + i + 1] << 16) : w[Q + i];
			out = v4u{o[0], o[1], o[2], o[3]};
		}
		dst[v] = out;
	}
}

__global__ void __launch_bounds__(kCopyThreads) k_pack_copy(CopyParams p)
{
	const int tid = (int)threadIdx.x;
	size_t s = blockIdx.x;
	int b = 0;
	if (p.mode == 2) { s = blockIdx.x / (unsigned)p.nblocks; b = (int)(blockIdx.x % (unsigned)p.nblocks); }
	const rtlfm_packed_row row = p.index[s];
	const int16_t *src = p.R + s * p.rstride;
	unsigned long long dst = row.offset;
	long long n = row.len;
	if (p.mode == 2) {
		const int po = p.piece_off[blockIdx.x];
		const int p0 = p.D > 1 ? p.sin[s].prev_index : 0;
		const int t0 = p.mul * dec_block_begin(b, p.N, p.D, p0);
		n = po < 0 ? 0 : p.mul * dec_block_begin(b + 1, p.N, p.D, p0) - t0;
		src += t0;
		dst += po < 0 ? 0 : po;
	}
	if (b == 0 && blockIdx.y == 0 && tid < ((8 - (row.len & 7)) & 7)) {  // behind the row's last sample
		const unsigned long long e = row.offset + (unsigned long long)row.len + tid;
		if (e < p.cap) p.packed[e] = 0;
	}
	if (n <= 0 || dst >= p.cap) return;
	if (p.cap - dst < (unsigned long long)n) n = (long long)(p.cap - dst);
	int head = (int)((8 - (dst & 7)) & 7);
	if (head > n) head = (int)n;
	const int nv = (int)((n - head) >> 3);
	const int tail = (int)(n - head - 8ll * nv);
	int16_t *d = p.packed + dst;
	if (blockIdx.y == 0) {
		if (tid < head) d[tid] = src[tid];
		const long long k = head + 8ll * nv + (tid - 8);
		if (tid >= 8 && tid < 8 + tail) d[k] = src[k];
	}
	if (nv < 1) return;
	const uintptr_t A = (uintptr_t)(src + head);
	const v4u *a = reinterpret_cast<const v4u *>(A & ~(uintptr_t)15);
	v4u *dv = reinterpret_cast<v4u *>(d + head);
	switch ((int)(A & 15)) {  // the same in every lane of the piece
	case 0: copy_vectors<0>(a, dv, nv); break;
	case 2: copy_vectors<2>(a, dv, nv); break;
	case 4: copy_vectors<4>(a, dv, nv); break;
	case 6: copy_vectors<6>(a, dv, nv); break;
	case 8: copy_vectors<8>(a, dv, nv); break;
	case 10: copy_vectors<10>(a, dv, nv); break;
	case 12: copy_vectors<12>(a, dv, nv); break;
	default: copy_vectors<14>(a, dv, nv); break;
	}
}

// most_piece: the longest piece the launch can meet (int16), which sizes the grid's second dimension
static inline int launch_pack(const PlanParams &pp, const CopyParams &cp, size_t most_piece, hipStream_t q)
{
	if (pp.S < 1) return -EINVAL;
	const size_t pieces = pp.mode == 2 ? (size_t)pp.S * pp.nblocks : (size_t)pp.S;
	if (pieces > 0x7fffffffu) return -E2BIG;
	size_t gy = (most_piece + kCopyPart - 1) / kCopyPart;
	if (gy < 1) gy = 1;
	if (gy > kCopyMaxParts) gy = kCopyMaxParts;
	k_pack_plan<<<1, kPlanThreads, 0, q>>>(pp);
	k_pack_copy<<<dim3((unsigned)pieces, (unsigned)gy), kCopyThreads, 0, q>>>(cp);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

}  // namespace pack
}  // namespace rtlfm
