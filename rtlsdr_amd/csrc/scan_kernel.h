// scan_kernel.h — the two device pieces of scanning ("use multiple -f for scanning (requires squelch)"):
//
//   k_scan_gate   the demod thread's rule (demod_thread_fn, src/rtl_fm.c:1366-1370) for every buffer of a run: while
//                 squelch_hits > conseq_squelch the buffer is NOT handed to the output thread and the counter is held at
//                 conseq_squelch + 1.  The counter itself moves as full_demod() moves it (:1206-1213) on the per-buffer
//                 rms() the run keeps in d_levels.  Runs LAST in a run, behind the front end, the squelch and any audio
//                 tail: a held buffer has passed through all of them (its filter state counts), only its output is dropped.
//   k_scan_mute   the callback's mute (rtlsdr_callback, :1289-1296): the first bytes after a retune read 127.
//
// k_scan_gate, one workgroup per stream:
//   1. lane 0 walks the run's levels in order from sin[s].squelch_hits - a short, true dependency chain -, writes one
//      rtlfm_gate_rec per buffer and leaves the emit flags in LDS (kGateChunk buffers at a time);
//   2. the whole workgroup compacts the stream's PCM row in place, buffer by buffer: emitted buffers move down over the
//      held ones, in order.  Buffer b's samples are [mul * dec_block_begin(b), mul * dec_block_begin(b + 1)) of the row
//      (exactly k_squelch_apply's t0 / t1; mul = 2 for -M raw's I, Q pairs).
//   Ordering of the move: the destination of an emitted buffer never lies above its source (dst <= src, by induction:
//   dst_end(b) = dst(b) + n(b) <= src(b) + n(b) = src(b + 1)), so nothing is overwritten before it has been read by a
//   LATER buffer or chunk.  Inside one chunk of kGateMove samples every lane loads its piece, the workgroup meets at a
//   barrier, then every lane stores: the stores of chunk i can only land on sources of chunk i itself (all loaded before
//   the barrier) or of earlier chunks.  One barrier per chunk is enough: a lane stores chunk i + 1 only behind barrier
//   i + 1, which every lane passes after its loads of chunk i + 1.
//   A stream with nothing held moves nothing (dst == src throughout); one with everything held moves nothing either.
//   It reads sin and the uncompacted row and writes sout / the records / the count: executing it twice on a freshly
//   demodulated row gives the same bytes (verify_twice).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/rtlfm_hip.h"
#include "staged_kernels.h"

namespace rtlfm {
namespace scan {

constexpr int kGateThreads = 256;
constexpr int kGateChunk = 1024;               // buffers whose flags lane 0 leaves in LDS at a time
constexpr int kGateMove = kGateThreads * 8;    // int16 samples per chunk of the move: 16 bytes per lane

struct GateParams {
	const int32_t *levels;   // [nstreams][nblocks] rms() per buffer of this run
	const state_t *sin;
	state_t *sout;
	int16_t *R;              // the run's final rows
	size_t rstride;          // int16 per stream
	rtlfm_gate_rec *recs;    // record of buffer b of stream s at recs[s * rec_stride + b]
	int rec_stride;
	int32_t *cnt, *cnt2;     // per-stream int16 count behind the gate (either may be null)
	int nblocks, N, D, mul;  // N input samples per buffer through a boxcar D (1: a uniform N outputs per buffer)
	int level, conseq;
};

// n int16 from src down to dst (dst < src) by the whole workgroup
__device__ __forceinline__ void move_down(int16_t *dst, const int16_t *src, int n)
{
	typedef uint32_t v4u __attribute__((ext_vector_type(4)));
	const int tid = (int)threadIdx.x;
	int done = 0;
	if ((((uintptr_t)dst | (uintptr_t)src) & 15) == 0) {
		const int nv = n & ~7;
		for (; done < nv; done += kGateMove) {
			const int at = done + tid * 8;
			v4u v = {0, 0, 0, 0};
			if (at < nv) v = *reinterpret_cast<const v4u *>(src + at);
			__syncthreads();
			if (at < nv) *reinterpret_cast<v4u *>(dst + at) = v;
		}
		done = nv;
	}
	for (; done < n; done += kGateMove) {
		int16_t v[8];
#pragma unroll
		for (int k = 0; k < 8; k++) {
			const int at = done + k * kGateThreads + tid;
			v[k] = at < n ? src[at] : (int16_t)0;
		}
		__syncthreads();
#pragma unroll
		for (int k = 0; k < 8; k++) {
			const int at = done + k * kGateThreads + tid;
			if (at < n) dst[at] = v[k];
		}
	}
}

// The rule for one buffer (k_scan_gate, and k_pack_plan of pack_kernel.h): the counter moves as full_demod() moves it on the
// buffer's rms() `sr` - a negative level changes nothing -, the buffer is held while hits > conseq, and a held buffer
// leaves the counter at conseq + 1.  Clamping does not change a decision: a counter above conseq stays above it until a
// level at or above the squelch zeroes it, clamped or not.  Returns whether the buffer is emitted.
__device__ __forceinline__ bool gate_step(int &hits, int sr, int level, int conseq)
{
	if (sr >= 0) hits = sr < level ? hits + 1 : 0;       // src/rtl_fm.c:1206-1213
	const bool hold = hits > conseq;                      // :1366
	if (hold) hits = conseq + 1;                          // :1368
	return !hold;
}

__global__ void __launch_bounds__(kGateThreads) k_scan_gate(GateParams p)
{
	__shared__ uint8_t emit[kGateChunk];
	__shared__ int32_t carry_hits;
	const size_t s = blockIdx.x;
	const int tid = (int)threadIdx.x;
	const int p0 = p.D > 1 ? p.sin[s].prev_index : 0;
	int16_t *row = p.R + s * p.rstride;
	if (tid == 0) carry_hits = p.sin[s].squelch_hits;
	int dst = 0;  // the same in every lane
	for (int c0 = 0; c0 < p.nblocks; c0 += kGateChunk) {
		const int c1 = c0 + kGateChunk < p.nblocks ? c0 + kGateChunk : p.nblocks;
		__syncthreads();  // the flags of the chunk before have been used
		if (tid == 0) {
			int hits = carry_hits;
			for (int b = c0; b < c1; b++) {
				const bool emitted = gate_step(hits, p.levels[s * p.nblocks + b], p.level, p.conseq);
				rtlfm_gate_rec r;
				r.hits_after = hits; r.emit = emitted ? 1 : 0; r.pad[0] = r.pad[1] = r.pad[2] = 0;
				p.recs[s * p.rec_stride + b] = r;
				emit[b - c0] = r.emit;
			}
			carry_hits = hits;
		}
		__syncthreads();
		for (int b = c0; b < c1; b++) {
			if (!emit[b - c0]) continue;
			const int src = p.mul * dec_block_begin(b, p.N, p.D, p0);
			const int n = p.mul * dec_block_begin(b + 1, p.N, p.D, p0) - src;
			if (dst != src && n > 0) move_down(row + dst, row + src, n);
			dst += n;
		}
	}
	if (tid == 0) {
		p.sout[s].squelch_hits = carry_hits;
		if (p.cnt) p.cnt[s] = dst;
		if (p.cnt2) p.cnt2[s] = dst;
	}
}

static inline int launch_gate(const GateParams &p, int nstreams, hipStream_t q)
{
	k_scan_gate<<<(unsigned)nstreams, kGateThreads, 0, q>>>(p);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

// ---- the mute -------------------------------------------------------------------------------------------------
// One entry per buffer that has bytes to mute: the first `nbytes` bytes at base + offset become 127.  Grid (entries,
// 16-byte units): whole aligned units as 16-byte stores of 0x7f7f7f7f words, the bytes in front of the first aligned
// unit and behind the last one bytewise by the first lanes of the entry's first workgroup.
struct MuteEntry {
	unsigned long long offset;
	uint32_t nbytes;
	uint32_t pad_;
};
constexpr int kMuteThreads = 256;

__global__ void __launch_bounds__(kMuteThreads) k_scan_mute(uint8_t *base, const MuteEntry *entries)
{
	typedef uint32_t v4u __attribute__((ext_vector_type(4)));
	const MuteEntry e = entries[blockIdx.x];
	uint8_t *p = base + e.offset;
	const uint32_t n = e.nbytes;
	uint32_t head = (uint32_t)((16 - ((uintptr_t)p & 15)) & 15);
	if (head > n) head = n;
	const uint32_t units = (n - head) / 16;
	const uint32_t tail = n - head - units * 16;
	const v4u fill = {0x7f7f7f7fu, 0x7f7f7f7fu, 0x7f7f7f7fu, 0x7f7f7f7fu};
	for (uint32_t u = blockIdx.y * kMuteThreads + threadIdx.x; u < units; u += gridDim.y * kMuteThreads)
		*reinterpret_cast<v4u *>(p + head + (size_t)u * 16) = fill;
	if (blockIdx.y == 0 && threadIdx.x < 16) {
		if (threadIdx.x < head) p[threadIdx.x] = 127;
		if (threadIdx.x < tail) p[head + (size_t)units * 16 + threadIdx.x] = 127;
	}
}

// max_bytes: the largest nbytes among the entries (sizes the grid)
static inline int launch_mute(uint8_t *base, const MuteEntry *d_entries, int nentries, uint32_t max_bytes, hipStream_t q)
{
	if (nentries < 1) return 0;
	unsigned gy = (unsigned)((max_bytes / 16 + kMuteThreads - 1) / kMuteThreads);
	if (gy < 1) gy = 1;
	if (gy > 64) gy = 64;
	k_scan_mute<<<dim3((unsigned)nentries, gy), kMuteThreads, 0, q>>>(base, d_entries);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

}  // namespace scan
}  // namespace rtlfm
