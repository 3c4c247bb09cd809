// channel_kernel.h — K channels per wideband source: the NCO mixer in the place of rotate16_neg90.
//
// The reference's only frequency translation is rotate16_neg90 (src/rtl_fm.c:424-434): fs/4, fixed, one channel per
// dongle.  Here a stream is channel s % per_source of source s / per_source, and sample n of the run is turned by
//     phase = (uint32)((pos + n) * step[s]),   (c, s) = table[phase >> 22]   (1024 entries, Q14, built on the host)
//     I' = (x c + y s + 8192) >> 14,   Q' = (y c - x s + 8192) >> 14         (x = I - 127, y = Q - 127)
// which is e^(-j theta): step = 2^30 is the reference's 1, -j, -1, +j to the bit, step = 0 the identity
// (offset_tuning).  Everything behind the mixer is the reference's chain on I', Q' (include/rtlfm_hip.h,
// rtlfm_gpu_set_channels).
//
//   k_channel_mix      k_convert with the mixer: packed int16 IQ at the capture rate for the staged kernels.  Every
//                      configuration; the cross-check.
//   k_channel_boxcar   low_pass() (src/rtl_fm.c:461-481) behind the mixer in one launch, source bytes to decimated IQ:
//                      a workgroup stages an 8 KiB tile of ONE source in LDS once, and each of its waves mixes and sums
//                      it for another channel of that source.  Nothing at the capture rate goes back to memory.
//   k_source_history   the cross-checks' copy of the carried source history (the one-launch kernels write it themselves).
//   k_source_dc_smooth option source_dc: dc_block_raw_filter's averages per SOURCE and buffer, as the list of what comes off
//                      every 256-sample piece in front of the mixers, the filter and the bank (the DC forms of the kernels).
//
// The channel filter (channel_fir_kernel.h) and the channel bank (channel_bank_kernel.h) stand in k_channel_boxcar's place
// and share what is here: the launch frame, the output schedule, the rounding of a sum and the source history.
#pragma once

#include <cmath>

#include "staged_kernels.h"

namespace rtlfm {
namespace channel {

constexpr int kTableBits = 10;
constexpr int kTableSize = 1 << kTableBits;  // entries: int16 cos | int16 sin << 16
constexpr int kPhaseShift = 32 - kTableBits;
constexpr int kTileSamples = 4096;           // complex samples per tile (8 KiB of source bytes)
constexpr int kTileUnits = kTileSamples * 2 / 16;  // 16-byte pieces
constexpr int kWaves = 4;                    // channels per workgroup
constexpr int kLaneSamples = kTileSamples / 64;    // consecutive samples of a tile one lane owns
constexpr int kRowDwords = kLaneSamples / 2;       // ... as source dwords (two samples each)
constexpr int kRowStride = kRowDwords + 4;   // rows 144 bytes apart: the lanes of a ds_read_b128 group cover all 64 banks
constexpr int kMaxD = kTileSamples;          // up to here one warm-up tile reaches back a whole boxcar; beyond, one segment
constexpr int kStageMinD = 4;                // from here on a tile's outputs of a channel leave through LDS, as whole lines
constexpr int kOutCap = kTileSamples / kStageMinD + 8;  // ... and this is room for them (4096 / D + 1 at most)
// The history: what the handle carries from run to run for the filter and the bank is every SOURCE's last kHist complex
// samples as raw bytes (bytes 127 where nothing has been consumed yet: they mix to 0 at every phase), in two copies: a run
// reads one and writes the other, and the handle changes over once per run - the two executions of verify_twice read the
// same history.
constexpr int kHist = 4096;
static_assert(kHist % 8 == 0, "the history moves in 16-byte pieces");

// the table as rtlfm_channel_table hands it out: [i][0] = lround(16384 cos(2 pi i / 1024)), [i][1] = the same of sin
inline void build_table(int16_t *cos_sin)
{
	for (int i = 0; i < kTableSize; i++) {
		const double a = 2.0 * M_PI * (double)i / (double)kTableSize;
		cos_sin[2 * i] = (int16_t)lround(16384.0 * cos(a));
		cos_sin[2 * i + 1] = (int16_t)lround(16384.0 * sin(a));
	}
}

typedef short pk16 __attribute__((ext_vector_type(2)));

// Sample `half` (0 / 1) of a source dword (bytes I0 Q0 I1 Q1) times e^(-j theta), cs = the table entry of theta:
// (x, y) = (I - 127, Q - 127) as one packed pair, then I' = (x, y) . (c, s) and Q' = (y, x) . (c, -s), each one
// v_dot2_i32_i16 with the rounding constant as its accumulator (the compiler keeps the wait states of its own dots).
// bias: what comes off the bytes - (127, 127), or with option source_dc (127 + aI, 127 + aQ) of the sample's buffer.
__device__ __forceinline__ void mix_bias(uint32_t w, int half, uint32_t cs, pk16 bias, int &i, int &q)
{
	const uint32_t spread = __builtin_amdgcn_perm(0u, w, half ? 0x0c030c02u : 0x0c010c00u);  // I | Q << 16
	const pk16 xy = __builtin_bit_cast(pk16, spread) - bias;
	const uint32_t xyw = __builtin_bit_cast(uint32_t, xy);
	const pk16 yx = __builtin_bit_cast(pk16, (xyw >> 16) | (xyw << 16));
	const pk16 c_s = __builtin_bit_cast(pk16, cs);
	const pk16 c_ms = c_s * (pk16){1, -1};
	i = __builtin_amdgcn_sdot2(xy, c_s, 8192, false) >> 14;
	q = __builtin_amdgcn_sdot2(yx, c_ms, 8192, false) >> 14;
}
__device__ __forceinline__ void mix(uint32_t w, int half, uint32_t cs, int &i, int &q)
{
	mix_bias(w, half, cs, (pk16){127, 127}, i, q);
}

// (one wave's LDS operations complete in the order it issues them: the fences are for the compiler)
__device__ __forceinline__ void wave_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// an int32 sum of the filter or the bank as a sample: rounded, shifted, saturated, packed
__device__ __forceinline__ uint32_t round_sat_pack(int ai, int aq, int shift)
{
	const int r = shift ? 1 << (shift - 1) : 0;
	return pack_iq(min(max((ai + r) >> shift, -32768), 32767), min(max((aq + r) >> shift, -32768), 32767));
}

// What every front end has in common: the run, its cut into segments, and where the results go.
struct Frame {
	const uint8_t *iq;        // source rows
	size_t src_stride;
	uint32_t pos;             // complex samples consumed before this run (mod 2^32: all the phase needs)
	int T;                    // complex samples of the run (a multiple of 256: buffers are multiples of 512 bytes)
	int D;                    // outputs every D samples
	int maxout;               // most outputs a stream's run can have; a Y row has room for one dword more
	int per_source;           // channels per source
	int segs, tiles_per_seg, ntiles;
	uint32_t *Y;              // decimated IQ, packed int16 pairs
	size_t ystride;           // dwords per stream
	int32_t *cnt;             // [nstreams] outputs of the run
	const state_t *sin;
	state_t *sout;            // already a copy of sin: prev_index (the boxcar: and now_r, now_j) is written here
};

// Where a run's outputs fall: with p0 = prev_index samples of an output already consumed, output k is due at run sample
// (k + 1) D - p0 - 1 (low_pass(), src/rtl_fm.c:461-481).  The count and the record take p0 as it is; the filter and the
// bank place their outputs by p0c (a broken record moves outputs, never an index out of its row).
struct Schedule {
	int p0c;         // p0 inside [0, D)
	int E;           // outputs of the run
	int prev_index;  // p0 of the next run
};
__device__ __forceinline__ Schedule schedule(int p0, int T, int D)
{
	Schedule sc;
	sc.p0c = min(max(p0, 0), D - 1);
	sc.E = (p0 + T) / D;
	sc.prev_index = p0 + T - sc.E * D;
	return sc;
}
__device__ __forceinline__ void leave_schedule(state_t *sout, int32_t *cnt, size_t s, const Schedule &sc)
{
	sout[s].prev_index = sc.prev_index;
	cnt[s] = sc.E;
}

// Where the new history's 16-byte piece u comes from: run sample T - kHist + 8 u, or - a run shorter than the history -
// the old history, shifted.  (T is a multiple of 8: nothing straddles.)
__device__ __forceinline__ uint4 history_piece(const uint8_t *row, const uint8_t *hold, int T, int u)
{
	const int n = T - kHist + u * 8;
	return n >= 0 ? *reinterpret_cast<const uint4 *>(row + (size_t)n * 2)
	              : *reinterpret_cast<const uint4 *>(hold + (size_t)(kHist + n) * 2);
}

__global__ void __launch_bounds__(256)
k_source_history(const uint8_t *__restrict__ iq, size_t src_stride, const uint8_t *__restrict__ hist_in, uint8_t *__restrict__ hist_out,
                 int nsources, int T)
{
	RTLFM_GRID_STRIDE(g, (size_t)nsources * (kHist / 8)) {
		const size_t src = g / (kHist / 8);
		const int u = (int)(g % (kHist / 8));
		reinterpret_cast<uint4 *>(hist_out + src * (size_t)(kHist * 2))[u] =
			history_piece(iq + src * src_stride, hist_in + src * (size_t)(kHist * 2), T, u);
	}
}

// ------------------------------------------------------------------ source_dc ----
// Option source_dc (include/rtlfm_hip.h): dc_block_raw_filter's averages (src/rtl_fm.c:1043-1065) per SOURCE and buffer,
// taken off every sample in front of every front end.  What the front ends read is one list per source, a dword per
// 256-sample piece - buffers are whole multiples of 256 samples, so a piece has one buffer and one pair -:
//     dc[source][kDcHist + T / 256],   entry j = the piece that starts at run sample (j - kDcHist) * 256
// the history's sixteen pieces in front, then the run's.  An entry is the BIAS of its piece, (127 + aI) | (127 + aQ) << 16
// as two int16: what mix_bias() and the bank take off the bytes; kDcNone where nothing was subtracted (a = 0).  The list's
// last kDcHist entries are the next run's history, whatever T is: a run shorter than the history shifts whole pieces.
constexpr int kDcPiece = 256;
constexpr int kDcShift = 8;
constexpr int kDcHist = kHist / kDcPiece;
constexpr uint32_t kDcNone = 0x007f007fu;
static_assert(kHist % kDcPiece == 0 && (1 << kDcShift) == kDcPiece, "the history is whole pieces");

// the bias of run sample g (>= -kHist) out of a source's list
__device__ __forceinline__ pk16 dc_bias(const uint32_t *dcrow, int g)
{
	return __builtin_bit_cast(pk16, dcrow[(g + kHist) >> kDcShift]);
}

// k_rdc_smooth by source: the recurrence runs down one lane out of LDS as there.  The carried value is channel 0's,
// clamped to [-128, 128] on the way in (a broken record moves values, never a bound: |a| <= 128 by induction); every
// channel's record receives the last one.  Writes the source's list - the history's entries from hist_in (none: kDcNone),
// the run's - and the next history's entries to hist_out (none: a run of the boxcar, which carries no history).
__global__ void __launch_bounds__(64)
k_source_dc_smooth(const long long *__restrict__ sums /* [source][b][2] */, uint32_t L, int nblocks, int nsources, int per_source, int k,
                   const state_t *__restrict__ sin, state_t *__restrict__ sout, const uint32_t *__restrict__ hist_in,
                   uint32_t *__restrict__ hist_out, uint32_t *__restrict__ dc, size_t dc_stride)
{
	const size_t src = blockIdx.x;
	if (src >= (size_t)nsources) return;
	const int lane = (int)threadIdx.x;
	uint32_t *row = dc + src * dc_stride;
	__shared__ int2 m[64];
	__shared__ int2 last;
	if (lane < kDcHist) row[lane] = hist_in ? hist_in[src * kDcHist + lane] : kDcNone;
	const state_t &rec = sin[src * (size_t)per_source];
	int pi = min(max(rec.dc_avgI, -128), 128), pq = min(max(rec.dc_avgQ, -128), 128);
	const int pairs = (int)(L / 2), ppb = (int)(L / (2 * kDcPiece));
	for (int base = 0; base < nblocks; base += 64) {
		const int b = base + lane;
		const int cnt = nblocks - base < 64 ? nblocks - base : 64;
		if (b < nblocks)
			m[lane] = make_int2((int)(sums[(src * nblocks + b) * 2] / pairs), (int)(sums[(src * nblocks + b) * 2 + 1] / pairs));
		__syncthreads();
		if (lane == 0) {
			for (int t = 0; t < cnt; t++) {
				const int2 v = m[t];
				pi = sdiv_trunc(v.x + pi * k, k + 1);  // (|v| <= 128, |p| <= 128, k <= 65535: no overflow; k + 1 > 0)
				pq = sdiv_trunc(v.y + pq * k, k + 1);
				m[t] = make_int2(pi, pq);
			}
			last = make_int2(pi, pq);
		}
		__syncthreads();
		for (int i = lane; i < cnt * ppb; i += 64) {
			const int2 a = m[i / ppb];
			row[kDcHist + (size_t)base * ppb + i] = (uint32_t)(uint16_t)(127 + a.x) | (uint32_t)(uint16_t)(127 + a.y) << 16;
		}
		__syncthreads();
	}
	// (the block's own stores, behind a barrier)
	if (hist_out && lane < kDcHist) hist_out[src * kDcHist + lane] = row[(size_t)nblocks * ppb + lane];
	for (int c = lane; c < per_source; c += 64) {
		sout[src * (size_t)per_source + c].dc_avgI = last.x;
		sout[src * (size_t)per_source + c].dc_avgQ = last.y;
	}
}

// ---------------------------------------------------------------- k_channel_mix ----
// One thread per 16 source bytes = 8 complex samples of one stream, as k_convert; the row read is the SOURCE's.
// DC (k_channel_mix<true>; option source_dc): the bias of the thread's eight samples from entry dc_off + n / 256 of the
// source's list - dc_off = kDcHist for a run, kDcHist - halo / 256 for the end of the history the filter's cross-check
// mixes.  (The body stands in the kernel itself, for both forms: behind a call, even an inlined one, the compiler lays the
// off form out differently from the kernel it was - profiles/source_dc_isa_compare.txt.)
template <bool DC>
__global__ void __launch_bounds__(256)
k_channel_mix(const uint8_t *__restrict__ iq, size_t src_stride, uint32_t L, int nblocks, int nstreams, int per_source,
              const uint32_t *__restrict__ steps, const uint32_t *__restrict__ table, uint32_t pos,
              uint32_t *__restrict__ X, size_t xstride, const uint32_t *__restrict__ dc, size_t dc_stride, int dc_off)
{
	__shared__ uint32_t s_table[kTableSize];
	for (int i = threadIdx.x; i < kTableSize; i += blockDim.x) s_table[i] = table[i];
	__syncthreads();
	const size_t per_block = L / 16;
	const size_t total = (size_t)nstreams * nblocks * per_block;
	RTLFM_GRID_STRIDE(g, total) {
		const size_t j = g % per_block;
		const size_t sb = g / per_block;
		const int b = (int)(sb % nblocks);
		const size_t s = sb / nblocks;
		const size_t src = s / (size_t)per_source;
		const uint4 raw = *reinterpret_cast<const uint4 *>(iq + src * src_stride + (size_t)b * L + j * 16);
		const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
		const uint32_t step = steps[s];
		const uint32_t n = (uint32_t)b * (L / 2) + (uint32_t)j * 8;  // sample of the run
		uint32_t ph = (pos + n) * step;
		[[maybe_unused]] pk16 bias;
		if constexpr (DC) bias = __builtin_bit_cast(pk16, dc[src * dc_stride + (size_t)dc_off + (n >> kDcShift)]);
		uint32_t o[8];
#pragma unroll
		for (int k = 0; k < 8; k++) {
			int re, im;
			if constexpr (DC) mix_bias(w[k >> 1], k & 1, s_table[ph >> kPhaseShift], bias, re, im);
			else mix(w[k >> 1], k & 1, s_table[ph >> kPhaseShift], re, im);
			ph += step;
			o[k] = pack_iq(re, im);
		}
		uint4 *dst = reinterpret_cast<uint4 *>(X + s * xstride + (size_t)b * (L / 2) + j * 8);
		dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
		dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
	}
}

// ------------------------------------------------------------- k_channel_boxcar ----
struct BoxParams {
	Frame f;                  // (D: the boxcar's length)
	const uint32_t *steps;    // [nstreams]
	const uint32_t *table;    // [kTableSize]
	int groups;               // workgroups that share a source tile = ceil(per_source / kWaves)
	const uint32_t *dc;       // k_channel_boxcar<STAGE, true>: the sources' lists of biases (option source_dc), dc_stride dwords apart
	size_t dc_stride;
};

// inclusive prefix sum over the wave's 64 lanes (wrapping)
__device__ __forceinline__ uint32_t wave_scan(uint32_t v, int lane)
{
#pragma unroll
	for (int off = 1; off < 64; off <<= 1) {
		const uint32_t u = (uint32_t)__shfl_up((int)v, off, 64);
		if (lane >= off) v += u;
	}
	return v;
}

// Grid: ((source * segs) + seg) * groups + group; 4 waves, wave w = channel group * 4 + w of the source.
//
// With p0 = prev_index samples already summed in (now_r, now_j), output k of a stream ends behind run sample
// e_k = (k + 1) D - p0 (k_boxcar's definition).  P(n) = now_r + the mixed samples [0, n), wrapping; output k =
// P(e_k) - P(e_(k-1)) with P(e_(-1)) = 0, and the int16 store takes its low half as the reference's does
// (src/rtl_fm.c:473-474).  A lane owns 64 consecutive samples of a tile: it mixes them once, sums from boundary to
// boundary and stores every output that ends inside its stretch at once; the first of them lacks what lay between the
// last boundary in front of the stretch and the stretch, which a wave scan of the lanes' totals tells the lane afterwards.
// A segment owns the outputs that end inside it; from the second segment on, the tile in front of it is run without
// stores, which leaves the boundary the first own output starts from (D <= kMaxD; beyond that a stream is one segment).
// STAGE (D >= kStageMinD): a tile's outputs of a channel are gathered in LDS and leave as consecutive dwords of the whole
// wave; without it every lane stores its own, 4 bytes wherever a boundary falls (at /10: 13 cache lines per store
// instruction; LAB.md I.38).
// DC (option source_dc): a lane's 64 samples lie in one 256-sample piece, so one bias per lane and tile comes off them in
// the mixer.  (One kernel body for both forms, as k_channel_mix.)
template <bool STAGE, bool DC>
__global__ void __launch_bounds__(kWaves * 64) k_channel_boxcar(const BoxParams p)
{
	__shared__ uint32_t s_table[kTableSize];
	__shared__ __attribute__((aligned(16))) uint32_t s_tile[64 * kRowStride];
	__shared__ uint32_t s_out[STAGE ? kWaves * kOutCap : 1];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int group = (int)(blockIdx.x % (unsigned)p.groups);
	const int sseg = (int)(blockIdx.x / (unsigned)p.groups);
	const int seg = sseg % p.f.segs;
	const size_t src = (size_t)(sseg / p.f.segs);
	const int ch = group * kWaves + wave;
	const bool active = ch < p.f.per_source;
	const size_t s = src * (size_t)p.f.per_source + (size_t)(active ? ch : 0);

	for (int i = tid; i < kTableSize; i += kWaves * 64) s_table[i] = p.table[i];

	const int t_begin = seg * p.f.tiles_per_seg;
	const int t_end = min(p.f.ntiles, t_begin + p.f.tiles_per_seg);
	const int t_first = seg > 0 ? t_begin - 1 : 0;  // the warm-up tile
	const uint8_t *row = p.f.iq + src * p.f.src_stride;
	const size_t run_bytes = (size_t)p.f.T * 2;

	// the tile a thread stages: 16-byte pieces tid and tid + 256
	uint4 r0 = make_uint4(0, 0, 0, 0), r1 = r0;
	auto fetch = [&](int t) {
		const size_t b0 = (size_t)t * (kTileSamples * 2) + (size_t)tid * 16, b1 = b0 + 256 * 16;
		r0 = b0 < run_bytes ? *reinterpret_cast<const uint4 *>(row + b0) : make_uint4(0, 0, 0, 0);
		r1 = b1 < run_bytes ? *reinterpret_cast<const uint4 *>(row + b1) : make_uint4(0, 0, 0, 0);
	};
	fetch(t_first);

	const uint32_t step = p.steps[s];
	const int D = p.f.D;
	const int p0 = p.f.sin[s].prev_index;
	// P at the current tile's first sample, and P at the last boundary so far (wave-uniform)
	uint32_t carry_i = 0, carry_q = 0, last_i = 0, last_q = 0;
	if (seg == 0) { carry_i = (uint32_t)p.f.sin[s].now_r; carry_q = (uint32_t)p.f.sin[s].now_j; }
	uint32_t *Ys = p.f.Y + s * p.f.ystride;
	uint32_t *outw = &s_out[STAGE ? wave * kOutCap : 0];

	for (int t = t_first; t < t_end; t++) {
		__syncthreads();  // the tile before this one has been read by every wave
		*reinterpret_cast<uint4 *>(&s_tile[(tid >> 3) * kRowStride + (tid & 7) * 4]) = r0;
		*reinterpret_cast<uint4 *>(&s_tile[((tid + 256) >> 3) * kRowStride + (tid & 7) * 4]) = r1;
		__syncthreads();
		if (t + 1 < t_end) fetch(t + 1);  // in flight while this tile is mixed
		if (!active) continue;
		const bool emit = t >= t_begin;
		const int a = t * kTileSamples + lane * kLaneSamples;  // the lane's first sample of the run
		// sums from the lane's first sample on, and what they were at the stretch's last boundary so far
		uint32_t run_i = 0, run_q = 0, pb_i = 0, pb_q = 0;
		const uint32_t k0 = (uint32_t)((a + p0) / D);  // the output that ends at the stretch's first boundary
		uint32_t k = k0;
		// stores go to min(max(k, lo), hi): the output's place, or - in the warm-up tile, and for an index a broken record
		// would lead to - the spare dword behind the row's last possible output
		const uint32_t hi = (uint32_t)p.f.maxout, lo = emit ? 0u : hi;
		const uint32_t kt0 = (uint32_t)((t * kTileSamples + p0) / D);  // the first output that ends inside the tile
		if (a < p.f.T) {
			int left = (int)(k0 + 1) * D - p0 - a;  // samples up to and including the one the next output ends behind
			uint32_t ph = (p.f.pos + (uint32_t)a) * step;
			[[maybe_unused]] pk16 bias;
			if constexpr (DC) bias = dc_bias(p.dc + src * p.dc_stride, a);
			const uint4 *rowp = reinterpret_cast<const uint4 *>(&s_tile[lane * kRowStride]);
			for (int v = 0; v < kRowDwords / 4; v++) {
				const uint4 raw = rowp[v];
				const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
				uint32_t cs[8];  // the eight table entries first: the gathers are in flight together
#pragma unroll
				for (int j = 0; j < 8; j++) {
					cs[j] = s_table[ph >> kPhaseShift];
					ph += step;
				}
#pragma unroll
				for (int j = 0; j < 8; j++) {
					int re, im;
					if constexpr (DC) mix_bias(w[j >> 1], j & 1, cs[j], bias, re, im);
					else mix(w[j >> 1], j & 1, cs[j], re, im);
					run_i += (uint32_t)re; run_q += (uint32_t)im;
					if (--left == 0) {
						// (the stretch's first output lacks what lay in front of the stretch: added below)
						const uint32_t o = pack_iq((int)(run_i - pb_i), (int)(run_q - pb_q));
						if constexpr (STAGE) outw[min(k - kt0, (uint32_t)(kOutCap - 1))] = o;
						else Ys[min(max(k, lo), hi)] = o;
						pb_i = run_i; pb_q = run_q;
						k++;
						left = D;
					}
				}
			}
		}
		const uint32_t tot_i = run_i, tot_q = run_q;
		const uint32_t inc_i = wave_scan(tot_i, lane), inc_q = wave_scan(tot_q, lane);
		const uint32_t pex_i = carry_i + inc_i - tot_i, pex_q = carry_q + inc_q - tot_q;  // P at the lane's first sample
		const uint32_t pl_i = pex_i + pb_i, pl_q = pex_q + pb_q;                          // P at the lane's last boundary
		const unsigned long long have = __ballot(k != k0);
		const unsigned long long below = have & ((1ull << lane) - 1ull);
		const int from = below ? 63 - __clzll((long long)below) : 0;
		const uint32_t got_i = (uint32_t)__shfl((int)pl_i, from, 64), got_q = (uint32_t)__shfl((int)pl_q, from, 64);
		const uint32_t prev_i = below ? got_i : last_i, prev_q = below ? got_q : last_q;
		// the lane's own store of a moment ago, completed by P(first sample) - P(the boundary in front of it)
		if constexpr (STAGE) {
			if (k != k0) {
				const uint32_t at = min(k0 - kt0, (uint32_t)(kOutCap - 1));
				const iq16 mine = unpack_iq(outw[at]);
				outw[at] = pack_iq((int)((uint32_t)(int)mine.i + pex_i - prev_i), (int)((uint32_t)(int)mine.q + pex_q - prev_q));
			}
			wave_sync();
			if (emit) {
				const int tile_end = min((t + 1) * kTileSamples, p.f.T);
				const uint32_t kt1 = min((uint32_t)((tile_end + p0) / D), hi);  // one past the last output that ends inside the tile
				for (uint32_t i = (uint32_t)lane; kt0 + i < kt1 && i < (uint32_t)kOutCap; i += 64) Ys[kt0 + i] = outw[i];
			}
		} else if (emit && k != k0 && k0 < hi) {
			const iq16 mine = unpack_iq(Ys[k0]);
			Ys[k0] = pack_iq((int)((uint32_t)(int)mine.i + pex_i - prev_i), (int)((uint32_t)(int)mine.q + pex_q - prev_q));
		}
		if (have) {
			const int top = 63 - __clzll((long long)have);
			last_i = (uint32_t)__shfl((int)pl_i, top, 64);
			last_q = (uint32_t)__shfl((int)pl_q, top, 64);
		}
		carry_i += (uint32_t)__shfl((int)inc_i, 63, 64);
		carry_q += (uint32_t)__shfl((int)inc_q, 63, 64);
	}
	if (active && seg == p.f.segs - 1 && lane == 0) {
		// the partial sum that stays behind
		p.f.sout[s].now_r = (int)(carry_i - last_i);
		p.f.sout[s].now_j = (int)(carry_q - last_q);
		leave_schedule(p.f.sout, p.f.cnt, s, schedule(p0, p.f.T, D));
	}
}


// segments per stream: enough waves to fill the GPU, no segment shorter than min_tiles (each but the first re-runs a tile)
inline void plan(int nstreams, int ntiles, int D, int target_waves, int min_tiles, int tiles_per_seg, int *segs, int *tps)
{
	int n = 1;
	if (D <= kMaxD) {
		if (tiles_per_seg > 0) {
			n = (ntiles + tiles_per_seg - 1) / tiles_per_seg;
		} else {
			n = (target_waves + nstreams - 1) / nstreams;
			const int most = ntiles / (min_tiles > 0 ? min_tiles : 1);
			if (n > most) n = most;
		}
	}
	if (n < 1) n = 1;
	if (n > ntiles) n = ntiles;
	*tps = (ntiles + n - 1) / n;
	*segs = (ntiles + *tps - 1) / *tps;
}

}  // namespace channel
}  // namespace rtlfm
