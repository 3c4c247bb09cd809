// channel_fir_kernel.h — a caller-supplied FIR channel filter behind the NCO mixer, in k_channel_boxcar's place.
//
// A boxcar /D is a sinc: its first sidelobe lies 13 dB down, and a channel cut out of a wideband capture has no tuner
// filter in front of it.  With a filter set (include/rtlfm_hip.h, rtlfm_gpu_set_channel_filter)
// an output is due at the samples e at which low_pass() (src/rtl_fm.c:461-481) emits one, and its value is
//     sat16((sum_{j < ntaps} taps[j] m[e - j] + r) >> shift),   r = shift ? 1 << (shift - 1) : 0
// of the mixed samples m (channel_kernel.h: the same table, phase and rounding), on I' and on Q'.  The sum is an int32
// that cannot overflow (rtlfm_channel_filter_check), so every order of summation gives the same bits.
//
// What is carried from run to run is the source history (channel_kernel.h, kHist: at least ntaps - 1 samples whatever
// ntaps is): the mixer is a pure function of pos and the bytes, so a launch mixes what it needs of the history again.
//
//   k_channel_fir        the product.  One launch from source bytes to every channel's decimated IQ, in k_channel_boxcar's
//                        frame: a workgroup is kWaves channels of one source over a stretch of tiles; a tile's source
//                        bytes and the halo in front of them are staged in LDS once for all of them, each wave mixes
//                        them for its channel into LDS (I' and Q' apart, packed int16 pairs), and a lane forms an output
//                        from 16-byte LDS reads of its window and of the taps with v_dot2_i32_i16.  Nothing at the capture
//                        rate goes to memory.  A segment owns the outputs that end inside it and needs no warm-up but the
//                        halo: there is no running sum, so any D goes with any segmentation.
//   k_channel_fir_plain  the cross-check: one lane per output over what k_channel_mix left of the history's last kHaloMax
//                        samples and the run (channel::k_source_history then writes the new history; k_channel_fir
//                        writes it itself).
#pragma once

#include "channel_kernel.h"
#include "fused_kernel.h"

namespace rtlfm {
namespace chanfir {

constexpr int kMaxTaps = RTLFM_CHANNEL_MAX_TAPS;
constexpr int kHaloMax = 1024;   // samples of the history the cross-check mixes in front of a run (>= kMaxTaps - 1, a multiple of 8)
constexpr int kTile = 1024;      // complex samples per tile (2 KiB of source bytes)
constexpr int kWaves = channel::kWaves;
constexpr int kGroup = 8;        // int16 per 16-byte LDS read: windows and taps are read in groups of eight
constexpr int kPad = 16;         // int16 behind a wave's mixed samples that a window's last group may reach into
static_assert(channel::kHist >= kMaxTaps - 1 && kHaloMax >= kMaxTaps - 1 && kHaloMax <= channel::kHist && kHaloMax % kGroup == 0 &&
              kTile % 256 == 0, "history / tile geometry");

// taps as the kernels read them: ntaps rounded up so that a window that starts anywhere in a group ends in a whole one
inline int padded_taps(int ntaps) { return (ntaps + 2 * kGroup - 2) / kGroup * kGroup; }
// samples in front of a tile that a launch stages with it: ntaps - 1, in whole 16-byte pieces of source bytes
inline int halo_of(int ntaps) { return (ntaps - 1 + kGroup - 1) / kGroup * kGroup; }
// dwords of one wave's I' (or Q') row in LDS
inline int mixed_row_dwords(int halo) { return (kTile + halo + kPad) / 2; }
inline size_t lds_bytes(int ntaps)
{
	const int halo = halo_of(ntaps);
	return 4 * ((size_t)channel::kTableSize + (size_t)kGroup * padded_taps(ntaps) / 2 + (size_t)(kTile + halo) / 2 +
	            (size_t)kWaves * 2 * mixed_row_dwords(halo));
}

// The eight copies of the taps a window reads them from: copy v is the taps in the order of the samples (oldest first),
// v zeros in front and zeros behind up to nt8 - the window of an output whose first sample is v int16 into a group.
inline void shifted_taps(const int16_t *taps, int ntaps, int16_t *out /* [kGroup][padded_taps(ntaps)] */)
{
	const int nt8 = padded_taps(ntaps);
	for (int v = 0; v < kGroup; v++)
		for (int i = 0; i < nt8; i++) {
			const int j = i - v;
			out[v * nt8 + i] = (j >= 0 && j < ntaps) ? taps[ntaps - 1 - j] : (int16_t)0;
		}
}

struct FirParams {
	channel::Frame f;         // (sout: now_r, now_j stay the copy's)
	const uint8_t *hist_in;   // [sources][channel::kHist * 2]: the bytes in front of the run
	uint8_t *hist_out;        // the same behind it (another buffer)
	const uint32_t *steps;    // [nstreams]
	const uint32_t *table;    // [channel::kTableSize]
	const uint32_t *taps8;    // shifted_taps(), as dwords
	int ntaps, nt8, halo, shift;
	int groups;               // workgroups that share a source tile = ceil(per_source / kWaves)
	const uint32_t *dc;       // k_channel_fir<true>: the sources' lists of biases (option source_dc; channel_kernel.h), dc_stride dwords apart
	size_t dc_stride;
	int dc_entries;           // ... and entries of a list: channel::kDcHist + T / 256
};

// Grid: ((source * segs) + seg) * groups + group; wave w = channel group * kWaves + w of the source (k_channel_boxcar's).
// Dynamic LDS: lds_bytes(ntaps).
// DC (k_channel_fir<true>; option source_dc; dynamic LDS: lds_bytes(ntaps) + kDcLds): the staged span covers several buffers
// and reaches into the history, so the biases of its 256-sample pieces - nine at most - are staged with it, behind the
// mixed samples, and a lane looks its dword's up there: the 64 lanes of a turn cover 128 samples, one or two entries, which
// LDS hands to all of them at once.
constexpr int kDcSlots = 16;
constexpr size_t kDcLds = kDcSlots * sizeof(uint32_t);
static_assert((kTile + kHaloMax) / channel::kDcPiece + 1 <= kDcSlots, "a span's pieces fit their slots");

// (One kernel body for both forms, as channel::k_channel_mix.)
template <bool DC>
__global__ void __launch_bounds__(kWaves * 64) k_channel_fir(const FirParams p)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	const int span = kTile + p.halo;  // samples staged per tile
	const int W = (span + kPad) / 2;
	uint32_t *s_table = lds;
	uint32_t *s_taps = s_table + channel::kTableSize;
	uint32_t *s_src = s_taps + kGroup * p.nt8 / 2;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	uint32_t *mI = s_src + span / 2 + wave * 2 * W, *mQ = mI + W;
	[[maybe_unused]] uint32_t *s_dc = s_src + span / 2 + kWaves * 2 * W;  // (DC only)
	const int group = (int)(blockIdx.x % (unsigned)p.groups);
	const int sseg = (int)(blockIdx.x / (unsigned)p.groups);
	const int seg = sseg % p.f.segs;
	const size_t src = (size_t)(sseg / p.f.segs);
	const int ch = group * kWaves + wave;
	const bool active = ch < p.f.per_source;
	const size_t s = src * (size_t)p.f.per_source + (size_t)(active ? ch : 0);

	for (int i = tid; i < channel::kTableSize; i += kWaves * 64) s_table[i] = p.table[i];
	for (int i = tid; i < kGroup * p.nt8 / 2; i += kWaves * 64) s_taps[i] = p.taps8[i];

	const int t_begin = seg * p.f.tiles_per_seg;
	const int t_end = min(p.f.ntiles, t_begin + p.f.tiles_per_seg);
	const uint8_t *row = p.f.iq + src * p.f.src_stride;
	const uint8_t *hold = p.hist_in + src * (size_t)(channel::kHist * 2);
	const uint32_t step = p.steps[s];
	const int D = p.f.D;
	const int p0 = p.f.sin[s].prev_index;
	const int p0c = channel::schedule(p0, p.f.T, D).p0c;
	uint32_t *Ys = p.f.Y + s * p.f.ystride;

	for (int t = t_begin; t < t_end; t++) {
		const int g0 = t * kTile - p.halo;  // the run sample staged first (below 0: the history's)
		__syncthreads();  // the source bytes of the tile before this one have been mixed by every wave
		[[maybe_unused]] const int pc0 = (g0 + channel::kHist) >> channel::kDcShift;  // the list's entry of the span's first piece (halo <= kHist: >= 0)
		if constexpr (DC) {
			// (past the run's end the span holds bytes 127: nothing comes off them but 127)
			if (tid < kDcSlots) s_dc[tid] = pc0 + tid < p.dc_entries ? p.dc[src * p.dc_stride + (size_t)(pc0 + tid)] : channel::kDcNone;
		}
		for (int u = tid; u < span / kGroup; u += kWaves * 64) {
			const int g = g0 + u * kGroup;
			uint4 v = make_uint4(0x7f7f7f7fu, 0x7f7f7f7fu, 0x7f7f7f7fu, 0x7f7f7f7fu);
			if (g < 0) v = *reinterpret_cast<const uint4 *>(hold + (size_t)(channel::kHist + g) * 2);
			else if (g < p.f.T) v = *reinterpret_cast<const uint4 *>(row + (size_t)g * 2);
			reinterpret_cast<uint4 *>(s_src)[u] = v;
		}
		__syncthreads();
		if (!active) continue;
		// the channel's mixed samples of the halo and the tile: two per lane and turn
		for (int i = lane; i < span / 2; i += 64) {
			const uint32_t w = s_src[i];
			const uint32_t ph = (p.f.pos + (uint32_t)(g0 + 2 * i)) * step;
			int i0, q0, i1, q1;
			if constexpr (DC) {
				const channel::pk16 bias = __builtin_bit_cast(channel::pk16, s_dc[((g0 + 2 * i + channel::kHist) >> channel::kDcShift) - pc0]);
				channel::mix_bias(w, 0, s_table[ph >> channel::kPhaseShift], bias, i0, q0);
				channel::mix_bias(w, 1, s_table[(ph + step) >> channel::kPhaseShift], bias, i1, q1);
			} else {
				channel::mix(w, 0, s_table[ph >> channel::kPhaseShift], i0, q0);
				channel::mix(w, 1, s_table[(ph + step) >> channel::kPhaseShift], i1, q1);
			}
			mI[i] = pack_iq(i0, i1);
			mQ[i] = pack_iq(q0, q1);
		}
		channel::wave_sync();
		// the outputs that end inside the tile, one per lane and turn: consecutive lanes store consecutive dwords
		const int ts = t * kTile, te = min(ts + kTile, p.f.T);
		const int kt0 = (ts + p0c) / D, kt1 = min((te + p0c) / D, p.f.maxout);
		for (int k = kt0 + lane; k < kt1; k += 64) {
			const int e = (k + 1) * D - p0c - 1;                            // the run sample the output is due at
			const int l0 = min(max(e - g0 - p.ntaps + 1, 0), span - p.ntaps);  // its window's first sample, as staged
			const uint4 *pt = reinterpret_cast<const uint4 *>(s_taps) + (l0 & (kGroup - 1)) * (p.nt8 / kGroup);
			const uint4 *pi = reinterpret_cast<const uint4 *>(mI) + (l0 >> 3);
			const uint4 *pq = reinterpret_cast<const uint4 *>(mQ) + (l0 >> 3);
			int ai = 0, aq = 0;
			for (int j = 0; j < p.nt8 / kGroup; j++) {
				const uint4 a = pt[j], x = pi[j], y = pq[j];
				int r0, r1, r2, r3, r4, r5, r6, r7;
				fused::dot2_pair(a.x, x.x, y.x, r0, r1);
				fused::dot2_pair(a.y, x.y, y.y, r2, r3);
				fused::dot2_pair(a.z, x.z, y.z, r4, r5);
				fused::dot2_pair(a.w, x.w, y.w, r6, r7);
				ai += (r0 + r2) + (r4 + r6);
				aq += (r1 + r3) + (r5 + r7);
			}
			Ys[k] = channel::round_sat_pack(ai, aq, p.shift);
		}
	}
	if (active && seg == p.f.segs - 1 && lane == 0) channel::leave_schedule(p.f.sout, p.f.cnt, s, channel::schedule(p0, p.f.T, D));
	if (group == 0 && seg == p.f.segs - 1) {
#pragma unroll
		for (int u = tid; u < channel::kHist / kGroup; u += kWaves * 64)
			reinterpret_cast<uint4 *>(p.hist_out + src * (size_t)(channel::kHist * 2))[u] = channel::history_piece(row, hold, p.f.T, u);
	}
}


// ---- the cross-check ----
// X: [nstreams][xstride] mixed samples, the history's last kHaloMax in front of the run's T (k_channel_mix, twice).
__global__ void __launch_bounds__(256)
k_channel_fir_plain(const uint32_t *__restrict__ X, size_t xstride, int nstreams, int T, int D, const int16_t *__restrict__ taps,
                    int ntaps, int shift, int maxout, uint32_t *__restrict__ Y, size_t ystride, int32_t *__restrict__ cnt,
                    const state_t *__restrict__ sin, state_t *__restrict__ sout)
{
	RTLFM_GRID_STRIDE(g, (size_t)nstreams * maxout) {
		const size_t s = g / (size_t)maxout;
		const int k = (int)(g % (size_t)maxout);
		const channel::Schedule sc = channel::schedule(sin[s].prev_index, T, D);
		if (k == 0) channel::leave_schedule(sout, cnt, s, sc);
		if (k >= (T + sc.p0c) / D) continue;
		const uint32_t *x = X + s * xstride + kHaloMax + ((k + 1) * D - sc.p0c - 1);
		int ai = 0, aq = 0;
		for (int j = 0; j < ntaps; j++) {
			const iq16 m = unpack_iq(x[-j]);
			ai += (int)taps[j] * m.i;
			aq += (int)taps[j] * m.q;
		}
		Y[s * ystride + k] = channel::round_sat_pack(ai, aq, shift);
	}
}

}  // namespace chanfir
}  // namespace rtlfm
