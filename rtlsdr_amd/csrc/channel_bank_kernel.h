// channel_bank_kernel.h — the channel bank: K uniformly spaced channels of one wideband source by K polyphase sums and one
// K-point fix_fft per output instant, in the mixer bank's place (include/rtlfm_hip.h, rtlfm_gpu_set_channel_bank;
// DESIGN.md section 8.5).
//
// With x[n] = (I - 127, Q - 127) of the source, n = pos + the index within the run, an output is due at the samples e at
// which low_pass() (src/rtl_fm.c:461-481) emits one for the source's channel 0, and per component
//     u_r = sum over j < ntaps with (e - j) mod K == r of taps[j] x[e - j],   v_r = sat16((u_r + rnd) >> shift)
//     Y   = fix_fft(v) as rtl_power defines it (src/rtl_power.c:271-327) with N_WAVE = K
// channel c's decimated IQ sample is Y[bins[c]].  u_r is an int32 that cannot overflow (rtlfm_channel_bank_check), so every
// order of summation gives the same bits; every butterfly is rtlpower::butterfly (fix_fft_butterfly.h), the reference's
// bit for bit, and the butterflies of one stage are independent of each other.
//
// What is carried from run to run is the source history (channel_kernel.h, kHist; bytes 127: x = 0).
//
//   k_channel_bank   the product.  One launch from source bytes to every selected channel's decimated IQ.  A workgroup is
//                    one source over a stretch of tiles of F output instants ("frames").  Per tile the bytes the frames'
//                    windows cover are staged in LDS once, as int16 in polyphase order (I and Q apart, the samples of one
//                    residue contiguous); the taps lie there per branch, reversed, in two copies (one shifted by a sample:
//                    a window starts on either parity of its row), so that a sum is v_dot2_i32_i16 over pairs.  A lane
//                    forms one (frame, residue) sum and writes it where fix_fft's bit reversal would put it; a wave then
//                    runs the log2 K stages over its batch of max(128, K) points (128 / K frames, or one frame with two
//                    butterflies per lane), leaves the last stage's results in LDS as [bin][frame], and the workgroup
//                    hands every selected bin's row its stretch of frames as one contiguous piece.
//   k_channel_bank_survey, k_bank_survey_reduce
//                    option bank_survey (rtlfm_gpu_bank_survey): the same body, which also adds up every bin's Yi^2 + Yq^2
//                    over the segment's frames out of the [bin][frame] results, and the sum over the segments.
//   k_bank_power_plain
//                    the survey's cross-check: one lane per (source, bin) over the cross-check's transforms.
//   k_bank_sums, k_bank_fft, k_bank_scatter
//                    the cross-check: one lane per (frame, residue) forms v in memory, one lane per frame runs fix_fft in
//                    the reference's own loop order with FIX_MPY spelled out, a scatter and channel::k_source_history
//                    follow.
#pragma once

#include "channel_kernel.h"
#include "fix_fft_butterfly.h"
#include "fused_kernel.h"

namespace rtlfm {
namespace chanbank {

constexpr int kMaxTaps = RTLFM_BANK_MAX_TAPS;
constexpr int kHist = channel::kHist;
constexpr int kMinLog2 = 2, kMaxLog2 = 8;
constexpr int kWaves = 4;
constexpr int kBatchMin = 128;    // points a wave transforms at once: every lane has a butterfly in every stage
constexpr int kOutDwords = 4096;  // [bin][frame] results of a tile
constexpr int kSpanMax = 6144;    // samples staged per tile at most
constexpr int kFramesMax = 256;
constexpr size_t kLdsMax = 64 * 1024;
static_assert(kHist >= kMaxTaps - 1, "history geometry");

// What host and kernel agree on for one (K, ntaps, D).
struct Geometry {
	int m, K;
	int Q;      // taps per branch (the longest)
	int Qp;     // int16 per branch as stored: Q, a sample of shift, zeros up to an even count whose half is odd (LDS banks)
	int lead;   // samples staged in front of a tile's first frame: (Q + 1) K, so that no window index is negative
	int F;      // frames per tile
	int Ls;     // int16 per residue row of the staged samples (even, its half odd)
	int Fs;     // dwords per bin row of the results (odd)
	int batch;  // points per wave and turn
	int extra;  // dwords behind the results: the survey's sums of the segment's end, or none
	size_t lds; // bytes
};

inline size_t lds_of(const Geometry &g)
{
	return 4 * ((size_t)g.K + (size_t)g.K * g.Qp + (size_t)g.K * g.Ls + (size_t)kWaves * g.batch + (size_t)g.K * g.Fs + (size_t)g.extra);
}

// survey: with room behind the results for k_channel_bank_survey's 256 64-bit sums (F shrinks where that needs it)
inline Geometry geometry(int m, int ntaps, int D, bool survey = false)
{
	Geometry g{};
	g.m = m; g.K = 1 << m;
	g.extra = survey ? 2 * kWaves * 64 : 0;
	g.Q = (ntaps + g.K - 1) / g.K;
	g.Qp = (g.Q + 2) & ~1;
	if (!((g.Qp / 2) & 1)) g.Qp += 2;
	g.lead = (g.Q + 1) * g.K;
	g.batch = g.K > kBatchMin ? g.K : kBatchMin;
	long long f = ((long long)kSpanMax - g.lead - 1) / D + 1;
	if (f > kOutDwords / g.K) f = kOutDwords / g.K;
	if (f > kFramesMax) f = kFramesMax;
	if (f < 1) f = 1;
	g.F = (int)f;
	for (;;) {
		const long long span = (long long)(g.F - 1) * D + g.lead + 1;
		const int qmax = (int)((span + g.K - 2) >> m);  // the last row index a staged sample gets
		g.Ls = (qmax + 6 + 1) & ~1;                     // a window reads up to Qp - Q <= 4 entries past its newest sample
		if (!((g.Ls / 2) & 1)) g.Ls += 2;
		g.Fs = g.F | 1;
		g.lds = lds_of(g);
		if (g.lds <= kLdsMax || g.F == 1) break;
		g.F = (g.F + 1) / 2;
	}
	return g;
}

// The two copies of the taps: copy v, branch b, entry i multiplies the row sample i - v places behind the window's first,
// the window's newest sample being entry Q - 1 + v: taps[b + (Q - 1 + v - i) K], zero outside the filter.
inline void branch_taps(const int16_t *taps, int ntaps, const Geometry &g, int16_t *out /* [2][K][Qp] */)
{
	for (int v = 0; v < 2; v++)
		for (int b = 0; b < g.K; b++)
			for (int i = 0; i < g.Qp; i++) {
				const int qq = g.Q - 1 + v - i;
				const long long j = (long long)b + (long long)qq * g.K;
				out[((size_t)v * g.K + b) * g.Qp + i] = (qq >= 0 && qq < g.Q && j < ntaps) ? taps[j] : (int16_t)0;
			}
}

struct BankParams {
	channel::Frame f;         // (tiles: of F frames; T need only be a multiple of 8)
	const uint8_t *hist_in;   // [sources][kHist * 2]: the bytes in front of the run
	uint8_t *hist_out;        // the same behind it (another buffer)
	const uint32_t *taps2;    // branch_taps(), as dwords
	const uint32_t *tw;       // [K] fix_fft's twiddles per stage, doubled and packed (fix_fft_butterfly.h)
	const int32_t *bins;      // [per_source], or [sources][per_source] with bins_stride = per_source (rtlfm_gpu_set_channel_bins)
	int m, Q, Qp, lead, F, Ls, Fs, shift;
	int bins_stride;          // 0: one list for every source
	unsigned long long *survey;  // k_channel_bank_survey: [sources][segs][K] partial sums
	const uint32_t *dc;       // the _dc kernels: the sources' lists of biases (option source_dc; channel_kernel.h), dc_stride dwords apart
	size_t dc_stride;
};

// What comes off run sample g's bytes: 127, or - option source_dc - the bias of its piece.  Silence (sample_at) stays x = 0.
template <bool DC>
__device__ __forceinline__ channel::pk16 bias_at(const uint32_t *dcrow, int T, int g)
{
	if constexpr (DC) {
		if (g < T && g >= -kHist) return channel::dc_bias(dcrow, g);
	}
	return (channel::pk16){127, 127};
}

// One complex sample of the source as a dword (I | Q << 8): run sample g, the history in front of the run, or silence.
__device__ __forceinline__ uint32_t sample_at(const uint8_t *row, const uint8_t *hold, int T, int g)
{
	if (g >= T || g < -kHist) return 0x7f7fu;
	return g >= 0 ? (uint32_t)*reinterpret_cast<const uint16_t *>(row + (size_t)g * 2)
	              : (uint32_t)*reinterpret_cast<const uint16_t *>(hold + (size_t)(kHist + g) * 2);
}

// The body of k_channel_bank and k_channel_bank_survey.  SURVEY: every bin's power over the frames of the workgroup's segment
// as well (rtlfm_gpu_bank_survey): a lane owns bin tid % K and, per tile, the frames [c len, (c + 1) len) with c = tid / K -
// len = K below 32 bins (one pass covers 256 frames), else the tile's frames shared out among the 256 / K lanes of a bin.
// The rows of s_out are an odd number of dwords apart, so the 32 lanes of a half wave - min(K, 32) bins, the frame groups
// a multiple of K apart where K < 32 - read 32 different banks whatever Fs is.  The lane keeps its sum in a 64-bit
// register over all tiles; at the segment's end the lanes of a bin inside a wave add up by shuffles, the waves through LDS.
// DC (the _dc kernels; option source_dc): the bias of a sample's piece comes off in the staging loop in 127's place, so the
// survey sees a bin 0 without the spike with no further change.
template <bool SURVEY, bool DC>
__device__ __forceinline__ void bank_body(const BankParams &p)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
	const int m = p.m, K = 1 << m, Km = K - 1;
	const int batch = K > kBatchMin ? K : kBatchMin;
	const int Lh = p.Ls / 2, Qh = p.Qp / 2;
	uint32_t *s_tw = lds;
	uint32_t *s_taps = s_tw + K;
	uint32_t *s_I = s_taps + K * p.Qp;
	uint32_t *s_Q = s_I + K * Lh;
	uint32_t *s_work = s_Q + K * Lh;
	uint32_t *s_out = s_work + kWaves * batch;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int seg = (int)(blockIdx.x % (unsigned)p.f.segs);
	const size_t src = (size_t)(blockIdx.x / (unsigned)p.f.segs);
	const size_t s0 = src * (size_t)p.f.per_source;
	const int32_t *bins = p.bins + src * (size_t)p.bins_stride;

	for (int i = tid; i < K; i += kWaves * 64) s_tw[i] = p.tw[i];
	for (int i = tid; i < K * p.Qp; i += kWaves * 64) s_taps[i] = p.taps2[i];

	const uint8_t *row = p.f.iq + src * p.f.src_stride;
	const uint8_t *hold = p.hist_in + src * (size_t)(kHist * 2);
	const uint32_t *dcrow = DC ? p.dc + src * p.dc_stride : nullptr;
	const int D = p.f.D;
	const int p0 = p.f.sin[s0].prev_index;         // one schedule per source: channel 0's
	const channel::Schedule sc = channel::schedule(p0, p.f.T, D);
	const int p0c = sc.p0c;
	const int E = min((p.f.T + p0c) / D, p.f.maxout);
	const int t_begin = seg * p.f.tiles_per_seg;
	const int t_end = min(p.f.ntiles, t_begin + p.f.tiles_per_seg);
	int16_t *hI = reinterpret_cast<int16_t *>(s_I), *hQ = reinterpret_cast<int16_t *>(s_Q);
	uint32_t *wk = s_work + wave * batch;
	const int gf = batch >> m;  // frames per batch
	unsigned long long sv_acc = 0;
	const int sv_bin = tid & Km, sv_c = tid >> m;
	const int sv_len = K < 32 ? K : (p.F + (kWaves * 64 >> m) - 1) / (kWaves * 64 >> m);

	for (int t = t_begin; t < t_end; t++) {
		const int k0 = t * p.F;
		if (k0 >= E) break;  // (the same for the whole workgroup)
		const int nf = min(p.F, E - k0);
		const int e0 = (k0 + 1) * D - p0c - 1;  // the run sample the tile's first frame is due at
		const int g0 = e0 - p.lead;             // the run sample staged first (below 0: the history's)
		const int base = (int)((p.f.pos + (uint32_t)g0) & (uint32_t)Km);  // its residue: row index = (u + base) >> m
		const int span = (nf - 1) * D + p.lead + 1;
		__syncthreads();  // the tile before this one has been summed and stored by every wave
		for (int u = tid; u < span; u += kWaves * 64) {
			const uint32_t w = sample_at(row, hold, p.f.T, g0 + u);
			const int up = u + base;
			const int at = (up & Km) * p.Ls + (up >> m);
			const channel::pk16 bias = bias_at<DC>(dcrow, p.f.T, g0 + u);
			hI[at] = (int16_t)((int)(w & 0xffu) - bias.x);
			hQ[at] = (int16_t)((int)(w >> 8) - bias.y);
		}
		__syncthreads();
		const int nb = (nf + gf - 1) / gf;
		for (int bt = wave; bt < nb; bt += kWaves) {
			channel::wave_sync();  // (the batch before this one has left the work buffer)
			// the polyphase sums, one (frame, residue) per lane and turn, to where the bit reversal puts them
			for (int i = lane; i < batch; i += 64) {
				const int f = min(bt * gf + (i >> m), nf - 1);  // (a frame past the tile's end repeats the last; never stored)
				const int r = i & Km;
				const int ue = f * D + p.lead + base;
				const int b = (ue - r) & Km;      // the branch: the newest tap that meets residue r
				const int qn = (ue - b) >> m;     // row index of the newest sample of the window
				const int qs = qn - p.Q + 1, v = qs & 1;
				const uint32_t *pt = s_taps + (v * K + b) * Qh;
				const uint32_t *pi = s_I + r * Lh + ((qs - v) >> 1);
				const uint32_t *pq = s_Q + r * Lh + ((qs - v) >> 1);
				int ai = 0, aq = 0;
				for (int j = 0; j < Qh; j++) {
					int r0, r1;
					fused::dot2_pair(pt[j], pi[j], pq[j], r0, r1);
					ai += r0;
					aq += r1;
				}
				wk[(i & ~Km) | (int)(__brev((unsigned)r) >> (32 - m))] = channel::round_sat_pack(ai, aq, p.shift);
			}
			channel::wave_sync();
			for (int st = 0; st < m; st++) {
				const int half = 1 << st;
				for (int t2 = lane; t2 < batch / 2; t2 += 64) {
					const int fr = t2 >> (m - 1), tt = t2 & (K / 2 - 1);
					const int q = tt & (half - 1);
					const int i = ((tt >> st) << (st + 1)) | q;
					const int at = (fr << m) | i;
					uint32_t a = wk[at], b = wk[at + half];
					rtlpower::butterfly<0>(a, b, s_tw[half - 1 + q]);
					if (st < m - 1) {
						wk[at] = a;
						wk[at + half] = b;
					} else {
						const int f = bt * gf + fr;
						if (f < nf) {
							s_out[i * p.Fs + f] = a;
							s_out[(i + half) * p.Fs + f] = b;
						}
					}
				}
				channel::wave_sync();
			}
		}
		__syncthreads();
		// every selected bin's row receives the tile's frames as one contiguous piece: consecutive lanes, consecutive dwords
		for (int x = tid; x < p.f.per_source * nf; x += kWaves * 64) {
			const int c = x / nf, f = x - c * nf;
			p.f.Y[(s0 + (size_t)c) * p.f.ystride + (size_t)(k0 + f)] = s_out[bins[c] * p.Fs + f];
		}
		if constexpr (SURVEY) {
			const uint32_t *ro = s_out + sv_bin * p.Fs;
			const int f1 = min(min(nf, sc.E - k0), (sv_c + 1) * sv_len);  // (sc.E: what frames says - a broken record's count may be smaller than E)
			for (int f = sv_c * sv_len; f < f1; f++) {
				const iq16 y = unpack_iq(ro[f]);
				sv_acc += (uint32_t)(y.i * y.i) + (uint32_t)(y.q * y.q);  // (at most 2^31: a dword; the sum is 64 bits from the first addition)
			}
		}
	}
	if constexpr (SURVEY) {
		// (also of a segment that owns no frame, and of a run with none: zeros, never what an earlier run left)
		for (int off = K; off < 64; off <<= 1) {
			const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)sv_acc, off, 64);
			const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(sv_acc >> 32), off, 64);
			sv_acc += (unsigned long long)hi << 32 | lo;
		}
		unsigned long long *s_fin = reinterpret_cast<unsigned long long *>(s_out + ((K * p.Fs + 1) & ~1));  // [256]
		s_fin[tid] = sv_acc;
		__syncthreads();
		const int stride = K < 64 ? 64 : K;
		for (int b = tid; b < K; b += kWaves * 64) {
			unsigned long long sum = 0;
			for (int at = b; at < kWaves * 64; at += stride) sum += s_fin[at];
			p.survey[(src * (size_t)p.f.segs + (size_t)seg) * (size_t)K + (size_t)b] = sum;
		}
	}
	if (seg == p.f.segs - 1) {
		for (int c = tid; c < p.f.per_source; c += kWaves * 64) channel::leave_schedule(p.f.sout, p.f.cnt, s0 + c, sc);
		for (int u = tid; u < kHist / 8; u += kWaves * 64)
			reinterpret_cast<uint4 *>(p.hist_out + src * (size_t)(kHist * 2))[u] = channel::history_piece(row, hold, p.f.T, u);
	}
}

// Grid: source * segs + seg.  Dynamic LDS: Geometry::lds.
__global__ void __launch_bounds__(kWaves * 64) k_channel_bank(const BankParams p) { bank_body<false, false>(p); }
__global__ void __launch_bounds__(kWaves * 64) k_channel_bank_dc(const BankParams p) { bank_body<false, true>(p); }

// ... the same with the survey's partial sums, [source][seg][K], stored at the segment's end (Geometry of survey = true)
__global__ void __launch_bounds__(kWaves * 64) k_channel_bank_survey(const BankParams p) { bank_body<true, false>(p); }
__global__ void __launch_bounds__(kWaves * 64) k_channel_bank_survey_dc(const BankParams p) { bank_body<true, true>(p); }

// The segments' partial sums into power [source][K], and the frames the run emitted for the source into frames [source]:
// one lane per (source, bin).
__global__ void __launch_bounds__(256)
k_bank_survey_reduce(const unsigned long long *__restrict__ partial, int segs, int m, int nsources, int per_source, int T, int D,
                     const state_t *__restrict__ sin, unsigned long long *__restrict__ power, int32_t *__restrict__ frames)
{
	RTLFM_GRID_STRIDE(g, (size_t)nsources << m) {
		const size_t src = g >> m;
		const size_t b = g & (((size_t)1 << m) - 1);
		unsigned long long sum = 0;
		for (int sg = 0; sg < segs; sg++) sum += partial[((src * (size_t)segs + (size_t)sg) << m) + b];
		power[g] = sum;
		if (b == 0) frames[src] = channel::schedule(sin[src * per_source].prev_index, T, D).E;
	}
}

// ---- the cross-check ----
// V: [sources][maxout][K] the sums v, then in place their transforms.
template <bool DC>
__global__ void __launch_bounds__(256)
k_bank_sums(const uint8_t *__restrict__ iq, size_t src_stride, const uint8_t *__restrict__ hist_in, const int16_t *__restrict__ taps,
            int ntaps, int m, int shift, uint32_t pos, int nsources, int per_source, int T, int D, int maxout,
            const state_t *__restrict__ sin, uint32_t *__restrict__ V, const uint32_t *__restrict__ dc, size_t dc_stride)
{
	const int K = 1 << m;
	RTLFM_GRID_STRIDE(g, ((size_t)nsources * maxout) << m) {
		const int r = (int)(g & (size_t)(K - 1));
		const size_t sk = g >> m;
		const int k = (int)(sk % (size_t)maxout);
		const size_t src = sk / (size_t)maxout;
		const int p0c = channel::schedule(sin[src * per_source].prev_index, T, D).p0c;
		if (k >= min((T + p0c) / D, maxout)) continue;
		const int e = (k + 1) * D - p0c - 1;
		const uint8_t *row = iq + src * src_stride;
		const uint8_t *hold = hist_in + src * (size_t)(kHist * 2);
		int ai = 0, aq = 0;
		for (int j = (int)((pos + (uint32_t)e - (uint32_t)r) & (uint32_t)(K - 1)); j < ntaps; j += K) {
			const uint32_t w = sample_at(row, hold, T, e - j);
			const channel::pk16 bias = bias_at<DC>(dc + src * dc_stride, T, e - j);
			ai += (int)taps[j] * ((int)(w & 0xffu) - bias.x);
			aq += (int)taps[j] * ((int)(w >> 8) - bias.y);
		}
		V[g] = channel::round_sat_pack(ai, aq, shift);
	}
}

// fix_fft (src/rtl_power.c:271-327) on one frame per lane, in the reference's loop order; sine: sine_table(m), [3 K / 4]
__global__ void __launch_bounds__(256)
k_bank_fft(uint32_t *__restrict__ V, const int16_t *__restrict__ sine, int m, int nsources, int per_source, int T, int D, int maxout,
           const state_t *__restrict__ sin)
{
	const int n = 1 << m;
	RTLFM_GRID_STRIDE(g, (size_t)nsources * maxout) {
		const int k = (int)(g % (size_t)maxout);
		const size_t src = g / (size_t)maxout;
		const int p0c = channel::schedule(sin[src * per_source].prev_index, T, D).p0c;
		if (k >= min((T + p0c) / D, maxout)) continue;
		uint32_t *x = V + (g << m);
		int rev = 0;
		for (int idx = 1; idx <= n - 1; idx++) {
			int bit = n;
			do {
				bit >>= 1;
			} while (rev + bit > n - 1);
			rev = (rev & (bit - 1)) + bit;
			if (rev <= idx) continue;
			const uint32_t tmp = x[idx];
			x[idx] = x[rev];
			x[rev] = tmp;
		}
		int kk = m - 1;
		for (int half = 1; half < n; half <<= 1, kk--) {
			const int step = half << 1;
			for (int q = 0; q < half; q++) {
				const int j = q << kk;
				const int wr = (int)(int16_t)sine[j + n / 4] >> 1, wi = (int)(int16_t)(-sine[j]) >> 1;
				for (int i = q; i < n; i += step) {
					const iq16 a = unpack_iq(x[i]), b = unpack_iq(x[i + half]);
					const int tr = (int)(int16_t)(rtlpower::fix_mpy(wr, b.i) - rtlpower::fix_mpy(wi, b.q));
					const int ti = (int)(int16_t)(rtlpower::fix_mpy(wr, b.q) + rtlpower::fix_mpy(wi, b.i));
					const int qr = a.i >> 1, qi = a.q >> 1;
					x[i + half] = pack_iq((int)(int16_t)(qr - tr), (int)(int16_t)(qi - ti));
					x[i] = pack_iq((int)(int16_t)(qr + tr), (int)(int16_t)(qi + ti));
				}
			}
		}
	}
}

__global__ void __launch_bounds__(256)
k_bank_scatter(const uint32_t *__restrict__ V, const int32_t *__restrict__ bins, size_t bins_stride, int m, int nstreams, int per_source, int T, int D,
               int maxout, uint32_t *__restrict__ Y, size_t ystride, int32_t *__restrict__ cnt, const state_t *__restrict__ sin,
               state_t *__restrict__ sout)
{
	RTLFM_GRID_STRIDE(g, (size_t)nstreams * maxout) {
		const size_t s = g / (size_t)maxout;
		const int k = (int)(g % (size_t)maxout);
		const size_t src = s / (size_t)per_source;
		const int c = (int)(s % (size_t)per_source);
		const channel::Schedule sc = channel::schedule(sin[src * per_source].prev_index, T, D);
		if (k == 0) channel::leave_schedule(sout, cnt, s, sc);
		if (k >= min((T + sc.p0c) / D, maxout)) continue;
		Y[s * ystride + k] = V[(((src * (size_t)maxout) + k) << m) + bins[src * bins_stride + c]];
	}
}

// The survey's cross-check: one lane per (source, bin) walks the transforms in V frame by frame.
__global__ void __launch_bounds__(256)
k_bank_power_plain(const uint32_t *__restrict__ V, int m, int nsources, int per_source, int T, int D, int maxout,
                   const state_t *__restrict__ sin, unsigned long long *__restrict__ power, int32_t *__restrict__ frames)
{
	RTLFM_GRID_STRIDE(g, (size_t)nsources << m) {
		const size_t src = g >> m;
		const size_t b = g & (((size_t)1 << m) - 1);
		const channel::Schedule sc = channel::schedule(sin[src * per_source].prev_index, T, D);
		const int E = min(min((T + sc.p0c) / D, maxout), sc.E);  // (the frames written, and no more than frames says)
		unsigned long long sum = 0;
		for (int k = 0; k < E; k++) {
			const iq16 y = unpack_iq(V[(((src * (size_t)maxout) + k) << m) + b]);
			sum += (uint32_t)(y.i * y.i) + (uint32_t)(y.q * y.q);
		}
		power[g] = sum;
		if (b == 0) frames[src] = sc.E;
	}
}

}  // namespace chanbank
}  // namespace rtlfm
