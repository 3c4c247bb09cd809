// run_plan.h — what an rtl_fm run launches, decided before its first launch.
//
// plan_run() is a pure function of the configuration, the run's buffer count, the handle's stream count, the handful of
// options in rtlfm_route_opts and the alignment of the caller's rows.  It reads no handle, no allocation and never
// touches the device; rtlfm_hip.hip's run_device_once() calls it once per run and switches on its route, and
// rtlfm_run_route() exports it.  Everything it is built from lives here too: the configuration's validation, the
// predicates of the front ends (what k_fused and k_boxcar_scan cover in each of their forms), the audio tail's plan.
// No HIP in this file unless hipcc compiles it: tools/fm_route_check.cpp builds it with a plain host compiler.
#pragma once

#include <cerrno>
#include <cstddef>
#include <cstdint>

#include "../../include/rtlfm_hip.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define RTLFM_HOST_DEVICE __host__ __device__
#else
#define RTLFM_HOST_DEVICE
#endif

#ifndef RTLFM_PASS0_DEFAULT
#define RTLFM_PASS0_DEFAULT 1  // 0: always v_dot4 on the VALU, 1: int8 MFMA where it is faster (RTLFM_PASS0=valu|mfma overrides)
#endif

namespace rtlfm {

constexpr int kDeemphGap = 62;  // candidates per chunk must fit a wave (staged_kernels.h, k_deemph_scan_*)

// k_deep_rest's tail lengths per level for `passes` (index 0 = level 6): what the next level, the filter and the demodulator
// reach back (staged_kernels.h; the kernel and the planner both ask)
RTLFM_HOST_DEVICE inline void deep_rest_tails(int passes, int fir, int k[6])
{
	const int L = passes - 6;
	k[L] = fir ? 10 : 1;
	for (int j = L - 1; j >= 0; j--) {
		k[j] = 2 * k[j + 1] + 5;
		if (k[j] < 6) k[j] = 6;
	}
}

// ---- the two conditions every front end's predicates share ----
// fm / am / usb / lsb: the front end can demodulate (-M raw's output is the decimated IQ itself)
inline bool pcm_mode(const rtlfm_cfg &c)
{
	return c.mode == RTLFM_MODE_FM || c.mode == RTLFM_MODE_AM || c.mode == RTLFM_MODE_USB || c.mode == RTLFM_MODE_LSB;
}
// the power squelch or -L: rms() of every buffer's decimated IQ is wanted (src/rtl_fm.c:1204-1237)
inline bool wants_levels(const rtlfm_cfg &c) { return c.squelch_level != 0 || c.report_levels != 0; }

namespace fused {

constexpr int kLaneSamples = 64;
constexpr int kTileSamples = 64 * kLaneSamples;  // 4096
constexpr int kTileBytes = 2 * kTileSamples;     // 8192
constexpr int kMaxP = 6;

// the pass-0 engine a launch will use: the handle's choice (option pass0_engine), else the compiled default
inline int effective_engine(int pass0_engine) { return pass0_engine >= 0 ? pass0_engine : (RTLFM_PASS0_DEFAULT ? 1 : 0); }

// buffers that are not whole 8 KiB tiles (-W n) take the partial-tile kernels: MFMA engine
inline bool needs_partial_tiles(const rtlfm_cfg &c) { return (c.block_len % kTileBytes) != 0; }

// one launch from the bytes to the PCM: up to six passes, no squelch
// (-E rdc: the RDC instantiations; -W n: the PT ones - both MFMA pass 0 only; plan_run checks the engine)
inline bool supported(const rtlfm_cfg &c)
{
	return pcm_mode(c) && c.downsample_passes >= 1 && c.downsample_passes <= kMaxP && !wants_levels(c);
}

// What the front end in emit mode plus staged kernels covers beyond supported(): 7..10 passes, -M raw, and the squelch
// (rtlfm_hip.hip: run_fused_emit)
inline bool supported_emit(const rtlfm_cfg &c)
{
	if (c.downsample_passes < 1 || c.downsample_passes > RTLFM_MAX_PASSES) return false;
	return c.downsample_passes > kMaxP || c.mode == RTLFM_MODE_RAW || wants_levels(c);
}

// the power squelch / -L with rms()'s sums taken by the front end itself and k_squelch_apply behind it (as
// boxfused::supported_sq): up to six passes, at most 32768 decimated elements per buffer (beyond that rms() looks at
// every step-th element only, src/rtl_fm.c:1090-1092)
inline bool supported_sq(const rtlfm_cfg &c)
{
	if (!pcm_mode(c) || !wants_levels(c)) return false;
	if (c.downsample_passes < 1 || c.downsample_passes > kMaxP) return false;
	return (c.block_len >> c.downsample_passes) <= 32768;
}

}  // namespace fused

namespace boxfused {

// the decimator itself: what both forms of the launch need
inline bool supported_front(const rtlfm_cfg &c)
{
	// at least two outputs per 4096-sample tile: a wave that starts mid-stream takes its first
	// "previous output" from its warm-up tile
	// (downsample == 1, rtl_fm -s 1.2M: low_pass() hands every sample on - 4096 outputs per tile, the same kernel)
	// (beyond /2047 - rtl_fm -s 400 - a tile completes two outputs at most and a mid-stream wave could not warm up on one
	// tile: those runs take ONE wave per stream, launch(); round 6)
	if (c.downsample_passes != 0 || c.downsample < 1) return false;
	if (c.comp_fir_size) return false;
	// -E rdc: any buffer size (round 6: a tile of buffers shorter than itself looks its averages up in a table in LDS);
	// with the rotation the constant sums to zero over every four samples, with offset tuning - no rotation - it adds up
	// linearly: one packed multiply-add per look-up
	return true;  // else any buffer length (a multiple of 512 bytes): the run is one continuous sample stream here
}

// one launch from the bytes to the PCM
inline bool supported(const rtlfm_cfg &c) { return pcm_mode(c) && !wants_levels(c) && supported_front(c); }

// the power squelch / -L with the sums taken by the front end itself (SQ kernels) and k_squelch_apply behind it: one launch
// over the input + a small one over the PCM, no emit mode.  Buffers of at least 8192 samples (a tile's outputs then
// belong to two buffers at most); -M raw keeps the emit mode (the samples themselves are the output).
inline bool supported_sq(const rtlfm_cfg &c)
{
	if (!pcm_mode(c) || !wants_levels(c)) return false;
	if (c.block_len < 16384) return false;
	// rms() looks at every step-th element once a buffer holds more than 32768 of them (src/rtl_fm.c:1090-1092): the sums
	// taken here are over all of them
	if (c.downsample < 1 || 2 * ((int)(c.block_len / 2) / c.downsample + 1) > 32768) return false;
	return supported_front(c);
}

// emit mode: the launch stores the decimated IQ, and the squelch (src/rtl_fm.c:1204-1215), the -L levels
// (:1217-1237) and mode_demod incl. -M raw (:1006-1009, 1256-1259) follow on 1 / D of the data
inline bool supported_emit(const rtlfm_cfg &c) { return supported_front(c) && (c.mode == RTLFM_MODE_RAW || wants_levels(c)); }

}  // namespace boxfused

namespace plan {

// ------------------------------------------------------- the configuration ----

// the first fifth_order pass that is handed a length which is not a multiple of four elements (src/rtl_fm.c:1188-1191),
// or downsample_passes if there is none; buffers are multiples of 512 bytes, so this is pass 8 or 9
inline int first_irregular_pass(const rtlfm_cfg &c)
{
	for (int p = 0; p < c.downsample_passes; p++)
		if ((c.block_len >> p) % 4) return p;
	return c.downsample_passes;
}

// per-block decimated complex samples, or -1 when the boxcar phase makes it vary
inline int dec_per_block(const rtlfm_cfg *c)
{
	int n0 = (int)(c->block_len / 2);
	if (c->downsample_passes > 0) return n0 >> c->downsample_passes;
	if (c->downsample <= 1) return n0;
	return n0 % c->downsample == 0 ? n0 / c->downsample : -1;
}

inline int validate_cfg(const rtlfm_cfg *c)
{
	if (c->mode < RTLFM_MODE_FM || c->mode > RTLFM_MODE_RAW) return -EINVAL;
	if (c->block_len < 512 || c->block_len > RTLFM_MAX_BLOCK_LEN || c->block_len % 512) return -EINVAL;
	if (c->downsample_passes < 0 || c->downsample_passes > RTLFM_MAX_PASSES) return -EINVAL;
	// (a buffer the passes do not divide - nine or ten passes, 512 n bytes with n odd / n % 4 != 0 - is something the
	// reference runs, src/rtl_fm.c:1188-1191: the last passes then see lengths that are not multiples of four elements;
	// k_fifth_irregular, staged_kernels.h)
	if (c->downsample_passes == 0 && c->downsample < 1) return -EINVAL;
	// a buffer shorter than the boxcar leaves low_pass() with lp_len == 0 and fm_demod() then reads
	// lowpassed[-2] (src/rtl_fm.c:955-956): outside the reference's domain
	if (c->downsample_passes == 0 && (uint32_t)c->downsample > c->block_len / 2) return -EDOM;
	if (c->comp_fir_size != 0 && c->comp_fir_size != 9) return -EINVAL;
	if (c->custom_atan < RTLFM_ATAN_STD || c->custom_atan > RTLFM_ATAN_LUT) return -EINVAL;
	if (c->max_blocks < 1) return -EINVAL;
	// a stream's run is counted in int everywhere, on the host and in the kernels: the most a run can hold must fit
	// (16384 buffers of 262144 bytes - 4 GiB per stream and run - is the first that does not)
	if ((long long)c->max_blocks * (c->block_len / 2) > INT32_MAX) return -E2BIG;
	if (c->post_downsample < 1 || c->post_downsample > 16) return -EINVAL;
	if (c->deemph && c->deemph_a < 1) return -EINVAL;
	if (c->mode != RTLFM_MODE_RAW) {
		int per = dec_per_block(c);
		// low_pass_simple: "length must be multiple of step" (src/rtl_fm.c:740); otherwise the
		// reference sums stale samples past result_len.  Behind a boxcar that does not divide the
		// buffer the per-buffer count alternates, so no step > 1 can divide it every time.
		if (c->post_downsample > 1 && (per < 0 || per % c->post_downsample)) return -EDOM;
		if (c->rate_out2 > 0) {
			if (c->rate_out <= 0) return -EINVAL;
			if (c->resampler == RTLFM_RESAMPLE_LOW_PASS_REAL) {
				// the reference divides by zero here (src/rtl_fm.c:769)
				if (c->rate_out / c->rate_out2 == 0) return -EDOM;
			} else if (c->resampler == RTLFM_RESAMPLE_ARBITRARY) {
				// per < 0: the per-buffer count is n or n + 1 (boxcar not dividing the buffer)
				int n = per < 0 ? (int)(c->block_len / 2) / c->downsample : per / c->post_downsample;
				// (a buffer of one sample: both resamplers read b1[1], src/rtl_fm.c:1121, 1148.  len2 == 0 - rate_out2 so small
				// that n * rate_out2 / rate_out truncates to nothing - is a run of no output the reference makes: not refused)
				if (n < 2) return -EINVAL;
			} else {
				return -EINVAL;
			}
		}
	}
	return 0;
}

// ----------------------------------------------------------- the audio tail ----

// Audio tail shared by all routes: everything full_demod() does after mode_demod() (src/rtl_fm.c:1260-1271).
struct TailPlan {
	bool post, deemph, adc, lpr, arb;
	bool deemph_spec;  // deemph_filter alone on a long run: the one-pass kernel, which works OUT of place (k_deemph_spec)
	int oop() const { return (post ? 1 : 0) + (deemph_spec ? 1 : 0) + ((lpr || arb) ? 1 : 0); }
	bool any() const { return post || deemph || adc || lpr || arb; }
};
// the time-parallel forms of deemph_filter apply: a long run, a divisor whose contracted interval fits a wave
// (2 a + 2 <= kDeemphGap, written so that no divisor overflows)
inline bool deemph_scans(const rtlfm_cfg &c, const rtlfm_route_opts &o, int T)
{
	return T >= 2048 && c.deemph_a >= 2 && c.deemph_a <= (kDeemphGap - 2) / 2 && !o.no_deemph_scan && !o.deemph_sequential;
}
// nblocks: the buffers of the run (the plan depends on how long a stream's run is)
inline TailPlan plan_tail(const rtlfm_cfg &c, const rtlfm_route_opts &o, int nblocks)
{
	TailPlan t{};
	if (c.mode == RTLFM_MODE_RAW) return t;
	t.post = c.post_downsample > 1;
	t.deemph = c.deemph != 0;
	t.adc = c.dc_block_audio != 0;
	t.lpr = c.rate_out2 > 0 && c.resampler == RTLFM_RESAMPLE_LOW_PASS_REAL;
	t.arb = c.rate_out2 > 0 && c.resampler == RTLFM_RESAMPLE_ARBITRARY;
	if (t.deemph && !t.lpr && !t.arb && !o.deemph_four_pass) {
		// the demodulated samples of a stream's run, as run_tail() will be told (an upper bound behind a boxcar that does not
		// divide the buffer)
		const long long n0 = c.block_len / 2;
		long long T = c.downsample_passes > 0 ? (long long)nblocks * (n0 >> c.downsample_passes)
		                                      : ((long long)nblocks * n0) / c.downsample + ((n0 % c.downsample) ? 1 : 0);
		if (t.post) T /= c.post_downsample;
		t.deemph_spec = T < (1ll << 30) && deemph_scans(c, o, (int)T);
	}
	return t;
}

// Config 3's own tail (deemph + arbitrary_upsample: 16384 short waves that fill the GPU by themselves, 63 us alone) behind a
// front end of thousands of streams is better off IN LINE, on the front end's stream: beside the next front end it takes
// 1.5 % more of the step than behind this one, and a front end with nothing beside it runs best in few long segments
// (the planner's no-tail target: another 3 %, LAB.md I.31).  A rule of the configuration and the stream count only - a
// handle's tail never changes streams between runs.
inline bool arb_tail_in_line(const rtlfm_cfg &c, const rtlfm_route_opts &o, int nstreams, const TailPlan &tp)
{
	return tp.deemph && tp.arb && !tp.post && !tp.adc && !tp.lpr && c.rate_out2 > c.rate_out &&
	       (o.arb_serial > 0 || (o.arb_serial < 0 && nstreams >= 2048));
}

// ------------------------------------------------------------------ the run ----

// One run's geometry, for the launchers, the gate and k_squelch_apply.  Buffer b of a stream owns the decimated samples
// [dec_block_begin(b), dec_block_begin(b + 1)) of the run - Nblk input samples per buffer through a boxcar D with the
// carried prev_index; behind fifth_order passes (Nblk, 1): a uniform count of Nblk per buffer.
struct RunGeom {
	int N0;         // complex samples per buffer
	int Nblk, D;
	int Tin;        // complex samples of a stream's run
	int T, maxout;  // outputs of a stream's run (varcnt: at most); the most the boxcar can leave (Tin / D + 1)
	bool varcnt;    // the boxcar does not divide a buffer: per-stream counts
	int level;      // passes the fused front end runs itself (six at most)
	int first_irr;  // first_irregular_pass()
};
// (validate_cfg and nblocks <= max_blocks: Tin fits an int)
inline RunGeom run_geometry(const rtlfm_cfg &c, int nblocks)
{
	RunGeom g{};
	g.N0 = (int)(c.block_len / 2);
	g.Tin = nblocks * g.N0;
	g.level = c.downsample_passes < fused::kMaxP ? c.downsample_passes : fused::kMaxP;
	g.first_irr = first_irregular_pass(c);
	if (c.downsample_passes > 0) {
		g.Nblk = g.N0 >> c.downsample_passes;
		g.D = 1;
		g.T = g.maxout = nblocks * g.Nblk;
	} else {
		g.Nblk = g.N0;
		g.D = c.downsample;
		g.maxout = g.Tin / g.D + 1;
		g.varcnt = (g.N0 % g.D) != 0;
		g.T = g.varcnt ? g.maxout : g.Tin / g.D;
	}
	return g;
}

struct RunPlan {
	int route;          // enum rtlfm_route, or a negative errno (nothing is launched)
	int rest;           // enum rtlfm_rest
	bool sq_front;      // the front end takes rms()'s sums (d_sq_sums cleared in front of it, k_squelch_apply behind it)
	bool copy_state;    // the record is copied sin -> sout first: the staged kernels and the channel front ends each update
	                    // their own fields, k_fused and k_boxcar_scan copy it themselves
	bool tail_follows;  // fused::Workspace::tail_follows of the front end's launch
	int last_path;
	TailPlan tp;
	RunGeom g;
};

constexpr rtlfm_route_opts kRouteDefaults = {0, -1, 1, 1, 0, 0, -1, 0, RTLFM_CHANNELS_OFF};

// k_deep_rest takes passes six and up, generic_fir and the demodulator in one launch where the buffers are long against
// the tails it recomputes from the buffer before (staged_kernels.h)
inline bool deep_rest_fits(const rtlfm_cfg &c, const RunGeom &g)
{
	int kk[6];
	deep_rest_tails(c.downsample_passes, c.comp_fir_size == 9, kk);
	const int n6 = g.N0 >> g.level, nF = g.N0 >> c.downsample_passes;
	return n6 >= 2 * kk[0] && nF - kk[c.downsample_passes - g.level] >= 3;
}

// what the staged decimators leave to: the reference's own loops where a pass is handed a length it does not divide
inline int staged_rest(const rtlfm_cfg &c, const RunGeom &g)
{
	return g.first_irr < c.downsample_passes ? RTLFM_REST_IRREGULAR : RTLFM_REST_BACK_HALF;
}

// The plan.  (c: validated; a view of a ragged run plans for its own block_len like any run.)
//
// Why the branches below need no more terms than they have (LAB.md I.53 has the arguments in full):
//  * boxfused::supported_front() implies supported() or supported_emit(): with the decimator itself covered, a PCM mode
//    without levels is supported(), -M raw or levels are supported_emit().  So BOXCAR_EMIT is reached exactly under -M raw
//    or where the SQ form declines levels (squelch_fused = 0, buffers below 16384 bytes, more than 32768 elements a
//    buffer), and the order of the two tests is the whole rule.
//  * fused::supported() and fused::supported_emit() exclude each other (a PCM mode without levels and at most six passes
//    against more passes, -M raw or levels), and the SQ form implies levels: FUSED comes first and takes the SQ form or
//    supported(), FUSED_EMIT what is left of supported_emit().  Both need the engine.
//  * The 16-byte rule is the planner's alone: k_fused writes the caller's rows only where the tail has no out-of-place
//    stage; else it writes res[], whose rows are 128-byte multiples apart in an allocation of the runtime's.  fused::launch
//    keeps its own test of the rows it is handed, and its own engine tests, as defences that never fire.
//  * path == 2 is refused exactly where last_path would be 1 - one rule for channels and everything else.
//  * The state copy is made exactly where the front end does not copy the record itself: STAGED and every channel route.
inline RunPlan plan_run(const rtlfm_cfg &c, int nstreams, int nblocks, const rtlfm_route_opts &o, unsigned out_low_bits, size_t out_stride)
{
	RunPlan p{};
	p.g = run_geometry(c, nblocks);
	p.tp = plan_tail(c, o, nblocks);
	const RunGeom &g = p.g;
	const bool levels = wants_levels(c);
	const bool raw_plain = c.mode == RTLFM_MODE_RAW && !levels;      // what the front end emits IS the output (raw_demod() copies lowpassed[])
	const bool rows16 = !(out_low_bits & 15) && !(out_stride & 7);  // the caller's rows take 16-byte stores
	const bool one_launch = o.path != 1;                             // rtlfm_gpu_set_path(1): the staged kernels, the cross-checks
	// the raw DC block rides on the MFMA pass 0, and only that engine has the partial-tile kernels (-W n)
	const bool engine_ok = !((c.dc_block_raw || fused::needs_partial_tiles(c)) && fused::effective_engine(o.pass0_engine) != 1);
	// k_fused stores 16-byte vectors: into res[] where the tail has an out-of-place stage, else straight into the caller's rows
	const bool pcm_rows_ok = p.tp.oop() > 0 || rows16;
	const bool fuse_sq = o.squelch_fused && fused::supported_sq(c);

	p.last_path = 2;
	if (o.channels != RTLFM_CHANNELS_OFF) {
		// Channels on: the boxcar, the filter and the bank have a one-launch front end each; every other decimator runs staged
		// behind k_channel_mix.  (All leave the other fields of the record to the copy, as the staged kernels always do.)
		// (a filter or a bank is only ever set on a handle without fifth_order passes: with one, both paths are its own)
		const bool boxed = one_launch && c.downsample_passes == 0;
		p.copy_state = true;
		if (!boxed) p.last_path = 1;
		if (o.channels == RTLFM_CHANNELS_BANK) p.route = boxed ? RTLFM_ROUTE_CHAN_BANK : RTLFM_ROUTE_CHAN_BANK_PLAIN;
		else if (o.channels == RTLFM_CHANNELS_FILTER) p.route = boxed ? RTLFM_ROUTE_CHAN_FIR : RTLFM_ROUTE_CHAN_FIR_PLAIN;
		else p.route = boxed ? RTLFM_ROUTE_CHAN_BOXCAR : RTLFM_ROUTE_CHAN_MIX;
		// -M raw without the squelch behind k_channel_boxcar: what the launch leaves IS the output and goes straight into the
		// caller's rows where a row has one spare dword behind its last possible output (channel_kernel.h)
		if (p.route == RTLFM_ROUTE_CHAN_MIX) p.rest = staged_rest(c, g);
		else p.rest = p.route == RTLFM_ROUTE_CHAN_BOXCAR && raw_plain && out_stride / 2 >= (size_t)g.Tin / g.D + 2 ? RTLFM_REST_NONE
		                                                                                                           : RTLFM_REST_BACK_HALF;
	} else if (one_launch && (boxfused::supported(c) || (o.squelch_fused && boxfused::supported_sq(c)))) {
		p.route = RTLFM_ROUTE_BOXCAR;
		p.rest = RTLFM_REST_TAIL;
		p.sq_front = levels;
		p.tail_follows = p.tp.any() || levels;
	} else if (one_launch && boxfused::supported_emit(c)) {
		p.route = RTLFM_ROUTE_BOXCAR_EMIT;
		p.rest = raw_plain ? RTLFM_REST_NONE : RTLFM_REST_BACK_HALF;  // (the launch's rows: one dword a sample, any alignment)
		p.tail_follows = !raw_plain;  // kernels follow on this stream and, with a tail, on the tail's
	} else if (one_launch && engine_ok && pcm_rows_ok && (fuse_sq || fused::supported(c))) {
		// the squelch / -L with rms()'s sums taken by the front end itself comes before the emit mode (supported() itself
		// never competes with it: see above)
		p.route = RTLFM_ROUTE_FUSED;
		p.rest = RTLFM_REST_TAIL;
		p.sq_front = levels;
		// (a tail in line leaves the next front end alone: the plan of a front end that nothing runs beside)
		p.tail_follows = (p.tp.any() && !arb_tail_in_line(c, o, nstreams, p.tp)) || levels;
	} else if (one_launch && engine_ok && fused::supported_emit(c)) {
		// With up to six passes k_fused emits the decimated, FIR-compensated IQ (what full_demod() hands on after
		// src/rtl_fm.c:1202); with 7..10 passes the /64 IQ, and what follows runs the remaining passes and the FIR on 1/64 of
		// the data.
		p.route = RTLFM_ROUTE_FUSED_EMIT;
		const bool deep = c.downsample_passes > g.level;
		if (raw_plain && !deep && rows16) p.rest = RTLFM_REST_NONE;  // straight into the caller's rows where they take 16-byte stores
		else if (deep && g.first_irr >= c.downsample_passes && o.deep_rest && deep_rest_fits(c, g))
			p.rest = levels || c.mode == RTLFM_MODE_RAW ? RTLFM_REST_DEEP_IQ : RTLFM_REST_DEEP_DEMOD;
		else if (g.first_irr < c.downsample_passes) p.rest = RTLFM_REST_IRREGULAR;  // nine or ten passes on buffers they do not divide
		else p.rest = deep ? RTLFM_REST_PER_PASS : RTLFM_REST_BACK_HALF;
		p.tail_follows = p.rest != RTLFM_REST_NONE;
	} else {
		p.route = RTLFM_ROUTE_STAGED;
		p.rest = staged_rest(c, g);
		p.copy_state = true;
		p.last_path = 1;
	}
	if (o.path == 2 && p.last_path == 1) p.route = -ENOTSUP;  // rtlfm_gpu_set_path(2): no fused form for this run
	return p;
}

// rtlfm_run_route() (include/rtlfm_hip.h): the arguments as rtlfm_gpu_run_device and the setters judge them, then the plan
inline int run_route(const rtlfm_cfg *cfg, int nstreams, int nblocks, unsigned out_low_bits, size_t out_stride, const rtlfm_route_opts *opts,
                     rtlfm_route_plan *out)
{
	if (!cfg) return -EINVAL;
	int v = validate_cfg(cfg);
	if (v < 0) return v;
	const rtlfm_route_opts &o = opts ? *opts : kRouteDefaults;
	if (nstreams < 1 || nblocks < 1 || (out_low_bits & 3) || (out_stride & 1)) return -EINVAL;
	if (nblocks > cfg->max_blocks) return -E2BIG;
	if (o.path < 0 || o.path > 2 || o.pass0_engine < -1 || o.pass0_engine > 1 || o.arb_serial < -1 || o.arb_serial > 1) return -EINVAL;
	if (o.channels < RTLFM_CHANNELS_OFF || o.channels > RTLFM_CHANNELS_BANK) return -EINVAL;
	// what the channel setters refuse: -E rdc with channels; a filter or a bank in front of fifth_order passes
	if (o.channels != RTLFM_CHANNELS_OFF && cfg->dc_block_raw) return -ENOTSUP;
	if (o.channels >= RTLFM_CHANNELS_FILTER && cfg->downsample_passes > 0) return -ENOTSUP;
	const RunPlan p = plan_run(*cfg, nstreams, nblocks, o, out_low_bits, out_stride);
	if (p.route < 0) return p.route;
	if (out) {
		const TailPlan &t = p.tp;
		const RunGeom &g = p.g;
		*out = rtlfm_route_plan{p.route, p.rest, p.last_path, p.sq_front, p.copy_state, p.tail_follows,
		                        (t.post ? 1 : 0) | (t.deemph ? 2 : 0) | (t.adc ? 4 : 0) | (t.lpr ? 8 : 0) | (t.arb ? 16 : 0) | (t.deemph_spec ? 32 : 0),
		                        g.N0, g.Nblk, g.D, g.T, g.varcnt, g.level, g.first_irr};
	}
	return p.route;
}

}  // namespace plan
}  // namespace rtlfm
