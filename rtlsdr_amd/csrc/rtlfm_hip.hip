// rtlfm_hip.hip — the C ABI of include/rtlfm_hip.h on HIP / gfx950.
//
// Host side: handle, HBM buffers, stage sequencing that reproduces the order
// of full_demod() (reference src/rtl_fm.c:1179-1272) behind the
// rtlsdr_read_async callback boundary (include/rtl-sdr.h:472-492).
// There is deliberately no CPU fallback anywhere in this file.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "../../include/rtlfm_hip.h"
#include "device_own.h"
#include "debug_poison.h"
#include "stream_pool.h"
#include "run_plan.h"
#include "staged_kernels.h"
#include "fused_kernel.h"
#include "boxcar_kernel.h"
#include "input_stats_kernel.h"
#include "input_health_kernel.h"
#include "source_prepass_kernel.h"
#include "source_iq_kernel.h"
#include "scan_kernel.h"
#include "pack_kernel.h"
#include "state_kernel.h"
#include "channel_kernel.h"
#include "channel_fir_kernel.h"
#include "channel_bank_kernel.h"
#include "../../include/rtlfm_snapshot.h"
#include "../../include/rtlfm_chansnap.h"

using namespace rtlfm;
using namespace rtlfm::plan;

#define HIP_TRY(expr)                                                              \
	do {                                                                           \
		hipError_t e_ = (expr);                                                    \
		if (e_ != hipSuccess) {                                                    \
			fprintf(stderr, "rtlfm_hip: %s -> %s (%s:%d)\n", #expr,                \
			        hipGetErrorString(e_), __FILE__, __LINE__);                    \
			return e_ == hipErrorOutOfMemory ? -ENOMEM : -EIO;                     \
		}                                                                          \
	} while (0)

struct rtlfm_gpu {
	rtlfm_cfg cfg;
	int nstreams = 0;
	int device = 0;
	hipStream_t own_stream = nullptr;
	hipStream_t stream = nullptr;
	Event ev_wait, ev_release;  // rtlfm_gpu_wait_for / _release_to
	int path = kRouteDefaults.path, last_path = 0;
	int last_route = 0, last_rest = 0;  // options "last_route" / "last_rest" (read-only): the plan the last run took (run_plan.h)

	// geometry
	size_t xstride = 0;   // dwords per stream in a work buffer
	size_t rstride = 0;   // int16 per stream in a result buffer
	int cap_blocks = 0;

	// device memory
	DevBuf<uint32_t> bufA, bufB;
	// demodulated samples on their way through the audio tail: [step parity][ping / pong], tstride
	// int16 per stream.  Two sets, because the tail of step k runs on its own stream while the front
	// end of step k + 1 already fills the other set.
	DevBuf<int16_t> res[2][2];  // (placed: res[0][0] owns ONE block for both parities and res[1][0] is an alias into it)
	size_t tstride = 0;
	DevBuf<int32_t> d_cnt[2], d_cnt2;  // d_cnt: per step parity
	DevBuf<DeemphChunk> d_deemph_tab;  // time-parallel deemph (k_deemph_scan_*): [nstreams][chunks]
	DevBuf<uint32_t> d_deemph_inc;
	DevBuf<LprChunk> d_lpr_chunks;     // low_pass_real folded into the replay pass: [nstreams][chunks]
	DevBuf<int32_t> d_arb_i;              // k_deemph_spec_arb: (i, frac) of every output of a buffer, [arb_len2]
	DevBuf<double> d_arb_frac;
	int arb_len2 = 0, arb_len1 = 0;
	DevBuf<uint32_t> deepA, deepB;  // /64 IQ work buffers of the 7..10-pass path
	size_t deep_stride = 0;
	// Carried state, three copies in rotation: step k reads st[cur] and writes st[(cur + 1) % 3].
	// The tail of step k (own stream) still reads st[cur] / writes the tail's fields of the next copy
	// while the front end of step k + 1 reads that copy and writes the third one.
	DevBuf<state_t> st[3];
	int st_cur = 0;
	unsigned step = 0;                      // parity selects res[] / d_cnt[] / the events
	hipStream_t tail_stream = nullptr;
	int tail_priority = 0;
	int tail_prio_value = 0;                // the HIP priority tail_stream was taken from the pool with
	Event ev_front[2], ev_tail[2];
	bool tail_pending[2] = {false, false};  // ev_tail[p] has been recorded and not yet waited for
	bool tail_overlap = true;
	bool tail_serial_asked = false;         // option tail_serial: never overlap, whatever the stream
	DevBuf<int32_t> d_lut;
	DevBuf<int32_t> d_mute;           // [nstreams*cap_blocks]
	DevBuf<int32_t> d_levels;         // [nstreams*cap_blocks] rms() per buffer of the last run
	int last_nblocks = 0;
	DevBuf<rtlfm_input_stat> d_istats;     // [nstreams*cap_blocks] ADC statistics of the raw bytes (option input_stats), allocated on first use
	int stats_nblocks = 0;                 // buffers of the last run that have records ([stream][stats_nblocks])
	DevBuf<rtlfm_input_health> d_ihealth;  // the same for option input_health
	int health_nblocks = 0;
	// scanning (scan_kernel.h): the gate's records of the last run, allocated on first use, and the hop mute's counts
	DevBuf<rtlfm_gate_rec> d_gate;    // [nstreams*cap_blocks]
	int gate_nblocks = 0;
	size_t gate_rec_off = 0;               // stream-range views (ragged runs) write buffer j of the run: [stream][gate_rec_stride] + j
	int gate_rec_stride = 0;               // 0: the run's own buffer count
	std::shared_ptr<uint32_t[]> mute_left; // host, [nstreams]: bytes rtlfm_gpu_mute still owes each stream; allocated by the first call (a view's copy shares it)
	int mute_streams = 0;                  // streams with a count pending
	DevBuf<scan::MuteEntry> d_mute_entries;
	DevBuf<int32_t> d_move_map;            // [nstreams]: rtlfm_gpu_state_move's map on the device, allocated by the first move into this handle
	// channels (channel_kernel.h; rtlfm_gpu_set_channels): stream s = channel s % chan_per of source s / chan_per
	int chan_per = 0;                      // 0: off
	uint64_t chan_pos = 0;                 // complex samples consumed since set_channels / reset / seek: ONE counter, the streams run in lockstep
	DevBuf<uint32_t> d_chan_steps;         // [nstreams]
	DevBuf<uint32_t> d_chan_table;         // [channel::kTableSize], uploaded by the first set_channels
	DevBuf<uint32_t> chan_iq;              // what a channel front end leaves for the back half: [nstreams][chan_stride] decimated IQ
	size_t chan_stride = 0;
	// the source history of the filter and the bank (channel_kernel.h, kHist): [src_hist_srcs][channel::kHist * 2] raw bytes,
	// every SOURCE's last samples; a run reads [src_hist_cur] and writes the other
	DevBuf<uint8_t> d_src_hist[2];
	int src_hist_cur = 0, src_hist_srcs = 0;
	// option source_dc (channel_kernel.h, k_source_dc_smooth): allocated when the option is first set, for as many sources as
	// there are streams.  The history's biases change over with d_src_hist.
	DevBuf<long long> d_sdc_sums;          // [sources][cap_blocks][2] k_rdc_sums_wide's, by source
	DevBuf<uint32_t> d_sdc;                // [sources][sdc_stride] a run's list of biases: the history's pieces, then the run's
	size_t sdc_stride = 0;
	DevBuf<uint32_t> d_sdc_hist[2];        // [sources][channel::kDcHist]
	// options source_stats / source_health: the readers' records per (SOURCE, buffer) of a run that channels take, allocated
	// on first use for the sources there are then and regrown when rtlfm_gpu_set_channels makes them more
	DevBuf<rtlfm_input_stat> d_src_stats;      // [sources][cap_blocks]
	DevBuf<rtlfm_input_health> d_src_health;
	int src_stats_nblocks = 0, src_health_nblocks = 0;  // buffers of the last run that have records; 0: that run left none
	size_t src_rec_off = 0;                    // a view (run_ragged) files buffer j of the run: [source][src_rec_stride] + j
	int src_rec_stride = 0;                    // 0: the run's own buffer count
	// option source_iq (source_iq_kernel.h): the corrected source rows every front end reads in the caller's place and the
	// records of the raw bytes, allocated by the first run that needs them, regrown with the sources, freed with the option;
	// the coefficients, identity on a fresh handle and after rtlfm_gpu_set_channels, for as many sources as there are streams
	DevBuf<uint8_t> d_siq_rows;                // [sources][siq_stride]
	size_t siq_stride = 0;                     // cap_blocks * cfg.block_len of the HANDLE (a view keeps it)
	DevBuf<rtlfm_iq_sums> d_siq_sums;          // [sources][cap_blocks], filed as the records above
	int siq_nblocks = 0;                       // buffers of the last run that have records; 0: that run left none
	std::vector<int16_t> siq_coef;             // [nstreams][4], what the getter hands back
	DevBuf<int16_t> d_siq_coef;
	static constexpr int kIqStages = 4;        // rtlfm_gpu_set_source_iq's rotation, as the bins'
	PinnedBuf<int16_t> h_siq_stage[kIqStages];
	Event ev_siq_stage[kIqStages];
	int siq_stage_next = 0;
	// the channel filter (channel_fir_kernel.h; rtlfm_gpu_set_channel_filter): acts while channels are on
	int fir_ntaps = 0, fir_shift = 0;      // 0 taps: none, the boxcar
	std::vector<int16_t> fir_taps;         // what the getter hands back
	DevBuf<int16_t> d_fir_taps;            // [ntaps], k_channel_fir_plain's
	DevBuf<uint32_t> d_fir_taps8;          // chanfir::shifted_taps(), k_channel_fir's
	DevBuf<uint32_t> chan_fir_x;           // path 1: k_channel_mix's samples of the history's end and the run, [nstreams][chan_fir_xstride]
	size_t chan_fir_xstride = 0;
	// the channel bank (channel_bank_kernel.h; rtlfm_gpu_set_channel_bank): while on it takes the mixer paths' place
	int bank_m = 0, bank_K = 0, bank_ntaps = 0, bank_shift = 0;  // K == 0: none
	std::vector<int16_t> bank_taps;        // what the getter hands back
	std::vector<int32_t> bank_bins;        // [chan_per]
	DevBuf<int16_t> d_bank_taps;           // [ntaps], k_bank_sums'
	DevBuf<uint32_t> d_bank_taps2;         // chanbank::branch_taps(), k_channel_bank's
	DevBuf<uint32_t> d_bank_tw;            // [K] twiddles per stage, doubled and packed
	DevBuf<int16_t> d_bank_sine;           // [3 K / 4] sine_table(m), k_bank_fft's
	DevBuf<int32_t> d_bank_bins;           // [chan_per]
	DevBuf<uint32_t> bank_v;               // path 1: [sources][maxout][K] sums, transformed in place
	// per-source bins (rtlfm_gpu_set_channel_bins): while set they rule in d_bank_bins' place, chan_per apart per source.
	// The setter copies through a rotation of pinned buffers on the handle's stream and waits for nothing but a buffer
	// whose own copy, kBinStages calls ago, has not left yet.
	static constexpr int kBinStages = 4;
	std::vector<int32_t> bank_bins_ps;     // [sources][chan_per]; empty: the shared list
	DevBuf<int32_t> d_bank_bins_ps;
	PinnedBuf<int32_t> h_bins_stage[kBinStages];
	Event ev_bins_stage[kBinStages];
	int bins_stage_next = 0;
	// the survey (option bank_survey; rtlfm_gpu_bank_survey): two sets in rotation, as the ring's halves rotate - a surveyed
	// run writes the set the last surveyed run did not; allocated by the first surveyed run
	struct Survey {
		DevBuf<unsigned long long> d_power[2];                // [sources][K]
		DevBuf<int32_t> d_frames[2];                          // [sources]
		Event ev[2];                                          // behind the set's last launch
		int cap_srcs = 0;
		DevBuf<unsigned long long> d_partial;                 // k_channel_bank_survey's: [sources][segs][K]
		int K[2] = {0, 0}, nsrc[2] = {0, 0};                  // what the set holds
		int last = -1, prev = -1;                             // the set of the last run and of the run before it; -1: that run carried none
		int writing = -1;                                     // the set the run being launched writes
		int next = 0;
	} sv;
	DevBuf<long long> d_sums;         // [nstreams*cap_blocks*2]  dc_block_raw (front end's stream)
	DevBuf<long long> d_adc_sums;     // [nstreams*cap_blocks]    dc_block_audio (the tail's stream)
	DevBuf<uint32_t> d_sq_sums;       // [nstreams*cap_blocks*2]  rms()'s sums taken by the boxcar front end (SQ kernels)
	DevBuf<int2> d_rdc_avg;           // [nstreams*cap_blocks]
	struct Ingest *ing = nullptr;     // the callback side (push / run / fetch), allocated on first use
	bool no_deemph_scan = false;      // stream-range views (ragged runs) keep to the sequential filter
	// placement of the write streams (rtlfm_gpu_malloc_apart_ex): what the searches found and what they cost
	struct Placement {
		int budget_gb = 16;             // option apart_budget_gb: most a search may hold in candidates; 0 = no search
		int force_retry = 0;            // option ring_force_retry (tests): the ring's first search counts as failed
		int ring_tries = 0;             // searches the ring's placement took (2: the device inputs were moved once)
		int ring_apart = -1;            // -1: not allocated yet; 0 / 1: the ring's result buffers (both halves) are a quarter away from d_in
		int res_apart = -1;             // the same for the audio tail's work buffers against the first run's input
		int deep_apart = -1;            // ... and for what a front end's emit mode writes (deepA)
		double search_ms = 0;           // wall time of all searches of this handle
		size_t walked_peak = 0;         // most a search held in temporary allocations (bytes)
	} place;
	fused::Workspace fws;
	// A/B switches (rtlfm_gpu_set_option); none of them changes a result.  (Those that steer a run's plan start at
	// kRouteDefaults' values, run_plan.h: rtlfm_run_route without options plans as a fresh handle runs.)
	struct Options {
		int deemph_sequential = kRouteDefaults.deemph_sequential, deemph_four_pass = kRouteDefaults.deemph_four_pass, lpr_separate = 0, lpr_scalar_stores = 0, tail_sync = 0;
		int lpr_chunk = 5440;  // samples per lane of the one-pass deemph + low_pass_real kernel (round 5: 2720 -> 5440 with the outputs leaving through LDS)
		int deep_rest = kRouteDefaults.deep_rest;  // 0: the passes beyond six, generic_fir and the demodulator as a launch each (round 4) instead of k_deep_rest
		int squelch_fused = kRouteDefaults.squelch_fused;  // 0: the squelch / -L behind the boxcar through the emit mode and k_squelch_rms / _hits / _zero / k_fm_demod (round 4) also where the front end can take rms()'s sums itself
		int lpr_ring = 1;      // 0: the one-pass deemph + low_pass_real kernel's outputs leave in 16-byte groups from registers (round 3) instead of 64-byte pieces from LDS
		int arb_serial = kRouteDefaults.arb_serial;  // deemph + arbitrary_upsample behind the front end on ITS stream: -1 = from 2048 streams on, 0 never, 1 always
		int lpr_threads = 256; // lanes per workgroup of k_deemph_spec_lpr: 64, 128, 192 or 256
		int arb_waves = 0;     // waves per stream of k_deemph_spec_arb: 0 = about 16384 waves in all, else 1 .. 8
		int verify_inject = 0; // tests: the shadow execution's first sample of stream 0 is overwritten before the comparison (it must be noticed)
		int input_stats = 0;   // 1: k_input_stats in front of every run's front end (rtlfm_gpu_input_stats)
		int input_stats_nt = 1; // its loads non-temporal (the A/B of LAB.md)
		int input_health = 0;  // 1: k_input_health in front of every run's front end (rtlfm_gpu_input_health)
		int squelch_gate = 0;  // 1: k_scan_gate at the end of every run (rtlfm_gpu_gate)
		int conseq_squelch = 10;  // demod_init(), src/rtl_fm.c:1613
		int verify_twice = 0;  // debug: every run_device runs twice - into a shadow output, then into the caller's - and the two are compared on the device
		int source_ring = 0;   // 1: while channels are on the ring's input side has one row per SOURCE (ring_rows) and the ring calls are open
		int pack_results = 0;  // 1 / 2: every ring run ends with k_pack_plan + k_pack_copy (pack_kernel.h; rtlfm_gpu_fetch_packed)
		int bank_survey = 0;   // 1: a run the bank takes leaves every bin's power as well (k_channel_bank_survey; rtlfm_gpu_bank_survey)
		int source_dc = 0;     // 1: runs that channels take subtract every source's smoothed buffer averages in front of the front end (k_source_dc_smooth)
		int source_stats = 0;  // 1: runs that channels take leave the ADC statistics of every source's raw bytes (rtlfm_gpu_source_stats)
		int source_health = 0; // 1: ... and the health records (rtlfm_gpu_source_health)
		int source_iq = 0;     // 1: runs that channels take rewrite every source's bytes with its IQ-balance coefficients first (k_source_iq)
	} opt;
	// verify_twice (round 6): shadow rows / lengths / state, and what the comparisons found so far
	DevBuf<int16_t> vt_out;
	DevBuf<int32_t> vt_len, vt_len2;
	DevBuf<state_t> vt_state;
	DevBuf<rtlfm_gate_rec> vt_gate;        // the first execution's gate records
	DevBuf<unsigned long long> vt_cnt;     // [4]: differing PCM dwords, differing lengths, differing state dwords, first differing (stream << 32 | index) + 1
	long vt_mismatches = 0, vt_runs = 0;

	// timing of the decimating front end
	bool timing = false;
	std::vector<std::pair<Event, Event>> ev_pending;
	std::vector<std::pair<Event, Event>> ev_free;
};

// ------------------------------------------------------------ host planner ----

extern "C" void rtlfm_cfg_default(rtlfm_cfg *c)
{
	// demod_init(), src/rtl_fm.c:1608-1640
	memset(c, 0, sizeof(*c));
	c->mode = RTLFM_MODE_FM;
	c->downsample = 1;
	c->post_downsample = 1;
	c->rate_out = 24000;
	c->rate_out2 = -1;
	c->adc_block_const = 9;
	c->rdc_block_const = 9;
	c->output_scale = 1;
	c->block_len = 16384;  // dongle_init(), src/rtl_fm.c:1605
	c->max_blocks = 1;
}

extern "C" int rtlfm_optimal_settings(rtlfm_cfg *cfg, uint32_t freq, int32_t rate_in,
                                      int32_t min_capture_rate, int use_fifth_order, int edge,
                                      uint32_t *capture_freq, uint32_t *capture_rate)
{
	// optimal_settings(), src/rtl_fm.c:1407-1445
	if (!cfg || rate_in <= 0) return -EINVAL;
	cfg->downsample = min_capture_rate / rate_in + 1;
	cfg->downsample_passes = 0;
	if (use_fifth_order) {
		cfg->downsample_passes = (int)log2((double)cfg->downsample) + 1;
		cfg->downsample = 1 << cfg->downsample_passes;
	}
	uint32_t rate = (uint32_t)cfg->downsample * (uint32_t)rate_in;
	uint32_t f = freq;
	if (!cfg->offset_tuning) f = freq - rate / 4;
	f += (uint32_t)(edge * rate_in / 2);
	cfg->output_scale = (1 << 15) / (128 * cfg->downsample);
	if (cfg->output_scale < 1) cfg->output_scale = 1;
	if (cfg->mode == RTLFM_MODE_FM) cfg->output_scale = 1;
	if (capture_freq) *capture_freq = f;
	if (capture_rate) *capture_rate = rate;
	return 0;
}

extern "C" int32_t rtlfm_deemph_a(int32_t rate_out, int32_t tc_us)
{
	// src/rtl_fm.c:1929-1931
	double tc = (double)tc_us * 1e-6;
	return (int32_t)round(1.0 / (1.0 - exp(-1.0 / (rate_out * tc))));
}

// (first_irregular_pass, dec_per_block, validate_cfg: run_plan.h)

extern "C" int rtlfm_result_len(const rtlfm_cfg *c)
{
	if (!c) return -EINVAL;
	int n = dec_per_block(c);
	if (n < 0) return -1;
	if (c->mode == RTLFM_MODE_RAW) return c->downsample_passes > 0 ? (int)(c->block_len >> c->downsample_passes) : 2 * n;
	if (c->post_downsample > 1) n /= c->post_downsample;
	if (c->rate_out2 > 0) {
		if (c->resampler == RTLFM_RESAMPLE_ARBITRARY)
			return (int)((long long)n * c->rate_out2 / c->rate_out);
		return -1;
	}
	return n;
}

extern "C" int rtlfm_result_cap(const rtlfm_cfg *c)
{
	if (!c) return -EINVAL;
	int n0 = (int)(c->block_len / 2);
	int n = c->downsample_passes > 0 ? n0 >> c->downsample_passes
	                                  : (c->downsample > 1 ? n0 / c->downsample + 1 : n0);
	if (c->mode == RTLFM_MODE_RAW) return 2 * n + 1;
	if (c->rate_out2 > 0 && c->resampler == RTLFM_RESAMPLE_ARBITRARY && c->rate_out > 0) {
		long long up = (long long)n * c->rate_out2 / c->rate_out + 2;
		if (up > n) n = (int)up;
	}
	return n + 2;
}

extern "C" int rtlfm_cfg_validate(const rtlfm_cfg *cfg) { return cfg ? validate_cfg(cfg) : -EINVAL; }

// ----------------------------------------------------------------- handle ----

static void init_states_host(std::vector<state_t> &v)
{
	for (auto &s : v) {
		memset(&s, 0, sizeof(s));
		s.squelch_hits = 11;  // demod_init(), src/rtl_fm.c:1615
	}
}

static int create_body(rtlfm_gpu *h);
static int options_from_env(rtlfm_gpu *h);
static long placement_held_mb(rtlfm_gpu *h);
static void ingest_destroy(rtlfm_gpu *h);
static void ingest_reset(rtlfm_gpu *h);
static bool ingest_busy(rtlfm_gpu *h);
static bool ingest_queued(rtlfm_gpu *h);
static int ingest_resize(rtlfm_gpu *h);
static int ingest_pack_free(rtlfm_gpu *h);
static int ingest_pack_us(rtlfm_gpu *h, long *us);
static int survey_free(rtlfm_gpu *h, bool wait);

// Rows of the ring's input side (h_stage, d_in, h_len, pushed, open_slot): one per stream - or, with option source_ring
// and channels on, one per source.  The result side is per stream whatever this says.
static inline int ring_rows(const rtlfm_gpu *h)
{
	return h->opt.source_ring && h->chan_per > 0 ? h->nstreams / h->chan_per : h->nstreams;
}

// everything the handle has launched: the front end's stream, then the audio tail's
static hipError_t sync_all(rtlfm_gpu *h)
{
	hipError_t e = hipStreamSynchronize(h->stream);
	if (e != hipSuccess) return e;
	return h->tail_stream ? hipStreamSynchronize(h->tail_stream) : hipSuccess;
}

extern "C" int rtlfm_gpu_create(const rtlfm_cfg *cfg, int nstreams, int device, rtlfm_gpu **out)
{
	if (!cfg || !out || nstreams < 1) return -EINVAL;
	int v = validate_cfg(cfg);
	if (v < 0) return v;
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
		fprintf(stderr, "rtlfm_hip: no usable HIP device (count=%d, asked %d); there is no CPU fallback\n",
		        ndev, device);
		return -ENODEV;
	}
	HIP_TRY(hipSetDevice(device));
	rtlfm_gpu *h = new rtlfm_gpu();
	h->cfg = *cfg;
	h->nstreams = nstreams;
	h->device = device;
	// every failure below releases what was allocated so far (a service retrying on -ENOMEM must
	// not leak device memory); *out is written on success only
	int r = create_body(h);
	if (r < 0) {
		rtlfm_gpu_destroy(h);
		return r;
	}
	*out = h;
	return 0;
}

static int create_body(rtlfm_gpu *h)
{
	const rtlfm_cfg *cfg = &h->cfg;
	const int nstreams = h->nstreams;
	h->cap_blocks = cfg->max_blocks;
	const size_t L = cfg->block_len;
	h->xstride = (size_t)h->cap_blocks * (L / 2) + 16;
	size_t rs = (size_t)h->cap_blocks * L + 64;  // raw mode: 2 int16 per complex sample
	if (cfg->rate_out2 > 0 && cfg->resampler == RTLFM_RESAMPLE_ARBITRARY && cfg->rate_out2 > cfg->rate_out)
		rs = (size_t)((double)rs * cfg->rate_out2 / cfg->rate_out) + 64;
	h->rstride = (rs + 7) & ~(size_t)7;
	HIP_TRY(rtl_pool::stream_get(h->device, 0, &h->own_stream));  // (from the process-wide pool: stream_pool.h)
	h->stream = h->own_stream;
	const size_t S = (size_t)nstreams;
	for (int k = 0; k < 3; k++) OWN_TRY(h->st[k].alloc(S));
	for (int k = 0; k < 2; k++) {
		OWN_TRY(h->d_cnt[k].alloc(S));
		OWN_TRY(h->ev_front[k].create(hipEventDisableTiming));
		OWN_TRY(h->ev_tail[k].create(hipEventDisableTiming));
	}
	// (default priority: the highest and the lowest one were both tried - round 3: highest 1 % slower; round 4,
	// three alternations on one box: c3 0.883 / 0.881 / 0.883 ms, wbfm 1.381 / 1.381 / 1.379 for default / lowest /
	// highest - the dispatcher does not seem to look at it between two compute queues)
	// Round 5: the LOWEST priority, and not for the dispatcher's sake: HIP maps the streams of one priority onto four
	// hardware queues in turn, and in a process that has created one or two other streams the tail's stream and the front
	// end's came to share one - the tail then runs behind the next front end instead of beside it (-M wbfm 1.31 -> 1.47 ms;
	// tools/queue_share_probe.py, profiles/r05_queue_share.txt).  A stream of another priority takes its queue from another pool.
	{
		int lo = 0, hi = 0;
		HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
		HIP_TRY(rtl_pool::stream_get(h->device, lo, &h->tail_stream));
		h->tail_priority = -1;
		h->tail_prio_value = lo;
	}
	h->tail_overlap = true;
	{
		// what mode_demod() can leave per stream and run: the decimated count (+1 per buffer behind a
		// boxcar that does not divide it); every later stage but the last one only shrinks it
		const size_t n0 = L / 2;
		const size_t per = cfg->downsample_passes > 0 ? n0 >> cfg->downsample_passes
		                                              : (cfg->downsample > 1 ? n0 / cfg->downsample + 1 : n0);
		h->tstride = ((size_t)h->cap_blocks * per + 64 + 63) & ~(size_t)63;
	}
	OWN_TRY(h->d_cnt2.alloc(S));
	OWN_TRY(h->d_mute.alloc(S * h->cap_blocks));
	OWN_TRY(h->d_levels.alloc(S * h->cap_blocks));
	OWN_TRY(h->d_sums.alloc(S * h->cap_blocks * 2));
	OWN_TRY(h->d_adc_sums.alloc(S * h->cap_blocks));
	OWN_TRY(h->d_rdc_avg.alloc(S * h->cap_blocks + 32));  // (+ slack: k_boxcar_scan reads kRdcMany entries from a tile's first buffer on)
	OWN_TRY(h->d_sq_sums.alloc(S * h->cap_blocks * 2));
	if (cfg->custom_atan == RTLFM_ATAN_LUT) {
		// atan_lut_init(), src/rtl_fm.c:881-892 — built with the host libm, as
		// the reference builds it
		std::vector<int32_t> lut(131072);
		for (int i = 0; i < 131072; i++)
			lut[i] = (int32_t)(atan((double)i / 256.0) / 3.14159 * 16384.0);
		OWN_TRY(h->d_lut.alloc(lut.size()));
		HIP_TRY(hipMemcpy(h->d_lut, lut.data(), lut.size() * sizeof(int32_t), hipMemcpyHostToDevice));
	}
	int r = options_from_env(h);
	if (r < 0) return r;
	return rtlfm_gpu_reset(h);
}

static int ensure_work_buffers(rtlfm_gpu *h)
{
	const size_t S = (size_t)h->nstreams;
	OWN_TRY(h->bufA.alloc(S * h->xstride));
	return h->bufB.alloc(S * h->xstride);
}
// the decimated IQ a front end in emit mode leaves for the staged kernels: /2^level behind fifth_order passes
// (run_fused_emit), 1 / D (+ 1 per buffer) behind the boxcar (run_boxfused_emit)
extern "C" int rtlfm_gpu_malloc_apart_ex(int device, size_t bytes, const void *other, size_t other_bytes, size_t budget_bytes,
                                         void **out, int *apart, double *search_ms, size_t *walked_bytes);

// d_iq / iq_bytes: the input the first run streams from - what the front end's emit mode writes (deepA) goes a quarter of
// the HBM away from it, as the result buffers do (ensure_res_buffers; option "deep_apart" says whether it worked)
static int ensure_deep_buffers(rtlfm_gpu *h, const uint8_t *d_iq = nullptr, size_t iq_bytes = 0)
{
	if (h->deepA) return 0;
	const int N0 = (int)(h->cfg.block_len / 2);
	const bool fifth = fused::supported_emit(h->cfg);
	if (!fifth && !boxfused::supported_emit(h->cfg)) return 0;
	if (fifth) {
		const int level = h->cfg.downsample_passes < fused::kMaxP ? h->cfg.downsample_passes : fused::kMaxP;
		h->deep_stride = (size_t)h->cap_blocks * (N0 >> level);
	} else {
		h->deep_stride = (((size_t)h->cap_blocks * N0) / h->cfg.downsample + 1 + 16 + 3) & ~(size_t)3;  // rows start on 16-byte lines
	}
	const size_t bytes = (size_t)h->nstreams * h->deep_stride * sizeof(uint32_t);
	// (no search in the middle of an asynchronous call on a stream the caller owns, nor for buffers too small to matter)
	const bool search = d_iq && h->stream == h->own_stream && h->place.budget_gb > 0 && bytes >= ((size_t)32 << 20);
	if (search) {
		void *q = nullptr; int apart = 0; double ms = 0; size_t walked = 0;
		int r = rtlfm_gpu_malloc_apart_ex(h->device, bytes, d_iq, iq_bytes, (size_t)h->place.budget_gb << 30, &q, &apart, &ms, &walked);
		if (r < 0) return r;
		OWN_TRY(h->deepA.adopt(q, bytes / sizeof(uint32_t)));
		h->place.search_ms += ms;
		if (walked > h->place.walked_peak) h->place.walked_peak = walked;
		h->place.deep_apart = apart;
	} else {
		OWN_TRY(h->deepA.alloc(bytes / sizeof(uint32_t)));
		h->place.deep_apart = 0;
	}
	if (fifth) OWN_TRY(h->deepB.alloc(bytes / sizeof(uint32_t)));
	return 0;
}
// d_iq / iq_bytes: the input the first run streams from - the buffers the front end writes the demodulated
// samples into ([parity][0]) go a quarter of the HBM away from it where they are large enough to matter
static int ensure_res_buffers(rtlfm_gpu *h, const uint8_t *d_iq = nullptr, size_t iq_bytes = 0)
{
	const size_t S = (size_t)h->nstreams;
	if (!h->res[0][0]) {
		// The search times probe launches on the null stream and synchronises the device: not in the middle
		// of an asynchronous call on a stream the caller owns - there the buffers are plain allocations, and
		// res_apart says 0 (the caller can place its OWN output with rtlfm_gpu_malloc_apart: INTEGRATION.md).
		const bool search = d_iq && h->stream == h->own_stream && h->place.budget_gb > 0;
		const size_t one = (S * h->tstride * sizeof(int16_t) + 255) & ~(size_t)255;
		int apart = 0;
		if (search) {
			// the two buffers the front end writes (one per step parity) as ONE placed block, the second an alias into it:
			// one search, and a candidate that had to be larger than the request (rtlfm_gpu_malloc_apart_ex) is shared by both
			void *q = nullptr; double ms = 0; size_t walked = 0;
			int r = rtlfm_gpu_malloc_apart_ex(h->device, 2 * one, d_iq, iq_bytes, (size_t)h->place.budget_gb << 30, &q, &apart, &ms, &walked);
			if (r < 0) return r;
			h->place.search_ms += ms;
			if (walked > h->place.walked_peak) h->place.walked_peak = walked;
			OWN_TRY(h->res[0][0].adopt(q, 2 * one / sizeof(int16_t)));
			h->res[1][0] = h->res[0][0].alias(one / sizeof(int16_t));
		} else {
			for (int p = 0; p < 2; p++) OWN_TRY(h->res[p][0].alloc(one / sizeof(int16_t)));
		}
		for (int p = 0; p < 2; p++) OWN_TRY(h->res[p][1].alloc(one / sizeof(int16_t)));
		h->place.res_apart = apart;
	}
	return 0;
}
// bytes of the caller's input a run really covers: (S - 1) strides + the last stream's buffers (the stride may be padded)
static inline size_t iq_extent(const rtlfm_gpu *h, size_t stream_stride, int nblocks)
{
	const int rows = h->chan_per > 0 ? h->nstreams / h->chan_per : h->nstreams;  // (channels on: one row per SOURCE)
	return (size_t)(rows - 1) * stream_stride + (size_t)nblocks * h->cfg.block_len;
}

extern "C" int rtlfm_gpu_destroy(rtlfm_gpu *h)
{
	if (!h) return -EINVAL;
	hipSetDevice(h->device);
	if (h->stream) hipStreamSynchronize(h->stream);
	if (h->tail_stream) hipStreamSynchronize(h->tail_stream);
	ingest_destroy(h);
	// The streams go back to the process-wide pool, never to hipStreamDestroy (stream_pool.h: the runtime releases a freed
	// object of a destroyed stream once more, later, in whoever's memory it has become - LAB.md I.21).
	// RTLFM_DESTROY_STREAMS=1 (tools/host_uaf_probe.py --mode destroy) restores round 5's behaviour for the comparison.
	static const bool destroy_streams = [] { const char *e = getenv("RTLFM_DESTROY_STREAMS"); return e && *e == '1'; }();
	if (destroy_streams) {
		if (h->own_stream) hipStreamDestroy(h->own_stream);
		if (h->tail_stream) hipStreamDestroy(h->tail_stream);
	} else {
		rtl_pool::stream_put(h->device, 0, h->own_stream);
		rtl_pool::stream_put(h->device, h->tail_prio_value, h->tail_stream);
	}
	delete h;
	return 0;
}

// Option source_dc: the sums, the lists of biases and the history's biases, for the most sources and the longest run the
// handle can have (a view - run_ragged - cannot allocate).
static int ensure_source_dc(rtlfm_gpu *h)
{
	const size_t S = (size_t)h->nstreams;
	h->sdc_stride = (size_t)channel::kDcHist + (size_t)h->cap_blocks * (h->cfg.block_len / (2 * channel::kDcPiece));
	OWN_TRY(h->d_sdc_sums.alloc(S * h->cap_blocks * 2));
	OWN_TRY(h->d_sdc.alloc(S * h->sdc_stride));
	for (int i = 0; i < 2; i++) OWN_TRY(h->d_sdc_hist[i].alloc(S * channel::kDcHist));
	return 0;
}

// Options source_stats / source_health: the records of whichever is on, [sources][cap_blocks] for the sources there are now
// (a view - run_ragged - cannot allocate: the handle's run does, before the first view).  Allocated on first use, regrown
// - never shrunk - when there are more sources than they were sized for (DevBuf::grow waits for the handle's stream first);
// what they held is gone then, and the callers have said so (src_*_nblocks = 0) or are about to overwrite it.
static int ensure_source_records(rtlfm_gpu *h)
{
	if (h->chan_per <= 0 || (!h->opt.source_stats && !h->opt.source_health)) return 0;
	const int nsrc = h->nstreams / h->chan_per;
	const size_t need = (size_t)nsrc * h->cap_blocks;
	if (h->opt.source_stats) OWN_TRY(h->d_src_stats.grow(need, h->stream));
	if (h->opt.source_health) OWN_TRY(h->d_src_health.grow(need, h->stream));
	return 0;
}

// Option source_iq.  The coefficients on the host, [nstreams][4]: the identity until somebody sets them.
static void siq_identity(rtlfm_gpu *h)
{
	h->siq_coef.assign((size_t)h->nstreams * 4, 0);
	for (int s = 0; s < h->nstreams; s++) h->siq_coef[(size_t)s * 4] = h->siq_coef[(size_t)s * 4 + 3] = 16384;
}
// ... and on the device: allocated by whoever needs them first, with what rules now (a blocking copy: nothing reads them yet)
static int ensure_source_iq_coef(rtlfm_gpu *h)
{
	if (h->d_siq_coef) return 0;
	if (h->siq_coef.empty()) siq_identity(h);
	OWN_TRY(h->d_siq_coef.alloc((size_t)h->nstreams * 4));
	HIP_TRY(hipMemcpy(h->d_siq_coef, h->siq_coef.data(), h->siq_coef.size() * sizeof(int16_t), hipMemcpyHostToDevice));
	return 0;
}
// The corrected rows, [sources][cap_blocks * block_len], and the records, [sources][cap_blocks], for the sources there are now
// (a view cannot allocate: the handle's run does, before the first view).  Grown - never shrunk - behind the handle's stream;
// the rows hold nothing a later run needs, and the callers have said what became of the records (siq_nblocks = 0).
static int ensure_source_iq(rtlfm_gpu *h)
{
	if (h->chan_per <= 0 || !h->opt.source_iq) return 0;
	const size_t nsrc = (size_t)(h->nstreams / h->chan_per);
	h->siq_stride = (size_t)h->cap_blocks * h->cfg.block_len;  // (a multiple of 512: rows start on 16-byte lines)
	OWN_TRY(h->d_siq_rows.grow(nsrc * h->siq_stride, h->stream));
	OWN_TRY(h->d_siq_sums.grow(nsrc * h->cap_blocks, h->stream));
	return ensure_source_iq_coef(h);
}

// The source history - every source's carried bytes - back to 127: mixed zeros, m[n < 0] = 0 and x[n < 0] = 0.  On the
// handle's stream: behind the runs already queued, in front of the next.
static int history_clear(rtlfm_gpu *h)
{
	if (!h->d_src_hist[0]) return 0;
	HIP_TRY(hipMemsetAsync(h->d_src_hist[h->src_hist_cur], 127, (size_t)h->src_hist_srcs * channel::kHist * 2, h->stream));
	// (option source_dc: with them what was subtracted from them - nothing)
	if (h->d_sdc_hist[0])
		HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)h->d_sdc_hist[h->src_hist_cur].get(), (int)channel::kDcNone,
		                          (size_t)h->nstreams * channel::kDcHist, h->stream));
	return 0;
}

// The history's two copies, for the sources there are now: allocated or grown (never shrunk) once channels are on and a
// filter or a bank is set - a filter may be set while channels are off, when nobody knows how many sources there will be -
// and cleared, as every caller is about to ask anyway (what a fresh allocation holds must not reach a run).  The handle is
// idle: its callers have waited for it.
static int ensure_history(rtlfm_gpu *h)
{
	const int nsrc = h->chan_per > 0 && (h->fir_ntaps > 0 || h->bank_K > 0) ? h->nstreams / h->chan_per : 0;
	if (h->src_hist_srcs < nsrc) {
		h->src_hist_srcs = 0;  // (until both copies are there: chan_run_prepare refuses a run without them)
		for (int i = 0; i < 2; i++) {
			OWN_TRY(h->d_src_hist[i].grow((size_t)nsrc * channel::kHist * 2, h->stream));
		}
		h->src_hist_srcs = nsrc;
	}
	return history_clear(h);
}

extern "C" int rtlfm_gpu_reset(rtlfm_gpu *h)
{
	if (!h) return -EINVAL;
	HIP_TRY(hipSetDevice(h->device));
	std::vector<state_t> init((size_t)h->nstreams);
	init_states_host(init);
	HIP_TRY(sync_all(h));
	HIP_TRY(hipMemcpy(h->st[h->st_cur], init.data(), init.size() * sizeof(state_t), hipMemcpyHostToDevice));
	ingest_reset(h);
	h->chan_pos = 0;
	return history_clear(h);
}

extern "C" int rtlfm_gpu_state_get(rtlfm_gpu *h, int stream, rtlfm_stream_state *st)
{
	if (!h || !st || stream < 0 || stream >= h->nstreams) return -EINVAL;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(sync_all(h));
	HIP_TRY(hipMemcpy(st, h->st[h->st_cur] + stream, sizeof(*st), hipMemcpyDeviceToHost));
	return 0;
}

extern "C" int rtlfm_gpu_state_set(rtlfm_gpu *h, int stream, const rtlfm_stream_state *st)
{
	if (!h || !st || stream < 0 || stream >= h->nstreams) return -EINVAL;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(sync_all(h));
	HIP_TRY(hipMemcpy(h->st[h->st_cur] + stream, st, sizeof(*st), hipMemcpyHostToDevice));
	return 0;
}

// ---- the stream lifecycle: every stream's carried state in one operation (include/rtlfm_hip.h) ----

extern "C" int rtlfm_gpu_state_get_all(rtlfm_gpu *h, rtlfm_stream_state *out, int cap, int *n)
{
	if (!h || !out || !n) return -EINVAL;
	*n = h->nstreams;
	if (cap < h->nstreams) return -ENOBUFS;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(sync_all(h));
	HIP_TRY(hipMemcpy(out, h->st[h->st_cur], (size_t)h->nstreams * sizeof(state_t), hipMemcpyDeviceToHost));
	return 0;
}

extern "C" int rtlfm_gpu_state_set_all(rtlfm_gpu *h, const rtlfm_stream_state *in, int n)
{
	if (!h || !in || n != h->nstreams) return -EINVAL;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(sync_all(h));
	HIP_TRY(hipMemcpy(h->st[h->st_cur], in, (size_t)h->nstreams * sizeof(state_t), hipMemcpyHostToDevice));
	return 0;
}

// every stream's owed mute at once (what rtlfm_gpu_mute keeps per stream)
static int set_mutes(rtlfm_gpu *h, const uint32_t *mutes)
{
	bool any = false;
	for (int s = 0; s < h->nstreams; s++) any |= mutes[s] != 0;
	if (!h->mute_left) {
		if (!any) return 0;
		h->mute_left.reset(new (std::nothrow) uint32_t[(size_t)h->nstreams]());
		if (!h->mute_left) return -ENOMEM;
	}
	h->mute_streams = 0;
	for (int s = 0; s < h->nstreams; s++) {
		h->mute_left[s] = mutes[s];
		h->mute_streams += mutes[s] ? 1 : 0;
	}
	return 0;
}

// dst[k] = src[map[k]] (-1: the initial record), state and owed mute; one launch (k_state_move, state_kernel.h).
// Ordering, also for dst == src: both handles are idle behind sync_all - no run, no tail reads or writes any state copy -,
// the kernel reads src->st[src->st_cur] and writes dst's NEXT copy, which nothing reads before st_cur has advanced, and
// st_cur advances only behind the synchronisation that follows the launch.  A failure before that leaves st_cur, and so
// the handle's state, where it was.
extern "C" int rtlfm_gpu_state_move(rtlfm_gpu *dst, rtlfm_gpu *src, const int32_t *map, int n)
{
	if (!dst || !src || !map || n != dst->nstreams) return -EINVAL;
	if (dst->chan_per > 0 || src->chan_per > 0) return -ENOTSUP;  // (channels: the record does not hold pos)
	for (int k = 0; k < n; k++)
		if (map[k] < -1 || map[k] >= src->nstreams) return -EINVAL;
	if (dst->device != src->device) return -EXDEV;
	if (ingest_busy(dst) || (src != dst && ingest_busy(src))) return -EBUSY;
	std::vector<uint32_t> mutes;  // (taken before anything changes: in place, map reads what the loop below would overwrite)
	try {
		mutes.assign((size_t)n, 0u);
	} catch (const std::bad_alloc &) {
		return -ENOMEM;
	}
	if (src->mute_left)
		for (int k = 0; k < n; k++)
			if (map[k] >= 0) mutes[(size_t)k] = src->mute_left[map[k]];
	HIP_TRY(hipSetDevice(dst->device));
	OWN_TRY(dst->d_move_map.alloc((size_t)n));
	HIP_TRY(sync_all(src));
	if (src != dst) HIP_TRY(sync_all(dst));
	HIP_TRY(hipMemcpy(dst->d_move_map, map, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
	const int next = (dst->st_cur + 1) % 3;
	const int r = statemove::launch(dst->st[next], src->st[src->st_cur], dst->d_move_map, n, dst->stream);
	if (r < 0) return r;
	HIP_TRY(hipStreamSynchronize(dst->stream));
	const int m = set_mutes(dst, mutes.data());
	if (m < 0) return m;
	dst->st_cur = next;
	return 0;
}

// what a stream carries depends on every field of the configuration but these two
static bool same_carried_cfg(rtlfm_cfg a, const rtlfm_cfg &b)
{
	a.max_blocks = b.max_blocks;
	a.report_levels = b.report_levels;
	return memcmp(&a, &b, sizeof(a)) == 0;
}

extern "C" int rtlfm_gpu_save(rtlfm_gpu *h, const char *path)
{
	if (!h || !path) return -EINVAL;
	if (h->chan_per > 0) return -ENOTSUP;  // (channels: a snapshot does not hold pos)
	std::vector<state_t> st;
	std::vector<uint32_t> mutes;
	try {
		st.resize((size_t)h->nstreams);
		mutes.assign((size_t)h->nstreams, 0u);
	} catch (const std::bad_alloc &) {
		return -ENOMEM;
	}
	int n = 0;
	const int r = rtlfm_gpu_state_get_all(h, st.data(), h->nstreams, &n);
	if (r < 0) return r;
	if (h->mute_left) memcpy(mutes.data(), h->mute_left.get(), mutes.size() * sizeof(uint32_t));
	return rtlfm_snapshot_write(path, &h->cfg, h->nstreams, st.data(), mutes.data());
}

extern "C" int rtlfm_gpu_load(rtlfm_gpu *h, const char *path)
{
	if (!h || !path) return -EINVAL;
	if (h->chan_per > 0) return -ENOTSUP;
	rtlfm_cfg cfg;
	int n = 0;
	int r = rtlfm_snapshot_info(path, &cfg, &n);  // (checks the whole file, the checksum included)
	if (r < 0) return r;
	if (n != h->nstreams) return -ERANGE;
	if (!same_carried_cfg(cfg, h->cfg)) return -EMEDIUMTYPE;
	std::vector<state_t> st;
	std::vector<uint32_t> mutes;
	try {
		st.resize((size_t)n);
		mutes.assign((size_t)n, 0u);
	} catch (const std::bad_alloc &) {
		return -ENOMEM;
	}
	int got = 0;
	if ((r = rtlfm_snapshot_read(path, nullptr, st.data(), mutes.data(), n, &got)) < 0) return r;
	if (got != n) return -EILSEQ;  // (the file changed between the two reads)
	if ((r = rtlfm_gpu_state_set_all(h, st.data(), n)) < 0) return r;
	return set_mutes(h, mutes.data());
}

// ---- channels: K channels per wideband source (include/rtlfm_hip.h, channel_kernel.h) ----

extern "C" uint32_t rtlfm_channel_step(int32_t shift_hz, uint32_t capture_rate)
{
	if (!capture_rate) return 0;
	// round_half_up(shift * 2^32 / rate) = floor((2 shift 2^32 + rate) / (2 rate)), exactly; the result modulo 2^32
	const __int128 a = (((__int128)shift_hz) << 33) + (__int128)capture_rate, b = 2 * (__int128)capture_rate;
	__int128 quo = a / b;
	if (a % b < 0) quo -= 1;  // C truncates towards zero
	return (uint32_t)(unsigned __int128)quo;
}

extern "C" int rtlfm_channel_table(int16_t *cos_sin)
{
	if (!cos_sin) return -EINVAL;
	channel::build_table(cos_sin);
	return 0;
}

extern "C" int rtlfm_gpu_set_channels(rtlfm_gpu *h, int per_source, const uint32_t *steps)
{
	if (!h || per_source < 0) return -EINVAL;
	if (per_source > 0 && (!steps || h->nstreams % per_source)) return -EINVAL;
	if (ingest_busy(h) || h->mute_streams > 0) return -EBUSY;
	if (h->opt.source_ring && ingest_queued(h)) return -EBUSY;  // (queued buffers lie in rows of the old count)
	if (per_source > 0 && (h->cfg.dc_block_raw || h->opt.input_stats || h->opt.input_health || h->opt.squelch_gate)) return -ENOTSUP;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(sync_all(h));
	if (per_source > 0) {
		if (!h->d_chan_table) {
			std::vector<int16_t> tab(2 * channel::kTableSize);
			channel::build_table(tab.data());  // (int16 cos, int16 sin = the kernels' packed dword)
			DevBuf<uint32_t> d;
			OWN_TRY(d.alloc(channel::kTableSize));
			if (hipMemcpy(d, tab.data(), channel::kTableSize * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) return -EIO;
			h->d_chan_table = std::move(d);
		}
		OWN_TRY(h->d_chan_steps.alloc((size_t)h->nstreams));
		HIP_TRY(hipMemcpy(h->d_chan_steps, steps, (size_t)h->nstreams * sizeof(uint32_t), hipMemcpyHostToDevice));
	}
	h->chan_per = per_source;
	h->chan_pos = 0;
	h->bank_K = 0;  // (the bank's bins belong to the old per_source)
	h->bank_bins_ps.clear();
	h->src_stats_nblocks = h->src_health_nblocks = 0;  // (options source_stats / source_health: records of the old rows)
	h->siq_nblocks = 0;                                // (option source_iq: the same, and every source back to the identity)
	siq_identity(h);
	if (h->d_siq_coef)
		HIP_TRY(hipMemcpy(h->d_siq_coef, h->siq_coef.data(), h->siq_coef.size() * sizeof(int16_t), hipMemcpyHostToDevice));
	int r = ensure_history(h);
	if (r < 0) return r;
	if ((r = ensure_source_records(h)) < 0) return r;
	if ((r = ensure_source_iq(h)) < 0) return r;
	return ingest_resize(h);  // (option source_ring: the ring's input side for the new number of sources)
}

extern "C" int rtlfm_gpu_channels_seek(rtlfm_gpu *h, uint64_t pos)
{
	if (!h) return -EINVAL;
	h->chan_pos = pos;  // (read by the next run's launch; runs already queued took theirs by value)
	if (!h->d_src_hist[0]) return 0;
	HIP_TRY(hipSetDevice(h->device));
	return history_clear(h);  // (the history belongs to the old position)
}

// ---- the channel filter: a caller-supplied FIR in the boxcar's place (include/rtlfm_hip.h, channel_fir_kernel.h) ----

extern "C" int rtlfm_channel_filter_check(const int16_t *taps, int ntaps, int shift)
{
	if (!taps || ntaps < 1 || ntaps > RTLFM_CHANNEL_MAX_TAPS || shift < 0 || shift > 30) return -EINVAL;
	long long sum = 0;
	for (int j = 0; j < ntaps; j++) sum += taps[j] < 0 ? -(long long)taps[j] : (long long)taps[j];
	const long long r = shift ? 1ll << (shift - 1) : 0;
	return 182 * sum + r <= 0x7fffffffll ? 0 : -ERANGE;  // |m| <= 182: the int32 sum and its rounding cannot overflow
}

extern "C" int rtlfm_channel_filter_check_dc(const int16_t *taps, int ntaps, int shift)
{
	if (!taps || ntaps < 1 || ntaps > RTLFM_CHANNEL_MAX_TAPS || shift < 0 || shift > 30) return -EINVAL;
	long long sum = 0;
	for (int j = 0; j < ntaps; j++) sum += taps[j] < 0 ? -(long long)taps[j] : (long long)taps[j];
	const long long r = shift ? 1ll << (shift - 1) : 0;
	return 362 * sum + r <= 0x7fffffffll ? 0 : -ERANGE;  // option source_dc: |x|, |y| <= 256, so |m| <= 362
}

extern "C" int rtlfm_channel_lowpass(int ntaps, double cutoff, int D, int16_t *taps, int *shift)
{
	if (!taps || !shift || ntaps < 1 || ntaps > RTLFM_CHANNEL_MAX_TAPS || D < 1 || !(cutoff > 0.0 && cutoff < 0.5)) return -EINVAL;
	std::vector<double> hh((size_t)ntaps);
	const double mid = (ntaps - 1) / 2.0;
	double sum = 0;
	for (int j = 0; j < (ntaps + 1) / 2; j++) {  // (one half computed, the other its mirror image: symmetric to the bit)
		const double x = 2.0 * cutoff * ((double)j - mid);
		const double sinc = x == 0.0 ? 1.0 : sin(M_PI * x) / (M_PI * x);
		const double win = ntaps > 1 ? 0.54 - 0.46 * cos(2.0 * M_PI * (double)j / (double)(ntaps - 1)) : 1.0;
		hh[j] = hh[ntaps - 1 - j] = sinc * win;
	}
	for (int j = 0; j < ntaps; j++) sum += hh[j];
	if (!(fabs(sum) > 0.0)) return -ERANGE;
	std::vector<int16_t> q((size_t)ntaps);
	for (int j = 0; j < ntaps; j++) {
		const double v = floor(hh[j] / sum * (double)D * 16384.0 + 0.5);
		if (!(v >= -32768.0 && v <= 32767.0)) return -ERANGE;
		q[j] = (int16_t)v;
	}
	const int r = rtlfm_channel_filter_check(q.data(), ntaps, 14);
	if (r < 0) return r;
	memcpy(taps, q.data(), (size_t)ntaps * sizeof(int16_t));
	*shift = 14;
	return 0;
}

extern "C" int rtlfm_gpu_set_channel_filter(rtlfm_gpu *h, const int16_t *taps, int ntaps, int shift)
{
	if (!h) return -EINVAL;
	if (ntaps != 0) {
		int r = rtlfm_channel_filter_check(taps, ntaps, shift);
		if (r == 0 && h->opt.source_dc) r = rtlfm_channel_filter_check_dc(taps, ntaps, shift);
		if (r < 0) return r;
	}
	if (h->cfg.downsample_passes > 0) return -ENOTSUP;  // (the filter takes the boxcar's place, not fifth_order's)
	if (ingest_busy(h)) return -EBUSY;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(sync_all(h));
	if (ntaps > 0) {
		OWN_TRY(h->d_fir_taps.alloc(RTLFM_CHANNEL_MAX_TAPS));
		OWN_TRY(h->d_fir_taps8.alloc((size_t)chanfir::kGroup * chanfir::padded_taps(RTLFM_CHANNEL_MAX_TAPS) * sizeof(int16_t) / sizeof(uint32_t)));
		std::vector<int16_t> t8((size_t)chanfir::kGroup * chanfir::padded_taps(ntaps));
		chanfir::shifted_taps(taps, ntaps, t8.data());
		HIP_TRY(hipMemcpy(h->d_fir_taps, taps, (size_t)ntaps * sizeof(int16_t), hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(h->d_fir_taps8, t8.data(), t8.size() * sizeof(int16_t), hipMemcpyHostToDevice));
		h->fir_taps.assign(taps, taps + ntaps);
	} else {
		h->fir_taps.clear();
	}
	h->fir_ntaps = ntaps;
	h->fir_shift = ntaps > 0 ? shift : 0;
	return ensure_history(h);  // (cleared also where the bank is on and the filter rests: one history)
}

// ---- the channel bank: uniform channels by polyphase sums and one fix_fft (include/rtlfm_hip.h, channel_bank_kernel.h) ----

extern "C" int rtlfm_channel_bank_check(int K, const int16_t *taps, int ntaps, int shift)
{
	int m = 0;
	while (m <= chanbank::kMaxLog2 && (1 << m) != K) m++;
	if (m < chanbank::kMinLog2 || m > chanbank::kMaxLog2) return -EINVAL;
	if (!taps || ntaps < 1 || ntaps > RTLFM_BANK_MAX_TAPS || shift < 0 || shift > 30) return -EINVAL;
	long long most = 0;
	for (int b = 0; b < K && b < ntaps; b++) {
		long long sum = 0;
		for (int j = b; j < ntaps; j += K) sum += taps[j] < 0 ? -(long long)taps[j] : (long long)taps[j];
		if (sum > most) most = sum;
	}
	const long long r = shift ? 1ll << (shift - 1) : 0;
	return 128 * most + r <= 0x7fffffffll ? 0 : -ERANGE;  // |x| <= 128: a branch's int32 sum and its rounding cannot overflow
}

extern "C" int rtlfm_channel_bank_check_dc(int K, const int16_t *taps, int ntaps, int shift)
{
	const int e = rtlfm_channel_bank_check(K, taps, ntaps, shift);
	if (e != 0 && e != -ERANGE) return e;
	long long most = 0;
	for (int b = 0; b < K && b < ntaps; b++) {
		long long sum = 0;
		for (int j = b; j < ntaps; j += K) sum += taps[j] < 0 ? -(long long)taps[j] : (long long)taps[j];
		if (sum > most) most = sum;
	}
	const long long r = shift ? 1ll << (shift - 1) : 0;
	return 256 * most + r <= 0x7fffffffll ? 0 : -ERANGE;  // option source_dc: |x| <= 256
}

template <typename T>
static int bank_upload(DevBuf<T> &dst, const T *src, size_t n)
{
	dst.reset();  // (the handle is idle: the caller has waited for it)
	OWN_TRY(dst.alloc(n));
	HIP_TRY(hipMemcpy(dst, src, n * sizeof(T), hipMemcpyHostToDevice));
	return 0;
}

extern "C" int rtlfm_gpu_set_channel_bank(rtlfm_gpu *h, int K, const int32_t *bins, const int16_t *taps, int ntaps, int shift)
{
	if (!h) return -EINVAL;
	if (K != 0) {
		int r = rtlfm_channel_bank_check(K, taps, ntaps, shift);
		if (r == 0 && h->opt.source_dc) r = rtlfm_channel_bank_check_dc(K, taps, ntaps, shift);
		if (r < 0) return r;
	}
	if (ingest_busy(h)) return -EBUSY;  // (a begun run means channels off: asked first, or it could never be the answer)
	if (h->cfg.downsample_passes > 0) return -ENOTSUP;  // (the bank takes the boxcar front end's place, not fifth_order's)
	if (K != 0) {
		if (h->chan_per <= 0) return -EINVAL;
		if (!bins && h->chan_per != K) return -EINVAL;
		for (int c = 0; bins && c < h->chan_per; c++)
			if (bins[c] < 0 || bins[c] >= K) return -EINVAL;
	}
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(sync_all(h));
	if (K == 0) {
		h->bank_K = 0;
		h->bank_bins_ps.clear();
		return history_clear(h);
	}
	int m = 0;
	while ((1 << m) != K) m++;
	std::vector<int32_t> b((size_t)h->chan_per);
	for (int c = 0; c < h->chan_per; c++) b[c] = bins ? bins[c] : c;
	const chanbank::Geometry g = chanbank::geometry(m, ntaps, h->cfg.downsample);
	std::vector<int16_t> t2((size_t)2 * K * g.Qp);
	chanbank::branch_taps(taps, ntaps, g, t2.data());
	// sine_table(), src/rtl_power.c:247-261, for N_WAVE = K, and regrouped per stage as rtl_power's transforms read it:
	// entry (1 << s) - 1 + q holds (2 wr, 2 wi) of wr = Sinewave[j + K/4] >> 1, wi = -Sinewave[j] >> 1 at j = q << (m - 1 - s)
	std::vector<int16_t> sine((size_t)K * 3 / 4 + 1);
	for (int i = 0; i < K * 3 / 4; i++) sine[i] = (int16_t)(int)round(32767 * sin((double)i * 2.0 * M_PI / K));
	std::vector<uint32_t> tw((size_t)K, 0u);
	for (int st = 0; st < m; st++)
		for (int q = 0; q < (1 << st); q++) {
			const int j = q << (m - 1 - st);
			int16_t wr = sine[j + K / 4], wi = (int16_t)(-sine[j]);
			wr >>= 1; wi >>= 1;
			tw[(size_t)(1 << st) - 1 + q] = (uint32_t)(uint16_t)(wr * 2) | ((uint32_t)(uint16_t)(wi * 2) << 16);
		}
	int r;
	if ((r = bank_upload(h->d_bank_taps, taps, (size_t)ntaps)) < 0) return r;
	if ((r = bank_upload(h->d_bank_taps2, reinterpret_cast<const uint32_t *>(t2.data()), t2.size() / 2)) < 0) return r;
	if ((r = bank_upload(h->d_bank_tw, tw.data(), tw.size())) < 0) return r;
	if ((r = bank_upload(h->d_bank_sine, sine.data(), sine.size())) < 0) return r;
	if ((r = bank_upload(h->d_bank_bins, b.data(), b.size())) < 0) return r;
	h->bank_taps.assign(taps, taps + ntaps);
	h->bank_bins = b;
	h->bank_bins_ps.clear();  // (the shared list again)
	h->bank_m = m; h->bank_K = K; h->bank_ntaps = ntaps; h->bank_shift = shift;
	return ensure_history(h);
}

extern "C" int rtlfm_gpu_get_channel_bank(rtlfm_gpu *h, int *K, int32_t *bins, int bins_cap, int16_t *taps, int taps_cap, int *ntaps,
                                          int *shift)
{
	if (!h || !K || !ntaps || !shift || bins_cap < 0 || taps_cap < 0 || (bins_cap > 0 && !bins) || (taps_cap > 0 && !taps)) return -EINVAL;
	*K = h->bank_K;  // (written even where bins or taps do not fit)
	*ntaps = h->bank_K ? h->bank_ntaps : 0;
	*shift = h->bank_K ? h->bank_shift : 0;
	if (!h->bank_K) return 0;
	if ((int)h->bank_bins.size() > bins_cap || h->bank_ntaps > taps_cap) return -ENOBUFS;
	// (per-source bins set: source 0's)
	memcpy(bins, h->bank_bins_ps.empty() ? h->bank_bins.data() : h->bank_bins_ps.data(), h->bank_bins.size() * sizeof(int32_t));
	memcpy(taps, h->bank_taps.data(), (size_t)h->bank_ntaps * sizeof(int16_t));
	return 0;
}

// Per-source bins for the bank that is set: nothing else moves - pos, the history, the taps, every stream's record - and
// nothing is waited for but a staging buffer whose own copy has not left yet.  The copy is ordered on the handle's stream:
// runs queued before the call read the old bins, runs after it the new.
extern "C" int rtlfm_gpu_set_channel_bins(rtlfm_gpu *h, const int32_t *bins)
{
	if (!h || !bins || h->bank_K <= 0 || h->chan_per <= 0) return -EINVAL;
	const size_t n = (size_t)h->nstreams;  // sources * per_source
	for (size_t i = 0; i < n; i++)
		if (bins[i] < 0 || bins[i] >= h->bank_K) return -EINVAL;
	if (ingest_busy(h)) return -EBUSY;
	HIP_TRY(hipSetDevice(h->device));
	OWN_TRY(h->d_bank_bins_ps.alloc(n));  // (the first call: a handle's stream count never changes)
	for (int k = 0; k < rtlfm_gpu::kBinStages; k++) {
		OWN_TRY(h->h_bins_stage[k].alloc(n));
		OWN_TRY(h->ev_bins_stage[k].create(hipEventDisableTiming));
	}
	const int k = h->bins_stage_next;
	HIP_TRY(hipEventSynchronize(h->ev_bins_stage[k]));  // (an event never recorded is complete)
	memcpy(h->h_bins_stage[k], bins, n * sizeof(int32_t));
	HIP_TRY(hipMemcpyAsync(h->d_bank_bins_ps, h->h_bins_stage[k], n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
	HIP_TRY(hipEventRecord(h->ev_bins_stage[k], h->stream));
	h->bins_stage_next = (k + 1) % rtlfm_gpu::kBinStages;
	h->bank_bins_ps.assign(bins, bins + n);
	return 0;
}

extern "C" int rtlfm_gpu_get_channel_bins(rtlfm_gpu *h, int32_t *bins, int cap)
{
	if (!h || !bins || cap < 0 || h->bank_K <= 0 || h->chan_per <= 0) return -EINVAL;
	if (cap < h->nstreams) return -ENOBUFS;
	for (int s = 0; s < h->nstreams; s++)
		bins[s] = h->bank_bins_ps.empty() ? h->bank_bins[(size_t)(s % h->chan_per)] : h->bank_bins_ps[(size_t)s];
	return 0;
}

// Option source_iq's coefficients, (a, b, p, q) per source: the bins' pattern - nothing is waited for but a staging buffer
// whose own copy has not left yet, and the copy is ordered on the handle's stream: runs queued before the call read the old
// coefficients, runs after it the new.
extern "C" int rtlfm_gpu_set_source_iq(rtlfm_gpu *h, const int16_t *coef)
{
	if (!h || !coef) return -EINVAL;
	if (h->chan_per <= 0) return -ENOTSUP;
	if (ingest_busy(h)) return -EBUSY;
	HIP_TRY(hipSetDevice(h->device));
	const size_t n = (size_t)(h->nstreams / h->chan_per) * 4, cap = (size_t)h->nstreams * 4;
	int r = ensure_source_iq_coef(h);
	if (r < 0) return r;
	for (int k = 0; k < rtlfm_gpu::kIqStages; k++) {
		OWN_TRY(h->h_siq_stage[k].alloc(cap));  // (the first call: a handle's stream count never changes)
		OWN_TRY(h->ev_siq_stage[k].create(hipEventDisableTiming));
	}
	const int k = h->siq_stage_next;
	HIP_TRY(hipEventSynchronize(h->ev_siq_stage[k]));  // (an event never recorded is complete)
	memcpy(h->h_siq_stage[k], coef, n * sizeof(int16_t));
	HIP_TRY(hipMemcpyAsync(h->d_siq_coef, h->h_siq_stage[k], n * sizeof(int16_t), hipMemcpyHostToDevice, h->stream));
	HIP_TRY(hipEventRecord(h->ev_siq_stage[k], h->stream));
	h->siq_stage_next = (k + 1) % rtlfm_gpu::kIqStages;
	std::copy(coef, coef + n, h->siq_coef.begin());
	return 0;
}

extern "C" int rtlfm_gpu_get_source_iq(rtlfm_gpu *h, int16_t *coef, int cap)
{
	if (!h || !coef || cap < 0) return -EINVAL;
	if (h->chan_per <= 0) return -ENOTSUP;
	const size_t n = (size_t)(h->nstreams / h->chan_per) * 4;
	if ((size_t)cap < n) return -ENOBUFS;
	if (h->siq_coef.empty()) siq_identity(h);
	memcpy(coef, h->siq_coef.data(), n * sizeof(int16_t));
	return 0;
}

extern "C" int rtlfm_gpu_get_channel_filter(rtlfm_gpu *h, int16_t *taps, int cap, int *ntaps, int *shift)
{
	if (!h || !ntaps || !shift || cap < 0 || (cap > 0 && !taps)) return -EINVAL;
	*ntaps = h->fir_ntaps;  // (written even where the taps do not fit, as rtlfm_gpu_levels' count)
	*shift = h->fir_shift;
	if (h->fir_ntaps > cap) return -ENOBUFS;
	if (h->fir_ntaps > 0) memcpy(taps, h->fir_taps.data(), (size_t)h->fir_ntaps * sizeof(int16_t));
	return 0;
}

extern "C" int rtlfm_gpu_channels_tell(rtlfm_gpu *h, uint64_t *pos)
{
	if (!h || !pos) return -EINVAL;
	*pos = h->chan_pos;
	return 0;
}

// ---- the channel lifecycle: what a handle with channels on carries beyond the records (include/rtlfm_hip.h) ----

static_assert(statemove::kHistPieces * 16 == channel::kHist * 2 && statemove::kDcWords == channel::kDcHist, "k_source_move moves the history the channel kernels keep");
static_assert(RTLFM_CHANSNAP_HIST == channel::kHist && RTLFM_CHANSNAP_DC_PIECES == channel::kDcHist && RTLFM_CHANSNAP_DC_NONE == channel::kDcNone,
              "the file holds the history the channel kernels keep");

// a history is carried: channels on and something set that re-reads it
static inline bool carries_history(const rtlfm_gpu *h) { return h->chan_per > 0 && (h->fir_ntaps > 0 || h->bank_K > 0); }

// what _channels_move, _channels_history_set and _channels_load must not interrupt
static bool lifecycle_busy(rtlfm_gpu *h) { return ingest_busy(h) || (h->opt.source_ring && ingest_queued(h)); }

extern "C" int rtlfm_gpu_channels_history_get(rtlfm_gpu *h, uint8_t *bytes, size_t cap_bytes, uint32_t *dc, size_t cap_dc, int *sources)
{
	if (!h || !sources) return -EINVAL;
	*sources = h->chan_per > 0 ? h->nstreams / h->chan_per : 0;
	if (h->chan_per <= 0) return -ENOTSUP;
	if (!carries_history(h)) return -ENODATA;
	if (!bytes || (h->opt.source_dc && !dc)) return -EINVAL;
	const size_t nsrc = (size_t)*sources;
	if (cap_bytes < nsrc * channel::kHist * 2 || (h->opt.source_dc && cap_dc < nsrc * channel::kDcHist)) return -ENOBUFS;
	if (!h->d_src_hist[0] || !h->d_src_hist[1] || (size_t)h->src_hist_srcs < nsrc) return -EFAULT;
	if (h->opt.source_dc && (!h->d_sdc_hist[0] || !h->d_sdc_hist[1])) return -EFAULT;  // (before anything is written to an output)
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(sync_all(h));
	HIP_TRY(hipMemcpy(bytes, h->d_src_hist[h->src_hist_cur], nsrc * channel::kHist * 2, hipMemcpyDeviceToHost));
	if (h->opt.source_dc) {
		HIP_TRY(hipMemcpy(dc, h->d_sdc_hist[h->src_hist_cur], nsrc * channel::kDcHist * sizeof(uint32_t), hipMemcpyDeviceToHost));
	}
	return 0;
}

// A history and its biases into the buffers that are NOT current; the caller changes over (src_hist_cur ^= 1) once everything
// that belongs together has arrived, so a copy that fails half way leaves the history where it was.  The handle is idle
// behind sync_all - nothing reads or writes either copy - and the buffers are there: the callers have seen to both.
static int history_stage(rtlfm_gpu *h, const uint8_t *bytes, const uint32_t *dc, size_t nsrc)
{
	const int next = h->src_hist_cur ^ 1;
	HIP_TRY(hipMemcpy(h->d_src_hist[next], bytes, nsrc * channel::kHist * 2, hipMemcpyHostToDevice));
	if (!h->opt.source_dc) return 0;
	if (dc) {
		HIP_TRY(hipMemcpy(h->d_sdc_hist[next], dc, nsrc * channel::kDcHist * sizeof(uint32_t), hipMemcpyHostToDevice));
	} else {
		HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)h->d_sdc_hist[next].get(), (int)channel::kDcNone, nsrc * channel::kDcHist, h->stream));
		HIP_TRY(hipStreamSynchronize(h->stream));
	}
	return 0;
}

extern "C" int rtlfm_gpu_channels_history_set(rtlfm_gpu *h, const uint8_t *bytes, const uint32_t *dc, int sources)
{
	if (!h || !bytes) return -EINVAL;
	if (h->chan_per <= 0) return -ENOTSUP;
	if (sources != h->nstreams / h->chan_per) return -EINVAL;
	if (!carries_history(h)) return -ENODATA;
	if (lifecycle_busy(h)) return -EBUSY;
	const size_t nsrc = (size_t)sources;
	if (!h->d_src_hist[0] || !h->d_src_hist[1] || (size_t)h->src_hist_srcs < nsrc) return -EFAULT;
	if (h->opt.source_dc && (!h->d_sdc_hist[0] || !h->d_sdc_hist[1])) return -EFAULT;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(sync_all(h));
	const int r = history_stage(h, bytes, dc, nsrc);
	if (r < 0) return r;
	h->src_hist_cur ^= 1;
	return 0;
}

// -EMEDIUMTYPE's comparison, for the move and the load: the carried cfg, per_source, source_dc, the filter and the bank
static bool same_carried(const rtlfm_cfg &cfg, int per, int source_dc, int fir_ntaps, int fir_shift, const int16_t *fir_taps, int bank_K, int bank_ntaps,
                         int bank_shift, const int16_t *bank_taps, const rtlfm_gpu *h)
{
	if (!same_carried_cfg(cfg, h->cfg) || per != h->chan_per || (source_dc != 0) != (h->opt.source_dc != 0)) return false;
	if (fir_ntaps != h->fir_ntaps || fir_shift != h->fir_shift) return false;
	if (fir_ntaps > 0 && memcmp(fir_taps, h->fir_taps.data(), (size_t)fir_ntaps * sizeof(int16_t)) != 0) return false;
	if (bank_K != h->bank_K) return false;
	if (bank_K > 0) {
		if (bank_ntaps != h->bank_ntaps || bank_shift != h->bank_shift) return false;
		if (memcmp(bank_taps, h->bank_taps.data(), (size_t)bank_ntaps * sizeof(int16_t)) != 0) return false;
	}
	return true;
}

// The regroup by SOURCE, one launch (k_source_move, state_kernel.h).  Ordering as rtlfm_gpu_state_move's, also for dst == src:
// both handles are idle behind sync_all, the kernel reads src's current state copy and current history and writes dst's NEXT
// state copy and the history buffers that are NOT current, which nothing reads before st_cur / src_hist_cur have changed
// over, and they change over - with pos - only behind the synchronisation that follows the launch.  A failure before that
// leaves the handle where it was.
extern "C" int rtlfm_gpu_channels_move(rtlfm_gpu *dst, rtlfm_gpu *src, const int32_t *source_map, int nsources)
{
	if (!dst || !src || !source_map) return -EINVAL;
	if (dst->chan_per <= 0 || src->chan_per <= 0) return -ENOTSUP;
	const int dsrcs = dst->nstreams / dst->chan_per, ssrcs = src->nstreams / src->chan_per;
	if (nsources != dsrcs) return -EINVAL;
	for (int a = 0; a < nsources; a++)
		if (source_map[a] < -1 || source_map[a] >= ssrcs) return -EINVAL;
	if (dst->device != src->device) return -EXDEV;
	if (!same_carried(src->cfg, src->chan_per, src->opt.source_dc, src->fir_ntaps, src->fir_shift, src->fir_taps.data(), src->bank_K, src->bank_ntaps,
	                  src->bank_shift, src->bank_taps.data(), dst))
		return -EMEDIUMTYPE;
	if (lifecycle_busy(dst) || (src != dst && lifecycle_busy(src))) return -EBUSY;
	const bool hist = carries_history(dst), dc = hist && dst->opt.source_dc;
	if (hist && (!dst->d_src_hist[0] || !dst->d_src_hist[1] || !src->d_src_hist[0] || !src->d_src_hist[1] || dst->src_hist_srcs < dsrcs || src->src_hist_srcs < ssrcs)) return -EFAULT;
	if (dc && (!dst->d_sdc_hist[0] || !dst->d_sdc_hist[1] || !src->d_sdc_hist[0] || !src->d_sdc_hist[1])) return -EFAULT;
	HIP_TRY(hipSetDevice(dst->device));
	OWN_TRY(dst->d_move_map.alloc((size_t)dst->nstreams));  // (nstreams: rtlfm_gpu_state_move shares it once channels are off)
	HIP_TRY(sync_all(src));
	if (src != dst) HIP_TRY(sync_all(dst));
	HIP_TRY(hipMemcpy(dst->d_move_map, source_map, (size_t)nsources * sizeof(int32_t), hipMemcpyHostToDevice));
	const int next = (dst->st_cur + 1) % 3, hnext = dst->src_hist_cur ^ 1;
	statemove::SourceMove p{};
	p.dst_rec = reinterpret_cast<uint32_t *>(dst->st[next].get());
	p.src_rec = reinterpret_cast<const uint32_t *>(src->st[src->st_cur].get());
	if (hist) {
		p.dst_hist = reinterpret_cast<uint4 *>(dst->d_src_hist[hnext].get());
		p.src_hist = reinterpret_cast<const uint4 *>(src->d_src_hist[src->src_hist_cur].get());
	}
	if (dc) {
		p.dst_dc = dst->d_sdc_hist[hnext].get();
		p.src_dc = src->d_sdc_hist[src->src_hist_cur].get();
	}
	p.map = dst->d_move_map;
	p.nsrc = (uint32_t)nsources;
	p.per = (uint32_t)dst->chan_per;
	p.dc_none = channel::kDcNone;
	const int r = statemove::launch_source_move(p, dst->stream);
	if (r < 0) return r;
	HIP_TRY(hipStreamSynchronize(dst->stream));
	dst->st_cur = next;
	if (hist) dst->src_hist_cur = hnext;
	dst->chan_pos = src->chan_pos;
	return 0;
}

extern "C" int rtlfm_gpu_channels_save(rtlfm_gpu *h, const char *path)
{
	if (!h || !path) return -EINVAL;
	if (h->chan_per <= 0) return -ENOTSUP;
	// (a run begun and not ended: pos and the records are between two states; buffers queued over the source ring: the file
	// would silently lack them)
	if (lifecycle_busy(h)) return -EBUSY;
	const size_t n = (size_t)h->nstreams, nsrc = n / (size_t)h->chan_per;
	const bool hist = carries_history(h), dc = hist && h->opt.source_dc;
	std::vector<state_t> st;
	std::vector<uint32_t> steps, dcw;
	std::vector<uint8_t> bytes;
	std::vector<int32_t> bins;
	try {
		st.resize(n);
		steps.resize(n);
		if (hist) bytes.resize(nsrc * channel::kHist * 2);
		if (dc) dcw.resize(nsrc * channel::kDcHist);
		if (h->bank_K > 0) bins.resize(n);
	} catch (const std::bad_alloc &) {
		return -ENOMEM;
	}
	int got = 0, r;
	if ((r = rtlfm_gpu_state_get_all(h, st.data(), h->nstreams, &got)) < 0) return r;
	if (hist && (r = rtlfm_gpu_channels_history_get(h, bytes.data(), bytes.size(), dc ? dcw.data() : nullptr, dcw.size(), &got)) < 0) return r;
	HIP_TRY(hipMemcpy(steps.data(), h->d_chan_steps, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (h->bank_K > 0 && (r = rtlfm_gpu_get_channel_bins(h, bins.data(), h->nstreams)) < 0) return r;
	rtlfm_chansnap_hdr hd{};
	hd.pos = h->chan_pos;
	hd.nstreams = (uint32_t)h->nstreams;
	hd.per_source = (uint32_t)h->chan_per;
	hd.flags = (h->opt.source_dc ? RTLFM_CHANSNAP_FLAG_SOURCE_DC : 0u) | (hist ? RTLFM_CHANSNAP_FLAG_HISTORY : 0u);
	hd.fir_ntaps = (uint32_t)h->fir_ntaps;
	hd.fir_shift = (uint32_t)h->fir_shift;
	hd.bank_K = (uint32_t)h->bank_K;
	hd.bank_ntaps = h->bank_K > 0 ? (uint32_t)h->bank_ntaps : 0u;
	hd.bank_shift = h->bank_K > 0 ? (uint32_t)h->bank_shift : 0u;
	rtlfm_chansnap_parts pt{};
	pt.cfg = &h->cfg;
	pt.steps = steps.data();
	pt.fir_taps = h->fir_taps.data();
	pt.bank_taps = h->bank_taps.data();
	pt.bins = bins.data();
	pt.states = st.data();
	pt.hist = bytes.data();
	pt.dc = dc ? dcw.data() : nullptr;
	return rtlfm_chansnap_write(path, &hd, &pt);
}

extern "C" int rtlfm_gpu_channels_load(rtlfm_gpu *h, const char *path)
{
	if (!h || !path) return -EINVAL;
	if (h->chan_per <= 0) return -ENOTSUP;
	rtlfm_chansnap_hdr hd;
	rtlfm_cfg cfg;
	int r = rtlfm_chansnap_info(path, &hd, &cfg);  // (checks the whole file, the checksum included)
	if (r < 0) return r;
	if (hd.nstreams != (uint32_t)h->nstreams) return -ERANGE;
	const size_t n = hd.nstreams, nsrc = n / hd.per_source;
	const bool hist = (hd.flags & RTLFM_CHANSNAP_FLAG_HISTORY) != 0, dc = hist && (hd.flags & RTLFM_CHANSNAP_FLAG_SOURCE_DC);
	std::vector<state_t> st;
	std::vector<uint32_t> dcw;
	std::vector<uint8_t> bytes;
	std::vector<int16_t> ftaps, btaps;
	try {
		st.resize(n);
		ftaps.resize(hd.fir_ntaps);
		btaps.resize(hd.bank_ntaps);
		if (hist) bytes.resize(nsrc * channel::kHist * 2);
		if (dc) dcw.resize(nsrc * channel::kDcHist);
	} catch (const std::bad_alloc &) {
		return -ENOMEM;
	}
	rtlfm_chansnap_hdr hd2;
	rtlfm_chansnap_bufs b{};
	b.fir_taps = ftaps.data(); b.cap_fir_taps = ftaps.size();
	b.bank_taps = btaps.data(); b.cap_bank_taps = btaps.size();
	b.states = st.data(); b.cap_states = st.size();
	b.hist = hist ? bytes.data() : nullptr; b.cap_hist = bytes.size();
	b.dc = dc ? dcw.data() : nullptr; b.cap_dc = dcw.size();
	if ((r = rtlfm_chansnap_read(path, &hd2, &b)) < 0) return r == -ENOBUFS ? -EILSEQ : r;
	if (memcmp(&hd, &hd2, sizeof(hd)) != 0) return -EILSEQ;  // (the file changed between the two reads)
	if (!same_carried(cfg, (int)hd.per_source, (hd.flags & RTLFM_CHANSNAP_FLAG_SOURCE_DC) != 0, (int)hd.fir_ntaps, (int)hd.fir_shift, ftaps.data(),
	                  (int)hd.bank_K, (int)hd.bank_ntaps, (int)hd.bank_shift, btaps.data(), h))
		return -EMEDIUMTYPE;
	if (lifecycle_busy(h)) return -EBUSY;
	if (hist && (!h->d_src_hist[0] || !h->d_src_hist[1] || (size_t)h->src_hist_srcs < nsrc)) return -EFAULT;
	if (dc && (!h->d_sdc_hist[0] || !h->d_sdc_hist[1])) return -EFAULT;
	// As rtlfm_gpu_channels_move: the handle idle behind sync_all, the records into the NEXT state copy and the history into the
	// buffers that are not current, which nothing reads before the change-over; st_cur, src_hist_cur and pos change over
	// together behind the last copy, so a copy that fails leaves the handle where it was.
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(sync_all(h));
	if (hist && (r = history_stage(h, bytes.data(), dc ? dcw.data() : nullptr, nsrc)) < 0) return r;
	const int next = (h->st_cur + 1) % 3;
	HIP_TRY(hipMemcpy(h->st[next], st.data(), n * sizeof(state_t), hipMemcpyHostToDevice));
	h->st_cur = next;
	if (hist) h->src_hist_cur ^= 1;
	h->chan_pos = hd.pos;
	return 0;
}

extern "C" int rtlfm_gpu_sync(rtlfm_gpu *h)
{
	if (!h) return -EINVAL;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(sync_all(h));
	return 0;
}

extern "C" int rtlfm_gpu_set_stream(rtlfm_gpu *h, void *s)
{
	if (!h) return -EINVAL;
	HIP_TRY(sync_all(h));
	h->stream = s ? (hipStream_t)s : h->own_stream;
	// On a caller-owned stream everything the handle launches is ordered on THAT stream: the audio
	// tail does not move to the handle's second stream, so a consumer enqueued on the caller's stream
	// behind rtlfm_gpu_run_device() sees the finished d_out / d_out_len without any further call.
	h->tail_overlap = h->stream == h->own_stream && !h->tail_serial_asked;
	return 0;
}

// Cross-stream ordering without a host synchronisation.  NULL names the legacy default stream
// (what torch's default stream is), which hipEventRecord / hipStreamWaitEvent accept as such.
extern "C" int rtlfm_gpu_wait_for(rtlfm_gpu *h, void *producer_stream)
{
	if (!h) return -EINVAL;
	if ((hipStream_t)producer_stream == h->stream) return 0;
	HIP_TRY(hipSetDevice(h->device));
	OWN_TRY(h->ev_wait.create(hipEventDisableTiming));
	HIP_TRY(hipEventRecord(h->ev_wait, (hipStream_t)producer_stream));
	HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_wait, 0));
	return 0;
}

extern "C" int rtlfm_gpu_release_to(rtlfm_gpu *h, void *consumer_stream)
{
	if (!h) return -EINVAL;
	if ((hipStream_t)consumer_stream == h->stream) return 0;
	HIP_TRY(hipSetDevice(h->device));
	OWN_TRY(h->ev_release.create(hipEventDisableTiming));
	HIP_TRY(hipEventRecord(h->ev_release, h->stream));
	HIP_TRY(hipStreamWaitEvent((hipStream_t)consumer_stream, h->ev_release, 0));
	for (int p = 0; p < 2; p++)  // and for the audio tails still running on their own stream
		if (h->tail_pending[p]) HIP_TRY(hipStreamWaitEvent((hipStream_t)consumer_stream, h->ev_tail[p], 0));
	return 0;
}

extern "C" int rtlfm_gpu_set_path(rtlfm_gpu *h, int path)
{
	if (!h || path < 0 || path > 4) return -EINVAL;
	h->path = path > 2 ? 2 : path;
	if (path == 2) h->fws.pass0_engine = -1;  // the compiled default
	if (path > 2) h->fws.pass0_engine = path - 3;
	return 0;
}
extern "C" int rtlfm_gpu_last_path(rtlfm_gpu *h) { return h ? h->last_path : -EINVAL; }

// What the squelch gate (scan_kernel.h) needs of a configuration: a squelch, and a final PCM row in which buffer b owns the
// samples dec_block_begin(b) .. dec_block_begin(b + 1) - no resampler, no low_pass_simple, no pass that is handed a length
// it does not divide.  (-M raw returns in front of the audio tail: its rows are the decimated I, Q pairs whatever the rest says.)
static int gate_supported(const rtlfm_cfg &c)
{
	if (!c.squelch_level) return -EINVAL;
	if (c.mode != RTLFM_MODE_RAW && (c.rate_out2 > 0 || c.post_downsample > 1)) return -ENOTSUP;
	if (c.downsample_passes > 0 && first_irregular_pass(c) < c.downsample_passes) return -ENOTSUP;
	return 0;
}

// The one place the library's tunables and A/B switches live (no environment look-ups on the
// launch path).  RTLFM_OPTIONS="name=value,..." is applied once, by rtlfm_gpu_create.
static int *option_slot(rtlfm_gpu *h, const char *name)
{
	struct { const char *n; int *p; } tab[] = {
		{"fused_waves", &h->fws.target_waves}, {"fused_waves_tail", &h->fws.target_waves_tail}, {"fused_min_tiles", &h->fws.min_tiles},
		{"fused_tiles_per_seg", &h->fws.tiles_per_seg}, {"fused_debug", &h->fws.debug}, {"fused_gss", &h->fws.gss_x10},
		{"pass0_engine", &h->fws.pass0_engine},
		{"deemph_sequential", &h->opt.deemph_sequential}, {"deemph_four_pass", &h->opt.deemph_four_pass},
		{"lpr_separate", &h->opt.lpr_separate}, {"lpr_scalar_stores", &h->opt.lpr_scalar_stores}, {"lpr_chunk", &h->opt.lpr_chunk},
		{"tail_sync", &h->opt.tail_sync}, {"apart_budget_gb", &h->place.budget_gb}, {"ring_force_retry", &h->place.force_retry},
		{"arb_waves", &h->opt.arb_waves}, {"lpr_threads", &h->opt.lpr_threads}, {"arb_serial", &h->opt.arb_serial}, {"lpr_ring", &h->opt.lpr_ring}, {"squelch_fused", &h->opt.squelch_fused}, {"deep_rest", &h->opt.deep_rest}, {"box_store", &h->fws.box_store}, {"fused_store", &h->fws.fused_store},
		{"verify_twice", &h->opt.verify_twice}, {"verify_inject", &h->opt.verify_inject},
		{"input_stats", &h->opt.input_stats}, {"input_stats_nt", &h->opt.input_stats_nt},
		{"input_health", &h->opt.input_health},
		{"squelch_gate", &h->opt.squelch_gate}, {"conseq_squelch", &h->opt.conseq_squelch},
		{"source_ring", &h->opt.source_ring}, {"pack_results", &h->opt.pack_results}, {"bank_survey", &h->opt.bank_survey},
		{"source_dc", &h->opt.source_dc},
		{"source_stats", &h->opt.source_stats}, {"source_health", &h->opt.source_health},
		{"source_iq", &h->opt.source_iq},
	};
	for (auto &t : tab)
		if (!strcmp(t.n, name)) return t.p;
	return nullptr;
}

extern "C" int rtlfm_gpu_set_option(rtlfm_gpu *h, const char *name, long value)
{
	if (!h || !name) return -EINVAL;
	if (!strcmp(name, "tail_serial")) {
		// the audio tail on the front end's stream instead of its own
		HIP_TRY(sync_all(h));
		h->tail_overlap = value == 0 && h->stream == h->own_stream;
		h->tail_serial_asked = value != 0;
		return 0;
	}
	if (!strcmp(name, "tail_priority")) {
		// the tail's stream re-created with a priority of its own: -1 lowest, 0 default, 1 highest (a stream of another
		// priority never shares a hardware queue with the front end's: LAB.md I.8)
		if (value < -1 || value > 1) return -EINVAL;
		HIP_TRY(sync_all(h));
		int lo = 0, hi = 0;
		HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));  // lo = the numerically greatest = lowest priority
		hipStream_t q = nullptr;
		const int pv = value < 0 ? lo : value > 0 ? hi : 0;
		HIP_TRY(rtl_pool::stream_get(h->device, pv, &q));
		rtl_pool::stream_put(h->device, h->tail_prio_value, h->tail_stream);
		h->tail_stream = q;
		h->tail_priority = (int)value;
		h->tail_prio_value = pv;
		return 0;
	}
	int *slot = option_slot(h, name);
	if (!slot) return -ENOENT;
	// channels on: what reads or owns per-STREAM input rows stays off (rtlfm_gpu_set_channels)
	if (h->chan_per > 0 && value != 0 && (!strcmp(name, "input_stats") || !strcmp(name, "input_health") || !strcmp(name, "squelch_gate")))
		return -ENOTSUP;
	// every range check first: a refused value must leave the handle as it was
	if ((!strcmp(name, "fused_waves") || !strcmp(name, "fused_waves_tail")) && value < 1) return -EINVAL;
	if (!strcmp(name, "pass0_engine") && (value < -1 || value > 1)) return -EINVAL;
	if ((!strcmp(name, "fused_min_tiles") || !strcmp(name, "fused_tiles_per_seg")) && value < 0) return -EINVAL;
	if (!strcmp(name, "apart_budget_gb") && (value < 0 || value > 256)) return -EINVAL;
	if ((!strcmp(name, "box_store") || !strcmp(name, "fused_store")) && (value < -1 || value > 1)) return -EINVAL;
	// the chunk tables of the one-pass deemph + low_pass_real kernel are sized from it: keep it in a sane range
	if (!strcmp(name, "lpr_chunk") && (value < 256 || value > (1 << 20))) return -EINVAL;
	if ((!strcmp(name, "input_stats") || !strcmp(name, "input_stats_nt") || !strcmp(name, "input_health")) && value != 0 && value != 1)
		return -EINVAL;
	if (!strcmp(name, "squelch_gate")) {
		if (value != 0 && value != 1) return -EINVAL;
		if (value == 1) {
			const int g = gate_supported(h->cfg);
			if (g < 0) return g;
			if (h->opt.pack_results == 2) return -EINVAL;  // mode 2 reads uncompacted rows
		}
	}
	if (!strcmp(name, "pack_results")) {
		if (value < 0 || value > 2) return -EINVAL;
		if (value == 2) {
			const int g = gate_supported(h->cfg);  // the rule needs what the gate needs ...
			if (g < 0) return g;
			if (h->opt.squelch_gate) return -EINVAL;  // ... but not the gate's rows: they are compacted already
		}
		if (ingest_busy(h)) return -EBUSY;
		h->opt.pack_results = (int)value;
		return value == 0 ? ingest_pack_free(h) : 0;
	}
	if (!strcmp(name, "bank_survey")) {
		if (value != 0 && value != 1) return -EINVAL;
		if (ingest_busy(h)) return -EBUSY;
		h->opt.bank_survey = (int)value;
		return value == 0 ? survey_free(h, true) : 0;
	}
	if (!strcmp(name, "source_dc")) {
		// (include/rtlfm_hip.h: every refusal leaves the handle as it was)
		if (value != 0 && value != 1) return -EINVAL;
		if (value == 1 && (h->cfg.rdc_block_const < 0 || h->cfg.rdc_block_const > 65535)) return -EINVAL;
		if (h->cfg.dc_block_raw) return -ENOTSUP;
		if (ingest_busy(h) || (h->opt.source_ring && ingest_queued(h))) return -EBUSY;
		if (value == 1 && h->fir_ntaps > 0 && rtlfm_channel_filter_check_dc(h->fir_taps.data(), h->fir_ntaps, h->fir_shift) < 0) return -ERANGE;
		if (value == 1 && h->bank_K > 0 &&
		    rtlfm_channel_bank_check_dc(h->bank_K, h->bank_taps.data(), h->bank_ntaps, h->bank_shift) < 0)
			return -ERANGE;
		HIP_TRY(hipSetDevice(h->device));
		HIP_TRY(sync_all(h));
		if (value == 1) {
			int r = ensure_source_dc(h);
			if (r < 0) return r;
		}
		h->opt.source_dc = (int)value;
		return history_clear(h);  // (the history belongs to the old rule; the records stay)
	}
	if (!strcmp(name, "source_stats") || !strcmp(name, "source_health")) {
		// (they read source rows and act only on runs that channels take: free to set with channels off.  Setting 0 frees
		// nothing; the records are allocated by the first run that needs them)
		if (value != 0 && value != 1) return -EINVAL;
		if (ingest_busy(h)) return -EBUSY;
		*slot = (int)value;
		return 0;
	}
	if (!strcmp(name, "source_iq")) {
		// (include/rtlfm_hip.h: acts only on runs that channels take, free to set with channels off; the history stays)
		if (value != 0 && value != 1) return -EINVAL;
		if (ingest_busy(h) || (h->opt.source_ring && ingest_queued(h))) return -EBUSY;
		HIP_TRY(hipSetDevice(h->device));
		HIP_TRY(sync_all(h));
		h->opt.source_iq = (int)value;
		h->siq_nblocks = 0;
		if (value == 0) {  // the rows and the records go; the coefficients stay as they rule
			h->d_siq_rows.reset();
			h->d_siq_sums.reset();
			h->siq_stride = 0;
		}
		return 0;
	}
	if (!strcmp(name, "conseq_squelch") && (value < 0 || value > INT32_MAX - 1)) return -EINVAL;
	if (!strcmp(name, "source_ring")) {
		// the ring's rows change with it while channels are on: only on a ring that holds nothing and is in the middle of nothing
		if (value != 0 && value != 1) return -EINVAL;
		if (ingest_busy(h) || ingest_queued(h)) return -EBUSY;
		h->opt.source_ring = (int)value;
		return ingest_resize(h);
	}
	if (!strcmp(name, "arb_waves") && (value < 0 || value > kSpecArbMaxWaves)) return -EINVAL;
	if (!strcmp(name, "lpr_threads") && (value < 64 || value > kSpecLprThreads || value % 64)) return -EINVAL;
	if (!strcmp(name, "arb_serial")) {
		if (value < -1 || value > 1) return -EINVAL;
		HIP_TRY(sync_all(h));  // the tail may change streams: nothing of either in flight
	}
	// ... then what an accepted value implies
	if (!strcmp(name, "fused_waves")) h->fws.target_waves_tail = (int)value;  // one number for both unless fused_waves_tail follows
	if (!strcmp(name, "fused_waves") || !strcmp(name, "fused_waves_tail")) h->fws.target_waves_tail_fifth = 0;  // an explicit number rules
	if (!strcmp(name, "fused_waves") || !strcmp(name, "fused_min_tiles")) h->fws.plan_by_caller = true;       // ... and so do these
	*slot = (int)value;
	return 0;
}

extern "C" int rtlfm_gpu_get_option(rtlfm_gpu *h, const char *name, long *value)
{
	if (!h || !name || !value) return -EINVAL;
	if (!strcmp(name, "tail_serial")) { *value = h->tail_overlap ? 0 : 1; return 0; }
	if (!strcmp(name, "tail_priority")) { *value = h->tail_priority; return 0; }
	// read-only: where the write streams' buffers ended up (rtlfm_gpu_malloc_apart_ex) and what finding out cost
	if (!strcmp(name, "ring_apart")) { *value = h->place.ring_apart; return 0; }
	if (!strcmp(name, "ring_tries")) { *value = h->place.ring_tries; return 0; }
	if (!strcmp(name, "poison")) { *value = rtl_debug::poison_on() ? 1 : 0; return 0; }  // RTLFM_POISON=1 (debug_poison.h)
	if (!strcmp(name, "res_apart")) { *value = h->place.res_apart; return 0; }
	if (!strcmp(name, "deep_apart")) { *value = h->place.deep_apart; return 0; }
	if (!strcmp(name, "placement_ms")) { *value = (long)(h->place.search_ms + 0.5); return 0; }
	if (!strcmp(name, "placement_walked_mb")) { *value = (long)(h->place.walked_peak >> 20); return 0; }
	if (!strcmp(name, "placement_held_mb")) { *value = placement_held_mb(h); return 0; }
	if (!strcmp(name, "verify_mismatches")) { *value = h->vt_mismatches; return 0; }  // verify_twice: runs whose two executions differed
	if (!strcmp(name, "verify_runs")) { *value = h->vt_runs; return 0; }
	if (!strcmp(name, "last_route")) { *value = h->last_route; return 0; }  // the plan the last run took (enum rtlfm_route / rtlfm_rest)
	if (!strcmp(name, "last_rest")) { *value = h->last_rest; return 0; }
	if (!strcmp(name, "block_len")) { *value = (long)h->cfg.block_len; return 0; }  // what the handle was created with
	if (!strcmp(name, "pack_us")) return ingest_pack_us(h, value);
	// debugging (tests/test_soak_gpu.py): the host addresses of the runtime objects the handle owns - a hipStream_t / hipEvent_t
	// IS the address of the runtime's object, which the runtime frees when the handle is destroyed
	if (!strcmp(name, "dbg_own_stream")) { *value = (long)(uintptr_t)h->own_stream; return 0; }
	if (!strcmp(name, "dbg_tail_stream")) { *value = (long)(uintptr_t)h->tail_stream; return 0; }
	if (!strncmp(name, "dbg_event", 9) && name[9] >= '0' && name[9] <= '5' && !name[10]) {
		const hipEvent_t ev[6] = {h->ev_wait, h->ev_release, h->ev_front[0], h->ev_front[1], h->ev_tail[0], h->ev_tail[1]};
		*value = (long)(uintptr_t)ev[name[9] - '0'];
		return 0;
	}
	if (!strcmp(name, "dbg_handle")) { *value = (long)(uintptr_t)h; return 0; }
	if (!strcmp(name, "dbg_handle_bytes")) { *value = (long)sizeof(*h); return 0; }
	int *slot = option_slot(h, name);
	if (!slot) return -ENOENT;
	*value = *slot;
	return 0;
}

static int options_from_env(rtlfm_gpu *h)
{
	const char *e = getenv("RTLFM_OPTIONS");
	if (!e || !*e) return 0;
	std::string all(e);
	size_t at = 0;
	while (at < all.size()) {
		size_t end = all.find(',', at);
		if (end == std::string::npos) end = all.size();
		const std::string kv = all.substr(at, end - at);
		const size_t eq = kv.find('=');
		if (eq != std::string::npos) {
			int r = rtlfm_gpu_set_option(h, kv.substr(0, eq).c_str(), atol(kv.c_str() + eq + 1));
			if (r < 0) { fprintf(stderr, "rtlfm_hip: RTLFM_OPTIONS: '%s' not accepted (%d)\n", kv.c_str(), r); return r; }
		}
		at = end + 1;
	}
	return 0;
}

extern "C" int rtlfm_gpu_timing_enable(rtlfm_gpu *h, int on)
{
	if (!h) return -EINVAL;
	h->timing = on != 0;
	return 0;
}

static int report_clock_stamps(rtlfm_gpu *h);

extern "C" int rtlfm_gpu_timing_read(rtlfm_gpu *h, double *front_ms, int *launches)
{
	if (!h) return -EINVAL;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(sync_all(h));
	if (h->fws.stamps && (h->fws.debug & 16)) {
		int r2 = report_clock_stamps(h);
		if (r2 < 0) return r2;
	}
	double total = 0;
	int n = 0;
	for (auto &p : h->ev_pending) {
		float ms = 0;
		HIP_TRY(hipEventElapsedTime(&ms, p.first, p.second));
		total += ms;
		n++;
		h->ev_free.push_back(std::move(p));
	}
	h->ev_pending.clear();
	if (front_ms) *front_ms = total;
	if (launches) *launches = n;
	return 0;
}

static int timing_begin(rtlfm_gpu *h, std::pair<Event, Event> &ev)
{
	if (!h->timing) return 0;
	if (!h->ev_free.empty()) {
		ev = std::move(h->ev_free.back());
		h->ev_free.pop_back();
	} else {
		OWN_TRY(ev.first.create());
		OWN_TRY(ev.second.create());
	}
	HIP_TRY(hipEventRecord(ev.first, h->stream));
	return 0;
}
static int timing_end(rtlfm_gpu *h, std::pair<Event, Event> &ev)
{
	if (!h->timing) return 0;
	HIP_TRY(hipEventRecord(ev.second, h->stream));
	h->ev_pending.push_back(std::move(ev));
	return 0;
}

// ------------------------------------------------------------ the chain ----

static inline int grid_for(size_t work, int block = 256, int cap = 256 * 16)
{
	size_t g = (work + block - 1) / block;
	if (g < 1) g = 1;
	if (g > (size_t)cap) g = cap;
	return (int)g;
}

// Audio tail shared by both paths: everything full_demod() does after
// mode_demod() (src/rtl_fm.c:1260-1271).  `src` holds per-stream demodulated
// samples (uniform count T, or per-stream d_cnt when `varcnt`); the final
// result is left in dst with dst_stride and its per-stream length in
// d_out_len (may be NULL).
// (TailPlan, plan_tail: run_plan.h - a run's plan holds it.)  What run_tail asks again while it runs:
static rtlfm_route_opts route_opts(const rtlfm_gpu *h);
static bool deemph_scans(const rtlfm_gpu *h, int T) { return plan::deemph_scans(h->cfg, route_opts(h), T); }
static bool arb_tail_in_line(const rtlfm_gpu *h, const TailPlan &tp) { return plan::arb_tail_in_line(h->cfg, route_opts(h), h->nstreams, tp); }

// Where mode_demod() should write so that the chain ends in `final`.
static void tail_route(rtlfm_gpu *h, const TailPlan &tp, int16_t *final_dst, size_t final_stride,
                       int16_t **demod_dst, size_t *demod_stride)
{
	if (tp.oop() == 0) {
		*demod_dst = final_dst;
		*demod_stride = final_stride;
	} else {
		*demod_dst = h->res[h->step & 1][0];
		*demod_stride = h->tstride;
	}
}

// The form deemph_filter takes in a run, with the resampler where one kernel does both: decided ONCE, at the top of
// run_tail(), from the plan and the run as the front end left it.
enum class Deemph {
	none,
	identity,       // a == 1: the filter is the identity on the samples and keeps the last one (k_deemph_identity)
	sequential,     // a lane per stream (k_deemph): short runs, ragged views, an interval of candidate states beyond a wave
	spec,           // nothing behind it, a long run: one pass OUT of place (k_deemph_spec) - plan_tail()'s promise
	spec_lpr,       // the whole tail as one kernel: filter + low_pass_real (k_deemph_spec_lpr, -M wbfm)
	spec_arb,       // the whole tail as one kernel: filter + arbitrary_upsample (k_deemph_spec_arb, config 3)
	four_pass,      // few, long streams: parallel over time, in place (k_deemph_scan_a1 / _a2 / _b / _c)
	four_pass_lpr,  // ... the filtered samples going straight into low_pass_real's accumulator (k_deemph_scan_c_lpr)
};
// The one-kernel tails write every field a tail of their configuration owns, for every stream, and the counts.
static bool whole_tail(Deemph d) { return d == Deemph::spec_lpr || d == Deemph::spec_arb; }

// deemph_a as the kernels take it: the step's constants, the form of its division (the kernels' MAGIC: 0 a division,
// 1 a multiply-high, 2 a shift) and the samples a one-pass kernel settles over in front of a chunk
struct DeemphForm { DeemphStep st; int M, Ws; };
static DeemphForm deemph_form(int a)
{
	DeemphForm f{};
	f.st.a = (uint32_t)a; f.st.half = (uint32_t)(a / 2);
	const bool pow2 = a >= 1 && a <= 32768 && (a & (a - 1)) == 0;
	const bool magic = !pow2 && a >= 2 && a <= 32768;
	if (pow2) { while ((1u << f.st.magic) < f.st.a) f.st.magic++; }
	else if (magic) f.st.magic = (uint32_t)((0x100000000ull + f.st.a - 1) / f.st.a);
	f.M = pow2 ? 2 : magic ? 1 : 0;
	f.Ws = a <= 32768 ? ((16 * a + 64 + 63) / 64) * 64 : 0;  // (the kernels that settle run for 2 a + 2 <= kDeemphGap only)
	return f;
}
// ... and that form as a constant: with_magic(M, [&](auto mm) { k<decltype(mm)::value><<<...>>>(...); })
template <class F>
static void with_magic(int M, F &&launch)
{
	if (M == 2) launch(std::integral_constant<int, 2>{});
	else if (M == 1) launch(std::integral_constant<int, 1>{});
	else launch(std::integral_constant<int, 0>{});
}

// What the stages of one tail share: its queue, the state copies, and the samples where they stand now.
// Buffer extents: buffer b of a stream owns the decimated samples [dec_block_begin(b),
// dec_block_begin(b + 1)) of the run — Nblk input samples per buffer through a boxcar D with the
// carried prev_index; (Nblk, 1) describes a uniform count of Nblk per buffer.
struct TailRun {
	rtlfm_gpu *h;
	const rtlfm_cfg &c;
	int S;
	hipStream_t q;
	const state_t *sin;
	state_t *sout;
	int16_t *cur; size_t cur_stride;
	int T; int32_t *cnt;  // samples per stream; the per-stream counts where they differ (T is then their upper bound)
	int nblocks, Nblk, D;
	int16_t *final_dst; size_t final_stride;
	int remaining_oop;    // out-of-place stages still to come: the last of them writes final_dst
	int16_t *dst; size_t dst_stride;  // where the out-of-place stage at hand writes (out_of_place() ... arrived())
	void out_of_place()
	{
		const DevBuf<int16_t> *res = h->res[h->step & 1];
		dst = --remaining_oop == 0 ? final_dst : cur == res[0] ? res[1] : res[0];
		dst_stride = remaining_oop == 0 ? final_stride : h->tstride;
	}
	void arrived() { cur = dst; cur_stride = dst_stride; }
	void stage_done(const char *what) const  // option tail_sync
	{
		if (h->opt.tail_sync) fprintf(stderr, "rtlfm_hip[tail]: %s done (%s)\n", what, hipGetErrorString(hipStreamSynchronize(q)));
	}
};

static Deemph deemph_route(const TailPlan &tp, const DeemphForm &f, const TailRun &r)
{
	const rtlfm_gpu *h = r.h;
	if (!tp.deemph) return Deemph::none;
	if (r.c.deemph_a == 1) return Deemph::identity;
	// plan_tail() promised the out-of-place stage from an upper bound of T before the front end ran, and the routing
	// (oop()) is built on it: tail_deemph_spec() keeps the promise for the runs that turn out otherwise
	if (tp.deemph_spec) return Deemph::spec;
	if (!deemph_scans(h, tp.post ? r.T / r.c.post_downsample : r.T)) return Deemph::sequential;
	if (!tp.post && !tp.adc && !h->opt.deemph_four_pass) {
		// One pass where the resampler follows directly: every chunk finds its incoming state from the W samples before
		// it (staged_kernels.h, k_deemph_spec_lpr); a stream it cannot settle that way (silence) is redone by the
		// kernel's own last lane for that stream.
		if (tp.lpr && !h->opt.lpr_separate) return Deemph::spec_lpr;
		// ... and where arbitrary_resample follows directly, on uniform buffers that it upsamples (config 3): one pass from
		// the demodulated samples to the resampled output (k_deemph_spec_arb)
		const int arb_l2 = (int)((long long)r.Nblk * r.c.rate_out2 / r.c.rate_out);
		if (tp.arb && r.D == 1 && !r.cnt && r.Nblk >= 2 && arb_l2 > r.Nblk && (long long)(r.Nblk + 1) * arb_l2 < (1ll << 31) && f.Ws <= 256 &&
		    (uintptr_t)r.cur % 16 == 0 && r.cur_stride % 8 == 0 && r.T == r.nblocks * r.Nblk)
			return Deemph::spec_arb;
	}
	return tp.lpr && !tp.adc && !h->opt.lpr_separate ? Deemph::four_pass_lpr : Deemph::four_pass;
}

// Samples per lane of a one-pass kernel: `want` where the run fills the GPU that way (-M wbfm at 1024 streams: 64 K lanes);
// with fewer samples in all, shorter chunks - about 64 K lanes again, never so short that the settling (Ws samples walked
// twice per chunk) outweighs the chunk (256 streams of rtl_fm -s 48k -r 24k -E deemp: 294 waves on 1024 SIMDs took 1.45 ms
// for 102 M samples)
static int fit_chunk(int want, int S, int T, int Ws)
{
	const long long fit = std::max((long long)S * T / 65536, std::max(6ll * Ws, 512ll));
	return fit < want ? (int)fit : want;
}

static void tail_deemph_sequential(TailRun &r, const DeemphForm &f)
{
	with_magic(f.M, [&](auto mm) {
		k_deemph<decltype(mm)::value><<<(unsigned)((r.S + 63) / 64), 64, 0, r.q>>>(r.cur, r.cur_stride, r.T, r.cnt, r.S, f.st, r.sin, r.sout);
	});
}

// deemph_filter with no resampler behind it, a long run: ONE pass, out of place (staged_kernels.h, k_deemph_spec)
static int tail_deemph_spec(TailRun &r, const DeemphForm &f)
{
	r.out_of_place();
	const bool congruent = (((uintptr_t)r.cur ^ (uintptr_t)r.dst) & 15) == 0 && ((r.cur_stride * 2) & 15) == ((r.dst_stride * 2) & 15);
	if (deemph_scans(r.h, r.T) && congruent) {
		const int Lc = (fit_chunk(r.h->opt.lpr_chunk, r.S, r.T, f.Ws) + 63) & ~63;  // whole 128-byte rounds
		const int mcd = r.T / Lc + 2;
		const int spw = mcd >= kSpecLprThreads ? 1 : kSpecLprThreads / mcd;
		with_magic(f.M, [&](auto mm) {
			k_deemph_spec<decltype(mm)::value><<<(unsigned)((r.S + spw - 1) / spw), kSpecLprThreads, 0, r.q>>>(
			    r.cur, r.cur_stride, r.dst, r.dst_stride, r.T, r.cnt, r.S, f.st, mcd, Lc, f.Ws, r.sin, r.sout);
		});
		r.stage_done("one pass (deemph)");
	} else {
		// (the plan promised an out-of-place stage and the run turned out otherwise - rows that do not share their
		// alignment, a run that is shorter than planned: the sequential filter in place, then a copy)
		tail_deemph_sequential(r, f);
		r.stage_done("sequential");
		HIP_TRY(hipMemcpy2DAsync(r.dst, r.dst_stride * sizeof(int16_t), r.cur, r.cur_stride * sizeof(int16_t), (size_t)r.T * sizeof(int16_t), r.S,
		                         hipMemcpyDeviceToDevice, r.q));
	}
	r.arrived();
	return 0;
}

// (i, frac) of every output of a buffer, as arbitrary_upsample's loop (src/rtl_fm.c:1114-1135) has them when it writes
// buf2[j]: walked once here, shared by every stream and buffer
// (d_arb_i: the i, a gap, then the padded LDS offset of sample i - 1 for k_deemph_spec_arb's resampler)
static int arb_tables(rtlfm_gpu *h, hipStream_t q, int Nblk, int arb_l2)
{
	if (h->arb_len2 == arb_l2 && h->arb_len1 == Nblk) return 0;
	std::vector<int32_t> ti(2 * (size_t)arb_l2 + kArbTabGap);
	std::vector<double> tf((size_t)arb_l2);
	int i = 1, tick = 0;
	for (int j = 0; j < arb_l2; j++) {
		ti[j] = i;
		tf[j] = (double)tick / (double)arb_l2;
		ti[(size_t)arb_l2 + kArbTabGap + j] = 2 * i + 16 * (i >> 5) - 2;
		tick += Nblk;
		if (tick > arb_l2) { tick -= arb_l2; i++; }
		if (i >= Nblk) { i = Nblk - 1; tick = arb_l2; }
	}
	h->arb_len2 = 0; h->arb_len1 = 0;  // (no key to the tables until both hold the new geometry)
	if (h->d_arb_i) HIP_TRY(hipStreamSynchronize(q));  // (the tables of another geometry may still be in use)
	OWN_TRY(h->d_arb_i.grow(ti.size(), q));
	OWN_TRY(h->d_arb_frac.grow(tf.size(), q));
	HIP_TRY(hipMemcpy(h->d_arb_i, ti.data(), ti.size() * sizeof(int32_t), hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(h->d_arb_frac, tf.data(), tf.size() * sizeof(double), hipMemcpyHostToDevice));
	h->arb_len2 = arb_l2; h->arb_len1 = Nblk;
	return 0;
}

// The one operation of config 3's tail: filter, resampler, state and counts
static int tail_deemph_spec_arb(TailRun &r, const DeemphForm &f, int32_t *cnt_dst)
{
	rtlfm_gpu *h = r.h;
	const int arb_l2 = (int)((long long)r.Nblk * r.c.rate_out2 / r.c.rate_out);
	const size_t arb_lds = (size_t)(f.Ws / kArbChunk + 64) * kArbStride * sizeof(int16_t);
	const int e = arb_tables(h, r.q, r.Nblk, arb_l2);
	if (e < 0) return e;
	r.out_of_place();
	const int nspans = (r.T + 64 * kArbChunk - 1) / (64 * kArbChunk);
	// a workgroup per stream (nothing crosses workgroups), its spans dealt to up to eight waves: about 16384
	// waves in all - two and a half rounds of what the GPU holds, so that the last round is a small part of
	// the launch (8192: config 3's tail alone 70 us instead of 65, LAB.md I.31)
	const int wpw = std::max(1, std::min({h->opt.arb_waves > 0 ? h->opt.arb_waves : 16384 / r.S, nspans, kSpecArbMaxWaves}));
	auto launch = [&](auto mm) {
		k_deemph_spec_arb<decltype(mm)::value><<<(unsigned)r.S, 64 * wpw, arb_lds * wpw, r.q>>>(
		    r.cur, r.cur_stride, r.T, r.S, f.st, f.Ws, nspans, r.Nblk, arb_l2, r.nblocks, h->d_arb_i, h->d_arb_frac, r.dst, r.dst_stride, r.sin,
		    r.sout, arb_lds, cnt_dst);
	};
	// a == 2 (rtl_fm -s 24k -E deemp): the filter step is (x + avg + [x > avg]) >> 1
	if (r.c.deemph_a == 2) launch(std::integral_constant<int, 3>{});
	else with_magic(f.M, launch);
	r.stage_done("one pass (arb)");
	r.arrived();
	return 0;
}

// The one operation of -M wbfm's tail
static int tail_deemph_spec_lpr(TailRun &r, const DeemphForm &f, int32_t *cnt_dst)
{
	rtlfm_gpu *h = r.h;
	const int T = r.T;
	// chunk length of the one-pass form: about 2720 samples (2040: +1 %, 1360: +2 % on the wbfm step),
	// and a multiple of the resampler's period fast / gcd(fast, slow) where that is short - then all
	// chunks of a stream start at the same phase, the lanes of a wave emit at the same samples and
	// the emission branch is taken by whole waves instead of by a few lanes every sample
	const int Lwant = fit_chunk(h->opt.lpr_chunk, r.S, T, f.Ws);  // lpr_chunk: 256 .. 2^20 (rtlfm_gpu_set_option)
	int Ls = Lwant;
	int mcsp;
	long long gg = r.c.rate_out, bb = r.c.rate_out2;
	while (bb) { const long long t = gg % bb; gg = bb; bb = t; }
	long long per = r.c.rate_out / gg;
	while (per % 8) per *= 2;
	if ((long long)T >= 48ll * Lwant) {
		// long runs: a stream's chunks fill whole waves.  (T / 2720 + 2 = 130 chunks of the wbfm shape were two
		// full waves and a third with ONE busy lane that issued every instruction of the walk again:
		// SQ_INSTS_VALU 23.8 lane-operations per sample against 18.4 with packed lanes.)
		const int n64 = (int)(((long long)T + 32ll * Lwant) / (64ll * Lwant));
		const int lanes = 64 * (n64 < 1 ? 1 : n64);
		long long L0 = ((long long)T + lanes - 1) / lanes;
		L0 = per <= L0 ? per * ((L0 + per - 1) / per) : ((L0 + 7) & ~7ll);
		Ls = (int)L0;
		mcsp = lanes;
	} else {
		if (per <= Lwant) Ls = (int)(per * ((Lwant + per / 2) / per));
		mcsp = T / Ls + 2;
	}
	OWN_TRY(h->d_lpr_chunks.grow((size_t)r.S * mcsp, r.q));
	r.out_of_place();
	// outputs leave in 64-byte pieces through LDS (2; any row alignment), else in 16-byte groups where the rows allow
	// it (1), else one by one (staged_kernels.h, LprSink)
	int lpr_vec = (uintptr_t)r.dst % 16 == 0 && r.dst_stride % 8 == 0 && !h->opt.lpr_scalar_stores;
	if (h->opt.lpr_ring && !h->opt.lpr_scalar_stores) lpr_vec = 2;
	const int nthr = h->opt.lpr_threads;
	const size_t lpr_lds = lpr_vec == 2 ? (size_t)nthr * kLprRingStride * sizeof(int16_t) : 0;
	// a workgroup owns whole streams: 256 / chunks of them, or one with a loop over its chunks
	const int spw = mcsp >= nthr ? 1 : nthr / mcsp;
	with_magic(f.M, [&](auto mm) {
		k_deemph_spec_lpr<decltype(mm)::value><<<(unsigned)((r.S + spw - 1) / spw), nthr, lpr_lds, r.q>>>(
		    r.cur, r.cur_stride, T, r.cnt, r.S, f.st, mcsp, Ls, f.Ws, r.dst, r.dst_stride, r.c.rate_out, r.c.rate_out2, r.sin, r.sout,
		    h->d_lpr_chunks, lpr_vec, cnt_dst);
	});
	r.stage_done("one pass (lpr)");
	r.arrived();
	return 0;
}

// The four passes, for every stream; with `fuse_lpr` the last one is low_pass_real too (counts in d_cnt2)
static int tail_deemph_four_pass(TailRun &r, const DeemphForm &f, bool fuse_lpr)
{
	rtlfm_gpu *h = r.h;
	const int S = r.S, T = r.T, fast = r.c.rate_out, slow = r.c.rate_out2;
	// chunk length: each of the passes A1 and C is one chunk long in time; a chunk must be
	// long enough for the interval to contract (~100 samples) and, normally, to merge
	const int L = T >= 8192 ? 1024 : 512;
	const int mc = T / L + 2;
	OWN_TRY(h->d_deemph_tab.grow((size_t)S * mc, r.q));
	OWN_TRY(h->d_deemph_inc.grow((size_t)S * mc, r.q));
	if (fuse_lpr) OWN_TRY(h->d_lpr_chunks.grow((size_t)S * mc, r.q));
	if (fuse_lpr) r.out_of_place();
	const int lpr_vec = fuse_lpr && (uintptr_t)r.dst % 16 == 0 && r.dst_stride % 8 == 0 && !h->opt.lpr_scalar_stores;
	int lpc = 8;  // lanes per chunk in pass A2: the contracted interval (<= 2a + 2 states) must fit
	while (lpc < 2 * r.c.deemph_a + 3) lpc *= 2;
	const size_t per_wave = 64 / lpc;
	const unsigned ga = (unsigned)(((size_t)S * mc + per_wave - 1) / per_wave), gc = (unsigned)(((size_t)S * mc + 63) / 64);
	with_magic(f.M, [&](auto mm) {
		constexpr int MM = decltype(mm)::value;
		k_deemph_scan_a1<MM><<<gc, 64, 0, r.q>>>(r.cur, r.cur_stride, T, r.cnt, S, f.st, mc, L, lpc, h->d_deemph_tab);
		r.stage_done("a1");
		k_deemph_scan_a2<MM><<<ga, 64, 0, r.q>>>(r.cur, r.cur_stride, T, r.cnt, S, f.st, mc, L, lpc, h->d_deemph_tab);
		r.stage_done("a2");
		k_deemph_scan_b<MM><<<gc, 64, 0, r.q>>>(r.cur, r.cur_stride, T, r.cnt, S, f.st, mc, L, h->d_deemph_tab, h->d_deemph_inc, r.sin, r.sout);
		r.stage_done("b");
		if (fuse_lpr) {
			k_deemph_scan_c_lpr<MM><<<gc, 64, 0, r.q>>>(r.cur, r.cur_stride, T, r.cnt, S, f.st, mc, L, h->d_deemph_inc, r.dst, r.dst_stride, fast, slow,
			                                           r.sin, r.sout, h->d_lpr_chunks, lpr_vec);
			k_lpr_fixup<<<gc, 64, 0, r.q>>>(r.cur, r.cur_stride, T, r.cnt, S, mc, L, h->d_lpr_chunks, r.dst, r.dst_stride, fast, slow, r.sin, r.sout,
			                              h->d_cnt2);
		} else {
			k_deemph_scan_c<MM><<<gc, 64, 0, r.q>>>(r.cur, r.cur_stride, T, r.cnt, S, f.st, mc, L, h->d_deemph_inc, r.sout);
		}
		r.stage_done("c");
	});
	if (fuse_lpr) r.arrived();
	return 0;
}

// The tail in order: post -> de-emphasis (in some forms with its resampler) -> -E dc -> resampler -> counts.
// (T, varcnt, nblocks, Nblk, D: the run as the front end left it, see TailRun.)
static int run_tail(rtlfm_gpu *h, const TailPlan &tp, int16_t *cur, size_t cur_stride, int T, bool varcnt,
                    int nblocks, int Nblk, int D, int16_t *final_dst, size_t final_stride, int32_t *d_out_len)
{
	const rtlfm_cfg &c = h->cfg;
	const int S = h->nstreams;
	const int par = (int)(h->step & 1);
	TailRun r{h, c, S, h->stream, h->st[h->st_cur], h->st[(h->st_cur + 1) % 3], cur, cur_stride, T, varcnt ? h->d_cnt[par] : nullptr,
	          nblocks, Nblk, D, final_dst, final_stride, tp.oop(), nullptr, 0};
	const DeemphForm f = deemph_form(c.deemph_a);
	const Deemph form = deemph_route(tp, f, r);
	// The tail runs behind the front end on a stream of its own, so that the front end of the next
	// step (a different res[] set, d_cnt[] and state copy, see struct rtlfm_gpu) overlaps it: at
	// config 3 the tail is a quarter of the step but 3 % of the bytes.  rtlfm_gpu_run_device() makes
	// the step after next wait for it before it reuses this parity's buffers.
	// ... but config 3's own tail in line (arb_tail_in_line above)
	const bool own_stream = tp.any() && h->tail_overlap && !arb_tail_in_line(h, tp);
	if (own_stream) {
		HIP_TRY(hipEventRecord(h->ev_front[par], h->stream));
		HIP_TRY(hipStreamWaitEvent(h->tail_stream, h->ev_front[par], 0));
		r.q = h->tail_stream;
		// The front end copied the whole record sin -> sout while the previous step's tail may still
		// have been writing the tail's fields of sin.  The tail stream is in order, so here those are
		// final: carry them over before any stage of this tail runs (a stage that leaves a field
		// alone - a skipped stream - then leaves the right value behind).
		// The one-kernel tails write every field a tail of their configuration owns, for every stream: no copy.
		if (!whole_tail(form)) k_tail_state_copy<<<grid_for(S, 64), 64, 0, r.q>>>(r.sin, r.sout, S);
	}
	struct Done {  // whatever path leaves: mark the end of this step's tail
		rtlfm_gpu *h; int par; bool on;
		~Done() { if (on && hipEventRecord(h->ev_tail[par], h->tail_stream) == hipSuccess) h->tail_pending[par] = true; }
	} done{h, par, own_stream};
	if (tp.post) {
		// low_pass_simple: "length must be multiple of step" (src/rtl_fm.c:740) — validate_cfg only
		// lets uniform per-buffer counts through
		r.out_of_place();
		r.T /= c.post_downsample;
		k_post_downsample<<<grid_for((size_t)S * r.T), 256, 0, r.q>>>(r.cur, r.cur_stride, r.dst, r.dst_stride, r.T, S, c.post_downsample);
		r.stage_done("post");
		r.arrived();
		r.Nblk = r.T / nblocks; r.D = 1;
	}
	int32_t *cnt_dst = d_out_len ? d_out_len : h->d_cnt2;  // where a one-kernel tail leaves the counts
	int e = 0;
	switch (form) {
	case Deemph::none: break;
	case Deemph::identity: k_deemph_identity<<<grid_for(S, 64), 64, 0, r.q>>>(r.cur, r.cur_stride, r.T, r.cnt, S, r.sout); r.stage_done("identity"); break;
	case Deemph::sequential: tail_deemph_sequential(r, f); r.stage_done("sequential"); break;
	case Deemph::spec: e = tail_deemph_spec(r, f); break;
	case Deemph::spec_lpr: e = tail_deemph_spec_lpr(r, f, cnt_dst); break;
	case Deemph::spec_arb: e = tail_deemph_spec_arb(r, f, cnt_dst); break;
	case Deemph::four_pass: e = tail_deemph_four_pass(r, f, false); break;
	case Deemph::four_pass_lpr: e = tail_deemph_four_pass(r, f, true); break;
	}
	if (e < 0) return e;
	if (tp.adc) {
		// dc_block_audio_filter (src/rtl_fm.c:1028-1041): sums per buffer, then the smoothing recurrence and the subtraction
		// in one launch (staged_kernels.h, k_adc_smooth_apply)
		k_adc_sums<<<S * nblocks, 256, 0, r.q>>>(r.cur, r.cur_stride, r.Nblk, r.D, nblocks, r.sin, h->d_adc_sums);
		k_adc_smooth_apply<<<S * nblocks, 256, (size_t)(nblocks + 1) * sizeof(int32_t), r.q>>>(r.cur, r.cur_stride, r.Nblk, r.D, nblocks,
		                                                                                    c.adc_block_const, h->d_adc_sums, r.sin, r.sout);
		r.stage_done("adc");
	}
	const bool resampled = whole_tail(form) || form == Deemph::four_pass_lpr;
	if (tp.lpr && !resampled) {
		r.out_of_place();
		const int maxout = (int)(((long long)c.rate_out - 1 + (long long)r.T * c.rate_out2) / c.rate_out);
		k_low_pass_real<<<grid_for((size_t)S * (maxout + 1)), 256, 0, r.q>>>(r.cur, r.cur_stride, r.dst, r.dst_stride, r.T, r.cnt, S, c.rate_out,
		                                                                   c.rate_out2, r.sin, r.sout, h->d_cnt2);
		r.stage_done("lpr");
		r.arrived();
	} else if (tp.arb && !resampled) {
		// arbitrary_resample per buffer on whatever result_len it has (src/rtl_fm.c:1168-1177, 1270)
		r.out_of_place();
		const int nlo = r.Nblk / r.D, nhi = (r.Nblk % r.D) ? nlo + 1 : nlo;
		const int l2lo = (int)((long long)nlo * c.rate_out2 / c.rate_out);
		const int l2hi = (int)((long long)nhi * c.rate_out2 / c.rate_out);
		const bool any_up = nlo < l2lo || nhi < l2hi, any_down = !(nlo < l2lo) || !(nhi < l2hi);
		const ArbPlan ap{r.Nblk, r.D, nlo, l2lo, (int)((long long)(nlo + 1) * c.rate_out2 / c.rate_out)};
		if (any_up)
			k_arb_upsample<<<grid_for((size_t)S * nblocks * l2hi), 256, 0, r.q>>>(r.cur, r.cur_stride, r.dst, r.dst_stride, ap, l2hi, nblocks, S, r.sin,
			                                                                     h->d_cnt2);
		if (any_up) r.stage_done("arb up");
		if (any_down)
			k_arb_downsample<<<grid_for((size_t)S * nblocks, 64), 64, 0, r.q>>>(r.cur, r.cur_stride, r.dst, r.dst_stride, ap, nblocks, S, r.sin, h->d_cnt2);
		if (any_down) r.stage_done("arb down");
		r.arrived();
	}
	if (r.cur != final_dst) return -EFAULT;  // routing bug
	if (!d_out_len || whole_tail(form)) return 0;
	if (tp.lpr || tp.arb)
		HIP_TRY(hipMemcpyAsync(d_out_len, h->d_cnt2, S * sizeof(int32_t), hipMemcpyDeviceToDevice, r.q));
	else if (varcnt)
		HIP_TRY(hipMemcpyAsync(d_out_len, h->d_cnt[par], S * sizeof(int32_t), hipMemcpyDeviceToDevice, r.q));
	else
		k_fill_cnt<<<grid_for(S, 64), 64, 0, r.q>>>(d_out_len, S, r.T);
	return 0;
}


// One run as its launchers see it: the plan, the caller's arguments, and what each of them used to spell out for itself -
// the stream, the two state copies, this step's counts, where mode_demod() writes (route_demod), the timed pair.
struct RunFrame {
	rtlfm_gpu *h;
	const RunPlan &pl;
	const uint8_t *d_iq; size_t stream_stride; int nblocks;
	int16_t *d_out; size_t out_stride; int32_t *d_out_len;
	hipStream_t q;
	const state_t *sin; state_t *sout;
	int32_t *dcnt;            // per-stream counts of a boxcar that does not divide the buffer (this step parity's)
	int16_t *dd; size_t dds;  // where mode_demod() writes so that the audio tail ends in d_out
	std::pair<Event, Event> ev;
	size_t iq_bytes() const { return iq_extent(h, stream_stride, nblocks); }
	const int32_t *cnt() const { return pl.g.varcnt ? dcnt : nullptr; }
	// the audio tail's work buffers, a quarter of the HBM away from the first run's input where that matters
	int ensure_res() { return pl.tp.any() ? ensure_res_buffers(h, d_iq, iq_bytes()) : 0; }
	void route_demod() { tail_route(h, pl.tp, d_out, out_stride, &dd, &dds); }  // (behind ensure_res)
	// the audio tail behind whatever demodulated into dd (run_tail: T, varcnt, Nblk, D as the front end left them)
	int tail() { return run_tail(h, pl.tp, dd, dds, pl.g.T, pl.g.varcnt, nblocks, pl.g.Nblk, pl.g.D, d_out, out_stride, d_out_len); }
};

// -M raw: two int16 per decimated sample - of the counts the front end left, or of T everywhere
static int raw_out_len(RunFrame &f)
{
	const int S = f.h->nstreams;
	if (!f.d_out_len) return 0;
	if (f.cnt()) {
		HIP_TRY(hipMemcpyAsync(f.d_out_len, f.cnt(), S * sizeof(int32_t), hipMemcpyDeviceToDevice, f.q));
		k_scale_cnt<<<grid_for(S, 64), 64, 0, f.q>>>(f.d_out_len, S, 2, 1);
	} else {
		k_fill_cnt<<<grid_for(S, 64), 64, 0, f.q>>>(f.d_out_len, S, 2 * f.pl.g.T);
	}
	return 0;
}

// The back half of full_demod() behind every decimator that leaves IQ (run_staged, the emit modes of both front ends, the
// channel front ends): the power squelch (src/rtl_fm.c:1204-1215) and -L levels, mode_demod incl. -M raw (:1256-1259), the
// audio tail.  `cur`: the decimated IQ of the plan's geometry.
// late_res: run_staged, which has not allocated the tail's work buffers in front of its launches as the front ends do - it
// does so here, behind the squelch's kernels, where it always did.
static int run_back_half(RunFrame &f, uint32_t *cur, size_t xstride, bool late_res = false)
{
	rtlfm_gpu *h = f.h;
	const rtlfm_cfg &c = h->cfg;
	const RunGeom &g = f.pl.g;
	const int S = h->nstreams, nblocks = f.nblocks;
	hipStream_t q = f.q;
	if (wants_levels(c))
		k_squelch_rms<<<S * nblocks, 256, 0, q>>>(cur, xstride, g.Nblk, g.D, nblocks, f.sin, c.squelch_level,
		                                         c.dc_block_raw, h->d_mute, h->d_levels);
	if (c.squelch_level) {
		k_squelch_hits<<<grid_for(S, 64), 64, 0, q>>>(h->d_mute, nblocks, S, f.sin, f.sout);
		k_squelch_zero<<<S * nblocks, 256, 0, q>>>(cur, xstride, g.Nblk, g.D, nblocks, S, g.T, f.sin,
		                                                     h->d_mute);
	}
	if (late_res) {
		const int r = f.ensure_res();
		if (r < 0) return r;
	}
	f.route_demod();
	if (c.mode == RTLFM_MODE_FM)
		k_fm_demod<<<S * nblocks, 256, 0, q>>>(cur, xstride, f.dd, f.dds, g.T, S, g.Nblk, g.D, nblocks,
		                                         c.custom_atan, h->d_lut, f.cnt(), f.sin, f.sout);
	else
		k_simple_demod<<<grid_for((size_t)S * g.T), 256, 0, q>>>(cur, xstride, f.dd, f.dds, g.T, S, c.mode,
		                                                     c.output_scale, f.cnt());
	if (c.mode == RTLFM_MODE_RAW) return raw_out_len(f);
	return f.tail();
}

// REST_IRREGULAR.  Passes first_irr .. passes - 1 where first_irr is handed a length that is not a multiple of four
// elements, and everything up to mode_demod() behind them (staged_kernels.h, k_fifth_irregular); then the ordinary audio
// tail.  `cur` holds the level in front of that pass (n_in samples per buffer, buffers back to back).
static int run_irregular_rest(RunFrame &f, const uint32_t *cur, size_t xstride)
{
	rtlfm_gpu *h = f.h;
	const rtlfm_cfg &c = h->cfg;
	const int S = h->nstreams, nblocks = f.nblocks, first = f.pl.g.first_irr;
	int r = f.ensure_res();
	if (r < 0) return r;
	f.route_demod();
	IrregularParams ip{};
	ip.X = cur; ip.xstride = xstride; ip.n_in = f.pl.g.N0 >> first; ip.nblocks = nblocks; ip.nstreams = S;
	ip.first = first; ip.passes = c.downsample_passes; ip.lp_len = (int)(c.block_len >> c.downsample_passes);
	ip.fir = c.comp_fir_size == 9 ? 1 : 0; ip.mode = c.mode; ip.variant = c.custom_atan; ip.output_scale = c.output_scale;
	ip.squelch_level = c.squelch_level; ip.report_levels = c.report_levels; ip.omit_dc_fix = c.dc_block_raw;
	ip.lut = h->d_lut; ip.R = f.dd; ip.rstride = f.dds;
	ip.levels = wants_levels(c) ? h->d_levels : nullptr;
	ip.sin = f.sin; ip.sout = f.sout;
	if (2 * ip.n_in + 8 > kIrregularMaxElems) return -ENOTSUP;  // (never: pass 8 of RTLFM_MAX_BLOCK_LEN is handed 512 samples)
	k_fifth_irregular<<<(unsigned)S, 64, 0, f.q>>>(ip);  // one wave per stream
	if (c.mode == RTLFM_MODE_RAW) {
		if (f.d_out_len) k_fill_cnt<<<grid_for(S, 64), 64, 0, f.q>>>(f.d_out_len, S, nblocks * ip.lp_len);
		return 0;
	}
	if (f.pl.g.T == 0) {  // every buffer is down to one element or none: fm_demod() has nothing to pair
		if (f.d_out_len) k_fill_cnt<<<grid_for(S, 64), 64, 0, f.q>>>(f.d_out_len, S, 0);
		return 0;
	}
	return f.tail();
}

// Options source_stats / source_health: where this run's records go (a view files single buffers into the run's rows)
static rtlfm_input_stat *source_stats_out(const rtlfm_gpu *h) { return h->opt.source_stats ? h->d_src_stats + h->src_rec_off : nullptr; }
static rtlfm_input_health *source_health_out(const rtlfm_gpu *h) { return h->opt.source_health ? h->d_src_health + h->src_rec_off : nullptr; }

// Option source_dc's pre-pass, in front of a channel front end and inside its timed pair: every source's buffer sums
// (k_rdc_sums_wide / _small on the source rows - one more read of the source bytes), then k_source_dc_smooth, which leaves
// the run's list of biases in d_sdc, the averages in every channel's record of sout and - hist: a filter or a bank carries
// a history - the next history's biases in the copy the run writes.  records: k_source_prepass in k_rdc_sums_*'s place,
// which leaves the same sums and the records of options source_stats / source_health from the same read.
static int launch_source_dc(rtlfm_gpu *h, const uint8_t *d_iq, size_t stream_stride, int nblocks, const state_t *sin, state_t *sout, bool hist,
                            bool records)
{
	const int nsrc = h->nstreams / h->chan_per;
	const uint32_t L = h->cfg.block_len;
	if (!h->d_sdc || !h->d_sdc_sums || !h->d_sdc_hist[0] || !h->d_sdc_hist[1]) return -EFAULT;
	if ((size_t)channel::kDcHist + (size_t)nblocks * (L / (2 * channel::kDcPiece)) > h->sdc_stride) return -E2BIG;
	const size_t total = (size_t)nsrc * nblocks;
	if (records) {
		const int r = sprepass::launch(d_iq, stream_stride, L, nblocks, nsrc, h->d_sdc_sums, source_health_out(h), source_stats_out(h),
		                               h->src_rec_stride ? h->src_rec_stride : nblocks, h->opt.input_stats_nt != 0, h->stream);
		if (r < 0) return r;
	} else if (L < 8192)
		k_rdc_sums_small<<<(unsigned)((total + 3) / 4), 256, 0, h->stream>>>(d_iq, stream_stride, L, nblocks, total, h->d_sdc_sums);
	else
		k_rdc_sums_wide<<<(unsigned)total, 256, 0, h->stream>>>(d_iq, stream_stride, L, nblocks, h->d_sdc_sums);
	channel::k_source_dc_smooth<<<(unsigned)nsrc, 64, 0, h->stream>>>(
		h->d_sdc_sums, L, nblocks, nsrc, h->chan_per, h->cfg.rdc_block_const, sin, sout,
		hist ? h->d_sdc_hist[h->src_hist_cur].get() : nullptr, hist ? h->d_sdc_hist[h->src_hist_cur ^ 1].get() : nullptr, h->d_sdc, h->sdc_stride);
	return 0;
}

// Options source_stats / source_health without the pre-pass kernel: the stream readers' launches over the SOURCE rows -
// k_input_health, which takes the statistics along when both are on, or k_input_stats alone.
static int launch_source_readers(rtlfm_gpu *h, const uint8_t *d_iq, size_t stream_stride, int nblocks)
{
	rtlfm_input_stat *so = source_stats_out(h);
	rtlfm_input_health *ho = source_health_out(h);
	const int nsrc = h->nstreams / h->chan_per, rs = h->src_rec_stride ? h->src_rec_stride : nblocks;
	const bool nt = h->opt.input_stats_nt != 0;
	if (ho) return ihealth::launch(d_iq, stream_stride, h->cfg.block_len, nblocks, nsrc, ho, rs, nt, h->stream, so);
	if (so) return istats::launch(d_iq, stream_stride, h->cfg.block_len, nblocks, nsrc, so, rs, nt, h->stream);
	return 0;
}

// What a channel run does with its source rows in front of its front end, inside the front end's timed pair: source_dc's
// pre-pass and the records of options source_stats / source_health, both over the raw bytes (the records are in front of
// source_dc's subtraction: nothing here changes a byte).  With source_dc and a record option on, ONE read: k_source_prepass
// (k_rdc_sums_* and the readers behind them, the same results from two reads, lost the A/B of LAB.md at 1024 sources x 4).
//
// Option source_iq comes first: k_source_iq reads the caller's rows (raw) and leaves the corrected rows in the handle's
// buffer, where source_iq_redirect has pointed the run (d_iq).  The records describe the ADC and stay on the raw rows - the
// readers' own launches, as with source_dc off -, source_dc's sums come from k_rdc_sums_* on the corrected rows, and
// k_source_prepass is not used: one more read.
static int launch_source_side(rtlfm_gpu *h, const uint8_t *raw, size_t raw_stride, const uint8_t *d_iq, size_t stream_stride, int nblocks,
                              const state_t *sin, state_t *sout, bool hist)
{
	const bool records = h->opt.source_stats || h->opt.source_health;
	if (records && ((h->opt.source_stats && !h->d_src_stats) || (h->opt.source_health && !h->d_src_health))) return -EFAULT;  // (views do not allocate)
	int r;
	if (h->opt.source_iq) {
		const int nsrc = h->nstreams / h->chan_per;
		if (!h->d_siq_rows || !h->d_siq_sums || !h->d_siq_coef || d_iq != h->d_siq_rows.get()) return -EFAULT;
		if ((size_t)nsrc * h->siq_stride > h->d_siq_rows.capacity() || (size_t)nblocks * h->cfg.block_len > h->siq_stride) return -E2BIG;
		const int rs = h->src_rec_stride ? h->src_rec_stride : nblocks;
		if (h->src_rec_off + (size_t)(nsrc - 1) * rs + nblocks > h->d_siq_sums.capacity()) return -E2BIG;
		if ((r = siq::launch(raw, raw_stride, h->cfg.block_len, nblocks, nsrc, h->d_siq_coef, h->d_siq_rows, h->siq_stride,
		                     h->d_siq_sums + h->src_rec_off, rs, h->opt.input_stats_nt != 0, h->stream)) < 0)
			return r;
	}
	const bool one = records && h->opt.source_dc && !h->opt.source_iq;
	if (h->opt.source_dc && (r = launch_source_dc(h, d_iq, stream_stride, nblocks, sin, sout, hist, one)) < 0) return r;
	return records && !one ? launch_source_readers(h, raw, raw_stride, nblocks) : 0;
}

// Option source_iq: from here on the run's source rows are the handle's corrected rows (what the run was handed comes back
// in raw / raw_stride for launch_source_side).  Before anything takes the frame's pointers.
static void source_iq_redirect(RunFrame &f, const uint8_t **raw, size_t *raw_stride)
{
	*raw = f.d_iq; *raw_stride = f.stream_stride;
	if (f.h->chan_per > 0 && f.h->opt.source_iq) {
		f.d_iq = f.h->d_siq_rows;
		f.stream_stride = f.h->siq_stride;
	}
}

// ROUTE_STAGED and ROUTE_CHAN_MIX: a kernel per stage through the work buffers.  The timed pair holds the decimator with
// its own raw-DC sums (k_rdc_sums / k_rdc_smooth, not the front ends' pre-pass); the tail's buffers are allocated behind
// it, in the back half.
static int run_staged(RunFrame &f)
{
	rtlfm_gpu *h = f.h;
	const rtlfm_cfg &c = h->cfg;
	const RunGeom &g = f.pl.g;
	const int S = h->nstreams, nblocks = f.nblocks;
	const uint32_t L = c.block_len;
	const uint8_t *raw; size_t raw_stride;
	source_iq_redirect(f, &raw, &raw_stride);
	const uint8_t *d_iq = f.d_iq;
	const size_t stream_stride = f.stream_stride;
	hipStream_t q = f.q;
	const state_t *sin = f.sin;
	state_t *sout = f.sout;
	int r = ensure_work_buffers(h);
	if (r < 0) return r;
	r = timing_begin(h, f.ev);
	if (r < 0) return r;
	// --- rtlsdr_callback: convert, raw DC block, rotate (src/rtl_fm.c:1326-1338)
	const int2 *rdc = nullptr;
	if (c.dc_block_raw) {
		k_rdc_sums<<<S * nblocks, 256, 0, q>>>(d_iq, stream_stride, L, nblocks, h->d_sums);
		k_rdc_smooth<<<(unsigned)S, 64, 0, q>>>(h->d_sums, L, nblocks, S, c.rdc_block_const, sin, sout,
		                                           h->d_rdc_avg);
		rdc = h->d_rdc_avg;
	}
	if (h->chan_per > 0 && (r = launch_source_side(h, raw, raw_stride, d_iq, stream_stride, nblocks, sin, sout, false)) < 0) return r;  // (no filter, no bank here: no history)
	if (h->chan_per > 0 && h->opt.source_dc) {  // ... behind option source_dc's pre-pass
		channel::k_channel_mix<true><<<grid_for((size_t)S * nblocks * (L / 16)), 256, 0, q>>>(d_iq, stream_stride, L, nblocks, S, h->chan_per,
		                                                                                  h->d_chan_steps, h->d_chan_table,
		                                                                                  (uint32_t)h->chan_pos, h->bufA, h->xstride, h->d_sdc,
		                                                                                  h->sdc_stride, channel::kDcHist);
	} else if (h->chan_per > 0)  // channels: the NCO mixer in rotate16_neg90's place, the source's row in the stream's
		channel::k_channel_mix<false><<<grid_for((size_t)S * nblocks * (L / 16)), 256, 0, q>>>(d_iq, stream_stride, L, nblocks, S, h->chan_per,
		                                                                                      h->d_chan_steps, h->d_chan_table,
		                                                                                      (uint32_t)h->chan_pos, h->bufA, h->xstride, nullptr, 0, 0);
	else
		k_convert<<<grid_for((size_t)S * nblocks * (L / 16)), 256, 0, q>>>(d_iq, stream_stride, L, nblocks, S,
		                                                                  h->bufA, h->xstride,
		                                                                  c.offset_tuning ? 0 : 1, rdc);
	uint32_t *cur = h->bufA, *oth = h->bufB;
	// --- decimation (src/rtl_fm.c:1187-1202)
	if (c.downsample_passes > 0) {
		for (int p = 0; p < g.first_irr; p++) {
			int N = g.N0 >> p;
			k_fifth<<<grid_for((size_t)S * nblocks * (N / 2)), 256, 0, q>>>(cur, oth, h->xstride, N, nblocks, S,
			                                                              p, sin, sout);
			std::swap(cur, oth);
		}
		if (f.pl.rest == RTLFM_REST_IRREGULAR) {
			r = timing_end(h, f.ev);
			if (r < 0) return r;
			return run_irregular_rest(f, cur, h->xstride);
		}
		if (c.comp_fir_size == 9) {
			k_fir9<<<grid_for((size_t)S * g.T), 256, 0, q>>>(cur, oth, h->xstride, g.T, S, c.downsample_passes,
			                                              sin, sout);
			std::swap(cur, oth);
		}
	} else {
		k_boxcar<<<grid_for((size_t)S * (g.maxout + 1)), 256, 0, q>>>(cur, oth, h->xstride, g.Tin, S, g.D, sin, sout,
		                                                          f.dcnt);
		std::swap(cur, oth);
	}
	r = timing_end(h, f.ev);
	if (r < 0) return r;
	return run_back_half(f, cur, h->xstride, true);
}


// shader clock held during the last fused fifth_order launch: every wave stamps s_memtime (shader
// clock) and s_memrealtime (100 MHz) at its first and last instruction
static int read_clock_stamps(rtlfm_gpu *h, double *mhz, double *span_ms, int *waves)
{
	HIP_TRY(sync_all(h));
	if (!h->fws.stamps || h->fws.stamp_last <= 0) return -ENODATA;
	std::vector<unsigned long long> st((size_t)h->fws.stamp_last * 4);
	HIP_TRY(hipMemcpy(st.data(), h->fws.stamp_half(0), st.size() * 8, hipMemcpyDeviceToHost));
	double sum = 0; int n = 0; unsigned long long t0 = ~0ull, t1 = 0;
	for (int w = 0; w < h->fws.stamp_last; w++) {
		double dc = (double)(st[w * 4 + 1] - st[w * 4]), dr = (double)(st[w * 4 + 3] - st[w * 4 + 2]);
		if (dr > 0) { sum += dc / dr * 100.0; n++; }
		if (st[w * 4 + 2] < t0) t0 = st[w * 4 + 2];
		if (st[w * 4 + 3] > t1) t1 = st[w * 4 + 3];
	}
	if (!n) return -ENODATA;
	if (mhz) *mhz = sum / n;
	if (span_ms) *span_ms = (double)(t1 - t0) / 1e5;
	if (waves) *waves = n;
	return 0;
}
static int report_clock_stamps(rtlfm_gpu *h)
{
	double mhz = 0, span = 0; int n = 0;
	int r = read_clock_stamps(h, &mhz, &span, &n);
	if (r < 0) return r == -ENODATA ? 0 : r;
	fprintf(stderr, "rtlfm_hip[debug]: mean shader clock %.0f MHz over %d waves, kernel span %.3f ms\n", mhz, n, span);
	return 0;
}

extern "C" int rtlfm_gpu_clock_probe(rtlfm_gpu *h, int on)
{
	if (!h) return -EINVAL;
	h->fws.want_stamps = on != 0;
	return 0;
}
extern "C" int rtlfm_gpu_clock_read(rtlfm_gpu *h, double *shader_mhz, double *span_ms)
{
	if (!h) return -EINVAL;
	HIP_TRY(hipSetDevice(h->device));
	return read_clock_stamps(h, shader_mhz, span_ms, nullptr);
}

// dc_block_raw_filter needs every buffer's mean before its first sample: one more pass over the input (the
// per-buffer sums), the smoothing recurrence over a stream's buffers; the averages then ride on the front end
// (fused_kernel.h: the MFMA accumulators' start values; boxcar_kernel.h: a correction of the prefix sums)
static const int2 *rdc_prepass(rtlfm_gpu *h, const uint8_t *d_iq, size_t stream_stride, int nblocks)
{
	const rtlfm_cfg &c = h->cfg;
	if (!c.dc_block_raw) return nullptr;
	const int S = h->nstreams;
	if (c.block_len < 8192) {  // buffers shorter than a tile: a wave per buffer (staged_kernels.h)
		const size_t total = (size_t)S * nblocks;
		k_rdc_sums_small<<<(unsigned)((total + 3) / 4), 256, 0, h->stream>>>(d_iq, stream_stride, c.block_len, nblocks, total, h->d_sums);
	} else
		k_rdc_sums_wide<<<(unsigned)((size_t)S * nblocks), 256, 0, h->stream>>>(d_iq, stream_stride, c.block_len, nblocks, h->d_sums);
	k_rdc_smooth<<<(unsigned)S, 64, 0, h->stream>>>(h->d_sums, c.block_len, nblocks, S, c.rdc_block_const, h->st[h->st_cur],
	                                                  h->st[(h->st_cur + 1) % 3], h->d_rdc_avg);
	return h->d_rdc_avg;
}

// What the four launchers of k_fused and k_boxcar_scan share around their launch, in the one order all four had: the
// buffers the plan asks for (what an emit mode writes, the audio tail's), then inside the timed pair the raw-DC pre-pass,
// the cleared rms() sums where the front end takes them, the launch; behind the pair k_squelch_apply on those sums.
// `launch(rdc)`: the front end itself, given the pre-pass's averages (or nullptr).
template <class Launch>
static int run_front_end(RunFrame &f, Launch &&launch)
{
	rtlfm_gpu *h = f.h;
	const rtlfm_cfg &c = h->cfg;
	const RunPlan &pl = f.pl;
	const int S = h->nstreams;
	const bool emits = pl.route == RTLFM_ROUTE_FUSED_EMIT || pl.route == RTLFM_ROUTE_BOXCAR_EMIT;
	int r;
	if (pl.rest != RTLFM_REST_NONE) {  // (REST_NONE: the launch writes the caller's rows and nothing follows but their lengths)
		if (emits && (r = ensure_deep_buffers(h, f.d_iq, f.iq_bytes())) < 0) return r;
		if ((r = f.ensure_res()) < 0) return r;
	}
	f.route_demod();
	if ((r = timing_begin(h, f.ev)) < 0) return r;
	h->fws.tail_follows = pl.tail_follows;
	const int2 *rdc = rdc_prepass(h, f.d_iq, f.stream_stride, f.nblocks);  // -E rdc; in emit mode in front of -M raw, the squelch, 7-10 passes
	if (pl.sq_front) HIP_TRY(hipMemsetAsync(h->d_sq_sums, 0, (size_t)S * f.nblocks * 2 * sizeof(uint32_t), f.q));
	if ((r = launch(rdc)) < 0) return r;
	if ((r = timing_end(h, f.ev)) < 0) return r;
	if (pl.sq_front)  // the front end took rms()'s sums, k_squelch_apply decides (fused_kernel.h; boxcar_kernel.h, SQ)
		k_squelch_apply<<<(unsigned)S, 256, (size_t)f.nblocks * sizeof(int32_t), f.q>>>(
		    h->d_sq_sums, f.dd, f.dds, pl.g.Nblk, pl.g.D, f.nblocks, S, c.squelch_level, c.dc_block_raw, c.mode == RTLFM_MODE_FM ? 1 : 0,
		    f.cnt(), pl.g.T, f.sin, f.sout, h->d_levels);
	return 0;
}
// where an emit mode writes: the caller's rows (REST_NONE), else the handle's work buffer
static uint32_t *emit_to(const RunFrame &f) { return f.pl.rest == RTLFM_REST_NONE ? reinterpret_cast<uint32_t *>(f.d_out) : f.h->deepA.get(); }
static size_t emit_stride(const RunFrame &f) { return f.pl.rest == RTLFM_REST_NONE ? f.out_stride / 2 : f.h->deep_stride; }

// ROUTE_FUSED: k_fused from the bytes to the PCM.
static int run_fused(RunFrame &f)
{
	rtlfm_gpu *h = f.h;
	int r = run_front_end(f, [&](const int2 *rdc) {
		return fused::launch(h->fws, h->cfg, h->nstreams, f.d_iq, f.stream_stride, f.nblocks, f.dd, f.dds, f.sin, f.sout, h->d_lut, f.q, nullptr, 0,
		                     rdc, f.pl.sq_front ? h->d_sq_sums.get() : nullptr);
	});
	if (r < 0) return r;
	// bit 2 with bit 8: report the stamps of every launch (synchronises, so the GPU idles between
	// launches and clocks up); bit 2 alone with bit 16: only when timing_read() asks, i.e. the last
	// launch of an uninterrupted sequence
	if (h->fws.stamps && (h->fws.debug & 2) && !(h->fws.debug & 16)) {
		int r2 = report_clock_stamps(h);
		if (r2 < 0) return r2;
	}
	return f.tail();
}

// REST_DEEP_DEMOD / REST_DEEP_IQ.  Seven and more passes on buffers they divide: the passes beyond six, generic_fir and
// (without a squelch) the demodulator in ONE launch, a workgroup per (stream, buffer) in LDS (staged_kernels.h, k_deep_rest)
static int rest_deep(RunFrame &f)
{
	rtlfm_gpu *h = f.h;
	const rtlfm_cfg &c = h->cfg;
	const RunGeom &g = f.pl.g;
	const bool demod_here = f.pl.rest == RTLFM_REST_DEEP_DEMOD;
	int kk[6];
	deep_rest_tails(c.downsample_passes, c.comp_fir_size == 9, kk);
	DeepRestParams dp{};
	dp.X = h->deepA; dp.xstride = h->deep_stride; dp.n6 = g.N0 >> g.level; dp.nblocks = f.nblocks; dp.nstreams = h->nstreams;
	dp.passes = c.downsample_passes;
	dp.fir = c.comp_fir_size == 9 ? 1 : 0; dp.kt = kk[0];
	dp.mode = c.mode; dp.variant = c.custom_atan; dp.output_scale = c.output_scale; dp.lut = h->d_lut;
	dp.sin = f.sin; dp.sout = f.sout;
	if (demod_here) { dp.R = f.dd; dp.rstride = f.dds; }
	else { dp.Y = h->deepB; dp.ystride = h->deep_stride; }
	const size_t lds_b = (size_t)2 * (kk[0] + dp.n6 + 8) * sizeof(uint32_t);
	k_deep_rest<<<(unsigned)((size_t)h->nstreams * f.nblocks), 256, lds_b, f.q>>>(dp);
	if (demod_here) return f.tail();
	return run_back_half(f, h->deepB, h->deep_stride);  // the squelch, -L, -M raw on the final level
}

// REST_PER_PASS / REST_IRREGULAR behind six fused passes: a launch per remaining pass the buffers divide; then generic_fir
// and the back half, or - nine or ten passes on buffers they do not divide - the reference's own loops from there.
static int rest_passes(RunFrame &f)
{
	rtlfm_gpu *h = f.h;
	const rtlfm_cfg &c = h->cfg;
	const RunGeom &g = f.pl.g;
	const int S = h->nstreams;
	uint32_t *cur = h->deepA, *oth = h->deepB;
	for (int p = g.level; p < g.first_irr; p++) {
		const int N = g.N0 >> p;
		k_fifth<<<grid_for((size_t)S * f.nblocks * (N / 2)), 256, 0, f.q>>>(cur, oth, h->deep_stride, N, f.nblocks, S, p, f.sin, f.sout);
		std::swap(cur, oth);
	}
	if (f.pl.rest == RTLFM_REST_IRREGULAR) return run_irregular_rest(f, cur, h->deep_stride);
	if (c.comp_fir_size == 9) {
		k_fir9<<<grid_for((size_t)S * g.T), 256, 0, f.q>>>(cur, oth, h->deep_stride, g.T, S, c.downsample_passes, f.sin, f.sout);
		std::swap(cur, oth);
	}
	return run_back_half(f, cur, h->deep_stride);
}

// ROUTE_FUSED_EMIT.  The fused front end in emit mode + staged kernels for what it does not do itself: with up to
// six passes it emits the decimated, FIR-compensated IQ (what full_demod() hands on after
// src/rtl_fm.c:1202); with 7..10 passes the /64 IQ, and the staged kernels run the remaining
// passes and the FIR on 1/64 of the data.  Then, as in full_demod(): squelch (:1204-1215),
// mode_demod incl. -M raw (:1256-1259), audio tail.  The work buffer has the staged path's
// layout for that level (a stream's buffers back to back).
static int run_fused_emit(RunFrame &f)
{
	rtlfm_gpu *h = f.h;
	int r = run_front_end(f, [&](const int2 *rdc) {
		return fused::launch(h->fws, h->cfg, h->nstreams, f.d_iq, f.stream_stride, f.nblocks, nullptr, 0, f.sin, f.sout, h->d_lut, f.q, emit_to(f),
		                     emit_stride(f), rdc);
	});
	if (r < 0) return r;
	switch (f.pl.rest) {
	case RTLFM_REST_NONE: return raw_out_len(f);
	case RTLFM_REST_DEEP_DEMOD:
	case RTLFM_REST_DEEP_IQ: return rest_deep(f);
	case RTLFM_REST_PER_PASS:
	case RTLFM_REST_IRREGULAR: return rest_passes(f);
	case RTLFM_REST_BACK_HALF: return run_back_half(f, h->deepA, h->deep_stride);
	default: return -EFAULT;  // planning bug
	}
}

// ROUTE_BOXCAR.  The boxcar (low_pass) front end in one launch; output counts may differ per buffer and
// per stream (d_cnt), which the order-insensitive tail stages accept (run_tail, varcnt).
static int run_boxfused(RunFrame &f)
{
	rtlfm_gpu *h = f.h;
	int r = run_front_end(f, [&](const int2 *rdc) {
		return boxfused::launch(h->fws, h->cfg, h->nstreams, f.d_iq, f.stream_stride, f.nblocks, f.dd, f.dds, f.dcnt, f.sin, f.sout, f.q, nullptr, 0,
		                        rdc, f.pl.sq_front ? h->d_sq_sums.get() : nullptr);
	});
	return r < 0 ? r : f.tail();
}

// ROUTE_BOXCAR_EMIT.  The boxcar front end in emit mode + staged kernels on 1 / D of the data, as full_demod() goes on
// behind low_pass(): power squelch (src/rtl_fm.c:1204-1215), -L levels (:1217-1237), mode_demod incl. -M raw
// (:1006-1009, 1256-1259), audio tail.  The everyday scanner line - rtl_fm -M fm -s 12k -l 50 - is this.
// (REST_NONE, -M raw without the squelch: what the launch emits IS the output - raw_demod() copies lowpassed[],
// src/rtl_fm.c:1002-1009 - and goes straight into the caller's rows; round 5: a copy kernel over 429 M samples cost more
// than the decimator)
static int run_boxfused_emit(RunFrame &f)
{
	rtlfm_gpu *h = f.h;
	int r = run_front_end(f, [&](const int2 *rdc) {
		return boxfused::launch(h->fws, h->cfg, h->nstreams, f.d_iq, f.stream_stride, f.nblocks, nullptr, 0, f.dcnt, f.sin, f.sout, f.q, emit_to(f),
		                        emit_stride(f), rdc);
	});
	if (r < 0) return r;
	return f.pl.rest == RTLFM_REST_NONE ? raw_out_len(f) : run_back_half(f, h->deepA, h->deep_stride);
}

// Channels on.  One of three front ends takes the source bytes to every channel's decimated IQ (chan_iq), then full_demod()
// goes on as behind low_pass() (run_back_half).  What the three share of a run beyond the plan's geometry (RunGeom: Tin
// complex samples of the run, an output every D of them, maxout the most a run can have):
struct ChanRun {
	const RunGeom &g;
	int nsrc, nblocks;
	int target_waves;      // for channel::plan
	int32_t *dcnt;
	const state_t *sin;
	state_t *sout;
	const uint8_t *hist_in;  // the source history in front of the run
	uint8_t *hist_out;       // ... and behind it; rtlfm_gpu_run_device changes over once per run
	channel::Frame f;        // (segs, tiles_per_seg, ntiles: the front end's own)
};

// What the channel front ends allocate at first use, sized from the handle's own buffer length: a view of the handle on a
// shorter buffer (run_ragged) must find them there - it is a copy and cannot allocate (device_own.h).  The decimated IQ; on path 1 the
// filter's mixed samples and the bank's sums.
static int ensure_chan_iq(rtlfm_gpu *h)
{
	if (h->chan_iq) return 0;
	h->chan_stride = (((size_t)h->cap_blocks * (h->cfg.block_len / 2)) / h->cfg.downsample + 1 + 16 + 3) & ~(size_t)3;  // rows start on 16-byte lines
	return h->chan_iq.alloc((size_t)h->nstreams * h->chan_stride);
}
static int ensure_chan_fir_x(rtlfm_gpu *h)
{
	if (h->chan_fir_x) return 0;
	h->chan_fir_xstride = (size_t)chanfir::kHaloMax + (size_t)h->cap_blocks * (h->cfg.block_len / 2);
	return h->chan_fir_x.alloc((size_t)h->nstreams * h->chan_fir_xstride);
}
static int ensure_bank_v(rtlfm_gpu *h, size_t vneed /* 0: the most a run of this handle can need */)
{
	const size_t nsrc = (size_t)(h->nstreams / h->chan_per);
	const size_t most = (nsrc * ((size_t)h->cap_blocks * (h->cfg.block_len / 2) / h->cfg.downsample + 1)) << h->bank_m;
	if (h->bank_v.capacity() >= (vneed ? vneed : most)) return 0;
	return h->bank_v.grow(most, h->stream);
}
// ... all of them, for the front end and the path the handle is set to, before the first view is made
static int ensure_channel_buffers(rtlfm_gpu *h)
{
	int r = ensure_chan_iq(h);
	if (r < 0 || h->path != 1) return r;
	if (h->bank_K > 0) return ensure_bank_v(h, 0);
	return h->fir_ntaps > 0 ? ensure_chan_fir_x(h) : 0;
}

// What the three front ends are handed (REST_NONE - the boxcar alone, -M raw without the squelch: the launch's rows ARE the
// output, as run_boxfused_emit's)
static int chan_run_prepare(RunFrame &rf, ChanRun &cr)
{
	rtlfm_gpu *h = rf.h;
	const RunGeom &g = rf.pl.g;
	const bool direct = rf.pl.rest == RTLFM_REST_NONE;
	cr.nsrc = h->nstreams / h->chan_per;
	cr.nblocks = rf.nblocks;
	if (rf.pl.route != RTLFM_ROUTE_CHAN_BOXCAR && h->src_hist_srcs < cr.nsrc) return -ENOMEM;  // (ensure_history failed in the setter, which said so)
	int r;
	if (!direct && ((r = ensure_chan_iq(h)) < 0 || (r = rf.ensure_res()) < 0)) return r;
	cr.target_waves = rf.pl.tp.any() ? h->fws.target_waves_tail : h->fws.target_waves;
	cr.dcnt = rf.dcnt;
	cr.sin = rf.sin; cr.sout = rf.sout;
	cr.hist_in = h->d_src_hist[h->src_hist_cur]; cr.hist_out = h->d_src_hist[h->src_hist_cur ^ 1];
	channel::Frame &f = cr.f;
	f = channel::Frame{};
	f.iq = rf.d_iq; f.src_stride = rf.stream_stride;
	f.pos = (uint32_t)h->chan_pos;
	f.T = g.Tin; f.D = g.D;
	f.maxout = g.maxout;
	f.per_source = h->chan_per;
	f.Y = direct ? reinterpret_cast<uint32_t *>(rf.d_out) : h->chan_iq.get();
	f.ystride = direct ? rf.out_stride / 2 : h->chan_stride;
	f.cnt = cr.dcnt; f.sin = cr.sin; f.sout = cr.sout;
	return 0;
}

// The boxcar: k_channel_boxcar, one launch (channel_kernel.h).
static int launch_channel_boxcar(rtlfm_gpu *h, const ChanRun &cr)
{
	channel::BoxParams p{};
	p.f = cr.f;
	p.steps = h->d_chan_steps; p.table = h->d_chan_table;
	p.groups = (h->chan_per + channel::kWaves - 1) / channel::kWaves;
	p.f.ntiles = (cr.g.Tin + channel::kTileSamples - 1) / channel::kTileSamples;
	channel::plan(h->nstreams, p.f.ntiles, cr.g.D, cr.target_waves, h->fws.min_tiles, h->fws.tiles_per_seg, &p.f.segs, &p.f.tiles_per_seg);
	const size_t grid = (size_t)cr.nsrc * p.f.segs * p.groups;
	if (grid > 0x7fffffffu) return -E2BIG;
	if (h->opt.source_dc) {
		p.dc = h->d_sdc; p.dc_stride = h->sdc_stride;
		if (cr.g.D >= channel::kStageMinD) channel::k_channel_boxcar<true, true><<<(unsigned)grid, channel::kWaves * 64, 0, h->stream>>>(p);
		else channel::k_channel_boxcar<false, true><<<(unsigned)grid, channel::kWaves * 64, 0, h->stream>>>(p);
		return 0;
	}
	if (cr.g.D >= channel::kStageMinD) channel::k_channel_boxcar<true, false><<<(unsigned)grid, channel::kWaves * 64, 0, h->stream>>>(p);
	else channel::k_channel_boxcar<false, false><<<(unsigned)grid, channel::kWaves * 64, 0, h->stream>>>(p);
	return 0;
}

// A filter set (rtlfm_gpu_set_channel_filter): the filter in the boxcar's place.  fused: k_channel_fir, one launch from
// source bytes to decimated IQ; else the cross-check - k_channel_mix over the end of the history and over the run,
// k_channel_fir_plain, k_source_history.
static int launch_channel_fir(rtlfm_gpu *h, bool fused_path, const ChanRun &cr)
{
	const int S = h->nstreams;
	hipStream_t q = h->stream;
	if (fused_path) {
		chanfir::FirParams p{};
		p.f = cr.f;
		p.hist_in = cr.hist_in; p.hist_out = cr.hist_out;
		p.steps = h->d_chan_steps; p.table = h->d_chan_table; p.taps8 = h->d_fir_taps8;
		p.ntaps = h->fir_ntaps; p.nt8 = chanfir::padded_taps(h->fir_ntaps); p.halo = chanfir::halo_of(h->fir_ntaps); p.shift = h->fir_shift;
		p.groups = (h->chan_per + chanfir::kWaves - 1) / chanfir::kWaves;
		p.f.ntiles = (cr.g.Tin + chanfir::kTile - 1) / chanfir::kTile;
		// (kMaxD's limit is the boxcar's warm-up tile; here every D goes with every segmentation: D = 1 for the plan)
		channel::plan(S, p.f.ntiles, 1, cr.target_waves, h->fws.min_tiles, h->fws.tiles_per_seg, &p.f.segs, &p.f.tiles_per_seg);
		const size_t grid = (size_t)cr.nsrc * p.f.segs * p.groups;
		if (grid > 0x7fffffffu) return -E2BIG;
		if (h->opt.source_dc) {
			p.dc = h->d_sdc; p.dc_stride = h->sdc_stride; p.dc_entries = channel::kDcHist + cr.g.Tin / channel::kDcPiece;
			chanfir::k_channel_fir<true><<<(unsigned)grid, chanfir::kWaves * 64, chanfir::lds_bytes(h->fir_ntaps) + chanfir::kDcLds, q>>>(p);
			return 0;
		}
		chanfir::k_channel_fir<false><<<(unsigned)grid, chanfir::kWaves * 64, chanfir::lds_bytes(h->fir_ntaps), q>>>(p);
		return 0;
	}
	constexpr int halo = chanfir::kHaloMax;
	int r = ensure_chan_fir_x(h);
	if (r < 0) return r;
	if (h->opt.source_dc) {
		// (the history's last `halo` samples are the list's entries kDcHist - halo / 256 ... kDcHist - 1)
		channel::k_channel_mix<true><<<grid_for((size_t)S * (halo / 8)), 256, 0, q>>>(
			cr.hist_in + (size_t)(channel::kHist - halo) * 2, (size_t)channel::kHist * 2, (uint32_t)halo * 2, 1, S, h->chan_per, h->d_chan_steps,
			h->d_chan_table, (uint32_t)h->chan_pos - (uint32_t)halo, h->chan_fir_x, h->chan_fir_xstride, h->d_sdc, h->sdc_stride,
			channel::kDcHist - halo / channel::kDcPiece);
		channel::k_channel_mix<true><<<grid_for((size_t)S * cr.nblocks * (h->cfg.block_len / 16)), 256, 0, q>>>(
			cr.f.iq, cr.f.src_stride, h->cfg.block_len, cr.nblocks, S, h->chan_per, h->d_chan_steps, h->d_chan_table, (uint32_t)h->chan_pos,
			h->chan_fir_x + halo, h->chan_fir_xstride, h->d_sdc, h->sdc_stride, channel::kDcHist);
	} else {
	// (the history's last `halo` samples: rows channel::kHist * 2 bytes apart, one buffer of halo * 2 bytes each)
	channel::k_channel_mix<false><<<grid_for((size_t)S * (halo / 8)), 256, 0, q>>>(
		cr.hist_in + (size_t)(channel::kHist - halo) * 2, (size_t)channel::kHist * 2, (uint32_t)halo * 2, 1, S, h->chan_per, h->d_chan_steps,
		h->d_chan_table, (uint32_t)h->chan_pos - (uint32_t)halo, h->chan_fir_x, h->chan_fir_xstride, nullptr, 0, 0);
	channel::k_channel_mix<false><<<grid_for((size_t)S * cr.nblocks * (h->cfg.block_len / 16)), 256, 0, q>>>(
		cr.f.iq, cr.f.src_stride, h->cfg.block_len, cr.nblocks, S, h->chan_per, h->d_chan_steps, h->d_chan_table, (uint32_t)h->chan_pos,
		h->chan_fir_x + halo, h->chan_fir_xstride, nullptr, 0, 0);
	}
	chanfir::k_channel_fir_plain<<<grid_for((size_t)S * cr.g.maxout), 256, 0, q>>>(h->chan_fir_x, h->chan_fir_xstride, S, cr.g.Tin, cr.g.D,
	                                                                          h->d_fir_taps, h->fir_ntaps, h->fir_shift, cr.g.maxout, h->chan_iq,
	                                                                          h->chan_stride, cr.dcnt, cr.sin, cr.sout);
	channel::k_source_history<<<grid_for((size_t)cr.nsrc * (channel::kHist / 8)), 256, 0, q>>>(cr.f.iq, cr.f.src_stride, cr.hist_in, cr.hist_out,
	                                                                                        cr.nsrc, cr.g.Tin);
	return 0;
}

// The bank set (rtlfm_gpu_set_channel_bank): K polyphase sums and one fix_fft per output instant in the mixer paths' place.
// fused: k_channel_bank, one launch; else the cross-check - k_bank_sums, k_bank_fft, k_bank_scatter, k_source_history.
static int launch_channel_bank(rtlfm_gpu *h, bool fused_path, const ChanRun &cr)
{
	const int S = h->nstreams;
	hipStream_t q = h->stream;
	const bool ps = !h->bank_bins_ps.empty();
	const int32_t *bins = ps ? h->d_bank_bins_ps : h->d_bank_bins;
	const int bins_stride = ps ? h->chan_per : 0;
	const int sv = h->sv.writing;  // -1: no survey (run_device_impl)
	if (fused_path) {
		const chanbank::Geometry g = chanbank::geometry(h->bank_m, h->bank_ntaps, cr.g.D, sv >= 0);
		chanbank::BankParams p{};
		p.f = cr.f;
		p.hist_in = cr.hist_in; p.hist_out = cr.hist_out;
		p.taps2 = h->d_bank_taps2; p.tw = h->d_bank_tw; p.bins = bins; p.bins_stride = bins_stride;
		p.m = g.m; p.Q = g.Q; p.Qp = g.Qp; p.lead = g.lead; p.F = g.F; p.Ls = g.Ls; p.Fs = g.Fs; p.shift = h->bank_shift;
		p.f.ntiles = (cr.g.maxout + g.F - 1) / g.F;
		// (frames are independent: every D goes with every segmentation - D = 1 for the plan; one workgroup per source and segment)
		channel::plan(cr.nsrc * chanbank::kWaves, p.f.ntiles, 1, cr.target_waves, h->fws.min_tiles, h->fws.tiles_per_seg, &p.f.segs,
		              &p.f.tiles_per_seg);
		const size_t grid = (size_t)cr.nsrc * p.f.segs;
		if (grid > 0x7fffffffu) return -E2BIG;
		const bool dc = h->opt.source_dc != 0;
		if (dc) { p.dc = h->d_sdc; p.dc_stride = h->sdc_stride; }
		if (sv < 0) {
			if (dc) chanbank::k_channel_bank_dc<<<(unsigned)grid, chanbank::kWaves * 64, g.lds, q>>>(p);
			else chanbank::k_channel_bank<<<(unsigned)grid, chanbank::kWaves * 64, g.lds, q>>>(p);
			return 0;
		}
		const size_t need = (grid << h->bank_m);
		OWN_TRY(h->sv.d_partial.grow(need, q));  // (waits for what reads it)
		p.survey = h->sv.d_partial;
		if (dc) chanbank::k_channel_bank_survey_dc<<<(unsigned)grid, chanbank::kWaves * 64, g.lds, q>>>(p);
		else chanbank::k_channel_bank_survey<<<(unsigned)grid, chanbank::kWaves * 64, g.lds, q>>>(p);
		chanbank::k_bank_survey_reduce<<<grid_for((size_t)cr.nsrc << h->bank_m), 256, 0, q>>>(h->sv.d_partial, p.f.segs, h->bank_m, cr.nsrc,
		                                                                                   h->chan_per, cr.g.Tin, cr.g.D, cr.sin, h->sv.d_power[sv],
		                                                                                   h->sv.d_frames[sv]);
		return 0;
	}
	const size_t vneed = ((size_t)cr.nsrc * cr.g.maxout) << h->bank_m;
	int r = ensure_bank_v(h, vneed);
	if (r < 0) return r;
	if (h->opt.source_dc)
		chanbank::k_bank_sums<true><<<grid_for(vneed), 256, 0, q>>>(cr.f.iq, cr.f.src_stride, cr.hist_in, h->d_bank_taps, h->bank_ntaps, h->bank_m,
		                                                        h->bank_shift, (uint32_t)h->chan_pos, cr.nsrc, h->chan_per, cr.g.Tin, cr.g.D,
		                                                        cr.g.maxout, cr.sin, h->bank_v, h->d_sdc, h->sdc_stride);
	else
		chanbank::k_bank_sums<false><<<grid_for(vneed), 256, 0, q>>>(cr.f.iq, cr.f.src_stride, cr.hist_in, h->d_bank_taps, h->bank_ntaps, h->bank_m,
		                                                            h->bank_shift, (uint32_t)h->chan_pos, cr.nsrc, h->chan_per, cr.g.Tin, cr.g.D,
		                                                            cr.g.maxout, cr.sin, h->bank_v, nullptr, 0);
	chanbank::k_bank_fft<<<grid_for((size_t)cr.nsrc * cr.g.maxout), 256, 0, q>>>(h->bank_v, h->d_bank_sine, h->bank_m, cr.nsrc, h->chan_per, cr.g.Tin,
	                                                                          cr.g.D, cr.g.maxout, cr.sin);
	chanbank::k_bank_scatter<<<grid_for((size_t)S * cr.g.maxout), 256, 0, q>>>(h->bank_v, bins, (size_t)bins_stride, h->bank_m, S, h->chan_per, cr.g.Tin,
	                                                                        cr.g.D, cr.g.maxout, h->chan_iq, h->chan_stride, cr.dcnt, cr.sin, cr.sout);
	if (sv >= 0)
		chanbank::k_bank_power_plain<<<grid_for((size_t)cr.nsrc << h->bank_m), 256, 0, q>>>(h->bank_v, h->bank_m, cr.nsrc, h->chan_per, cr.g.Tin, cr.g.D,
		                                                                                 cr.g.maxout, cr.sin, h->sv.d_power[sv], h->sv.d_frames[sv]);
	channel::k_source_history<<<grid_for((size_t)cr.nsrc * (channel::kHist / 8)), 256, 0, q>>>(cr.f.iq, cr.f.src_stride, cr.hist_in, cr.hist_out,
	                                                                                        cr.nsrc, cr.g.Tin);
	return 0;
}

// ROUTE_CHAN_BOXCAR / _FIR / _FIR_PLAIN / _BANK / _BANK_PLAIN: the channel front end of a run and what follows it.  (The
// boxcar's cross-check is run_staged behind k_channel_mix, ROUTE_CHAN_MIX: not here.)  Option source_dc's pre-pass runs
// inside the timed pair, as the front ends' raw-DC pre-pass does.
static int run_channels(RunFrame &f)
{
	rtlfm_gpu *h = f.h;
	const int route = f.pl.route;
	ChanRun cr{f.pl.g};
	const uint8_t *raw; size_t raw_stride;
	source_iq_redirect(f, &raw, &raw_stride);
	int r = chan_run_prepare(f, cr);
	if (r < 0) return r;
	if ((r = timing_begin(h, f.ev)) < 0) return r;
	if ((r = launch_source_side(h, raw, raw_stride, f.d_iq, f.stream_stride, f.nblocks, cr.sin, cr.sout, route != RTLFM_ROUTE_CHAN_BOXCAR)) < 0) return r;
	switch (route) {
	case RTLFM_ROUTE_CHAN_BOXCAR: r = launch_channel_boxcar(h, cr); break;
	case RTLFM_ROUTE_CHAN_FIR: r = launch_channel_fir(h, true, cr); break;
	case RTLFM_ROUTE_CHAN_FIR_PLAIN: r = launch_channel_fir(h, false, cr); break;
	case RTLFM_ROUTE_CHAN_BANK: r = launch_channel_bank(h, true, cr); break;
	case RTLFM_ROUTE_CHAN_BANK_PLAIN: r = launch_channel_bank(h, false, cr); break;
	default: return -EFAULT;  // planning bug
	}
	if (r < 0) return r;
	if ((r = timing_end(h, f.ev)) < 0) return r;
	if (f.pl.rest == RTLFM_REST_NONE) return raw_out_len(f);
	return run_back_half(f, h->chan_iq, h->chan_stride);
}

// Option source_dc's pre-pass alone, as one timed pair (tools/source_dc_bench.py): the sums and the smoothing over d_iq's
// source rows, into the handle's list.  Nothing a run carries moves: the records it writes are the next copy's, which every
// run overwrites first, and no history is read or written.
extern "C" int rtlfm_gpu_source_dc_prepass(rtlfm_gpu *h, const uint8_t *d_iq, size_t stream_stride, int nblocks)
{
	if (!h || !d_iq || nblocks < 1) return -EINVAL;
	if (nblocks > h->cap_blocks) return -E2BIG;
	if (((uintptr_t)d_iq & 15) || (stream_stride & 15) || stream_stride < (size_t)nblocks * h->cfg.block_len) return -EINVAL;
	if (!h->opt.source_dc || h->chan_per <= 0) return -ENOTSUP;
	if (ingest_busy(h)) return -EBUSY;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(sync_all(h));  // (the next state copy may still be an audio tail's)
	std::pair<Event, Event> ev;
	int r = timing_begin(h, ev);
	if (r < 0) return r;
	if ((r = launch_source_dc(h, d_iq, stream_stride, nblocks, h->st[h->st_cur], h->st[(h->st_cur + 1) % 3], false, false)) < 0) return r;
	if ((r = timing_end(h, ev)) < 0) return r;
	HIP_TRY(hipGetLastError());
	return 0;
}

static int ensure_input_stats(rtlfm_gpu *h)
{
	return h->d_istats.alloc((size_t)h->nstreams * h->cap_blocks);
}

static int ensure_input_health(rtlfm_gpu *h)
{
	return h->d_ihealth.alloc((size_t)h->nstreams * h->cap_blocks);
}

// The raw-byte readers in front of a run's front end: with input_health on, k_input_health, which takes the statistics
// along when input_stats is on as well (the input is read once); with input_stats alone, k_input_stats as ever.
// Records of buffer j of stream s at [(s0 + s) * rec_stride + j0 + j].
static int launch_input_readers(rtlfm_gpu *h, const uint8_t *d_iq, size_t stream_stride, uint32_t len, int nblocks, int S,
                                size_t rec_off, int rec_stride)
{
	const bool nt = h->opt.input_stats_nt != 0;
	if (h->opt.input_health)
		return ihealth::launch(d_iq, stream_stride, len, nblocks, S, h->d_ihealth + rec_off, rec_stride, nt, h->stream,
		                       h->opt.input_stats ? h->d_istats + rec_off : nullptr);
	if (h->opt.input_stats)
		return istats::launch(d_iq, stream_stride, len, nblocks, S, h->d_istats + rec_off, rec_stride, nt, h->stream);
	return 0;
}

static int ensure_gate(rtlfm_gpu *h)
{
	return h->d_gate.alloc((size_t)h->nstreams * h->cap_blocks);
}

// The squelch gate, the last launch of a run (option squelch_gate): on the handle's stream, behind the audio tail wherever
// that ran.  Reads this step's sin and the finished rows; writes the records, the clamped squelch_hits of sout and the
// per-stream counts (d_cnt of this step and the caller's d_out_len).
static int launch_gate(rtlfm_gpu *h, const RunGeom &g, int nblocks, int16_t *d_out, size_t out_stride, int32_t *d_out_len)
{
	const rtlfm_cfg &c = h->cfg;
	if (gate_supported(c) < 0) return -ENOTSUP;  // (a short buffer of a ragged run may be one the passes do not divide)
	if (!h->d_gate) return -EFAULT;              // views do not allocate: rtlfm_gpu_run_device / run_ragged did
	const int par = (int)(h->step & 1);
	if (h->tail_pending[par]) HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_tail[par], 0));  // this step's tail, on its own stream
	scan::GateParams p{};
	p.levels = h->d_levels;
	p.sin = h->st[h->st_cur]; p.sout = h->st[(h->st_cur + 1) % 3];
	p.R = d_out; p.rstride = out_stride;
	p.recs = h->d_gate + h->gate_rec_off;
	p.rec_stride = h->gate_rec_stride ? h->gate_rec_stride : nblocks;
	p.cnt = h->d_cnt[par]; p.cnt2 = d_out_len;
	p.nblocks = nblocks;
	p.N = g.Nblk; p.D = g.D;
	p.mul = c.mode == RTLFM_MODE_RAW ? 2 : 1;
	p.level = c.squelch_level; p.conseq = h->opt.conseq_squelch;
	std::pair<Event, Event> ev;
	int r = timing_begin(h, ev);
	if (r < 0) return r;
	if ((r = scan::launch_gate(p, h->nstreams, h->stream)) < 0) return r;
	return timing_end(h, ev);
}

// what of the handle steers a run's plan (rtlfm_route_opts): the bank, while set, takes precedence over the filter, and
// the filter over the boxcar
static rtlfm_route_opts route_opts(const rtlfm_gpu *h)
{
	const int channels = h->chan_per <= 0 ? RTLFM_CHANNELS_OFF
	                     : h->bank_K > 0 ? RTLFM_CHANNELS_BANK : h->fir_ntaps > 0 ? RTLFM_CHANNELS_FILTER : RTLFM_CHANNELS_MIXER;
	return rtlfm_route_opts{h->path, h->fws.pass0_engine, h->opt.squelch_fused, h->opt.deep_rest, h->opt.deemph_four_pass,
	                        h->opt.deemph_sequential, h->opt.arb_serial, h->no_deemph_scan ? 1 : 0, channels};
}

extern "C" int rtlfm_run_route(const rtlfm_cfg *cfg, int nstreams, int nblocks, unsigned out_low_bits, size_t out_stride,
                               const rtlfm_route_opts *opts, rtlfm_route_plan *plan)
{
	return run_route(cfg, nstreams, nblocks, out_low_bits, out_stride, opts, plan);
}

// one execution of a run: everything rtlfm_gpu_run_device does except moving on to the next state copy / step.
// The plan (run_plan.h) decides what can be decided before the first launch; one launcher per route does the rest.
static int run_device_once(rtlfm_gpu *h, const uint8_t *d_iq, size_t stream_stride, int nblocks,
                           int16_t *d_out, size_t out_stride, int32_t *d_out_len)
{
	rtl_debug::poison_lds(h->stream);  // RTLFM_POISON=1 only
	const size_t S = (size_t)h->nstreams;
	const int par = (int)(h->step & 1);
	int r;
	// this step reuses the res[] / d_cnt[] set and the state copy the step before last handed to
	// its audio tail
	if (h->tail_pending[par]) {
		HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_tail[par], 0));
		h->tail_pending[par] = false;
	}
	const RunPlan pl = plan_run(h->cfg, h->nstreams, nblocks, route_opts(h), (unsigned)((uintptr_t)d_out & 15), out_stride);
	if (pl.route < 0) return pl.route;
	// the callback's ADC statistics (src/rtl_fm.c:1302-1324) come before the conversion: in front of whichever front end runs
	// (channels on: the readers and the gate are off - rtlfm_gpu_set_channels and the options refuse each other)
	if (h->opt.input_stats && (r = ensure_input_stats(h)) < 0) return r;
	if (h->opt.input_health && (r = ensure_input_health(h)) < 0) return r;
	if ((r = launch_input_readers(h, d_iq, stream_stride, h->cfg.block_len, nblocks, (int)S, 0, nblocks)) < 0) return r;
	// state is double-buffered: kernels read st[cur], write the next copy.  The staged kernels and the channel front ends
	// each update their own fields, so the record is copied first; k_fused and k_boxcar_scan copy it themselves.
	state_t *sout = h->st[(h->st_cur + 1) % 3];
	if (pl.copy_state) HIP_TRY(hipMemcpyAsync(sout, h->st[h->st_cur], S * sizeof(state_t), hipMemcpyDeviceToDevice, h->stream));
	RunFrame f{h, pl, d_iq, stream_stride, nblocks, d_out, out_stride, d_out_len, h->stream, h->st[h->st_cur], sout, h->d_cnt[par]};
	switch (pl.route) {
	case RTLFM_ROUTE_STAGED:
	case RTLFM_ROUTE_CHAN_MIX: r = run_staged(f); break;
	case RTLFM_ROUTE_FUSED: r = run_fused(f); break;
	case RTLFM_ROUTE_FUSED_EMIT: r = run_fused_emit(f); break;
	case RTLFM_ROUTE_BOXCAR: r = run_boxfused(f); break;
	case RTLFM_ROUTE_BOXCAR_EMIT: r = run_boxfused_emit(f); break;
	default: r = run_channels(f); break;
	}
	if (r < 0) return r;
	h->last_path = pl.last_path;
	h->last_route = pl.route;
	h->last_rest = pl.rest;
	if (h->opt.squelch_gate && (r = launch_gate(h, pl.g, nblocks, d_out, out_stride, d_out_len)) < 0) return r;
	HIP_TRY(hipGetLastError());
	return 0;
}

// verify_twice: rows of two executions of one run, dword by dword up to each stream's length; lengths; state records
__global__ void k_verify_rows(const int16_t *a, const int16_t *b, size_t stride, const int32_t *la, const int32_t *lb, int S,
                              unsigned long long *cnt)
{
	const int s = blockIdx.x;
	if (s >= S) return;
	const int n = la[s];
	if (threadIdx.x == 0 && n != lb[s]) atomicAdd(cnt + 1, 1ull);
	const int16_t *ra = a + (size_t)s * stride, *rb = b + (size_t)s * stride;
	unsigned long long bad = 0, first = 0;
	for (int i = threadIdx.x; i < n; i += blockDim.x)
		if (ra[i] != rb[i]) { bad++; if (!first) first = ((unsigned long long)s << 32 | (unsigned)i) + 1; }
	if (bad) { atomicAdd(cnt, bad); atomicMin(cnt + 3, first); }
}
__global__ void k_verify_words(const uint32_t *a, const uint32_t *b, size_t n, unsigned long long *cnt)
{
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n && a[i] != b[i]) atomicAdd(cnt + 2, 1ull);
}

// The debug option verify_twice (round 6, VERDICT r5 task 1b): the run is executed twice from the same carried state -
// first into shadow rows, then into the caller's - with the device idle in between, and rows, lengths and the state
// records the two executions left are compared on the device.  A difference is a TRANSIENT fault of the device code
// (the kernels are deterministic functions of their input: tools/determinism_stress.py); a result that differs from the
// oracle while the two executions agree is a deterministic fault, or one outside the launch (the upload, the download).
static int run_device_verified(rtlfm_gpu *h, const uint8_t *d_iq, size_t stream_stride, int nblocks,
                               int16_t *d_out, size_t out_stride, int32_t *d_out_len)
{
	const size_t S = (size_t)h->nstreams;
	const size_t need = S * out_stride;
	OWN_TRY(h->vt_out.grow(need, h->stream));
	OWN_TRY(h->vt_len.alloc(S));
	OWN_TRY(h->vt_len2.alloc(S));
	OWN_TRY(h->vt_state.alloc(S));
	OWN_TRY(h->vt_cnt.alloc(4));
	state_t *sout = h->st[(h->st_cur + 1) % 3];
	int r = run_device_once(h, d_iq, stream_stride, nblocks, h->vt_out, out_stride, h->vt_len);
	if (r < 0) return r;
	HIP_TRY(sync_all(h));
	// (on the handle's own stream and waited for: a device-to-device hipMemcpy is only ordered on the NULL stream and returns
	// before it has run - the second execution, on a non-blocking stream, then overwrote the record while it was being copied,
	// and the comparison reported state words that had never differed: one red run of the suite in round 6)
	HIP_TRY(hipMemcpyAsync(h->vt_state, sout, S * sizeof(state_t), hipMemcpyDeviceToDevice, h->stream));
	if (h->opt.squelch_gate) {
		OWN_TRY(h->vt_gate.alloc(S * h->cap_blocks));
		HIP_TRY(hipMemcpyAsync(h->vt_gate, h->d_gate, S * nblocks * sizeof(rtlfm_gate_rec), hipMemcpyDeviceToDevice, h->stream));
	}
	HIP_TRY(hipStreamSynchronize(h->stream));
	if (h->opt.verify_inject) {
		// (tests: a difference the comparison must report - the shadow's first sample with every bit turned over)
		int16_t v = 0;
		HIP_TRY(hipMemcpy(&v, h->vt_out, sizeof(v), hipMemcpyDeviceToHost));
		v = (int16_t)~v;
		HIP_TRY(hipMemcpy(h->vt_out, &v, sizeof(v), hipMemcpyHostToDevice));
	}
	int32_t *len2 = d_out_len ? d_out_len : h->vt_len2;
	r = run_device_once(h, d_iq, stream_stride, nblocks, d_out, out_stride, len2);
	if (r < 0) return r;
	HIP_TRY(sync_all(h));
	const unsigned long long init[4] = {0, 0, 0, ~0ull};
	HIP_TRY(hipMemcpy(h->vt_cnt, init, sizeof(init), hipMemcpyHostToDevice));
	k_verify_rows<<<(unsigned)S, 256, 0, h->stream>>>(h->vt_out, d_out, out_stride, h->vt_len, len2, (int)S, h->vt_cnt);
	const size_t nw = S * sizeof(state_t) / 4;
	k_verify_words<<<(unsigned)((nw + 255) / 256), 256, 0, h->stream>>>(reinterpret_cast<const uint32_t *>(h->vt_state.get()),
	                                                                  reinterpret_cast<const uint32_t *>(sout), nw, h->vt_cnt);
	if (h->opt.squelch_gate) {  // the gate's records count with the state words
		const size_t gw = S * nblocks * sizeof(rtlfm_gate_rec) / 4;
		k_verify_words<<<(unsigned)((gw + 255) / 256), 256, 0, h->stream>>>(reinterpret_cast<const uint32_t *>(h->vt_gate.get()),
		                                                                  reinterpret_cast<const uint32_t *>(h->d_gate.get()), gw, h->vt_cnt);
	}
	unsigned long long got[4];
	HIP_TRY(hipMemcpyAsync(got, h->vt_cnt, sizeof(got), hipMemcpyDeviceToHost, h->stream));
	HIP_TRY(hipStreamSynchronize(h->stream));
	h->vt_runs++;
	if (got[0] || got[1] || got[2]) {
		h->vt_mismatches++;
		fprintf(stderr, "rtlfm_hip: verify_twice: two executions of one run differ: %llu PCM samples, %llu lengths, %llu state words; "
		        "first at stream %llu sample %llu (run %ld of this handle, input %p, rows %p / shadow %p)\n",
		        got[0], got[1], got[2], got[0] ? (got[3] - 1) >> 32 : 0ull, got[0] ? (got[3] - 1) & 0xffffffffull : 0ull,
		        h->vt_runs, (const void *)d_iq, (void *)d_out, (void *)h->vt_out);
	}
	return 0;
}

static int run_device_impl(rtlfm_gpu *h, const uint8_t *d_iq, size_t stream_stride, int nblocks,
                           int16_t *d_out, size_t out_stride, int32_t *d_out_len);

// ---- the survey's two sets (option bank_survey) ----

static int survey_free(rtlfm_gpu *h, bool wait)
{
	rtlfm_gpu::Survey &sv = h->sv;
	if (wait && sv.d_power[0]) {
		HIP_TRY(hipSetDevice(h->device));
		HIP_TRY(sync_all(h));
	}
	sv = rtlfm_gpu::Survey{};  // (the sets go with it)
	return 0;
}

// the sets, for the sources and the K there are now (grown behind whatever still reads them: what they held is gone)
static int survey_ensure(rtlfm_gpu *h)
{
	rtlfm_gpu::Survey &sv = h->sv;
	const int nsrc = h->nstreams / h->chan_per;
	const size_t need = (size_t)nsrc * h->bank_K;
	if (sv.d_power[0] && sv.d_power[0].capacity() >= need && sv.cap_srcs >= nsrc) return 0;
	int r = survey_free(h, true);
	if (r < 0) return r;
	for (int k = 0; k < 2; k++) {
		OWN_TRY(sv.d_power[k].alloc(need));
		OWN_TRY(sv.d_frames[k].alloc((size_t)nsrc));
		OWN_TRY(sv.ev[k].create(hipEventDisableTiming));
	}
	sv.cap_srcs = nsrc;
	return 0;
}

// a run has been queued: `wrote` is the set it wrote, or -1
static void survey_advance(rtlfm_gpu *h, int wrote)
{
	rtlfm_gpu::Survey &sv = h->sv;
	sv.prev = sv.last;
	sv.last = wrote;
	if (wrote >= 0) {
		sv.K[wrote] = h->bank_K;
		sv.nsrc[wrote] = h->nstreams / h->chan_per;
		sv.next = wrote ^ 1;
	}
}

static int survey_fetch(rtlfm_gpu *h, bool prev, uint64_t *power, size_t cap, int32_t *frames, int *K)
{
	if (!h || !K || !frames || (!power && cap)) return -EINVAL;
	const rtlfm_gpu::Survey &sv = h->sv;
	const int k = prev ? sv.prev : sv.last;
	if (k < 0 || !sv.d_power[k]) return -ENODATA;
	*K = sv.K[k];  // (written even where power does not fit)
	const size_t n = (size_t)sv.nsrc[k] * sv.K[k];
	if (cap < n) return -ENOBUFS;
	HIP_TRY(hipSetDevice(h->device));
	if (prev) {
		HIP_TRY(hipEventSynchronize(sv.ev[k]));  // (that run's own event: not the run started since)
	} else {
		HIP_TRY(sync_all(h));
	}
	HIP_TRY(hipMemcpy(power, sv.d_power[k], n * sizeof(uint64_t), hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(frames, sv.d_frames[k], (size_t)sv.nsrc[k] * sizeof(int32_t), hipMemcpyDeviceToHost));
	return 0;
}

extern "C" int rtlfm_gpu_bank_survey(rtlfm_gpu *h, uint64_t *power, size_t cap, int32_t *frames, int *K)
{
	return survey_fetch(h, false, power, cap, frames, K);
}

extern "C" int rtlfm_gpu_bank_survey_prev(rtlfm_gpu *h, uint64_t *power, size_t cap, int32_t *frames, int *K)
{
	return survey_fetch(h, true, power, cap, frames, K);
}

extern "C" int rtlfm_gpu_run_device(rtlfm_gpu *h, const uint8_t *d_iq, size_t stream_stride, int nblocks,
                                    int16_t *d_out, size_t out_stride, int32_t *d_out_len)
{
	if (!h) return -EINVAL;
	if (h->mute_streams > 0) return -EBUSY;  // the input is const here: a pending rtlfm_gpu_mute belongs to push / run
	return run_device_impl(h, d_iq, stream_stride, nblocks, d_out, out_stride, d_out_len);
}

static int run_device_impl(rtlfm_gpu *h, const uint8_t *d_iq, size_t stream_stride, int nblocks,
                           int16_t *d_out, size_t out_stride, int32_t *d_out_len)
{
	if (!h || !d_iq || !d_out || nblocks < 1) return -EINVAL;
	if (nblocks > h->cap_blocks) return -E2BIG;
	if (((uintptr_t)d_iq & 15) || (stream_stride & 15) || ((uintptr_t)d_out & 3) || (out_stride & 1)) return -EINVAL;
	if (stream_stride < (size_t)nblocks * h->cfg.block_len) return -EINVAL;
	HIP_TRY(hipSetDevice(h->device));
	if (h->opt.squelch_gate && !h->gate_rec_stride) {  // (a view's records were allocated by run_ragged)
		const int g = ensure_gate(h);
		if (g < 0) return g;
	}
	if (!h->src_rec_stride) {  // (the same)
		int e = ensure_source_records(h);
		if (e < 0 || (e = ensure_source_iq(h)) < 0) return e;
	}
	// the survey: of every run the bank takes while the option is on (both executions of a verified run write the same set:
	// each stores, neither adds)
	const bool surveyed = h->opt.bank_survey && h->chan_per > 0 && h->bank_K > 0;
	if (surveyed) {
		const int e = survey_ensure(h);
		if (e < 0) return e;
		h->sv.writing = h->sv.next;
	}
	const int r = h->opt.verify_twice ? run_device_verified(h, d_iq, stream_stride, nblocks, d_out, out_stride, d_out_len)
	                                  : run_device_once(h, d_iq, stream_stride, nblocks, d_out, out_stride, d_out_len);
	const int wrote = h->sv.writing;
	h->sv.writing = -1;
	if (r < 0) return r;
	survey_advance(h, wrote);
	if (wrote >= 0) HIP_TRY(hipEventRecord(h->sv.ev[wrote], h->stream));
	h->st_cur = (h->st_cur + 1) % 3;
	h->step++;
	if (h->chan_per > 0) h->chan_pos += (uint64_t)nblocks * (h->cfg.block_len / 2);  // (once per run, also under verify_twice)
	if (h->chan_per > 0 && (h->bank_K > 0 || h->fir_ntaps > 0)) h->src_hist_cur ^= 1;  // (the same: both executions read one history and wrote the other)
	h->last_nblocks = nblocks;
	h->stats_nblocks = h->opt.input_stats ? nblocks : 0;
	h->health_nblocks = h->opt.input_health ? nblocks : 0;
	h->gate_nblocks = h->opt.squelch_gate ? nblocks : 0;
	h->src_stats_nblocks = h->chan_per > 0 && h->opt.source_stats ? nblocks : 0;
	h->src_health_nblocks = h->chan_per > 0 && h->opt.source_health ? nblocks : 0;
	h->siq_nblocks = h->chan_per > 0 && h->opt.source_iq ? nblocks : 0;
	return 0;
}

// The records a run leaves per buffer on the device, [stream][count]: one stream's, or (`all`) every stream's as rows of
// `cap` records.  One contract for all of them, rtlfm_gpu_levels': bad arguments, then "not enabled", then the count -
// written even where it does not fit -, then the copy.
template <class Rec>
static int fetch_records(rtlfm_gpu *h, DevBuf<Rec> rtlfm_gpu::*recs, int rtlfm_gpu::*count_of, bool (*enabled)(const rtlfm_gpu *),
                         bool all, int stream, Rec *out, int cap, int *n, bool by_source = false)
{
	// (by_source: rows are sources, of a handle whose last run channels took - `enabled` says -ENODATA otherwise)
	const int rows = !h ? 0 : !by_source ? h->nstreams : h->chan_per > 0 ? h->nstreams / h->chan_per : h->nstreams;
	if (!h || !out || !n || (!all && (stream < 0 || stream >= rows))) return -EINVAL;
	if (!enabled(h)) return -ENODATA;
	const int count = h->*count_of;
	*n = count;
	if (count > cap) return -ENOBUFS;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(sync_all(h));
	if (count <= 0) return 0;
	const size_t row = (size_t)count * sizeof(Rec);
	if (all)
		HIP_TRY(hipMemcpy2D(out, (size_t)cap * sizeof(Rec), h->*recs, row, row, (size_t)rows, hipMemcpyDeviceToHost));
	else
		HIP_TRY(hipMemcpy(out, h->*recs + (size_t)stream * count, row, hipMemcpyDeviceToHost));
	return 0;
}
static bool levels_on(const rtlfm_gpu *h) { return h->cfg.squelch_level || h->cfg.report_levels; }
static bool gate_on(const rtlfm_gpu *h) { return h->opt.squelch_gate != 0; }
static bool stats_on(const rtlfm_gpu *h) { return h->opt.input_stats != 0; }
static bool health_on(const rtlfm_gpu *h) { return h->opt.input_health != 0; }

// rms() per buffer of the last run (the squelch's, -L's)
extern "C" int rtlfm_gpu_levels(rtlfm_gpu *h, int stream, int32_t *rms, int cap, int *n)
{
	return fetch_records(h, &rtlfm_gpu::d_levels, &rtlfm_gpu::last_nblocks, levels_on, false, stream, rms, cap, n);
}
extern "C" int rtlfm_gpu_levels_all(rtlfm_gpu *h, int32_t *rms, int cap, int *n)
{
	return fetch_records(h, &rtlfm_gpu::d_levels, &rtlfm_gpu::last_nblocks, levels_on, true, 0, rms, cap, n);
}
// The last run's gate records (k_scan_gate, option squelch_gate)
extern "C" int rtlfm_gpu_gate(rtlfm_gpu *h, int stream, rtlfm_gate_rec *out, int cap, int *n)
{
	return fetch_records(h, &rtlfm_gpu::d_gate, &rtlfm_gpu::gate_nblocks, gate_on, false, stream, out, cap, n);
}
extern "C" int rtlfm_gpu_gate_all(rtlfm_gpu *h, rtlfm_gate_rec *out, int cap, int *n)
{
	return fetch_records(h, &rtlfm_gpu::d_gate, &rtlfm_gpu::gate_nblocks, gate_on, true, 0, out, cap, n);
}
// The last run's ADC statistics (k_input_stats, option input_stats)
extern "C" int rtlfm_gpu_input_stats(rtlfm_gpu *h, int stream, rtlfm_input_stat *out, int cap, int *n)
{
	return fetch_records(h, &rtlfm_gpu::d_istats, &rtlfm_gpu::stats_nblocks, stats_on, false, stream, out, cap, n);
}
extern "C" int rtlfm_gpu_input_stats_all(rtlfm_gpu *h, rtlfm_input_stat *out, int cap, int *n)
{
	return fetch_records(h, &rtlfm_gpu::d_istats, &rtlfm_gpu::stats_nblocks, stats_on, true, 0, out, cap, n);
}
// The last run's input health records (k_input_health, option input_health)
extern "C" int rtlfm_gpu_input_health(rtlfm_gpu *h, int stream, rtlfm_input_health *out, int cap, int *n)
{
	return fetch_records(h, &rtlfm_gpu::d_ihealth, &rtlfm_gpu::health_nblocks, health_on, false, stream, out, cap, n);
}
extern "C" int rtlfm_gpu_input_health_all(rtlfm_gpu *h, rtlfm_input_health *out, int cap, int *n)
{
	return fetch_records(h, &rtlfm_gpu::d_ihealth, &rtlfm_gpu::health_nblocks, health_on, true, 0, out, cap, n);
}

// The last run's records per SOURCE (options source_stats / source_health): -ENODATA while the option is off and while the
// last run was not one that channels took
static bool source_stats_on(const rtlfm_gpu *h) { return h->opt.source_stats != 0 && h->chan_per > 0 && h->src_stats_nblocks > 0; }
static bool source_health_on(const rtlfm_gpu *h) { return h->opt.source_health != 0 && h->chan_per > 0 && h->src_health_nblocks > 0; }
extern "C" int rtlfm_gpu_source_stats(rtlfm_gpu *h, int source, rtlfm_input_stat *out, int cap, int *n)
{
	return fetch_records(h, &rtlfm_gpu::d_src_stats, &rtlfm_gpu::src_stats_nblocks, source_stats_on, false, source, out, cap, n, true);
}
extern "C" int rtlfm_gpu_source_stats_all(rtlfm_gpu *h, rtlfm_input_stat *out, int cap, int *n)
{
	return fetch_records(h, &rtlfm_gpu::d_src_stats, &rtlfm_gpu::src_stats_nblocks, source_stats_on, true, 0, out, cap, n, true);
}
extern "C" int rtlfm_gpu_source_health(rtlfm_gpu *h, int source, rtlfm_input_health *out, int cap, int *n)
{
	return fetch_records(h, &rtlfm_gpu::d_src_health, &rtlfm_gpu::src_health_nblocks, source_health_on, false, source, out, cap, n, true);
}
extern "C" int rtlfm_gpu_source_health_all(rtlfm_gpu *h, rtlfm_input_health *out, int cap, int *n)
{
	return fetch_records(h, &rtlfm_gpu::d_src_health, &rtlfm_gpu::src_health_nblocks, source_health_on, true, 0, out, cap, n, true);
}

// The last run's second moments per SOURCE (option source_iq, k_source_iq): the same contract
static bool source_iq_on(const rtlfm_gpu *h) { return h->opt.source_iq != 0 && h->chan_per > 0 && h->siq_nblocks > 0; }
extern "C" int rtlfm_gpu_source_iq_sums(rtlfm_gpu *h, int source, rtlfm_iq_sums *out, int cap, int *n)
{
	return fetch_records(h, &rtlfm_gpu::d_siq_sums, &rtlfm_gpu::siq_nblocks, source_iq_on, false, source, out, cap, n, true);
}
extern "C" int rtlfm_gpu_source_iq_sums_all(rtlfm_gpu *h, rtlfm_iq_sums *out, int cap, int *n)
{
	return fetch_records(h, &rtlfm_gpu::d_siq_sums, &rtlfm_gpu::siq_nblocks, source_iq_on, true, 0, out, cap, n, true);
}

// The raw-byte readers as standalone operators on device memory (no handle): tools/input_stats_bench.py times them, and a
// caller that only wants to know which front ends clip needs no demodulator.  `outs`: the record arrays, 16-byte aligned.
template <class Launch>
static int reader_device_op(int device, const uint8_t *d_iq, std::initializer_list<const void *> outs, Launch launch)
{
	if (!d_iq) return -EINVAL;
	for (const void *p : outs)
		if (!p || ((uintptr_t)p & 15)) return -EINVAL;
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return -ENODEV;
	HIP_TRY(hipSetDevice(device));
	const int r = launch();
	if (r < 0) return r;
	HIP_TRY(hipGetLastError());
	return 0;
}

extern "C" int rtlfm_gpu_input_stats_device(int device, const uint8_t *d_iq, size_t stream_stride, uint32_t block_len, int nblocks,
                                            int nstreams, rtlfm_input_stat *d_out, int nontemporal, void *hip_stream)
{
	return reader_device_op(device, d_iq, {d_out}, [&] {
		return istats::launch(d_iq, stream_stride, block_len, nblocks, nstreams, d_out, nblocks, nontemporal != 0, (hipStream_t)hip_stream);
	});
}

extern "C" int rtlfm_gpu_input_health_device(int device, const uint8_t *d_iq, size_t stream_stride, uint32_t block_len, int nblocks,
                                             int nstreams, rtlfm_input_health *d_out, int nontemporal, void *hip_stream)
{
	return reader_device_op(device, d_iq, {d_out}, [&] {
		return ihealth::launch(d_iq, stream_stride, block_len, nblocks, nstreams, d_out, nblocks, nontemporal != 0, (hipStream_t)hip_stream);
	});
}

// ... and the launch a handle with both options on makes: both record arrays from one read of the input
extern "C" int rtlfm_gpu_input_health_stats_device(int device, const uint8_t *d_iq, size_t stream_stride, uint32_t block_len, int nblocks,
                                                   int nstreams, rtlfm_input_health *d_out, rtlfm_input_stat *d_stats, int nontemporal,
                                                   void *hip_stream)
{
	return reader_device_op(device, d_iq, {d_out, d_stats}, [&] {
		return ihealth::launch(d_iq, stream_stride, block_len, nblocks, nstreams, d_out, nblocks, nontemporal != 0, (hipStream_t)hip_stream,
		                       d_stats);
	});
}

extern "C" int rtlfm_gpu_mute(rtlfm_gpu *h, int stream, uint32_t nbytes)
{
	if (!h || stream < 0 || stream >= h->nstreams) return -EINVAL;
	if (h->chan_per > 0) return -ENOTSUP;  // (channels: the mute counts a stream's own input bytes)
	if (!h->mute_left) {
		if (!nbytes) return 0;
		h->mute_left.reset(new (std::nothrow) uint32_t[(size_t)h->nstreams]());
		if (!h->mute_left) return -ENOMEM;
	}
	h->mute_streams += (nbytes ? 1 : 0) - (h->mute_left[stream] ? 1 : 0);
	h->mute_left[stream] = nbytes;  // replaces what was pending, as `dongle.mute = ...`
	return 0;
}

extern "C" int rtlfm_gpu_mute_device(int device, uint8_t *d_iq, size_t stream_stride, int nstreams, size_t row_bytes,
                                     const uint32_t *mute_bytes, void *hip_stream)
{
	if (!d_iq || !mute_bytes || nstreams < 1) return -EINVAL;
	if (nstreams > 1 && stream_stride < row_bytes) return -EINVAL;
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return -ENODEV;
	HIP_TRY(hipSetDevice(device));
	std::vector<scan::MuteEntry> ent;
	uint32_t mx = 0;
	for (int s = 0; s < nstreams; s++) {
		const uint32_t m = (size_t)mute_bytes[s] < row_bytes ? mute_bytes[s] : (uint32_t)row_bytes;
		if (!m) continue;
		ent.push_back({(unsigned long long)s * stream_stride, m, 0});
		if (m > mx) mx = m;
	}
	if (ent.empty()) return 0;
	hipStream_t q = (hipStream_t)hip_stream;
	DevBuf<scan::MuteEntry> d_ent;
	OWN_TRY(d_ent.alloc(ent.size()));
	hipError_t e = hipMemcpy(d_ent, ent.data(), ent.size() * sizeof(scan::MuteEntry), hipMemcpyHostToDevice);
	int r = e == hipSuccess ? scan::launch_mute(d_iq, d_ent, (int)ent.size(), mx, q) : -EIO;
	if (hipStreamSynchronize(q) != hipSuccess) r = -EIO;  // the entries go when this returns
	return r;
}

// --------------------------------------------- callback-side: push / fetch ----
//
// What sits behind rtlsdr_read_async's callback (include/rtl-sdr.h:472).  librtlsdr owns the
// callback's buffer and resubmits it to USB the moment the callback returns
// (src/librtlsdr.c:2705-2707), so push() copies — into a pinned staging ring of two halves:
//
//   callbacks --memcpy--> h_stage[fill]      (shared lock: any number of streams at once, a slot
//                                             per (stream, buffer), per-stream atomic counters)
//   rtlfm_gpu_run(): flips `fill` (exclusive lock held only for the count check and the flip),
//                    then h_stage[f] --async H2D, copy stream--> d_in[f] --kernels--> d_result[f]
//
// so callbacks never wait for a transfer or a kernel: while run k's H2D and kernels are in
// flight the callbacks fill the other half, and run k + 1's H2D overlaps run k's kernels.  A half
// is handed back to the callbacks when its H2D has completed (event), d_in[f] is overwritten when
// the kernels that read it are done (event), results are double-buffered likewise: those of a run
// stay valid until the second run after it.
//
// len is the transfer's actual_length and may be short (src/rtl_fm.c:1326-1341 uses len
// throughout).  Full buffers take the batched path; a run that holds a short buffer goes buffer
// by buffer, each contiguous range of streams with the same length through a view of the handle
// configured for that length (the chain's carried state makes this exact, and rare).
//
// Rows.  The input side - h_stage, d_in, h_len, pushed, open_slot - has ring_rows() rows: one per stream, or one per
// SOURCE with option source_ring while channels are on (the `stream` of push / acquire / commit is then the source).  The
// result side is per stream throughout.  set_channels and the option rebuild the input side when the count changes
// (ingest_resize), on a ring that holds nothing; results of earlier runs stay where they are.
struct Ingest {
	int rows = 0;                               // of the input side, as built (0: a rebuild failed; ingest_ensure tries again)
	struct Input {                              // what a change of the row count replaces (ingest_resize_locked), as one
		PinnedBuf<uint8_t> h_stage[2];          // pinned, [row][cap_blocks][block_len]
		DevBuf<uint8_t> d_in[2];
	} inp;
	std::vector<uint32_t> h_len[2];             // bytes in each slot
	std::unique_ptr<std::atomic<int>[]> pushed[2];
	std::unique_ptr<std::atomic<int>[]> open_slot;  // [stream] 1 + half while a slot is out between acquire and commit
	int fill = 0;                               // guarded by mu (shared: read, exclusive: flip)
	std::shared_mutex mu;
	hipStream_t copy_stream = nullptr;
	Event ev_h2d[2], ev_run[2];
	bool h2d_pending[2] = {false, false}, run_pending[2] = {false, false};
	DevBuf<int16_t> d_result[2];                // ostride int16 per stream; [1] is an alias into [0]'s block unless it had to be placed apart
	DevBuf<int32_t> d_result_len[2];
	size_t ostride = 0;
	int pending_f = -1, pending_nb = 0;         // rtlfm_gpu_run_begin() has flipped the halves, _end() has not run yet
	bool pending_ragged = false;
	int last = -1;                              // half of the last run
	int prev = -1;                              // ... and of the run before it (rtlfm_gpu_fetch_all_prev)
	int tail_par[2] = {0, 0};                   // per half: step parity of its run, and whether that run left an audio tail
	bool tail_any[2] = {false, false};          // on the tail stream (ev_tail[parity])
	PinnedBuf<int16_t> h_result;                // pinned mirror of the last run's results (per-stream fetch)
	PinnedBuf<int32_t> h_result_len;
	bool mirror_valid = false;
	DevBuf<int16_t> d_tmp;                      // ragged runs: one buffer's results before they are appended
	DevBuf<int32_t> d_tmp_len;
	// packed results (option pack_results; pack_kernel.h): per half, allocated by the first packed run; the option back
	// at 0 drops them as one (ingest_pack_free)
	struct Pack {
		DevBuf<int16_t> d_packed[2];                // every row rounded up to 8, the worst case
		DevBuf<rtlfm_packed_row> d_pack_index[2];   // [nstreams]
		DevBuf<unsigned long long> d_pack_total[2];
		DevBuf<int32_t> d_piece_off;                // mode 2: [nstreams][cap_blocks], k_pack_plan's to k_pack_copy (one: both on the handle's stream)
		int pack_mode[2] = {0, 0};                  // how the half's run was packed (0: it was not)
		Event ev_pack[2][2];                        // around the two launches while timing is on
		bool pack_timed[2] = {false, false};
	} pk;
};

static std::mutex g_ingest_alloc_mu;

// what the handle's placed blocks really hold (a winning candidate of a placement search may be larger than the request:
// rtlfm_gpu_malloc_apart_ex): the ring's result block(s), the audio tail's work buffers, the emit mode's buffer
static size_t alloc_size(const void *p)
{
	hipDeviceptr_t base = nullptr;
	size_t size = 0;
	if (!p || hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return 0; }
	return size;
}
static long placement_held_mb(rtlfm_gpu *h)
{
	size_t b = alloc_size(h->res[0][0]) + (h->res[1][0].is_alias() ? 0 : alloc_size(h->res[1][0])) + alloc_size(h->deepA);
	if (Ingest *in = __atomic_load_n(&h->ing, __ATOMIC_ACQUIRE))
		b += alloc_size(in->d_result[0]) + (in->d_result[1].is_alias() ? 0 : alloc_size(in->d_result[1]));
	return (long)(b >> 20);
}

// option pack_results back to 0: what the pack allocated goes, behind whatever still reads or writes it
static int ingest_pack_free(rtlfm_gpu *h)
{
	Ingest *in = __atomic_load_n(&h->ing, __ATOMIC_ACQUIRE);
	if (!in || !in->pk.d_packed[0]) return 0;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(sync_all(h));
	in->pk = Ingest::Pack{};
	return 0;
}

static int ingest_pack_us(rtlfm_gpu *h, long *us)
{
	Ingest *in = __atomic_load_n(&h->ing, __ATOMIC_ACQUIRE);
	*us = -1;
	if (!in || in->last < 0 || !in->pk.pack_mode[in->last] || !in->pk.pack_timed[in->last]) return 0;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(hipEventSynchronize(in->pk.ev_pack[in->last][1]));
	float ms = 0;
	HIP_TRY(hipEventElapsedTime(&ms, in->pk.ev_pack[in->last][0], in->pk.ev_pack[in->last][1]));
	*us = (long)(ms * 1000.0f + 0.5f);
	return 0;
}

static void ingest_free(Ingest *in)
{
	if (!in) return;
	if (in->copy_stream) { int dev_ = 0; (void)hipGetDevice(&dev_); rtl_pool::stream_put(dev_, 0, in->copy_stream); }
	delete in;
}

// the input side, for the rows there are now
static int ingest_build_input(rtlfm_gpu *h, Ingest *in)
{
	const size_t R = (size_t)ring_rows(h);
	const size_t bytes = R * h->cap_blocks * h->cfg.block_len;
	for (int k = 0; k < 2; k++) {
		OWN_TRY(in->inp.h_stage[k].alloc(bytes));
		OWN_TRY(in->inp.d_in[k].alloc(bytes));
		in->h_len[k].assign(R * h->cap_blocks, 0);
		in->pushed[k].reset(new std::atomic<int>[R]);
		for (size_t s = 0; s < R; s++) in->pushed[k][s].store(0);
	}
	in->open_slot.reset(new std::atomic<int>[R]);
	for (size_t s = 0; s < R; s++) in->open_slot[s].store(0);
	in->rows = (int)R;
	return 0;
}

static int ingest_build(rtlfm_gpu *h, Ingest *in)
{
	const size_t S = (size_t)h->nstreams;
	HIP_TRY(hipSetDevice(h->device));
	in->ostride = ((size_t)rtlfm_result_cap(&h->cfg) * h->cap_blocks + 16 + 63) & ~(size_t)63;
	HIP_TRY(rtl_pool::stream_get(h->device, 0, &in->copy_stream));
	int rb = ingest_build_input(h, in);
	if (rb < 0) return rb;
	const size_t bytes = (size_t)in->rows * h->cap_blocks * h->cfg.block_len;
	for (int k = 0; k < 2; k++) {
		OWN_TRY(in->d_result_len[k].alloc(S));
		OWN_TRY(in->ev_h2d[k].create(hipEventDisableTiming));
		OWN_TRY(in->ev_run[k].create(hipEventDisableTiming));
	}
	{
		// the results away from the input they are demodulated from (rtlfm_gpu_malloc_apart_ex; plain memory when the
		// ring is too small for it to matter).  Both halves' results as ONE block placed against the first half's input;
		// the second half's input was allocated right behind the first and is almost always of the same class - one probe
		// says whether it is, and only if not the second half gets a block and a search of its own.
		const size_t one = (S * in->ostride * sizeof(int16_t) + 255) & ~(size_t)255;
		const size_t budget = (size_t)h->place.budget_gb << 30;
		const size_t one_elems = one / sizeof(int16_t);
		void *q = nullptr;
		DevBuf<int16_t> p;
		int apart = 0; double ms = 0; size_t walked = 0;
		int r = rtlfm_gpu_malloc_apart_ex(h->device, 2 * one, in->inp.d_in[0], bytes, budget, &q, &apart, &ms, &walked);
		if (r < 0) return r;
		OWN_TRY(p.adopt(q, 2 * one_elems));
		h->place.search_ms += ms;
		if (walked > h->place.walked_peak) h->place.walked_peak = walked;
		h->place.ring_tries = 1;
		if ((!apart && walked > 0) || h->place.force_retry) {  // (force_retry: option "ring_force_retry", tests)
			// A search was made and every candidate within its bound shared the input's class (round 5 met boxes where one class
			// runs on for more than 16 GB).  Here the handle owns the OTHER side as well: the ring's device inputs move - new ones
			// are allocated while the old ones are still held, so that they come from somewhere else - and the search runs once
			// more against them.  One retry; whatever it finds is what the ring gets.
			DevBuf<uint8_t> n0, n1;
			if (n0.alloc(bytes, true) == 0 && n1.alloc(bytes, true) == 0) {  // (quietly: without them there is simply no retry)
				p.reset();
				int apart2 = 0;
				r = rtlfm_gpu_malloc_apart_ex(h->device, 2 * one, n0, bytes, budget, &q, &apart2, &ms, &walked);
				if (r < 0) return r;
				OWN_TRY(p.adopt(q, 2 * one_elems));
				h->place.search_ms += ms;
				if (walked > h->place.walked_peak) h->place.walked_peak = walked;
				h->place.ring_tries = 2;
				in->inp.d_in[0] = std::move(n0); in->inp.d_in[1] = std::move(n1);
				apart = apart2;
			} else {
				(void)hipGetLastError();
			}
		}
		in->d_result[0] = std::move(p);
		in->d_result[1] = in->d_result[0].alias(one_elems);
		h->place.ring_apart = apart;
		if (apart) {
			double rd = 0, rw = 0;
			const auto t0 = std::chrono::steady_clock::now();
			const int both = rtlfm_gpu_placement_probe(h->device, in->inp.d_in[1], bytes, in->d_result[1], one, &rd, &rw);
			h->place.search_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
			if (both < 0) return both;
			if (!both) {
				void *p2 = nullptr; int apart2 = 0;
				r = rtlfm_gpu_malloc_apart_ex(h->device, one, in->inp.d_in[1], bytes, budget, &p2, &apart2, &ms, &walked);
				if (r < 0) return r;
				h->place.search_ms += ms;
				if (walked > h->place.walked_peak) h->place.walked_peak = walked;
				in->d_result[1].reset();  // (the alias goes: an owner of its own)
				OWN_TRY(in->d_result[1].adopt(p2, one_elems));
				h->place.ring_apart = apart2;
			}
		}
	}
	return 0;
}

// The row count has changed (rtlfm_gpu_set_channels, option source_ring): the input side once more, for the rows there are
// now.  The callers have found the ring idle and empty; what is in flight on the device is waited for.  The result side,
// `last` and `prev` stay: results of earlier runs remain fetchable.  (The results were placed against the old d_in:
// option ring_apart speaks of the ring as first built.)
static int ingest_resize_locked(rtlfm_gpu *h, Ingest *in)
{
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(sync_all(h));
	HIP_TRY(hipStreamSynchronize(in->copy_stream));
	std::unique_lock<std::shared_mutex> g(in->mu);
	in->inp = Ingest::Input{};
	in->rows = 0;
	in->h2d_pending[0] = in->h2d_pending[1] = false;
	return ingest_build_input(h, in);
}
static int ingest_resize(rtlfm_gpu *h)
{
	Ingest *in = __atomic_load_n(&h->ing, __ATOMIC_ACQUIRE);
	if (!in || in->rows == ring_rows(h)) return 0;
	std::lock_guard<std::mutex> g(g_ingest_alloc_mu);
	return ingest_resize_locked(h, in);
}

// the ring is built by whoever comes first (callbacks of many streams may arrive at once) and
// published only when it is complete
static int ingest_ensure(rtlfm_gpu *h)
{
	if (Ingest *in = __atomic_load_n(&h->ing, __ATOMIC_ACQUIRE))
		if (in->rows == ring_rows(h)) return 0;
	std::lock_guard<std::mutex> g(g_ingest_alloc_mu);
	if (h->ing) return h->ing->rows == ring_rows(h) ? 0 : ingest_resize_locked(h, h->ing);  // (a rebuild that failed in the setter)
	Ingest *in = new Ingest();
	int r = ingest_build(h, in);
	if (r < 0) {
		ingest_free(in);
		return r;
	}
	__atomic_store_n(&h->ing, in, __ATOMIC_RELEASE);
	return 0;
}

static void ingest_destroy(rtlfm_gpu *h)
{
	ingest_free(h->ing);
	h->ing = nullptr;
}

static void ingest_reset(rtlfm_gpu *h)
{
	Ingest *in = h->ing;
	if (!in) return;
	std::unique_lock<std::shared_mutex> g(in->mu);
	for (int k = 0; k < 2; k++)
		for (int s = 0; s < in->rows; s++) in->pushed[k][s].store(0);
	for (int s = 0; s < in->rows; s++) in->open_slot[s].store(0);
	in->last = -1;
	in->prev = -1;
	in->pending_f = -1;
	in->mirror_valid = false;
}

// a run begun and not ended, or a slot out between acquire and commit: the ring is in the middle of something
static bool ingest_busy(rtlfm_gpu *h)
{
	Ingest *in = __atomic_load_n(&h->ing, __ATOMIC_ACQUIRE);
	if (!in) return false;
	std::shared_lock<std::shared_mutex> g(in->mu);
	if (in->pending_f >= 0) return true;
	for (int s = 0; s < in->rows; s++)
		if (in->open_slot[s].load(std::memory_order_acquire)) return true;
	return false;
}

// buffers wait in the filling half
static bool ingest_queued(rtlfm_gpu *h)
{
	Ingest *in = __atomic_load_n(&h->ing, __ATOMIC_ACQUIRE);
	if (!in) return false;
	std::shared_lock<std::shared_mutex> g(in->mu);
	for (int s = 0; s < in->rows; s++)
		if (in->pushed[in->fill][s].load(std::memory_order_acquire) > 0) return true;
	return false;
}

extern "C" int rtlfm_gpu_push(rtlfm_gpu *h, int stream, const uint8_t *iq, uint32_t len)
{
	if (!h || !iq || stream < 0 || stream >= ring_rows(h)) return -EINVAL;  // (option source_ring with channels: the SOURCE)
	if (h->chan_per > 0 && !h->opt.source_ring) return -ENOTSUP;  // (channels: the ring's rows are per stream)
	// actual_length of a bulk transfer: whole 512-byte USB packets, at most the buffer
	if (len == 0 || len > h->cfg.block_len || len % 512) return -EINVAL;
	if (len != h->cfg.block_len) {
		// a short buffer is demodulated as a buffer of that length: refuse here, before anything is
		// queued, what the chain cannot take (e.g. a length the fifth_order passes do not divide)
		rtlfm_cfg c = h->cfg;
		c.block_len = len;
		c.max_blocks = 1;
		const int v = validate_cfg(&c);
		if (v < 0) return v;
	}
	int r = ingest_ensure(h);
	if (r < 0) return r;
	Ingest *in = h->ing;
	// shared: pushes of different streams run side by side; rtlfm_gpu_run() takes the lock
	// exclusively only to flip the halves, so it sees every buffer whole or not at all
	std::shared_lock<std::shared_mutex> g(in->mu);
	// a slot of this stream is out between acquire and commit: a push would land in that very slot
	if (in->open_slot[stream].load(std::memory_order_acquire)) return -EBUSY;
	const int f = in->fill;
	const int slot = in->pushed[f][stream].fetch_add(1, std::memory_order_acq_rel);
	if (slot >= h->cap_blocks) {
		in->pushed[f][stream].fetch_sub(1, std::memory_order_acq_rel);
		return -ENOSPC;
	}
	const size_t at = (size_t)stream * h->cap_blocks + slot;
	memcpy(in->inp.h_stage[f] + at * h->cfg.block_len, iq, len);
	in->h_len[f][at] = len;
	return 0;
}

// Zero-copy ingest: the producer fills the pinned ring slot itself.  The reference has this at the
// USB side (use_zerocopy, src/librtlsdr.c:2744-2810: the kernel's transfer buffers are mapped into
// the process and handed to the callback as they are); here the device layer - a file reader, an
// rtl_tcp receiver, anything that can write to a pointer - asks for the next slot of its stream,
// writes the samples there, and commits the length.  No memcpy between the producer and the H2D copy.
extern "C" int rtlfm_gpu_acquire(rtlfm_gpu *h, int stream, uint8_t **buf, uint32_t *cap)
{
	if (!h || !buf || stream < 0 || stream >= ring_rows(h)) return -EINVAL;
	if (h->chan_per > 0 && !h->opt.source_ring) return -ENOTSUP;
	int r = ingest_ensure(h);
	if (r < 0) return r;
	Ingest *in = h->ing;
	std::shared_lock<std::shared_mutex> g(in->mu);
	const int f = in->fill;
	if (in->open_slot[stream].load(std::memory_order_acquire)) return -EBUSY;  // one open slot per stream
	const int slot = in->pushed[f][stream].load(std::memory_order_acquire);
	if (slot >= h->cap_blocks) return -ENOSPC;
	in->open_slot[stream].store(1 + f, std::memory_order_release);
	*buf = in->inp.h_stage[f] + ((size_t)stream * h->cap_blocks + slot) * h->cfg.block_len;
	if (cap) *cap = h->cfg.block_len;
	return 0;
}

extern "C" int rtlfm_gpu_commit(rtlfm_gpu *h, int stream, uint32_t len)
{
	if (!h || stream < 0 || stream >= ring_rows(h)) return -EINVAL;
	if (h->chan_per > 0 && !h->opt.source_ring) return -ENOTSUP;
	Ingest *in = h->ing;
	if (!in || in->rows != ring_rows(h)) return -EINVAL;
	std::shared_lock<std::shared_mutex> g(in->mu);
	const int o = in->open_slot[stream].load(std::memory_order_acquire);
	if (!o) return -EINVAL;
	const int f = o - 1;  // rtlfm_gpu_run() does not flip the halves while a slot is open: f is still the filling half
	if (len == 0) {       // nothing arrived: give the slot back
		in->open_slot[stream].store(0, std::memory_order_release);
		return 0;
	}
	if (len > h->cfg.block_len || len % 512) return -EINVAL;
	if (len != h->cfg.block_len) {
		rtlfm_cfg c = h->cfg;
		c.block_len = len;
		c.max_blocks = 1;
		const int v = validate_cfg(&c);
		if (v < 0) return v;
	}
	const int slot = in->pushed[f][stream].load(std::memory_order_acquire);
	in->h_len[f][(size_t)stream * h->cap_blocks + slot] = len;
	in->pushed[f][stream].store(slot + 1, std::memory_order_release);
	in->open_slot[stream].store(0, std::memory_order_release);
	return 0;
}

// results of one buffer (tmp, tmp_len per stream) appended behind what the run has so far
__global__ void k_append_results(int16_t *dst, size_t dstride, int32_t *dst_len, const int16_t *src, size_t sstride,
                                 const int32_t *src_len, int s0, int ns, int cap)
{
	const int s = s0 + (int)blockIdx.x;
	if (s >= s0 + ns) return;
	const int n = src_len[s], at = dst_len[s];
	for (int k = threadIdx.x; k < n && at + k < cap; k += blockDim.x) dst[s * dstride + at + k] = src[s * sstride + k];
	__syncthreads();
	if (threadIdx.x == 0) dst_len[s] = at + n;
}

// A view of the handle on streams [s0, s0 + ns) with another buffer length: same device buffers,
// per-stream pointers shifted, everything on the handle's stream (no tail overlap, no timing).  The copy is all aliases
// (device_own.h): it owns nothing, frees nothing, and an allocation through it fails with -EINVAL.
static rtlfm_gpu make_view(rtlfm_gpu *h, int s0, int ns, uint32_t block_len)
{
	rtlfm_gpu v = *h;
	v.nstreams = ns;
	v.cfg.block_len = block_len;
	v.ing = nullptr;
	v.tail_overlap = false;
	v.timing = false;
	v.no_deemph_scan = true;
	v.opt.input_stats = 0;   // run_ragged takes the statistics itself, into the run's own rows
	v.opt.input_health = 0;  // ... and the health records
	v.mute_streams = 0;      // rtlfm_gpu_run_end has applied the mute to the whole run's input
	v.opt.verify_twice = 0;  // (the shadow rows are sized by the run: a view cannot grow them) ragged runs are not verified
	v.opt.bank_survey = 0;   // ... nor surveyed: a survey is one run's, a view runs one buffer (run_ragged says so on the handle)
	v.ev_pending.clear(); v.ev_free.clear();
	const size_t cb = (size_t)h->cap_blocks;
	for (int k = 0; k < 3; k++) v.st[k] = h->st[k].alias(s0);
	for (int k = 0; k < 2; k++) {
		v.d_cnt[k] = h->d_cnt[k].alias(s0);
		for (int j = 0; j < 2; j++) v.res[k][j] = h->res[k][j].alias((size_t)s0 * h->tstride);
	}
	v.d_cnt2 = h->d_cnt2.alias(s0);
	v.d_mute = h->d_mute.alias(s0 * cb);
	v.d_levels = h->d_levels.alias(s0 * cb);
	v.d_sums = h->d_sums.alias(s0 * cb * 2);
	v.d_sq_sums = h->d_sq_sums.alias(s0 * cb * 2);
	v.d_adc_sums = h->d_adc_sums.alias(s0 * cb);
	v.d_rdc_avg = h->d_rdc_avg.alias(s0 * cb);
	v.bufA = h->bufA.alias((size_t)s0 * h->xstride); v.bufB = h->bufB.alias((size_t)s0 * h->xstride);
	v.deepA = h->deepA.alias((size_t)s0 * h->deep_stride);
	v.deepB = h->deepB.alias((size_t)s0 * h->deep_stride);
	return v;
}

// what a view's run advanced that belongs to the handle (the view itself owned nothing)
static void view_done(rtlfm_gpu *h, const rtlfm_gpu &v)
{
	h->fws.stamp_seq = v.fws.stamp_seq;
	h->fws.stamp_last = v.fws.stamp_last;
	h->last_path = v.last_path;
	h->last_route = v.last_route;
	h->last_rest = v.last_rest;
}

// a run that holds short buffers: buffer by buffer, ranges of streams with equal length
static int run_ragged(rtlfm_gpu *h, Ingest *in, int f, int nb)
{
	const int S = h->nstreams;
	const size_t stride = (size_t)h->cap_blocks * h->cfg.block_len;
	int r;
	// A view cannot allocate (device_own.h: it holds aliases): everything any path may need exists before the first one is
	// made - the front ends' workspace too: the dummy tile, k_fused's pass-0 tap table for the handle's rotation where the
	// engine is the MFMA one, and, while waves leave clock stamps, room for the most waves a one-buffer launch can have.
	if ((r = ensure_work_buffers(h)) < 0 || (r = ensure_res_buffers(h)) < 0 || (r = ensure_deep_buffers(h)) < 0) return r;
	if ((r = fused::ensure_dummy_tile(h->fws)) < 0) return r;
	if (h->cfg.downsample_passes > 0 && fused::effective_engine(h->fws) == 1 &&  // (k_fused's: fifth_order passes only)
	    (r = fused::ensure_mfma_taps(h->fws, h->cfg.offset_tuning ? 0 : 1)) < 0)
		return r;
	if (h->fws.want_stamps || (h->fws.debug & 2)) {
		const size_t tiles = (h->cfg.block_len + fused::kTileBytes - 1) / fused::kTileBytes;  // (a segment is a tile at least)
		if ((r = h->fws.stamps.grow((size_t)S * tiles * 8, h->stream)) < 0) return r;
	}
	if (h->opt.input_stats && (r = ensure_input_stats(h)) < 0) return r;
	if (h->opt.input_health && (r = ensure_input_health(h)) < 0) return r;
	if (h->opt.squelch_gate && (r = ensure_gate(h)) < 0) return r;
	if (h->chan_per > 0 && (r = ensure_channel_buffers(h)) < 0) return r;
	if ((r = ensure_source_records(h)) < 0 || (r = ensure_source_iq(h)) < 0) return r;
	OWN_TRY(in->d_tmp.alloc((size_t)S * in->ostride));
	OWN_TRY(in->d_tmp_len.alloc((size_t)S));
	// The views run their audio tail on the handle's main stream: the tails of the two previous
	// (batched) steps may still be running on the tail stream, writing the state copy and the res[]
	// sets the views are about to read.  Order the main stream behind both, on the handle itself.
	for (int p = 0; p < 2; p++)
		if (h->tail_pending[p]) {
			HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_tail[p], 0));
			h->tail_pending[p] = false;
		}
	HIP_TRY(hipMemsetAsync(in->d_result_len[f], 0, (size_t)S * sizeof(int32_t), h->stream));
	for (int j = 0; j < nb; j++) {
		// every range of this buffer reads st[cur] and writes the next copy; the rotation advances once
		const int cur = h->st_cur;
		const unsigned step = h->step;
		if (h->chan_per > 0) {
			// Channels (option source_ring): rtlfm_gpu_run_begin has found buffer j of one length on every source, so ONE view of
			// the whole handle runs it.  The view is a copy: what a channel run advances on it - pos, the history's current
			// copy - goes back to the handle here, once per buffer; the rotation advances below as for every ragged run.
			const uint32_t len = in->h_len[f][j];
			rtlfm_cfg c = h->cfg;
			c.block_len = len;
			c.max_blocks = 1;
			if ((r = validate_cfg(&c)) < 0) return r;
			rtlfm_gpu v = make_view(h, 0, S, len);
			v.st_cur = cur;
			v.step = step;
			v.src_rec_off = (size_t)j;  // options source_stats / source_health: each buffer's record over its own length, [source][nb]
			v.src_rec_stride = nb;
			r = run_device_impl(&v, in->inp.d_in[f] + (size_t)j * h->cfg.block_len, stride, 1, in->d_tmp, in->ostride, in->d_tmp_len);
			view_done(h, v);
			if (r < 0) return r;
			h->chan_pos = v.chan_pos;
			h->src_hist_cur = v.src_hist_cur;
		}
		for (int s0 = 0; s0 < S && h->chan_per == 0;) {
			const uint32_t len = in->h_len[f][(size_t)s0 * h->cap_blocks + j];
			int s1 = s0 + 1;
			while (s1 < S && in->h_len[f][(size_t)s1 * h->cap_blocks + j] == len) s1++;
			rtlfm_cfg c = h->cfg;
			c.block_len = len;
			c.max_blocks = 1;
			if ((r = validate_cfg(&c)) < 0) return r;
			// each buffer's statistics over its own length, filed as [stream][nb] like a batched run's
			if ((r = launch_input_readers(h, in->inp.d_in[f] + (size_t)s0 * stride + (size_t)j * h->cfg.block_len, stride, len, 1, s1 - s0,
			                              (size_t)s0 * nb + j, nb)) < 0)
				return r;
			rtlfm_gpu v = make_view(h, s0, s1 - s0, len);
			v.st_cur = cur;
			v.step = step;
			v.gate_rec_off = (size_t)s0 * nb + j;  // the gate's records filed as [stream][nb] like a batched run's
			v.gate_rec_stride = nb;
			r = run_device_impl(&v, in->inp.d_in[f] + (size_t)s0 * stride + (size_t)j * h->cfg.block_len, stride, 1,
			                         in->d_tmp + (size_t)s0 * in->ostride, in->ostride, in->d_tmp_len + s0);
			view_done(h, v);
			if (r < 0) return r;
			s0 = s1;
		}
		h->st_cur = (cur + 1) % 3;
		h->step = step + 1;
		k_append_results<<<S, 256, 0, h->stream>>>(in->d_result[f], in->ostride, in->d_result_len[f], in->d_tmp, in->ostride,
		                                          in->d_tmp_len, 0, S, (int)in->ostride);
	}
	h->stats_nblocks = h->opt.input_stats ? nb : 0;
	h->health_nblocks = h->opt.input_health ? nb : 0;
	h->gate_nblocks = h->opt.squelch_gate ? nb : 0;
	h->src_stats_nblocks = h->chan_per > 0 && h->opt.source_stats ? nb : 0;
	h->src_health_nblocks = h->chan_per > 0 && h->opt.source_health ? nb : 0;
	h->siq_nblocks = h->chan_per > 0 && h->opt.source_iq ? nb : 0;
	survey_advance(h, -1);  // (a run of short buffers carries no survey: rtlfm_gpu_bank_survey says -ENODATA)
	HIP_TRY(hipGetLastError());
	return 0;
}

// The hop mute (rtlfm_gpu_mute) on the run's device input, behind its transfer and in front of everything that reads it:
// of every stream with a count pending the first bytes of its buffers, in order, each buffer over its own length, until
// the count is used up or the run ends (what is left waits for the next run).  One launch.
static int apply_mute(rtlfm_gpu *h, Ingest *in, int f, int nb)
{
	const size_t L = h->cfg.block_len;
	std::vector<scan::MuteEntry> ent;
	uint32_t mx = 0;
	for (int s = 0; s < h->nstreams; s++) {
		uint32_t left = h->mute_left[s];
		if (!left) continue;
		for (int j = 0; j < nb && left; j++) {
			const size_t at = (size_t)s * h->cap_blocks + j;
			const uint32_t len = in->h_len[f][at];
			const uint32_t m = left < len ? left : len;
			ent.push_back({(unsigned long long)(at * L), m, 0});
			if (m > mx) mx = m;
			left -= m;
		}
		h->mute_left[s] = left;
		if (!left) h->mute_streams--;
	}
	if (ent.empty()) return 0;
	OWN_TRY(h->d_mute_entries.grow((size_t)h->nstreams * h->cap_blocks, h->stream));  // (the most a run can have)
	// (a blocking copy: the entries are on the device before the launch is queued, and an earlier run's launch that read
	// the same array has been waited for by it)
	HIP_TRY(hipStreamSynchronize(h->stream));
	HIP_TRY(hipMemcpy(h->d_mute_entries, ent.data(), ent.size() * sizeof(scan::MuteEntry), hipMemcpyHostToDevice));
	std::pair<Event, Event> ev;
	int r = timing_begin(h, ev);
	if (r < 0) return r;
	if ((r = scan::launch_mute(in->inp.d_in[f], h->d_mute_entries, (int)ent.size(), mx, h->stream)) < 0) return r;
	return timing_end(h, ev);
}

// Option pack_results: the two launches of pack_kernel.h behind a ring run that has just been queued (the rotation has
// moved on: the state copy the run STARTED from is two copies on, and stays as it is until the run after next writes it -
// queued behind this).  On the handle's stream, behind the run's audio tail where that went to its own stream, as
// launch_gate waits for it; under verify_twice behind the comparison, once.  Reads the half's rows and lengths, the run's
// levels and that state copy; writes the half's packed buffer, index and total, and d_piece_off.
static int ring_pack(rtlfm_gpu *h, Ingest *in, int f, int nb)
{
	const rtlfm_cfg &c = h->cfg;
	const size_t S = (size_t)h->nstreams;
	const int mode = h->opt.pack_results;
	if (mode == 2 && gate_supported(c) < 0) return -ENOTSUP;
	for (int k = 0; k < 2; k++) {
		OWN_TRY(in->pk.d_packed[k].alloc(S * in->ostride));  // (ostride is a multiple of 64)
		OWN_TRY(in->pk.d_pack_index[k].alloc(S));
		OWN_TRY(in->pk.d_pack_total[k].alloc(1));
	}
	if (mode == 2) OWN_TRY(in->pk.d_piece_off.alloc(S * h->cap_blocks));
	const int par = (int)((h->step - 1) & 1);
	if (h->tail_pending[par]) HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_tail[par], 0));
	pack::PlanParams pp{};
	pp.mode = mode; pp.S = (int)S;
	pp.lens = in->d_result_len[f];
	pp.levels = h->d_levels;
	pp.sin = h->st[(h->st_cur + 2) % 3];
	pp.piece_off = in->pk.d_piece_off;
	pp.nblocks = nb;
	pp.N = c.downsample_passes > 0 ? (int)((c.block_len / 2) >> c.downsample_passes) : (int)(c.block_len / 2);  // (as launch_gate)
	pp.D = c.downsample_passes > 0 ? 1 : c.downsample;
	pp.mul = c.mode == RTLFM_MODE_RAW ? 2 : 1;
	pp.level = c.squelch_level; pp.conseq = h->opt.conseq_squelch;
	pp.index = in->pk.d_pack_index[f]; pp.total = in->pk.d_pack_total[f];
	pack::CopyParams cp{};
	cp.mode = mode;
	cp.R = in->d_result[f]; cp.rstride = in->ostride;
	cp.packed = in->pk.d_packed[f]; cp.cap = in->pk.d_packed[f].capacity();
	cp.index = pp.index; cp.sin = pp.sin; cp.piece_off = pp.piece_off;
	cp.nblocks = nb; cp.N = pp.N; cp.D = pp.D; cp.mul = pp.mul;
	const size_t most = mode == 2 ? (size_t)pp.mul * (pp.N / pp.D + 1) : in->ostride;
	in->pk.pack_timed[f] = h->timing;
	if (h->timing) {
		for (Event &e : in->pk.ev_pack[f]) OWN_TRY(e.create());
		HIP_TRY(hipEventRecord(in->pk.ev_pack[f][0], h->stream));
	}
	const int r = pack::launch_pack(pp, cp, most, h->stream);
	if (r < 0) return r;
	if (h->timing) HIP_TRY(hipEventRecord(in->pk.ev_pack[f][1], h->stream));
	in->pk.pack_mode[f] = mode;
	return 0;
}

// rtlfm_gpu_run() in two steps, for a caller that gates its producers around the flip only (host/rtl_fm_hip.cpp): _begin
// takes what the ring's filling half holds - every stream the same number of buffers, no slot open - and flips the
// halves, which is all that must exclude the producers; _end queues the H2D copy and the kernels.  Between the two the
// producers already fill the other half.  *taken (may be NULL) = buffers per stream the run took.
extern "C" int rtlfm_gpu_run_begin(rtlfm_gpu *h, int *taken)
{
	if (!h) return -EINVAL;
	if (h->chan_per > 0 && !h->opt.source_ring) return -ENOTSUP;  // (so rtlfm_gpu_run: it begins here)
	int r = ingest_ensure(h);
	if (r < 0) return r;
	Ingest *in = h->ing;
	if (in->pending_f >= 0) return -EBUSY;  // a begun run has not been ended
	HIP_TRY(hipSetDevice(h->device));
	const int S = in->rows;  // (option source_ring with channels: the sources)
	const uint32_t L = h->cfg.block_len;
	int f, nb;
	bool ragged = false;
	{
		// the half the callbacks will fill next must have left for the GPU (its H2D done); waited
		// for before the lock, so that callbacks are never held up by a transfer
		const int other_guess = in->fill ^ 1;
		if (in->h2d_pending[other_guess]) {
			HIP_TRY(hipEventSynchronize(in->ev_h2d[other_guess]));
			in->h2d_pending[other_guess] = false;
		}
		std::unique_lock<std::shared_mutex> g(in->mu);
		f = in->fill;
		nb = in->pushed[f][0].load();
		for (int s = 1; s < S; s++)
			if (in->pushed[f][s].load() != nb) return -EAGAIN;
		if (nb == 0) return -EAGAIN;
		for (int s = 0; s < S; s++)
			if (in->open_slot[s].load(std::memory_order_acquire)) return -EAGAIN;  // a producer is still writing its slot
		for (int s = 0; s < S && !ragged; s++)
			for (int j = 0; j < nb; j++)
				if (in->h_len[f][(size_t)s * h->cap_blocks + j] != L) { ragged = true; break; }
		// channels: pos is ONE counter per handle, so buffer j must have one length on every source.  Nothing is taken; the
		// caller empties the ring (rtlfm_gpu_reset).
		if (ragged && h->chan_per > 0)
			for (int s = 1; s < S; s++)
				for (int j = 0; j < nb; j++)
					if (in->h_len[f][(size_t)s * h->cap_blocks + j] != in->h_len[f][j]) return -ERANGE;
		// pack_results 2 knows a buffer's extent from the handle's buffer length: a ragged run is not taken either
		if (ragged && h->opt.pack_results == 2) return -ENOTSUP;
		for (int s = 0; s < S; s++) in->pushed[f ^ 1][s].store(0);
		in->fill = f ^ 1;
	}
	in->pending_f = f; in->pending_nb = nb; in->pending_ragged = ragged;
	if (taken) *taken = nb;
	return 0;
}

extern "C" int rtlfm_gpu_run_end(rtlfm_gpu *h)
{
	if (!h || !h->ing) return -EINVAL;
	Ingest *in = h->ing;
	if (in->pending_f < 0) return -EINVAL;  // nothing begun
	HIP_TRY(hipSetDevice(h->device));
	const int S = in->rows;  // input rows: the run's results are per stream (run_device_impl, run_ragged)
	const uint32_t L = h->cfg.block_len;
	const size_t stride = (size_t)h->cap_blocks * L;
	const int f = in->pending_f, nb = in->pending_nb;
	const bool ragged = in->pending_ragged;
	in->pending_f = -1;  // whatever happens below, the buffers of this run are gone from the ring
	int r;
	// d_in[f] is free once the kernels of the run that read it are done
	if (in->run_pending[f]) {
		HIP_TRY(hipStreamWaitEvent(in->copy_stream, in->ev_run[f], 0));
		in->run_pending[f] = false;
	}
	if (nb == h->cap_blocks)
		HIP_TRY(hipMemcpyAsync(in->inp.d_in[f], in->inp.h_stage[f], stride * S, hipMemcpyHostToDevice, in->copy_stream));
	else
		HIP_TRY(hipMemcpy2DAsync(in->inp.d_in[f], stride, in->inp.h_stage[f], stride, (size_t)nb * L, S, hipMemcpyHostToDevice,
		                         in->copy_stream));
	HIP_TRY(hipEventRecord(in->ev_h2d[f], in->copy_stream));
	in->h2d_pending[f] = true;
	HIP_TRY(hipStreamWaitEvent(h->stream, in->ev_h2d[f], 0));
	if (h->mute_streams > 0 && (r = apply_mute(h, in, f, nb)) < 0) return r;
	if (ragged) r = run_ragged(h, in, f, nb);
	else r = run_device_impl(h, in->inp.d_in[f], stride, nb, in->d_result[f], in->ostride, in->d_result_len[f]);
	if (r < 0) return r;
	in->pk.pack_mode[f] = 0;
	if (h->opt.pack_results && (r = ring_pack(h, in, f, nb)) < 0) return r;
	HIP_TRY(hipEventRecord(in->ev_run[f], h->stream));
	in->run_pending[f] = true;
	in->tail_par[f] = (int)((h->step - 1) & 1);
	in->tail_any[f] = !ragged && h->tail_pending[in->tail_par[f]];
	in->prev = in->last;
	in->last = f;
	in->mirror_valid = false;
	return 0;
}

extern "C" int rtlfm_gpu_run(rtlfm_gpu *h)
{
	int r = rtlfm_gpu_run_begin(h, nullptr);
	if (r < 0) return r;
	return rtlfm_gpu_run_end(h);
}

// Results of the run BEFORE the last one (they stay valid until the second run after theirs).  Waits for
// that run only - its front end's event and, if it left one, its audio tail's - not for the run that has
// been started since: a server that calls run(k + 1) as soon as the buffers of k + 1 are in and only then
// collects run k keeps the H2D copies of consecutive runs back to back on the link (host/ingest_bench.cpp
// --depth 2), where run / fetch / run leaves it idle for a kernel and a D2H copy per run.
extern "C" int rtlfm_gpu_fetch_all_prev(rtlfm_gpu *h, int16_t *out, size_t out_stride, int32_t *lens)
{
	if (!h || !out || !lens) return -EINVAL;
	Ingest *in = h->ing;
	if (!in || in->prev < 0 || in->prev == in->last) return -EAGAIN;
	HIP_TRY(hipSetDevice(h->device));
	const int f = in->prev;
	HIP_TRY(hipEventSynchronize(in->ev_run[f]));
	if (in->tail_any[f]) HIP_TRY(hipEventSynchronize(h->ev_tail[in->tail_par[f]]));
	const int S = h->nstreams;
	HIP_TRY(hipMemcpy(lens, in->d_result_len[f], (size_t)S * sizeof(int32_t), hipMemcpyDeviceToHost));
	int mx = 0;
	for (int s = 0; s < S; s++) mx = lens[s] > mx ? lens[s] : mx;
	if ((size_t)mx > out_stride) return -ENOBUFS;
	if (mx > 0)
		HIP_TRY(hipMemcpy2D(out, out_stride * sizeof(int16_t), in->d_result[f], in->ostride * sizeof(int16_t),
		                    (size_t)mx * sizeof(int16_t), S, hipMemcpyDeviceToHost));
	return 0;
}

extern "C" int rtlfm_gpu_fetch_all(rtlfm_gpu *h, int16_t *out, size_t out_stride, int32_t *lens)
{
	if (!h || !out || !lens) return -EINVAL;
	Ingest *in = h->ing;
	if (!in || in->last < 0) return -EAGAIN;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(sync_all(h));
	const int f = in->last;
	const int S = h->nstreams;
	HIP_TRY(hipMemcpy(lens, in->d_result_len[f], (size_t)S * sizeof(int32_t), hipMemcpyDeviceToHost));
	int mx = 0;
	for (int s = 0; s < S; s++) mx = lens[s] > mx ? lens[s] : mx;
	if ((size_t)mx > out_stride) return -ENOBUFS;
	if (mx > 0)
		HIP_TRY(hipMemcpy2D(out, out_stride * sizeof(int16_t), in->d_result[f], in->ostride * sizeof(int16_t),
		                    (size_t)mx * sizeof(int16_t), S, hipMemcpyDeviceToHost));
	return 0;
}

// The packed form of the last run (prev: of the run before it), waited for as rtlfm_gpu_fetch_all (_prev) waits: the
// index, then the rows in one transfer.  The total is the end of the last row.
static int fetch_packed(rtlfm_gpu *h, bool prev, int16_t *out, size_t cap, rtlfm_packed_row *rows, size_t *total)
{
	if (!h || !rows || !total || (!out && cap)) return -EINVAL;
	Ingest *in = h->ing;
	if (!in || (prev ? in->prev < 0 || in->prev == in->last : in->last < 0)) return -EAGAIN;
	const int f = prev ? in->prev : in->last;
	if (!in->pk.pack_mode[f] || !in->pk.d_packed[f]) return -ENODATA;
	HIP_TRY(hipSetDevice(h->device));
	if (prev) {
		HIP_TRY(hipEventSynchronize(in->ev_run[f]));  // (recorded behind the pack, which waited for the run's tail)
	} else {
		HIP_TRY(sync_all(h));
	}
	const size_t S = (size_t)h->nstreams;
	HIP_TRY(hipMemcpy(rows, in->pk.d_pack_index[f], S * sizeof(rtlfm_packed_row), hipMemcpyDeviceToHost));
	const size_t need = (size_t)rows[S - 1].offset + (((size_t)rows[S - 1].len + 7) & ~(size_t)7);
	*total = need;
	if (need > cap) return -ENOBUFS;
	if (need > 0) HIP_TRY(hipMemcpy(out, in->pk.d_packed[f], need * sizeof(int16_t), hipMemcpyDeviceToHost));
	return 0;
}

extern "C" int rtlfm_gpu_fetch_packed(rtlfm_gpu *h, int16_t *out, size_t cap, rtlfm_packed_row *rows, size_t *total)
{
	return fetch_packed(h, false, out, cap, rows, total);
}

extern "C" int rtlfm_gpu_fetch_packed_prev(rtlfm_gpu *h, int16_t *out, size_t cap, rtlfm_packed_row *rows, size_t *total)
{
	return fetch_packed(h, true, out, cap, rows, total);
}

extern "C" int rtlfm_gpu_pack_device(int device, const int16_t *d_rows, size_t stride, const int32_t *d_lens, int nstreams,
                                     int16_t *d_packed, size_t cap, rtlfm_packed_row *d_index, uint64_t *d_total, void *hip_stream)
{
	if (!d_rows || !d_lens || !d_packed || !d_index || !d_total || nstreams < 1) return -EINVAL;
	if (((uintptr_t)d_rows & 1) || ((uintptr_t)d_packed & 15) || ((uintptr_t)d_index & 7) || ((uintptr_t)d_total & 7)) return -EINVAL;
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return -ENODEV;
	HIP_TRY(hipSetDevice(device));
	pack::PlanParams pp{};
	pp.mode = 1; pp.S = nstreams; pp.lens = d_lens;
	pp.index = d_index; pp.total = reinterpret_cast<unsigned long long *>(d_total);
	pack::CopyParams cp{};
	cp.mode = 1; cp.R = d_rows; cp.rstride = stride; cp.packed = d_packed; cp.cap = cap; cp.index = d_index;
	return pack::launch_pack(pp, cp, stride, (hipStream_t)hip_stream);
}

extern "C" int rtlfm_gpu_fetch(rtlfm_gpu *h, int stream, int16_t *out, int cap, int *n)
{
	if (!h || !out || !n || stream < 0 || stream >= h->nstreams) return -EINVAL;
	Ingest *in = h->ing;
	if (!in || in->last < 0) return -EAGAIN;
	HIP_TRY(hipSetDevice(h->device));
	if (!in->mirror_valid) {
		// one transfer for all streams, then every per-stream fetch is a host copy
		OWN_TRY(in->h_result.alloc((size_t)h->nstreams * in->ostride));
		OWN_TRY(in->h_result_len.alloc((size_t)h->nstreams));
		int r = rtlfm_gpu_fetch_all(h, in->h_result, in->ostride, in->h_result_len);
		if (r < 0) return r;
		in->mirror_valid = true;
	}
	const int32_t len = in->h_result_len[stream];
	*n = len;
	if (len > cap) return -ENOBUFS;
	if (len > 0) memcpy(out, in->h_result + (size_t)stream * in->ostride, (size_t)len * sizeof(int16_t));
	return 0;
}

extern "C" long rtlfm_debug_live(int kind)
{
	return kind >= 0 && kind <= 2 ? rtl_own::live(kind).load() : -EINVAL;
}

__global__ void k_selftest_atan2(const int32_t *yx, int n, int32_t *a, int32_t *b)
{
	RTLFM_GRID_STRIDE(i, n) {
		int y = yx[2 * i], x = yx[2 * i + 1];
		if (a) a[i] = atan2_q14(y, x, AtanNodesConst());
		if (b) b[i] = atan2_q14_libm(y, x);
	}
}
__global__ void k_selftest_fast_atan2(const int32_t *yx, int n, int32_t *a)
{
	RTLFM_GRID_STRIDE(i, n) a[i] = fast_atan2_q14(yx[2 * i], yx[2 * i + 1]);
}

__global__ void k_selftest_const_div(const int32_t *nd, int n, int32_t *q)
{
	RTLFM_GRID_STRIDE(i, n) {
		const ConstDiv cd(nd[2 * i + 1]);
		q[i] = cd(nd[2 * i]);
	}
}

extern "C" int rtlfm_gpu_selftest_const_div(int device, const int32_t *nd, int n, int32_t *q)
{
	if (!nd || !q || n < 1) return -EINVAL;
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return -ENODEV;
	HIP_TRY(hipSetDevice(device));
	DevBuf<int32_t> d_in, d_q;
	OWN_TRY(d_in.alloc((size_t)n * 2));
	OWN_TRY(d_q.alloc((size_t)n));
	HIP_TRY(hipMemcpy(d_in, nd, (size_t)n * 8, hipMemcpyHostToDevice));
	k_selftest_const_div<<<grid_for((size_t)n), 256>>>(d_in, n, d_q);
	HIP_TRY(hipDeviceSynchronize());
	HIP_TRY(hipMemcpy(q, d_q, (size_t)n * 4, hipMemcpyDeviceToHost));
	return 0;
}

extern "C" int rtlfm_gpu_selftest_fast_atan2(int device, const int32_t *yx, int n, int32_t *q14)
{
	if (!yx || !q14 || n < 1) return -EINVAL;
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return -ENODEV;
	HIP_TRY(hipSetDevice(device));
	DevBuf<int32_t> d_in, d_a;
	OWN_TRY(d_in.alloc((size_t)n * 2));
	OWN_TRY(d_a.alloc((size_t)n));
	HIP_TRY(hipMemcpy(d_in, yx, (size_t)n * 8, hipMemcpyHostToDevice));
	k_selftest_fast_atan2<<<grid_for((size_t)n), 256>>>(d_in, n, d_a);
	HIP_TRY(hipDeviceSynchronize());
	HIP_TRY(hipMemcpy(q14, d_a, (size_t)n * 4, hipMemcpyDeviceToHost));
	return 0;
}

extern "C" int rtlfm_gpu_selftest_atan2(int device, const int32_t *yx, int n, int32_t *q14, int32_t *q14_libm)
{
	if (!yx || n < 1) return -EINVAL;
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return -ENODEV;
	HIP_TRY(hipSetDevice(device));
	DevBuf<int32_t> d_in, d_a, d_b;
	OWN_TRY(d_in.alloc((size_t)n * 2));
	OWN_TRY(d_a.alloc((size_t)n));
	OWN_TRY(d_b.alloc((size_t)n));
	HIP_TRY(hipMemcpy(d_in, yx, (size_t)n * 8, hipMemcpyHostToDevice));
	k_selftest_atan2<<<grid_for((size_t)n), 256>>>(d_in, n, q14 ? d_a.get() : nullptr, q14_libm ? d_b.get() : nullptr);
	HIP_TRY(hipDeviceSynchronize());
	if (q14) HIP_TRY(hipMemcpy(q14, d_a, (size_t)n * 4, hipMemcpyDeviceToHost));
	if (q14_libm) HIP_TRY(hipMemcpy(q14_libm, d_b, (size_t)n * 4, hipMemcpyDeviceToHost));
	return 0;
}

// rotate_90 (u8): per 8 bytes [a0 b0 a1 b1 a2 b2 a3 b3] -> [a0 b0 ~b1 a1 ~a2 ~b2 b3 ~a3]
// (~x = 255 - x).  Pure byte shuffling: one v_perm and one v_xor per dword, 16 bytes per lane.
__global__ void __launch_bounds__(256) k_rotate_90_u8(uint4 *buf, size_t n16)
{
	RTLFM_GRID_STRIDE(i, n16) {
		uint4 v = buf[i];
		v.x = __builtin_amdgcn_perm(0, v.x, 0x02030100u) ^ 0x00ff0000u;
		v.y = __builtin_amdgcn_perm(0, v.y, 0x02030100u) ^ 0xff00ffffu;
		v.z = __builtin_amdgcn_perm(0, v.z, 0x02030100u) ^ 0x00ff0000u;
		v.w = __builtin_amdgcn_perm(0, v.w, 0x02030100u) ^ 0xff00ffffu;
		buf[i] = v;
	}
}

__global__ void k_rotate_90_u8_tail(uint2 *p)  // an odd group of eight bytes at the end
{
	uint2 v = *p;
	v.x = __builtin_amdgcn_perm(0, v.x, 0x02030100u) ^ 0x00ff0000u;
	v.y = __builtin_amdgcn_perm(0, v.y, 0x02030100u) ^ 0xff00ffffu;
	*p = v;
}

extern "C" int rtlfm_gpu_rotate_90_u8(int device, void *d_buf, size_t len, void *hip_stream)
{
	if (!d_buf || (len & 7) || ((uintptr_t)d_buf & 15)) return -EINVAL;
	if (len == 0) return 0;
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return -ENODEV;
	HIP_TRY(hipSetDevice(device));
	hipStream_t q = (hipStream_t)hip_stream;
	const size_t n16 = len / 16;
	if (n16) k_rotate_90_u8<<<grid_for(n16), 256, 0, q>>>((uint4 *)d_buf, n16);
	if (len & 8) k_rotate_90_u8_tail<<<1, 1, 0, q>>>((uint2 *)((uint8_t *)d_buf + len - 8));
	HIP_TRY(hipGetLastError());
	return 0;
}

extern "C" int rtlfm_gpu_clock_stamps(rtlfm_gpu *h, uint64_t *out, int cap_waves, int *waves)
{
	if (!h || !waves) return -EINVAL;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(sync_all(h));
	if (!h->fws.stamps || h->fws.stamp_last <= 0) return -ENODATA;
	*waves = h->fws.stamp_last;
	if (!out) return 0;
	if (cap_waves < h->fws.stamp_last) return -ENOBUFS;
	// fused_debug bit 64: the launch BEFORE the last one (the two alternate between the halves of the buffer), so that
	// a tool can see the gap between two launches that followed each other (tools/launch_gap.py)
	HIP_TRY(hipMemcpy(out, h->fws.stamp_half((h->fws.debug & 64) ? 1 : 0), (size_t)h->fws.stamp_last * 32, hipMemcpyDeviceToHost));
	return 0;
}

// How a front-end launch would be cut into waves (fused::plan_segments), without a GPU: for the planner's unit test.
// starts[0 .. *segs] = tile boundaries of a stream's segments (cap entries at least *segs + 1, else -ENOBUFS).
extern "C" int rtlfm_plan_segments(int nstreams, int total_tiles, int fifth_order, int tail_follows, int target_waves, int min_tiles,
                                   int tiles_per_seg, int gss_x10, int *segs, int *starts, int cap)
{
	if (nstreams < 1 || total_tiles < 1 || !segs || !starts) return -EINVAL;
	fused::Workspace ws;
	ws.tail_follows = tail_follows != 0;
	if (target_waves > 0) { ws.target_waves = target_waves; ws.target_waves_tail = target_waves; ws.target_waves_tail_fifth = 0; ws.plan_by_caller = true; }
	if (min_tiles > 0) { ws.min_tiles = min_tiles; ws.plan_by_caller = true; }
	ws.tiles_per_seg = tiles_per_seg;
	ws.gss_x10 = gss_x10;
	const fused::SegPlan sp = fused::plan_segments(ws, nstreams, total_tiles, fifth_order != 0);
	*segs = sp.segs;
	if (cap < sp.segs + 1) return -ENOBUFS;
	for (int j = 0; j <= sp.segs; j++) {
		int at = sp.nlist > 0 ? sp.start[j] : j * sp.tiles_per_seg;
		starts[j] = at < total_tiles ? at : total_tiles;
	}
	return 0;
}

extern "C" const char *rtlfm_gpu_strerror(int err)
{
	switch (err) {
	case 0: return "ok";
	case -EINVAL: return "invalid argument, option value or configuration";
	case -ENODEV: return "no usable HIP device (there is no CPU fallback)";
	case -ENOMEM: return "out of device memory";
	case -ENOSPC: return "max_blocks already queued for this stream";
	case -EAGAIN: return "streams have unequal / zero queued blocks, or a producer still holds an acquired slot";
	case -EBUSY: return "the stream's previous slot is still open (rtlfm_gpu_acquire without rtlfm_gpu_commit), or rtlfm_gpu_run_device while "
	                    "a rtlfm_gpu_mute count is pending (it never writes its input), or rtlfm_gpu_state_move while a handle has a run "
	                    "begun and not ended or a ring slot open, or the options source_ring / pack_results set in such a moment; "
	                    "rtlfm_gpu_channels_move / _channels_history_set / _channels_load in such a moment, or (option source_ring) with buffers queued";
	case -EXDEV: return "rtlfm_gpu_state_move: the handles are on different devices (use rtlfm_gpu_state_get_all / _set_all); rtlfm_gpu_channels_move: "
	                    "the same (with them rtlfm_gpu_channels_history_get / _set and rtlfm_gpu_channels_tell / _seek)";
	case -ERANGE: return "the snapshot holds another number of streams than the handle";  // (rtlfm_gpu_load and rtlfm_gpu_channels_load)
	case -EMEDIUMTYPE: return "the snapshot was saved under another configuration (a rtlfm_cfg field other than max_blocks / report_levels differs); "
	                          "rtlfm_gpu_channels_load / _channels_move: the two sides do not carry the same things (that, or per_source, the option "
	                          "source_dc, the channel filter or the channel bank differs)";
	case -EILSEQ: return "the snapshot file is damaged or no snapshot (magic, version, sizes, length or checksum); a file of the other kind: "
	                     "RTLFMSNP files belong to rtlfm_gpu_load, RTLFMCHN files to rtlfm_gpu_channels_load";
	case -ENOTSUP: return "configuration not supported on this path; squelch_gate and pack_results 2: not behind a resampler "
	                      "(rate_out2 > 0), post_downsample > 1 or a buffer the fifth_order passes do not divide; pack_results 2: "
	                      "not on a run that holds a short buffer; rtlfm_gpu_save / _load / _state_move with channels on (use rtlfm_gpu_channels_save / _load / "
	                      "_move) and rtlfm_gpu_channels_* with channels off (use rtlfm_gpu_save / rtlfm_gpu_load / rtlfm_gpu_state_move)";
	case -EDOM: return "outside the reference's own domain: a boxcar longer than the buffer (fm_demod reads lowpassed[-2]), low_pass_simple on a "
	                   "count its step does not divide (src/rtl_fm.c:740), or rate_out2 > rate_out with low_pass_real (division by zero, :769)";
	case -E2BIG: return "more blocks than cfg.max_blocks; a configuration whose max_blocks buffers exceed 2^31 - 1 complex samples per stream";
	case -ENOBUFS: return "output buffer too small";
	case -EIO: return "HIP runtime error";
	case -ENODATA: return "no clock stamps recorded (rtlfm_gpu_clock_probe, fused fifth_order path only); no records of this kind "
	                      "(the option was off); rtlfm_gpu_fetch_packed: that run was not packed (option pack_results was 0); "
	                      "rtlfm_gpu_bank_survey: that run carried no survey (option bank_survey off, no bank, or no run yet); "
	                      "rtlfm_gpu_channels_history_get: neither a channel filter nor a bank is set, so no history is carried";
	default: return strerror(-err);
	}
}

extern "C" int rtlfm_gpu_version(void) { return (0 << 16) | (1 << 8) | 0; }
