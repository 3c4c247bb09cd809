// rtl_fm_hip — an rtl_fm-shaped command line over the C ABI.
//
// Keeps the reference tool's structure (src/rtl_fm.c): getopt with the same
// option letters (:1721-1880), the `-M wbfm` preset (:1831-1840), rate planning
// through optimal_settings (:1407-1445) and deemph_a (:1929-1934), a dongle
// thread that sits in rtlsdr_read_async() and hands each buffer over from the
// callback (:1346-1351, :1274-1344), a demod thread (:1353-1391) and an output
// thread that fwrite()s int16 PCM (:1393-1405) — but the callback body and
// full_demod() are rtlfm_gpu_push() / rtlfm_gpu_run() / rtlfm_gpu_fetch().
// The device is whatever exports the rtlsdr_* API; here librtlsdr_file.so
// (RTLSDR_FILE=<raw u8 IQ file>).  Unlike the reference's condvar hand-off
// (:1339-1343) nothing is ever dropped: the callback waits while the queue is
// full, so the output is a deterministic function of the input file.
//
// -N n (not a reference option) demodulates devices d .. d+n-1 as streams 0 .. n-1 of ONE handle, one run
// per step for all of them (see run_multi below): one dongle thread per device, as the reference has for its
// one dongle, each filling a host queue of its own; the demod thread takes the same number of buffers from
// every queue, so the library's equal-count rule holds, and the slowest source sets the pace.  A source that
// ends leaves the batch and the others go on, their carried state moved to a handle with fewer streams.
// With RTLSDR_FILE_LIST=<list of sources> the device layer has one device per line.
//
// -C file (the reference's command file, src/rtl_fm.c:527-736, README.rtlfm_cmdfile) is restated for -N n sources
// WITHOUT the hop: measurement line i of the file is watched permanently by source i (include/rtlfm_monitor.h).  As
// in the reference -C sets -M raw and takes each source's frequency and gain from its line; it switches report_levels
// and the library's option input_stats on, the demod thread feeds the monitor after every run, -v prints each event
// in the reference's wording (:716-718, :731-733, behind "stream i: "), a fired event with a command starts it in
// the background (posix_spawnp, no shell; !freq! !gain! !mlevel! !crit! !reflevel! !reftol! replaced as at :722-727;
// the children are waited for at exit), and the statistics per line are printed at exit (:2033-2040).  Every buffer
// of every source is still written (the reference's demod thread drops the buffer a cycle ends on, :1375-1380) and
// the lines are not limited to FREQUENCIES_LIMIT.
//
// -O string (the reference's driver options, src/librtlsdr.c:3114-3200) goes to rtlsdr_set_opt_string() whole, as in the
// reference; its parts agc=0|1|2 are also read here (anything else after agc= is refused before a device is opened).
// agc=2 is the reference's SOFTWARE AGC (gain mode 2, softagc(), src/librtlsdr.c:3288-3327), run here for every source
// at once: the library's option input_health is switched on, the records of every run's raw bytes (taken on the GPU)
// are fed to the engine of include/rtlfm_agc.h with each buffer's own length, and after every run each source's last
// index is applied to its device (rtlamd_file_set_gain_index).  settle = the buffers one run may take: they were
// captured before a change could act.  -v prints every change and every flip of rtl_tcp's overload verdict
// (detect_overload(), src/rtl_tcp.c:235-244); the final indices are printed at exit.
//
// -S file (not a reference letter) is the reference's scanning ("use multiple -f for scanning (requires squelch)",
// controller_thread_fn, src/rtl_fm.c:1495-1507) for -N n sources (n = 1 without -N): line i of the file is source i's
// frequency list (single frequencies and a:b:step ranges, rtlfm_scan_parse_list; blank lines and lines that start with
// '#' are skipped).  -f keeps its meaning (where a source is tuned first; without -f that is its list's first entry).
// The squelch gate runs on the device (option squelch_gate), after every run the gate's records go to the engine of
// include/rtlfm_scan.h, a source whose run held a buffer hops to its list's next entry: rtlsdr_set_center_freq() with
// the capture frequency optimal_settings() gives for it, and the first DEFAULT_BUFFER_DUMP = 4096 bytes of its next
// buffer read 127 (rtlfm_gpu_mute).  At most one hop per source and run, settle = the buffers one run may take: the
// output is a deterministic function of the input files.  -v prints every hop, the hop counts are printed at exit.
//
// -l / -t hold the output back as demod_thread_fn does (:1366-1370): on the device (squelch_gate / conseq_squelch) where
// the configuration has a gate, else per stream through the carried state.  -L prints full_demod()'s level lines.
//
// -K file / -R file (not reference letters): keep and resume.  -K writes every stream's carried state (the persisting
// fields of struct demod_state, src/rtl_fm.c:172-208; include/rtlfm_snapshot.h) at exit, behind the last run; -R loads
// such a file after the handle is created and before the first buffer, so that the output continues as if the tool had
// never stopped: the PCM of "first half with -K" + "second half with -R" is the PCM of the whole capture.  Under -N n the
// file holds n records in source order; a source that left the batch earlier contributes the record it had when it left.
// -R wants a file of exactly n records saved under the same configuration (everything the command line plans but how
// many buffers a run takes); anything else is refused with the library's text, exit status 2, before a device is opened.
// Not with -S, -C or -O agc=2: those host engines carry state of their own (hop position and settle counters, the
// monitor's cycles, the AGC's index and counters) that the snapshot does not hold.
//
// -X file (not a reference letter): channels.  Line i of the file is the list of channel frequencies of source i, in -S's
// grammar (blanks, tabs or commas, a:b:step ranges, k / M / G; blank lines and lines that start with '#' are skipped), and
// every line stands for the same number K of channels: n lines with -N n, one without.  Source i is tuned to its -f AS
// GIVEN - no capture_rate / 4 offset, no +16 kHz under -M wbfm: the library's NCO mixers take the rotation's place, channel
// c of source i with the step rtlfm_channel_step(channel_freq - f_i, capture_rate) (include/rtlfm_hip.h,
// rtlfm_gpu_set_channels), and a channel further than capture_rate / 2 from its source's -f is refused.  The rate plan is
// optimal_settings()' as under -N; -m chooses the capture rate.  ONE handle of n x K streams with the library's option
// source_ring, so that the ring has a row per SOURCE: handle stream s = channel s % K of source s / K writes the file
// with %d = s; -H, -L ("stream s:") and -l work per stream as under -N without the device gate.  -x ntaps puts the channel
// filter rtlfm_channel_lowpass(ntaps, 0.4 / D, D) in the boxcar's place (not with -F: the filter stands where the boxcar
// stands; where its taps do not fit an int16 - fewer taps than D needs - the same filter at D / 2^k and shift 14 - k).  The demod thread pushes the same number of buffers for every source and run (run_channels below); the
// streams run in lockstep on ONE sample counter, and no handle is shrunk (the library refuses state_move with channels):
// a source's short last buffer is completed with bytes 127 - which mix to 0 at every phase - to the full length and
// demodulated, a source that has ended is fed buffers of bytes 127 and its K files receive nothing more, until the last
// source ends.  Not with -S, -C, -K, -R, -Z, -O agc=2 or -E rdc: each needs what the library refuses while channels are on.
//
// Not restated (out of scope): the command file's own hop (its 2 x 3 200 000 byte mute, the DC-filter reset, -B), and
// -t negative (terminate on squelch).
#include <getopt.h>
#include <pthread.h>
#include <spawn.h>
#include <sys/wait.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/rtlfm_hip.h"
#include "../../../include/rtlfm_agc.h"
#include "../../../include/rtlfm_monitor.h"
#include "../../../include/rtlfm_scan.h"
#include "../../../include/rtlfm_snapshot.h"
#include "../../../include/rtlsdr_file.h"
#include "wavhdr.h"

namespace {

// atofs(): a number with an optional k / M / G suffix (src/convenience/convenience.c:67-96)
double atofs(const char *s)
{
	std::string t(s);
	double mul = 1.0;
	if (!t.empty()) {
		switch (t.back()) {
		case 'g': case 'G': mul = 1e9; t.pop_back(); break;
		case 'm': case 'M': mul = 1e6; t.pop_back(); break;
		case 'k': case 'K': mul = 1e3; t.pop_back(); break;
		default: break;
		}
	}
	return atof(t.c_str()) * mul;
}

struct Plumbing {
	std::mutex m;
	std::condition_variable cv_room, cv_work, cv_out;
	int queued = 0;          // buffers committed to the ring and not yet handed to rtlfm_gpu_run()
	bool slot_open = false;  // -Z: the device layer is writing into a slot of the ring (acquire ... commit)
	bool want_run = false;   // the demod thread is about to run: no new slot is handed out until it has
	bool eof = false, failed = false;
	std::deque<std::vector<int16_t>> out_q;
	bool out_done = false;
};

// -O agc=2: the software AGC and the overload report for every source (include/rtlfm_agc.h)
struct Health {
	rtlfm_agc *agc = nullptr;
	std::vector<rtlsdr_dev_t *> devs;
	std::vector<std::vector<int>> gains;  // each source's gain table, tenths of a dB
	std::vector<int> applied;             // the index each device has
	std::vector<int> overloaded;          // detect_overload's verdict on each source's last buffer
	std::vector<long long> serial;        // buffers of each source so far
	std::vector<rtlfm_input_health> recs;
	int verbosity = 0;
};

int health_create(Health *hl, const std::vector<rtlsdr_dev_t *> &devs, int settle, int verbosity)
{
	hl->devs = devs;
	hl->verbosity = verbosity;
	std::vector<int32_t> counts;
	for (rtlsdr_dev_t *d : devs) {
		const int n = rtlsdr_get_tuner_gains(d, nullptr);
		std::vector<int> g((size_t)(n > 0 ? n : 1), 0);
		if (n > 0) rtlsdr_get_tuner_gains(d, g.data());
		counts.push_back((int32_t)g.size());
		hl->gains.push_back(std::move(g));
	}
	hl->applied.assign(devs.size(), 0);  // mode 2 starts at index 0 (src/librtlsdr.c:1547)
	hl->overloaded.assign(devs.size(), 0);
	hl->serial.assign(devs.size(), 0);
	int r = rtlfm_agc_create((int)devs.size(), counts.data(), nullptr, &hl->agc);
	if (r == 0) r = rtlfm_agc_set_settle(hl->agc, settle);
	return r;
}

// after a run: stream k of the handle is source live[k], whose buffers of this run were lens[k] bytes long
int health_step(Health *hl, rtlfm_gpu *gpu, int cap, const std::vector<int> &live, const std::vector<std::vector<uint32_t>> &lens)
{
	hl->recs.resize(live.size() * (size_t)cap);
	int n = 0;
	int r = rtlfm_gpu_input_health_all(gpu, hl->recs.data(), cap, &n);
	if (r < 0) return r;
	for (size_t k = 0; k < live.size(); k++) {
		const int i = live[k];
		if ((int)lens[k].size() != n) return -EPROTO;
		const rtlfm_input_health *rec = hl->recs.data() + k * (size_t)cap;
		if ((r = rtlfm_agc_feed(hl->agc, i, rec, lens[k].data(), n)) < 0) return r;
		for (int b = 0; b < n; b++) {
			const int ov = 8000ll * rec[b].overload >= (long long)lens[k][(size_t)b] ? 1 : 0;  // src/rtl_tcp.c:243
			if (ov != hl->overloaded[(size_t)i] && hl->verbosity)
				fprintf(stderr, "stream %d: buffer %lld: overload %s\n", i, hl->serial[(size_t)i], ov ? "begins" : "ends");
			hl->overloaded[(size_t)i] = ov;
			hl->serial[(size_t)i]++;
		}
	}
	rtlfm_agc_event ev[64];
	for (;;) {
		int ne = 0;
		if ((r = rtlfm_agc_poll(hl->agc, ev, 64, &ne)) < 0) return r;
		if (hl->verbosity)
			for (int e = 0; e < ne; e++)
				fprintf(stderr, "stream %d: buffer %lld: gain index %d -> %d, gain %d (%s)\n", ev[e].stream, (long long)ev[e].buffer_serial,
				        ev[e].old_index, ev[e].new_index, hl->gains[(size_t)ev[e].stream][(size_t)ev[e].new_index],
				        ev[e].overloaded ? "overload" : "low level");
		if (ne < 64) break;
	}
	for (int i : live) {
		int32_t idx = 0;
		if ((r = rtlfm_agc_state(hl->agc, i, &idx, nullptr, nullptr, nullptr)) < 0) return r;
		if (idx != hl->applied[(size_t)i]) {
			rtlamd_file_set_gain_index(hl->devs[(size_t)i], idx);
			hl->applied[(size_t)i] = idx;
		}
	}
	return 0;
}

void health_report(Health *hl)
{
	for (size_t i = 0; i < hl->devs.size(); i++) {
		int32_t idx = 0;
		uint64_t total = 0, dropped = 0;
		rtlfm_agc_state(hl->agc, (int)i, &idx, nullptr, &total, &dropped);
		fprintf(stderr, "stream %zu: final gain index %d, gain %d\n", i, idx, hl->gains[i][(size_t)idx]);
	}
}

// the parts agc=<n> of a -O string: the last one's value, -1 when there is none, -2 for anything but 0, 1, 2
int opt_string_agc(const char *opts)
{
	int agc = -1;
	const std::string t(opts);
	for (size_t at = 0; at <= t.size();) {
		size_t end = t.find(':', at);
		if (end == std::string::npos) end = t.size();
		const std::string part = t.substr(at, end - at);
		if (part.compare(0, 4, "agc=") == 0) {
			if (part.size() != 5 || part[4] < '0' || part[4] > '2') return -2;
			agc = part[4] - '0';
		}
		at = end + 1;
	}
	return agc;
}

struct App {
	rtlfm_cfg cfg;
	rtlfm_gpu *gpu = nullptr;
	rtlsdr_dev_t *dev = nullptr;
	Plumbing p;
	FILE *file = nullptr;
	rtlamd_wave wave{};
	int verbosity = 0;
	int conseq_squelch = 10;
	// -L (src/rtl_fm.c:109-113, 1217-1237)
	int print_levels = 0, print_level_no = 1, level_max = 0, level_max_max = 0;
	double level_sum = 0.0;
	uint32_t user_freq = 0;
	uint64_t blocks_in = 0, samples_out = 0, blocks_squelched = 0;
	bool use_gate = false;             // -l through the device's squelch gate (rtlfm_gpu_gate)
	const char *keep_file = nullptr;   // -K: the snapshot written at exit
	bool zero_copy = false;            // -Z: the device layer reads straight into the pinned staging ring
	unsigned char *open_slot = nullptr;  // the slot the device layer is filling (rtlfm_gpu_acquire)
	Health hl;                         // -O agc=2
	std::deque<uint32_t> in_lens;      // ... the lengths of the buffers in the ring, oldest first (under p.m)
};

// -Z: where the device layer reads its next buffer to (rtlamd_file_set_buffer_source): a slot of the GPU
// layer's pinned ring, the counterpart of the reference's zero-copy USB buffers (src/librtlsdr.c:2744-2810)
int next_slot(void *ctx, unsigned char **buf, uint32_t *cap)
{
	App *a = static_cast<App *>(ctx);
	// rtlfm_gpu_run() refuses to start while a slot is open (it takes every buffer whole or not at all), and
	// this thread asks for its next slot the moment a callback returns: the slot is handed out under the
	// plumbing's lock, and not while the demod thread has announced a run or the ring is full - otherwise
	// the demod thread would hardly ever find the ring closed and committed buffers would sit there.
	std::unique_lock<std::mutex> g(a->p.m);
	for (;;) {
		a->p.cv_room.wait(g, [&] { return (!a->p.want_run && a->p.queued < a->cfg.max_blocks) || a->p.failed; });
		if (a->p.failed) return -1;
		uint8_t *p = nullptr;
		int r = rtlfm_gpu_acquire(a->gpu, 0, &p, cap);
		if (r == 0) { a->open_slot = p; a->p.slot_open = true; *buf = p; return 0; }
		if (r != -ENOSPC) return r;  // not fatal: the device layer falls back to its own buffer and the callback pushes
		// the ring's filling half is full although `queued` says otherwise (a run that has not flipped the halves
		// yet): wait for the demod thread's next notification instead of spinning
		a->p.cv_room.wait_for(g, std::chrono::milliseconds(2));
	}
}

// the rtlsdr_read_async callback (reference rtlsdr_callback, src/rtl_fm.c:1274)
void on_buffer(unsigned char *buf, uint32_t len, void *ctx)
{
	App *a = static_cast<App *>(ctx);
	len -= len % 512;  // actual_length comes in whole USB packets; a file's last bytes may not
	if (a->open_slot && buf == a->open_slot) {
		// the samples are already where they belong: say how many (0 gives the slot back)
		a->open_slot = nullptr;
		int r = rtlfm_gpu_commit(a->gpu, 0, len);
		std::lock_guard<std::mutex> g(a->p.m);
		a->p.slot_open = false;
		if (r < 0) {
			fprintf(stderr, "rtlfm_gpu_commit: %s\n", rtlfm_gpu_strerror(r));
			a->p.failed = true;
			rtlsdr_cancel_async(a->dev);
		} else if (len) {
			a->p.queued++;
			a->blocks_in++;
			if (a->hl.agc) a->in_lens.push_back(len);
		}
		a->p.cv_work.notify_all();
		return;
	}
	if (len == 0) return;
	// the copy is made under the plumbing's lock and not while the demod thread has announced a run: `queued`
	// is then exactly what the ring holds when rtlfm_gpu_run() takes it
	std::unique_lock<std::mutex> g(a->p.m);
	for (;;) {
		a->p.cv_room.wait(g, [&] { return (!a->p.want_run && a->p.queued < a->cfg.max_blocks) || a->p.failed; });
		if (a->p.failed) return;
		int r = rtlfm_gpu_push(a->gpu, 0, buf, len);
		if (r == 0) break;
		if (r != -ENOSPC) {
			fprintf(stderr, "rtlfm_gpu_push: %s\n", rtlfm_gpu_strerror(r));
			a->p.failed = true;
			rtlsdr_cancel_async(a->dev);  // the reference's error pattern, src/rtl_sdr.c:109-112
			a->p.cv_work.notify_all();
			return;
		}
		a->p.cv_room.wait_for(g, std::chrono::milliseconds(2));
	}
	a->p.queued++;
	a->blocks_in++;
	if (a->hl.agc) a->in_lens.push_back(len);
	a->p.cv_work.notify_all();
}

void dongle_thread(App *a)
{
	if (a->zero_copy) rtlamd_file_set_buffer_source(a->dev, next_slot, a);
	rtlsdr_read_async(a->dev, on_buffer, a, 0, a->cfg.block_len);
	std::lock_guard<std::mutex> g(a->p.m);
	a->p.eof = true;
	a->p.cv_work.notify_all();
}

void demod_thread(App *a)
{
	const int cap = rtlfm_result_cap(&a->cfg) * a->cfg.max_blocks + 16;
	for (;;) {
		int taken = 0;
		{
			std::unique_lock<std::mutex> g(a->p.m);
			a->p.cv_work.wait(g, [&] { return a->p.queued > 0 || a->p.eof || a->p.failed; });
			if (a->p.failed || (a->p.queued == 0 && a->p.eof)) break;
			// -Z: no new slot from here on (next_slot), and the one that is open is committed first
			a->p.want_run = true;
			a->p.cv_work.wait(g, [&] { return !a->p.slot_open || a->p.failed; });
			if (a->p.failed) break;
			taken = a->p.queued;  // rtlfm_gpu_run takes everything that is queued
		}
		// The gate is held around the FLIP of the ring's halves only (rtlfm_gpu_run_begin): the transfer, a first run's
		// allocations and the kernel launches (rtlfm_gpu_run_end) happen with the device thread already filling the other
		// half - a callback never waits for a transfer or a kernel, as include/rtlfm_hip.h promises.
		std::vector<std::vector<uint32_t>> run_lens;
		int r = rtlfm_gpu_run_begin(a->gpu, &taken);
		{
			std::lock_guard<std::mutex> g(a->p.m);
			a->p.want_run = false;
			// the count goes down only for a run that has started: on -EAGAIN the buffers are still in the ring
			if (r == 0) a->p.queued -= taken;
			if (r == 0 && a->hl.agc) {
				run_lens.assign(1, std::vector<uint32_t>(a->in_lens.begin(), a->in_lens.begin() + taken));
				a->in_lens.erase(a->in_lens.begin(), a->in_lens.begin() + taken);
			}
			a->p.cv_room.notify_all();
		}
		if (r == -EAGAIN) { std::this_thread::yield(); continue; }
		if (r == 0) r = rtlfm_gpu_run_end(a->gpu);
		std::vector<int16_t> pcm((size_t)cap);
		int n = 0;
		if (r == 0) r = rtlfm_gpu_fetch(a->gpu, 0, pcm.data(), cap, &n);
		if (r == 0 && a->hl.agc) r = health_step(&a->hl, a->gpu, a->cfg.max_blocks, {0}, run_lens);
		if (r < 0) {
			fprintf(stderr, "rtlfm_gpu_run/fetch: %s\n", rtlfm_gpu_strerror(r));
			std::lock_guard<std::mutex> g(a->p.m);
			a->p.failed = true;
			rtlsdr_cancel_async(a->dev);
			a->p.cv_room.notify_all();
			break;
		}
		pcm.resize((size_t)n);
		if (a->print_levels) {
			// full_demod()'s level printing, src/rtl_fm.c:1217-1237, on the rms() the GPU layer kept
			int32_t sr = 0;
			int nl = 0;
			if (rtlfm_gpu_levels(a->gpu, 0, &sr, 1, &nl) == 0 && nl == 1) {
				--a->print_level_no;
				if (sr >= 0) {
					a->level_sum += sr;
					if (a->level_max < sr) a->level_max = sr;
					if (a->level_max_max < sr) a->level_max_max = sr;
					if (!a->print_level_no) {
						a->print_level_no = a->print_levels;
						const double avg_rms = a->level_sum / a->print_levels;
						fprintf(stderr, "%.3f kHz, %.1f avg rms, %d max rms, %d max max rms, %d squelch rms, %d rms, %.1f dB rms level, %.2f dB avg rms level\n",
						        a->user_freq / 1000.0, avg_rms, a->level_max, a->level_max_max, a->cfg.squelch_level, (int)sr,
						        20.0 * log10(1E-10 + sr), 20.0 * log10(1E-10 + avg_rms));
						a->level_max = 0;
						a->level_sum = 0;
					}
				}
			}
		}
		if (a->use_gate) {
			// the same rule, applied on the device: a held buffer comes back with no samples and its record says so
			rtlfm_gate_rec g1;
			int ng = 0;
			if (rtlfm_gpu_gate(a->gpu, 0, &g1, 1, &ng) == 0 && ng == 1 && !g1.emit) {
				a->blocks_squelched++;
				continue;
			}
		} else if (a->cfg.squelch_level) {
			// demod_thread_fn(), src/rtl_fm.c:1366-1370: while the squelch has been closed for more than
			// conseq_squelch buffers nothing goes to the output thread, and the counter is held one above
			// the limit ("hair trigger").  squelch_hits starts at 11 (:1615): silence until it first opens.
			// One read of the state per run, and a write only when the counter was clamped.
			rtlfm_stream_state st;
			int ns = 0;
			if (rtlfm_gpu_state_get_all(a->gpu, &st, 1, &ns) == 0 && st.squelch_hits > a->conseq_squelch) {
				if (st.squelch_hits != a->conseq_squelch + 1) {
					st.squelch_hits = a->conseq_squelch + 1;
					rtlfm_gpu_state_set_all(a->gpu, &st, 1);
				}
				a->blocks_squelched++;
				continue;
			}
		}
		std::lock_guard<std::mutex> g(a->p.m);
		a->p.out_q.push_back(std::move(pcm));
		a->p.cv_out.notify_one();
	}
	std::lock_guard<std::mutex> g(a->p.m);
	a->p.out_done = true;
	a->p.cv_out.notify_all();
}

void output_thread(App *a)
{
	for (;;) {
		std::vector<int16_t> pcm;
		{
			std::unique_lock<std::mutex> g(a->p.m);
			a->p.cv_out.wait(g, [&] { return !a->p.out_q.empty() || a->p.out_done; });
			if (a->p.out_q.empty()) break;
			pcm = std::move(a->p.out_q.front());
			a->p.out_q.pop_front();
		}
		fwrite(pcm.data(), 2, pcm.size(), a->file);  // src/rtl_fm.c:1400
		a->wave.data_size += 2 * (uint32_t)pcm.size();  // waveDataSize, :1401
		a->samples_out += pcm.size();
	}
	fflush(a->file);
}

// ---- -N n: devices d .. d+n-1 as streams 0 .. n-1 of one handle ----------------------------------------
//
// rtlfm_gpu_run() takes every stream's queued buffers and wants the same number from each (-EAGAIN otherwise), so
// the callbacks do not push into the ring themselves: each copies its buffer into a host queue of its own stream
// (at most `depth` buffers; a full queue makes the callback wait, nothing is dropped), and the demod thread, once
// every live stream has a buffer, takes b = min(what every queue holds, max_blocks) from each, pushes them and runs.
// The slowest source sets the pace of all.  A stream whose source has ended and whose queue is empty leaves the
// batch: the others move, carried state and all, to a handle with one stream fewer for each that left.  Between runs
// nothing is left in the ring (every push is taken by the run right behind it, whose results are fetched before the
// next push), so the state is all there is to move, and no stream loses a sample or sees one twice.

struct Multi;

struct Source {
	int index = 0;                            // stream index: output file, %d, "stream i:"
	rtlsdr_dev_t *dev = nullptr;
	uint32_t user_freq = 0, capture_freq = 0;
	FILE *file = nullptr;
	rtlamd_wave wave{};
	Multi *m = nullptr;
	std::deque<std::vector<uint8_t>> q;       // buffers copied by the callback, not yet taken by a run
	std::vector<std::vector<uint8_t>> spare;  // taken buffers come back here, so a callback hardly ever allocates
	std::vector<std::vector<uint8_t>> taken;  // what the current run pushes
	int copying = 0;                          // callbacks copying into a reserved place of the queue
	bool eof = false;
	std::condition_variable cv_room;
	// -L (src/rtl_fm.c:109-113, 1217-1237), per stream
	int print_level_no = 1, level_max = 0, level_max_max = 0;
	double level_sum = 0.0;
	uint64_t blocks_in = 0, samples_out = 0, blocks_squelched = 0;
};

struct RunOut {
	std::vector<int16_t> pcm;  // handle stream k at k * stride
	std::vector<int32_t> lens;
	std::vector<int> who;      // handle stream k -> source
	size_t stride = 0;
};

struct Multi {
	rtlfm_cfg cfg;
	rtlfm_gpu *gpu = nullptr;
	std::vector<Source> src;
	int depth = 0;
	int verbosity = 0, conseq_squelch = 10, print_levels = 0;
	std::mutex m;
	std::condition_variable cv_work, cv_out;
	bool failed = false, out_done = false;
	std::deque<RunOut> out_q;
	// -C: the level monitor, rule i = source i
	rtlfm_monitor *mon = nullptr;
	std::vector<rtlfm_monitor_rule> rules;
	std::vector<pid_t> children;
	uint64_t events = 0, fired = 0;
	Health hl;  // -O agc=2
	bool use_gate = false;  // -l through the device's squelch gate
	// -S: the hop engine, list i = source i
	rtlfm_scan *scan = nullptr;
	std::vector<rtlfm_gate_rec> gate_recs;
	bool wb_mode = false;
	int rate_in = 0, min_capture = 0, fifth = 0, edge = 0;  // what optimal_settings() is asked with for a hop
	// -K: record i = source i.  A source that leaves the batch leaves its record here (shrink); the others' are read at exit
	const char *keep_file = nullptr;
	std::vector<rtlfm_stream_state> kept;
	std::vector<int> live;                   // handle stream k -> source, as the demod thread left it
	std::vector<rtlfm_stream_state> states;  // one rtlfm_gpu_state_get_all: -l without a device gate, -K
	// -X: K channels per source; chan[s] = what handle stream s owns (its file, wave header, -L counters), index = s
	int chan_per = 0;
	std::vector<Source> chan;
};

// the options a handle of this tool runs with besides its configuration
int handle_options(Multi *m, rtlfm_gpu *h)
{
	int r = 0;
	if (m->mon) r = rtlfm_gpu_set_option(h, "input_stats", 1);
	if (r == 0 && m->hl.agc) r = rtlfm_gpu_set_option(h, "input_health", 1);
	if (r == 0 && m->use_gate) r = rtlfm_gpu_set_option(h, "conseq_squelch", m->conseq_squelch);
	if (r == 0 && m->use_gate) r = rtlfm_gpu_set_option(h, "squelch_gate", 1);
	return r;
}

// with m->m held
void fail_multi(Multi *m, const char *what, int r)
{
	fprintf(stderr, "%s: %s\n", what, rtlfm_gpu_strerror(r));
	m->failed = true;
	for (Source &s : m->src) {
		rtlsdr_cancel_async(s.dev);
		s.cv_room.notify_all();
	}
	m->cv_work.notify_all();
}

void on_buffer_multi(unsigned char *buf, uint32_t len, void *ctx)
{
	Source *s = static_cast<Source *>(ctx);
	Multi *m = s->m;
	len -= len % 512;  // as on_buffer
	if (len == 0) return;
	std::vector<uint8_t> b;
	{
		std::unique_lock<std::mutex> g(m->m);
		s->cv_room.wait(g, [&] { return (int)s->q.size() + s->copying < m->depth || m->failed; });
		if (m->failed) return;
		s->copying++;
		if (!s->spare.empty()) {
			b = std::move(s->spare.back());
			s->spare.pop_back();
		}
	}
	b.assign(buf, buf + len);  // outside the lock: the other devices' callbacks copy at the same time
	std::lock_guard<std::mutex> g(m->m);
	s->copying--;
	s->q.push_back(std::move(b));
	s->blocks_in++;
	m->cv_work.notify_one();
}

void dongle_thread_multi(Source *s)
{
	rtlsdr_read_async(s->dev, on_buffer_multi, s, 0, s->m->cfg.block_len);
	std::lock_guard<std::mutex> g(s->m->m);
	s->eof = true;  // after the last callback: the queue holds everything the source gave
	s->m->cv_work.notify_one();
}

// -K: the records of the handle's streams (stream k = source live[k]) into m->kept - with `stay`, only those of the
// sources that are not in it (the ones that leave)
int keep_states(Multi *m, const std::vector<int> &live, const std::vector<int> *stay)
{
	m->states.resize(live.size());
	int n = 0;
	const int r = rtlfm_gpu_state_get_all(m->gpu, m->states.data(), (int)live.size(), &n);
	if (r < 0) return r;
	for (size_t k = 0; k < live.size(); k++)
		if (!stay || std::find(stay->begin(), stay->end(), live[k]) == stay->end()) m->kept[(size_t)live[k]] = m->states[k];
	return 0;
}

// the streams in `stay` (a subsequence of `live`) go on, on a new handle with stay.size() streams: ONE
// rtlfm_gpu_state_move, which takes each stream's carried state and the hop mute the old handle still owed it
int shrink(Multi *m, const std::vector<int> &live, const std::vector<int> &stay)
{
	int r = 0;
	if (m->keep_file && (r = keep_states(m, live, &stay)) < 0) return r;  // in front of the regroup: what the leaving sources carried
	rtlfm_gpu *nh = nullptr;
	r = rtlfm_gpu_create(&m->cfg, (int)stay.size(), 0, &nh);
	if (r < 0) return r;
	std::vector<int32_t> map;
	for (size_t i = 0, k = 0; i < live.size() && k < stay.size(); i++) {
		if (live[i] != stay[k]) continue;
		map.push_back((int32_t)i);
		k++;
	}
	r = map.size() == stay.size() ? handle_options(m, nh) : -EPROTO;
	if (r == 0) r = rtlfm_gpu_state_move(nh, m->gpu, map.data(), (int)map.size());
	if (r < 0) {
		rtlfm_gpu_destroy(nh);
		return r;
	}
	rtlfm_gpu_destroy(m->gpu);
	m->gpu = nh;
	return 0;
}

void levels_multi(Multi *m, Source &s, int k)
{
	// as demod_thread's -L block, per stream
	int32_t sr = 0;
	int nl = 0;
	if (rtlfm_gpu_levels(m->gpu, k, &sr, 1, &nl) != 0 || nl != 1) return;
	--s.print_level_no;
	if (sr < 0) return;
	s.level_sum += sr;
	if (s.level_max < sr) s.level_max = sr;
	if (s.level_max_max < sr) s.level_max_max = sr;
	if (s.print_level_no) return;
	s.print_level_no = m->print_levels;
	const double avg_rms = s.level_sum / m->print_levels;
	fprintf(stderr, "stream %d: %.3f kHz, %.1f avg rms, %d max rms, %d max max rms, %d squelch rms, %d rms, %.1f dB rms level, %.2f dB avg rms level\n",
	        s.index, s.user_freq / 1000.0, avg_rms, s.level_max, s.level_max_max, m->cfg.squelch_level, (int)sr,
	        20.0 * log10(1E-10 + sr), 20.0 * log10(1E-10 + avg_rms));
	s.level_max = 0;
	s.level_sum = 0;
}

// -C: a fired event's command, in the background and without a shell: argv[0] = the command, the arguments split at
// blanks, an argument that IS one of the placeholders replaced (src/rtl_fm.c:722-727, executeInBackground)
void start_command(Multi *m, const rtlfm_monitor_rule &r, const rtlfm_monitor_event &ev)
{
	static const char *crit_names[] = {"in", "out", "<", ">"};  // aCritStr, :116
	fprintf(stderr, "command to trigger is '%s %s'\n", r.command, r.args);
	char v_freq[32], v_gain[32], v_level[32], v_ref[32], v_tol[32];
	snprintf(v_freq, sizeof(v_freq), "%u", r.freq);
	snprintf(v_gain, sizeof(v_gain), "%d", r.gain);
	snprintf(v_level, sizeof(v_level), "%d", (int)(0.5 + ev.level_db * 10.0));
	snprintf(v_ref, sizeof(v_ref), "%d", (int)(0.5 + r.ref_level * 10.0));
	snprintf(v_tol, sizeof(v_tol), "%d", (int)(0.5 + r.ref_tol * 10.0));
	const char *names[] = {"!freq!", "!gain!", "!mlevel!", "!crit!", "!reflevel!", "!reftol!"};
	const char *values[] = {v_freq, v_gain, v_level, crit_names[r.crit & 3], v_ref, v_tol};
	std::vector<std::string> words{r.command};
	std::string cur;
	for (const char *p = r.args;; p++) {
		if (*p && *p != ' ' && *p != '\t') { cur += *p; continue; }
		if (!cur.empty()) {
			for (int k = 0; k < 6; k++)
				if (cur == names[k]) { cur = values[k]; break; }
			words.push_back(cur);
			cur.clear();
		}
		if (!*p) break;
	}
	std::vector<char *> argv;
	for (std::string &w : words) argv.push_back(&w[0]);
	argv.push_back(nullptr);
	pid_t pid = 0;
	const int e = posix_spawnp(&pid, r.command, nullptr, nullptr, argv.data(), environ);
	if (e) fprintf(stderr, "cannot start '%s': %s\n", r.command, strerror(e));
	else m->children.push_back(pid);
}

// -C: after a run, feed the monitor and act on what it reports.  While every source is alive the handle's streams ARE
// the file's lines (rtlfm_monitor_update: one copy of the levels, one of the records); once sources have left, stream k
// of the handle is line live[k].
int monitor_step(Multi *m, const std::vector<int> &live)
{
	int r = 0;
	if (live.size() == m->src.size()) {
		r = rtlfm_monitor_update(m->mon, m->gpu);
	} else {
		const int cap = m->cfg.max_blocks;
		std::vector<int32_t> lv(live.size() * (size_t)cap);
		std::vector<rtlfm_input_stat> st(live.size() * (size_t)cap);
		int n = 0, ns = 0;
		r = rtlfm_gpu_levels_all(m->gpu, lv.data(), cap, &n);
		if (r == 0) r = rtlfm_gpu_input_stats_all(m->gpu, st.data(), cap, &ns);
		for (size_t k = 0; k < live.size() && r == 0; k++)
			r = rtlfm_monitor_feed(m->mon, live[k], lv.data() + k * cap, ns == n ? st.data() + k * cap : nullptr, n);
	}
	if (r < 0) return r;
	rtlfm_monitor_event ev[64];
	for (;;) {
		int n = 0;
		if ((r = rtlfm_monitor_poll(m->mon, ev, 64, &n)) < 0) return r;
		for (int i = 0; i < n; i++) {
			const rtlfm_monitor_rule &rule = m->rules[(size_t)ev[i].stream];
			m->events++;
			if (m->verbosity) {
				char line[512];
				rtlfm_monitor_format_event(&rule, &ev[i], line, sizeof(line));
				fprintf(stderr, "stream %d: %s\n", ev[i].stream, line);
			}
			if (ev[i].fired) {
				m->fired++;
				if (rule.command[0]) start_command(m, rule, ev[i]);
			}
		}
		if (n < 64) return 0;
	}
}

// -l on the device, and -S: after a run, the gate's records of every stream in one copy - what was held is counted, and
// with -S the records go to the hop engine: every hop retunes its source (controller_thread_fn, src/rtl_fm.c:1504-1507)
// and leaves a mute for the source's next buffer.  Stream k of the handle is source live[k].
int gate_step(Multi *m, const std::vector<int> &live)
{
	const int cap = m->cfg.max_blocks;
	m->gate_recs.resize(live.size() * (size_t)cap);
	int n = 0;
	int r = rtlfm_gpu_gate_all(m->gpu, m->gate_recs.data(), cap, &n);
	if (r < 0) return r;
	for (size_t k = 0; k < live.size(); k++) {
		Source &s = m->src[(size_t)live[k]];
		for (int b = 0; b < n; b++)
			if (!m->gate_recs[k * (size_t)cap + b].emit) s.blocks_squelched++;
		if (m->scan && (r = rtlfm_scan_feed(m->scan, live[k], m->gate_recs.data() + k * (size_t)cap, n)) < 0) return r;
	}
	if (!m->scan) return 0;
	rtlfm_scan_event ev[64];
	for (;;) {
		int ne = 0;
		if ((r = rtlfm_scan_events(m->scan, ev, 64, &ne)) < 0) return r;
		for (int e = 0; e < ne; e++) {
			Source &s = m->src[(size_t)ev[e].stream];
			const uint32_t f_new = ev[e].freq + (m->wb_mode ? 16000u : 0u);  // src/rtl_fm.c:1455-1460
			rtlfm_cfg ci = m->cfg;
			uint32_t cf = 0;
			rtlfm_optimal_settings(&ci, f_new, m->rate_in, m->min_capture, m->fifth, m->edge, &cf, nullptr);
			rtlsdr_set_center_freq(s.dev, cf);  // :1506
			if (m->verbosity)
				fprintf(stderr, "stream %d: hop %u -> %u at buffer %lld\n", ev[e].stream, s.user_freq, f_new, (long long)ev[e].buffer_serial);
			s.user_freq = f_new;
			s.capture_freq = cf;
		}
		if (ne < 64) break;
	}
	std::vector<int32_t> hopped(m->src.size());
	int nh = 0;
	if ((r = rtlfm_scan_take_hopped(m->scan, hopped.data(), (int)hopped.size(), &nh)) < 0) return r;
	for (int i = 0; i < nh; i++) {
		const size_t k = (size_t)(std::find(live.begin(), live.end(), (int)hopped[(size_t)i]) - live.begin());
		if (k == live.size()) continue;
		if ((r = rtlfm_gpu_mute(m->gpu, (int)k, RTLFM_SCAN_DEFAULT_DUMP)) < 0) return r;  // dongle.mute = DEFAULT_BUFFER_DUMP, :1507
	}
	return 0;
}

void demod_thread_multi(Multi *m)
{
	const size_t stride = ((size_t)rtlfm_result_cap(&m->cfg) * m->cfg.max_blocks + 16 + 63) / 64 * 64;
	std::vector<int> live;
	for (size_t i = 0; i < m->src.size(); i++) live.push_back((int)i);
	// -vv: where this thread's time goes (waiting for the slowest source, the copy into the ring, run + fetch, the
	// per-stream -l / -L calls)
	using clk = std::chrono::steady_clock;
	double t_wait = 0, t_push = 0, t_run = 0, t_per_stream = 0;
	uint64_t runs = 0;
	auto since = [](clk::time_point t0) { return std::chrono::duration<double>(clk::now() - t0).count(); };
	for (;;) {
		std::vector<int> stay;
		int b = m->cfg.max_blocks;
		clk::time_point t0 = clk::now();
		{
			std::unique_lock<std::mutex> g(m->m);
			m->cv_work.wait(g, [&] {
				if (m->failed) return true;
				for (int i : live)
					if (m->src[i].q.empty() && !m->src[i].eof) return false;
				return true;
			});
			if (m->failed) break;
			for (int i : live)
				if (!m->src[i].q.empty()) stay.push_back(i);  // an empty queue here means the source has ended
			for (int i : stay) b = std::min(b, (int)m->src[i].q.size());
			for (int i : stay) {
				Source &s = m->src[i];
				for (int j = 0; j < b; j++) {
					s.taken.push_back(std::move(s.q.front()));
					s.q.pop_front();
				}
				s.cv_room.notify_all();
			}
		}
		if (stay.empty()) break;
		if (stay.size() != live.size()) {
			int r = shrink(m, live, stay);
			if (r < 0) {
				std::lock_guard<std::mutex> g(m->m);
				fail_multi(m, "rtlfm_gpu_create / rtlfm_gpu_state_move", r);
				break;
			}
			if (m->verbosity)
				fprintf(stderr, "%zu of %zu streams go on (the others' sources have ended)\n", stay.size(), m->src.size());
			live = stay;
		}
		// the pushes of different streams may run concurrently (rtlfm_hip.h): a few threads share the copy into the ring
		t_wait += since(t0);
		t0 = clk::now();
		const size_t ns = live.size();
		const size_t nt = std::min<size_t>(16, (ns + 15) / 16);
		std::vector<int> err(nt, 0);
		auto push_some = [&](size_t t) {
			for (size_t k = t * ns / nt; k < (t + 1) * ns / nt && !err[t]; k++)
				for (const std::vector<uint8_t> &buf : m->src[live[k]].taken) {
					int r = rtlfm_gpu_push(m->gpu, (int)k, buf.data(), (uint32_t)buf.size());
					if (r < 0) { err[t] = r; break; }
				}
		};
		if (nt == 1) {
			push_some(0);
		} else {
			std::vector<std::thread> th;
			for (size_t t = 0; t < nt; t++) th.emplace_back(push_some, t);
			for (std::thread &t : th) t.join();
		}
		int r = 0;
		for (int e : err) if (e < 0 && r == 0) r = e;
		t_push += since(t0);
		t0 = clk::now();
		int ran = 0;
		if (r == 0) r = rtlfm_gpu_run_begin(m->gpu, &ran);
		if (r == 0 && ran != b) r = -EPROTO;
		if (r == 0) r = rtlfm_gpu_run_end(m->gpu);
		RunOut o;
		o.stride = stride;
		o.pcm.resize(ns * stride);
		o.lens.resize(ns);
		o.who = live;
		if (r == 0) r = rtlfm_gpu_fetch_all(m->gpu, o.pcm.data(), stride, o.lens.data());
		if (r < 0) {
			std::lock_guard<std::mutex> g(m->m);
			fail_multi(m, "rtlfm_gpu_push/run/fetch_all", r);
			break;
		}
		if (m->hl.agc) {
			std::vector<std::vector<uint32_t>> lens(ns);
			for (size_t k = 0; k < ns; k++)
				for (const std::vector<uint8_t> &buf : m->src[live[k]].taken) lens[k].push_back((uint32_t)buf.size());
			if ((r = health_step(&m->hl, m->gpu, m->cfg.max_blocks, live, lens)) < 0) {
				std::lock_guard<std::mutex> g(m->m);
				fail_multi(m, "rtlfm_gpu_input_health_all / rtlfm_agc_feed", r);
				break;
			}
		}
		if (m->mon && (r = monitor_step(m, live)) < 0) {
			std::lock_guard<std::mutex> g(m->m);
			fail_multi(m, "rtlfm_monitor_update / feed", r);
			break;
		}
		if (m->use_gate && (r = gate_step(m, live)) < 0) {
			std::lock_guard<std::mutex> g(m->m);
			fail_multi(m, "rtlfm_gpu_gate_all / rtlfm_scan_feed / rtlfm_gpu_mute", r);
			break;
		}
		t_run += since(t0);
		t0 = clk::now();
		runs++;
		if (m->print_levels)
			for (size_t k = 0; k < ns; k++) levels_multi(m, m->src[live[k]], (int)k);
		if (m->cfg.squelch_level && !m->use_gate) {
			// demod_thread's squelch rule (src/rtl_fm.c:1366-1370), per stream; max_blocks is 1 here.  Every stream's state in
			// one copy, and one copy back only in a run that clamped a counter
			m->states.resize(ns);
			int got = 0;
			bool clamped = false;
			if (rtlfm_gpu_state_get_all(m->gpu, m->states.data(), (int)ns, &got) == 0) {
				for (size_t k = 0; k < ns; k++) {
					rtlfm_stream_state &st = m->states[k];
					if (st.squelch_hits <= m->conseq_squelch) continue;
					clamped |= st.squelch_hits != m->conseq_squelch + 1;
					st.squelch_hits = m->conseq_squelch + 1;
					m->src[live[k]].blocks_squelched++;
					o.lens[k] = 0;
				}
				if (clamped) rtlfm_gpu_state_set_all(m->gpu, m->states.data(), (int)ns);
			}
		}
		t_per_stream += since(t0);
		std::lock_guard<std::mutex> g(m->m);
		for (int i : live) {
			Source &s = m->src[i];
			for (std::vector<uint8_t> &buf : s.taken) s.spare.push_back(std::move(buf));
			s.taken.clear();
		}
		m->out_q.push_back(std::move(o));
		m->cv_out.notify_one();
	}
	m->live = live;
	if (m->verbosity >= 2)
		fprintf(stderr, "demod thread: %llu runs; %.3f s waiting for buffers, %.3f s pushing, %.3f s run + fetch_all, %.3f s -l / -L\n",
		        (unsigned long long)runs, t_wait, t_push, t_run, t_per_stream);
	std::lock_guard<std::mutex> g(m->m);
	m->out_done = true;
	m->cv_out.notify_all();
}

void output_thread_multi(Multi *m)
{
	for (;;) {
		RunOut o;
		{
			std::unique_lock<std::mutex> g(m->m);
			m->cv_out.wait(g, [&] { return !m->out_q.empty() || m->out_done; });
			if (m->out_q.empty()) break;
			o = std::move(m->out_q.front());
			m->out_q.pop_front();
		}
		for (size_t k = 0; k < o.who.size(); k++) {
			Source &s = m->chan_per ? m->chan[o.who[k]] : m->src[o.who[k]];  // (-X: who = the handle's streams)
			const size_t n = (size_t)o.lens[k];
			if (!n) continue;
			fwrite(o.pcm.data() + k * o.stride, 2, n, s.file);
			s.wave.data_size += 2 * (uint32_t)n;
			s.samples_out += n;
		}
	}
	for (Source &s : m->chan_per ? m->chan : m->src) fflush(s.file);
}

// everything after option parsing for n > 1 (main has refused what -N does not allow)
int run_multi(const rtlfm_cfg &planned, int n, int dev_index, const std::vector<uint32_t> &freqs,
              const std::vector<uint32_t> &capture_freqs, uint32_t capture_rate, int gain, int ppm, const std::string &pattern,
              bool write_wav, int verbosity, int conseq_squelch, int print_levels, const std::vector<rtlfm_monitor_rule> &rules,
              const char *opt_string, int agc, const std::vector<std::vector<uint32_t>> &scan_lists, bool wb_mode, int rate_in,
              int min_capture, int fifth, int edge, const char *keep_file, const char *resume_file)
{
	Multi m;
	m.keep_file = keep_file;
	m.kept.resize((size_t)n);
	m.wb_mode = wb_mode; m.rate_in = rate_in; m.min_capture = min_capture; m.fifth = fifth; m.edge = edge;
	m.rules = rules;
	m.cfg = planned;
	rtlfm_cfg &c = m.cfg;
	m.depth = 2 * c.max_blocks;
	m.verbosity = verbosity;
	m.conseq_squelch = conseq_squelch;
	m.print_levels = print_levels;
	m.src = std::vector<Source>((size_t)n);
	const uint32_t count = rtlsdr_get_device_count();
	if (count == 0) { fprintf(stderr, "No supported devices found (set RTLSDR_FILE or RTLSDR_FILE_LIST).\n"); return 1; }
	if ((uint64_t)dev_index + (uint64_t)n > count) {
		fprintf(stderr, "-d %d -N %d needs devices %d .. %d, and there are %u.\n", dev_index, n, dev_index, dev_index + n - 1, count);
		return 1;
	}
	int ret = 0;
	for (int i = 0; i < n && !ret; i++) {
		Source &s = m.src[i];
		s.index = i;
		s.m = &m;
		s.user_freq = freqs[i];
		s.capture_freq = capture_freqs[i];
		if (rtlsdr_open(&s.dev, (uint32_t)(dev_index + i)) < 0) {
			fprintf(stderr, "Failed to open rtlsdr device #%d.\n", dev_index + i);
			ret = 1;
			break;
		}
		const int g_i = rules.empty() ? gain : rules[(size_t)i].gain;  // -C: each source's gain from its line
		if (g_i == -100) rtlsdr_set_tuner_gain_mode(s.dev, 0);
		else { rtlsdr_set_tuner_gain_mode(s.dev, 1); rtlsdr_set_tuner_gain(s.dev, g_i); }
		if (opt_string) rtlsdr_set_opt_string(s.dev, opt_string, verbosity);
		if (agc >= 0) rtlsdr_set_tuner_gain_mode(s.dev, agc);  // the string's agc=<tuner_gain_mode>, src/librtlsdr.c:3166-3171
		rtlsdr_set_freq_correction_ppb(s.dev, ppm * 1000);
		rtlsdr_set_offset_tuning(s.dev, c.offset_tuning);
		rtlsdr_set_center_freq(s.dev, s.capture_freq);
		if (rtlsdr_set_sample_rate(s.dev, capture_rate) < 0 && i == 0)
			fprintf(stderr, "WARNING: capture rate %u Hz is outside what an RTL2832 can do.\n", capture_rate);
		if (verbosity || i == 0 || capture_freqs[i] != capture_freqs[0])
			fprintf(stderr, "stream %d: device #%d, tuned to %u Hz.\n", i, dev_index + i, s.capture_freq);
	}
	if (!ret) {
		fprintf(stderr, "%d streams.\nOversampling input by: %ix.\nSampling at %u S/s.\nOutput at %u Hz.\n", n, c.downsample,
		        capture_rate, (unsigned)(c.rate_out2 > 0 ? c.rate_out2 : c.rate_out));
		if (verbosity)
			fprintf(stderr, "downsample_passes = %d, downsample = %d, deemph_a = %d, buffer = %u B, host queue = %d buffers per stream\n",
			        c.downsample_passes, c.downsample, c.deemph_a, c.block_len, m.depth);
		int r = rtlfm_gpu_create(&c, n, 0, &m.gpu);
		if (r < 0) {
			fprintf(stderr, "rtlfm_gpu_create: %s\n", rtlfm_gpu_strerror(r));
			ret = 2;
		}
		if (!ret && agc == 2) {
			std::vector<rtlsdr_dev_t *> devs;
			for (Source &s : m.src) devs.push_back(s.dev);
			r = rtlfm_gpu_set_option(m.gpu, "input_health", 1);
			if (r == 0) r = health_create(&m.hl, devs, c.max_blocks, verbosity);
			if (r < 0) {
				fprintf(stderr, "rtlfm_agc_create: %s\n", rtlfm_gpu_strerror(r));
				ret = 2;
			}
		}
		if (!ret && !rules.empty()) {
			r = rtlfm_gpu_set_option(m.gpu, "input_stats", 1);
			if (r == 0) r = rtlfm_monitor_create(n, rules.data(), &m.mon);
			if (r < 0) {
				fprintf(stderr, "rtlfm_monitor_create: %s\n", rtlfm_gpu_strerror(r));
				ret = 2;
			}
		}
		if (!ret && resume_file && (r = rtlfm_gpu_load(m.gpu, resume_file)) < 0) {
			fprintf(stderr, "-R %s: %s\n", resume_file, rtlfm_gpu_strerror(r));
			ret = 2;
		}
		if (!ret && c.squelch_level) {
			// -l: demod_thread_fn's rule on the device where the configuration has a gate (not behind a resampler)
			r = rtlfm_gpu_set_option(m.gpu, "conseq_squelch", conseq_squelch);
			if (r == 0) r = rtlfm_gpu_set_option(m.gpu, "squelch_gate", 1);
			m.use_gate = r == 0;
			if (r < 0 && (r != -ENOTSUP || !scan_lists.empty())) {
				fprintf(stderr, "squelch_gate: %s\n", rtlfm_gpu_strerror(r));
				ret = 2;
			}
		}
		if (!ret && !scan_lists.empty()) {
			r = rtlfm_scan_create(n, RTLFM_SCAN_DEFAULT_DUMP, c.max_blocks, &m.scan);
			for (int i = 0; i < n && r == 0; i++)
				r = rtlfm_scan_set_list(m.scan, i, scan_lists[(size_t)i].data(), (int)scan_lists[(size_t)i].size());
			if (r < 0) {
				fprintf(stderr, "rtlfm_scan_create: %s\n", rtlfm_gpu_strerror(r));
				ret = 2;
			}
		}
	}
	const size_t at = pattern.find("%d");
	for (int i = 0; i < n && !ret; i++) {
		Source &s = m.src[i];
		const std::string name = at == std::string::npos ? pattern : pattern.substr(0, at) + std::to_string(i) + pattern.substr(at + 2);
		s.file = fopen(name.c_str(), "wb");
		if (!s.file) { fprintf(stderr, "Failed to open %s\n", name.c_str()); ret = 1; break; }
		if (write_wav)
			rtlamd_wave_write_header(&s.wave, (unsigned)(c.rate_out2 > 0 ? c.rate_out2 : c.rate_out), s.user_freq, 16,
			                         c.mode == RTLFM_MODE_RAW ? 2 : 1, s.file);
		rtlsdr_reset_buffer(s.dev);
	}
	if (!ret) {
		std::thread t_out(output_thread_multi, &m), t_demod(demod_thread_multi, &m);
		std::vector<std::thread> t_dongle;
		for (Source &s : m.src) t_dongle.emplace_back(dongle_thread_multi, &s);
		for (std::thread &t : t_dongle) t.join();
		t_demod.join();
		t_out.join();
		uint64_t in = 0, out = 0, sq = 0;
		for (Source &s : m.src) {
			in += s.blocks_in;
			out += s.samples_out;
			sq += s.blocks_squelched;
		}
		fprintf(stderr, "%llu buffers in, %llu samples out, %llu buffers held back by the squelch%s\n", (unsigned long long)in,
		        (unsigned long long)out, (unsigned long long)sq, m.failed ? " (FAILED)" : "");
		if (verbosity)
			for (Source &s : m.src)
				fprintf(stderr, "stream %d: %llu buffers in, %llu samples out, %llu buffers held back by the squelch\n", s.index,
				        (unsigned long long)s.blocks_in, (unsigned long long)s.samples_out, (unsigned long long)s.blocks_squelched);
		if (m.mon) {
			fprintf(stderr, "%llu monitor events, %llu fired\n", (unsigned long long)m.events, (unsigned long long)m.fired);
			// the scan statistics of src/rtl_fm.c:2033-2040, one line per command-file line that reported a level
			for (int i = 0; i < n; i++) {
				rtlfm_monitor_stat st;
				if (rtlfm_monitor_stats(m.mon, i, &st) == 0 && st.count > 0)
					fprintf(stderr, "%u, %.1f, %.2f, %.1f\n", rules[(size_t)i].freq, st.min_level, st.sum_levels / st.count, st.max_level);
			}
		}
		if (m.hl.agc) health_report(&m.hl);
		if (m.scan)
			for (int i = 0; i < n; i++) {
				uint32_t f = 0;
				uint64_t hops = 0, held = 0;
				rtlfm_scan_freq(m.scan, i, &f, nullptr, &hops, nullptr, &held);
				fprintf(stderr, "stream %d: %llu hops, %llu buffers held, last on %u Hz\n", i, (unsigned long long)hops,
				        (unsigned long long)held, f + (wb_mode ? 16000u : 0u));
			}
		if (m.failed) ret = 3;
		if (!ret && keep_file) {
			// behind the last run: the sources that were in the batch to the end, beside the records the others left
			int r = keep_states(&m, m.live, nullptr);
			if (r == 0) r = rtlfm_snapshot_write(keep_file, &c, n, m.kept.data(), nullptr);
			if (r < 0) {
				fprintf(stderr, "-K %s: %s\n", keep_file, rtlfm_gpu_strerror(r));
				ret = 3;
			}
		}
	}
	if (m.scan) rtlfm_scan_destroy(m.scan);
	if (m.hl.agc) rtlfm_agc_destroy(m.hl.agc);
	for (pid_t pid : m.children) waitpid(pid, nullptr, 0);  // the triggered commands run in the background; none outlives the tool
	if (m.mon) rtlfm_monitor_destroy(m.mon);
	for (Source &s : m.src) {
		if (s.file) {
			if (write_wav) rtlamd_wave_finalize(&s.wave, s.file);
			fclose(s.file);
		}
		if (s.dev) rtlsdr_close(s.dev);
	}
	if (m.gpu) rtlfm_gpu_destroy(m.gpu);
	return ret;
}

// ---- -X: K channels per source, one handle of n x K streams over the library's source-indexed ring ------------------
//
// The device side is -N's: on_buffer_multi / dongle_thread_multi, a host queue per source.  The demod thread takes
// b = min(what every live queue holds, max_blocks) buffers from every live source and pushes them with the SOURCE's index
// (option source_ring); a short buffer - a file's last - is completed with bytes 127 to the full length, and a source
// that has ended is fed b buffers of bytes 127, so that every source has one length per buffer index and the handle's one
// sample counter holds for all.  The streams of an ended source write nothing more.  The run ends with the last source.
void demod_thread_channels(Multi *m)
{
	const int n = (int)m->src.size(), K = m->chan_per, S = n * K;
	const size_t stride = ((size_t)rtlfm_result_cap(&m->cfg) * m->cfg.max_blocks + 16 + 63) / 64 * 64;
	const uint32_t L = m->cfg.block_len;
	const std::vector<uint8_t> silence(L, 127);
	std::vector<int> who((size_t)S);
	for (int s = 0; s < S; s++) who[(size_t)s] = s;
	std::vector<char> ended((size_t)n, 0);
	for (;;) {
		int b = m->cfg.max_blocks, live = 0;
		{
			std::unique_lock<std::mutex> g(m->m);
			m->cv_work.wait(g, [&] {
				if (m->failed) return true;
				for (int i = 0; i < n; i++)
					if (!ended[(size_t)i] && m->src[(size_t)i].q.empty() && !m->src[(size_t)i].eof) return false;
				return true;
			});
			if (m->failed) break;
			for (int i = 0; i < n; i++) {
				Source &s = m->src[(size_t)i];
				if (!ended[(size_t)i] && s.q.empty()) ended[(size_t)i] = 1;  // an empty queue here means the source has ended
				if (ended[(size_t)i]) continue;
				live++;
				b = std::min(b, (int)s.q.size());
			}
			for (int i = 0; i < n; i++) {
				Source &s = m->src[(size_t)i];
				if (ended[(size_t)i]) continue;
				for (int j = 0; j < b; j++) {
					s.taken.push_back(std::move(s.q.front()));
					s.q.pop_front();
				}
				s.cv_room.notify_all();
			}
		}
		if (!live) break;
		int r = 0;
		for (int i = 0; i < n && r == 0; i++) {
			if (ended[(size_t)i]) {
				for (int j = 0; j < b && r == 0; j++) r = rtlfm_gpu_push(m->gpu, i, silence.data(), L);
				continue;
			}
			for (std::vector<uint8_t> &buf : m->src[(size_t)i].taken) {
				if (buf.size() < L) buf.resize(L, 127);  // the source's short last buffer, completed
				if ((r = rtlfm_gpu_push(m->gpu, i, buf.data(), L)) < 0) break;
			}
		}
		int ran = 0;
		if (r == 0) r = rtlfm_gpu_run_begin(m->gpu, &ran);
		if (r == 0 && ran != b) r = -EPROTO;
		if (r == 0) r = rtlfm_gpu_run_end(m->gpu);
		RunOut o;
		o.stride = stride;
		o.pcm.resize((size_t)S * stride);
		o.lens.resize((size_t)S);
		o.who = who;
		if (r == 0) r = rtlfm_gpu_fetch_all(m->gpu, o.pcm.data(), stride, o.lens.data());
		if (r < 0) {
			std::lock_guard<std::mutex> g(m->m);
			fail_multi(m, "rtlfm_gpu_push/run/fetch_all", r);
			break;
		}
		for (int s = 0; s < S; s++)
			if (ended[(size_t)(s / K)]) o.lens[(size_t)s] = 0;
		if (m->print_levels)
			for (int s = 0; s < S; s++)
				if (!ended[(size_t)(s / K)]) levels_multi(m, m->chan[(size_t)s], s);
		if (m->cfg.squelch_level) {
			// demod_thread's squelch rule per stream, as demod_thread_multi applies it without the device gate (max_blocks is 1)
			m->states.resize((size_t)S);
			int got = 0;
			bool clamped = false;
			if (rtlfm_gpu_state_get_all(m->gpu, m->states.data(), S, &got) == 0) {
				for (int s = 0; s < S; s++) {
					rtlfm_stream_state &st = m->states[(size_t)s];
					if (st.squelch_hits <= m->conseq_squelch) continue;
					clamped |= st.squelch_hits != m->conseq_squelch + 1;
					st.squelch_hits = m->conseq_squelch + 1;
					if (!ended[(size_t)(s / K)]) m->chan[(size_t)s].blocks_squelched++;
					o.lens[(size_t)s] = 0;
				}
				if (clamped) rtlfm_gpu_state_set_all(m->gpu, m->states.data(), S);
			}
		}
		std::lock_guard<std::mutex> g(m->m);
		for (Source &s : m->src) {
			for (std::vector<uint8_t> &buf : s.taken) s.spare.push_back(std::move(buf));
			s.taken.clear();
		}
		m->out_q.push_back(std::move(o));
		m->cv_out.notify_one();
	}
	std::lock_guard<std::mutex> g(m->m);
	m->out_done = true;
	m->cv_out.notify_all();
}

// everything after option parsing for -X (main has refused what -X does not allow): freqs[i] = source i's -f as given,
// chan_freqs[i] = its K channel frequencies, each within capture_rate / 2 of freqs[i]
int run_channels(const rtlfm_cfg &planned, int n, int dev_index, const std::vector<uint32_t> &freqs,
                 const std::vector<std::vector<uint32_t>> &chan_freqs, uint32_t capture_rate, int gain, int ppm,
                 const std::string &pattern, bool write_wav, int verbosity, int conseq_squelch, int print_levels,
                 const char *opt_string, int agc, int ntaps)
{
	Multi m;
	m.cfg = planned;
	rtlfm_cfg &c = m.cfg;
	const int K = (int)chan_freqs[0].size(), S = n * K;
	m.chan_per = K;
	m.depth = 2 * c.max_blocks;
	m.verbosity = verbosity;
	m.conseq_squelch = conseq_squelch;
	m.print_levels = print_levels;
	m.src = std::vector<Source>((size_t)n);
	m.chan = std::vector<Source>((size_t)S);
	const uint32_t count = rtlsdr_get_device_count();
	if (count == 0) { fprintf(stderr, "No supported devices found (set RTLSDR_FILE or RTLSDR_FILE_LIST).\n"); return 1; }
	if ((uint64_t)dev_index + (uint64_t)n > count) {
		fprintf(stderr, "-d %d with %d sources needs devices %d .. %d, and there are %u.\n", dev_index, n, dev_index, dev_index + n - 1, count);
		return 1;
	}
	int ret = 0;
	for (int i = 0; i < n && !ret; i++) {
		Source &s = m.src[(size_t)i];
		s.index = i;
		s.m = &m;
		s.user_freq = s.capture_freq = freqs[(size_t)i];  // as given: the mixers take the rotation's place
		if (rtlsdr_open(&s.dev, (uint32_t)(dev_index + i)) < 0) {
			fprintf(stderr, "Failed to open rtlsdr device #%d.\n", dev_index + i);
			ret = 1;
			break;
		}
		if (gain == -100) rtlsdr_set_tuner_gain_mode(s.dev, 0);
		else { rtlsdr_set_tuner_gain_mode(s.dev, 1); rtlsdr_set_tuner_gain(s.dev, gain); }
		if (opt_string) rtlsdr_set_opt_string(s.dev, opt_string, verbosity);
		if (agc >= 0) rtlsdr_set_tuner_gain_mode(s.dev, agc);
		rtlsdr_set_freq_correction_ppb(s.dev, ppm * 1000);
		rtlsdr_set_offset_tuning(s.dev, c.offset_tuning);
		rtlsdr_set_center_freq(s.dev, s.capture_freq);
		if (rtlsdr_set_sample_rate(s.dev, capture_rate) < 0 && i == 0)
			fprintf(stderr, "WARNING: capture rate %u Hz is outside what an RTL2832 can do.\n", capture_rate);
		fprintf(stderr, "source %d: device #%d, tuned to %u Hz, streams %d .. %d.\n", i, dev_index + i, s.capture_freq, i * K, i * K + K - 1);
	}
	if (!ret) {
		fprintf(stderr, "%d sources x %d channels = %d streams.\nOversampling input by: %ix.\nSampling at %u S/s.\nOutput at %u Hz.\n", n, K, S,
		        c.downsample, capture_rate, (unsigned)(c.rate_out2 > 0 ? c.rate_out2 : c.rate_out));
		std::vector<uint32_t> steps((size_t)S);
		for (int s = 0; s < S; s++) {
			const uint32_t cf = chan_freqs[(size_t)(s / K)][(size_t)(s % K)];
			steps[(size_t)s] = rtlfm_channel_step((int32_t)((int64_t)cf - (int64_t)freqs[(size_t)(s / K)]), capture_rate);
			if (verbosity) fprintf(stderr, "stream %d: source %d, %u Hz, step %u\n", s, s / K, cf, steps[(size_t)s]);
		}
		const char *what = "rtlfm_gpu_create";
		int r = rtlfm_gpu_create(&c, S, 0, &m.gpu);
		if (r == 0) { what = "option source_ring"; r = rtlfm_gpu_set_option(m.gpu, "source_ring", 1); }
		if (r == 0) { what = "rtlfm_gpu_set_channels"; r = rtlfm_gpu_set_channels(m.gpu, K, steps.data()); }
		if (r == 0 && ntaps > 0) {
			// the cutoff the benchmarks use: 0.4 of the output rate, in cycles per capture sample
			std::vector<int16_t> taps((size_t)ntaps);
			int shift = 0;
			what = "rtlfm_channel_lowpass";
			// (-ERANGE: fewer taps than the gain D needs at shift 14 - a tap beyond an int16, a short filter at a large D.  The
			// same filter at half the scale and one bit less shift has the same DC gain, as long as D stays whole.)
			int gain = c.downsample, less = 0;
			r = rtlfm_channel_lowpass(ntaps, 0.4 / c.downsample, gain, taps.data(), &shift);
			while (r == -ERANGE && gain % 2 == 0 && less < 14) {
				gain /= 2;
				less++;
				r = rtlfm_channel_lowpass(ntaps, 0.4 / c.downsample, gain, taps.data(), &shift);
			}
			shift -= less;
			if (r == 0 && (less || verbosity)) fprintf(stderr, "-x %d: gain %d at shift %d\n", ntaps, gain, shift);
			if (r == 0) { what = "rtlfm_gpu_set_channel_filter"; r = rtlfm_gpu_set_channel_filter(m.gpu, taps.data(), ntaps, shift); }
		}
		if (r < 0) {
			fprintf(stderr, "%s: %s\n", what, rtlfm_gpu_strerror(r));
			ret = 2;
		}
	}
	const size_t at = pattern.find("%d");
	for (int s = 0; s < S && !ret; s++) {
		Source &ch = m.chan[(size_t)s];
		ch.index = s;
		ch.user_freq = chan_freqs[(size_t)(s / K)][(size_t)(s % K)];
		const std::string name = at == std::string::npos ? pattern : pattern.substr(0, at) + std::to_string(s) + pattern.substr(at + 2);
		ch.file = fopen(name.c_str(), "wb");
		if (!ch.file) { fprintf(stderr, "Failed to open %s\n", name.c_str()); ret = 1; break; }
		if (write_wav)
			rtlamd_wave_write_header(&ch.wave, (unsigned)(c.rate_out2 > 0 ? c.rate_out2 : c.rate_out), ch.user_freq, 16,
			                         c.mode == RTLFM_MODE_RAW ? 2 : 1, ch.file);
	}
	if (!ret) {
		for (Source &s : m.src) rtlsdr_reset_buffer(s.dev);
		std::thread t_out(output_thread_multi, &m), t_demod(demod_thread_channels, &m);
		std::vector<std::thread> t_dongle;
		for (Source &s : m.src) t_dongle.emplace_back(dongle_thread_multi, &s);
		for (std::thread &t : t_dongle) t.join();
		t_demod.join();
		t_out.join();
		uint64_t in = 0, out = 0, sq = 0;
		for (Source &s : m.src) in += s.blocks_in;
		for (Source &ch : m.chan) {
			out += ch.samples_out;
			sq += ch.blocks_squelched;
		}
		fprintf(stderr, "%llu buffers in, %llu samples out, %llu buffers held back by the squelch%s\n", (unsigned long long)in,
		        (unsigned long long)out, (unsigned long long)sq, m.failed ? " (FAILED)" : "");
		if (verbosity)
			for (Source &ch : m.chan)
				fprintf(stderr, "stream %d: %llu samples out, %llu buffers held back by the squelch\n", ch.index,
				        (unsigned long long)ch.samples_out, (unsigned long long)ch.blocks_squelched);
		if (m.failed) ret = 3;
	}
	for (Source &ch : m.chan)
		if (ch.file) {
			if (write_wav) rtlamd_wave_finalize(&ch.wave, ch.file);
			fclose(ch.file);
		}
	for (Source &s : m.src)
		if (s.dev) rtlsdr_close(s.dev);
	if (m.gpu) rtlfm_gpu_destroy(m.gpu);
	return ret;
}

// -R: the file against what the command line plans, before a device is opened: 0, or the exit status (2) behind the
// library's text.  The handle checks the same again when it loads the file (rtlfm_gpu_load).
int check_resume(const char *path, const rtlfm_cfg &planned, int nstreams)
{
	rtlfm_cfg saved;
	int n = 0;
	int r = rtlfm_snapshot_info(path, &saved, &n);
	if (r == 0 && n != nstreams) r = -ERANGE;
	if (r == 0) {
		saved.max_blocks = planned.max_blocks;        // how much a run takes and what it reports, not what a stream carries
		saved.report_levels = planned.report_levels;
		if (memcmp(&saved, &planned, sizeof(saved)) != 0) r = -EMEDIUMTYPE;
	}
	if (r == 0) return 0;
	fprintf(stderr, "-R %s: %s\n", path, rtlfm_gpu_strerror(r));
	return 2;
}

void usage()
{
	fprintf(stderr,
	        "rtl_fm_hip, rtl_fm's demodulator on an AMD GPU (one stream, or -N streams in one batch)\n"
	        "Use:\trtl_fm_hip -f freq [-options] [filename]   (input: RTLSDR_FILE=<raw u8 IQ file>\n"
	        "\t                                                or RTLSDR_FILE_LIST=<file with one source per line>)\n"
	        "\t-f frequency_to_tune_to [Hz]  (with -N n: once for every device, or n times, one per device)\n"
	        "\t[-N n  demodulate devices d .. d+n-1 (d = -d) in one batch; filename must hold one %%d (stream index),\n"
	        "\t       not '-'; a source that ends leaves the batch, the slowest source sets the pace; not with -Z]\n"
	        "\t[-C command_file  with -N n: measurement line i of the file (freq, gain, in|out|lt|gt, level dB, tolerance dB,\n"
	        "\t       #meas, #blocks, command, args) is watched by source i - the file must hold n such lines; adc / adcmax /\n"
	        "\t       adcrms lines add the ADC statistics of the raw bytes; sets -M raw; -v prints every event]\n"
	        "\t[-S scan_file  scanning: line i of the file is the frequency list of source i (-N n, or one source): frequencies\n"
	        "\t       and a:b:step ranges; needs -l; a source whose squelch holds a buffer hops to its next frequency; not with -C]\n"
	        "\t[-X channel_file  channels: line i of the file is the list of channel frequencies of source i (-N n, or one source), in\n"
	        "\t       -S's grammar, the same number K on every line; source i's centre frequency is its -f as given and its K channels are mixed\n"
	        "\t       down on the GPU; stream s = channel s %% K of source s / K writes the file with %%d = s; not with -S -C -K -R -Z,\n"
	        "\t       -O agc=2 or -E rdc]\n"
	        "\t[-x ntaps  with -X: a windowed-sinc channel filter of ntaps taps (cutoff 0.4 of the output rate) in the boxcar's place; not with -F]\n"
	        "\t[-K file  keep: write every stream's carried filter state to file at exit (with -N n: n records, in source order)]\n"
	        "\t[-R file  resume: load such a file before the first buffer - it must hold as many records as there are sources and\n"
	        "\t       come from the same -M / -s / -r / -F / -A / -E / -l / -W ... plan, else exit 2; the output continues as if the tool had\n"
	        "\t       never stopped.  -K / -R not with -S, -C or -O agc=2: those engines carry state the file does not hold]\n"
	        "\t[-M modulation (default: fm)]  fm, wbfm, raw, am, usb, lsb\n"
	        "\t[-s sample_rate (default: 24k)]  [-r resample_rate (default: none / same as -s)]\n"
	        "\t[-m minimum_capture_rate Hz (default: 1m)]\n"
	        "\t[-F fir_size (default: off)]  enables the fifth-order low pass; 0 or 9 (9 = droop compensation)\n"
	        "\t[-A std/fast/lut choose atan math (default: std)]\n"
	        "\t[-E enable_option]  edge, dc, rdc, deemp, offset\n"
	        "\t[-c de-emphasis_time_constant in us: us (75), eu (50) or a number]\n"
	        "\t[-o oversampling (default: 1)]  [-l squelch_level]  [-t squelch_delay (default: 10)]  [-q rdc_block_const]\n"
	        "\t[-L N  prints levels every N calculations (with -N: per stream, as 'stream i: ...')]\n"
	        "\t[-W length of one buffer in units of 512 bytes (default: 32 = 16384 B)]\n"
	        "\t[-H write a wave header with the auxi chunk SDR programs read the frequency from]  [-v verbose]\n"
	        "\t[-Z zero-copy: the device layer reads straight into the GPU layer's pinned staging ring]\n"
	        "\t[-d device_index] [-g gain] [-p ppm]  accepted and passed to the device layer\n"
	        "\t[-O driver options separated with ':', passed to the device layer; agc=0|1|2 is read here as well:\n"
	        "\t       agc=2 = software AGC for every source from the GPU's records of the raw bytes; -v prints every change]\n"
	        "\tfilename ('-' means stdout)\n");
	exit(1);
}

}  // namespace

int main(int argc, char **argv)
{
	App a;
	rtlfm_cfg_default(&a.cfg);
	rtlfm_cfg &c = a.cfg;
	int rate_in = 24000, min_capture = 1000000, time_constant = 75;
	int fifth = 0, edge = 0, dev_index = 0, gain = -100, ppm = 0;
	uint32_t freq = 0;
	std::vector<uint32_t> freqs;  // every -f, in order (-N)
	int nstreams = 1;
	bool have_freq = false, write_wav = false, wb_mode = false;
	int conseq_squelch = 10;  // demod_init(), src/rtl_fm.c:1613
	const char *cmd_file = nullptr, *opt_string = nullptr, *scan_file = nullptr, *keep_file = nullptr, *resume_file = nullptr;
	const char *chan_file = nullptr;  // -X
	int chan_taps = -1;               // -x; -1: not given
	int agc = -1;  // -O agc=<n>; -1: not given
	c.rate_out = 24000;
	c.max_blocks = 8;
	int opt;
	while ((opt = getopt(argc, argv, "d:f:g:s:l:o:t:r:p:E:F:A:M:hm:L:q:c:W:HvZN:C:O:S:K:R:X:x:")) != -1) {
		switch (opt) {
		case 'd': dev_index = atoi(optarg); break;
		case 'f': freq = (uint32_t)atofs(optarg); freqs.push_back(freq); have_freq = true; break;
		case 'N': nstreams = atoi(optarg); break;
		case 'C': cmd_file = optarg; break;
		case 'S': scan_file = optarg; break;
		case 'K': keep_file = optarg; break;
		case 'R': resume_file = optarg; break;
		case 'X': chan_file = optarg; break;
		case 'x': chan_taps = atoi(optarg); break;
		case 'O':
			opt_string = optarg;
			agc = opt_string_agc(optarg);
			if (agc == -2) {
				fprintf(stderr, "-O %s: agc= takes 0 (hardware AGC), 1 (manual) or 2 (software AGC).\n", optarg);
				return 1;
			}
			break;
		case 'g': gain = (int)(atof(optarg) * 10); break;
		case 'p': ppm = (int)atof(optarg); break;
		case 'm': min_capture = (int)atofs(optarg); break;
		case 'l': c.squelch_level = (int)atof(optarg); break;
		case 'L': a.print_levels = (int)atof(optarg); break;  // src/rtl_fm.c:1757-1759
		case 't':  // src/rtl_fm.c:1774-1781 (a negative value also asks to terminate on squelch: not restated)
			conseq_squelch = (int)atof(optarg);
			if (conseq_squelch < 0) conseq_squelch = -conseq_squelch;
			break;
		case 's': rate_in = (int)atofs(optarg); c.rate_out = rate_in; break;
		case 'r': c.rate_out2 = (int)atofs(optarg); break;
		case 'o': c.post_downsample = (int)atof(optarg); break;
		case 'q': c.rdc_block_const = atoi(optarg); break;
		case 'E':
			if (!strcmp(optarg, "edge")) edge = 1;
			if (!strcmp(optarg, "dc") || !strcmp(optarg, "adc")) c.dc_block_audio = 1;
			if (!strcmp(optarg, "rdc")) c.dc_block_raw = 1;
			if (!strcmp(optarg, "deemp")) c.deemph = 1;
			if (!strcmp(optarg, "offset")) c.offset_tuning = 1;
			break;
		case 'F': fifth = 1; c.comp_fir_size = atoi(optarg); break;
		case 'A':
			if (!strcmp(optarg, "std")) c.custom_atan = RTLFM_ATAN_STD;
			if (!strcmp(optarg, "fast")) c.custom_atan = RTLFM_ATAN_FAST;
			if (!strcmp(optarg, "lut")) c.custom_atan = RTLFM_ATAN_LUT;
			break;
		case 'M':
			if (!strcmp(optarg, "fm") || !strcmp(optarg, "nbfm") || !strcmp(optarg, "nfm")) c.mode = RTLFM_MODE_FM;
			if (!strcmp(optarg, "raw") || !strcmp(optarg, "iq")) c.mode = RTLFM_MODE_RAW;
			if (!strcmp(optarg, "am")) c.mode = RTLFM_MODE_AM;
			if (!strcmp(optarg, "usb")) c.mode = RTLFM_MODE_USB;
			if (!strcmp(optarg, "lsb")) c.mode = RTLFM_MODE_LSB;
			if (!strcmp(optarg, "wbfm") || !strcmp(optarg, "wfm")) {
				// the preset of src/rtl_fm.c:1831-1840
				c.mode = RTLFM_MODE_FM;
				rate_in = 170000; c.rate_out = 170000; c.rate_out2 = 32000;
				c.custom_atan = RTLFM_ATAN_FAST;
				c.deemph = 1;
				c.squelch_level = 0;
				wb_mode = true;
			}
			break;
		case 'c':
			if (!strcmp(optarg, "us")) time_constant = 75;
			else if (!strcmp(optarg, "eu")) time_constant = 50;
			else time_constant = (int)atof(optarg);
			break;
		case 'W': {
			long v = 512L * atoi(optarg);
			if (v > (long)RTLFM_MAX_BLOCK_LEN) v = RTLFM_MAX_BLOCK_LEN;  // src/rtl_fm.c:1869-1873
			c.block_len = (uint32_t)v;
			break;
		}
		case 'H': write_wav = true; break;
		case 'Z': a.zero_copy = true; break;
		case 'v': a.verbosity++; break;
		default: usage();
		}
	}
	if (chan_taps != -1 && !chan_file) {
		fprintf(stderr, "-x (taps of the channel filter) needs -X (the channel file): the filter acts on channels only.\n");
		return 1;
	}
	if (chan_file) {
		// everything -X refuses for what it is combined with is refused here, before a device is opened or a handle created:
		// each of these needs what the library refuses while channels are on (include/rtlfm_hip.h, rtlfm_gpu_set_channels)
		const char *with = nullptr, *why = nullptr;
		if (scan_file) { with = "-S (scan lists)"; why = "a hop needs the hop mute and the squelch gate, which read per-stream input rows"; }
		else if (cmd_file) { with = "-C (command file)"; why = "the monitor needs the option input_stats, which reads per-stream input rows"; }
		else if (keep_file) { with = "-K (keep)"; why = "a snapshot does not hold the channels' sample counter"; }
		else if (resume_file) { with = "-R (resume)"; why = "a snapshot does not hold the channels' sample counter"; }
		else if (a.zero_copy) { with = "-Z (zero-copy)"; why = "the ring is filled from the sources' host queues, in lockstep"; }
		else if (agc == 2) { with = "-O agc=2 (software AGC)"; why = "it needs the option input_health, which reads per-stream input rows"; }
		else if (c.dc_block_raw) { with = "-E rdc (raw DC block)"; why = "it rides on the rotation's kernel, whose place the mixers take"; }
		else if (chan_taps != -1 && fifth) { with = "-x (channel filter) with -F (fifth-order low pass)"; why = "the channel filter stands in the boxcar's place, and -F leaves no boxcar"; }
		if (with) {
			fprintf(stderr, "-X (channel file) does not go with %s: %s.\n", with, why);
			return 1;
		}
		if (chan_taps != -1 && (chan_taps < 1 || chan_taps > RTLFM_CHANNEL_MAX_TAPS)) {
			fprintf(stderr, "-x %d with -X: the channel filter takes 1 .. %d taps.\n", chan_taps, RTLFM_CHANNEL_MAX_TAPS);
			return 1;
		}
	}
	if ((keep_file || resume_file) && (scan_file || cmd_file || agc == 2)) {
		// before a device is opened: the hop engine, the monitor and the software AGC carry state of their own
		fprintf(stderr, "-K / -R (keep / resume the carried state) do not go with -S, -C or -O agc=2: those engines carry state of "
		                "their own that the snapshot does not hold.\n");
		return 1;
	}
	std::vector<std::vector<uint32_t>> scan_lists;
	if (scan_file) {
		// everything -S refuses is refused here, before a device is opened
		if (nstreams < 1) { fprintf(stderr, "-N wants a number of streams >= 1.\n"); usage(); }
		if (cmd_file) { fprintf(stderr, "-S (scan lists) and -C (command file) exclude each other.\n"); usage(); }
		if (!c.squelch_level) { fprintf(stderr, "Please specify a squelch level.  Required for scanning multiple frequencies.\n"); return 1; }  // src/rtl_fm.c:1693
		FILE *sf = fopen(scan_file, "r");
		if (!sf) { fprintf(stderr, "-S %s: cannot open the scan file\n", scan_file); usage(); }
		char line[65536];
		int lineno = 0;
		while (fgets(line, sizeof(line), sf)) {
			lineno++;
			const char *t = line;
			while (*t == ' ' || *t == '\t') t++;
			if (*t == '#' || *t == '\n' || *t == '\r' || !*t) continue;
			int nf = 0;
			int pr = rtlfm_scan_parse_list(t, nullptr, 0, &nf);
			std::vector<uint32_t> fl((size_t)(nf > 0 ? nf : 0));
			if (pr == -ENOBUFS) pr = rtlfm_scan_parse_list(t, fl.data(), nf, &nf);
			if (pr < 0) { fclose(sf); fprintf(stderr, "-S %s: line %d is no frequency list\n", scan_file, lineno); usage(); }
			scan_lists.push_back(std::move(fl));
		}
		fclose(sf);
		if ((int)scan_lists.size() != nstreams) {
			fprintf(stderr, "-S %s holds %zu lists, -N %d needs exactly %d: line i of the file is the list of source i.\n", scan_file,
			        scan_lists.size(), nstreams, nstreams);
			usage();
		}
		if (!have_freq) {  // a source starts on its list's first entry
			for (const std::vector<uint32_t> &fl : scan_lists) freqs.push_back(fl[0]);
			freq = freqs[0];
			have_freq = true;
		}
	}
	std::vector<rtlfm_monitor_rule> rules;
	if (cmd_file) {
		// src/rtl_fm.c:1738-1741: the command file implies -M raw; here its lines are the -N sources, in order
		if (nstreams < 1) { fprintf(stderr, "-N wants a number of streams >= 1.\n"); usage(); }
		rules.resize((size_t)nstreams);
		int found = 0;
		const int pr = rtlfm_monitor_parse_file(cmd_file, rules.data(), nstreams, &found, nullptr, nullptr);
		if (pr < 0 && pr != -ENOBUFS) {
			fprintf(stderr, "-C %s: %s\n", cmd_file, pr == -ENOENT ? "cannot open the command file" : "no valid measurement line");
			usage();
		}
		if (found != nstreams) {
			fprintf(stderr, "-C %s holds %d measurement lines, -N %d needs exactly %d: line i of the file is watched by source i.\n",
			        cmd_file, found, nstreams, nstreams);
			usage();
		}
		c.mode = RTLFM_MODE_RAW;
		c.report_levels = 1;
		c.max_blocks = 1;  // as -L: one buffer per run, so that a source's short last buffer keeps its place among the levels
		freqs.clear();
		for (const rtlfm_monitor_rule &r : rules) freqs.push_back(r.freq);
		freq = freqs[0];
		have_freq = true;
		wb_mode = false;
	}
	if (!have_freq) { fprintf(stderr, "Please specify a frequency.\n"); return 1; }
	if (wb_mode) freq += 16000;  // controller_thread_fn(), src/rtl_fm.c:1455-1460: "wbfm: adding 16000 Hz to every input frequency"
	a.conseq_squelch = conseq_squelch;
	if (c.squelch_level) c.max_blocks = 1;  // the squelch rule below is the reference's per-buffer rule
	if (a.print_levels > 0) { c.report_levels = 1; c.max_blocks = 1; }
	a.user_freq = freq;  // dongle.userFreq, src/rtl_fm.c:1440
	rate_in *= c.post_downsample;  // src/rtl_fm.c:1886
	const char *filename = optind < argc ? argv[optind] : "-";

	if (nstreams < 1) { fprintf(stderr, "-N wants a number of streams >= 1.\n"); usage(); }
	if (chan_file) {
		// -X: the file, the names and the plan, all before a device is opened or a GPU handle created
		std::vector<std::vector<uint32_t>> chan_freqs;
		std::vector<int> chan_lineno;
		FILE *xf = fopen(chan_file, "r");
		if (!xf) { fprintf(stderr, "-X %s: cannot open the channel file\n", chan_file); return 1; }
		char line[65536];
		int lineno = 0;
		while (fgets(line, sizeof(line), xf)) {
			lineno++;
			const char *t = line;
			while (*t == ' ' || *t == '\t') t++;
			if (*t == '#' || *t == '\n' || *t == '\r' || !*t) continue;
			int nf = 0;
			int pr = rtlfm_scan_parse_list(t, nullptr, 0, &nf);
			std::vector<uint32_t> fl((size_t)(nf > 0 ? nf : 0));
			if (pr == -ENOBUFS) pr = rtlfm_scan_parse_list(t, fl.data(), nf, &nf);
			if (pr < 0) { fclose(xf); fprintf(stderr, "-X %s: line %d is no frequency list\n", chan_file, lineno); return 1; }
			chan_freqs.push_back(std::move(fl));
			chan_lineno.push_back(lineno);
		}
		fclose(xf);
		if ((int)chan_freqs.size() != nstreams) {
			fprintf(stderr, "-X %s holds %zu lists, -N %d needs exactly %d: line i of the file is the channel list of source i.\n", chan_file,
			        chan_freqs.size(), nstreams, nstreams);
			return 1;
		}
		for (size_t i = 1; i < chan_freqs.size(); i++)
			if (chan_freqs[i].size() != chan_freqs[0].size()) {
				fprintf(stderr, "-X %s: line %d stands for %zu channels and line %d for %zu; every source needs the same number of channels "
				        "(-N sources share one handle).\n", chan_file, chan_lineno[i], chan_freqs[i].size(), chan_lineno[0], chan_freqs[0].size());
				return 1;
			}
		const size_t total = chan_freqs.size() * chan_freqs[0].size();
		if (freqs.size() != 1 && freqs.size() != (size_t)nstreams) {
			fprintf(stderr, "-X with -N %d: give -f once (every source) or %d times (one per source), not %zu times.\n", nstreams, nstreams,
			        freqs.size());
			return 1;
		}
		if (freqs.size() == 1) freqs.assign((size_t)nstreams, freqs[0]);
		const std::string pattern(filename);
		const size_t at = pattern.find("%d");
		if (total > 1 && (at == std::string::npos || pattern.find("%d", at + 2) != std::string::npos)) {
			fprintf(stderr, "-X with %zu streams: the filename must hold exactly one %%d (the stream index), e.g. out_%%d.raw.\n", total);
			return 1;
		}
		if (pattern == "-" || (total == 1 && at != std::string::npos && pattern.find("%d", at + 2) != std::string::npos)) {
			fprintf(stderr, "-X: no stdout and at most one %%d; name the files, e.g. out_%%d.raw.\n");
			return 1;
		}
		if (c.deemph) c.deemph_a = rtlfm_deemph_a(c.rate_out, time_constant);
		// one plan for all sources, as under -N; a source's capture frequency is its -f as given (no capture_rate / 4 offset,
		// no +16 kHz under -M wbfm)
		rtlfm_cfg planned = c;
		uint32_t capture_rate = 0;
		for (int i = 0; i < nstreams; i++) {
			rtlfm_cfg ci = c;
			uint32_t cr = 0;
			rtlfm_optimal_settings(&ci, freqs[(size_t)i], rate_in, min_capture, fifth, edge, nullptr, &cr);
			if (i == 0) {
				planned = ci;
				capture_rate = cr;
			} else if (memcmp(&ci, &planned, sizeof(ci)) != 0 || cr != capture_rate) {
				fprintf(stderr, "-X: the rate plan for %u Hz differs from the one for %u Hz; one handle needs one plan.\n", freqs[(size_t)i], freqs[0]);
				return 1;
			}
		}
		for (size_t i = 0; i < chan_freqs.size(); i++)
			for (size_t k = 0; k < chan_freqs[i].size(); k++) {
				const int64_t off = (int64_t)chan_freqs[i][k] - (int64_t)freqs[i];
				if (2 * (off < 0 ? -off : off) > (int64_t)capture_rate) {
					fprintf(stderr, "-X %s: line %d, entry %zu: %u Hz is further than capture_rate / 2 = %u Hz from the -f of source %zu, %u Hz.\n",
					        chan_file, chan_lineno[i], k + 1, chan_freqs[i][k], capture_rate / 2, i, freqs[i]);
					return 1;
				}
			}
		return run_channels(planned, nstreams, dev_index, freqs, chan_freqs, capture_rate, gain, ppm, pattern, write_wav, a.verbosity,
		                    conseq_squelch, a.print_levels, opt_string, agc, chan_taps > 0 ? chan_taps : 0);
	}
	int r_resume = 0;
	if (nstreams > 1 || cmd_file || scan_file) {
		// everything -N refuses is refused here, before a device is opened or a GPU handle created
		const std::string pattern(filename);
		const size_t at = pattern.find("%d");
		if (freqs.size() != 1 && freqs.size() != (size_t)nstreams) {
			fprintf(stderr, "-N %d: give -f once (every device) or %d times (one per device), not %zu times.\n", nstreams,
			        nstreams, freqs.size());
			usage();
		}
		if (pattern == "-") { fprintf(stderr, "-N %d: no stdout; name the files, e.g. out_%%d.raw.\n", nstreams); usage(); }
		if (nstreams == 1 && scan_file && at == std::string::npos) {
			// one source: the name as it is
		} else if (at == std::string::npos || pattern.find("%d", at + 2) != std::string::npos) {
			fprintf(stderr, "-N %d: the filename must hold exactly one %%d (the stream index), e.g. out_%%d.raw.\n", nstreams);
			usage();
		}
		if (a.zero_copy) {
			// -Z writes a device's buffer straight into the ring, but with -N the ring is filled from the host
			// queues (run_multi): there is no slot a device could own
			fprintf(stderr, "-Z (zero-copy) works with one stream only, not with -N %d.\n", nstreams);
			usage();
		}
		if (freqs.size() == 1) freqs.assign((size_t)nstreams, freqs[0]);
		if (wb_mode)
			for (uint32_t &f : freqs) f += 16000;  // the -M wbfm rule above, for every device
		if (c.deemph) c.deemph_a = rtlfm_deemph_a(c.rate_out, time_constant);
		// one plan for all streams: optimal_settings() must not depend on the frequency for what this CLI accepts
		rtlfm_cfg planned = c;
		std::vector<uint32_t> capture_freqs((size_t)nstreams);
		uint32_t capture_rate = 0;
		for (int i = 0; i < nstreams; i++) {
			rtlfm_cfg ci = c;
			uint32_t cr = 0;
			rtlfm_optimal_settings(&ci, freqs[i], rate_in, min_capture, fifth, edge, &capture_freqs[i], &cr);
			if (i == 0) {
				planned = ci;
				capture_rate = cr;
			} else if (memcmp(&ci, &planned, sizeof(ci)) != 0 || cr != capture_rate) {
				fprintf(stderr, "-N: the rate plan for %u Hz differs from the one for %u Hz; one handle needs one plan.\n",
				        freqs[i], freqs[0]);
				return 1;
			}
		}
		if (resume_file && (r_resume = check_resume(resume_file, planned, nstreams)) != 0) return r_resume;
		return run_multi(planned, nstreams, dev_index, freqs, capture_freqs, capture_rate, gain, ppm, pattern, write_wav,
		                 a.verbosity, conseq_squelch, a.print_levels, rules, opt_string, agc, scan_lists, wb_mode, rate_in, min_capture,
		                 fifth, edge, keep_file, resume_file);
	}

	if (resume_file) {
		// the plan the handle will be created with, before a device is opened (optimal_settings() and deemph_a are host arithmetic)
		rtlfm_cfg planned = c;
		if (planned.deemph) planned.deemph_a = rtlfm_deemph_a(planned.rate_out, time_constant);
		rtlfm_optimal_settings(&planned, freq, rate_in, min_capture, fifth, edge, nullptr, nullptr);
		if ((r_resume = check_resume(resume_file, planned, 1)) != 0) return r_resume;
	}
	if (rtlsdr_get_device_count() == 0) { fprintf(stderr, "No supported devices found (set RTLSDR_FILE).\n"); return 1; }
	if (rtlsdr_open(&a.dev, (uint32_t)dev_index) < 0) { fprintf(stderr, "Failed to open rtlsdr device #%d.\n", dev_index); return 1; }
	if (c.deemph) c.deemph_a = rtlfm_deemph_a(c.rate_out, time_constant);
	uint32_t capture_freq = 0, capture_rate = 0;
	rtlfm_optimal_settings(&c, freq, rate_in, min_capture, fifth, edge, &capture_freq, &capture_rate);
	if (gain == -100) rtlsdr_set_tuner_gain_mode(a.dev, 0);
	else { rtlsdr_set_tuner_gain_mode(a.dev, 1); rtlsdr_set_tuner_gain(a.dev, gain); }
	if (opt_string) rtlsdr_set_opt_string(a.dev, opt_string, a.verbosity);
	if (agc >= 0) rtlsdr_set_tuner_gain_mode(a.dev, agc);  // the string's agc=<tuner_gain_mode>, src/librtlsdr.c:3166-3171
	rtlsdr_set_freq_correction_ppb(a.dev, ppm * 1000);
	rtlsdr_set_offset_tuning(a.dev, c.offset_tuning);
	rtlsdr_set_center_freq(a.dev, capture_freq);
	if (rtlsdr_set_sample_rate(a.dev, capture_rate) < 0)
		fprintf(stderr, "WARNING: capture rate %u Hz is outside what an RTL2832 can do.\n", capture_rate);
	fprintf(stderr, "Tuned to %u Hz.\nOversampling input by: %ix.\nSampling at %u S/s.\nOutput at %u Hz.\n", capture_freq,
	        c.downsample, capture_rate, (unsigned)(c.rate_out2 > 0 ? c.rate_out2 : c.rate_out));
	if (a.verbosity)
		fprintf(stderr, "downsample_passes = %d, downsample = %d, deemph_a = %d, buffer = %u B\n", c.downsample_passes,
		        c.downsample, c.deemph_a, c.block_len);

	int r = rtlfm_gpu_create(&c, 1, 0, &a.gpu);
	if (r < 0) { fprintf(stderr, "rtlfm_gpu_create: %s\n", rtlfm_gpu_strerror(r)); return 2; }
	if (resume_file && (r = rtlfm_gpu_load(a.gpu, resume_file)) < 0) { fprintf(stderr, "-R %s: %s\n", resume_file, rtlfm_gpu_strerror(r)); return 2; }
	a.keep_file = keep_file;
	if (c.squelch_level) {
		// -l: demod_thread_fn's rule on the device where the configuration has a gate (not behind a resampler)
		r = rtlfm_gpu_set_option(a.gpu, "conseq_squelch", conseq_squelch);
		if (r == 0) r = rtlfm_gpu_set_option(a.gpu, "squelch_gate", 1);
		a.use_gate = r == 0;
		if (r < 0 && r != -ENOTSUP) { fprintf(stderr, "squelch_gate: %s\n", rtlfm_gpu_strerror(r)); return 2; }
	}
	if (agc == 2) {
		r = rtlfm_gpu_set_option(a.gpu, "input_health", 1);
		if (r == 0) r = health_create(&a.hl, {a.dev}, c.max_blocks, a.verbosity);
		if (r < 0) { fprintf(stderr, "rtlfm_agc_create: %s\n", rtlfm_gpu_strerror(r)); return 2; }
	}
	a.file = !strcmp(filename, "-") ? stdout : fopen(filename, "wb");
	if (!a.file) { fprintf(stderr, "Failed to open %s\n", filename); return 1; }
	if (write_wav && a.file != stdout)  // src/rtl_fm.c:1990-1995
		rtlamd_wave_write_header(&a.wave, (unsigned)(c.rate_out2 > 0 ? c.rate_out2 : c.rate_out), freq, 16,
		                         c.mode == RTLFM_MODE_RAW ? 2 : 1, a.file);
	rtlsdr_reset_buffer(a.dev);

	std::thread t_out(output_thread, &a), t_demod(demod_thread, &a), t_dongle(dongle_thread, &a);
	t_dongle.join();
	t_demod.join();
	t_out.join();
	if (a.file != stdout) {
		if (write_wav) rtlamd_wave_finalize(&a.wave, a.file);  // src/rtl_fm.c:2041-2045
		fclose(a.file);
	}
	fprintf(stderr, "%llu buffers in, %llu samples out, %llu buffers held back by the squelch%s\n", (unsigned long long)a.blocks_in,
	        (unsigned long long)a.samples_out, (unsigned long long)a.blocks_squelched, a.p.failed ? " (FAILED)" : "");
	if (a.hl.agc) {
		health_report(&a.hl);
		rtlfm_agc_destroy(a.hl.agc);
	}
	if (a.keep_file && !a.p.failed && (r = rtlfm_gpu_save(a.gpu, a.keep_file)) < 0) {  // behind the last run
		fprintf(stderr, "-K %s: %s\n", a.keep_file, rtlfm_gpu_strerror(r));
		a.p.failed = true;
	}
	rtlfm_gpu_destroy(a.gpu);
	rtlsdr_close(a.dev);
	return a.p.failed ? 3 : 0;
}
