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
// the configuration has a gate, else per stream through the carried state.  Behind the device gate under -N, and under -X
// (where the library refuses the gate: there the rule itself runs as option pack_results 2), only what the squelch let
// through comes back from the device (rtlfm_gpu_fetch_packed).  -L prints full_demod()'s level lines.
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
// with %d = s; -H, -L ("stream s:") and -l work per stream (-l: the library's option pack_results 2 applies the rule and
// counts what it held; hold_back only where that is refused, behind a resampler).  -x ntaps puts the channel
// filter rtlfm_channel_lowpass(ntaps, 0.4 / D, D) in the boxcar's place (not with -F: the filter stands where the boxcar
// stands; where its taps do not fit an int16 - fewer taps than D needs - the same filter at D / 2^k and shift 14 - k).
// The demod thread pushes the same number of buffers for every source and run (demod_thread_channels below); the
// streams run in lockstep on ONE sample counter, and no handle is shrunk (the library refuses state_move with channels):
// a source's short last buffer is completed with bytes 127 - which mix to 0 at every phase - to the full length and
// demodulated, a source that has ended is fed buffers of bytes 127 and its K files receive nothing more, until the last
// source ends.  Not with -S, -C, -K, -R, -Z, -O agc=2 or -E rdc: each needs what the library refuses while channels are on.
// -E srcdc (with -X only, not with -E rdc) sets the library's option source_dc: every source's DC spike comes off in front of
// the mixers.
// -E srcagc (with -X only, not with any agc= part in -O) is -O agc=2 for the SOURCES of -X: gain mode 2 on every device, the
// library's option source_health (records of every source's raw bytes, in front of everything), the engine of
// include/rtlfm_agc.h fed after every run with input i = source i, each source's last index applied to its device, and the
// lines of -N -O agc=2 -v with "source %d:" where those say "stream %d:" (under -X a stream is a channel).  The engine is
// fed the full length for a completed short last buffer - the record is over the completed buffer - and nothing for a
// source that has ended: the bytes 127 it is fed must not ramp its gain.  The PCM files are those of the run without it.
// -E srciq (with -X only) is rtl_tcp -c for the SOURCES of -X: the library's option source_iq (every source's second
// moments measured and its bytes rewritten on the device, in front of everything else), the engine of include/rtlfm_iq.h
// fed after every run, and its coefficients handed to the handle for the next run (rtlfm_gpu_set_source_iq).  -v prints
// "source %d: iq a b p q" for every change, "source %d: iq rejected g s" for a window the engine refuses, and every
// source's coefficients at exit.  A source that has ended is fed bytes 127: weak windows, which change nothing.
//
// -k file / -u file (not reference letters; with -X only): keep / take up, -K / -R for channels.  -k writes, behind the last
// run, everything the handle carries - every stream's record, the handle's sample counter, every source's history and its
// bias pieces - to a channel snapshot (rtlfm_gpu_channels_save, include/rtlfm_chansnap.h: its own file kind, magic RTLFMCHN);
// -u loads such a file in front of the first buffer (rtlfm_gpu_channels_load).  -u's file is checked against what the command
// line plans before a device is opened: n x K records, K per source, -x's taps and shift, -E srcdc, the configuration;
// anything else is refused with the library's text, exit status 2.  The PCM of "first half with -k" + "second half with
// -u" is the PCM of the whole capture, cut at a buffer boundary, for every out_%d.raw.  Not without -X (-K / -R are the
// letters for independent streams), not with -S, -C or -E srcagc: those engines carry state of their own that the file does
// not hold.  -X with -K / -R stays refused.
//
// Not restated (out of scope): the command file's own hop (its 2 x 3 200 000 byte mute, the DC-filter reset, -B), and
// -t negative (terminate on squelch).
//
// How the file is laid out.  main fills ONE Settings from the command line and hands it, const, to the mode that runs:
// run_single (one source: Plumbing, next_slot, on_buffer, demod_thread - the callback pushes or commits straight into the
// ring, which is what -Z and stdout need), run_multi (-N, -C, -S) or run_channels (-X).  What the modes share exists
// once: open_source (a device and its tuner calls), Sink (an output file with its wave header, its counters and its -L
// bookkeeping), print_level (the -L line), hold_back (demod_thread_fn's rule from the carried state), squelch_gate_on and
// handle_setup (what a handle gets after it is created), read_list_file (-S and -X), plan_one / plan_for_all (the rate
// plan), summary (the closing lines), and for the two modes with host queues take_batch, run_and_fetch, deliver and fail.
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
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/rtlfm_hip.h"
#include "../../../include/rtlfm_agc.h"
#include "../../../include/rtlfm_iq.h"
#include "../../../include/rtlfm_monitor.h"
#include "../../../include/rtlfm_scan.h"
#include "../../../include/rtlfm_snapshot.h"
#include "../../../include/rtlfm_chansnap.h"
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

// everything main parses; the modes read it and change nothing
struct Settings {
	rtlfm_cfg cfg;              // what the handle is created with: the command line's, then plan_for_all's
	uint32_t capture_rate = 0;  // ... and the capture rate of that plan
	int rate_in = 24000, min_capture = 1000000, fifth = 0, edge = 0, time_constant = 75;  // what the plan is asked with
	int gain = -100, ppm = 0, dev_index = 0, verbosity = 0;
	int conseq_squelch = 10;  // demod_init(), src/rtl_fm.c:1613
	int print_levels = 0;     // -L (src/rtl_fm.c:1757-1759)
	bool write_wav = false, wb_mode = false;
	bool zero_copy = false;  // -Z: the device layer reads straight into the pinned staging ring
	const char *filename = "-", *cmd_file = nullptr, *scan_file = nullptr, *keep_file = nullptr, *resume_file = nullptr;
	const char *chan_file = nullptr, *opt_string = nullptr;
	const char *chan_keep_file = nullptr, *chan_resume_file = nullptr;  // -k / -u: -K / -R for -X (a channel snapshot)
	bool source_dc = false;  // -E srcdc: the library's option source_dc (with -X only)
	bool source_agc = false; // -E srcagc: the software AGC per source (with -X only; not with agc= in -O)
	bool source_iq = false;  // -E srciq: IQ balance per source (with -X only)
	int agc = -1;        // -O agc=<n>; -1: not given
	int chan_taps = -1;  // -x; -1: not given
};

unsigned out_rate(const rtlfm_cfg &c) { return (unsigned)(c.rate_out2 > 0 ? c.rate_out2 : c.rate_out); }

// optimal_settings() (src/rtl_fm.c:1407-1445) for one frequency, asked with what the command line gave
void plan_one(const Settings &st, uint32_t freq, rtlfm_cfg *cfg, uint32_t *capture_freq, uint32_t *capture_rate)
{
	rtlfm_optimal_settings(cfg, freq, st.rate_in, st.min_capture, st.fifth, st.edge, capture_freq, capture_rate);
}

// One plan for all sources (deemph_a, src/rtl_fm.c:1929-1934, and optimal_settings(), which must not depend on the
// frequency for what this CLI accepts) into st.cfg / st.capture_rate, each source's capture frequency into capture_freqs
// where the caller wants them: 0, or the index of the first source whose plan differs from source 0's (st is then as it was)
int plan_for_all(Settings &st, const std::vector<uint32_t> &freqs, std::vector<uint32_t> *capture_freqs)
{
	rtlfm_cfg c = st.cfg, planned = c;
	if (c.deemph) c.deemph_a = rtlfm_deemph_a(c.rate_out, st.time_constant);
	if (capture_freqs) capture_freqs->assign(freqs.size(), 0);
	uint32_t capture_rate = 0;
	for (size_t i = 0; i < freqs.size(); i++) {
		rtlfm_cfg ci = c;
		uint32_t cr = 0;
		plan_one(st, freqs[i], &ci, capture_freqs ? &(*capture_freqs)[i] : nullptr, &cr);
		if (i == 0) {
			planned = ci;
			capture_rate = cr;
		} else if (memcmp(&ci, &planned, sizeof(ci)) != 0 || cr != capture_rate) {
			return (int)i;
		}
	}
	st.cfg = planned;
	st.capture_rate = capture_rate;
	return 0;
}

// A file of frequency lists (-S, -X): one list per line in rtlfm_scan_parse_list's grammar, blank lines and lines that
// start with '#' skipped.  0, -ENOENT (cannot open it) or -EINVAL with *bad_line = the line that is no list
int read_list_file(const char *path, std::vector<std::vector<uint32_t>> &lists, std::vector<int> *linenos, int *bad_line)
{
	FILE *f = fopen(path, "r");
	if (!f) return -ENOENT;
	char line[65536];
	int lineno = 0, r = 0;
	while (r == 0 && fgets(line, sizeof(line), f)) {
		lineno++;
		const char *t = line;
		while (*t == ' ' || *t == '\t') t++;
		if (*t == '#' || *t == '\n' || *t == '\r' || !*t) continue;
		int nf = 0;
		int pr = rtlfm_scan_parse_list(t, nullptr, 0, &nf);
		std::vector<uint32_t> fl((size_t)(nf > 0 ? nf : 0));
		if (pr == -ENOBUFS) pr = rtlfm_scan_parse_list(t, fl.data(), nf, &nf);
		if (pr < 0) {
			*bad_line = lineno;
			r = -EINVAL;
			break;
		}
		lists.push_back(std::move(fl));
		if (linenos) linenos->push_back(lineno);
	}
	fclose(f);
	return r;
}

// Device dev_index + i, open and set up as the reference's main does it (src/rtl_fm.c:1945-1985): gain, the -O string, ppm,
// offset tuning, frequency, rate.  nullptr behind the message when it cannot be opened.  The caller says where it is tuned.
rtlsdr_dev_t *open_source(const Settings &st, int i, int gain, uint32_t capture_freq)
{
	rtlsdr_dev_t *dev = nullptr;
	if (rtlsdr_open(&dev, (uint32_t)(st.dev_index + i)) < 0) {
		fprintf(stderr, "Failed to open rtlsdr device #%d.\n", st.dev_index + i);
		return nullptr;
	}
	if (gain == -100) rtlsdr_set_tuner_gain_mode(dev, 0);
	else { rtlsdr_set_tuner_gain_mode(dev, 1); rtlsdr_set_tuner_gain(dev, gain); }
	if (st.opt_string) rtlsdr_set_opt_string(dev, st.opt_string, st.verbosity);
	if (st.agc >= 0) rtlsdr_set_tuner_gain_mode(dev, st.agc);  // the string's agc=<tuner_gain_mode>, src/librtlsdr.c:3166-3171
	if (st.source_agc) rtlsdr_set_tuner_gain_mode(dev, 2);     // -E srcagc: as agc=2 (main has refused the two together)
	rtlsdr_set_freq_correction_ppb(dev, st.ppm * 1000);
	rtlsdr_set_offset_tuning(dev, st.cfg.offset_tuning);
	rtlsdr_set_center_freq(dev, capture_freq);
	if (rtlsdr_set_sample_rate(dev, st.capture_rate) < 0 && i == 0)
		fprintf(stderr, "WARNING: capture rate %u Hz is outside what an RTL2832 can do.\n", st.capture_rate);
	return dev;
}

// One output: the file, its wave header, what went into it and what the squelch held back, and its -L bookkeeping
// (src/rtl_fm.c:109-113, 1217-1237).  index = the %d of the file's name and the i of "stream i: "; -1 = the one output
// of a single source, whose name is taken as it is ('-' = stdout) and whose lines carry no prefix.
struct Sink {
	FILE *file = nullptr;
	rtlamd_wave wave{};
	int index = -1;
	uint32_t user_freq = 0;  // dongle.userFreq, src/rtl_fm.c:1440
	uint64_t samples_out = 0, blocks_squelched = 0;
	int print_level_no = 1, level_max = 0, level_max_max = 0;
	double level_sum = 0.0;

	bool open(const Settings &st, int idx, uint32_t freq)
	{
		index = idx;
		user_freq = freq;
		std::string name(st.filename);
		const size_t at = name.find("%d");
		if (idx >= 0 && at != std::string::npos) name = name.substr(0, at) + std::to_string(idx) + name.substr(at + 2);
		file = idx < 0 && name == "-" ? stdout : fopen(name.c_str(), "wb");
		if (!file) {
			fprintf(stderr, "Failed to open %s\n", name.c_str());
			return false;
		}
		if (st.write_wav)  // src/rtl_fm.c:1990-1995; nothing on stdout
			rtlamd_wave_write_header(&wave, out_rate(st.cfg), freq, 16, st.cfg.mode == RTLFM_MODE_RAW ? 2 : 1, file);
		return true;
	}
	void write(const int16_t *pcm, size_t n)
	{
		fwrite(pcm, 2, n, file);           // src/rtl_fm.c:1400
		wave.data_size += 2 * (uint32_t)n;  // waveDataSize, :1401
		samples_out += n;
	}
	void close()
	{
		if (!file || file == stdout) return;
		rtlamd_wave_finalize(&wave, file);  // src/rtl_fm.c:2041-2045; nothing where no header was written
		fclose(file);
		file = nullptr;
	}
};

// -L: full_demod()'s level printing, src/rtl_fm.c:1217-1237, on the rms() the GPU layer kept for handle stream k
void print_level(Sink &s, rtlfm_gpu *gpu, int k, const Settings &st)
{
	int32_t sr = 0;
	int nl = 0;
	if (rtlfm_gpu_levels(gpu, k, &sr, 1, &nl) != 0 || nl != 1) return;
	--s.print_level_no;
	if (sr < 0) return;
	s.level_sum += sr;
	if (s.level_max < sr) s.level_max = sr;
	if (s.level_max_max < sr) s.level_max_max = sr;
	if (s.print_level_no) return;
	s.print_level_no = st.print_levels;
	const double avg_rms = s.level_sum / st.print_levels;
	const std::string prefix = s.index < 0 ? "" : "stream " + std::to_string(s.index) + ": ";
	fprintf(stderr, "%s%.3f kHz, %.1f avg rms, %d max rms, %d max max rms, %d squelch rms, %d rms, %.1f dB rms level, %.2f dB avg rms level\n",
	        prefix.c_str(), s.user_freq / 1000.0, avg_rms, s.level_max, s.level_max_max, st.cfg.squelch_level, (int)sr,
	        20.0 * log10(1E-10 + sr), 20.0 * log10(1E-10 + avg_rms));
	s.level_max = 0;
	s.level_sum = 0;
}

// -l without a device gate: demod_thread_fn()'s rule (src/rtl_fm.c:1366-1370) from the carried state, after a run of one
// buffer per stream.  While a stream's squelch has been closed for more than conseq_squelch buffers its buffer does not go
// to the output thread - on_held(k) -, and the counter is held one above the limit ("hair trigger").  squelch_hits starts
// at 11 (:1615): silence until it first opens.  Every stream's state in one copy, and one copy back only in a run that
// clamped a counter.
template <class F>
void hold_back(rtlfm_gpu *gpu, int nstreams, int conseq_squelch, std::vector<rtlfm_stream_state> &states, F on_held)
{
	states.resize((size_t)nstreams);
	int got = 0;
	bool clamped = false;
	if (rtlfm_gpu_state_get_all(gpu, states.data(), nstreams, &got) != 0) return;
	for (int k = 0; k < nstreams; k++) {
		rtlfm_stream_state &s = states[(size_t)k];
		if (s.squelch_hits <= conseq_squelch) continue;
		clamped |= s.squelch_hits != conseq_squelch + 1;
		s.squelch_hits = conseq_squelch + 1;
		on_held(k);
	}
	if (clamped) rtlfm_gpu_state_set_all(gpu, states.data(), nstreams);
}

// -l on the device: the same rule as the handle's squelch gate, where the configuration has one.  -ENOTSUP (behind a
// resampler) is no error unless the caller needs the gate (-S does): *on = false then, and hold_back applies the rule.
int squelch_gate_on(rtlfm_gpu *gpu, int conseq_squelch, bool needed, bool *on)
{
	int r = rtlfm_gpu_set_option(gpu, "conseq_squelch", conseq_squelch);
	if (r == 0) r = rtlfm_gpu_set_option(gpu, "squelch_gate", 1);
	*on = r == 0;
	return r == -ENOTSUP && !needed ? 0 : r;
}

// the closing lines: the totals of the n outputs of sources that gave in_all buffers, and with `each` a line per output -
// with its source's buffers where an output is a source's (in_each), without them where sources fan out into channels (-X)
void summary(const Sink *out, size_t n, uint64_t in_all, const uint64_t *in_each, bool failed, bool each)
{
	auto buffers = [](uint64_t b) { return std::to_string(b) + " buffers in, "; };
	auto line = [](const std::string &head, uint64_t samples, uint64_t held, const char *tail) {
		fprintf(stderr, "%s%llu samples out, %llu buffers held back by the squelch%s\n", head.c_str(), (unsigned long long)samples,
		        (unsigned long long)held, tail);
	};
	uint64_t samples = 0, held = 0;
	for (size_t s = 0; s < n; s++) {
		samples += out[s].samples_out;
		held += out[s].blocks_squelched;
	}
	line(buffers(in_all), samples, held, failed ? " (FAILED)" : "");
	for (size_t s = 0; each && s < n; s++)
		line("stream " + std::to_string(out[s].index) + ": " + (in_each ? buffers(in_each[s]) : ""), out[s].samples_out,
		     out[s].blocks_squelched, "");
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

// -O agc=2, and -E srcagc under -X: the software AGC and the overload report for every source (include/rtlfm_agc.h)
struct Health {
	bool by_source = false;               // -E srcagc: the records are the handle's per-SOURCE ones, row i = source i, and the lines say "source"
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

// after a run: stream k of the handle is source live[k], whose buffers of this run were lens[k] bytes long.  (by_source:
// the handle has a row of records for every source, live or not; only the live ones are fed.)
int health_step(Health *hl, rtlfm_gpu *gpu, int cap, const std::vector<int> &live, const std::vector<std::vector<uint32_t>> &lens)
{
	const char *noun = hl->by_source ? "source" : "stream";
	hl->recs.resize((hl->by_source ? hl->devs.size() : live.size()) * (size_t)cap);
	int n = 0;
	int r = hl->by_source ? rtlfm_gpu_source_health_all(gpu, hl->recs.data(), cap, &n) : rtlfm_gpu_input_health_all(gpu, hl->recs.data(), cap, &n);
	if (r < 0) return r;
	for (size_t k = 0; k < live.size(); k++) {
		const int i = live[k];
		if ((int)lens[k].size() != n) return -EPROTO;
		const rtlfm_input_health *rec = hl->recs.data() + (hl->by_source ? (size_t)i : k) * (size_t)cap;
		if ((r = rtlfm_agc_feed(hl->agc, i, rec, lens[k].data(), n)) < 0) return r;
		for (int b = 0; b < n; b++) {
			const int ov = 8000ll * rec[b].overload >= (long long)lens[k][(size_t)b] ? 1 : 0;  // src/rtl_tcp.c:243
			if (ov != hl->overloaded[(size_t)i] && hl->verbosity)
				fprintf(stderr, "%s %d: buffer %lld: overload %s\n", noun, i, hl->serial[(size_t)i], ov ? "begins" : "ends");
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
				fprintf(stderr, "%s %d: buffer %lld: gain index %d -> %d, gain %d (%s)\n", noun, ev[e].stream, (long long)ev[e].buffer_serial,
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
		fprintf(stderr, "%s %zu: final gain index %d, gain %d\n", hl->by_source ? "source" : "stream", i, idx, hl->gains[i][(size_t)idx]);
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

// What a handle gets after rtlfm_gpu_create, each with its message: -O agc=2 (the option input_health and the engine for
// `devs`), -R, and -l's device gate (*use_gate; `gate_needed` as squelch_gate_on's).  false = exit status 2
bool handle_setup(rtlfm_gpu *gpu, const Settings &st, const std::vector<rtlsdr_dev_t *> &devs, Health *hl, bool gate_needed, bool *use_gate)
{
	int r = 0;
	if (st.agc == 2) {
		r = rtlfm_gpu_set_option(gpu, "input_health", 1);
		if (r == 0) r = health_create(hl, devs, st.cfg.max_blocks, st.verbosity);
		if (r < 0) { fprintf(stderr, "rtlfm_agc_create: %s\n", rtlfm_gpu_strerror(r)); return false; }
	}
	if (st.resume_file && (r = rtlfm_gpu_load(gpu, st.resume_file)) < 0) {
		fprintf(stderr, "-R %s: %s\n", st.resume_file, rtlfm_gpu_strerror(r));
		return false;
	}
	if (st.cfg.squelch_level && (r = squelch_gate_on(gpu, st.conseq_squelch, gate_needed, use_gate)) < 0) {
		fprintf(stderr, "squelch_gate: %s\n", rtlfm_gpu_strerror(r));
		return false;
	}
	return true;
}

// ---- one source: the callback pushes or commits straight into the ring -------------------------------------

struct App {
	const Settings &st;
	rtlfm_gpu *gpu = nullptr;
	rtlsdr_dev_t *dev = nullptr;
	Plumbing p;
	Sink out;
	uint64_t blocks_in = 0;
	bool use_gate = false;               // -l through the device's squelch gate (rtlfm_gpu_gate)
	unsigned char *open_slot = nullptr;  // -Z: the slot the device layer is filling (rtlfm_gpu_acquire)
	Health hl;                           // -O agc=2
	std::deque<uint32_t> in_lens;        // ... the lengths of the buffers in the ring, oldest first (under p.m)
	explicit App(const Settings &s) : st(s) {}
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
		a->p.cv_room.wait(g, [&] { return (!a->p.want_run && a->p.queued < a->st.cfg.max_blocks) || a->p.failed; });
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
		a->p.cv_room.wait(g, [&] { return (!a->p.want_run && a->p.queued < a->st.cfg.max_blocks) || a->p.failed; });
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
	if (a->st.zero_copy) rtlamd_file_set_buffer_source(a->dev, next_slot, a);
	rtlsdr_read_async(a->dev, on_buffer, a, 0, a->st.cfg.block_len);
	std::lock_guard<std::mutex> g(a->p.m);
	a->p.eof = true;
	a->p.cv_work.notify_all();
}

void demod_thread(App *a)
{
	const rtlfm_cfg &c = a->st.cfg;
	const int cap = rtlfm_result_cap(&c) * c.max_blocks + 16;
	std::vector<rtlfm_stream_state> states;
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
		if (r == 0 && a->hl.agc) r = health_step(&a->hl, a->gpu, c.max_blocks, {0}, run_lens);
		if (r < 0) {
			fprintf(stderr, "rtlfm_gpu_run/fetch: %s\n", rtlfm_gpu_strerror(r));
			std::lock_guard<std::mutex> g(a->p.m);
			a->p.failed = true;
			rtlsdr_cancel_async(a->dev);
			a->p.cv_room.notify_all();
			break;
		}
		pcm.resize((size_t)n);
		if (a->st.print_levels) print_level(a->out, a->gpu, 0, a->st);
		bool held = false;
		if (a->use_gate) {
			// the rule applied on the device: a held buffer comes back with no samples and its record says so
			rtlfm_gate_rec g1;
			int ng = 0;
			held = rtlfm_gpu_gate(a->gpu, 0, &g1, 1, &ng) == 0 && ng == 1 && !g1.emit;
		} else if (c.squelch_level) {
			hold_back(a->gpu, 1, a->st.conseq_squelch, states, [&](int) { held = true; });
		}
		if (held) {
			a->out.blocks_squelched++;
			continue;
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
		a->out.write(pcm.data(), pcm.size());
	}
	fflush(a->out.file);
}

// everything after option parsing for one source; freq = where the user tunes it (+16 kHz under -M wbfm)
int run_single(const Settings &st, uint32_t freq, uint32_t capture_freq)
{
	App a(st);
	const rtlfm_cfg &c = st.cfg;
	if (rtlsdr_get_device_count() == 0) { fprintf(stderr, "No supported devices found (set RTLSDR_FILE).\n"); return 1; }
	if (!(a.dev = open_source(st, 0, st.gain, capture_freq))) return 1;
	fprintf(stderr, "Tuned to %u Hz.\nOversampling input by: %ix.\nSampling at %u S/s.\nOutput at %u Hz.\n", capture_freq,
	        c.downsample, st.capture_rate, out_rate(c));
	if (st.verbosity)
		fprintf(stderr, "downsample_passes = %d, downsample = %d, deemph_a = %d, buffer = %u B\n", c.downsample_passes,
		        c.downsample, c.deemph_a, c.block_len);
	int r = rtlfm_gpu_create(&c, 1, 0, &a.gpu);
	if (r < 0) { fprintf(stderr, "rtlfm_gpu_create: %s\n", rtlfm_gpu_strerror(r)); return 2; }
	if (!handle_setup(a.gpu, st, {a.dev}, &a.hl, false, &a.use_gate)) return 2;
	if (!a.out.open(st, -1, freq)) return 1;
	rtlsdr_reset_buffer(a.dev);

	std::thread t_out(output_thread, &a), t_demod(demod_thread, &a), t_dongle(dongle_thread, &a);
	t_dongle.join();
	t_demod.join();
	t_out.join();
	a.out.close();
	summary(&a.out, 1, a.blocks_in, nullptr, a.p.failed, false);
	if (a.hl.agc) {
		health_report(&a.hl);
		rtlfm_agc_destroy(a.hl.agc);
	}
	if (st.keep_file && !a.p.failed && (r = rtlfm_gpu_save(a.gpu, st.keep_file)) < 0) {  // behind the last run
		fprintf(stderr, "-K %s: %s\n", st.keep_file, rtlfm_gpu_strerror(r));
		a.p.failed = true;
	}
	rtlfm_gpu_destroy(a.gpu);
	rtlsdr_close(a.dev);
	return a.p.failed ? 3 : 0;
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
	rtlsdr_dev_t *dev = nullptr;
	Multi *m = nullptr;
	std::deque<std::vector<uint8_t>> q;       // buffers copied by the callback, not yet taken by a run
	std::vector<std::vector<uint8_t>> spare;  // taken buffers come back here, so a callback hardly ever allocates
	std::vector<std::vector<uint8_t>> taken;  // what the current run pushes
	int copying = 0;                          // callbacks copying into a reserved place of the queue
	bool eof = false;
	std::condition_variable cv_room;
	uint64_t blocks_in = 0;
};

struct RunOut {
	std::vector<int16_t> pcm;  // handle stream k at k * stride - or, fetched packed, at at[k]
	std::vector<int32_t> lens;
	std::vector<int> who;      // handle stream k -> output
	size_t stride = 0;
	std::vector<size_t> at;    // rtlfm_gpu_fetch_packed: where stream k's samples start (empty: rows of `stride`)
	std::vector<int32_t> held; // ... and how many of its buffers the rule left out (option pack_results 2)
};

struct Multi {
	const Settings &st;
	rtlfm_gpu *gpu = nullptr;
	std::vector<Source> src;
	std::vector<Sink> out;  // -N: out[i] is source i's; -X: out[s] is handle stream s's, channel s % K of source s / K
	int depth = 0;
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
	rtlfm_iq *iq = nullptr;  // -E srciq: the IQ-balance engine, input i = source i
	bool use_gate = false;  // -l through the device's squelch gate
	// -S: the hop engine, list i = source i
	rtlfm_scan *scan = nullptr;
	std::vector<rtlfm_gate_rec> gate_recs;
	// -K: record i = source i.  A source that leaves the batch leaves its record here (shrink); the others' are read at exit
	std::vector<rtlfm_stream_state> kept;
	std::vector<int> live;                   // handle stream k -> source, as the demod thread left it
	std::vector<rtlfm_stream_state> states;  // one rtlfm_gpu_state_get_all: -l without a device gate, -K
	int chan_per = 0;                        // -X: K channels per source
	bool packed = false;                     // the handle runs with option pack_results: rtlfm_gpu_fetch_packed brings the PCM
	explicit Multi(const Settings &s, size_t sources, size_t outputs) : st(s), src(sources), out(outputs), depth(2 * s.cfg.max_blocks) {}
};

// the options a handle of this tool runs with besides its configuration (shrink: what the first handle was given)
int handle_options(Multi *m, rtlfm_gpu *h)
{
	int r = 0;
	bool on = false;
	if (m->mon) r = rtlfm_gpu_set_option(h, "input_stats", 1);
	if (r == 0 && m->hl.agc) r = rtlfm_gpu_set_option(h, "input_health", 1);
	if (r == 0 && m->use_gate) r = squelch_gate_on(h, m->st.conseq_squelch, true, &on);
	// behind the gate most rows are short or empty: only what they hold comes back (rtlfm_gpu_fetch_packed)
	if (r == 0 && m->use_gate) r = rtlfm_gpu_set_option(h, "pack_results", 1);
	if (r == 0 && m->use_gate) m->packed = true;
	return r;
}

void fail(Multi *m, const char *what, int r)
{
	std::lock_guard<std::mutex> g(m->m);
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
	rtlsdr_read_async(s->dev, on_buffer_multi, s, 0, s->m->st.cfg.block_len);
	std::lock_guard<std::mutex> g(s->m->m);
	s->eof = true;  // after the last callback: the queue holds everything the source gave
	s->m->cv_work.notify_one();
}

// Taking a batch: wait until every source in `live` has a buffer or has ended; the ones that have ended (an empty queue
// then) leave `live`; from each of the others b = min(what every queue holds, max_blocks) buffers go to its `taken`, and
// its callback is woken.  Returns b, or 0 when the run has failed or no source is left.
int take_batch(Multi *m, std::vector<int> &live)
{
	std::unique_lock<std::mutex> g(m->m);
	m->cv_work.wait(g, [&] {
		if (m->failed) return true;
		for (int i : live)
			if (m->src[(size_t)i].q.empty() && !m->src[(size_t)i].eof) return false;
		return true;
	});
	if (m->failed) return 0;
	live.erase(std::remove_if(live.begin(), live.end(), [&](int i) { return m->src[(size_t)i].q.empty(); }), live.end());
	if (live.empty()) return 0;
	int b = m->st.cfg.max_blocks;
	for (int i : live) b = std::min(b, (int)m->src[(size_t)i].q.size());
	for (int i : live) {
		Source &s = m->src[(size_t)i];
		for (int j = 0; j < b; j++) {
			s.taken.push_back(std::move(s.q.front()));
			s.q.pop_front();
		}
		s.cv_room.notify_all();
	}
	return b;
}

// The run behind the pushes (r = what they returned) of b buffers per ring row, and the PCM of the handle's who.size()
// streams, stream k for output who[k].  false behind fail().
bool run_and_fetch(Multi *m, int r, int b, const std::vector<int> &who, RunOut &o)
{
	int ran = 0;
	if (r == 0) r = rtlfm_gpu_run_begin(m->gpu, &ran);
	if (r == 0 && ran != b) r = -EPROTO;
	if (r == 0) r = rtlfm_gpu_run_end(m->gpu);
	o.stride = ((size_t)rtlfm_result_cap(&m->st.cfg) * m->st.cfg.max_blocks + 16 + 63) / 64 * 64;
	o.pcm.resize(who.size() * o.stride);
	o.lens.resize(who.size());
	o.who = who;
	if (r == 0 && m->packed) {
		std::vector<rtlfm_packed_row> rows(who.size());
		size_t total = 0;
		r = rtlfm_gpu_fetch_packed(m->gpu, o.pcm.data(), o.pcm.size(), rows.data(), &total);
		o.at.resize(who.size());
		o.held.resize(who.size());
		for (size_t k = 0; k < who.size() && r == 0; k++) {
			o.at[k] = (size_t)rows[k].offset;
			o.lens[k] = rows[k].len;
			o.held[k] = rows[k].held;
		}
	} else if (r == 0) {
		r = rtlfm_gpu_fetch_all(m->gpu, o.pcm.data(), o.stride, o.lens.data());
	}
	if (r < 0) fail(m, "rtlfm_gpu_push/run/fetch", r);
	return r == 0;
}

// a run's PCM to the output thread, and what the run pushed back to the callbacks' spare buffers
void deliver(Multi *m, RunOut &o)
{
	std::lock_guard<std::mutex> g(m->m);
	for (Source &s : m->src) {
		for (std::vector<uint8_t> &buf : s.taken) s.spare.push_back(std::move(buf));
		s.taken.clear();
	}
	m->out_q.push_back(std::move(o));
	m->cv_out.notify_one();
}

void demod_done(Multi *m)
{
	std::lock_guard<std::mutex> g(m->m);
	m->out_done = true;
	m->cv_out.notify_all();
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
	if (m->st.keep_file && (r = keep_states(m, live, &stay)) < 0) return r;  // in front of the regroup: what the leaving sources carried
	rtlfm_gpu *nh = nullptr;
	r = rtlfm_gpu_create(&m->st.cfg, (int)stay.size(), 0, &nh);
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
		const int cap = m->st.cfg.max_blocks;
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
			if (m->st.verbosity) {
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
	const int cap = m->st.cfg.max_blocks;
	m->gate_recs.resize(live.size() * (size_t)cap);
	int n = 0;
	int r = rtlfm_gpu_gate_all(m->gpu, m->gate_recs.data(), cap, &n);
	if (r < 0) return r;
	for (size_t k = 0; k < live.size(); k++) {
		for (int b = 0; b < n; b++)
			if (!m->gate_recs[k * (size_t)cap + b].emit) m->out[(size_t)live[k]].blocks_squelched++;
		if (m->scan && (r = rtlfm_scan_feed(m->scan, live[k], m->gate_recs.data() + k * (size_t)cap, n)) < 0) return r;
	}
	if (!m->scan) return 0;
	rtlfm_scan_event ev[64];
	for (;;) {
		int ne = 0;
		if ((r = rtlfm_scan_events(m->scan, ev, 64, &ne)) < 0) return r;
		for (int e = 0; e < ne; e++) {
			Sink &o = m->out[(size_t)ev[e].stream];
			const uint32_t f_new = ev[e].freq + (m->st.wb_mode ? 16000u : 0u);  // src/rtl_fm.c:1455-1460
			rtlfm_cfg ci = m->st.cfg;
			uint32_t cf = 0;
			plan_one(m->st, f_new, &ci, &cf, nullptr);
			rtlsdr_set_center_freq(m->src[(size_t)ev[e].stream].dev, cf);  // :1506
			if (m->st.verbosity)
				fprintf(stderr, "stream %d: hop %u -> %u at buffer %lld\n", ev[e].stream, o.user_freq, f_new, (long long)ev[e].buffer_serial);
			o.user_freq = f_new;
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
	const rtlfm_cfg &c = m->st.cfg;
	std::vector<int> live;
	for (size_t i = 0; i < m->src.size(); i++) live.push_back((int)i);
	// -vv: where this thread's time goes (waiting for the slowest source, the copy into the ring, run + fetch, the
	// per-stream -l / -L calls)
	using clk = std::chrono::steady_clock;
	double t_wait = 0, t_push = 0, t_run = 0, t_per_stream = 0;
	uint64_t runs = 0;
	auto since = [](clk::time_point t0) { return std::chrono::duration<double>(clk::now() - t0).count(); };
	for (;;) {
		clk::time_point t0 = clk::now();
		std::vector<int> stay = live;
		const int b = take_batch(m, stay);
		if (!b) break;
		if (stay.size() != live.size()) {
			int r = shrink(m, live, stay);
			if (r < 0) {
				fail(m, "rtlfm_gpu_create / rtlfm_gpu_state_move", r);
				break;
			}
			if (m->st.verbosity)
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
		RunOut o;
		if (!run_and_fetch(m, r, b, live, o)) break;
		if (m->hl.agc) {
			std::vector<std::vector<uint32_t>> lens(ns);
			for (size_t k = 0; k < ns; k++)
				for (const std::vector<uint8_t> &buf : m->src[live[k]].taken) lens[k].push_back((uint32_t)buf.size());
			if ((r = health_step(&m->hl, m->gpu, c.max_blocks, live, lens)) < 0) {
				fail(m, "rtlfm_gpu_input_health_all / rtlfm_agc_feed", r);
				break;
			}
		}
		if (m->mon && (r = monitor_step(m, live)) < 0) {
			fail(m, "rtlfm_monitor_update / feed", r);
			break;
		}
		if (m->use_gate && (r = gate_step(m, live)) < 0) {
			fail(m, "rtlfm_gpu_gate_all / rtlfm_scan_feed / rtlfm_gpu_mute", r);
			break;
		}
		t_run += since(t0);
		t0 = clk::now();
		runs++;
		if (m->st.print_levels)
			for (size_t k = 0; k < ns; k++) print_level(m->out[(size_t)live[k]], m->gpu, (int)k, m->st);
		if (c.squelch_level && !m->use_gate)  // max_blocks is 1 here
			hold_back(m->gpu, (int)ns, m->st.conseq_squelch, m->states, [&](int k) {
				m->out[(size_t)live[(size_t)k]].blocks_squelched++;
				o.lens[(size_t)k] = 0;
			});
		t_per_stream += since(t0);
		deliver(m, o);
	}
	m->live = live;
	if (m->st.verbosity >= 2)
		fprintf(stderr, "demod thread: %llu runs; %.3f s waiting for buffers, %.3f s pushing, %.3f s run + fetch_all, %.3f s -l / -L\n",
		        (unsigned long long)runs, t_wait, t_push, t_run, t_per_stream);
	demod_done(m);
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
		for (size_t k = 0; k < o.who.size(); k++)
			if (o.lens[k]) m->out[(size_t)o.who[k]].write(o.pcm.data() + (o.at.empty() ? k * o.stride : o.at[k]), (size_t)o.lens[k]);
	}
	for (Sink &s : m->out) fflush(s.file);
}

// devices dev_index .. dev_index + n - 1 exist?  `asked` is how the caller's message names what wants them
bool devices_there(const Settings &st, int n, const std::string &asked)
{
	const uint32_t count = rtlsdr_get_device_count();
	if (count == 0) { fprintf(stderr, "No supported devices found (set RTLSDR_FILE or RTLSDR_FILE_LIST).\n"); return false; }
	if ((uint64_t)st.dev_index + (uint64_t)n > count) {
		fprintf(stderr, "-d %d %s needs devices %d .. %d, and there are %u.\n", st.dev_index, asked.c_str(), st.dev_index,
		        st.dev_index + n - 1, count);
		return false;
	}
	return true;
}

// the output thread, the mode's demod thread and a dongle thread per source, until the last source has ended
void run_threads(Multi *m, void (*demod)(Multi *))
{
	for (Source &s : m->src) rtlsdr_reset_buffer(s.dev);
	std::thread t_out(output_thread_multi, m), t_demod(demod, m);
	std::vector<std::thread> t_dongle;
	for (Source &s : m->src) t_dongle.emplace_back(dongle_thread_multi, &s);
	for (std::thread &t : t_dongle) t.join();
	t_demod.join();
	t_out.join();
}

void close_all(Multi *m)
{
	for (Sink &s : m->out) s.close();
	for (Source &s : m->src)
		if (s.dev) rtlsdr_close(s.dev);
	if (m->gpu) rtlfm_gpu_destroy(m->gpu);
}

// everything after option parsing for -N, -C and -S (main has refused what they do not allow): source i is tuned to
// capture_freqs[i] for the user's freqs[i]; rules (-C) and scan_lists (-S) are empty or hold one entry per source
int run_multi(const Settings &st, const std::vector<uint32_t> &freqs, const std::vector<uint32_t> &capture_freqs,
              const std::vector<rtlfm_monitor_rule> &rules, const std::vector<std::vector<uint32_t>> &scan_lists)
{
	const int n = (int)freqs.size();
	const rtlfm_cfg &c = st.cfg;
	Multi m(st, (size_t)n, (size_t)n);
	m.kept.resize((size_t)n);
	m.rules = rules;
	if (!devices_there(st, n, "-N " + std::to_string(n))) return 1;
	int ret = 0;
	for (int i = 0; i < n && !ret; i++) {
		Source &s = m.src[(size_t)i];
		s.m = &m;
		s.dev = open_source(st, i, rules.empty() ? st.gain : rules[(size_t)i].gain, capture_freqs[(size_t)i]);  // -C: each source's gain from its line
		if (!s.dev) ret = 1;
		else if (st.verbosity || i == 0 || capture_freqs[(size_t)i] != capture_freqs[0])
			fprintf(stderr, "stream %d: device #%d, tuned to %u Hz.\n", i, st.dev_index + i, capture_freqs[(size_t)i]);
	}
	if (!ret) {
		fprintf(stderr, "%d streams.\nOversampling input by: %ix.\nSampling at %u S/s.\nOutput at %u Hz.\n", n, c.downsample,
		        st.capture_rate, out_rate(c));
		if (st.verbosity)
			fprintf(stderr, "downsample_passes = %d, downsample = %d, deemph_a = %d, buffer = %u B, host queue = %d buffers per stream\n",
			        c.downsample_passes, c.downsample, c.deemph_a, c.block_len, m.depth);
		int r = rtlfm_gpu_create(&c, n, 0, &m.gpu);
		if (r < 0) {
			fprintf(stderr, "rtlfm_gpu_create: %s\n", rtlfm_gpu_strerror(r));
			ret = 2;
		}
		std::vector<rtlsdr_dev_t *> devs;
		for (Source &s : m.src) devs.push_back(s.dev);
		if (!ret && !handle_setup(m.gpu, st, devs, &m.hl, !scan_lists.empty(), &m.use_gate)) ret = 2;
		if (!ret && !rules.empty()) {
			r = rtlfm_gpu_set_option(m.gpu, "input_stats", 1);
			if (r == 0) r = rtlfm_monitor_create(n, rules.data(), &m.mon);
			if (r < 0) {
				fprintf(stderr, "rtlfm_monitor_create: %s\n", rtlfm_gpu_strerror(r));
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
	for (int i = 0; i < n && !ret; i++)
		if (!m.out[(size_t)i].open(st, i, freqs[(size_t)i])) ret = 1;
	if (!ret) {
		run_threads(&m, demod_thread_multi);
		std::vector<uint64_t> in;
		for (Source &s : m.src) in.push_back(s.blocks_in);
		summary(m.out.data(), m.out.size(), std::accumulate(in.begin(), in.end(), (uint64_t)0), in.data(), m.failed, st.verbosity > 0);
		if (m.mon) {
			fprintf(stderr, "%llu monitor events, %llu fired\n", (unsigned long long)m.events, (unsigned long long)m.fired);
			// the scan statistics of src/rtl_fm.c:2033-2040, one line per command-file line that reported a level
			for (int i = 0; i < n; i++) {
				rtlfm_monitor_stat ms;
				if (rtlfm_monitor_stats(m.mon, i, &ms) == 0 && ms.count > 0)
					fprintf(stderr, "%u, %.1f, %.2f, %.1f\n", rules[(size_t)i].freq, ms.min_level, ms.sum_levels / ms.count, ms.max_level);
			}
		}
		if (m.hl.agc) health_report(&m.hl);
		if (m.scan)
			for (int i = 0; i < n; i++) {
				uint32_t f = 0;
				uint64_t hops = 0, held = 0;
				rtlfm_scan_freq(m.scan, i, &f, nullptr, &hops, nullptr, &held);
				fprintf(stderr, "stream %d: %llu hops, %llu buffers held, last on %u Hz\n", i, (unsigned long long)hops,
				        (unsigned long long)held, f + (st.wb_mode ? 16000u : 0u));
			}
		if (m.failed) ret = 3;
		if (!ret && st.keep_file) {
			// behind the last run: the sources that were in the batch to the end, beside the records the others left
			int r = keep_states(&m, m.live, nullptr);
			if (r == 0) r = rtlfm_snapshot_write(st.keep_file, &c, n, m.kept.data(), nullptr);
			if (r < 0) {
				fprintf(stderr, "-K %s: %s\n", st.keep_file, rtlfm_gpu_strerror(r));
				ret = 3;
			}
		}
	}
	if (m.scan) rtlfm_scan_destroy(m.scan);
	if (m.hl.agc) rtlfm_agc_destroy(m.hl.agc);
	for (pid_t pid : m.children) waitpid(pid, nullptr, 0);  // the triggered commands run in the background; none outlives the tool
	if (m.mon) rtlfm_monitor_destroy(m.mon);
	close_all(&m);
	return ret;
}

// ---- -X: K channels per source, one handle of n x K streams over the library's source-indexed ring ------------------
//
// The device side is -N's: on_buffer_multi / dongle_thread_multi, a host queue per source.  The demod thread takes
// b = min(what every live queue holds, max_blocks) buffers from every live source (take_batch) and pushes them with the
// SOURCE's index (option source_ring); a short buffer - a file's last - is completed with bytes 127 to the full length, and
// a source that has ended is fed b buffers of bytes 127, so that every source has one length per buffer index and the
// handle's one sample counter holds for all.  The streams of an ended source write nothing more and count nothing more.
// The run ends with the last source.
// -E srciq after a run: the engine takes every source's records of the run (include/rtlfm_iq.h), says what it decided
// (-v), and its coefficients go to the handle - no wait: they rule from the next run on.
int iq_step(Multi *m)
{
	int r = rtlfm_iq_update(m->iq, m->gpu);
	if (r < 0) return r;
	rtlfm_iq_event ev[16];
	int n = 0;
	bool changed = false;
	do {
		if ((r = rtlfm_iq_poll(m->iq, ev, 16, &n)) < 0) return r;
		for (int k = 0; k < n; k++) {
			if (ev[k].kind == RTLFM_IQ_EVENT_CHANGED) changed = true;
			if (!m->st.verbosity) continue;
			if (ev[k].kind == RTLFM_IQ_EVENT_CHANGED)
				fprintf(stderr, "source %d: iq %d %d %d %d\n", ev[k].source, ev[k].coef[0], ev[k].coef[1], ev[k].coef[2], ev[k].coef[3]);
			else
				fprintf(stderr, "source %d: iq rejected %d %d\n", ev[k].source, ev[k].g_q14, ev[k].s_q14);
		}
	} while (n == 16);
	if (!changed) return 0;
	std::vector<int16_t> coef(m->src.size() * 4);
	if ((r = rtlfm_iq_coeffs(m->iq, coef.data())) < 0) return r;
	return rtlfm_gpu_set_source_iq(m->gpu, coef.data());
}

void demod_thread_channels(Multi *m)
{
	const int n = (int)m->src.size(), K = m->chan_per, S = n * K;
	const uint32_t L = m->st.cfg.block_len;
	const std::vector<uint8_t> silence(L, 127);
	std::vector<int> who((size_t)S), live((size_t)n);
	for (int s = 0; s < S; s++) who[(size_t)s] = s;
	for (int i = 0; i < n; i++) live[(size_t)i] = i;
	std::vector<char> ended((size_t)n, 0);
	for (;;) {
		const int b = take_batch(m, live);
		if (!b) break;
		std::fill(ended.begin(), ended.end(), 1);
		for (int i : live) ended[(size_t)i] = 0;
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
		RunOut o;
		if (!run_and_fetch(m, r, b, who, o)) break;
		if (m->hl.agc) {  // -E srcagc: every live source's b records, each over a full (completed) buffer; an ended source's are not fed
			const std::vector<std::vector<uint32_t>> lens(live.size(), std::vector<uint32_t>((size_t)b, L));
			if ((r = health_step(&m->hl, m->gpu, m->st.cfg.max_blocks, live, lens)) < 0) {
				fail(m, "rtlfm_gpu_source_health_all / rtlfm_agc_feed", r);
				break;
			}
		}
		if (m->iq && (r = iq_step(m)) < 0) {  // -E srciq: this run's records decide the next run's coefficients
			fail(m, "rtlfm_iq_update / rtlfm_gpu_set_source_iq", r);
			break;
		}
		for (int s = 0; s < S; s++)
			if (ended[(size_t)(s / K)]) o.lens[(size_t)s] = 0;
		if (m->st.print_levels)
			for (int s = 0; s < S; s++)
				if (!ended[(size_t)(s / K)]) print_level(m->out[(size_t)s], m->gpu, s, m->st);
		if (m->packed) {  // -l: the rule ran on the device (pack_results 2), a held buffer has left no samples; max_blocks is 1
			for (int s = 0; s < S; s++)
				if (!ended[(size_t)(s / K)]) m->out[(size_t)s].blocks_squelched += (uint64_t)o.held[(size_t)s];
		} else if (m->st.cfg.squelch_level)  // (a configuration pack_results 2 does not take) as -N without the device gate
			hold_back(m->gpu, S, m->st.conseq_squelch, m->states, [&](int s) {
				if (!ended[(size_t)(s / K)]) m->out[(size_t)s].blocks_squelched++;
				o.lens[(size_t)s] = 0;
			});
		deliver(m, o);
	}
	demod_done(m);
}

// -x's filter: rtlfm_channel_lowpass at the cutoff the benchmarks use, 0.4 of the output rate in cycles per capture sample.
// (-ERANGE: fewer taps than the gain D needs at shift 14 - a tap beyond an int16, a short filter at a large D.  The same
// filter at half the scale and one bit less shift has the same DC gain, as long as D stays whole.)  Host arithmetic: -u's
// check asks it before a device is opened, run_channels when it sets the filter.
int plan_chan_filter(const rtlfm_cfg &c, int ntaps, int16_t *taps, int *shift, int *gain_out)
{
	int gain = c.downsample, less = 0;
	int r = rtlfm_channel_lowpass(ntaps, 0.4 / c.downsample, gain, taps, shift);
	while (r == -ERANGE && gain % 2 == 0 && less < 14) {
		gain /= 2;
		less++;
		r = rtlfm_channel_lowpass(ntaps, 0.4 / c.downsample, gain, taps, shift);
	}
	*shift -= less;
	*gain_out = gain;
	return r;
}

// everything after option parsing for -X (main has refused what -X does not allow): freqs[i] = source i's -f as given,
// chan_freqs[i] = its K channel frequencies, each within capture_rate / 2 of freqs[i]
int run_channels(const Settings &st, const std::vector<uint32_t> &freqs, const std::vector<std::vector<uint32_t>> &chan_freqs)
{
	const rtlfm_cfg &c = st.cfg;
	const int n = (int)freqs.size(), K = (int)chan_freqs[0].size(), S = n * K, ntaps = st.chan_taps > 0 ? st.chan_taps : 0;
	Multi m(st, (size_t)n, (size_t)S);
	m.chan_per = K;
	if (!devices_there(st, n, "with " + std::to_string(n) + " sources")) return 1;
	int ret = 0;
	for (int i = 0; i < n && !ret; i++) {
		Source &s = m.src[(size_t)i];
		s.m = &m;
		s.dev = open_source(st, i, st.gain, freqs[(size_t)i]);  // as given: the mixers take the rotation's place
		if (!s.dev) ret = 1;
		else fprintf(stderr, "source %d: device #%d, tuned to %u Hz, streams %d .. %d.\n", i, st.dev_index + i, freqs[(size_t)i], i * K, i * K + K - 1);
	}
	if (!ret) {
		fprintf(stderr, "%d sources x %d channels = %d streams.\nOversampling input by: %ix.\nSampling at %u S/s.\nOutput at %u Hz.\n", n, K, S,
		        c.downsample, st.capture_rate, out_rate(c));
		std::vector<uint32_t> steps((size_t)S);
		for (int s = 0; s < S; s++) {
			const uint32_t cf = chan_freqs[(size_t)(s / K)][(size_t)(s % K)];
			steps[(size_t)s] = rtlfm_channel_step((int32_t)((int64_t)cf - (int64_t)freqs[(size_t)(s / K)]), st.capture_rate);
			if (st.verbosity) fprintf(stderr, "stream %d: source %d, %u Hz, step %u\n", s, s / K, cf, steps[(size_t)s]);
		}
		const char *what = "rtlfm_gpu_create";
		int r = rtlfm_gpu_create(&c, S, 0, &m.gpu);
		if (r == 0) { what = "option source_ring"; r = rtlfm_gpu_set_option(m.gpu, "source_ring", 1); }
		if (r == 0) { what = "rtlfm_gpu_set_channels"; r = rtlfm_gpu_set_channels(m.gpu, K, steps.data()); }
		if (r == 0 && st.source_dc) { what = "option source_dc"; r = rtlfm_gpu_set_option(m.gpu, "source_dc", 1); }
		if (r == 0 && st.source_agc) {
			// (settle = the buffers one run may take, as -O agc=2: they were captured before a change could act)
			what = "option source_health";
			r = rtlfm_gpu_set_option(m.gpu, "source_health", 1);
			std::vector<rtlsdr_dev_t *> devs;
			for (Source &s : m.src) devs.push_back(s.dev);
			m.hl.by_source = true;
			if (r == 0) { what = "rtlfm_agc_create"; r = health_create(&m.hl, devs, c.max_blocks, st.verbosity); }
		}
		if (r == 0 && st.source_iq) {
			what = "option source_iq";
			r = rtlfm_gpu_set_option(m.gpu, "source_iq", 1);
			if (r == 0) { what = "rtlfm_iq_create"; r = rtlfm_iq_create(n, &m.iq); }
		}
		if (r == 0 && c.squelch_level) {
			// -l: demod_thread_fn's rule on the device, and only what it let through comes back.  (-ENOTSUP, behind a
			// resampler: the rule from the carried state after every run, hold_back.)
			what = "option pack_results";
			r = rtlfm_gpu_set_option(m.gpu, "conseq_squelch", st.conseq_squelch);
			if (r == 0) r = rtlfm_gpu_set_option(m.gpu, "pack_results", 2);
			m.packed = r == 0;
			if (r == -ENOTSUP) r = 0;
		}
		if (r == 0 && ntaps > 0) {
			std::vector<int16_t> taps((size_t)ntaps);
			int shift = 0, gain = 0;
			what = "rtlfm_channel_lowpass";
			r = plan_chan_filter(c, ntaps, taps.data(), &shift, &gain);
			if (r == 0 && (gain != c.downsample || st.verbosity)) fprintf(stderr, "-x %d: gain %d at shift %d\n", ntaps, gain, shift);
			if (r == 0) { what = "rtlfm_gpu_set_channel_filter"; r = rtlfm_gpu_set_channel_filter(m.gpu, taps.data(), ntaps, shift); }
		}
		if (r == 0 && st.chan_resume_file) {  // -u: in front of the first buffer, behind everything that clears
			what = st.chan_resume_file;
			r = rtlfm_gpu_channels_load(m.gpu, st.chan_resume_file);
			if (r < 0) fprintf(stderr, "-u ");
		}
		if (r < 0) {
			fprintf(stderr, "%s: %s\n", what, rtlfm_gpu_strerror(r));
			ret = 2;
		}
	}
	for (int s = 0; s < S && !ret; s++)
		if (!m.out[(size_t)s].open(st, s, chan_freqs[(size_t)(s / K)][(size_t)(s % K)])) ret = 1;
	if (!ret) {
		run_threads(&m, demod_thread_channels);
		uint64_t in = 0;
		for (Source &s : m.src) in += s.blocks_in;
		summary(m.out.data(), m.out.size(), in, nullptr, m.failed, st.verbosity > 0);
		if (m.hl.agc) health_report(&m.hl);
		if (m.iq && st.verbosity) {  // -E srciq: where every source ended up
			std::vector<int16_t> coef((size_t)n * 4);
			if (rtlfm_iq_coeffs(m.iq, coef.data()) == 0)
				for (int i = 0; i < n; i++)
					fprintf(stderr, "source %d: iq %d %d %d %d at exit\n", i, coef[(size_t)i * 4], coef[(size_t)i * 4 + 1], coef[(size_t)i * 4 + 2],
					        coef[(size_t)i * 4 + 3]);
		}
		if (m.failed) ret = 3;
		if (!ret && st.chan_keep_file) {  // -k: behind the last run
			const int r = rtlfm_gpu_channels_save(m.gpu, st.chan_keep_file);
			if (r < 0) {
				fprintf(stderr, "-k %s: %s\n", st.chan_keep_file, rtlfm_gpu_strerror(r));
				ret = 3;
			}
		}
	}
	if (m.hl.agc) rtlfm_agc_destroy(m.hl.agc);
	if (m.iq) rtlfm_iq_destroy(m.iq);
	close_all(&m);
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

// -u: the channel snapshot against what the command line plans, before a device is opened: 0, or the exit status (2) behind
// the library's text.  The handle makes the same comparison again when it loads the file (rtlfm_gpu_channels_load).
int check_chan_resume(const char *path, const Settings &st, int nstreams, int K)
{
	const rtlfm_cfg &planned = st.cfg;
	const int ntaps = st.chan_taps > 0 ? st.chan_taps : 0;
	rtlfm_chansnap_hdr hd;
	rtlfm_cfg saved;
	int r = rtlfm_chansnap_info(path, &hd, &saved);
	if (r == 0 && hd.nstreams != (uint32_t)nstreams) r = -ERANGE;
	if (r == 0) {
		saved.max_blocks = planned.max_blocks;        // how much a run takes and what it reports, not what a stream carries
		saved.report_levels = planned.report_levels;
		const bool dc = (hd.flags & RTLFM_CHANSNAP_FLAG_SOURCE_DC) != 0;
		if (memcmp(&saved, &planned, sizeof(saved)) != 0 || hd.per_source != (uint32_t)K || dc != st.source_dc || hd.bank_K != 0 ||
		    hd.fir_ntaps != (uint32_t)ntaps)
			r = -EMEDIUMTYPE;
	}
	if (r == 0 && ntaps > 0) {
		std::vector<int16_t> want((size_t)ntaps), got((size_t)ntaps);
		int shift = 0, gain = 0;
		rtlfm_chansnap_bufs b{};
		b.fir_taps = got.data();
		b.cap_fir_taps = got.size();
		r = plan_chan_filter(planned, ntaps, want.data(), &shift, &gain);
		if (r == 0) r = rtlfm_chansnap_read(path, nullptr, &b);
		if (r == 0 && ((uint32_t)shift != hd.fir_shift || memcmp(want.data(), got.data(), got.size() * sizeof(int16_t)) != 0)) r = -EMEDIUMTYPE;
	}
	if (r == 0) return 0;
	fprintf(stderr, "-u %s: %s\n", path, rtlfm_gpu_strerror(r));
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
	        "\t       down on the GPU; stream s = channel s %% K of source s / K writes the file with %%d = s; not with -S -C -K -R -Z (-k / -u keep and take up),\n"
	        "\t       -O agc=2 or -E rdc; -E srcdc takes every source's DC spike off in front of the mixers (-q sets its constant);\n"
	        "\t       -E srcagc is the software AGC for every SOURCE from the GPU's records of its raw bytes (-v prints every change; not with agc= in -O);\n"
	        "\t       -E srciq is rtl_tcp -c for every SOURCE: its I/Q gain and phase mismatch measured and corrected on the GPU, so that no channel\n"
	        "\t       hears its mirror channel (-v prints every change of the four Q14 coefficients)]\n"
	        "\t[-x ntaps  with -X: a windowed-sinc channel filter of ntaps taps (cutoff 0.4 of the output rate) in the boxcar's place; not with -F]\n"
	        "\t[-k file  with -X: keep - write everything the handle carries (every stream's state, the sample counter, every source's\n"
	        "\t       history) to a channel snapshot at exit;  -u file  with -X: take up - load such a file before the first buffer; it must come\n"
	        "\t       from the same -N / -X (K) / -x / -E srcdc / -M / -s ... plan, else exit 2; the output continues as if the tool had never\n"
	        "\t       stopped.  Not without -X (there: -K / -R), not with -S, -C or -E srcagc: those engines carry state the file does not hold]\n"
	        "\t[-K file  keep: write every stream's carried filter state to file at exit (with -N n: n records, in source order)]\n"
	        "\t[-R file  resume: load such a file before the first buffer - it must hold as many records as there are sources and\n"
	        "\t       come from the same -M / -s / -r / -F / -A / -E / -l / -W ... plan, else exit 2; the output continues as if the tool had\n"
	        "\t       never stopped.  -K / -R not with -S, -C or -O agc=2: those engines carry state the file does not hold]\n"
	        "\t[-M modulation (default: fm)]  fm, wbfm, raw, am, usb, lsb\n"
	        "\t[-s sample_rate (default: 24k)]  [-r resample_rate (default: none / same as -s)]\n"
	        "\t[-m minimum_capture_rate Hz (default: 1m)]\n"
	        "\t[-F fir_size (default: off)]  enables the fifth-order low pass; 0 or 9 (9 = droop compensation)\n"
	        "\t[-A std/fast/lut choose atan math (default: std)]\n"
	        "\t[-E enable_option]  edge, dc, rdc, deemp, offset, srcdc (with -X only; not with rdc), srcagc (with -X only; not with agc= in -O),\n"
	        "\t                    srciq (with -X only)\n"
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
	Settings st;
	rtlfm_cfg_default(&st.cfg);
	rtlfm_cfg &c = st.cfg;
	uint32_t freq = 0;
	std::vector<uint32_t> freqs;  // every -f, in order (-N)
	int nstreams = 1;
	bool have_freq = false;
	c.rate_out = 24000;
	c.max_blocks = 8;
	int opt;
	while ((opt = getopt(argc, argv, "d:f:g:s:l:o:t:r:p:E:F:A:M:hm:L:q:c:W:HvZN:C:O:S:K:R:X:x:k:u:")) != -1) {
		switch (opt) {
		case 'd': st.dev_index = atoi(optarg); break;
		case 'f': freq = (uint32_t)atofs(optarg); freqs.push_back(freq); have_freq = true; break;
		case 'N': nstreams = atoi(optarg); break;
		case 'C': st.cmd_file = optarg; break;
		case 'S': st.scan_file = optarg; break;
		case 'K': st.keep_file = optarg; break;
		case 'R': st.resume_file = optarg; break;
		case 'X': st.chan_file = optarg; break;
		case 'x': st.chan_taps = atoi(optarg); break;
		case 'k': st.chan_keep_file = optarg; break;
		case 'u': st.chan_resume_file = optarg; break;
		case 'O':
			st.opt_string = optarg;
			st.agc = opt_string_agc(optarg);
			if (st.agc == -2) {
				fprintf(stderr, "-O %s: agc= takes 0 (hardware AGC), 1 (manual) or 2 (software AGC).\n", optarg);
				return 1;
			}
			break;
		case 'g': st.gain = (int)(atof(optarg) * 10); break;
		case 'p': st.ppm = (int)atof(optarg); break;
		case 'm': st.min_capture = (int)atofs(optarg); break;
		case 'l': c.squelch_level = (int)atof(optarg); break;
		case 'L': st.print_levels = (int)atof(optarg); break;
		case 't':  // src/rtl_fm.c:1774-1781 (a negative value also asks to terminate on squelch: not restated)
			st.conseq_squelch = (int)atof(optarg);
			if (st.conseq_squelch < 0) st.conseq_squelch = -st.conseq_squelch;
			break;
		case 's': st.rate_in = (int)atofs(optarg); c.rate_out = st.rate_in; break;
		case 'r': c.rate_out2 = (int)atofs(optarg); break;
		case 'o': c.post_downsample = (int)atof(optarg); break;
		case 'q': c.rdc_block_const = atoi(optarg); break;
		case 'E':
			if (!strcmp(optarg, "edge")) st.edge = 1;
			if (!strcmp(optarg, "dc") || !strcmp(optarg, "adc")) c.dc_block_audio = 1;
			if (!strcmp(optarg, "rdc")) c.dc_block_raw = 1;
			if (!strcmp(optarg, "srcdc")) st.source_dc = true;
			if (!strcmp(optarg, "srcagc")) st.source_agc = true;
			if (!strcmp(optarg, "srciq")) st.source_iq = true;
			if (!strcmp(optarg, "deemp")) c.deemph = 1;
			if (!strcmp(optarg, "offset")) c.offset_tuning = 1;
			break;
		case 'F': st.fifth = 1; c.comp_fir_size = atoi(optarg); break;
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
				st.rate_in = 170000; c.rate_out = 170000; c.rate_out2 = 32000;
				c.custom_atan = RTLFM_ATAN_FAST;
				c.deemph = 1;
				c.squelch_level = 0;
				st.wb_mode = true;
			}
			break;
		case 'c':
			if (!strcmp(optarg, "us")) st.time_constant = 75;
			else if (!strcmp(optarg, "eu")) st.time_constant = 50;
			else st.time_constant = (int)atof(optarg);
			break;
		case 'W': {
			long v = 512L * atoi(optarg);
			if (v > (long)RTLFM_MAX_BLOCK_LEN) v = RTLFM_MAX_BLOCK_LEN;  // src/rtl_fm.c:1869-1873
			c.block_len = (uint32_t)v;
			break;
		}
		case 'H': st.write_wav = true; break;
		case 'Z': st.zero_copy = true; break;
		case 'v': st.verbosity++; break;
		default: usage();
		}
	}
	if (st.source_dc && c.dc_block_raw) {
		fprintf(stderr, "-E srcdc (raw DC block per source, with -X) does not go with -E rdc (raw DC block per stream): choose one.\n");
		return 1;
	}
	if (st.source_dc && !st.chan_file) {
		fprintf(stderr, "-E srcdc (raw DC block per source) needs -X (the channel file): it acts in front of the channels' mixers only; "
		                "without channels -E rdc is the raw DC block.\n");
		return 1;
	}
	if (st.source_agc && !st.chan_file) {
		fprintf(stderr, "-E srcagc (software AGC per source) needs -X (the channel file): it reads the records of the sources' raw bytes "
		                "that only a handle with channels takes; without channels -O agc=2 is the software AGC.\n");
		return 1;
	}
	if (st.source_iq && !st.chan_file) {
		fprintf(stderr, "-E srciq (IQ balance per source) needs -X (the channel file): it measures and rewrites the sources' raw bytes "
		                "in front of the channels' mixers, which only a handle with channels does.\n");
		return 1;
	}
	if (st.source_agc && st.agc != -1) {
		fprintf(stderr, "-E srcagc (software AGC per source, gain mode 2 on every device) does not go with agc=%d in -O: one of them "
		                "sets the devices' gain mode.\n", st.agc);
		return 1;
	}
	if (st.chan_taps != -1 && !st.chan_file) {
		fprintf(stderr, "-x (taps of the channel filter) needs -X (the channel file): the filter acts on channels only.\n");
		return 1;
	}
	if (st.chan_keep_file || st.chan_resume_file) {
		// before a device is opened - and before -X's own refusals, so that the line names both letters
		const char *me = st.chan_keep_file ? "-k (keep the channels' carried state)" : "-u (take up the channels' carried state)";
		if (!st.chan_file) {
			fprintf(stderr, "%s needs -X (the channel file): a channel snapshot holds what a handle with channels carries; "
			                "for independent streams the letters are -K / -R.\n", me);
			return 1;
		}
		const char *with = st.scan_file ? "-S (scan lists)" : st.cmd_file ? "-C (command file)" : st.source_agc ? "-E srcagc (software AGC per source)"
		                   : st.source_iq ? "-E srciq (IQ balance per source)" : nullptr;
		if (with) {
			fprintf(stderr, "%s does not go with %s: -k / -u do not go with -S, -C, -E srcagc or -E srciq, those engines carry state of their own "
			                "that the file does not hold.\n", me, with);
			return 1;
		}
	}
	if (st.chan_file) {
		// everything -X refuses for what it is combined with is refused here, before a device is opened or a handle created:
		// each of these needs what the library refuses while channels are on (include/rtlfm_hip.h, rtlfm_gpu_set_channels)
		const char *with = nullptr, *why = nullptr;
		if (st.scan_file) { with = "-S (scan lists)"; why = "a hop needs the hop mute and the squelch gate, which read per-stream input rows"; }
		else if (st.cmd_file) { with = "-C (command file)"; why = "the monitor needs the option input_stats, which reads per-stream input rows"; }
		else if (st.keep_file) { with = "-K (keep)"; why = "a snapshot does not hold the channels' sample counter"; }
		else if (st.resume_file) { with = "-R (resume)"; why = "a snapshot does not hold the channels' sample counter"; }
		else if (st.zero_copy) { with = "-Z (zero-copy)"; why = "the ring is filled from the sources' host queues, in lockstep"; }
		else if (st.agc == 2) { with = "-O agc=2 (software AGC)"; why = "it needs the option input_health, which reads per-stream input rows"; }
		else if (c.dc_block_raw) { with = "-E rdc (raw DC block)"; why = "it rides on the rotation's kernel, whose place the mixers take"; }
		else if (st.chan_taps != -1 && st.fifth) { with = "-x (channel filter) with -F (fifth-order low pass)"; why = "the channel filter stands in the boxcar's place, and -F leaves no boxcar"; }
		if (with) {
			fprintf(stderr, "-X (channel file) does not go with %s: %s.\n", with, why);
			return 1;
		}
		if (st.chan_taps != -1 && (st.chan_taps < 1 || st.chan_taps > RTLFM_CHANNEL_MAX_TAPS)) {
			fprintf(stderr, "-x %d with -X: the channel filter takes 1 .. %d taps.\n", st.chan_taps, RTLFM_CHANNEL_MAX_TAPS);
			return 1;
		}
	}
	if ((st.keep_file || st.resume_file) && (st.scan_file || st.cmd_file || st.agc == 2)) {
		// before a device is opened: the hop engine, the monitor and the software AGC carry state of their own
		fprintf(stderr, "-K / -R (keep / resume the carried state) do not go with -S, -C or -O agc=2: those engines carry state of "
		                "their own that the snapshot does not hold.\n");
		return 1;
	}
	int bad_line = 0;
	std::vector<std::vector<uint32_t>> scan_lists;
	if (st.scan_file) {
		// everything -S refuses is refused here, before a device is opened
		if (nstreams < 1) { fprintf(stderr, "-N wants a number of streams >= 1.\n"); usage(); }
		if (st.cmd_file) { fprintf(stderr, "-S (scan lists) and -C (command file) exclude each other.\n"); usage(); }
		if (!c.squelch_level) { fprintf(stderr, "Please specify a squelch level.  Required for scanning multiple frequencies.\n"); return 1; }  // src/rtl_fm.c:1693
		const int lr = read_list_file(st.scan_file, scan_lists, nullptr, &bad_line);
		if (lr == -ENOENT) { fprintf(stderr, "-S %s: cannot open the scan file\n", st.scan_file); usage(); }
		if (lr < 0) { fprintf(stderr, "-S %s: line %d is no frequency list\n", st.scan_file, bad_line); usage(); }
		if ((int)scan_lists.size() != nstreams) {
			fprintf(stderr, "-S %s holds %zu lists, -N %d needs exactly %d: line i of the file is the list of source i.\n", st.scan_file,
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
	if (st.cmd_file) {
		// src/rtl_fm.c:1738-1741: the command file implies -M raw; here its lines are the -N sources, in order
		if (nstreams < 1) { fprintf(stderr, "-N wants a number of streams >= 1.\n"); usage(); }
		rules.resize((size_t)nstreams);
		int found = 0;
		const int pr = rtlfm_monitor_parse_file(st.cmd_file, rules.data(), nstreams, &found, nullptr, nullptr);
		if (pr < 0 && pr != -ENOBUFS) {
			fprintf(stderr, "-C %s: %s\n", st.cmd_file, pr == -ENOENT ? "cannot open the command file" : "no valid measurement line");
			usage();
		}
		if (found != nstreams) {
			fprintf(stderr, "-C %s holds %d measurement lines, -N %d needs exactly %d: line i of the file is watched by source i.\n",
			        st.cmd_file, found, nstreams, nstreams);
			usage();
		}
		c.mode = RTLFM_MODE_RAW;
		c.report_levels = 1;
		c.max_blocks = 1;  // as -L: one buffer per run, so that a source's short last buffer keeps its place among the levels
		freqs.clear();
		for (const rtlfm_monitor_rule &r : rules) freqs.push_back(r.freq);
		freq = freqs[0];
		have_freq = true;
		st.wb_mode = false;
	}
	if (!have_freq) { fprintf(stderr, "Please specify a frequency.\n"); return 1; }
	if (st.wb_mode) freq += 16000;  // controller_thread_fn(), src/rtl_fm.c:1455-1460: "wbfm: adding 16000 Hz to every input frequency"
	if (c.squelch_level) c.max_blocks = 1;  // the squelch rule (hold_back) is the reference's per-buffer rule
	if (st.print_levels > 0) { c.report_levels = 1; c.max_blocks = 1; }
	st.rate_in *= c.post_downsample;  // src/rtl_fm.c:1886
	if (optind < argc) st.filename = argv[optind];
	const std::string pattern(st.filename);
	const size_t at = pattern.find("%d");
	const bool two = at != std::string::npos && pattern.find("%d", at + 2) != std::string::npos;  // more than one %d

	if (nstreams < 1) { fprintf(stderr, "-N wants a number of streams >= 1.\n"); usage(); }
	if (st.chan_file) {
		// -X: the file, the names and the plan, all before a device is opened or a GPU handle created
		std::vector<std::vector<uint32_t>> chan_freqs;
		std::vector<int> chan_lineno;
		const int lr = read_list_file(st.chan_file, chan_freqs, &chan_lineno, &bad_line);
		if (lr == -ENOENT) { fprintf(stderr, "-X %s: cannot open the channel file\n", st.chan_file); return 1; }
		if (lr < 0) { fprintf(stderr, "-X %s: line %d is no frequency list\n", st.chan_file, bad_line); return 1; }
		if ((int)chan_freqs.size() != nstreams) {
			fprintf(stderr, "-X %s holds %zu lists, -N %d needs exactly %d: line i of the file is the channel list of source i.\n", st.chan_file,
			        chan_freqs.size(), nstreams, nstreams);
			return 1;
		}
		for (size_t i = 1; i < chan_freqs.size(); i++)
			if (chan_freqs[i].size() != chan_freqs[0].size()) {
				fprintf(stderr, "-X %s: line %d stands for %zu channels and line %d for %zu; every source needs the same number of channels "
				        "(-N sources share one handle).\n", st.chan_file, chan_lineno[i], chan_freqs[i].size(), chan_lineno[0], chan_freqs[0].size());
				return 1;
			}
		const size_t total = chan_freqs.size() * chan_freqs[0].size();
		if (freqs.size() != 1 && freqs.size() != (size_t)nstreams) {
			fprintf(stderr, "-X with -N %d: give -f once (every source) or %d times (one per source), not %zu times.\n", nstreams, nstreams,
			        freqs.size());
			return 1;
		}
		if (freqs.size() == 1) freqs.assign((size_t)nstreams, freqs[0]);
		if (total > 1 && (at == std::string::npos || two)) {
			fprintf(stderr, "-X with %zu streams: the filename must hold exactly one %%d (the stream index), e.g. out_%%d.raw.\n", total);
			return 1;
		}
		if (pattern == "-" || (total == 1 && two)) {
			fprintf(stderr, "-X: no stdout and at most one %%d; name the files, e.g. out_%%d.raw.\n");
			return 1;
		}
		// one plan for all sources, as under -N; a source's capture frequency is its -f as given (no capture_rate / 4 offset,
		// no +16 kHz under -M wbfm)
		if (const int i = plan_for_all(st, freqs, nullptr)) {
			fprintf(stderr, "-X: the rate plan for %u Hz differs from the one for %u Hz; one handle needs one plan.\n", freqs[(size_t)i], freqs[0]);
			return 1;
		}
		for (size_t i = 0; i < chan_freqs.size(); i++)
			for (size_t k = 0; k < chan_freqs[i].size(); k++) {
				const int64_t off = (int64_t)chan_freqs[i][k] - (int64_t)freqs[i];
				if (2 * (off < 0 ? -off : off) > (int64_t)st.capture_rate) {
					fprintf(stderr, "-X %s: line %d, entry %zu: %u Hz is further than capture_rate / 2 = %u Hz from the -f of source %zu, %u Hz.\n",
					        st.chan_file, chan_lineno[i], k + 1, chan_freqs[i][k], st.capture_rate / 2, i, freqs[i]);
					return 1;
				}
			}
		if (st.chan_resume_file)
			if (const int r = check_chan_resume(st.chan_resume_file, st, (int)total, (int)chan_freqs[0].size())) return r;
		return run_channels(st, freqs, chan_freqs);
	}
	const bool multi = nstreams > 1 || st.cmd_file || st.scan_file;
	if (multi) {
		// everything -N refuses is refused here, before a device is opened or a GPU handle created
		if (freqs.size() != 1 && freqs.size() != (size_t)nstreams) {
			fprintf(stderr, "-N %d: give -f once (every device) or %d times (one per device), not %zu times.\n", nstreams,
			        nstreams, freqs.size());
			usage();
		}
		if (pattern == "-") { fprintf(stderr, "-N %d: no stdout; name the files, e.g. out_%%d.raw.\n", nstreams); usage(); }
		if (nstreams == 1 && st.scan_file && at == std::string::npos) {
			// one source: the name as it is
		} else if (at == std::string::npos || two) {
			fprintf(stderr, "-N %d: the filename must hold exactly one %%d (the stream index), e.g. out_%%d.raw.\n", nstreams);
			usage();
		}
		if (st.zero_copy) {
			// -Z writes a device's buffer straight into the ring, but with -N the ring is filled from the host
			// queues (run_multi): there is no slot a device could own
			fprintf(stderr, "-Z (zero-copy) works with one stream only, not with -N %d.\n", nstreams);
			usage();
		}
		if (freqs.size() == 1) freqs.assign((size_t)nstreams, freqs[0]);
		if (st.wb_mode)
			for (uint32_t &f : freqs) f += 16000;  // the -M wbfm rule above, for every device
	} else {
		freqs.assign(1, freq);  // one source: the last -f
	}
	// the plan the handle will be created with, and -R's file against it, before a device is opened (optimal_settings() and
	// deemph_a are host arithmetic)
	std::vector<uint32_t> capture_freqs;
	if (const int i = plan_for_all(st, freqs, &capture_freqs)) {
		fprintf(stderr, "-N: the rate plan for %u Hz differs from the one for %u Hz; one handle needs one plan.\n", freqs[(size_t)i], freqs[0]);
		return 1;
	}
	if (st.resume_file)
		if (const int r = check_resume(st.resume_file, c, nstreams)) return r;
	return multi ? run_multi(st, freqs, capture_freqs, rules, scan_lists) : run_single(st, freq, capture_freqs[0]);
}
