// rtl_power_hip — an rtl_power-shaped command line over the C ABI.
//
// Same flow as the reference tool (src/rtl_power.c:767-1028): parse -f lower:upper:bin
// (:802-806), plan the hops with frequency_range (:438-540), then repeat scanner()
// (:642-720) — retune, rtlsdr_read_sync one buffer per hop, accumulate — and every
// `interval` seconds print one csv_dbm line per hop (:722-765, :992-1003).  The DSP of
// scanner() is rtlpower_gpu_scan(); every hop is one stream of the handle.
// Deterministic replay: RTLPOWER_PASSES=<n> reports after exactly n passes over the
// hops instead of by wall clock (the file device has no real-time pacing).
//
// -N n out_%d.csv: devices d .. d+n-1 (RTLSDR_FILE_LIST, one source per line) all scan the same -f plan
// through ONE handle; stream source * tune_count + hop.  One reader thread per source retunes and calls
// rtlsdr_read_sync once per hop into its rows of one staging batch; a pass over the hops is one
// rtlpower_gpu_scan_host, a report is one rtlpower_gpu_report(clear = 1) - csv_dbm()'s arithmetic and reset
// on the device - and one line per source and hop into that source's file, every source of a report
// with the same timestamp.  A source that delivers a short read ends the run for ALL sources after the
// last complete report.  (The reference says "Error: dropped samples." and goes on with what it got,
// src/rtl_power.c:658-659; this tool ends there, with or without -N, and under -N the other sources end
// with it, because a report covers every source.  The two paths differ in what they still write: without -N
// and without RTLPOWER_PASSES the single-source path prints one last report of the passes since the previous
// one, the incomplete pass included; the -N path never does, in wall-clock mode either: what was scanned
// after the last complete report is dropped.)  -N refuses -c 100% (no bin would be left; rtlpower_gpu_report
// takes 0 <= crop < 1).  Without -N the tool
// is the single-device program it was: rtlpower_gpu_scan / _fetch / rtlpower_csv_dbm / _clear.
#include <getopt.h>
#include <cmath>

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/rtlpower_hip.h"
#include "../../../include/rtlsdr_file.h"

static double atofs(const std::string &s)
{
	// src/convenience/convenience.c:67-96
	std::string t(s);
	double mul = 1.0;
	if (!t.empty()) switch (t.back()) {
	case 'g': case 'G': mul = 1e9; t.pop_back(); break;
	case 'm': case 'M': mul = 1e6; t.pop_back(); break;
	case 'k': case 'K': mul = 1e3; t.pop_back(); break;
	default: break;
	}
	return mul * atof(t.c_str());
}
static double atoft(const std::string &s)
{
	// src/convenience/convenience.c:98-124
	std::string t(s);
	double mul = 1.0;
	if (!t.empty()) switch (t.back()) {
	case 'h': case 'H': mul = 3600; t.pop_back(); break;
	case 'm': case 'M': mul = 60; t.pop_back(); break;
	case 's': case 'S': mul = 1; t.pop_back(); break;
	default: break;
	}
	return mul * atof(t.c_str());
}
static double atofp(const std::string &s)
{
	// src/convenience/convenience.c:126-144
	if (!s.empty() && s.back() == '%') return 0.01 * atof(s.substr(0, s.size() - 1).c_str());
	return atof(s.c_str());
}

// ---- -N: n sources, one handle --------------------------------------------------------

// the reader threads and main() meet twice per pass: "go" and "all rows are in"
struct Rendezvous {
	std::mutex m;
	std::condition_variable cv;
	int waiting = 0, parties = 0;
	unsigned long generation = 0;
	void arrive()
	{
		std::unique_lock<std::mutex> l(m);
		const unsigned long g = generation;
		if (++waiting == parties) { waiting = 0; generation++; cv.notify_all(); }
		else cv.wait(l, [&] { return generation != g; });
	}
};

static int run_sources(int n, int dev_index, const rtlpower_plan &plan, const rtlpower_cfg &cfg, const std::string &pattern,
                       int interval, int single, time_t exit_after)
{
	const uint32_t count = rtlsdr_get_device_count();
	if ((uint32_t)(dev_index + n) > count) {
		fprintf(stderr, "-d %d -N %d needs devices %d .. %d, and there are %u (RTLSDR_FILE_LIST: one source per line).\n", dev_index, n,
		        dev_index, dev_index + n - 1, count);
		return 1;
	}
	const size_t at = pattern.find("%d");
	if (at == std::string::npos || pattern.find("%d", at + 2) != std::string::npos) {
		fprintf(stderr, "-N %d: the filename must hold exactly one %%d (the source index), e.g. out_%%d.csv.\n", n);
		return 1;
	}
	const int T = plan.tune_count, S = n * T, bins = 1 << plan.bin_e;
	std::vector<rtlsdr_dev_t *> devs((size_t)n, nullptr);
	std::vector<FILE *> files((size_t)n, nullptr);
	for (int i = 0; i < n; i++) {
		if (rtlsdr_open(&devs[(size_t)i], (uint32_t)(dev_index + i)) < 0) {
			fprintf(stderr, "Failed to open rtlsdr device #%d.\n", dev_index + i);
			return 1;
		}
		const std::string name = pattern.substr(0, at) + std::to_string(i) + pattern.substr(at + 2);
		if (!(files[(size_t)i] = fopen(name.c_str(), "wb"))) { fprintf(stderr, "Failed to open %s\n", name.c_str()); return 1; }
		rtlsdr_reset_buffer(devs[(size_t)i]);
		rtlsdr_set_sample_rate(devs[(size_t)i], (uint32_t)plan.rate);
	}
	rtlpower_gpu *gpu = nullptr;
	int r = rtlpower_gpu_create(&cfg, S, 0, &gpu);
	if (r < 0) { fprintf(stderr, "rtlpower_gpu_create: %d\n", r); return 2; }
	fprintf(stderr, "%d sources x %d hops: %d streams of one handle.\n", n, T, S);

	const size_t L = (size_t)plan.buf_len;
	std::vector<uint8_t> batch((size_t)S * L);  // stream s = source * T + hop, one read each
	std::vector<char> short_read((size_t)n, 0);
	bool quit = false;  // written by main() between two rendezvous only
	Rendezvous rv;
	rv.parties = n + 1;
	std::vector<std::thread> readers;
	for (int i = 0; i < n; i++)
		readers.emplace_back([&, i] {
			for (;;) {
				rv.arrive();  // go
				if (quit) return;
				// scanner()'s device half, one read per hop (src/rtl_power.c:650-661)
				for (int hop = 0; hop < T && !short_read[(size_t)i]; hop++) {
					const int f = rtlpower_tune_freq(&plan, hop);
					if ((int)rtlsdr_get_center_freq(devs[(size_t)i]) != f) rtlsdr_set_center_freq(devs[(size_t)i], (uint32_t)f);
					int n_read = 0;
					rtlsdr_read_sync(devs[(size_t)i], batch.data() + ((size_t)i * T + hop) * L, plan.buf_len, &n_read);
					if (n_read != plan.buf_len) short_read[(size_t)i] = 1;
				}
				rv.arrive();  // all rows are in
			}
		});

	const char *pe = getenv("RTLPOWER_PASSES");
	const int passes_per_report = pe ? atoi(pe) : 0;
	const size_t width = (size_t)bins + 1;
	std::vector<int32_t> centi((size_t)S * width), lens((size_t)S), samples((size_t)S);
	std::vector<char> line((size_t)bins * 16 + 256);
	time_t next_tick = time(nullptr) + interval;
	if (exit_after) exit_after += time(nullptr);
	int passes = 0, rc = 0;
	for (bool stop = false; !stop;) {
		rv.arrive();
		rv.arrive();
		for (int i = 0; i < n; i++)
			if (short_read[(size_t)i]) { fprintf(stderr, "Error: dropped samples (source %d).\n", i); stop = true; }
		if (stop) break;  // the pass is incomplete: nothing of it is scanned, nothing more is reported
		r = rtlpower_gpu_scan_host(gpu, batch.data(), L, 1);
		if (r < 0) { fprintf(stderr, "rtlpower_gpu_scan_host: %d\n", r); rc = 2; break; }
		passes++;
		const time_t now = time(nullptr);
		if (!(passes_per_report ? (passes % passes_per_report == 0) : (now >= next_tick))) continue;
		char t_str[50];
		strftime(t_str, sizeof(t_str), "%Y-%m-%d, %H:%M:%S", localtime(&now));
		r = rtlpower_gpu_report(gpu, (double)plan.rate, plan.crop, 1);  // csv_dbm() of every stream, reset included (:722-765)
		if (r == 0) r = rtlpower_gpu_report_fetch_all(gpu, centi.data(), width, lens.data(), samples.data());
		if (r < 0) { fprintf(stderr, "rtlpower_gpu_report: %d\n", r); rc = 2; break; }
		for (int i = 0; i < n; i++) {
			for (int hop = 0; hop < T; hop++) {
				const size_t s = (size_t)i * T + hop;
				if (lens[s] == 0) continue;  // (never scanned: no line, as without -N)
				if (rtlpower_csv_report(&plan, hop, centi.data() + s * width, lens[s], samples[s], line.data(), line.size()) > 0)
					fprintf(files[(size_t)i], "%s, %s", t_str, line.data());
			}
			fflush(files[(size_t)i]);
		}
		while (time(nullptr) >= next_tick) next_tick += interval;
		if (single) stop = true;
		if (exit_after && time(nullptr) >= exit_after) stop = true;
	}
	quit = true;
	rv.arrive();
	for (auto &t : readers) t.join();
	for (int i = 0; i < n; i++) { fclose(files[(size_t)i]); rtlsdr_close(devs[(size_t)i]); }
	rtlpower_gpu_destroy(gpu);
	return rc;
}

int main(int argc, char **argv)
{
	std::string freq_arg;
	int interval = 10, single = 0, window = RTLPOWER_WIN_RECTANGLE, boxcar = 1, comp_fir = 0, peak_hold = 0;
	int dev_index = 0, nsources = 0;
	double crop = 0.0;
	time_t exit_after = 0;
	int opt;
	while ((opt = getopt(argc, argv, "f:i:s:t:d:g:p:e:w:c:F:N:1POhTD:")) != -1) {
		switch (opt) {
		case 'f': freq_arg = optarg; break;
		case 'd': dev_index = atoi(optarg); break;
		case 'c': crop = atofp(optarg); break;
		case 'i': interval = (int)round(atoft(optarg)); break;
		case 'e': exit_after = (time_t)((int)round(atoft(optarg))); break;
		case 'w':
			if (!strcmp(optarg, "rectangle")) window = RTLPOWER_WIN_RECTANGLE;
			if (!strcmp(optarg, "hamming")) window = RTLPOWER_WIN_HAMMING;
			if (!strcmp(optarg, "blackman")) window = RTLPOWER_WIN_BLACKMAN;
			if (!strcmp(optarg, "blackman-harris")) window = RTLPOWER_WIN_BLACKMAN_HARRIS;
			if (!strcmp(optarg, "hann-poisson")) window = RTLPOWER_WIN_HANN_POISSON;
			if (!strcmp(optarg, "youssef")) window = RTLPOWER_WIN_YOUSSEF;
			if (!strcmp(optarg, "kaiser")) window = RTLPOWER_WIN_KAISER;
			if (!strcmp(optarg, "bartlett")) window = RTLPOWER_WIN_BARTLETT;
			break;
		case 'F': boxcar = 0; comp_fir = atoi(optarg); break;  // src/rtl_power.c:866-869
		case 'P': peak_hold = 1; break;
		case 'N': nsources = atoi(optarg); break;
		case '1': single = 1; break;
		case 'g': case 'p': case 's': case 't': case 'O': case 'T': case 'D': break;  // device-side knobs
		default:
			fprintf(stderr, "rtl_power_hip -f lower:upper:bin_size [-i interval] [-1] [-c crop] [-w window] [-F 0|9] [-P] [-d device] [file]\n"
			                "rtl_power_hip -N n ... out_%%d.csv   devices d .. d+n-1 (RTLSDR_FILE_LIST) scan the same plan through one handle,\n"
			                "                                    one CSV file per source (%%d = source index); -c below 100%%\n");
			return 1;
		}
	}
	size_t c1 = freq_arg.find(':'), c2 = freq_arg.rfind(':');
	if (freq_arg.empty() || c1 == std::string::npos || c2 == c1) { fprintf(stderr, "No frequency range provided.\n"); return 1; }
	if (crop < 0.0 || crop > 1.0) { fprintf(stderr, "Crop value outside of 0 to 1.\n"); return 1; }
	rtlpower_plan plan;
	int r = rtlpower_frequency_range((int)atofs(freq_arg.substr(0, c1)), (int)atofs(freq_arg.substr(c1 + 1, c2 - c1 - 1)),
	                                 (int)atofs(freq_arg.substr(c2 + 1)), crop, boxcar, &plan);
	if (r < 0 || plan.tune_count == 0) { fprintf(stderr, "Error: bandwidth too wide.\n"); return 1; }
	const int bins = 1 << plan.bin_e;
	fprintf(stderr, "Number of frequency hops: %i\nDongle bandwidth: %iHz\nDownsampling by: %ix\nCropping by: %0.2f%%\n"
	        "Total FFT bins: %i\nLogged FFT bins: %i\nFFT bin size: %0.2fHz\nBuffer size: %i bytes (%0.2fms)\n",
	        plan.tune_count, plan.rate, plan.downsample, plan.crop * 100, plan.tune_count * bins,
	        (int)((double)(plan.tune_count * bins) * (1.0 - plan.crop)), plan.bin_size, plan.buf_len,
	        1000 * 0.5 * (float)plan.buf_len / (float)plan.rate);
	if (interval < 1) interval = 1;
	fprintf(stderr, "Reporting every %i seconds\n", interval);
	const char *filename = optind < argc ? argv[optind] : "-";
	if (nsources < 0) { fprintf(stderr, "-N needs a positive number of sources.\n"); return 1; }
	if (nsources > 0) {
		if (crop >= 1.0) { fprintf(stderr, "-N: a crop of 100%% leaves no bin to report; use -c below 1.\n"); return 1; }
		rtlpower_cfg ncfg;
		rtlpower_plan_cfg(&plan, window, boxcar, comp_fir, peak_hold, &ncfg);
		return run_sources(nsources, dev_index, plan, ncfg, filename, interval, single, exit_after);
	}

	rtlsdr_dev_t *dev = nullptr;
	if (rtlsdr_get_device_count() == 0 || rtlsdr_open(&dev, (uint32_t)dev_index) < 0) {
		fprintf(stderr, "Failed to open rtlsdr device #%d (set RTLSDR_FILE).\n", dev_index);
		return 1;
	}
	rtlpower_cfg cfg;
	rtlpower_plan_cfg(&plan, window, boxcar, comp_fir, peak_hold, &cfg);
	rtlpower_gpu *gpu = nullptr;
	r = rtlpower_gpu_create(&cfg, plan.tune_count, 0, &gpu);
	if (r < 0) { fprintf(stderr, "rtlpower_gpu_create: %d\n", r); return 2; }
	FILE *file = !strcmp(filename, "-") ? stdout : fopen(filename, "wb");
	if (!file) { fprintf(stderr, "Failed to open %s\n", filename); return 1; }
	rtlsdr_reset_buffer(dev);
	rtlsdr_set_sample_rate(dev, (uint32_t)plan.rate);

	const char *pe = getenv("RTLPOWER_PASSES");
	const int passes_per_report = pe ? atoi(pe) : 0;
	std::vector<uint8_t> buf((size_t)plan.buf_len);
	std::vector<int64_t> avg((size_t)bins);
	std::vector<char> line((size_t)bins * 16 + 256);
	time_t next_tick = time(nullptr) + interval;
	if (exit_after) exit_after += time(nullptr);
	bool stop = false;
	int passes = 0;
	while (!stop) {
		// scanner(): one read per hop (src/rtl_power.c:650-719)
		for (int i = 0; i < plan.tune_count && !stop; i++) {
			const int f = rtlpower_tune_freq(&plan, i);
			if ((int)rtlsdr_get_center_freq(dev) != f) {
				rtlsdr_set_center_freq(dev, (uint32_t)f);  // retune(), :542-552 (the settling dump is a hardware matter)
			}
			int n_read = 0;
			rtlsdr_read_sync(dev, buf.data(), plan.buf_len, &n_read);
			if (n_read != plan.buf_len) { fprintf(stderr, "Error: dropped samples.\n"); stop = true; break; }
			r = rtlpower_gpu_scan(gpu, i, buf.data(), (uint32_t)plan.buf_len);
			if (r < 0) { fprintf(stderr, "rtlpower_gpu_scan: %d\n", r); stop = true; }
		}
		passes++;
		const time_t now = time(nullptr);
		const bool report = passes_per_report ? (passes % passes_per_report == 0) : (now >= next_tick);
		if (!report && !stop) continue;
		if (stop && passes_per_report) break;
		char t_str[50];
		strftime(t_str, sizeof(t_str), "%Y-%m-%d, %H:%M:%S", localtime(&now));
		for (int i = 0; i < plan.tune_count; i++) {
			int32_t samples = 0;
			rtlpower_gpu_fetch(gpu, i, avg.data(), &samples);
			if (samples == 0) continue;
			if (rtlpower_csv_dbm(&plan, i, avg.data(), samples, line.data(), line.size()) > 0)
				fprintf(file, "%s, %s", t_str, line.data());
		}
		fflush(file);
		rtlpower_gpu_clear(gpu);  // csv_dbm zeroes the accumulators, :761-764
		while (time(nullptr) >= next_tick) next_tick += interval;
		if (single) stop = true;
		if (exit_after && time(nullptr) >= exit_after) stop = true;
	}
	if (file != stdout) fclose(file);
	rtlpower_gpu_destroy(gpu);
	rtlsdr_close(dev);
	return 0;
}
