// rtlpower_hip.hip — the C ABI of include/rtlpower_hip.h on HIP / gfx950.
// Host side of rtl_power's scanner() (reference src/rtl_power.c:642-720).
// No CPU fallback.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rtlpower_hip.h"
#define OWN_UNIT "rtlpower_hip"
#include "debug_poison.h"
#include "stream_pool.h"
#include "power_kernels.h"
#include "power_report_kernel.h"

using namespace rtlpower;

#define HIP_TRY(expr)                                                                         \
	do {                                                                                      \
		hipError_t e_ = (expr);                                                               \
		if (e_ != hipSuccess) {                                                               \
			fprintf(stderr, "rtlpower_hip: %s -> %s (%s:%d)\n", #expr, hipGetErrorString(e_), \
			        __FILE__, __LINE__);                                                      \
			return e_ == hipErrorOutOfMemory ? -ENOMEM : -EIO;                                \
		}                                                                                     \
	} while (0)

// What a configuration fixes about its scans (scan_geometry): a handle's from create on
struct ScanGeom {
	int N = 1, len_dec = 0, chunks = 0, dec_elems = 0;
	bool decimates = false;
	bool staged = false;  // bin_e 15 .. 21 or more points per read than a workgroup's LDS holds: transform in HBM
};

static const rtlpower_route_opts kRouteDefaults = {0, 1, 1, 0, 0, 1};

struct rtlpower_gpu : ScanGeom {
	rtlpower_cfg cfg;
	int nstreams = 0, device = 0;
	hipStream_t own_stream = nullptr, stream = nullptr;
	Event ev_wait, ev_release;
	DevBuf<int32_t> d_window;
	DevBuf<uint16_t> d_window16;  // the low halves (k_power_scan_big multiplies in 16 bits)
	DevBuf<uint32_t> d_tw;
	DevBuf<long long> d_avg;
	DevBuf<int32_t> d_samples;
	DevBuf<int16_t> d_decA, d_decB;
	DevBuf<uint8_t> d_one;  // landing zone of rtlpower_gpu_scan()
	bool timing = false;
	// the options a scan's plan reads (kOptions; what each does: include/rtlpower_hip.h, plan_scan)
	rtlpower_route_opts opt = kRouteDefaults;
	int last_kernel = 0;  // option "last_kernel" (read-only): which transform kernel the last scan took (RTLPOWER_KERNEL_*)
	unsigned lds_raised = 0;  // raise_lds: the kernels whose dynamic-LDS limit is raised on this handle's device (kLds*)
	DevBuf<uint32_t> d_work; DevBuf<int2> d_ave;
	// one undecimated frame per read, bin_e > 14: the window comb by comb, the batch's bytes likewise, the averages' partial sums
	DevBuf<uint16_t> d_window16T; DevBuf<uint8_t> d_tbuf; DevBuf<int2> d_part;
	// decimated scans (a range below 1 MHz, src/rtl_power.c:466-480) in two launches: k_power_downsample_iq (-F) or
	// k_power_boxcar into packed int16 pairs, k_power_scan_frames<13, true> on them
	DevBuf<uint32_t> d_dec32;
	// Fine bins (one frame per read beyond 16384 points), round 5: the batches of a scan as a two-stream pipeline (option
	// "staged_pipe").  The transform in LDS (k_power_scan_big<14, true>: issue-bound, 71 registers, one workgroup per CU)
	// runs on the handle's stream; what only moves bytes - the comb gather of the NEXT batch, the passes over HBM and the
	// accumulation of the one BEFORE - runs beside it on `aux` (their waves fit next to the transform's on every CU).  Two
	// sets of work buffers.
	struct Pipe {
		hipStream_t aux = nullptr;
		int aux_prio = 0;  // the HIP priority aux was taken from the stream pool with
		Event start, prep[2], scanned[2], done;
	} pipe;
	bool work_two = false;  // d_work / d_ave / d_tbuf / d_part hold two batches
	size_t work_reads = 0;                 // reads the work buffer holds per stream
	bool want_stamps = false;              // rtlpower_gpu_clock_probe
	DevBuf<unsigned long long> d_stamps;   // four per workgroup
	int stamp_last = 0;                    // workgroups of the last stamped launch
	std::vector<std::pair<Event, Event>> ev_pending, ev_free;
	// rtlpower_gpu_report (power_report_kernel.h): one device block - doubt counter, doubt list, samples, values - and its
	// pinned mirror, both allocated by the first report; `arrived` is the kernel's per-stream counter
	DevBuf<uint8_t> d_rep;
	PinnedBuf<uint8_t> h_rep;
	DevBuf<uint32_t> d_arrived;
	Event ev_rep;
	int rep_outn = 0;            // values per stream of the last report (the kept bins and the trailing value)
	double rep_rate = 0;
	bool rep_issued = false, rep_resolved = false;
	int rep_status = 0;          // what resolving found (0, -EOVERFLOW, -EIO)
	long rep_doubts = 0;         // option "report_doubts" (read-only)
	int rep_guard_ppm = 1;       // option "report_guard_ppm": the guard in millionths of a hundredth of a dB (tests widen it)
	DevBuf<uint8_t> d_in;  // landing zone of rtlpower_gpu_scan_host()
	Event ev_in;
};

// the window functions, src/rtl_power.c:329-408
static double window_fn(int window, int i, int length)
{
	const double n1 = (double)(length - 1);
	switch (window) {
	case RTLPOWER_WIN_HAMMING:
		return 25.0 / 46.0 - 21.0 / 46.0 * cos(2 * i * M_PI / n1);
	case RTLPOWER_WIN_BLACKMAN:
		return 7938.0 / 18608.0 - 9240.0 / 18608.0 * cos(2 * i * M_PI / n1) +
		       1430.0 / 18608.0 * cos(4 * i * M_PI / n1);
	case RTLPOWER_WIN_BLACKMAN_HARRIS:
		return 0.35875 - 0.48829 * cos(2 * i * M_PI / n1) + 0.14128 * cos(4 * i * M_PI / n1) -
		       0.01168 * cos(6 * i * M_PI / n1);
	case RTLPOWER_WIN_HANN_POISSON:
		return 0.5 * (1 - cos(2 * M_PI * i / n1)) * pow(M_E, (-2.0 * (double)abs((int)(n1 - 1 - 2 * i))) / n1);
	case RTLPOWER_WIN_YOUSSEF: {
		double w = 0.35875 - 0.48829 * cos(2 * i * M_PI / n1) + 0.14128 * cos(4 * i * M_PI / n1) -
		           0.01168 * cos(6 * i * M_PI / n1);
		return w * pow(M_E, (-0.0025 * (double)abs((int)(n1 - 1 - 2 * i))) / n1);
	}
	case RTLPOWER_WIN_BARTLETT: {
		double l = (double)length, w = (i - n1 / 2) / (l / 2);
		if (w < 0) w = -w;
		return 1 - w;
	}
	default:
		return 1.0;  // rectangle, and kaiser (a stub in the reference, :392-396)
	}
}

extern "C" int rtlpower_window_coefs(int window, int length, int32_t *out)
{
	if (!out || length < 1 || window < 0 || window > RTLPOWER_WIN_BARTLETT) return -EINVAL;
	for (int i = 0; i < length; i++)
		out[i] = (int32_t)(256 * window_fn(window, i, length));  // src/rtl_power.c:985-988
	return 0;
}

// ---- planner and CSV emitter (host only) ------------------------------------------

extern "C" int rtlpower_frequency_range(int32_t lower, int32_t upper, int32_t max_size, double crop, int boxcar,
                                        rtlpower_plan *out)
{
	// frequency_range(), src/rtl_power.c:438-540; MAXIMUM_RATE / MINIMUM_RATE :78-79, MAX_TUNES :111
	const int kMaxRate = 2800000, kMinRate = 1000000, kMaxTunes = 3000, kDefaultBuf = 16384;
	if (!out) return -EINVAL;
	int tune_count = 0, bw_seen = 0, bw_used = 0, downsample = 1, passes = 0, bin_e = 0;
	double bin_size = 0;
	for (int i = 1; i < 1500; i++) {  // evenly sized hops, as close to the maximum rate as possible
		bw_seen = (upper - lower) / i;
		bw_used = (int)((double)bw_seen / (1.0 - crop));
		if (bw_used > kMaxRate) continue;
		tune_count = i;
		break;
	}
	if (bw_used < kMinRate) {  // small bandwidth: one hop, decimated
		tune_count = 1;
		downsample = kMaxRate / bw_used;
		bw_used = bw_used * downsample;
	}
	if (!boxcar && downsample > 1) {
		passes = (int)log2((double)downsample);
		downsample = 1 << passes;
		bw_used = (int)((double)(bw_seen * downsample) / (1.0 - crop));
	}
	for (int i = 1; i <= 21; i++) {  // power-of-two bins no wider than asked
		bin_e = i;
		bin_size = (double)bw_used / (double)((1 << i) * downsample);
		if (bin_size <= (double)max_size) break;
	}
	if (max_size >= kMinRate) {  // giant bins: rms_power per hop
		bw_seen = max_size;
		bw_used = max_size;
		tune_count = (upper - lower) / bw_seen;
		bin_e = 0;
		crop = 0;
	}
	if (tune_count > kMaxTunes) return -E2BIG;
	int buf_len = 2 * (1 << bin_e) * downsample;
	if (buf_len < kDefaultBuf) buf_len = kDefaultBuf;
	out->lower = lower; out->upper = upper; out->max_size = max_size;
	out->tune_count = tune_count; out->bw_seen = bw_seen; out->rate = bw_used; out->bin_e = bin_e;
	out->downsample = downsample; out->downsample_passes = passes; out->buf_len = buf_len;
	out->crop = crop; out->bin_size = bin_size;
	return 0;
}

extern "C" int32_t rtlpower_tune_freq(const rtlpower_plan *p, int i)
{
	return p->lower + i * p->bw_seen + p->bw_seen / 2;  // src/rtl_power.c:509
}

extern "C" void rtlpower_plan_cfg(const rtlpower_plan *p, int window, int boxcar, int comp_fir_size, int peak_hold,
                                  rtlpower_cfg *c)
{
	memset(c, 0, sizeof(*c));
	c->bin_e = p->bin_e; c->window = window; c->downsample = p->downsample;
	c->downsample_passes = p->downsample_passes; c->boxcar = boxcar; c->comp_fir_size = comp_fir_size;
	c->peak_hold = peak_hold; c->buf_len = (uint32_t)p->buf_len;
}

extern "C" int rtlpower_csv_dbm(const rtlpower_plan *p, int tune, int64_t *avg, int32_t samples, char *out, size_t cap)
{
	// csv_dbm(), src/rtl_power.c:722-765
	if (!p || !avg || !out) return -EINVAL;
	const int len = 1 << p->bin_e, ds = p->downsample;
	const int freq = rtlpower_tune_freq(p, tune);
	if (p->bin_e > 0) {
		avg[0] = avg[1];  // "nuke DC component"
		for (int i = 0; i < len / 2; i++) {  // the FFT is translated by 180 degrees
			int64_t t = avg[i]; avg[i] = avg[i + len / 2]; avg[i + len / 2] = t;
		}
	}
	std::string sres;
	char tmp[96];
	const int bin_count = (int)((double)len * (1.0 - p->crop));
	const int bw2 = (int)(((double)p->rate * (double)bin_count) / (len * 2 * ds));
	snprintf(tmp, sizeof(tmp), "%i, %i, %.2f, %i, ", freq - bw2, freq + bw2, (double)p->rate / (double)(len * ds), samples);
	sres += tmp;
	const int i1 = 0 + (int)((double)len * p->crop * 0.5);
	const int i2 = (len - 1) - (int)((double)len * p->crop * 0.5);
	double dbm;
	for (int i = i1; i <= i2; i++) {
		dbm = (double)avg[i];
		dbm /= (double)p->rate;
		dbm /= (double)samples;
		dbm = 10 * log10(dbm);
		snprintf(tmp, sizeof(tmp), "%.2f, ", dbm);
		sres += tmp;
	}
	dbm = (double)avg[i2] / ((double)p->rate * (double)samples);
	if (p->bin_e == 0) dbm = ((double)avg[0] / ((double)p->rate * (double)samples));
	dbm = 10 * log10(dbm);
	snprintf(tmp, sizeof(tmp), "%.2f\n", dbm);
	sres += tmp;
	if (sres.size() + 1 > cap) return -ENOBUFS;
	memcpy(out, sres.c_str(), sres.size() + 1);
	return (int)sres.size();
}

// ---- the report: host definition and formatter (no GPU needed) ---------------------

// One value as glibc's own "%.2f" prints the reference's expression (src/rtl_power.c:749-753), read back into
// sign + hundredths: right by construction, and what the doubt list of k_power_report is resolved with.
static uint32_t report_centi_one(int64_t avg, int32_t samples, double rate, bool trailing)
{
	double dbm = (double)avg;
	if (trailing) {
		dbm = (double)avg / (rate * (double)samples);  // the line's last value, :755-758: one division
	} else {
		dbm /= rate;
		dbm /= (double)samples;
	}
	dbm = 10 * log10(dbm);
	char tmp[400];
	snprintf(tmp, sizeof(tmp), "%.2f", dbm);
	const char *t = tmp;
	uint32_t sign = 0;
	if (*t == '-') { sign = kCentiSign; t++; }
	if (*t == 'i') return sign | kCentiInf;
	if (*t == 'n') return sign | kCentiNan;
	uint64_t v = 0;
	for (; *t; t++)
		if (*t != '.') v = v * 10 + (uint64_t)(*t - '0');
	return sign | (uint32_t)(v < kCentiDoubt ? v : kCentiDoubt - 1);
}

// i1 and the number of kept bins, in doubles as csv_dbm() writes them (:746-747)
static int report_range(int bin_e, double crop, int *i1, int *outn)
{
	if (bin_e < 0 || bin_e > 21 || !(crop >= 0.0) || !(crop < 1.0)) return -EINVAL;
	const int len = 1 << bin_e;
	*i1 = 0 + (int)((double)len * crop * 0.5);
	const int i2 = (len - 1) - (int)((double)len * crop * 0.5);
	*outn = i2 - *i1 + 1;
	return *outn >= 1 ? 0 : -EINVAL;
}

extern "C" int rtlpower_report_host(const int64_t *avg, int32_t samples, double rate, int bin_e, double crop, int32_t *centi,
                                    int *n)
{
	int i1 = 0, outn = 0;
	if (!avg || !centi || !n || !(rate > 0.0)) return -EINVAL;
	const int r = report_range(bin_e, crop, &i1, &outn);
	if (r < 0) return r;
	*n = 0;
	if (samples == 0) return 0;  // no line for a hop that was never scanned
	const int len = 1 << bin_e;
	for (int j = 0; j < outn; j++) {
		int b = (j + i1 + len / 2) & (len - 1);
		if (bin_e > 0 && b == 0) b = 1;
		centi[j] = (int32_t)report_centi_one(avg[b], samples, rate, false);
		if (j == outn - 1) centi[outn] = (int32_t)report_centi_one(avg[b], samples, rate, true);
	}
	*n = outn + 1;
	return 0;
}

static inline char *put_centi(char *o, uint32_t w)
{
	if (w & kCentiSign) *o++ = '-';
	w &= ~kCentiSign;
	if (w == kCentiInf) { memcpy(o, "inf", 3); return o + 3; }
	if (w >= kCentiDoubt) { memcpy(o, "nan", 3); return o + 3; }
	char d[12];
	int k = 0;
	uint32_t whole = w / 100, frac = w % 100;
	do { d[k++] = (char)('0' + whole % 10); whole /= 10; } while (whole);
	while (k) *o++ = d[--k];
	*o++ = '.';
	*o++ = (char)('0' + frac / 10);
	*o++ = (char)('0' + frac % 10);
	return o;
}

extern "C" int rtlpower_csv_report(const rtlpower_plan *p, int tune, const int32_t *centi, int n, int32_t samples, char *out,
                                   size_t cap)
{
	// the line of csv_dbm(), src/rtl_power.c:740-760, from values already reduced to hundredths
	if (!p || !centi || !out || n < 0 || n == 1 || cap < 1) return -EINVAL;
	out[0] = 0;
	if (n == 0) return 0;
	const int len = 1 << p->bin_e, ds = p->downsample;
	const int freq = rtlpower_tune_freq(p, tune);
	const int bin_count = (int)((double)len * (1.0 - p->crop));
	const int bw2 = (int)(((double)p->rate * (double)bin_count) / (len * 2 * ds));
	char head[128];
	const int hn = snprintf(head, sizeof(head), "%i, %i, %.2f, %i, ", freq - bw2, freq + bw2, (double)p->rate / (double)(len * ds), samples);
	if ((size_t)hn + (size_t)(n + 1) * 16 + 2 > cap) return -ENOBUFS;  // (a value and its separator: at most 15 bytes)
	memcpy(out, head, (size_t)hn);
	char *o = out + hn;
	for (int j = 0; j < n - 1; j++) {
		o = put_centi(o, (uint32_t)centi[j]);
		*o++ = ','; *o++ = ' ';
	}
	o = put_centi(o, (uint32_t)centi[n - 1]);  // the last bin once more, as the reference forms it there (:755-760)
	*o++ = '\n';
	*o = 0;
	return (int)(o - out);
}

static int report_wait(rtlpower_gpu *h);

static int validate(const rtlpower_cfg *c)
{
	if (c->bin_e < 0 || c->bin_e > 21) return -EINVAL;  // frequency_range() plans 2^1 .. 2^21 bins (src/rtl_power.c:483-486)
	if (c->window < 0 || c->window > RTLPOWER_WIN_BARTLETT) return -EINVAL;
	if (c->buf_len < 16 || c->buf_len % 4 || c->buf_len > (1u << 26)) return -EINVAL;
	if (c->downsample < 1) return -EINVAL;
	if (c->comp_fir_size != 0 && c->comp_fir_size != 9) return -EINVAL;
	// remove_dc() divides by buf_len / ds and by one less (src/rtl_power.c:590, :692-693): the reference stops there
	if (c->bin_e > 0 && c->buf_len / (uint32_t)c->downsample < 2) return -EINVAL;
	if (!c->boxcar && c->downsample_passes) {
		if (c->downsample_passes < 1 || c->downsample_passes > 10) return -EINVAL;
		if (c->downsample != (1 << c->downsample_passes)) return -EINVAL;
		if (c->buf_len % (4u << c->downsample_passes)) return -EINVAL;
		if ((c->buf_len >> c->downsample_passes) < 48) return -EINVAL;  // ease-in reads x[0..8], fir 9 more
	}
	// scanner() transforms frames at offsets 0, 2N, ... < buf_len/ds (src/rtl_power.c:695).  A
	// trailing frame may run past the decimated data; inside buf_len it then sees this read's
	// own leftovers (reproduced here), but past buf_len it would see the previous read's FFT
	// output still lying in the reference's static fft_buf.  The reference's planner never
	// produces that (buf_len = 2N * downsample, at least 16384: src/rtl_power.c:501-504); it is rejected here.
	{
		const long long two_n = 2ll << c->bin_e;
		const long long per = (long long)c->buf_len / c->downsample;
		const long long frames = (per + two_n - 1) / two_n;
		if (frames * two_n > (long long)c->buf_len) return -EINVAL;
		// With fifth_order passes a partial trailing frame would cover the intermediate passes'
		// leftovers; powers of two never produce one through frequency_range(), only the boxcar
		// with an odd ratio does, and that case is reproduced.
		if (!c->boxcar && c->downsample_passes && per % two_n) return -EINVAL;
	}
	return 0;
}

extern "C" int rtlpower_cfg_validate(const rtlpower_cfg *cfg) { return cfg ? validate(cfg) : -EINVAL; }

static int power_create_body(rtlpower_gpu *h);

static ScanGeom scan_geometry(const rtlpower_cfg &c)
{
	ScanGeom g;
	g.N = 1 << c.bin_e;
	const int ds = c.downsample;
	g.decimates = (c.boxcar && ds > 1) || (!c.boxcar && c.downsample_passes > 0);
	g.len_dec = (int)c.buf_len / ds;  // what remove_dc() and the chunk loop are given (:692-696)
	if (c.bin_e > 0) {
		g.chunks = (g.len_dec + 2 * g.N - 1) / (2 * g.N);
		// what one workgroup's LDS cannot hold goes through the work buffer in HBM (power_kernels.h, k_power_fft_*)
		g.staged = c.bin_e > 14 || (long long)g.chunks * g.N > kMaxPoints;
		if (c.boxcar && ds > 1) g.dec_elems = 2 * (((int)c.buf_len / 2 + ds - 1) / ds);
		else if (g.decimates) g.dec_elems = (int)c.buf_len >> c.downsample_passes;
	}
	return g;
}

extern "C" int rtlpower_gpu_create(const rtlpower_cfg *cfg, int nstreams, int device, rtlpower_gpu **out)
{
	if (!cfg || !out || nstreams < 1) return -EINVAL;
	int v = validate(cfg);
	if (v < 0) return v;
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
		fprintf(stderr, "rtlpower_hip: no usable HIP device (count=%d); there is no CPU fallback\n", ndev);
		return -ENODEV;
	}
	HIP_TRY(hipSetDevice(device));
	rtlpower_gpu *h = new rtlpower_gpu();
	h->cfg = *cfg;
	h->nstreams = nstreams;
	h->device = device;
	// every failure releases what was allocated so far; *out is written on success only
	int r = power_create_body(h);
	if (r < 0) {
		rtlpower_gpu_destroy(h);
		return r;
	}
	*out = h;
	return 0;
}

static int power_create_body(rtlpower_gpu *h)
{
	const rtlpower_cfg *cfg = &h->cfg;
	const int nstreams = h->nstreams;
	static_cast<ScanGeom &>(*h) = scan_geometry(*cfg);
	HIP_TRY(rtl_pool::stream_get(h->device, 0, &h->own_stream));  // (from the process-wide pool: stream_pool.h)
	h->stream = h->own_stream;
	const size_t S = (size_t)nstreams;
	OWN_TRY(h->d_avg.alloc(S * h->N));
	OWN_TRY(h->d_samples.alloc(S));
	if (cfg->bin_e > 0) {
		std::vector<int32_t> w((size_t)h->N);
		rtlpower_window_coefs(cfg->window, h->N, w.data());
		OWN_TRY(h->d_window.alloc(w.size()));
		HIP_TRY(hipMemcpy(h->d_window, w.data(), w.size() * sizeof(int32_t), hipMemcpyHostToDevice));
		std::vector<uint16_t> w16(w.size());
		for (size_t i = 0; i < w.size(); i++) w16[i] = (uint16_t)(uint32_t)w[i];
		OWN_TRY(h->d_window16.alloc(w16.size()));
		HIP_TRY(hipMemcpy(h->d_window16, w16.data(), w16.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
		if (cfg->bin_e > 14) {
			// comb b of the frame = the points k << c | b: k_power_scan_big<14, true> reads its coefficients as it reads a read's
			const int cc = cfg->bin_e - 14;
			std::vector<uint16_t> wt(w16.size());
			for (size_t j = 0; j < w16.size(); j++) wt[((j & (((size_t)1 << cc) - 1)) << 14) | (j >> cc)] = w16[j];
			OWN_TRY(h->d_window16T.alloc(wt.size()));
			HIP_TRY(hipMemcpy(h->d_window16T, wt.data(), wt.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
		}
		// sine_table(), src/rtl_power.c:247-261, regrouped per FFT stage: stage s uses
		// wr = Sinewave[j + N/4] >> 1, wi = -Sinewave[j] >> 1 at j = m << (log2N - 1 - s)
		// for m < 2^s (:303-308); entry (1 << s) - 1 + m holds them DOUBLED and packed, (2 wr, 2 wi) - the
		// butterfly takes FIX_MPY as the high half of a 16 x 16 product (power_kernels.h); wr, wi lie in
		// -16384 .. 16383, so the doubled values still fit int16.
		std::vector<int16_t> sine((size_t)h->N * 3 / 4 + 1);
		for (int i = 0; i < h->N * 3 / 4; i++)
			sine[i] = (int16_t)(int)round(32767 * sin((double)i * 2.0 * M_PI / h->N));
		std::vector<uint32_t> tw((size_t)h->N, 0u);
		for (int st = 0; st < cfg->bin_e; st++) {
			const int k = cfg->bin_e - 1 - st;
			for (int m = 0; m < (1 << st); m++) {
				const int j = m << k;
				int16_t wr = sine[j + h->N / 4], wi = (int16_t)(-sine[j]);
				wr >>= 1; wi >>= 1;
				tw[(size_t)(1 << st) - 1 + m] = (uint32_t)(uint16_t)(wr * 2) | ((uint32_t)(uint16_t)(wi * 2) << 16);
			}
		}
		OWN_TRY(h->d_tw.alloc(tw.size()));
		HIP_TRY(hipMemcpy(h->d_tw, tw.data(), tw.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
	}
	return rtlpower_gpu_clear(h);
}

extern "C" int rtlpower_gpu_destroy(rtlpower_gpu *h)
{
	if (!h) return -EINVAL;
	(void)hipSetDevice(h->device);
	if (h->stream) (void)hipStreamSynchronize(h->stream);
	if (h->pipe.aux) (void)hipStreamSynchronize(h->pipe.aux);
	// back to the pool, never destroyed (stream_pool.h)
	rtl_pool::stream_put(h->device, h->pipe.aux_prio, h->pipe.aux);
	rtl_pool::stream_put(h->device, 0, h->own_stream);
	delete h;
	return 0;
}

extern "C" int rtlpower_gpu_clear(rtlpower_gpu *h)
{
	if (!h) return -EINVAL;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(hipMemsetAsync(h->d_avg, 0, (size_t)h->nstreams * h->N * sizeof(long long), h->stream));
	HIP_TRY(hipMemsetAsync(h->d_samples, 0, (size_t)h->nstreams * sizeof(int32_t), h->stream));
	return 0;
}

extern "C" int rtlpower_gpu_sync(rtlpower_gpu *h)
{
	if (!h) return -EINVAL;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(hipStreamSynchronize(h->stream));
	return 0;
}

extern "C" int rtlpower_gpu_set_stream(rtlpower_gpu *h, void *s)
{
	if (!h) return -EINVAL;
	HIP_TRY(hipStreamSynchronize(h->stream));
	h->stream = s ? (hipStream_t)s : h->own_stream;
	return 0;
}

// cross-stream ordering without a host synchronisation, as rtlfm_gpu_wait_for / _release_to
extern "C" int rtlpower_gpu_wait_for(rtlpower_gpu *h, void *producer_stream)
{
	if (!h) return -EINVAL;
	if ((hipStream_t)producer_stream == h->stream) return 0;
	HIP_TRY(hipSetDevice(h->device));
	OWN_TRY(h->ev_wait.create(hipEventDisableTiming));
	HIP_TRY(hipEventRecord(h->ev_wait, (hipStream_t)producer_stream));
	HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_wait, 0));
	return 0;
}

extern "C" int rtlpower_gpu_release_to(rtlpower_gpu *h, void *consumer_stream)
{
	if (!h) return -EINVAL;
	if ((hipStream_t)consumer_stream == h->stream) return 0;
	HIP_TRY(hipSetDevice(h->device));
	OWN_TRY(h->ev_release.create(hipEventDisableTiming));
	HIP_TRY(hipEventRecord(h->ev_release, h->stream));
	HIP_TRY(hipStreamWaitEvent((hipStream_t)consumer_stream, h->ev_release, 0));
	return 0;
}

// The options by name: one table for set_option and get_option.  A flag stores value != 0; a read-only name is unknown
// to set_option; "report_doubts" has no slot, its read waits for the report.
#define OPT_SLOT(field) [](rtlpower_gpu *h) -> int * { return &h->field; }
static const struct Option {
	const char *name;
	int *(*slot)(rtlpower_gpu *);
	long min, max;
	bool flag, read_only;
} kOptions[] = {
	{"groups", OPT_SLOT(opt.groups), 0, INT32_MAX, false, false},  // workgroups per stream of the FFT kernel (0 = automatic)
	{"staged_fast", OPT_SLOT(opt.staged_fast), 0, 1, true, false},
	{"dec_fast", OPT_SLOT(opt.dec_fast), 0, 1, true, false},
	{"staged_pipe", OPT_SLOT(opt.staged_pipe), 0, 2, false, false},
	{"staged_batch", OPT_SLOT(opt.staged_batch), 0, 1 << 20, false, false},  // reads per batch, 0 = by the work buffer's size
	{"scan_frames", OPT_SLOT(opt.scan_frames), 0, 1, true, false},
	{"report_guard_ppm", OPT_SLOT(rep_guard_ppm), 1, 500000, false, false},
	{"last_kernel", OPT_SLOT(last_kernel), 0, 0, false, true},
	{"report_doubts", nullptr, 0, 0, false, true},
};
#undef OPT_SLOT

static const Option *find_option(const char *name)
{
	for (const Option &o : kOptions)
		if (!strcmp(name, o.name)) return &o;
	return nullptr;
}

extern "C" int rtlpower_gpu_set_option(rtlpower_gpu *h, const char *name, long value)
{
	if (!h || !name) return -EINVAL;
	const Option *o = find_option(name);
	if (!o || o->read_only) return -ENOENT;
	if (o->flag) value = value != 0;
	if (value < o->min || value > o->max) return -EINVAL;
	*o->slot(h) = (int)value;
	return 0;
}

extern "C" int rtlpower_gpu_get_option(rtlpower_gpu *h, const char *name, long *value)
{
	if (!h || !name || !value) return -EINVAL;
	const Option *o = find_option(name);
	if (!o) return -ENOENT;
	if (o->slot) { *value = *o->slot(h); return 0; }
	if (!h->rep_issued) { *value = 0; return 0; }
	const int r = report_wait(h);
	*value = h->rep_doubts;
	return r == -EOVERFLOW ? 0 : r;  // (an overflowing report still says how many bins it was handed)
}

// The shader clock the FFT kernel's workgroups actually ran at (k_power_scan_big stamps s_memtime and the
// 100 MHz s_memrealtime at its first and last instruction): what the VALU-issue ceiling of a launch is priced at.
extern "C" int rtlpower_gpu_clock_probe(rtlpower_gpu *h, int on)
{
	if (!h) return -EINVAL;
	h->want_stamps = on != 0;
	if (!on) h->stamp_last = 0;
	return 0;
}

extern "C" int rtlpower_gpu_clock_read(rtlpower_gpu *h, double *shader_mhz, double *span_ms)
{
	if (!h) return -EINVAL;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(hipStreamSynchronize(h->stream));
	if (!h->d_stamps || h->stamp_last <= 0) return -ENODATA;
	std::vector<unsigned long long> st((size_t)h->stamp_last * 4);
	HIP_TRY(hipMemcpy(st.data(), h->d_stamps, st.size() * 8, hipMemcpyDeviceToHost));
	double sum = 0; int n = 0; unsigned long long t0 = ~0ull, t1 = 0;
	for (int w = 0; w < h->stamp_last; w++) {
		const double dc = (double)(st[w * 4 + 1] - st[w * 4]), dr = (double)(st[w * 4 + 3] - st[w * 4 + 2]);
		if (st[w * 4 + 3] == 0 || dr <= 0) continue;  // a workgroup that had no reads
		sum += dc / dr * 100.0; n++;
		if (st[w * 4 + 2] < t0) t0 = st[w * 4 + 2];
		if (st[w * 4 + 3] > t1) t1 = st[w * 4 + 3];
	}
	if (!n) return -ENODATA;
	if (shader_mhz) *shader_mhz = sum / n;
	if (span_ms) *span_ms = (double)(t1 - t0) / 1e5;
	return 0;
}

extern "C" int rtlpower_gpu_timing_enable(rtlpower_gpu *h, int on)
{
	if (!h) return -EINVAL;
	h->timing = on != 0;
	return 0;
}

extern "C" int rtlpower_gpu_timing_read(rtlpower_gpu *h, double *ms, int *launches)
{
	if (!h) return -EINVAL;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(hipStreamSynchronize(h->stream));
	double total = 0;
	int n = 0;
	for (auto &p : h->ev_pending) {
		float t = 0;
		HIP_TRY(hipEventElapsedTime(&t, p.first, p.second));
		total += t; n++;
		h->ev_free.push_back(std::move(p));
	}
	h->ev_pending.clear();
	if (ms) *ms = total;
	if (launches) *launches = n;
	return 0;
}

static inline int grid_for(size_t work, int block = 256, int cap = 256 * 16)
{
	size_t g = (work + block - 1) / block;
	if (g < 1) g = 1;
	if (g > (size_t)cap) g = cap;
	return (int)g;
}

// ---- a scan: its plan, made once (host only), and one launcher per route -----------

struct ScanPlan {
	int route = RTLPOWER_KERNEL_NONE;  // which launcher, as "last_kernel" names it; NONE: rms_power (bin_e == 0)
	// DECIMATED: points of a decimated read (2^dec_e of them) and what decimates
	int Pr = 0, dec_e = 0;
	bool by_fifth = false, by_boxcar = false;
	// STAGED / STAGED_FAST: reads per batch; fast_shape: the work buffers include the fast kernels'; two: two sets of
	// them; piped: the batches as the two-stream pipeline
	bool fast_shape = false, fast = false, two = false, piped = false;
	size_t batch = 0;
	// GENERAL / BIG / FRAMES, and DECIMATED's transform: points a workgroup holds, workgroups per stream, the grid
	bool big = false, frames = false;
	int M = 0, groups = 0;
	unsigned grid = 0;
};

// Workgroups per stream of an in-LDS transform: enough for the 256 CUs (a large-FFT workgroup fills a CU's LDS, the small
// ones share) - a stream's reads are split when there are few streams (power_kernels.h) - or what option "groups" says,
// and never more than `most`, the units of work a stream has
static int groups_per_stream(int S, int option, int most)
{
	int groups = option > 0 ? option : (512 + S - 1) / S;
	if (groups > most) groups = most;
	return groups < 1 ? 1 : groups;
}

// Reads per batch of a staged scan: at most ~1 GiB of work buffer.  The pipeline holds two batches: half the points each,
// and at least four batches where each still fills the GPU (measured, profiles/r05_power_big_pipe.txt: 2^19 .. 2^21 bins -
// two passes over HBM per batch - 4-5 % faster in two sessions and 6 % slower in a third; 2^15 .. 2^17 1-3 % SLOWER: the
// kernels do run at the same time, but beside the transform the accumulating pass takes three times as long as alone and
// becomes the longer chain; a scan of one batch only pays for the events.  Not the default.)
static size_t staged_batch_reads(const rtlpower_cfg &c, const ScanGeom &g, const rtlpower_route_opts &o, int S, int nreads, bool two)
{
	size_t batch = ((size_t)1 << (two ? 27 : 28)) / ((size_t)S * g.chunks * g.N);
	if (batch < 1) batch = 1;
	if (batch > (size_t)nreads) batch = (size_t)nreads;
	if (two && ((size_t)nreads + batch - 1) / batch < 4) {
		const size_t want = nreads < 4 ? (size_t)nreads : 4, b2 = ((size_t)nreads + want - 1) / want;
		if (((size_t)S * b2) << (c.bin_e - 14) >= 2048) batch = b2;  // (eight combs per CU and batch: 512 made a one-stream scan of 2^21 bins 1.6 x slower)
	}
	if (o.staged_batch > 0 && (size_t)o.staged_batch < batch) batch = (size_t)o.staged_batch;
	return batch;
}

// Which way `nreads` reads of S streams go, from the configuration, its geometry, the options and where the rows lie -
// nothing else: not what a handle has allocated, not what it ran before.
static ScanPlan plan_scan(const rtlpower_cfg &c, const ScanGeom &g, const rtlpower_route_opts &o, int S, int nreads,
                          size_t stride, unsigned addr_low)
{
	ScanPlan p;
	if (c.bin_e == 0) return p;
	// the conditions the fast kernels share
	const bool rows16 = !(stride & 15) && !(addr_low & 15) && !(c.buf_len & 15);  // rows take 16-byte loads
	const bool one_frame = !g.decimates && g.chunks == 1 && g.len_dec == 2 * g.N;  // a read is exactly one undecimated frame
	const bool whole = c.buf_len == (uint32_t)g.len_dec;  // ... and every byte of it (downsample > 1 without -F or boxcar divides len_dec only)
	const int Pr = g.len_dec / 2;
	const bool pow2_frames = Pr >= 512 && Pr <= 8192 && (Pr & (Pr - 1)) == 0 && g.len_dec == 2 * Pr;  // a decimated read is whole power-of-two frames
	// a decimated scan whose reads are whole frames of at least 512 points: two launches (power_kernels.h)
	const bool by_fifth = !c.boxcar && c.downsample_passes >= 1 && c.downsample_passes <= kDecMaxPasses &&
	                      (int)((c.buf_len / 2) >> c.downsample_passes) == Pr;
	const bool by_boxcar = c.boxcar && c.downsample > 1 && (long long)(c.buf_len / 2) == (long long)Pr * c.downsample;
	if (o.dec_fast && g.decimates && !g.staged && pow2_frames && rows16 && c.bin_e >= 3 && g.N <= Pr && (by_fifth || by_boxcar)) {
		p.route = RTLPOWER_KERNEL_DECIMATED;
		p.Pr = Pr; p.by_fifth = by_fifth; p.by_boxcar = by_boxcar;
		for (p.dec_e = 9; (1 << p.dec_e) < Pr; p.dec_e++) {}
		p.M = 8192;  // k_power_scan_frames<13, true> transforms groups of M / Pr reads
		p.groups = groups_per_stream(S, o.groups, (nreads + (p.M / Pr) - 1) / (p.M / Pr));
	} else if (g.staged) {
		// bin_e 15 .. 21 (or frames beyond one workgroup's LDS): the same stages over a work buffer in HBM, a batch of reads
		// at a time.  rtl_power's own fine-bin shape - an undecimated read is exactly one frame - takes the kernels written for it
		p.fast_shape = c.bin_e > 14 && !g.decimates && g.chunks == 1;
		p.fast = o.staged_fast && p.fast_shape && one_frame && whole && rows16;
		p.two = p.fast_shape && o.staged_fast && (o.staged_pipe == 2 || (o.staged_pipe == 1 && c.bin_e >= 18));
		p.batch = staged_batch_reads(c, g, o, S, nreads, p.two);
		p.piped = p.fast && p.two && (o.staged_pipe == 2 || (size_t)nreads > p.batch);
		p.route = p.fast ? RTLPOWER_KERNEL_STAGED_FAST : RTLPOWER_KERNEL_STAGED;
	} else {
		// in one workgroup's LDS.  k_power_scan_big: one frame of 8192 / 16384 points per read; k_power_scan_frames: several
		// frames per read (rtl_power's everyday shape: every scan below 8192 bins reads 16384 bytes), reads of exactly 8192
		// or 16384 points; k_power_scan: anything
		p.M = g.chunks * g.N;
		p.big = one_frame && (c.bin_e == 13 || c.bin_e == 14) && rows16;
		p.frames = o.scan_frames && !g.decimates && g.chunks > 1 && c.bin_e >= 3 && (p.M == 8192 || p.M == 16384) &&
		           g.len_dec == 2 * p.M && whole && rows16;
		p.route = p.big ? RTLPOWER_KERNEL_BIG : p.frames ? RTLPOWER_KERNEL_FRAMES : RTLPOWER_KERNEL_GENERAL;
		p.groups = groups_per_stream(S, o.groups, nreads);
	}
	p.grid = (unsigned)S * (unsigned)p.groups;
	return p;
}

extern "C" int rtlpower_scan_route(const rtlpower_cfg *cfg, int nstreams, int nreads, size_t stream_stride, unsigned addr_low_bits,
                                   const rtlpower_route_opts *opts)
{
	if (!cfg || nstreams < 1 || nreads < 1) return -EINVAL;
	const int v = validate(cfg);
	if (v < 0) return v;
	if (stream_stride < (size_t)nreads * cfg->buf_len) return -EINVAL;
	return plan_scan(*cfg, scan_geometry(*cfg), opts ? *opts : kRouteDefaults, nstreams, nreads, stream_stride, addr_low_bits).route;
}

static int timing_begin(rtlpower_gpu *h, std::pair<Event, Event> &ev)
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
static int timing_end(rtlpower_gpu *h, std::pair<Event, Event> &ev)
{
	if (!h->timing) return 0;
	HIP_TRY(hipEventRecord(ev.second, h->stream));
	h->ev_pending.push_back(std::move(ev));
	return 0;
}

// A kernel's dynamic-LDS limit, raised in front of its first launch: once per handle, not per process - the attribute
// belongs to the device the handle lives on, and one process may hold handles on several
enum : unsigned { kLdsScan = 1, kLdsBig13 = 2, kLdsBig14 = 4, kLdsFrames13 = 8, kLdsFrames14 = 16, kLdsFrames16 = 32, kLdsFft = 64, kLdsComb = 128 };
template <class K> static int raise_lds(rtlpower_gpu *h, unsigned bit, K kernel)
{
	if (h->lds_raised & bit) return 0;
	HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024));
	h->lds_raised |= bit;
	return 0;
}

struct ScanInput {  // stream s, read r at d_iq + s * stride + r * buf_len
	const uint8_t *d_iq;
	size_t stride;
	int nreads;
};
struct Decimated {  // decimate_general's output: stream s, read r at dec + s * dss + r * drs (int16 elements)
	const int16_t *dec = nullptr;
	size_t dss = 0, drs = 0;
};

static int scan_rms(rtlpower_gpu *h, const ScanInput &in)
{
	k_power_rms<<<h->nstreams, 256, 0, h->stream>>>(in.d_iq, in.stride, in.nreads, (int)h->cfg.buf_len, h->cfg.peak_hold, h->d_avg, h->d_samples);
	HIP_TRY(hipGetLastError());
	return 0;
}

// k_power_downsample_iq (-F) or k_power_boxcar into packed int16 pairs, k_power_scan_frames<13, true> on them
static int scan_decimated(rtlpower_gpu *h, const ScanPlan &pl, const ScanInput &in)
{
	const rtlpower_cfg &c = h->cfg;
	const int S = h->nstreams, Pr = pl.Pr, nreads = in.nreads;
	hipStream_t q = h->stream;
	if (pl.by_fifth) {
		DecimateParams dp{};
		dp.iq8 = in.d_iq; dp.stride8 = in.stride; dp.nreads = nreads; dp.buf_len = (int)c.buf_len;
		dp.passes = c.downsample_passes; dp.fir = c.comp_fir_size;
		dp.out = h->d_dec32; dp.out_stream_stride = (size_t)nreads * Pr; dp.out_per_read = Pr;
		dp.tile_out = kDecTileIn >> c.downsample_passes;
		dp.tiles_per_read = (Pr + dp.tile_out - 1) / dp.tile_out;
		dp.total_tiles = (size_t)S * nreads * dp.tiles_per_read;
		const unsigned g = (unsigned)(dp.total_tiles < 256 * 20 ? dp.total_tiles : 256 * 20);
		switch (c.downsample_passes) {
		case 1: k_power_downsample_iq<1><<<g, 256, 0, q>>>(dp); break;
		case 2: k_power_downsample_iq<2><<<g, 256, 0, q>>>(dp); break;
		case 3: k_power_downsample_iq<3><<<g, 256, 0, q>>>(dp); break;
		case 4: k_power_downsample_iq<4><<<g, 256, 0, q>>>(dp); break;
		case 5: k_power_downsample_iq<5><<<g, 256, 0, q>>>(dp); break;
		default: k_power_downsample_iq<6><<<g, 256, 0, q>>>(dp); break;
		}
	} else {
		k_power_boxcar<<<grid_for((size_t)S * nreads * Pr), 256, 0, q>>>(
		    in.d_iq, in.stride, nreads, (int)c.buf_len, c.downsample, S, reinterpret_cast<int16_t *>(h->d_dec32.get()),
		    (size_t)nreads * 2 * Pr, (size_t)2 * Pr, Pr);
	}
	ScanParams p{};
	p.dec32 = h->d_dec32; p.dec32_stream_stride = (size_t)nreads * Pr; p.dec_e = pl.dec_e;
	p.nreads = nreads; p.bin_e = c.bin_e; p.ds = c.downsample; p.peak_hold = c.peak_hold;
	p.window16 = h->d_window16; p.tw = h->d_tw; p.avg = h->d_avg; p.samples = h->d_samples;
	p.groups = pl.groups;
	OWN_TRY(raise_lds(h, kLdsFrames16, k_power_scan_frames<13, true>));
	const size_t lds16 = ((size_t)skewed_size(pl.M) + (size_t)h->N) * 4;
	hipLaunchKernelGGL((k_power_scan_frames<13, true>), dim3(pl.grid), dim3(kThreads), lds16, q, p);
	return 0;
}

// The general decimation: the boxcar, or one launch per fifth_order pass and generic_fir, into int16 pairs
static int decimate_general(rtlpower_gpu *h, const ScanInput &in, Decimated *out)
{
	const rtlpower_cfg &c = h->cfg;
	const int S = h->nstreams, nreads = in.nreads;
	hipStream_t q = h->stream;
	const size_t drs = (size_t)c.buf_len, dss = drs * nreads;  // elements reserved per read, per stream
	OWN_TRY(h->d_decA.grow((size_t)S * dss, q));
	OWN_TRY(h->d_decB.grow((size_t)S * dss, q));
	int16_t *cur = h->d_decA, *oth = h->d_decB;
	if (c.boxcar) {
		const int out_cplx = h->dec_elems / 2;
		k_power_boxcar<<<grid_for((size_t)S * nreads * out_cplx), 256, 0, q>>>(
		    in.d_iq, in.stride, nreads, (int)c.buf_len, c.downsample, S, cur, dss, drs, out_cplx);
	} else {
		for (int j = 0; j < c.downsample_passes; j++) {
			const int length = (int)c.buf_len >> j;
			k_power_fifth<<<grid_for((size_t)S * nreads * (length / 4)), 256, 0, q>>>(
			    j == 0 ? in.d_iq : nullptr, in.stride, j == 0 ? nullptr : cur, dss, drs, nreads, (int)c.buf_len,
			    length, S, j == 0 ? cur : oth, dss, drs);
			if (j > 0) std::swap(cur, oth);
		}
		if (c.comp_fir_size == 9) {
			const int cplx = ((int)c.buf_len >> c.downsample_passes) / 2;
			k_power_fir9<<<grid_for((size_t)S * nreads * cplx), 256, 0, q>>>(cur, oth, dss, drs, nreads, cplx, S,
			                                                               c.downsample_passes);
			std::swap(cur, oth);
		}
	}
	*out = Decimated{cur, dss, drs};
	return 0;
}

// ---- the staged route: a batch of reads at a time through work buffers in HBM ----

// Elements per set of the work buffers (piped: batch k uses set k & 1); the handle's allocation holds work_reads reads per set
struct StagedSets {
	size_t work, ave, tbuf, part;
};
static StagedSets staged_sets(const rtlpower_gpu *h, size_t reads)
{
	const size_t M = (size_t)h->chunks * h->N, n = (size_t)h->nstreams * reads;
	return {n * M, n, n * M * 2, n * (M / 8192)};
}

// Work buffers for pl.batch reads per set: kept from scan to scan, allocated anew where a scan needs more
static int staged_reserve(rtlpower_gpu *h, const ScanPlan &pl)
{
	if (h->work_reads >= pl.batch && (h->work_two || !pl.two)) return 0;
	HIP_TRY(hipStreamSynchronize(h->stream));
	if (h->pipe.aux) HIP_TRY(hipStreamSynchronize(h->pipe.aux));
	h->d_work.reset(); h->d_ave.reset(); h->d_tbuf.reset(); h->d_part.reset();
	h->work_reads = 0; h->work_two = false;
	const StagedSets n = staged_sets(h, (pl.two ? 2 : 1) * pl.batch);
	OWN_TRY(h->d_work.alloc(n.work));
	OWN_TRY(h->d_ave.alloc(n.ave));
	if (pl.fast_shape) {
		OWN_TRY(h->d_tbuf.alloc(n.tbuf));
		OWN_TRY(h->d_part.alloc(n.part));
	}
	h->work_reads = pl.batch; h->work_two = pl.two;
	return 0;
}

static int pipe_create(rtlpower_gpu *h)
{
	if (h->pipe.aux) return 0;
	int lo = 0, hi = 0;
	HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
	HIP_TRY(rtl_pool::stream_get(h->device, lo, &h->pipe.aux));  // (a priority of its own: a hardware queue of its own)
	h->pipe.aux_prio = lo;
	for (Event *e : {&h->pipe.start, &h->pipe.prep[0], &h->pipe.prep[1], &h->pipe.scanned[0], &h->pipe.scanned[1], &h->pipe.done})
		OWN_TRY(e->create(hipEventDisableTiming));
	return 0;
}

// One batch: reads r0 .. r0 + nb - 1 of every stream, into and out of set `set` of the work buffers
struct StagedBatch {
	int r0, nb, set;
	size_t frames;
	StagedSets at;  // where the set begins in each buffer
	StagedParams sp;
};
static StagedBatch staged_batch(rtlpower_gpu *h, const ScanPlan &pl, const ScanInput &in, const Decimated &d, int r0, int set)
{
	const rtlpower_cfg &c = h->cfg;
	StagedBatch b{};
	b.r0 = r0; b.nb = in.nreads - r0 < (int)pl.batch ? in.nreads - r0 : (int)pl.batch; b.set = set;
	b.frames = (size_t)h->nstreams * b.nb * h->chunks;
	const StagedSets n = staged_sets(h, h->work_reads);
	b.at = {set * n.work, set * n.ave, set * n.tbuf, set * n.part};
	StagedParams &sp = b.sp;
	sp.iq8 = d.dec ? nullptr : in.d_iq + (size_t)r0 * c.buf_len; sp.stride8 = in.stride;
	sp.dec = d.dec ? d.dec + (size_t)r0 * d.drs : nullptr; sp.dec_stream_stride = d.dss; sp.dec_read_stride = d.drs; sp.dec_elems = h->dec_elems;
	sp.nreads = b.nb; sp.buf_len = (int)c.buf_len; sp.len_dec = h->len_dec; sp.bin_e = c.bin_e; sp.chunks = h->chunks;
	sp.ds = c.downsample; sp.peak_hold = c.peak_hold; sp.window = h->d_window; sp.tw = h->d_tw;
	sp.ave = h->d_ave + b.at.ave; sp.work = h->d_work + b.at.work; sp.avg = h->d_avg; sp.samples = h->d_samples; sp.nstreams = h->nstreams;
	return b;
}

// the fast front: the comb gather and remove_dc's averages of a batch, on qa ...
static void staged_comb(rtlpower_gpu *h, const StagedBatch &b, hipStream_t qa)
{
	const rtlpower_cfg &c = h->cfg;
	const size_t frames = (size_t)h->nstreams * b.nb, tiles = frames << (c.bin_e - 13);
	k_power_comb_bytes<<<grid_for(tiles, 1, 256 * 32), 256, 0, qa>>>(b.sp.iq8, b.sp.stride8, b.nb, (int)c.buf_len, c.bin_e, tiles,
	                                                                   h->d_tbuf + b.at.tbuf, h->d_part + b.at.part);
	k_power_dc_fin<<<grid_for(frames, 64), 64, 0, qa>>>(h->d_part + b.at.part, 1 << (c.bin_e - 13), h->len_dec, frames, b.sp.ave);
}

// ... and stages 0 .. 13 of every comb in LDS, on the handle's stream
static void staged_transform(rtlpower_gpu *h, const StagedBatch &b)
{
	ScanParams cp{};
	cp.iq8 = h->d_tbuf + b.at.tbuf; cp.window16 = h->d_window16T; cp.tw = h->d_tw; cp.ave = b.sp.ave; cp.work = b.sp.work;
	cp.comb_c = h->cfg.bin_e - 14; cp.comb_blocks = b.frames << cp.comb_c;
	const size_t lds_big = ((size_t)skewed_size(16384) + 16384) * 4;
	const unsigned wgs = (unsigned)(cp.comb_blocks < 256 ? cp.comb_blocks : 256);
	hipLaunchKernelGGL((k_power_scan_big<14, true>), dim3(wgs), dim3(kThreads), lds_big, h->stream, cp);
}

// the general front: remove_dc, the points to their places in the work buffer, the stages one workgroup's LDS holds
static void staged_front_general(rtlpower_gpu *h, const StagedBatch &b)
{
	const rtlpower_cfg &c = h->cfg;
	hipStream_t q = h->stream;
	const size_t reads = (size_t)h->nstreams * b.nb;
	k_power_dc<<<(unsigned)reads, 256, 0, q>>>(b.sp);
	if (c.bin_e >= 12) k_power_place_tiled<<<grid_for(b.frames << (c.bin_e - 12), 1, 256 * 64), 256, 0, q>>>(b.sp);
	else k_power_place<<<grid_for(reads * h->chunks * h->N, 256, 256 * 64), 256, 0, q>>>(b.sp);
	const int eb = c.bin_e < 14 ? c.bin_e : 14;
	const size_t lds = ((size_t)skewed_size(1 << eb) + ((size_t)1 << eb)) * 4, nblk = b.frames << (c.bin_e - eb);
	hipLaunchKernelGGL(k_power_fft_lds, dim3((unsigned)(nblk < 4096 ? nblk : 4096)), dim3(kThreads), lds, q, h->d_work, h->d_tw, eb, nblk);
}

// stages 14 .. bin_e - 1 over HBM on qa, three per pass; the last pass accumulates (k_power_fft_gl_acc)
static void staged_back(rtlpower_gpu *h, const StagedBatch &b, hipStream_t qa)
{
	const rtlpower_cfg &c = h->cfg;
	for (int st = 14; st < c.bin_e;) {
		const int R = c.bin_e - st >= 3 ? 3 : c.bin_e - st;
		if (st + R == c.bin_e) {
			const int g = grid_for((size_t)h->nstreams << (c.bin_e - R), 256, 256 * 64);
			if (R == 3) k_power_fft_gl_acc<3><<<g, 256, 0, qa>>>(b.sp, st);
			else if (R == 2) k_power_fft_gl_acc<2><<<g, 256, 0, qa>>>(b.sp, st);
			else k_power_fft_gl_acc<1><<<g, 256, 0, qa>>>(b.sp, st);
		} else {
			const int g = grid_for(b.frames << (c.bin_e - R), 256, 256 * 64);
			k_power_fft_gl<3><<<g, 256, 0, qa>>>(b.sp.work, h->d_tw, c.bin_e, st, b.frames);
		}
		st += R;
	}
	if (c.bin_e <= 14) k_power_accum<<<grid_for((size_t)h->nstreams * h->N, 256, 256 * 64), 256, 0, h->stream>>>(b.sp);
}

static int scan_staged(rtlpower_gpu *h, const ScanPlan &pl, const ScanInput &in, const Decimated &d)
{
	hipStream_t q = h->stream;
	if (pl.fast) OWN_TRY(raise_lds(h, kLdsComb, k_power_scan_big<14, true>));
	OWN_TRY(raise_lds(h, kLdsFft, k_power_fft_lds));
	if (pl.piped) OWN_TRY(pipe_create(h));
	rtlpower_gpu::Pipe &pipe = h->pipe;
	hipStream_t qa = pl.piped ? pipe.aux : q;  // where the kernels that only move bytes go
	if (pl.piped) {
		// aux starts behind what the caller has queued on q (the producer of d_iq, an earlier scan's accumulation)
		HIP_TRY(hipEventRecord(pipe.start, q));
		HIP_TRY(hipStreamWaitEvent(qa, pipe.start, 0));
		staged_comb(h, staged_batch(h, pl, in, d, 0, 0), qa);
		HIP_TRY(hipEventRecord(pipe.prep[0], qa));
	}
	for (int r0 = 0, kb = 0; r0 < in.nreads; r0 += (int)pl.batch, kb++) {
		const int set = pl.piped ? (kb & 1) : 0, r1 = r0 + (int)pl.batch;
		const StagedBatch b = staged_batch(h, pl, in, d, r0, set);
		if (!pl.fast) {
			staged_front_general(h, b);
		} else if (!pl.piped) {
			staged_comb(h, b, q);
			staged_transform(h, b);
		} else {
			// this batch's combs and averages are there (and, aux being in order, the batch before the last has left this set)
			HIP_TRY(hipStreamWaitEvent(q, pipe.prep[set], 0));
			staged_transform(h, b);
			HIP_TRY(hipEventRecord(pipe.scanned[set], q));
			// beside this batch's transform: the next batch's combs into the other set (its last user, batch kb - 1's
			// passes over HBM, is already queued on aux in front of them) ...
			if (r1 < in.nreads) {
				staged_comb(h, staged_batch(h, pl, in, d, r1, set ^ 1), qa);
				HIP_TRY(hipEventRecord(pipe.prep[set ^ 1], qa));
			}
			// ... then, once the transform is through, this batch's stages beyond 13 and its accumulation
			HIP_TRY(hipStreamWaitEvent(qa, pipe.scanned[set], 0));
		}
		staged_back(h, b, qa);
	}
	if (pl.piped) {  // the scan is complete on q when aux is through
		HIP_TRY(hipEventRecord(pipe.done, qa));
		HIP_TRY(hipStreamWaitEvent(q, pipe.done, 0));
	}
	return 0;
}

// ---- the routes in one workgroup's LDS: k_power_scan_big, k_power_scan_frames, k_power_scan ----

static int scan_in_lds(rtlpower_gpu *h, const ScanPlan &pl, const ScanInput &in, const Decimated &d)
{
	const rtlpower_cfg &c = h->cfg;
	hipStream_t q = h->stream;
	ScanParams p{};
	p.iq8 = d.dec ? nullptr : in.d_iq; p.stride8 = in.stride;
	p.dec = d.dec; p.dec_stream_stride = d.dss; p.dec_read_stride = d.drs; p.dec_elems = h->dec_elems;
	p.nreads = in.nreads; p.buf_len = (int)c.buf_len; p.len_dec = h->len_dec;
	p.bin_e = c.bin_e; p.chunks = h->chunks; p.ds = c.downsample; p.peak_hold = c.peak_hold;
	p.window = h->d_window; p.window16 = h->d_window16; p.tw = h->d_tw; p.avg = h->d_avg; p.samples = h->d_samples;
	p.groups = pl.groups;
	OWN_TRY(raise_lds(h, kLdsScan, k_power_scan));
	if (pl.big) {
		OWN_TRY(raise_lds(h, kLdsBig13, k_power_scan_big<13>));
		OWN_TRY(raise_lds(h, kLdsBig14, k_power_scan_big<14>));
	}
	if (pl.big && h->want_stamps) {
		OWN_TRY(h->d_stamps.grow((size_t)pl.grid * 4, q));
		HIP_TRY(hipMemsetAsync(h->d_stamps, 0, (size_t)pl.grid * 32, q));
		p.stamps = h->d_stamps;
		h->stamp_last = (int)pl.grid;
	}
	if (pl.frames) {
		OWN_TRY(raise_lds(h, kLdsFrames13, k_power_scan_frames<13>));
		OWN_TRY(raise_lds(h, kLdsFrames14, k_power_scan_frames<14>));
	}
	const size_t lds = ((size_t)skewed_size(pl.M) + (size_t)h->N) * 4;
	const dim3 grid(pl.grid), block(kThreads);
	if (pl.big && c.bin_e == 14) hipLaunchKernelGGL(k_power_scan_big<14>, grid, block, lds, q, p);
	else if (pl.big) hipLaunchKernelGGL(k_power_scan_big<13>, grid, block, lds, q, p);
	else if (pl.frames && pl.M == 8192) hipLaunchKernelGGL(k_power_scan_frames<13>, grid, block, lds, q, p);
	else if (pl.frames) hipLaunchKernelGGL(k_power_scan_frames<14>, grid, block, lds, q, p);
	else hipLaunchKernelGGL(k_power_scan, grid, block, lds, q, p);
	return 0;
}

extern "C" int rtlpower_gpu_scan_device(rtlpower_gpu *h, const uint8_t *d_iq, size_t stream_stride, int nreads)
{
	if (!h || !d_iq || nreads < 1) return -EINVAL;
	if (stream_stride < (size_t)nreads * h->cfg.buf_len) return -EINVAL;
	HIP_TRY(hipSetDevice(h->device));
	const ScanInput in{d_iq, stream_stride, nreads};
	const ScanPlan pl = plan_scan(h->cfg, *h, h->opt, h->nstreams, nreads, stream_stride, (unsigned)((uintptr_t)d_iq & 15));
	rtl_debug::poison_lds(h->stream);  // RTLFM_POISON=1 only
	if (pl.route == RTLPOWER_KERNEL_NONE) return scan_rms(h, in);  // (no timing, and last_kernel stays)
	// outside the timed region: the general decimation and what the route allocates (growing waits for the stream)
	Decimated dec;
	if (pl.route == RTLPOWER_KERNEL_DECIMATED) OWN_TRY(h->d_dec32.grow((size_t)h->nstreams * nreads * pl.Pr, h->stream));
	else if (h->decimates) OWN_TRY(decimate_general(h, in, &dec));
	if (h->staged) OWN_TRY(staged_reserve(h, pl));
	std::pair<Event, Event> ev;
	OWN_TRY(timing_begin(h, ev));
	switch (pl.route) {
	case RTLPOWER_KERNEL_DECIMATED: OWN_TRY(scan_decimated(h, pl, in)); break;
	case RTLPOWER_KERNEL_STAGED:
	case RTLPOWER_KERNEL_STAGED_FAST: OWN_TRY(scan_staged(h, pl, in, dec)); break;
	default: OWN_TRY(scan_in_lds(h, pl, in, dec));
	}
	h->last_kernel = pl.route;
	HIP_TRY(hipGetLastError());
	return timing_end(h, ev);
}

extern "C" int rtlpower_gpu_scan(rtlpower_gpu *h, int stream, const uint8_t *buf, uint32_t len)
{
	// one tuning_state, one rtlsdr_read_sync() buffer (src/rtl_power.c:657): run it
	// through a one-stream view of the handle
	if (!h || !buf || stream < 0 || stream >= h->nstreams || len != h->cfg.buf_len) return -EINVAL;
	HIP_TRY(hipSetDevice(h->device));
	OWN_TRY(h->d_one.alloc(h->cfg.buf_len));
	HIP_TRY(hipMemcpyAsync(h->d_one, buf, len, hipMemcpyHostToDevice, h->stream));
	// A copy: aliases of the handle's device buffers (device_own.h), shifted to this stream.  Its work buffers - sized by the
	// scan - are its own: reset() leaves empty owners, and what the scan allocates into them goes with the view, at the end
	// of this function: behind the synchronisation, also when that failed.
	rtlpower_gpu view = *h;
	view.nstreams = 1;
	view.d_avg = h->d_avg.alias((size_t)stream * h->N);
	view.d_samples = h->d_samples.alias(stream);
	view.d_decA.reset(); view.d_decB.reset();
	view.d_work.reset(); view.d_ave.reset(); view.work_reads = 0; view.work_two = false;
	view.d_tbuf.reset(); view.d_part.reset();
	view.d_dec32.reset();
	if (!h->pipe.aux) view.pipe = rtlpower_gpu::Pipe{};  // (an owner's: whoever needs it first creates it)
	view.want_stamps = false;  // (the stamp buffer would be the view's: nothing for rtlpower_gpu_clock_read to find)
	view.ev_pending.clear(); view.ev_free.clear(); view.timing = false;
	int r = rtlpower_gpu_scan_device(&view, h->d_one, h->cfg.buf_len, 1);
	// what the view learnt about this device stays learnt (the kernels' dynamic-LDS limits are raised once per handle)
	h->lds_raised = view.lds_raised;
	h->last_kernel = view.last_kernel;
	if (!h->pipe.aux && view.pipe.aux) h->pipe = std::move(view.pipe);
	return hipStreamSynchronize(h->stream) == hipSuccess ? r : -EIO;
}

extern "C" int rtlpower_gpu_fetch(rtlpower_gpu *h, int stream, int64_t *avg, int32_t *samples)
{
	if (!h || stream < 0 || stream >= h->nstreams) return -EINVAL;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(hipStreamSynchronize(h->stream));
	if (avg) HIP_TRY(hipMemcpy(avg, h->d_avg + (size_t)stream * h->N, (size_t)h->N * sizeof(long long), hipMemcpyDeviceToHost));
	if (samples) HIP_TRY(hipMemcpy(samples, h->d_samples + stream, sizeof(int32_t), hipMemcpyDeviceToHost));
	return 0;
}

extern "C" int rtlpower_gpu_store(rtlpower_gpu *h, int stream, const int64_t *avg, int32_t samples)
{
	// the inverse of rtlpower_gpu_fetch: tuning_state.avg[] / .samples of one stream, behind what is queued
	if (!h || !avg || stream < 0 || stream >= h->nstreams) return -EINVAL;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(hipMemcpyAsync(h->d_avg + (size_t)stream * h->N, avg, (size_t)h->N * sizeof(long long), hipMemcpyHostToDevice, h->stream));
	HIP_TRY(hipMemcpyAsync(h->d_samples + stream, &samples, sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
	HIP_TRY(hipStreamSynchronize(h->stream));  // the caller's memory is free again
	return 0;
}

extern "C" int rtlpower_gpu_scan_host(rtlpower_gpu *h, const uint8_t *iq, size_t stream_stride, int nreads)
{
	// scanner()'s reads of every stream from host memory (stream s, read r at iq + s*stream_stride + r*buf_len):
	// one copy into a buffer the handle owns, one rtlpower_gpu_scan_device
	if (!h || !iq || nreads < 1) return -EINVAL;
	const size_t row = (size_t)nreads * h->cfg.buf_len;
	if (stream_stride < row) return -EINVAL;
	HIP_TRY(hipSetDevice(h->device));
	const size_t pitch = (row + 15) & ~(size_t)15;
	const size_t need = pitch * (size_t)h->nstreams;
	OWN_TRY(h->d_in.grow(need, h->stream));  // (behind an earlier scan that may still read the old buffer)
	OWN_TRY(h->ev_in.create(hipEventDisableTiming));
	HIP_TRY(hipMemcpy2DAsync(h->d_in, pitch, iq, stream_stride, row, (size_t)h->nstreams, hipMemcpyHostToDevice, h->stream));
	HIP_TRY(hipEventRecord(h->ev_in, h->stream));
	const int r = rtlpower_gpu_scan_device(h, h->d_in, pitch, nreads);
	HIP_TRY(hipEventSynchronize(h->ev_in));  // the copy has left the caller's memory; the scan itself stays asynchronous
	return r;
}

// ---- the report on the device (power_report_kernel.h) ------------------------------

static constexpr uint32_t kDoubtCap = 65536;
static constexpr size_t kRepDoubtsAt = 16, kRepSamplesAt = kRepDoubtsAt + (size_t)kDoubtCap * sizeof(ReportDoubt);
static inline size_t rep_values_at(int nstreams) { return kRepSamplesAt + (((size_t)nstreams * 4 + 15) & ~(size_t)15); }

extern "C" int rtlpower_gpu_report(rtlpower_gpu *h, double rate, double crop, int clear)
{
	// csv_dbm() (src/rtl_power.c:722-765) for every stream: enqueued behind the scans, results into pinned memory
	if (!h || !(rate > 0.0)) return -EINVAL;
	int i1 = 0, outn = 0;
	const int rr = report_range(h->cfg.bin_e, crop, &i1, &outn);
	if (rr < 0) return rr;
	HIP_TRY(hipSetDevice(h->device));
	const int S = h->nstreams;
	const size_t vals_at = rep_values_at(S);
	if (!h->ev_rep) {  // first use: sized for crop 0.  ev_rep is created last; a first use that failed half way starts over
		const size_t bytes = vals_at + (size_t)S * ((size_t)h->N + 1) * sizeof(uint32_t);
		OWN_TRY(h->d_rep.alloc(bytes));
		OWN_TRY(h->d_arrived.alloc((size_t)S));
		HIP_TRY(hipMemset(h->d_arrived, 0, (size_t)S * sizeof(uint32_t)));
		OWN_TRY(h->h_rep.alloc(bytes));
		OWN_TRY(h->ev_rep.create(hipEventDisableTiming));
	}
	if (h->rep_issued) HIP_TRY(hipEventSynchronize(h->ev_rep));  // the last report's copy has left the pinned block
	hipStream_t q = h->stream;
	ReportParams p{};
	p.avg = h->d_avg; p.samples = h->d_samples; p.len = h->N; p.i1 = i1; p.outn = outn;
	p.patch = h->cfg.bin_e > 0; p.clear = clear != 0;
	// one workgroup per stream where the streams alone fill the device, else segments of a row
	int groups = 1;
	if (S < 1024) {
		groups = (2048 + S - 1) / S;
		const int most = (h->N + 4 * kReportThreads - 1) / (4 * kReportThreads);
		if (groups > most) groups = most;
	}
	p.seg = ((h->N + groups - 1) / groups + kReportThreads - 1) / kReportThreads * kReportThreads;
	p.groups = (h->N + p.seg - 1) / p.seg;
	p.rate = rate; p.guard = (double)h->rep_guard_ppm * 1e-6;
	p.doubt_count = reinterpret_cast<uint32_t *>(h->d_rep.get());
	p.doubts = reinterpret_cast<ReportDoubt *>(h->d_rep + kRepDoubtsAt); p.doubt_cap = kDoubtCap;
	p.out_samples = reinterpret_cast<int32_t *>(h->d_rep + kRepSamplesAt);
	p.out = reinterpret_cast<uint32_t *>(h->d_rep + vals_at);
	p.arrived = h->d_arrived;
	HIP_TRY(hipMemsetAsync(h->d_rep, 0, kRepDoubtsAt, q));
	hipLaunchKernelGGL(k_power_report, dim3((unsigned)S * (unsigned)p.groups), dim3(kReportThreads), 0, q, p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(h->h_rep, h->d_rep, vals_at + (size_t)S * ((size_t)outn + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, q));
	HIP_TRY(hipEventRecord(h->ev_rep, q));
	h->rep_outn = outn + 1; h->rep_rate = rate;
	h->rep_issued = true; h->rep_resolved = false; h->rep_status = 0; h->rep_doubts = 0;
	return 0;
}

// waits for the last report's copy and decides, once, the bins the kernel left to the host
static int report_wait(rtlpower_gpu *h)
{
	if (!h->rep_issued) return -ENODATA;
	if (h->rep_resolved) return h->rep_status;
	HIP_TRY(hipSetDevice(h->device));
	HIP_TRY(hipEventSynchronize(h->ev_rep));
	const uint32_t count = *reinterpret_cast<const uint32_t *>(h->h_rep.get());
	h->rep_doubts = (long)count;
	h->rep_resolved = true;
	if (count > kDoubtCap) {
		fprintf(stderr, "rtlpower_hip: the report left %u bins to the host, the list holds %u; nothing is guessed\n", count, kDoubtCap);
		return h->rep_status = -EOVERFLOW;
	}
	const ReportDoubt *d = reinterpret_cast<const ReportDoubt *>(h->h_rep + kRepDoubtsAt);
	const int32_t *samples = reinterpret_cast<const int32_t *>(h->h_rep + kRepSamplesAt);
	uint32_t *vals = reinterpret_cast<uint32_t *>(h->h_rep + rep_values_at(h->nstreams));
	for (uint32_t k = 0; k < count; k++) {
		if (d[k].stream < 0 || d[k].stream >= h->nstreams || d[k].j < 0 || d[k].j >= h->rep_outn) return h->rep_status = -EIO;
		vals[(size_t)d[k].stream * h->rep_outn + d[k].j] =
		    report_centi_one(d[k].avg, samples[d[k].stream], h->rep_rate, d[k].j == h->rep_outn - 1);
	}
	return h->rep_status = 0;
}

extern "C" int rtlpower_gpu_report_fetch(rtlpower_gpu *h, int stream, int32_t *centi, int cap, int *n, int32_t *samples)
{
	if (!h || stream < 0 || stream >= h->nstreams || cap < 0) return -EINVAL;
	const int r = report_wait(h);
	if (r < 0) return r;
	const int32_t ns = reinterpret_cast<const int32_t *>(h->h_rep + kRepSamplesAt)[stream];
	const int len = ns == 0 ? 0 : h->rep_outn;
	if (n) *n = len;
	if (samples) *samples = ns;
	if (len > cap || (len && !centi)) return -ENOBUFS;
	if (len) memcpy(centi, h->h_rep + rep_values_at(h->nstreams) + (size_t)stream * h->rep_outn * 4, (size_t)len * 4);
	return 0;
}

extern "C" int rtlpower_gpu_report_fetch_all(rtlpower_gpu *h, int32_t *centi, size_t stream_stride, int32_t *n, int32_t *samples)
{
	// every stream: values of stream s at centi + s*stream_stride (int32 elements), n[s] of them (0 where samples[s] == 0)
	if (!h || !centi) return -EINVAL;
	const int r = report_wait(h);
	if (r < 0) return r;
	if (stream_stride < (size_t)h->rep_outn) return -ENOBUFS;
	const int32_t *ns = reinterpret_cast<const int32_t *>(h->h_rep + kRepSamplesAt);
	const uint8_t *vals = h->h_rep + rep_values_at(h->nstreams);
	for (int s = 0; s < h->nstreams; s++) {
		const int len = ns[s] == 0 ? 0 : h->rep_outn;
		if (n) n[s] = len;
		if (samples) samples[s] = ns[s];
		if (len) memcpy(centi + (size_t)s * stream_stride, vals + (size_t)s * h->rep_outn * 4, (size_t)len * 4);
	}
	return 0;
}
