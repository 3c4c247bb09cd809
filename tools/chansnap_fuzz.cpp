// tools/chansnap_fuzz.cpp — the channel snapshot's reader (rtlsdr_amd/csrc/chansnap.cpp) under AddressSanitizer + UBSan.
//
// A stand-alone CPU program, modelled on tools/snapshot_fuzz.cpp: it is compiled TOGETHER with chansnap.cpp (and with
// snapshot.cpp, for the two kinds' refusal of each other's files), is never loaded into Python and needs no GPU.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer
//       -o chansnap_fuzz tools/chansnap_fuzz.cpp rtlsdr_amd/csrc/chansnap.cpp rtlsdr_amd/csrc/snapshot.cpp   (one command line)
//   ./chansnap_fuzz [seed] [mutations]
//
// For a few good files - no history; a filter with an odd tap count, so that every later section is unaligned; a bank with
// source_dc - it feeds rtlfm_chansnap_info / rtlfm_chansnap_read
//   - the smallest file cut at every length, the others cut around every section's ends,
//   - single bytes flipped (every byte of the smallest file and of every header, a stride through the rest),
//   - every header field at out-of-range values with the checksum made right again,
//   - bytes behind the checksum, an RTLFMSNP file, and the RTLFMCHN file to the RTLFMSNP reader,
//   - `mutations` (default 4 000) seeded random mutations: a few random byte changes, half of them aimed at the header, a
//     random cut or extension, with the checksum repaired in half of them so that the header checks are reached,
// each time into heap blocks of EXACTLY the sizes the call was told, so that a write past them is a sanitizer report, and
// filled with a sentinel, so that a write INTO them by a refused file is noticed here.  Whatever the reader accepts must be
// a consistent file: its length is the one its header implies and every output is the file's bytes.
// Exit status 0 and the line "chansnap_fuzz: ok ..." when nothing was reported.
#include <unistd.h>

#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../include/rtlfm_chansnap.h"
#include "../include/rtlfm_snapshot.h"

namespace {

constexpr uint8_t kSentinel = 0x5A;
constexpr size_t kHeader = 68;
long g_calls = 0, g_accepted = 0, g_refused = 0;

uint64_t fnv1a64(const uint8_t *p, size_t n)
{
	uint64_t h = 0xcbf29ce484222325ull;
	for (size_t i = 0; i < n; i++) { h ^= p[i]; h *= 0x100000001b3ull; }
	return h;
}

void repair_sum(std::vector<uint8_t> &f)
{
	if (f.size() < 8) return;
	const uint64_t h = fnv1a64(f.data(), f.size() - 8);
	for (int i = 0; i < 8; i++) f[f.size() - 8 + i] = (uint8_t)(h >> (8 * i));
}

void put_file(const std::string &path, const std::vector<uint8_t> &f)
{
	FILE *fp = fopen(path.c_str(), "wb");
	if (!fp || (!f.empty() && fwrite(f.data(), 1, f.size(), fp) != f.size())) { perror(path.c_str()); exit(2); }
	fclose(fp);
}

std::vector<uint8_t> get_file(const std::string &path)
{
	std::vector<uint8_t> out;
	FILE *fp = fopen(path.c_str(), "rb");
	if (!fp) { perror(path.c_str()); exit(2); }
	uint8_t buf[4096];
	size_t k;
	while ((k = fread(buf, 1, sizeof(buf), fp)) > 0) out.insert(out.end(), buf, buf + k);
	fclose(fp);
	return out;
}

[[noreturn]] void die(const char *what, const char *name, long r)
{
	fprintf(stderr, "chansnap_fuzz: FAILED: %s (%s, code %ld)\n", what, name, r);
	exit(1);
}

uint32_t get32(const std::vector<uint8_t> &f, size_t at)
{
	uint32_t v = 0;
	for (int i = 0; i < 4; i++) v |= (uint32_t)f[at + i] << (8 * i);
	return v;
}

void put32(std::vector<uint8_t> &f, size_t at, uint32_t v)
{
	for (int i = 0; i < 4; i++) f[at + i] = (uint8_t)(v >> (8 * i));
}

// element counts a call announces: steps, filter taps, bank taps, bins, records, history bytes, bias words
struct Caps { size_t steps, fir, bank, bins, states, hist, dc; };

// a heap block of exactly `bytes` (one byte where that is nothing), filled with the sentinel
uint8_t *block(size_t bytes)
{
	uint8_t *p = (uint8_t *)malloc(bytes ? bytes : 1);
	if (!p) exit(2);
	memset(p, kSentinel, bytes ? bytes : 1);
	return p;
}

bool clean(const uint8_t *p, size_t bytes)
{
	for (size_t i = 0; i < bytes; i++)
		if (p[i] != kSentinel) return false;
	return true;
}

// the section lengths a header implies, from the file's own bytes (only called for accepted files)
struct Lens { size_t n, fir, bank, bins, hist, dc; };
Lens lens_of(const std::vector<uint8_t> &f)
{
	Lens l;
	l.n = get32(f, 20);
	const size_t nsrc = l.n / get32(f, 24);
	const uint32_t flags = get32(f, 28);
	l.fir = get32(f, 40);
	l.bank = get32(f, 52);
	l.bins = get32(f, 48) ? l.n : 0;
	l.hist = (flags & 2) ? nsrc * 8192 : 0;
	l.dc = (flags & 3) == 3 ? nsrc * 16 : 0;
	return l;
}

// one file through both readers, with exactly `c` of room
void feed(const std::string &path, const std::vector<uint8_t> &f, const Caps &c, const char *name)
{
	put_file(path, f);
	g_calls++;
	const size_t bytes[8] = {sizeof(rtlfm_cfg), c.steps * 4, c.fir * 2, c.bank * 2, c.bins * 4, c.states * sizeof(rtlfm_stream_state), c.hist, c.dc * 4};
	uint8_t *blk[8];
	for (int i = 0; i < 8; i++) blk[i] = block(bytes[i]);
	uint8_t *hdr = block(sizeof(rtlfm_chansnap_hdr));
	rtlfm_chansnap_bufs b;
	b.cfg = (rtlfm_cfg *)blk[0];
	b.steps = (uint32_t *)blk[1]; b.cap_steps = c.steps;
	b.fir_taps = (int16_t *)blk[2]; b.cap_fir_taps = c.fir;
	b.bank_taps = (int16_t *)blk[3]; b.cap_bank_taps = c.bank;
	b.bins = (int32_t *)blk[4]; b.cap_bins = c.bins;
	b.states = (rtlfm_stream_state *)blk[5]; b.cap_states = c.states;
	b.hist = blk[6]; b.cap_hist = c.hist;
	b.dc = (uint32_t *)blk[7]; b.cap_dc = c.dc;
	const int r = rtlfm_chansnap_read(path.c_str(), (rtlfm_chansnap_hdr *)hdr, &b);
	uint8_t *ihdr = block(sizeof(rtlfm_chansnap_hdr)), *icfg = block(sizeof(rtlfm_cfg));
	const int ri = rtlfm_chansnap_info(path.c_str(), (rtlfm_chansnap_hdr *)ihdr, (rtlfm_cfg *)icfg);
	if (ri == 0) {
		const Lens l = lens_of(f);
		size_t at = kHeader;
		const size_t want[8] = {sizeof(rtlfm_cfg), l.n * 4, l.fir * 2, l.bank * 2, l.bins * 4, l.n * sizeof(rtlfm_stream_state), l.hist, l.dc * 4};
		size_t total = kHeader + 8;
		for (size_t w : want) total += w;
		if (l.n < 1 || total != f.size()) die("an accepted file is inconsistent", name, (long)l.n);
		if (memcmp(icfg, f.data() + kHeader, sizeof(rtlfm_cfg)) != 0) die("info: cfg differs from the file", name, ri);
		const rtlfm_chansnap_hdr *h = (const rtlfm_chansnap_hdr *)ihdr;
		if (h->nstreams != l.n || h->fir_ntaps != l.fir || h->bank_ntaps != l.bank || h->hist_samples != 4096 || h->dc_pieces != 16)
			die("info: header differs from the file", name, ri);
		const bool fits = c.steps >= l.n && c.fir >= l.fir && c.bank >= l.bank && c.bins >= l.bins && c.states >= l.n && c.hist >= l.hist && c.dc >= l.dc;
		if (fits != (r == 0)) die("read disagrees with info and the caps", name, r);
		if (!fits && r != -ENOBUFS) die("a file that does not fit is not -ENOBUFS", name, r);
		if (r == 0) {
			g_accepted++;
			if (memcmp(hdr, ihdr, sizeof(rtlfm_chansnap_hdr)) != 0) die("read and info give different headers", name, r);
			for (int i = 0; i < 8; i++) {
				if (memcmp(blk[i], f.data() + at, want[i]) != 0) die("a section differs from the file", name, i);
				if (!clean(blk[i] + want[i], bytes[i] - want[i])) die("a section was written past its length", name, i);
				at += want[i];
			}
		}
	} else {
		if (ri != -EILSEQ) die("unexpected code from info", name, ri);
		if (r != -EILSEQ) die("read accepts what info refuses", name, r);
		if (!clean(ihdr, sizeof(rtlfm_chansnap_hdr)) || !clean(icfg, sizeof(rtlfm_cfg))) die("a refused info wrote an output", name, ri);
	}
	if (r != 0) {
		g_refused++;
		if (!clean(hdr, sizeof(rtlfm_chansnap_hdr))) die("a refused read wrote the header", name, r);
		for (int i = 0; i < 8; i++)
			if (!clean(blk[i], bytes[i])) die("a refused read wrote a section", name, i);
	}
	for (int i = 0; i < 8; i++) free(blk[i]);
	free(hdr);
	free(ihdr);
	free(icfg);
}

struct Good {
	std::vector<uint8_t> bytes;
	Caps caps;                 // exactly what the file holds
	std::vector<size_t> ends;  // where every section ends
};

Good make(std::mt19937 &rng, const std::string &path, uint32_t sources, uint32_t per, uint32_t fir, uint32_t K, uint32_t bank_ntaps, bool source_dc)
{
	const uint32_t n = sources * per;
	const bool hist = fir > 0 || K > 0;
	rtlfm_cfg cfg;
	std::vector<rtlfm_stream_state> st(n);
	std::vector<uint32_t> steps(n), dc(sources * 16);
	std::vector<int16_t> ft(fir), bt(bank_ntaps);
	std::vector<int32_t> bins(n);
	std::vector<uint8_t> hb(hist ? sources * 8192 : 0);
	for (size_t i = 0; i < sizeof(cfg); i++) ((uint8_t *)&cfg)[i] = (uint8_t)rng();
	for (size_t i = 0; i < st.size() * sizeof(st[0]); i++) ((uint8_t *)st.data())[i] = (uint8_t)rng();
	for (auto &v : steps) v = (uint32_t)rng();
	for (auto &v : dc) v = (uint32_t)rng();
	for (auto &v : ft) v = (int16_t)rng();
	for (auto &v : bt) v = (int16_t)rng();
	for (auto &v : bins) v = K ? (int32_t)(rng() % K) : 0;
	for (auto &v : hb) v = (uint8_t)rng();
	rtlfm_chansnap_hdr h;
	memset(&h, 0, sizeof(h));
	h.pos = ((uint64_t)rng() << 32) | rng();
	h.nstreams = n; h.per_source = per;
	h.flags = (source_dc ? RTLFM_CHANSNAP_FLAG_SOURCE_DC : 0u) | (hist ? RTLFM_CHANSNAP_FLAG_HISTORY : 0u);
	h.fir_ntaps = fir; h.fir_shift = fir ? rng() % 31 : 0;
	h.bank_K = K; h.bank_ntaps = K ? bank_ntaps : 0; h.bank_shift = K ? rng() % 31 : 0;
	rtlfm_chansnap_parts p;
	p.cfg = &cfg; p.steps = steps.data(); p.fir_taps = ft.data(); p.bank_taps = bt.data(); p.bins = bins.data(); p.states = st.data();
	p.hist = hb.data(); p.dc = dc.data();
	const int r = rtlfm_chansnap_write(path.c_str(), &h, &p);
	if (r < 0) die("the writer failed", "write", r);
	Good g;
	g.bytes = get_file(path);
	g.caps = Caps{n, fir, K ? bank_ntaps : 0, K ? n : 0, n, hb.size(), hist && source_dc ? (size_t)sources * 16 : 0};
	const size_t lens[] = {kHeader, sizeof(rtlfm_cfg), g.caps.steps * 4, g.caps.fir * 2, g.caps.bank * 2, g.caps.bins * 4, n * sizeof(rtlfm_stream_state),
	                       g.caps.hist, g.caps.dc * 4, 8};
	size_t at = 0;
	for (size_t l : lens) g.ends.push_back(at += l);
	if (at != g.bytes.size()) die("the writer's file has another length than the layout says", "write", (long)g.bytes.size());
	return g;
}

}  // namespace

int main(int argc, char **argv)
{
	const unsigned seed = argc > 1 ? (unsigned)strtoul(argv[1], nullptr, 0) : 20260101u;
	const long mutations = argc > 2 ? atol(argv[2]) : 4000;
	std::mt19937 rng(seed);
	char dir[] = "/tmp/chansnap_fuzz.XXXXXX";
	if (!mkdtemp(dir)) { perror("mkdtemp"); return 2; }
	const std::string path = std::string(dir) + "/s.chn", work = std::string(dir) + "/w.chn";

	std::vector<Good> goods;
	goods.push_back(make(rng, path, 1, 1, 0, 0, 0, false));  // the smallest file there is
	goods.push_back(make(rng, path, 2, 2, 3, 0, 0, false));  // odd taps: everything behind them lies on odd 2-byte boundaries
	goods.push_back(make(rng, path, 2, 2, 0, 4, 5, true));
	long want_accepted = 0;
	for (size_t gi = 0; gi < goods.size(); gi++) {
		const Good &g = goods[gi];
		const std::vector<uint8_t> &good = g.bytes;
		feed(work, good, g.caps, "good");
		if (g_accepted != ++want_accepted) die("the good file was refused", "good", (long)gi);
		// one element less of room in every section that has any; no room at all
		Caps c;
		c = g.caps; c.steps--; feed(work, good, c, "cap steps");
		c = g.caps; c.states--; feed(work, good, c, "cap states");
		if (g.caps.fir) { c = g.caps; c.fir--; feed(work, good, c, "cap fir"); }
		if (g.caps.bank) { c = g.caps; c.bank--; feed(work, good, c, "cap bank"); }
		if (g.caps.bins) { c = g.caps; c.bins--; feed(work, good, c, "cap bins"); }
		if (g.caps.hist) { c = g.caps; c.hist--; feed(work, good, c, "cap hist"); }
		if (g.caps.dc) { c = g.caps; c.dc--; feed(work, good, c, "cap dc"); }
		feed(work, good, Caps{0, 0, 0, 0, 0, 0, 0}, "cap 0");

		// truncations and flipped bytes: all of them for the smallest file, around the sections' ends and a stride otherwise
		for (size_t cut = 0; cut < good.size(); cut++) {
			bool near = gi == 0 || cut < kHeader + 8;
			for (size_t e : g.ends) near |= cut + 2 >= e && cut <= e + 2;
			if (!near) continue;
			feed(work, std::vector<uint8_t>(good.begin(), good.begin() + (long)cut), g.caps, "truncated");
		}
		for (size_t at = 0; at < good.size(); at += (gi == 0 || at < kHeader + sizeof(rtlfm_cfg) ? 1 : 61)) {
			std::vector<uint8_t> f = good;
			f[at] ^= (uint8_t)(1u << (at % 8));
			feed(work, f, g.caps, "flipped");
		}
		if (g_accepted != want_accepted) die("a truncated or flipped file was accepted", "sweep", g_accepted);
		// wrong header fields under a checksum that is right for them
		const uint32_t vals[] = {0u, 1u, 2u, 3u, 5u, 6u, 15u, 17u, 31u, 512u, 1025u, 4095u, 4097u, 8192u, 0x7fffffffu, 0x80000000u, 0xffffffffu, 0x01000004u};
		for (size_t field = 8; field < kHeader; field += 4) {
			if (field == 32 || field == 36) continue;  // (pos: every value is a good one)
			for (uint32_t v : vals) {
				std::vector<uint8_t> f = good;
				put32(f, field, v);
				if (f == good) continue;
				repair_sum(f);
				// (a field may turn the file into another consistent one only if the length still fits: shifts and K do)
				const long before = g_accepted;
				feed(work, f, g.caps, "header field");
				const bool harmless = (field == 44 && g.caps.fir && v <= 30) || (field == 56 && g.caps.bank && v <= 30) ||
				                      (field == 28 && v == 1 && !g.caps.hist);  // (source_dc on a handle that carries no history)
				if (g_accepted != before && !harmless) die("a wrong header field was accepted", "header", (long)field);
				if (g_accepted != before) want_accepted++;
			}
		}
		{
			std::vector<uint8_t> f = good;
			f[0] ^= 0x20;
			repair_sum(f);
			feed(work, f, g.caps, "magic");
			f = good;
			memcpy(f.data(), RTLFM_SNAPSHOT_MAGIC, 8);
			repair_sum(f);
			feed(work, f, g.caps, "the other kind's magic");
		}
		for (size_t extra : {1u, 7u, 8u, 332u, 4096u}) {
			std::vector<uint8_t> f = good;
			f.resize(good.size() + extra, 0);
			feed(work, f, g.caps, "trailing bytes");
		}
		if (g.caps.bins) {
			for (int32_t v : {4, -1, 1 << 30}) {
				std::vector<uint8_t> f = good;
				put32(f, g.ends[4] + 4 * (g.caps.bins - 1), (uint32_t)v);
				repair_sum(f);
				feed(work, f, g.caps, "bin out of range");
			}
		}
		if (g_accepted != want_accepted) die("a wrong magic, trailing bytes or a bad bin were accepted", "header", g_accepted);
		// the RTLFMSNP reader refuses this kind
		put_file(work, good);
		int n = -77;
		std::vector<rtlfm_stream_state> recs(8);
		if (rtlfm_snapshot_info(work.c_str(), nullptr, &n) != -EILSEQ || n != -77) die("rtlfm_snapshot_info took an RTLFMCHN file", "kinds", n);
		if (rtlfm_snapshot_read(work.c_str(), nullptr, recs.data(), nullptr, 8, &n) != -EILSEQ || n != -77) die("rtlfm_snapshot_read took an RTLFMCHN file", "kinds", n);
	}
	{
		// ... and this reader an RTLFMSNP file
		rtlfm_cfg cfg;
		memset(&cfg, 0, sizeof(cfg));
		std::vector<rtlfm_stream_state> st(4);
		memset(st.data(), 0, st.size() * sizeof(st[0]));
		if (rtlfm_snapshot_write(path.c_str(), &cfg, 4, st.data(), nullptr) < 0) die("rtlfm_snapshot_write failed", "kinds", 0);
		feed(work, get_file(path), goods[1].caps, "an RTLFMSNP file");
		if (g_accepted != want_accepted) die("an RTLFMSNP file was accepted", "kinds", g_accepted);
	}

	// seeded random mutations
	for (long i = 0; i < mutations; i++) {
		const Good &g = goods[rng() % goods.size()];
		std::vector<uint8_t> f = g.bytes;
		const unsigned kind = rng() % 8;
		const unsigned changes = 1 + rng() % 4;
		for (unsigned c = 0; c < changes; c++) {
			// (half of the changes aim at the header, where the lengths live)
			const size_t at = (rng() & 1) ? rng() % kHeader : rng() % f.size();
			f[at] = (rng() & 1) ? (uint8_t)rng() : (uint8_t)(f[at] ^ (1u << (rng() % 8)));
		}
		if (kind == 1) f.resize(rng() % (f.size() + 1));
		if (kind == 2) f.resize(f.size() + rng() % 700, (uint8_t)rng());
		if (kind == 3) {
			// a small count in a length field, the file cut or padded towards what that implies
			const size_t fields[] = {20, 24, 40, 48, 52};
			put32(f, fields[rng() % 5], rng() % 9);
			f.resize(f.size() + (rng() % 3 ? 0 : rng() % 64), (uint8_t)rng());
		}
		if (rng() & 1) repair_sum(f);
		Caps c = g.caps;
		if (rng() % 4 == 0) c = Caps{rng() % 9, rng() % 9, rng() % 9, rng() % 9, rng() % 9, rng() % 20000, rng() % 40};
		feed(work, f, c, "mutation");
	}
	unlink(path.c_str());
	unlink(work.c_str());
	rmdir(dir);
	printf("chansnap_fuzz: ok: seed %u, %ld files through rtlfm_chansnap_read + rtlfm_chansnap_info, %ld accepted (each consistent with its "
	       "bytes), %ld refused (none touched an output)\n", seed, g_calls, g_accepted, g_refused);
	return 0;
}
