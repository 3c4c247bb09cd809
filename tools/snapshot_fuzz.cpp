// tools/snapshot_fuzz.cpp — the snapshot reader (rtlsdr_amd/csrc/snapshot.cpp) under AddressSanitizer + UBSan.
//
// A stand-alone CPU program: it is compiled TOGETHER with snapshot.cpp, is never loaded into Python and needs no GPU.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer
//       -o snapshot_fuzz tools/snapshot_fuzz.cpp rtlsdr_amd/csrc/snapshot.cpp     (one command line)
//   ./snapshot_fuzz [seed] [mutations]
//
// It writes a good snapshot of 5 streams and feeds rtlfm_snapshot_info / rtlfm_snapshot_read
//   - the file cut at every length from 0 to its size,
//   - every single byte flipped,
//   - wrong magic / version / sizes / counts with the checksum made right again,
//   - bytes behind the checksum,
//   - `mutations` (default 10 000) seeded random mutations: a few random byte changes, a random cut or extension, with the
//     checksum repaired in half of them so that the header checks are reached and not only the sum,
// each time into output buffers allocated to EXACTLY the size the call was told (cap records), so that a write past them
// is a sanitizer report, and filled with a sentinel, so that a write INTO them by a refused file is noticed here.
// Whatever the reader accepts must be a consistent file: its count fits cap and its bytes are the ones in the file.
// Exit status 0 and the line "snapshot_fuzz: ok ..." when nothing was reported.
#include <unistd.h>

#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../include/rtlfm_snapshot.h"

namespace {

constexpr int kStreams = 5;
constexpr uint8_t kSentinel = 0x5A;
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

[[noreturn]] void die(const char *what, const char *name, int r)
{
	fprintf(stderr, "snapshot_fuzz: FAILED: %s (%s, code %d)\n", what, name, r);
	exit(1);
}

// one file through both readers, with exactly `cap` records of room
void feed(const std::string &path, const std::vector<uint8_t> &f, int cap, const char *name)
{
	put_file(path, f);
	g_calls++;
	std::vector<uint8_t> cfg(sizeof(rtlfm_cfg), kSentinel);
	// (heap blocks of exactly the announced size: one byte more is a sanitizer report)
	uint8_t *recs = (uint8_t *)malloc((size_t)cap * sizeof(rtlfm_stream_state) + (cap ? 0 : 1));
	uint8_t *mutes = (uint8_t *)malloc((size_t)cap * 4 + (cap ? 0 : 1));
	memset(recs, kSentinel, (size_t)cap * sizeof(rtlfm_stream_state));
	memset(mutes, kSentinel, (size_t)cap * 4);
	int n = -77;
	const int r = rtlfm_snapshot_read(path.c_str(), (rtlfm_cfg *)cfg.data(), (rtlfm_stream_state *)recs, (uint32_t *)mutes, cap, &n);
	rtlfm_cfg icfg;
	memset(&icfg, kSentinel, sizeof(icfg));
	int in = -77;
	const int ri = rtlfm_snapshot_info(path.c_str(), &icfg, &in);
	if (r == 0) {
		g_accepted++;
		const size_t want = 24 + sizeof(rtlfm_cfg) + (size_t)n * (4 + sizeof(rtlfm_stream_state)) + 8;
		if (n < 1 || n > cap || want != f.size()) die("an accepted file is inconsistent", name, n);
		if (memcmp(cfg.data(), f.data() + 24, sizeof(rtlfm_cfg)) != 0) die("cfg differs from the file", name, r);
		if (memcmp(mutes, f.data() + 24 + sizeof(rtlfm_cfg), (size_t)n * 4) != 0) die("mutes differ from the file", name, r);
		if (memcmp(recs, f.data() + 24 + sizeof(rtlfm_cfg) + (size_t)n * 4, (size_t)n * sizeof(rtlfm_stream_state)) != 0)
			die("records differ from the file", name, r);
		if (ri != 0 || in != n || memcmp(&icfg, f.data() + 24, sizeof(icfg)) != 0) die("info disagrees with read", name, ri);
	} else {
		g_refused++;
		if (r != -EILSEQ && r != -ENOBUFS) die("unexpected code from read", name, r);
		if (r == -EILSEQ && ri != -EILSEQ) die("read refuses what info accepts", name, ri);
		if (r == -ENOBUFS && (ri != 0 || in <= cap)) die("-ENOBUFS for a file that fits", name, ri);
		if (n != -77) die("a refused read wrote *n", name, r);
		for (uint8_t b : cfg)
			if (b != kSentinel) die("a refused read wrote the cfg", name, r);
		for (size_t i = 0; i < (size_t)cap * sizeof(rtlfm_stream_state); i++)
			if (recs[i] != kSentinel) die("a refused read wrote records", name, r);
		for (size_t i = 0; i < (size_t)cap * 4; i++)
			if (mutes[i] != kSentinel) die("a refused read wrote mutes", name, r);
		if (ri != 0) {
			const uint8_t *q = (const uint8_t *)&icfg;
			for (size_t i = 0; i < sizeof(icfg); i++)
				if (q[i] != kSentinel) die("a refused info wrote the cfg", name, ri);
			if (in != -77) die("a refused info wrote the count", name, ri);
		}
	}
	free(recs);
	free(mutes);
}

void put32(std::vector<uint8_t> &f, size_t at, uint32_t v)
{
	for (int i = 0; i < 4; i++) f[at + i] = (uint8_t)(v >> (8 * i));
}

}  // namespace

int main(int argc, char **argv)
{
	const unsigned seed = argc > 1 ? (unsigned)strtoul(argv[1], nullptr, 0) : 20260101u;
	const long mutations = argc > 2 ? atol(argv[2]) : 10000;
	std::mt19937 rng(seed);
	char dir[] = "/tmp/snapshot_fuzz.XXXXXX";
	if (!mkdtemp(dir)) { perror("mkdtemp"); return 2; }
	const std::string path = std::string(dir) + "/s.snap", work = std::string(dir) + "/w.snap";

	rtlfm_cfg cfg;
	std::vector<rtlfm_stream_state> st(kStreams);
	std::vector<uint32_t> mutes(kStreams);
	for (size_t i = 0; i < sizeof(cfg); i++) ((uint8_t *)&cfg)[i] = (uint8_t)rng();
	for (size_t i = 0; i < st.size() * sizeof(st[0]); i++) ((uint8_t *)st.data())[i] = (uint8_t)rng();
	for (uint32_t &m : mutes) m = (uint32_t)rng();
	int r = rtlfm_snapshot_write(path.c_str(), &cfg, kStreams, st.data(), mutes.data());
	if (r < 0) die("the writer failed", "write", r);
	std::vector<uint8_t> good;
	{
		FILE *fp = fopen(path.c_str(), "rb");
		if (!fp) { perror(path.c_str()); return 2; }
		uint8_t buf[4096];
		size_t k;
		while ((k = fread(buf, 1, sizeof(buf), fp)) > 0) good.insert(good.end(), buf, buf + k);
		fclose(fp);
	}
	feed(work, good, kStreams, "good");
	if (g_accepted != 1) die("the good file was refused", "good", 0);
	feed(work, good, kStreams - 1, "cap too small");
	feed(work, good, 0, "cap 0");

	// every truncation, every flipped byte
	for (size_t cut = 0; cut < good.size(); cut++) {
		std::vector<uint8_t> f(good.begin(), good.begin() + (long)cut);
		feed(work, f, kStreams, "truncated");
	}
	for (size_t at = 0; at < good.size(); at++) {
		std::vector<uint8_t> f = good;
		f[at] ^= (uint8_t)(1u << (at % 8));
		feed(work, f, kStreams, "flipped");
	}
	if (g_accepted != 1) die("a truncated or flipped file was accepted", "sweep", (int)g_accepted);
	// wrong header fields under a checksum that is right for them
	const uint32_t counts[] = {0u, 1u, 4u, 6u, 0x7fffffffu, 0x80000000u, 0xffffffffu, 0x01000005u};
	for (size_t field = 8; field < 24; field += 4)
		for (uint32_t v : counts) {
			std::vector<uint8_t> f = good;
			put32(f, field, v);
			if (f == good) continue;  // (the version IS 1)
			repair_sum(f);
			feed(work, f, kStreams, "header field");
		}
	{
		std::vector<uint8_t> f = good;
		f[0] ^= 0x20;
		repair_sum(f);
		feed(work, f, kStreams, "magic");
	}
	if (g_accepted != 1) die("a wrong header was accepted", "header", (int)g_accepted);
	for (size_t extra : {1u, 7u, 8u, 332u, 4096u}) {
		std::vector<uint8_t> f = good;
		f.resize(good.size() + extra, 0);
		feed(work, f, kStreams, "trailing bytes");
	}
	if (g_accepted != 1) die("trailing bytes were accepted", "trailing", (int)g_accepted);

	// seeded random mutations
	for (long i = 0; i < mutations; i++) {
		std::vector<uint8_t> f = good;
		const unsigned kind = rng() % 8;
		const unsigned changes = 1 + rng() % 4;
		for (unsigned c = 0; c < changes; c++) {
			// (half of the changes aim at the header, where the lengths live)
			const size_t at = (rng() & 1) ? rng() % 24 : rng() % f.size();
			f[at] = (rng() & 1) ? (uint8_t)rng() : (uint8_t)(f[at] ^ (1u << (rng() % 8)));
		}
		if (kind == 1) f.resize(rng() % (f.size() + 1));
		if (kind == 2) f.resize(f.size() + rng() % 700, (uint8_t)rng());
		if (kind == 3) {
			// a consistent file of another count, cut or padded to the length its header implies
			const uint32_t n = rng() % 9;
			put32(f, 20, n);
			f.resize(24 + sizeof(rtlfm_cfg) + (size_t)n * (4 + sizeof(rtlfm_stream_state)) + 8, (uint8_t)rng());
		}
		if (rng() & 1) repair_sum(f);
		feed(work, f, (int)(rng() % 9), "mutation");
	}
	unlink(path.c_str());
	unlink(work.c_str());
	rmdir(dir);
	printf("snapshot_fuzz: ok: seed %u, %ld files through rtlfm_snapshot_read + rtlfm_snapshot_info, %ld accepted (each consistent with its "
	       "bytes), %ld refused (none touched an output)\n", seed, g_calls, g_accepted, g_refused);
	return 0;
}
