// chansnap.cpp — include/rtlfm_chansnap.h: what a handle with channels on carries, in a file.  Host code only.
//
// As snapshot.cpp: the writer never leaves `path` half written (temporary file in the same directory, fsync, rename);
// the reader believes nothing in the file before it has checked all of it, and touches none of its outputs before that.
// The sections are copied bytewise: those behind an odd number of int16 taps lie on odd 2-byte boundaries.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/rtlfm_chansnap.h"

static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "the cfg, the records and the sections are written as they lie in memory: little-endian hosts");
static_assert(sizeof(rtlfm_cfg) % 4 == 0 && sizeof(rtlfm_stream_state) % 4 == 0, "no padding between the parts of the file");

namespace {

constexpr size_t kHeader = 68;
constexpr size_t kSum = 8;
constexpr uint64_t kHistBytes = 2ull * RTLFM_CHANSNAP_HIST;

uint64_t fnv1a64(const uint8_t *p, size_t n)
{
	uint64_t h = 0xcbf29ce484222325ull;
	for (size_t i = 0; i < n; i++) {
		h ^= p[i];
		h *= 0x100000001b3ull;
	}
	return h;
}

void put_le(uint8_t *p, uint64_t v, int bytes)
{
	for (int i = 0; i < bytes; i++) p[i] = (uint8_t)(v >> (8 * i));
}

uint64_t get_le(const uint8_t *p, int bytes)
{
	uint64_t v = 0;
	for (int i = 0; i < bytes; i++) v |= (uint64_t)p[i] << (8 * i);
	return v;
}

int write_all(int fd, const uint8_t *p, size_t n)
{
	while (n) {
		const ssize_t w = write(fd, p, n);
		if (w < 0) {
			if (errno == EINTR) continue;
			return -errno;
		}
		p += w;
		n -= (size_t)w;
	}
	return 0;
}

// the whole file as it is now (only regular files: a directory or a pipe is no snapshot)
int read_file(const char *path, std::vector<uint8_t> &out)
{
	const int fd = open(path, O_RDONLY | O_CLOEXEC);
	if (fd < 0) return -errno;
	struct stat sb;
	if (fstat(fd, &sb) < 0) {
		const int e = -errno;
		close(fd);
		return e;
	}
	if (!S_ISREG(sb.st_mode)) {
		close(fd);
		return -EILSEQ;
	}
	const size_t size = (size_t)sb.st_size;
	try {
		out.resize(size);
	} catch (const std::bad_alloc &) {
		close(fd);
		return -ENOMEM;
	}
	size_t got = 0;
	int r = 0;
	while (got < size) {
		const ssize_t k = read(fd, out.data() + got, size - got);
		if (k < 0) {
			if (errno == EINTR) continue;
			r = -errno;
			break;
		}
		if (k == 0) break;  // the file shrank under us: the length check fails
		got += (size_t)k;
	}
	close(fd);
	if (r < 0) return r;
	out.resize(got);
	return 0;
}

// where every section lies; lengths in bytes
struct Layout {
	uint64_t cfg, steps, fir, bank, bins, states, hist, dc, sum;  // offsets
	uint64_t nbins, nhist, ndc;                                    // elements: int32, bytes, words
	uint64_t total;
};

// Every check a header's fields can fail on their own.  false: a reader refuses such a file.
bool header_ok(const rtlfm_chansnap_hdr &h)
{
	if (h.nstreams < 1 || h.nstreams > (uint32_t)INT32_MAX) return false;
	if (h.per_source < 1 || h.nstreams % h.per_source) return false;
	if (h.flags & ~(RTLFM_CHANSNAP_FLAG_SOURCE_DC | RTLFM_CHANSNAP_FLAG_HISTORY)) return false;
	if (h.fir_ntaps > RTLFM_CHANNEL_MAX_TAPS || h.fir_shift > 30 || (h.fir_ntaps == 0 && h.fir_shift != 0)) return false;
	if (h.bank_K == 0) {
		if (h.bank_ntaps != 0 || h.bank_shift != 0) return false;
	} else {
		if (h.bank_K < 4 || h.bank_K > 256 || (h.bank_K & (h.bank_K - 1))) return false;
		if (h.bank_ntaps < 1 || h.bank_ntaps > RTLFM_BANK_MAX_TAPS || h.bank_shift > 30) return false;
	}
	if (h.hist_samples != RTLFM_CHANSNAP_HIST || h.dc_pieces != RTLFM_CHANSNAP_DC_PIECES) return false;
	// the history is carried exactly where something re-reads it
	const bool hist = (h.flags & RTLFM_CHANSNAP_FLAG_HISTORY) != 0;
	return hist == (h.fir_ntaps > 0 || h.bank_K > 0);
}

// (64-bit throughout: 2^31 records of 328 bytes do not wrap)
Layout layout(const rtlfm_chansnap_hdr &h)
{
	Layout l;
	const uint64_t n = h.nstreams, nsrc = n / h.per_source;
	const bool hist = (h.flags & RTLFM_CHANSNAP_FLAG_HISTORY) != 0;
	l.nbins = h.bank_K ? n : 0;
	l.nhist = hist ? nsrc * kHistBytes : 0;
	l.ndc = hist && (h.flags & RTLFM_CHANSNAP_FLAG_SOURCE_DC) ? nsrc * RTLFM_CHANSNAP_DC_PIECES : 0;
	l.cfg = kHeader;
	l.steps = l.cfg + sizeof(rtlfm_cfg);
	l.fir = l.steps + 4 * n;
	l.bank = l.fir + 2ull * h.fir_ntaps;
	l.bins = l.bank + 2ull * h.bank_ntaps;
	l.states = l.bins + 4 * l.nbins;
	l.hist = l.states + n * sizeof(rtlfm_stream_state);
	l.dc = l.hist + l.nhist;
	l.sum = l.dc + 4 * l.ndc;
	l.total = l.sum + kSum;
	return l;
}

// Every check of the format on the file's bytes.  0 with the header and the layout, or -EILSEQ.
int parse(const std::vector<uint8_t> &f, rtlfm_chansnap_hdr *hdr, Layout *lay)
{
	if (f.size() < kHeader + kSum) return -EILSEQ;
	const uint8_t *p = f.data();
	if (memcmp(p, RTLFM_CHANSNAP_MAGIC, 8) != 0) return -EILSEQ;
	if (get_le(p + 8, 4) != RTLFM_CHANSNAP_VERSION) return -EILSEQ;
	if (get_le(p + 12, 4) != sizeof(rtlfm_cfg) || get_le(p + 16, 4) != sizeof(rtlfm_stream_state)) return -EILSEQ;
	rtlfm_chansnap_hdr h;
	memset(&h, 0, sizeof(h));
	h.nstreams = (uint32_t)get_le(p + 20, 4);
	h.per_source = (uint32_t)get_le(p + 24, 4);
	h.flags = (uint32_t)get_le(p + 28, 4);
	h.pos = get_le(p + 32, 8);
	h.fir_ntaps = (uint32_t)get_le(p + 40, 4);
	h.fir_shift = (uint32_t)get_le(p + 44, 4);
	h.bank_K = (uint32_t)get_le(p + 48, 4);
	h.bank_ntaps = (uint32_t)get_le(p + 52, 4);
	h.bank_shift = (uint32_t)get_le(p + 56, 4);
	h.hist_samples = (uint32_t)get_le(p + 60, 4);
	h.dc_pieces = (uint32_t)get_le(p + 64, 4);
	if (!header_ok(h)) return -EILSEQ;
	const Layout l = layout(h);
	if (l.total != (uint64_t)f.size()) return -EILSEQ;  // truncated, or bytes behind the checksum
	if (get_le(p + l.sum, 8) != fnv1a64(p, (size_t)l.sum)) return -EILSEQ;
	for (uint64_t i = 0; i < l.nbins; i++) {
		int32_t b;
		memcpy(&b, p + l.bins + 4 * i, 4);
		if (b < 0 || (uint32_t)b >= h.bank_K) return -EILSEQ;
	}
	*hdr = h;
	*lay = l;
	return 0;
}

}  // namespace

extern "C" int rtlfm_chansnap_write(const char *path, const rtlfm_chansnap_hdr *hdr, const rtlfm_chansnap_parts *parts)
{
	if (!path || !*path || !hdr || !parts || !parts->cfg || !parts->steps || !parts->states) return -EINVAL;
	rtlfm_chansnap_hdr h = *hdr;
	h.hist_samples = RTLFM_CHANSNAP_HIST;
	h.dc_pieces = RTLFM_CHANSNAP_DC_PIECES;
	if (!header_ok(h)) return -EINVAL;
	const Layout l = layout(h);
	if ((h.fir_ntaps && !parts->fir_taps) || (h.bank_ntaps && !parts->bank_taps) || (l.nbins && !parts->bins) || (l.nhist && !parts->hist))
		return -EINVAL;
	for (uint64_t i = 0; i < l.nbins; i++)
		if (parts->bins[i] < 0 || (uint32_t)parts->bins[i] >= h.bank_K) return -EINVAL;
	std::vector<uint8_t> f;
	std::string tmp;
	try {
		f.resize((size_t)l.total);
		tmp = std::string(path) + ".tmpXXXXXX";
	} catch (const std::bad_alloc &) {
		return -ENOMEM;
	}
	uint8_t *p = f.data();
	memcpy(p, RTLFM_CHANSNAP_MAGIC, 8);
	put_le(p + 8, RTLFM_CHANSNAP_VERSION, 4);
	put_le(p + 12, sizeof(rtlfm_cfg), 4);
	put_le(p + 16, sizeof(rtlfm_stream_state), 4);
	put_le(p + 20, h.nstreams, 4);
	put_le(p + 24, h.per_source, 4);
	put_le(p + 28, h.flags, 4);
	put_le(p + 32, h.pos, 8);
	put_le(p + 40, h.fir_ntaps, 4);
	put_le(p + 44, h.fir_shift, 4);
	put_le(p + 48, h.bank_K, 4);
	put_le(p + 52, h.bank_ntaps, 4);
	put_le(p + 56, h.bank_shift, 4);
	put_le(p + 60, h.hist_samples, 4);
	put_le(p + 64, h.dc_pieces, 4);
	const size_t n = h.nstreams;
	memcpy(p + l.cfg, parts->cfg, sizeof(rtlfm_cfg));
	memcpy(p + l.steps, parts->steps, 4 * n);
	if (h.fir_ntaps) memcpy(p + l.fir, parts->fir_taps, 2 * (size_t)h.fir_ntaps);
	if (h.bank_ntaps) memcpy(p + l.bank, parts->bank_taps, 2 * (size_t)h.bank_ntaps);
	if (l.nbins) memcpy(p + l.bins, parts->bins, 4 * (size_t)l.nbins);
	memcpy(p + l.states, parts->states, n * sizeof(rtlfm_stream_state));
	if (l.nhist) memcpy(p + l.hist, parts->hist, (size_t)l.nhist);
	for (uint64_t i = 0; i < l.ndc; i++) put_le(p + l.dc + 4 * i, parts->dc ? parts->dc[i] : RTLFM_CHANSNAP_DC_NONE, 4);
	put_le(p + l.sum, fnv1a64(p, (size_t)l.sum), 8);

	const int fd = mkstemp(&tmp[0]);  // in path's own directory: rename() never crosses a file system
	if (fd < 0) return -errno;
	int r = write_all(fd, p, (size_t)l.total);
	if (r == 0 && fchmod(fd, 0644) < 0) r = -errno;
	if (r == 0 && fsync(fd) < 0) r = -errno;
	if (close(fd) < 0 && r == 0) r = -errno;
	if (r == 0 && rename(tmp.c_str(), path) < 0) r = -errno;
	if (r < 0) {
		unlink(tmp.c_str());
		return r;
	}
	// the rename itself on stable storage: the directory's entry (best effort - the file is complete either way)
	std::string dir(path);
	const size_t slash = dir.rfind('/');
	dir = slash == std::string::npos ? "." : (slash == 0 ? "/" : dir.substr(0, slash));
	const int dfd = open(dir.c_str(), O_RDONLY | O_DIRECTORY | O_CLOEXEC);
	if (dfd >= 0) {
		(void)fsync(dfd);
		close(dfd);
	}
	return 0;
}

extern "C" int rtlfm_chansnap_info(const char *path, rtlfm_chansnap_hdr *hdr_out, rtlfm_cfg *cfg_out)
{
	if (!path) return -EINVAL;
	std::vector<uint8_t> f;
	int r = read_file(path, f);
	if (r < 0) return r;
	rtlfm_chansnap_hdr h;
	Layout l;
	if ((r = parse(f, &h, &l)) < 0) return r;
	if (hdr_out) *hdr_out = h;
	if (cfg_out) memcpy(cfg_out, f.data() + l.cfg, sizeof(rtlfm_cfg));
	return 0;
}

extern "C" int rtlfm_chansnap_read(const char *path, rtlfm_chansnap_hdr *hdr_out, const rtlfm_chansnap_bufs *b)
{
	if (!path || !b) return -EINVAL;
	std::vector<uint8_t> f;
	int r = read_file(path, f);
	if (r < 0) return r;
	rtlfm_chansnap_hdr h;
	Layout l;
	if ((r = parse(f, &h, &l)) < 0) return r;
	const size_t n = h.nstreams;
	if ((b->steps && b->cap_steps < n) || (b->fir_taps && b->cap_fir_taps < h.fir_ntaps) || (b->bank_taps && b->cap_bank_taps < h.bank_ntaps) ||
	    (b->bins && b->cap_bins < l.nbins) || (b->states && b->cap_states < n) || (b->hist && b->cap_hist < l.nhist) ||
	    (b->dc && b->cap_dc < l.ndc))
		return -ENOBUFS;
	const uint8_t *p = f.data();
	if (hdr_out) *hdr_out = h;
	if (b->cfg) memcpy(b->cfg, p + l.cfg, sizeof(rtlfm_cfg));
	if (b->steps) memcpy(b->steps, p + l.steps, 4 * n);
	if (b->fir_taps && h.fir_ntaps) memcpy(b->fir_taps, p + l.fir, 2 * (size_t)h.fir_ntaps);
	if (b->bank_taps && h.bank_ntaps) memcpy(b->bank_taps, p + l.bank, 2 * (size_t)h.bank_ntaps);
	if (b->bins && l.nbins) memcpy(b->bins, p + l.bins, 4 * (size_t)l.nbins);
	if (b->states) memcpy(b->states, p + l.states, n * sizeof(rtlfm_stream_state));
	if (b->hist && l.nhist) memcpy(b->hist, p + l.hist, (size_t)l.nhist);
	if (b->dc && l.ndc) memcpy(b->dc, p + l.dc, 4 * (size_t)l.ndc);
	return 0;
}
