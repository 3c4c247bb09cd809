// snapshot.cpp — include/rtlfm_snapshot.h: the carried state of many streams in a file.  Host code only.
//
// The writer never leaves `path` half written (temporary file in the same directory, fsync, rename); the reader
// believes nothing in the file before it has checked all of it, and touches none of its outputs before that.
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

#include "../../include/rtlfm_snapshot.h"

static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "the cfg and the records are written as they lie in memory: little-endian hosts");
static_assert(sizeof(rtlfm_cfg) % 4 == 0 && sizeof(rtlfm_stream_state) % 4 == 0, "no padding between the parts of the file");

namespace {

constexpr size_t kHeader = 24;  // magic, version, two sizes, count
constexpr size_t kSum = 8;

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

// write() until everything is out
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
		if (k == 0) break;  // the file shrank under us: the length check below fails
		got += (size_t)k;
	}
	close(fd);
	if (r < 0) return r;
	out.resize(got);
	return 0;
}

// Every check of the format on the file's bytes.  0 and *n = the stream count, or -EILSEQ.
int parse(const std::vector<uint8_t> &f, uint32_t *n)
{
	if (f.size() < kHeader + kSum) return -EILSEQ;
	const uint8_t *p = f.data();
	if (memcmp(p, RTLFM_SNAPSHOT_MAGIC, 8) != 0) return -EILSEQ;
	if (get_le(p + 8, 4) != RTLFM_SNAPSHOT_VERSION) return -EILSEQ;
	if (get_le(p + 12, 4) != sizeof(rtlfm_cfg) || get_le(p + 16, 4) != sizeof(rtlfm_stream_state)) return -EILSEQ;
	const uint64_t count = get_le(p + 20, 4);
	if (count < 1 || count > (uint64_t)INT32_MAX) return -EILSEQ;
	// (64-bit: 2^31 records of 332 bytes do not wrap)
	const uint64_t want = kHeader + sizeof(rtlfm_cfg) + count * (4 + sizeof(rtlfm_stream_state)) + kSum;
	if (want != (uint64_t)f.size()) return -EILSEQ;  // truncated, or bytes behind the checksum
	if (get_le(p + f.size() - kSum, 8) != fnv1a64(p, f.size() - kSum)) return -EILSEQ;
	*n = (uint32_t)count;
	return 0;
}

}  // namespace

extern "C" int rtlfm_snapshot_write(const char *path, const rtlfm_cfg *cfg, int nstreams, const rtlfm_stream_state *states,
                                    const uint32_t *mutes)
{
	if (!path || !*path || !cfg || !states || nstreams < 1) return -EINVAL;
	const size_t n = (size_t)nstreams;
	const size_t total = kHeader + sizeof(rtlfm_cfg) + n * (4 + sizeof(rtlfm_stream_state)) + kSum;
	std::vector<uint8_t> f;
	std::string tmp;
	try {
		f.resize(total);
		tmp = std::string(path) + ".tmpXXXXXX";
	} catch (const std::bad_alloc &) {
		return -ENOMEM;
	}
	uint8_t *p = f.data();
	memcpy(p, RTLFM_SNAPSHOT_MAGIC, 8);
	put_le(p + 8, RTLFM_SNAPSHOT_VERSION, 4);
	put_le(p + 12, sizeof(rtlfm_cfg), 4);
	put_le(p + 16, sizeof(rtlfm_stream_state), 4);
	put_le(p + 20, (uint64_t)n, 4);
	size_t at = kHeader;
	memcpy(p + at, cfg, sizeof(rtlfm_cfg));
	at += sizeof(rtlfm_cfg);
	for (size_t s = 0; s < n; s++) put_le(p + at + 4 * s, mutes ? mutes[s] : 0u, 4);
	at += 4 * n;
	memcpy(p + at, states, n * sizeof(rtlfm_stream_state));
	at += n * sizeof(rtlfm_stream_state);
	put_le(p + at, fnv1a64(p, at), 8);

	const int fd = mkstemp(&tmp[0]);  // in path's own directory: rename() never crosses a file system
	if (fd < 0) return -errno;
	int r = write_all(fd, p, total);
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

extern "C" int rtlfm_snapshot_info(const char *path, rtlfm_cfg *cfg_out, int *nstreams_out)
{
	if (!path) return -EINVAL;
	std::vector<uint8_t> f;
	int r = read_file(path, f);
	if (r < 0) return r;
	uint32_t n = 0;
	if ((r = parse(f, &n)) < 0) return r;
	if (cfg_out) memcpy(cfg_out, f.data() + kHeader, sizeof(rtlfm_cfg));
	if (nstreams_out) *nstreams_out = (int)n;
	return 0;
}

extern "C" int rtlfm_snapshot_read(const char *path, rtlfm_cfg *cfg_out, rtlfm_stream_state *states, uint32_t *mutes, int cap,
                                   int *n_out)
{
	if (!path || !states || !n_out || cap < 0) return -EINVAL;
	std::vector<uint8_t> f;
	int r = read_file(path, f);
	if (r < 0) return r;
	uint32_t n = 0;
	if ((r = parse(f, &n)) < 0) return r;
	if (n > (uint32_t)cap) return -ENOBUFS;
	size_t at = kHeader;
	if (cfg_out) memcpy(cfg_out, f.data() + at, sizeof(rtlfm_cfg));
	at += sizeof(rtlfm_cfg);
	if (mutes)
		for (uint32_t s = 0; s < n; s++) mutes[s] = (uint32_t)get_le(f.data() + at + 4 * (size_t)s, 4);
	at += 4 * (size_t)n;
	memcpy(states, f.data() + at, (size_t)n * sizeof(rtlfm_stream_state));
	*n_out = (int)n;
	return 0;
}
