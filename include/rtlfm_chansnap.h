/*
 * rtlfm_chansnap.h — everything a handle with channels on carries, in a file (host only, no GPU needed).
 *
 * include/rtlfm_snapshot.h holds the records of independent streams.  A handle with channels on (rtlfm_gpu_set_channels)
 * carries three things more, which no rtlfm_stream_state record holds: pos, the handle's one sample counter; every
 * SOURCE's history, its last 4096 complex samples as raw bytes, which the channel filter and the bank re-read in front
 * of every run; and, with option source_dc, what was subtracted from each of the history's sixteen 256-sample pieces.
 * This is the file for all of it - a second kind beside the RTLFMSNP snapshot, with its own magic and its own version,
 * so neither reader takes the other's files.  rtlfm_gpu_channels_save / rtlfm_gpu_channels_load (include/rtlfm_hip.h)
 * are state_get_all + channels_history_get + channels_tell, and their inverses, around these three entry points.
 *
 * Layout, little-endian, no padding between the parts:
 *
 *   offset  bytes            what
 *   0       8                magic "RTLFMCHN"
 *   8       4                format version (RTLFM_CHANSNAP_VERSION = 1)
 *   12      4                sizeof(rtlfm_cfg)           of the writer
 *   16      4                sizeof(rtlfm_stream_state)  of the writer
 *   20      4                n = stream count (>= 1)
 *   24      4                per_source (>= 1, divides n); sources = n / per_source
 *   28      4                flags: bit 0 option source_dc was on, bit 1 the history is present; no other bit
 *   32      8                pos (uint64): complex samples the sources had delivered
 *   40      4                filter: ntaps (0: none, else 1 .. RTLFM_CHANNEL_MAX_TAPS)
 *   44      4                filter: shift (0 .. 30; 0 without a filter)
 *   48      4                bank: K (0: none, else a power of two, 4 .. 256)
 *   52      4                bank: ntaps (1 .. RTLFM_BANK_MAX_TAPS; 0 without a bank)
 *   56      4                bank: shift (0 .. 30; 0 without a bank)
 *   60      4                history samples per source (RTLFM_CHANSNAP_HIST = 4096)
 *   64      4                bias pieces per source    (RTLFM_CHANSNAP_DC_PIECES = 16)
 *   68      sizeof cfg       the rtlfm_cfg, as it lies in memory
 *   ...     4 n              uint32 steps[n]: every stream's NCO phase step
 *   ...     2 filter ntaps   int16 filter taps
 *   ...     2 bank ntaps     int16 bank taps
 *   ...     4 n              int32 bins[sources][per_source] as they rule, each in [0, K)     (only with a bank)
 *   ...     n sizeof state   the records, stream 0 first
 *   ...     8192 sources     the history's bytes, per source, oldest sample first             (only with flag bit 1)
 *   ...     64 sources       uint32 bias words [sources][16], as the kernels keep them        (only with bits 0 AND 1)
 *   ...     8                64-bit FNV-1a over every byte in front of it
 *
 * Every section's length follows from the header.  The history is present exactly where a filter or a bank is set:
 * flag bit 1 says what the two tap counts say, and a file in which they disagree is refused.  Sections behind an odd
 * number of int16 taps are not aligned; the reader copies them out bytewise.
 *
 * A reader checks ALL of it before it writes anything to any output: the magic, the version, both sizes against its
 * own structs, n >= 1, per_source, the flags, both tap counts and shifts, K, the two history constants against its own,
 * the file's length against what the header implies (a truncated file and one with bytes behind the checksum both fail
 * here - and this comes before anything is sized by a count from the file), the checksum, and every bin.  Every such
 * failure is -EILSEQ; a file that cannot be opened or read is the -errno of the call that failed.  An RTLFMSNP file is
 * -EILSEQ here by its magic, as an RTLFMCHN file is to rtlfm_snapshot_read.
 *
 * Steps and bins are in the file for whoever restarts a service from it; rtlfm_gpu_channels_load neither compares nor
 * applies them.
 */
#ifndef RTLFM_CHANSNAP_H
#define RTLFM_CHANSNAP_H

#include <stddef.h>
#include <stdint.h>

#include "rtlfm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTLFM_CHANSNAP_MAGIC "RTLFMCHN"
#define RTLFM_CHANSNAP_VERSION 1u
#define RTLFM_CHANSNAP_HIST 4096u     /* complex samples of history per source (2 bytes each) */
#define RTLFM_CHANSNAP_DC_PIECES 16u  /* bias words per source */
#define RTLFM_CHANSNAP_DC_NONE 0x007f007fu /* a bias word where nothing was subtracted (channel::kDcNone) */
#define RTLFM_CHANSNAP_FLAG_SOURCE_DC 1u
#define RTLFM_CHANSNAP_FLAG_HISTORY 2u

/* The header's fields behind the two struct sizes (48 bytes, no padding). */
typedef struct rtlfm_chansnap_hdr {
	uint64_t pos;
	uint32_t nstreams, per_source, flags;
	uint32_t fir_ntaps, fir_shift;
	uint32_t bank_K, bank_ntaps, bank_shift;
	uint32_t hist_samples, dc_pieces;  /* written as the two constants whatever the caller put here */
} rtlfm_chansnap_hdr;

/* The sections, for the writer.  A section the header makes empty may be NULL; dc == NULL with both flags set writes
 * "none subtracted" (RTLFM_CHANSNAP_DC_NONE) for every piece. */
typedef struct rtlfm_chansnap_parts {
	const rtlfm_cfg *cfg;
	const uint32_t *steps;             /* [nstreams] */
	const int16_t *fir_taps;           /* [fir_ntaps] */
	const int16_t *bank_taps;          /* [bank_ntaps] */
	const int32_t *bins;               /* [nstreams], only with a bank */
	const rtlfm_stream_state *states;  /* [nstreams] */
	const uint8_t *hist;               /* [sources][8192], only with RTLFM_CHANSNAP_FLAG_HISTORY */
	const uint32_t *dc;                /* [sources][16], only with both flags */
} rtlfm_chansnap_parts;

/* The same for the reader: where each section goes and how many ELEMENTS fit there.  A NULL pointer skips its section. */
typedef struct rtlfm_chansnap_bufs {
	rtlfm_cfg *cfg;
	uint32_t *steps;            size_t cap_steps;
	int16_t *fir_taps;          size_t cap_fir_taps;
	int16_t *bank_taps;         size_t cap_bank_taps;
	int32_t *bins;              size_t cap_bins;
	rtlfm_stream_state *states; size_t cap_states;
	uint8_t *hist;              size_t cap_hist;  /* bytes */
	uint32_t *dc;               size_t cap_dc;    /* words */
} rtlfm_chansnap_bufs;

/*
 * Writes the file so that `path` either keeps what it held or holds the whole new file: the bytes go to a temporary
 * file in the same directory (path + ".tmpXXXXXX"), which is fsync()ed and then rename()d over path.  The header is
 * checked as a reader would check it (-EINVAL where a reader would refuse the file, for a NULL argument and for a
 * missing section), else the -errno of the first call that failed; after a failure there is neither a partial file at
 * `path` nor a temporary left behind.
 */
int rtlfm_chansnap_write(const char *path, const rtlfm_chansnap_hdr *hdr, const rtlfm_chansnap_parts *parts);

/* The header fields and the configuration of a file that passes every check (the whole file is read and its checksum
 * verified, so a file this call accepts is one rtlfm_chansnap_read accepts).  Either output may be NULL. */
int rtlfm_chansnap_info(const char *path, rtlfm_chansnap_hdr *hdr_out, rtlfm_cfg *cfg_out);

/*
 * The whole file: the header to *hdr_out (may be NULL), every section to where `bufs` points.  -ENOBUFS when a
 * section holds more than its cap (ask rtlfm_chansnap_info first: every length follows from the header).  On ANY
 * failure nothing at all is written to any output.
 */
int rtlfm_chansnap_read(const char *path, rtlfm_chansnap_hdr *hdr_out, const rtlfm_chansnap_bufs *bufs);

#ifdef __cplusplus
}
#endif
#endif /* RTLFM_CHANSNAP_H */
