/*
 * rtlfm_snapshot.h — the carried state of many streams in a file (host only, no GPU needed).
 *
 * SURVEY.md §5 ("Checkpoint / resume" row) promised that a restart costs nothing because everything a stream carries
 * from one buffer to the next - the persisting fields of struct demod_state, src/rtl_fm.c:172-208, plus
 * deemph_filter's function-static avg - is one explicit, copyable record (rtlfm_stream_state).  This is the file
 * that holds those records for every stream of a handle, with the hop mute each stream is still owed
 * (rtlfm_gpu_mute) and the configuration they were carried under.  rtlfm_gpu_save / rtlfm_gpu_load
 * (include/rtlfm_hip.h) are get_all / set_all around these three entry points.
 *
 * Layout, little-endian, no padding between the parts:
 *
 *   offset  bytes            what
 *   0       8                magic "RTLFMSNP"
 *   8       4                format version (RTLFM_SNAPSHOT_VERSION = 1)
 *   12      4                sizeof(rtlfm_cfg)           of the writer
 *   16      4                sizeof(rtlfm_stream_state)  of the writer
 *   20      4                n = stream count (>= 1)
 *   24      sizeof cfg       the rtlfm_cfg, as it lies in memory
 *   ...     4 n              uint32 mute[n]: input bytes each stream's next buffers still read as 127
 *   ...     n sizeof state   the records, stream 0 first
 *   ...     8                64-bit FNV-1a over every byte in front of it
 *
 * A reader checks ALL of it before it writes anything to its outputs: the magic, the version, both sizes against
 * its own structs, n >= 1, the file's length against what the header implies (a truncated file and one with bytes
 * behind the checksum both fail here), and the checksum.  Every such failure is -EILSEQ; a file that cannot be
 * opened or read is the -errno of the call that failed.
 */
#ifndef RTLFM_SNAPSHOT_H
#define RTLFM_SNAPSHOT_H

#include <stdint.h>

#include "rtlfm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTLFM_SNAPSHOT_MAGIC "RTLFMSNP"
#define RTLFM_SNAPSHOT_VERSION 1u

/*
 * Writes the file so that `path` either keeps what it held or holds the whole new snapshot: the bytes go to a
 * temporary file in the same directory (path + ".tmpXXXXXX"), which is fsync()ed and then rename()d over path.
 * `mutes` may be NULL (all zero).  -EINVAL for a NULL argument or nstreams < 1, else the -errno of the first call
 * that failed; after a failure there is neither a partial file at `path` nor a temporary left behind.
 */
int rtlfm_snapshot_write(const char *path, const rtlfm_cfg *cfg, int nstreams, const rtlfm_stream_state *states,
                         const uint32_t *mutes);

/* The configuration and the stream count of a file that passes every check (the whole file is read and its checksum
 * verified, so a file this call accepts is one rtlfm_snapshot_read accepts).  Either output may be NULL. */
int rtlfm_snapshot_info(const char *path, rtlfm_cfg *cfg_out, int *nstreams_out);

/*
 * The whole file: *n records to states[0 .. *n), their mutes to mutes[0 .. *n), the configuration to *cfg_out
 * (cfg_out and mutes may be NULL).  -ENOBUFS when the file holds more than `cap` records (ask rtlfm_snapshot_info
 * for the count first).  On ANY failure nothing at all is written to the outputs, *n included.
 */
int rtlfm_snapshot_read(const char *path, rtlfm_cfg *cfg_out, rtlfm_stream_state *states, uint32_t *mutes, int cap,
                        int *n);

#ifdef __cplusplus
}
#endif
#endif /* RTLFM_SNAPSHOT_H */
