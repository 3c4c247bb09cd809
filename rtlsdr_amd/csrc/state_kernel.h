// state_kernel.h — k_state_move: the carried state of many streams regrouped on the device in one launch
// (and, further down, k_source_move: the same by SOURCE for handles with channels on, history included).
//
//   dst[k] = src[map[k]]   for k < n, as whole rtlfm_stream_state records;  map[k] == -1: the initial record
//
// What a stream carries from one buffer to the next (the persisting fields of struct demod_state, src/rtl_fm.c:172-208,
// and deemph_filter's static avg; SURVEY.md §5, "Checkpoint / resume") is one record per stream, [nstreams] of them per
// state copy of a handle.  A source that leaves a batch, one that joins, a permutation, a fan-out of one stream to
// several: all are this gather.  rtlfm_gpu_state_move (rtlfm_hip.hip) checks the map on the host - every entry in
// [-1, src streams) - before it uploads it, so the kernel indexes without looking.
//
// The work is flattened over (stream, dword of the record): lane i of the grid stores dword i of dst, so the stores
// of a wave are 256 contiguous bytes whatever the map holds; the loads are a gather of runs (82 dwords = 328 bytes per
// record, so a wave's 64 loads come from at most two records).  Duplicates in the map read a record several times,
// never write one twice.  src and dst never alias: between handles they are different allocations, and in place the
// handle passes st[st_cur] as src and its NEXT state copy as dst and advances st_cur behind the launch, exactly what a
// run does - a permutation in place therefore needs no cycle-chasing and no scratch.
// A whole handle of 4096 streams is 1.3 MB: the launch is all there is to the cost.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "../../include/rtlfm_hip.h"

namespace rtlfm {
namespace statemove {

static_assert(sizeof(rtlfm_stream_state) % sizeof(uint32_t) == 0 && alignof(rtlfm_stream_state) >= alignof(uint32_t),
              "k_state_move copies a record as whole dwords");
constexpr uint32_t kRecDwords = sizeof(rtlfm_stream_state) / sizeof(uint32_t);
constexpr uint32_t kHitsDword = offsetof(rtlfm_stream_state, squelch_hits) / sizeof(uint32_t);
static_assert(offsetof(rtlfm_stream_state, squelch_hits) % sizeof(uint32_t) == 0, "squelch_hits is one dword of the record");
constexpr uint32_t kInitSquelchHits = 11;  // demod_init(), src/rtl_fm.c:1615: the one field init_states_host does not zero
constexpr int kThreads = 256;

// dword w of the record demod_init() leaves
__device__ __forceinline__ uint32_t init_dword(uint32_t w) { return w == kHitsDword ? kInitSquelchHits : 0u; }

__global__ void __launch_bounds__(kThreads) k_state_move(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src,
                                                          const int32_t *__restrict__ map, uint32_t n)
{
	const size_t total = (size_t)n * kRecDwords;
	for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
		const uint32_t k = (uint32_t)(i / kRecDwords);
		const uint32_t w = (uint32_t)(i - (size_t)k * kRecDwords);
		const int32_t from = map[k];
		dst[i] = from < 0 ? init_dword(w) : src[(size_t)from * kRecDwords + w];
	}
}

// d_map: n entries on the device, each in [-1, streams behind src) - the caller has checked that
static inline int launch(rtlfm_stream_state *dst, const rtlfm_stream_state *src, const int32_t *d_map, int n, hipStream_t q)
{
	if (n < 1) return 0;
	const size_t total = (size_t)n * kRecDwords;
	size_t blocks = (total + kThreads - 1) / kThreads;
	if (blocks > 4096) blocks = 4096;  // 16 waves per CU: beyond that the lanes stride
	k_state_move<<<(unsigned)blocks, kThreads, 0, q>>>(reinterpret_cast<uint32_t *>(dst), reinterpret_cast<const uint32_t *>(src),
	                                                    d_map, (uint32_t)n);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

// ---- k_source_move: what a handle with channels on carries, regrouped by SOURCE in one launch ----
//
//   source a of dst  <-  source m = map[a] of src   for a < nsrc;   m == -1: a source that joins from silence
//
// Three parts, flattened one behind the other over dst so that every part's stores are contiguous whatever the map holds:
//   records   n = nsrc * per streams of kRecDwords dwords: stream k comes from stream map[k / per] * per + k % per
//             (channel c from channel c), or is init_dword for -1;
//   history   nsrc * kHistPieces 16-byte pieces of raw bytes (channel::kHist complex samples per source), bytes 127 for -1;
//   biases    nsrc * kDcWords words (option source_dc: what was subtracted from the history's pieces), dc_none for -1.
// The last two are skipped where the pointers are null: handles without a filter or a bank carry no history, handles
// without source_dc no biases.  rtlfm_gpu_channels_move (rtlfm_hip.hip) checks the map on the host - every entry in
// [-1, src sources) - and passes dst's NEXT state copy and the history buffers that are NOT current, so src and dst never
// alias, in place either: the host changes over behind the synchronisation that follows the launch, as k_state_move's.
constexpr uint32_t kHistPieces = 4096 * 2 / 16;  // channel::kHist complex samples as uint4 (rtlfm_hip.hip asserts the two agree)
constexpr uint32_t kDcWords = 16;                // channel::kDcHist

struct SourceMove {
	uint32_t *dst_rec;
	const uint32_t *src_rec;
	uint4 *dst_hist;          // null: no history part
	const uint4 *src_hist;
	uint32_t *dst_dc;         // null: no bias part
	const uint32_t *src_dc;
	const int32_t *map;       // [nsrc] on the device
	uint32_t nsrc, per, dc_none;
};

__global__ void __launch_bounds__(kThreads) k_source_move(SourceMove p)
{
	const size_t recs = (size_t)p.nsrc * p.per * kRecDwords;
	const size_t hist = p.dst_hist ? (size_t)p.nsrc * kHistPieces : 0;
	const size_t dcs = p.dst_dc ? (size_t)p.nsrc * kDcWords : 0;
	const size_t total = recs + hist + dcs;
	const size_t per_src = (size_t)p.per * kRecDwords;  // a source's records are one run of dwords in both handles
	for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
		if (i < recs) {
			const uint32_t a = (uint32_t)(i / per_src);
			const size_t w = i - (size_t)a * per_src;
			const int32_t from = p.map[a];
			p.dst_rec[i] = from < 0 ? init_dword((uint32_t)(w % kRecDwords)) : p.src_rec[(size_t)from * per_src + w];
		} else if (i < recs + hist) {
			const size_t j = i - recs;
			const uint32_t a = (uint32_t)(j / kHistPieces);
			const uint32_t u = (uint32_t)(j - (size_t)a * kHistPieces);
			const int32_t from = p.map[a];
			p.dst_hist[j] = from < 0 ? make_uint4(0x7f7f7f7fu, 0x7f7f7f7fu, 0x7f7f7f7fu, 0x7f7f7f7fu) : p.src_hist[(size_t)from * kHistPieces + u];
		} else {
			const size_t j = i - recs - hist;
			const uint32_t a = (uint32_t)(j / kDcWords);
			const uint32_t u = (uint32_t)(j - (size_t)a * kDcWords);
			const int32_t from = p.map[a];
			p.dst_dc[j] = from < 0 ? p.dc_none : p.src_dc[(size_t)from * kDcWords + u];
		}
	}
}

// p.map: nsrc entries on the device, each in [-1, sources behind the src pointers) - the caller has checked that
static inline int launch_source_move(const SourceMove &p, hipStream_t q)
{
	if (p.nsrc < 1 || p.per < 1) return 0;
	const size_t total = (size_t)p.nsrc * ((size_t)p.per * kRecDwords + (p.dst_hist ? kHistPieces : 0) + (p.dst_dc ? kDcWords : 0));
	size_t blocks = (total + kThreads - 1) / kThreads;
	if (blocks > 4096) blocks = 4096;  // (as k_state_move: beyond that the lanes stride)
	k_source_move<<<(unsigned)blocks, kThreads, 0, q>>>(p);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

}  // namespace statemove
}  // namespace rtlfm
