// state_kernel.h — k_state_move: the carried state of many streams regrouped on the device in one launch.
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

}  // namespace statemove
}  // namespace rtlfm
