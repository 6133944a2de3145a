// filter_route_kernels.h — the kernels of vss_search_batch_filtered_groups_auto ("Routing"): the plumbing between
// one request and the two existing answers.  The rule and the partition are filter_route.h; the walk is the ordinary search
// launch over a COMPACT batch of the graph-routed queries, the scan the kernels of exact_filtered_kernels.h over the
// exact-routed ones — neither sees a query of the other.
//
//   k_route_gather     compact row i <- query map[i] (and its group number)          before the walk
//   k_route_gather_words  further per-query words of the compact batch: a second column (the `hi` of a call by label range), or
//                         with a words-per-query stride the whole row of a matrix (a call by label set)
//   k_route_scatter    the caller's cells of query map[i] <- compact answer i        after the walk
//   k_route_blank      count 0, cells -1 / +inf for the queries of unknown groups
//   k_route_take_rows  block counts of the exact-routed used groups, made consecutive for k_filter_list_scatter
// One wave per query in the first three; none of them is ever a measurable share of a call.
#pragma once
#include "filter_route.h"
#include "exact_filtered_kernels.h"

namespace vss {

#ifdef VSS_ENGINE_TU

struct RouteGatherArgs {
	const float *queries;     // the caller's rows of q_stride floats
	const uint32_t *group_of; // ... and groups, or nullptr (nothing copied)
	const uint32_t *map;      // n query numbers, ascending
	uint32_t n, q_stride;
	uint32_t vec4;            // q_stride % 4 == 0 and both row pointers 16-byte aligned: rows move as float4
	float *out_queries;
	uint32_t *out_group_of;
};

__global__ __launch_bounds__(256) void k_route_gather(RouteGatherArgs a) {
	const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = lane_id();
	if (i >= a.n) // (wave-uniform; no barrier below)
		return;
	const uint32_t q = a.map[i];
	const float *src = a.queries + (size_t)q * a.q_stride;
	float *dst = a.out_queries + (size_t)i * a.q_stride;
	if (a.vec4) {
		const float4 *s4 = reinterpret_cast<const float4 *>(src);
		float4 *d4 = reinterpret_cast<float4 *>(dst);
		for (uint32_t c = lane; c < a.q_stride / 4; c += 64)
			d4[c] = s4[c];
	} else {
		for (uint32_t c = lane; c < a.q_stride; c += 64)
			dst[c] = src[c];
	}
	if (a.group_of && lane == 0)
		a.out_group_of[i] = a.group_of[q];
}

// one more per-query column for the compact batch (a call by label range carries two words per query: k_route_gather takes
// `lo` along as its group column, this takes `hi`): out[i] = words[map[i]]
__global__ __launch_bounds__(256) void k_route_gather_words(const uint32_t *words, const uint32_t *map, uint32_t n, uint32_t *out) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i < n)
		out[i] = words[map[i]];
}

// ... and with a words-per-query stride, for a call that carries a row-major MATRIX (a call by label set: every routed query's
// whole row of `per` words, in one launch): out[i][j] = words[map[i]][j]
__global__ __launch_bounds__(256) void k_route_gather_words(const uint32_t *words, const uint32_t *map, uint32_t n, uint32_t per,
                                                            uint32_t *out) {
	const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (t < (uint64_t)n * per) {
		const uint64_t i = t / per, j = t - i * per;
		out[t] = words[(uint64_t)map[i] * per + j];
	}
}

struct RouteScatterArgs {
	const uint32_t *map; // n query numbers
	uint32_t n, k;
	const int64_t *keys; // the compact batch's answers: n x k, n x k, n
	const float *dist;
	const uint32_t *count;
	int64_t *out_keys;   // the caller's cells
	float *out_dist;     // may be nullptr
	uint32_t *out_count;
};

__global__ __launch_bounds__(256) void k_route_scatter(RouteScatterArgs a) {
	const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = lane_id();
	if (i >= a.n)
		return;
	const size_t from = (size_t)i * a.k, to = (size_t)a.map[i] * a.k;
	for (uint32_t c = lane; c < a.k; c += 64) { // (padding cells come as the walk left them)
		a.out_keys[to + c] = a.keys[from + c];
		if (a.out_dist)
			a.out_dist[to + c] = a.dist[from + c];
	}
	if (lane == 0)
		a.out_count[a.map[i]] = a.count[i];
}

// the answer of a query whose group the table does not hold: what the exact call gives it
__global__ __launch_bounds__(256) void k_route_blank(const uint32_t *map, uint32_t n, uint32_t k, int64_t *out_keys, float *out_dist,
                                                     uint32_t *out_count) {
	const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = lane_id();
	if (i >= n)
		return;
	const size_t to = (size_t)map[i] * k;
	for (uint32_t c = lane; c < k; c += 64) {
		out_keys[to + c] = -1;
		if (out_dist)
			out_dist[to + c] = __builtin_inff();
	}
	if (lane == 0)
		out_count[map[i]] = 0;
}

// to[u'][*] = from[row_of[u']][*] for u' < n_rows, rows of n_blocks words: blockIdx.y strides over the rows, blockIdx.x over a
// row.  `to` and `from` do not overlap.
__global__ __launch_bounds__(256) void k_route_take_rows(const uint32_t *from, const uint32_t *row_of, uint32_t n_rows, uint32_t n_blocks,
                                                         uint32_t *to) {
	for (uint32_t u = blockIdx.y; u < n_rows; u += gridDim.y) {
		const uint32_t *src = from + (size_t)row_of[u] * n_blocks;
		uint32_t *dst = to + (size_t)u * n_blocks;
		for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n_blocks; i += gridDim.x * 256)
			dst[i] = src[i];
	}
}

#endif // VSS_ENGINE_TU

} // namespace vss
