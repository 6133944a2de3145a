// exact_filtered_kernels.h — the kernels of vss_search_exact_batch_filtered_groups: exact top-k under per-query predicates that
// scores only the rows a query's group admits.  The host plan is exact_filtered_plan.h.
//
//   listing    k_filter_list_count -> k_filter_list_scan -> k_filter_list_scatter: for every group IN USE, the ASCENDING list of
//              the live slots its bitmap admits.  A wave owns FL_WAVE_SLOTS consecutive slots and keeps their keys in registers:
//              keys[slot] is read once per launch, however many groups the launch lists.  Ascending, so that position order in a
//              list is slot order and ties come back by slot.  k_label_list_*, k_range_list_* and k_set_list_* make the same lists
//              from the index's label column, for wanted values, label ranges and label sets, and k_box_list_* from up to four
//              label columns, for a range on each, and k_box64_list_* the same for 64-bit ends over columns of either width,
//              and k_set_box_list_* for an IN-list on one column inside such a box (label_filter.h).
//   scoring    k_exact_filtered_scores: k_exact_metric_scores with the rows gathered through a list — the same lane-to-component
//              partition, accumulate4 / group_butterfly / finish_distance order, hence the bits k_exact_rerank computes.  One
//              launch covers every group of a pass through the plan's tile table.
//   selection  k_exact_select_lists: k_exact_select's plain mode with one column count per query; it keeps (distance, SLOT)
//              pairs, looked up through the list, so the running lists go to k_exact_rerank as they are.
//
// Scratch: the lists of one pass hold at most max(B, rows) entries (exact_filtered_plan.h); the block counts take one word per
// (group in use, FL_WAVE_SLOTS slots).
#pragma once
#include "exact_filtered_plan.h"
#include "exact_kernels.h"
#include "label_filter.h"

namespace vss {

#ifdef VSS_ENGINE_TU

constexpr uint32_t FL_KEYS_PER_LANE = 8, FL_WAVE_SLOTS = 64 * FL_KEYS_PER_LANE;

struct FilterListArgs {
	const int64_t *keys;
	uint32_t rows, n_blocks;  // n_blocks = ceil(rows / FL_WAVE_SLOTS): one wave each
	const uint64_t *table;    // the caller's bitmaps, `words` words each
	uint64_t words, n_bits;
	const uint32_t *groups;   // table group of used group u
	uint32_t u_begin, u_end;  // the used groups this launch lists
	uint32_t *counts;         // [u][n_blocks]: admitted rows per block (count), then where the block's rows start (scan)
	uint32_t *totals;         // [u]: the list's length (scan)
	const uint32_t *list_base; // [u]: where the list starts in `lists` (scatter)
	uint32_t *lists;
};

// keys of slots block * FL_WAVE_SLOTS + s * 64 + lane, s = 0 .. FL_KEYS_PER_LANE - 1: ascending in (s, lane)
__device__ __forceinline__ void filter_list_keys(const FilterListArgs &a, uint32_t block, int64_t (&key)[FL_KEYS_PER_LANE]) {
#pragma unroll
	for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s) {
		const uint32_t slot = block * FL_WAVE_SLOTS + s * 64 + lane_id();
		key[s] = slot < a.rows ? a.keys[slot] : host::EXACT_FILTER_FREE_KEY;
	}
}

__global__ __launch_bounds__(256) void k_filter_list_count(FilterListArgs a) {
	const uint32_t block = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (block >= a.n_blocks) // (wave-uniform; no barrier below)
		return;
	int64_t key[FL_KEYS_PER_LANE];
	filter_list_keys(a, block, key);
	for (uint32_t u = a.u_begin; u < a.u_end; ++u) {
		const uint64_t *bitmap = a.table + (size_t)a.groups[u] * a.words;
		uint32_t n = 0;
#pragma unroll
		for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s)
			n += __popcll(__ballot(host::exact_filter_admits(key[s], bitmap, a.n_bits)));
		if (lane_id() == 0)
			a.counts[(size_t)u * a.n_blocks + block] = n;
	}
}

// one workgroup per used group: counts[u][*] becomes its exclusive prefix sum, totals[u] the sum
__global__ __launch_bounds__(256) void k_filter_list_scan(FilterListArgs a) {
	__shared__ uint32_t wave_sum[4];
	uint32_t *row = a.counts + (size_t)(a.u_begin + blockIdx.x) * a.n_blocks;
	const int lane = lane_id(), wave = threadIdx.x >> 6;
	uint32_t running = 0;
	for (uint32_t base = 0; base < a.n_blocks; base += 256) {
		const uint32_t i = base + threadIdx.x;
		const uint32_t v = i < a.n_blocks ? row[i] : 0u;
		uint32_t incl = v;
		for (int o = 1; o < 64; o <<= 1) {
			const uint32_t up = __shfl_up(incl, o);
			if (lane >= o)
				incl += up;
		}
		if (lane == 63)
			wave_sum[wave] = incl;
		__syncthreads();
		uint32_t before = running;
		for (int w = 0; w < wave; ++w)
			before += wave_sum[w];
		if (i < a.n_blocks)
			row[i] = before + incl - v;
		running += wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
		__syncthreads();
	}
	if (threadIdx.x == 0)
		a.totals[a.u_begin + blockIdx.x] = running;
}

__global__ __launch_bounds__(256) void k_filter_list_scatter(FilterListArgs a) {
	const uint32_t block = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (block >= a.n_blocks)
		return;
	int64_t key[FL_KEYS_PER_LANE];
	filter_list_keys(a, block, key);
	const int lane = lane_id();
	for (uint32_t u = a.u_begin; u < a.u_end; ++u) {
		const uint64_t *bitmap = a.table + (size_t)a.groups[u] * a.words;
		// the rows this block found in the count pass (the index is read-locked in between: the same rows now)
		uint32_t at = a.list_base[u] + a.counts[(size_t)u * a.n_blocks + block];
#pragma unroll
		for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s) {
			const bool in = host::exact_filter_admits(key[s], bitmap, a.n_bits);
			const unsigned long long m = __ballot(in);
			if (in)
				a.lists[at + __popcll(m & lanes_below(lane))] = block * FL_WAVE_SLOTS + s * 64 + lane;
			at += __popcll(m);
		}
	}
}

// ---------------------------------------------------------------------------------------------------------
// The same lists from the label column (vss_search_batch_by_label, label_filter.h): used group u is a wanted VALUE, and a slot
// belongs to at most one of them — the one label_lookup finds its row's label to be.  A wave reads keys[slot] and labels[key]
// once per launch and then visits only the groups its FL_WAVE_SLOTS slots carry, one turn of the loop each: no pass over the
// groups, so the cost of a launch does not depend on how many values it lists.  Same counts[u][block] layout as above — the
// scan kernel is k_filter_list_scan — but a wave writes only the cells of the groups it meets: `counts` is ZEROED beforehand.
struct LabelListArgs {
	const int64_t *keys;
	uint32_t rows, n_blocks;
	const uint32_t *labels;   // one cell per row id below labelled_rows
	uint64_t labelled_rows;
	const uint32_t *values;   // [u]: the wanted value of used group u, ascending in u
	uint32_t u_begin, u_end;  // the used groups this launch lists
	uint32_t *counts;
	const uint32_t *list_base;
	uint32_t *lists;
};

// used group of slots block * FL_WAVE_SLOTS + s * 64 + lane among [u_begin, u_end), or NO_LABEL_GROUP
// (host::label_lookup in its pieces: the lane's FL_KEYS_PER_LANE lookups take every step together — their loads are in flight
//  side by side — and the number of steps is the launch's, floor(log2(groups)) + 1)
__device__ __forceinline__ void label_list_groups(const LabelListArgs &a, uint32_t block, uint32_t (&u)[FL_KEYS_PER_LANE]) {
	const uint32_t *values = a.values + a.u_begin;
	const uint32_t n = a.u_end - a.u_begin;
	uint32_t label[FL_KEYS_PER_LANE], lo[FL_KEYS_PER_LANE], hi[FL_KEYS_PER_LANE];
#pragma unroll
	for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s) {
		const uint32_t slot = block * FL_WAVE_SLOTS + s * 64 + lane_id();
		const int64_t key = slot < a.rows ? a.keys[slot] : host::EXACT_FILTER_FREE_KEY;
		const bool has_cell = key != host::EXACT_FILTER_FREE_KEY && key >= 0 && (uint64_t)key < a.labelled_rows;
		label[s] = has_cell ? a.labels[key] : host::NO_LABEL;
		lo[s] = 0, hi[s] = label[s] == host::NO_LABEL ? 0 : n; // (a row without a label looks nothing up)
	}
	for (uint32_t step = host::label_lookup_steps(n); step; --step) {
#pragma unroll
		for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s)
			host::label_lookup_step(values, label[s], lo[s], hi[s]);
	}
#pragma unroll
	for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s) {
		const uint32_t g = host::label_lookup_result(values, n, label[s], lo[s]);
		u[s] = g == host::NO_LABEL_GROUP ? host::NO_LABEL_GROUP : a.u_begin + g;
	}
}

// Calls visit(group) once for every group some lane still carries — the group of the lowest such lane's first such slot
// (wave-uniform) — and takes that group's slots out.  Inside, `u[s] == group` names the group's slots in (s, lane) order.
template <class Visit>
__device__ __forceinline__ void label_list_each_group(uint32_t (&u)[FL_KEYS_PER_LANE], Visit visit) {
	for (;;) {
		uint32_t mine = host::NO_LABEL_GROUP;
#pragma unroll
		for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s)
			mine = mine == host::NO_LABEL_GROUP ? u[s] : mine;
		const unsigned long long holders = __ballot(mine != host::NO_LABEL_GROUP);
		if (!holders)
			return;
		const uint32_t group = (uint32_t)__builtin_amdgcn_readlane((int)mine, uniform(__ffsll((long long)holders) - 1));
		visit(group);
		for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s) // (unrolled without being asked; asked, the pass order makes it a warning)
			u[s] = u[s] == group ? host::NO_LABEL_GROUP : u[s];
	}
}

__global__ __launch_bounds__(256) void k_label_list_count(LabelListArgs a) {
	const uint32_t block = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (block >= a.n_blocks) // (wave-uniform; no barrier below)
		return;
	uint32_t u[FL_KEYS_PER_LANE];
	label_list_groups(a, block, u);
	label_list_each_group(u, [&](uint32_t group) {
		uint32_t n = 0;
#pragma unroll
		for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s)
			n += __popcll(__ballot(u[s] == group));
		if (lane_id() == 0)
			a.counts[(size_t)group * a.n_blocks + block] = n;
	});
}

__global__ __launch_bounds__(256) void k_label_list_scatter(LabelListArgs a) {
	const uint32_t block = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (block >= a.n_blocks)
		return;
	uint32_t u[FL_KEYS_PER_LANE];
	label_list_groups(a, block, u);
	const int lane = lane_id();
	label_list_each_group(u, [&](uint32_t group) {
		// the rows this block found in the count pass (the index is read-locked in between: the same rows now)
		uint32_t at = a.list_base[group] + a.counts[(size_t)group * a.n_blocks + block];
#pragma unroll
		for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s) {
			const bool in = u[s] == group;
			const unsigned long long m = __ballot(in);
			if (in)
				a.lists[at + __popcll(m & lanes_below(lane))] = block * FL_WAVE_SLOTS + s * 64 + lane;
			at += __popcll(m);
		}
	});
}

// ---------------------------------------------------------------------------------------------------------
// The same lists under label RANGES (vss_search_batch_by_label_range, label_filter.h): used group u is a raw pair (lo, hi), cells
// 2u and 2u + 1 of `pairs`.  Ranges overlap, so a slot may belong to many groups and the wave loops over the used groups as
// k_filter_list_count does — but what it tests is in registers: keys[slot] and labels[key] are read ONCE per launch, and a group
// costs a slot two register compares where the bitmap form costs it a load.  Every counts[u][block] cell is written: no zeroing.
struct RangeListArgs {
	const int64_t *keys;
	uint32_t rows, n_blocks;
	const uint32_t *labels;   // one cell per row id below labelled_rows
	uint64_t labelled_rows;
	const uint32_t *pairs;    // [2u], [2u + 1]: lo and hi of used group u
	uint32_t u_begin, u_end;  // the used groups this launch lists
	uint32_t *counts;
	const uint32_t *list_base;
	uint32_t *lists;
};

// cells of slots block * FL_WAVE_SLOTS + s * 64 + lane: a free slot, a key without a cell and a row without a label all become
// NO_LABEL, which host::label_in_range finds in no range
// (Args: RangeListArgs, or the SetListArgs of the lists by label set below)
template <class Args>
__device__ __forceinline__ void range_list_labels(const Args &a, uint32_t block, uint32_t (&label)[FL_KEYS_PER_LANE]) {
#pragma unroll
	for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s) {
		const uint32_t slot = block * FL_WAVE_SLOTS + s * 64 + lane_id();
		const int64_t key = slot < a.rows ? a.keys[slot] : host::EXACT_FILTER_FREE_KEY;
		const bool has_cell = key != host::EXACT_FILTER_FREE_KEY && key >= 0 && (uint64_t)key < a.labelled_rows;
		label[s] = has_cell ? a.labels[key] : host::NO_LABEL;
	}
}

__global__ __launch_bounds__(256) void k_range_list_count(RangeListArgs a) {
	const uint32_t block = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (block >= a.n_blocks) // (wave-uniform; no barrier below)
		return;
	uint32_t label[FL_KEYS_PER_LANE];
	range_list_labels(a, block, label);
	for (uint32_t u = a.u_begin; u < a.u_end; ++u) {
		const uint32_t lo = a.pairs[2 * (size_t)u], hi = a.pairs[2 * (size_t)u + 1];
		uint32_t n = 0;
#pragma unroll
		for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s)
			n += __popcll(__ballot(host::label_in_range(label[s], lo, hi)));
		if (lane_id() == 0)
			a.counts[(size_t)u * a.n_blocks + block] = n;
	}
}

__global__ __launch_bounds__(256) void k_range_list_scatter(RangeListArgs a) {
	const uint32_t block = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (block >= a.n_blocks)
		return;
	uint32_t label[FL_KEYS_PER_LANE];
	range_list_labels(a, block, label);
	const int lane = lane_id();
	for (uint32_t u = a.u_begin; u < a.u_end; ++u) {
		const uint32_t lo = a.pairs[2 * (size_t)u], hi = a.pairs[2 * (size_t)u + 1];
		// the rows this block found in the count pass (the index is read-locked in between: the same rows now)
		uint32_t at = a.list_base[u] + a.counts[(size_t)u * a.n_blocks + block];
#pragma unroll
		for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s) {
			const bool in = host::label_in_range(label[s], lo, hi);
			const unsigned long long m = __ballot(in);
			if (in)
				a.lists[at + __popcll(m & lanes_below(lane))] = block * FL_WAVE_SLOTS + s * 64 + lane;
			at += __popcll(m);
		}
	}
}

// ---------------------------------------------------------------------------------------------------------
// The same lists under label SETS (vss_search_batch_by_label_set, label_filter.h): used group u is a raw row of `width` words,
// cells [u * width, (u + 1) * width) of `words`.  Sets overlap, so the wave loops over the used groups as k_range_list_count does,
// with the eight labels of a lane read ONCE into registers (range_list_labels); a group's words are wave-uniform, and a group
// costs a slot `width` register compares (host::label_in_set).  Every counts[u][block] cell is written: no zeroing.
struct SetListArgs {
	const int64_t *keys;
	uint32_t rows, n_blocks;
	const uint32_t *labels;   // one cell per row id below labelled_rows
	uint64_t labelled_rows;
	const uint32_t *words;    // [u * width + j]: word j of used group u
	uint32_t width;           // 1 .. host::LABEL_SET_MAX
	uint32_t u_begin, u_end;  // the used groups this launch lists
	uint32_t *counts;
	const uint32_t *list_base;
	uint32_t *lists;
};

__global__ __launch_bounds__(256) void k_set_list_count(SetListArgs a) {
	const uint32_t block = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (block >= a.n_blocks) // (wave-uniform; no barrier below)
		return;
	uint32_t label[FL_KEYS_PER_LANE];
	range_list_labels(a, block, label);
	for (uint32_t u = a.u_begin; u < a.u_end; ++u) {
		const uint32_t *set = a.words + (size_t)u * a.width;
		uint32_t n = 0;
#pragma unroll
		for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s)
			n += __popcll(__ballot(host::label_in_set(label[s], set, a.width)));
		if (lane_id() == 0)
			a.counts[(size_t)u * a.n_blocks + block] = n;
	}
}

__global__ __launch_bounds__(256) void k_set_list_scatter(SetListArgs a) {
	const uint32_t block = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (block >= a.n_blocks)
		return;
	uint32_t label[FL_KEYS_PER_LANE];
	range_list_labels(a, block, label);
	const int lane = lane_id();
	for (uint32_t u = a.u_begin; u < a.u_end; ++u) {
		const uint32_t *set = a.words + (size_t)u * a.width;
		// the rows this block found in the count pass (the index is read-locked in between: the same rows now)
		uint32_t at = a.list_base[u] + a.counts[(size_t)u * a.n_blocks + block];
#pragma unroll
		for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s) {
			const bool in = host::label_in_set(label[s], set, a.width);
			const unsigned long long m = __ballot(in);
			if (in)
				a.lists[at + __popcll(m & lanes_below(lane))] = block * FL_WAVE_SLOTS + s * 64 + lane;
			at += __popcll(m);
		}
	}
}

// ---------------------------------------------------------------------------------------------------------
// The same lists under BOXES over M label columns (vss_search_batch_by_label_box, label_filter.h): used group u is a raw row of
// 2M words (lo_0, hi_0, lo_1, hi_1, ...), cells [2M u, 2M (u + 1)) of `boxes`.  A wave reads keys[slot] and the cell of each named
// column ONCE into registers, FL_KEYS_PER_LANE x M words a lane; a slot without a cell in a column holds NO_LABEL there.  Then it
// loops over the used groups: a group's words are wave-uniform, and a group costs a slot 2M register compares
// (host::label_in_box).  Every counts[u][block] cell is written: no zeroing.  M is a template parameter so that the cells stay
// in registers.
struct BoxListArgs {
	const int64_t *keys;
	uint32_t rows, n_blocks;
	const uint32_t *labels[host::LABEL_COLUMNS_MAX]; // the named columns in call order, [0, M) used: one cell per row id below
	uint64_t labelled_rows[host::LABEL_COLUMNS_MAX]; // ... labelled_rows[j]
	const uint32_t *boxes;                           // [2M u + 2j], [2M u + 2j + 1]: lo and hi of used group u in named column j
	uint32_t u_begin, u_end;                         // the used groups this launch lists
	uint32_t *counts;
	const uint32_t *list_base;
	uint32_t *lists;
};

template <uint32_t M>
__device__ __forceinline__ void box_list_labels(const BoxListArgs &a, uint32_t block, uint32_t (&label)[FL_KEYS_PER_LANE][M]) {
#pragma unroll
	for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s) {
		const uint32_t slot = block * FL_WAVE_SLOTS + s * 64 + lane_id();
		const int64_t key = slot < a.rows ? a.keys[slot] : host::EXACT_FILTER_FREE_KEY;
		const bool live = key != host::EXACT_FILTER_FREE_KEY && key >= 0;
#pragma unroll
		for (uint32_t j = 0; j < M; ++j)
			label[s][j] = live && (uint64_t)key < a.labelled_rows[j] ? a.labels[j][key] : host::NO_LABEL;
	}
}

template <uint32_t M>
__global__ __launch_bounds__(256) void k_box_list_count(BoxListArgs a) {
	const uint32_t block = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (block >= a.n_blocks) // (wave-uniform; no barrier below)
		return;
	uint32_t label[FL_KEYS_PER_LANE][M];
	box_list_labels<M>(a, block, label);
	for (uint32_t u = a.u_begin; u < a.u_end; ++u) {
		const uint32_t *box = a.boxes + (size_t)u * 2 * M;
		uint32_t n = 0;
#pragma unroll
		for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s)
			n += __popcll(__ballot(host::label_in_box<M>(label[s], box)));
		if (lane_id() == 0)
			a.counts[(size_t)u * a.n_blocks + block] = n;
	}
}

template <uint32_t M>
__global__ __launch_bounds__(256) void k_box_list_scatter(BoxListArgs a) {
	const uint32_t block = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (block >= a.n_blocks)
		return;
	uint32_t label[FL_KEYS_PER_LANE][M];
	box_list_labels<M>(a, block, label);
	const int lane = lane_id();
	for (uint32_t u = a.u_begin; u < a.u_end; ++u) {
		const uint32_t *box = a.boxes + (size_t)u * 2 * M;
		// the rows this block found in the count pass (the index is read-locked in between: the same rows now)
		uint32_t at = a.list_base[u] + a.counts[(size_t)u * a.n_blocks + block];
#pragma unroll
		for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s) {
			const bool in = host::label_in_box<M>(label[s], box);
			const unsigned long long m = __ballot(in);
			if (in)
				a.lists[at + __popcll(m & lanes_below(lane))] = block * FL_WAVE_SLOTS + s * 64 + lane;
			at += __popcll(m);
		}
	}
}

// ---------------------------------------------------------------------------------------------------------
// The same lists under boxes of 64-BIT ENDS over M label columns of either width (vss_search_batch_by_label_box64,
// label_filter.h): used group u is a raw row of 4M 32-bit words, per named column lo then hi, each end as (high word, low word),
// cells [4M u, 4M (u + 1)) of `boxes`.  A wave reads keys[slot] and the cell of each named column ONCE into registers, WIDENED to
// 64 bits (a column's width is launch-uniform: bit j of `wide`), FL_KEYS_PER_LANE x M 64-bit values a lane; a slot without a cell
// in a column holds NO_LABEL64 there.  A group's words are wave-uniform, and a group costs a slot 2M 64-bit register compares
// (host::label_in_box64).  Every counts[u][block] cell is written: no zeroing.
struct Box64ListArgs {
	const int64_t *keys;
	uint32_t rows, n_blocks;
	const uint32_t *labels[host::LABEL_COLUMNS_MAX]; // the named columns in call order, [0, M) used: one cell per row id below
	uint64_t labelled_rows[host::LABEL_COLUMNS_MAX]; // ... labelled_rows[j]
	uint32_t wide;                                   // bit j: column j's cells are 64 bits wide (two words a cell)
	const uint32_t *boxes;                           // [4M u + 4j .. + 3]: lo and hi of used group u in named column j
	uint32_t u_begin, u_end;                         // the used groups this launch lists
	uint32_t *counts;
	const uint32_t *list_base;
	uint32_t *lists;
};

template <uint32_t M>
__device__ __forceinline__ void box64_list_labels(const Box64ListArgs &a, uint32_t block, uint64_t (&label)[FL_KEYS_PER_LANE][M]) {
#pragma unroll
	for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s) {
		const uint32_t slot = block * FL_WAVE_SLOTS + s * 64 + lane_id();
		const int64_t key = slot < a.rows ? a.keys[slot] : host::EXACT_FILTER_FREE_KEY;
		const bool live = key != host::EXACT_FILTER_FREE_KEY && key >= 0;
#pragma unroll
		for (uint32_t j = 0; j < M; ++j) {
			label[s][j] = host::NO_LABEL64;
			if (live && (uint64_t)key < a.labelled_rows[j]) {
				if ((a.wide >> j) & 1)
					label[s][j] = reinterpret_cast<const uint64_t *>(a.labels[j])[key];
				else
					label[s][j] = host::label_widen(a.labels[j][key]);
			}
		}
	}
}

template <uint32_t M>
__global__ __launch_bounds__(256) void k_box64_list_count(Box64ListArgs a) {
	const uint32_t block = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (block >= a.n_blocks) // (wave-uniform; no barrier below)
		return;
	uint64_t label[FL_KEYS_PER_LANE][M];
	box64_list_labels<M>(a, block, label);
	for (uint32_t u = a.u_begin; u < a.u_end; ++u) {
		const uint32_t *box = a.boxes + (size_t)u * 4 * M;
		uint32_t n = 0;
#pragma unroll
		for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s)
			n += __popcll(__ballot(host::label_in_box64<M>(label[s], box)));
		if (lane_id() == 0)
			a.counts[(size_t)u * a.n_blocks + block] = n;
	}
}

template <uint32_t M>
__global__ __launch_bounds__(256) void k_box64_list_scatter(Box64ListArgs a) {
	const uint32_t block = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (block >= a.n_blocks)
		return;
	uint64_t label[FL_KEYS_PER_LANE][M];
	box64_list_labels<M>(a, block, label);
	const int lane = lane_id();
	for (uint32_t u = a.u_begin; u < a.u_end; ++u) {
		const uint32_t *box = a.boxes + (size_t)u * 4 * M;
		// the rows this block found in the count pass (the index is read-locked in between: the same rows now)
		uint32_t at = a.list_base[u] + a.counts[(size_t)u * a.n_blocks + block];
#pragma unroll
		for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s) {
			const bool in = host::label_in_box64<M>(label[s], box);
			const unsigned long long m = __ballot(in);
			if (in)
				a.lists[at + __popcll(m & lanes_below(lane))] = block * FL_WAVE_SLOTS + s * 64 + lane;
			at += __popcll(m);
		}
	}
}

// ---------------------------------------------------------------------------------------------------------
// The same lists under an IN-LIST on one column inside a box of M ranges (vss_search_batch_by_label_set_box, label_filter.h): used
// group u is a travelling row of 2 width + 4M 32-bit words, cells [(2 width + 4M) u, ...) of `rows`.  A wave reads keys[slot] and
// the WIDENED cell of the set column and of each range column ONCE into registers, FL_KEYS_PER_LANE x (1 + M) 64-bit values a
// lane (a column's width is launch-uniform: bit 0 of `wide` the set column, bit 1 + j range column j); a slot without a cell in a
// column holds NO_LABEL64 there.  A group's words are wave-uniform; a group costs a slot `width` 64-bit register compares, one test
// against NO_LABEL64 and 2M range compares (host::label_in_set_box).  The set width is a run-time argument.  Every
// counts[u][block] cell is written: no zeroing.
struct SetBoxListArgs {
	const int64_t *keys;
	uint32_t rows_n, n_blocks;
	const uint32_t *labels[host::LABEL_COLUMNS_MAX]; // the set column, then the M range columns in call order
	uint64_t labelled_rows[host::LABEL_COLUMNS_MAX];
	uint32_t wide;                                   // bit j: column j of `labels` has 64-bit cells
	const uint32_t *rows;                            // the used groups' travelling rows
	uint32_t width;                                  // 1 .. host::LABEL_SET_MAX
	uint32_t u_begin, u_end;                         // the used groups this launch lists
	uint32_t *counts;
	const uint32_t *list_base;
	uint32_t *lists;
};

template <uint32_t M>
__device__ __forceinline__ void set_box_list_labels(const SetBoxListArgs &a, uint32_t block, uint64_t (&label)[FL_KEYS_PER_LANE][M + 1]) {
#pragma unroll
	for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s) {
		const uint32_t slot = block * FL_WAVE_SLOTS + s * 64 + lane_id();
		const int64_t key = slot < a.rows_n ? a.keys[slot] : host::EXACT_FILTER_FREE_KEY;
		const bool live = key != host::EXACT_FILTER_FREE_KEY && key >= 0;
#pragma unroll
		for (uint32_t j = 0; j < M + 1; ++j) {
			label[s][j] = host::NO_LABEL64;
			if (live && (uint64_t)key < a.labelled_rows[j]) {
				if ((a.wide >> j) & 1)
					label[s][j] = reinterpret_cast<const uint64_t *>(a.labels[j])[key];
				else
					label[s][j] = host::label_widen(a.labels[j][key]);
			}
		}
	}
}

template <uint32_t M>
__global__ __launch_bounds__(256) void k_set_box_list_count(SetBoxListArgs a) {
	const uint32_t block = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (block >= a.n_blocks) // (wave-uniform; no barrier below)
		return;
	uint64_t label[FL_KEYS_PER_LANE][M + 1];
	set_box_list_labels<M>(a, block, label);
	const uint32_t per = host::label_set_box_row_words(a.width, M);
	for (uint32_t u = a.u_begin; u < a.u_end; ++u) {
		const uint32_t *row = a.rows + (size_t)u * per;
		uint32_t n = 0;
#pragma unroll
		for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s)
			n += __popcll(__ballot(host::label_in_set_box<M>(label[s], row, a.width)));
		if (lane_id() == 0)
			a.counts[(size_t)u * a.n_blocks + block] = n;
	}
}

template <uint32_t M>
__global__ __launch_bounds__(256) void k_set_box_list_scatter(SetBoxListArgs a) {
	const uint32_t block = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (block >= a.n_blocks)
		return;
	uint64_t label[FL_KEYS_PER_LANE][M + 1];
	set_box_list_labels<M>(a, block, label);
	const uint32_t per = host::label_set_box_row_words(a.width, M);
	const int lane = lane_id();
	for (uint32_t u = a.u_begin; u < a.u_end; ++u) {
		const uint32_t *row = a.rows + (size_t)u * per;
		// the rows this block found in the count pass (the index is read-locked in between: the same rows now)
		uint32_t at = a.list_base[u] + a.counts[(size_t)u * a.n_blocks + block];
#pragma unroll
		for (uint32_t s = 0; s < FL_KEYS_PER_LANE; ++s) {
			const bool in = host::label_in_set_box<M>(label[s], row, a.width);
			const unsigned long long m = __ballot(in);
			if (in)
				a.lists[at + __popcll(m & lanes_below(lane))] = block * FL_WAVE_SLOTS + s * 64 + lane;
			at += __popcll(m);
		}
	}
}

// ---------------------------------------------------------------------------------------------------------
// Score rows t of `scores` are positions of the plan's group order (query order[t]); column c of a launch is list position
// pos_begin + c of that query's list.  blockIdx.y = tile of the pass, blockIdx.x strides over the list positions.
struct FilteredScoreArgs {
	RowSpace sp;
	const float *queries; // n_queries x q_stride
	uint32_t q_stride, dim;
	const uint32_t *order;
	const host::ExactFilterTile *tiles; // of this pass
	const uint32_t *lists;
	uint32_t pos_begin, chunk_stride;
	float *scores;
};

template <int MT>
__global__ __launch_bounds__(256) void k_exact_filtered_scores(FilteredScoreArgs a) {
	extern __shared__ __attribute__((aligned(16))) unsigned char fs_smem[];
	float4 *qs = reinterpret_cast<float4 *>(fs_smem); // [tile.n_queries][V], zero padded
	const host::ExactFilterTile tile = a.tiles[blockIdx.y];
	if (tile.list_length <= a.pos_begin) // (workgroup-uniform) this list ended in an earlier chunk
		return;
	const uint32_t pos_end = tile.list_length - a.pos_begin < a.chunk_stride ? tile.list_length : a.pos_begin + a.chunk_stride;
	const uint32_t V = a.sp.V, G = a.sp.G;
	const uint32_t nqt = tile.n_queries; // <= MS_QT
	for (uint32_t i = threadIdx.x; i < nqt * V * 4; i += blockDim.x) {
		const uint32_t t = i / (V * 4), c = i - t * (V * 4);
		reinterpret_cast<float *>(qs)[i] = c < a.dim ? a.queries[(size_t)a.order[tile.first_query + t] * a.q_stride + c] : 0.f;
	}
	__syncthreads();
	const uint32_t lane = threadIdx.x & 63, g = lane & (G - 1), sub = lane >> a.sp.logG, RG = 64u >> a.sp.logG;
	float qa2[MS_QT];
#pragma unroll
	for (int t = 0; t < MS_QT; ++t)
		qa2[t] = (MT == 1 && (uint32_t)t < nqt) ? wave_query_norm(a.sp, qs + (size_t)t * V) : 0.f;
	const uint32_t *list = a.lists + tile.list_offset;
	const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = gridDim.x * (blockDim.x >> 6);
	// (64-bit position: pos_begin + wave * RG may pass 2^32 on the last stride of a list of nearly 2^32 entries)
	for (uint64_t base = (uint64_t)a.pos_begin + (uint64_t)wave * RG; base < pos_end; base += (uint64_t)n_waves * RG) {
		const uint64_t pos = base + sub;
		const bool valid = pos < pos_end;
		const uint32_t row = list[valid ? (uint32_t)pos : pos_end - 1]; // 64 / G entries side by side
		const float4 *rp = a.sp.vectors + (size_t)row * V;
		float ab[MS_QT], b2 = 0.f, unused = 0.f;
#pragma unroll
		for (int t = 0; t < MS_QT; ++t)
			ab[t] = 0.f;
		for (uint32_t c = g; c < V; c += G) {
			const float4 x = rp[c];
#pragma unroll
			for (int t = 0; t < MS_QT; ++t)
				if ((uint32_t)t < nqt) {
					if (MT == 1 && t > 0) // (the row's own sum of squares does not depend on the query: once is enough)
						accumulate4<2>(qs[(size_t)t * V + c], x, ab[t], unused);
					else
						accumulate4<MT>(qs[(size_t)t * V + c], x, ab[t], b2);
				}
		}
		if (MT == 1)
			b2 = group_butterfly(b2, G);
#pragma unroll
		for (int t = 0; t < MS_QT; ++t)
			if ((uint32_t)t < nqt) {
				const float d = finish_distance<MT>(group_butterfly(ab[t], G), qa2[t], b2);
				if (g == 0 && valid)
					a.scores[(size_t)(tile.first_query + t) * a.chunk_stride + ((uint32_t)pos - a.pos_begin)] = d;
			}
	}
}

// ---------------------------------------------------------------------------------------------------------
// k_exact_select's plain mode where every query has its own column count: workgroup b serves position query_begin + b of the
// group order, whose list is lists[offset[t] .. offset[t] + length[t]); this launch's columns are its positions from pos_begin
// on.  Candidates are (distance, slot): lists ascend, so that order is the order by (distance, position).
struct SelectListsArgs {
	const float *scores;
	uint32_t chunk_stride, pos_begin, query_begin, KP;
	const uint32_t *offset, *length, *lists;
	float *best_s;
	uint32_t *best_i;
};

__global__ __launch_bounds__(SEL_THREADS) void k_exact_select_lists(SelectListsArgs a) {
	__shared__ float buf_s[SEL_CAP];
	__shared__ uint32_t buf_i[SEL_CAP];
	__shared__ float old_s[SEL_KP_MAX];
	__shared__ uint32_t old_i[SEL_KP_MAX];
	__shared__ float red_s[SEL_THREADS / 64];
	__shared__ uint32_t red_i[SEL_THREADS / 64];
	__shared__ uint32_t cnt;
	const uint32_t t = a.query_begin + blockIdx.x;
	const int tid = threadIdx.x;
	const uint32_t length = a.length[t];
	if (length <= a.pos_begin) // (workgroup-uniform) nothing of this query's list in this chunk
		return;
	const uint32_t cols = length - a.pos_begin < a.chunk_stride ? length - a.pos_begin : a.chunk_stride;
	const uint32_t *slots = a.lists + a.offset[t] + a.pos_begin;
	const float *row = a.scores + (size_t)t * a.chunk_stride;
	float *bs = a.best_s + (size_t)t * a.KP;
	uint32_t *bi = a.best_i + (size_t)t * a.KP;
	for (uint32_t i = tid; i < a.KP; i += SEL_THREADS)
		old_s[i] = bs[i], old_i[i] = bi[i];
	if (tid == 0)
		cnt = 0;
	__syncthreads();
	const float tau_s = old_s[a.KP - 1];
	const uint32_t tau_i = old_i[a.KP - 1];
	for (uint32_t c = tid; c < cols; c += SEL_THREADS) {
		const float s = row[c];
		if (s < 3.0e38f && !(tau_s < s)) { // (the slot is looked up only for what may enter)
			const uint32_t idx = slots[c];
			if (lex_less(s, idx, tau_s, tau_i)) {
				const uint32_t p = atomicAdd(&cnt, 1u);
				if (p < SEL_CAP)
					buf_s[p] = s, buf_i[p] = idx;
			}
		}
	}
	__syncthreads();
	const uint32_t n = cnt;
	if (n == 0)
		return;
	const bool overflow = n > SEL_CAP;
	// successive minima over (old top-K') U (buffer | whole chunk), strictly above the last one taken
	float last_s = -__builtin_inff();
	uint32_t last_i = 0;
	bool first = true;
	for (uint32_t out = 0; out < a.KP; ++out) {
		float s = __builtin_inff();
		uint32_t i = EMPTY_SLOT;
		auto consider = [&](float cs, uint32_t ci) {
			if ((first || lex_less(last_s, last_i, cs, ci)) && lex_less(cs, ci, s, i))
				s = cs, i = ci;
		};
		for (uint32_t j = tid; j < a.KP; j += SEL_THREADS)
			consider(old_s[j], old_i[j]);
		if (!overflow) {
			for (uint32_t j = tid; j < n; j += SEL_THREADS)
				consider(buf_s[j], buf_i[j]);
		} else {
			for (uint32_t c = tid; c < cols; c += SEL_THREADS)
				consider(row[c], slots[c]);
		}
		block_argmin(s, i, red_s, red_i);
		if (tid == 0)
			bs[out] = s, bi[out] = i;
		if (i == EMPTY_SLOT) { // nothing left: the rest stays (+inf, EMPTY)
			for (uint32_t j = out + 1 + tid; j < a.KP; j += SEL_THREADS)
				bs[j] = __builtin_inff(), bi[j] = EMPTY_SLOT;
			break;
		}
		last_s = s, last_i = i, first = false;
	}
}

#endif // VSS_ENGINE_TU

} // namespace vss
