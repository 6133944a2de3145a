// exact_filtered_plan.h — the host plan of vss_search_exact_batch_filtered_groups: pure arithmetic, no HIP, so that it can be
// compiled and run on a CPU (host/exact_filtered_check.cpp, under the sanitizers).  vss_engine.hip only carries it out.
//
// The call answers every query from the list of the live rows its group's bitmap admits.  The plan
//   1. orders the queries by group (stable) and names the groups in use            exact_filter_order
//   2. once the device has counted every such group's list, packs the groups, in group order, into passes whose lists
//      hold at most `budget` entries together, and cuts each group's queries into tiles of at most `qt` queries for
//      the scoring kernel                                                          exact_filter_pack
// Scratch bound: the lists of one pass hold at most max(B, rows) entries of 4 bytes (the engine passes that as `budget`;
// B = EXACT_FILTER_LIST_ENTRIES, or VSS_EXACT_FILTER_LIST_ENTRIES), because one group's list never exceeds `rows` and a
// group joins a pass only while the sum stays within the budget.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "filter_groups.h"

namespace vss {
namespace host {

constexpr uint64_t EXACT_FILTER_LIST_ENTRIES = 1ull << 23; // B: 32 MiB of list scratch
constexpr uint64_t EXACT_FILTER_LIST_ENTRIES_MIN = 1, EXACT_FILTER_LIST_ENTRIES_MAX = 1ull << 32;
constexpr int64_t EXACT_FILTER_FREE_KEY = 0x7FFFFFFFFFFFFFFFll; // the key of a removed row (hnsw_kernels.h: GraphView::admitted)

// THE admission rule (that of hnsw_kernels.h GraphView::admitted): the row is live, 0 <= rowid < n_bits, and bit `rowid` of
// the group's bitmap is set.  A set padding bit behind n_bits admits nothing.  constexpr: the listing kernels and the CPU
// check run this very code.
inline constexpr bool exact_filter_admits(int64_t key, const uint64_t *bitmap, uint64_t n_bits) {
	return key != EXACT_FILTER_FREE_KEY && key >= 0 && (uint64_t)key < n_bits && ((bitmap[(uint64_t)key >> 6] >> (key & 63)) & 1ull);
}

// what the scoring kernel reads per workgroup row: queries [first_query, first_query + n_queries) of the group order, all of
// table group `group`, against list entries [list_offset, list_offset + list_length) of the pass's list buffer
struct ExactFilterTile {
	uint32_t group, first_query, n_queries, list_offset, list_length;
};

// used groups [group_begin, group_end), their tiles and their queries (positions in `order`); `entries` list entries in all,
// the longest list `longest`
struct ExactFilterPass {
	uint32_t group_begin, group_end, tile_begin, tile_end, query_begin, query_end, longest;
	uint64_t entries;
};

struct ExactFilterPlan {
	// exact_filter_order
	std::vector<uint32_t> order;       // the known queries by (group, query), then the queries of unknown groups
	uint64_t n_known = 0;              // how many of `order` are known
	uint64_t first_unknown = NO_BAD_GROUP; // the first query whose group is not in the table
	std::vector<uint32_t> groups;      // the table groups in use, ascending ("used group" u = position here)
	std::vector<uint32_t> group_query; // groups.size() + 1: used group u owns order[group_query[u] .. group_query[u + 1])
	// exact_filter_pack
	std::vector<uint32_t> list_base;   // per used group: where its list starts in ITS pass's buffer
	std::vector<uint32_t> query_offset, query_length; // per position of `order`: its list (0, 0 for an unknown group)
	std::vector<ExactFilterTile> tiles;
	std::vector<ExactFilterPass> passes;
	uint64_t listed = 0, distances = 0; // sum of the used groups' lists; (query, row) pairs to score
};

// group_of == nullptr: every query takes group 0
inline void exact_filter_order(const uint32_t *group_of, uint64_t n_queries, uint64_t n_groups, ExactFilterPlan &p) {
	p = ExactFilterPlan();
	auto group = [&](uint64_t q) { return group_of ? group_of[q] : 0u; };
	std::vector<uint32_t> known;
	for (uint64_t q = 0; q != n_queries; ++q) {
		if (group(q) < n_groups)
			known.push_back((uint32_t)q);
		else if (p.first_unknown == NO_BAD_GROUP)
			p.first_unknown = q;
	}
	p.n_known = known.size();
	// stable order by group: sort the (group, query) pairs — queries of a chunk are few, the table may name thousands of groups
	std::vector<uint64_t> pairs(known.size());
	for (size_t i = 0; i != known.size(); ++i)
		pairs[i] = ((uint64_t)group(known[i]) << 32) | known[i];
	std::sort(pairs.begin(), pairs.end()); // (the pairs are distinct: this IS the stable order by group)
	p.order.reserve(n_queries);
	for (size_t i = 0; i != pairs.size(); ++i) {
		const uint32_t g = (uint32_t)(pairs[i] >> 32);
		if (p.groups.empty() || p.groups.back() != g) {
			p.groups.push_back(g);
			p.group_query.push_back((uint32_t)i);
		}
		p.order.push_back((uint32_t)pairs[i]);
	}
	p.group_query.push_back((uint32_t)pairs.size());
	for (uint64_t q = 0; q != n_queries; ++q)
		if (group(q) >= n_groups)
			p.order.push_back((uint32_t)q);
}

// lengths[u] = entries of used group u's list (<= budget each); qt = queries per tile (>= 1)
inline void exact_filter_pack(const uint32_t *lengths, uint64_t budget, uint32_t qt, ExactFilterPlan &p) {
	const size_t nu = p.groups.size();
	p.list_base.assign(nu, 0);
	p.query_offset.assign(p.order.size(), 0);
	p.query_length.assign(p.order.size(), 0);
	p.tiles.clear();
	p.passes.clear();
	p.listed = p.distances = 0;
	for (size_t u = 0; u != nu; ++u) {
		const uint32_t len = lengths[u];
		if (p.passes.empty() || p.passes.back().entries + len > budget) {
			ExactFilterPass fresh = {(uint32_t)u, (uint32_t)u, (uint32_t)p.tiles.size(), (uint32_t)p.tiles.size(),
			                         p.group_query[u], p.group_query[u], 0, 0};
			p.passes.push_back(fresh);
		}
		ExactFilterPass &pass = p.passes.back();
		const uint32_t base = (uint32_t)pass.entries;
		p.list_base[u] = base;
		for (uint32_t t = p.group_query[u]; t != p.group_query[u + 1]; ++t)
			p.query_offset[t] = base, p.query_length[t] = len;
		// a group without admitted rows has no tile: its queries keep their empty running lists
		for (uint32_t t = p.group_query[u]; len && t < p.group_query[u + 1]; t += qt) {
			const uint32_t n = p.group_query[u + 1] - t < qt ? p.group_query[u + 1] - t : qt;
			const ExactFilterTile tile = {p.groups[u], t, n, base, len};
			p.tiles.push_back(tile);
		}
		pass.group_end = (uint32_t)u + 1;
		pass.tile_end = (uint32_t)p.tiles.size();
		pass.query_end = p.group_query[u + 1];
		pass.entries += len;
		pass.longest = len > pass.longest ? len : pass.longest;
		p.listed += len;
		p.distances += (uint64_t)len * (p.group_query[u + 1] - p.group_query[u]);
	}
}

} // namespace host
} // namespace vss
