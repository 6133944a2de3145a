// filter_route.h — the rule and the partition plan of vss_search_batch_filtered_groups_auto: pure arithmetic, no HIP, so that
// it can be compiled and run on a CPU (host/filter_route_check.cpp, under the sanitizers).  vss_engine.hip only carries it out.
//
// A filtered query has two complete answers: the graph walk that traverses rejected rows like tombstones
// (vss_search_batch_filtered_groups) and the exact scan of the admitted rows (vss_search_exact_batch_filtered_groups).  The
// routed call counts every used group's live admitted rows on the device and sends each GROUP to the cheaper one.
//
// Model, in distance evaluations per query:  exact ~ len;  graph ~ C * (limit / 64) * L / len  — the unfiltered walk grows with
// the limit and is multiplied by the inverse of the admitted share.  The queries of a group cancel out.
//
//   RULE   group u goes EXACT  iff  len_u^2 * 64 <= C * limit * L
//
//   len_u  live admitted rows of used group u (exact_filter_admits, the admission rule of both calls)
//   L      live linked rows (what vss_search_exact_batch scans)
//   limit  max(k, ef); ef == 0 is the index's ef_search
//   C      FILTER_ROUTE_C unless the caller names one
// len_u == 0 is exact (count 0 without a traversal); so is every group of an empty index.
//
// FILTER_ROUTE_C = 62 500 comes from profiles/r14_exact_filtered_probe_1m128.txt (L = 10^6, limit 64): the exact call was
// faster at len = 250 000 and slower at 500 000, so the crossover len* = sqrt(C * L) lies in [250k, 500k).  The lower end is
// taken because a wrongly exact group cost 3.3x there, a wrongly graph group 27x to 7000x.  (DESIGN.md §8 says what of the
// model has been measured.)
//
//   MINIMUM WALK   (the engine's defaults only: a caller who names C gets the bare rule)
//   A walk is a launch of its own, and a launch has a floor of a millisecond or two however few queries it carries, while a call
//   that scans anyway takes a few more queries of a large group into its passes for much less.  So where some exact-routed
//   group admits a row (lists are built whatever happens) and the graph-routed groups together would cost the scan less than
//   FILTER_ROUTE_MIN_WALK = 2^24 distance evaluations — sum of queries_u * len_u over them —, they are scanned as well.  A call
//   with nothing to scan is left alone: there the scan's own fixed cost is the larger one.  Measured
//   (profiles/r16_filter_route_probe_1m128.txt): 8 queries of a 500 000-row tenant in a chunk of 204 (4 * 10^6) made the
//   routed call 0.93 ms slower than scanning everything, 51 in a chunk of 1024 (2.55 * 10^7) made it no slower.
#pragma once
#include <cstdint>
#include <vector>

#include "exact_filtered_plan.h"

namespace vss {
namespace host {

constexpr uint64_t FILTER_ROUTE_C = 62500;
constexpr uint64_t FILTER_ROUTE_MIN_WALK = 1ull << 24;
constexpr uint8_t FILTER_ROUTE_GRAPH = 0, FILTER_ROUTE_EXACT = 1, FILTER_ROUTE_UNKNOWN = 255;

// the limit both paths' cost is stated in: ef == 0 takes the index's ef_search (64 where that is 0 too, as the search does)
inline constexpr uint64_t filter_route_limit(uint64_t k, uint64_t ef, uint64_t ef_search) {
	const uint64_t e = ef ? ef : ef_search ? ef_search : 64;
	return e > k ? e : k;
}

// THE rule.  len < 2^32, so len^2 * 64 < 2^70 fits 128 bits; the right side may not (C and limit have 64 bits), hence the
// division form: for positive integers x <= a * b  iff  ceil(x / b) <= a.
inline constexpr bool filter_route_exact(uint64_t len, uint64_t L, uint64_t limit, uint64_t C) {
	if (!len || !L)
		return true;
	if (!limit || !C)
		return false;
	const unsigned __int128 lhs = (unsigned __int128)len * len * 64;
	const unsigned __int128 per_row = (lhs + (L - 1)) / L;
	const unsigned __int128 per_limit = (per_row + (limit - 1)) / limit;
	return per_limit <= C;
}

struct FilterRoutePlan {
	std::vector<uint8_t> route;          // per query: FILTER_ROUTE_GRAPH / _EXACT / _UNKNOWN (its group is not in the table)
	std::vector<uint8_t> group_route;    // per used group of the call (ExactFilterPlan::groups of the order over ALL queries)
	std::vector<uint32_t> graph_queries; // the graph-routed queries, in the caller's order: row i of the compact batch
	std::vector<uint32_t> graph_groups;  // ... and the group of each (empty where group_of == nullptr)
	std::vector<uint32_t> unknown_queries;
	// the exact-routed queries as exact_filter_order leaves a call of only them: order / groups / group_query are set, and
	// exact_filter_pack(exact_lengths, ...) completes it — lists exist for exact-routed groups only
	ExactFilterPlan exact;
	std::vector<uint32_t> exact_lengths; // per used group of `exact`
	std::vector<uint32_t> exact_rows;    // per used group of `exact`: its used group in the order over all queries (its row of counts)
	uint64_t n_graph_groups = 0, n_exact_groups = 0;
	bool walk_folded = false; // the rule sent groups to the graph, the minimum walk sent them back
};

// `all` = exact_filter_order over every query of the call; lengths[u] = live admitted rows of its used group u; min_walk: 0, or
// the distance evaluations a walk has to save the scan to be launched beside it (FILTER_ROUTE_MIN_WALK)
inline void filter_route_partition(const ExactFilterPlan &all, const uint32_t *lengths, const uint32_t *group_of,
                                   uint64_t n_queries, uint64_t L, uint64_t limit, uint64_t C, uint64_t min_walk, FilterRoutePlan &r) {
	r = FilterRoutePlan();
	const size_t nu = all.groups.size();
	r.route.assign(n_queries, FILTER_ROUTE_UNKNOWN);
	r.group_route.resize(nu);
	unsigned __int128 walk_saves = 0; // (queries < 2^32 and rows < 2^32 per group, at most 2^32 groups: no overflow)
	bool scans = false, walks = false;
	for (size_t u = 0; u != nu; ++u) {
		const bool exact = filter_route_exact(lengths[u], L, limit, C);
		r.group_route[u] = exact ? FILTER_ROUTE_EXACT : FILTER_ROUTE_GRAPH;
		scans |= exact && lengths[u];
		walks |= !exact;
		if (!exact)
			walk_saves += (unsigned __int128)(all.group_query[u + 1] - all.group_query[u]) * lengths[u];
	}
	r.walk_folded = walks && scans && walk_saves < min_walk;
	for (size_t u = 0; u != nu; ++u) {
		if (r.walk_folded)
			r.group_route[u] = FILTER_ROUTE_EXACT;
		const bool exact = r.group_route[u] == FILTER_ROUTE_EXACT;
		for (uint32_t t = all.group_query[u]; t != all.group_query[u + 1]; ++t)
			r.route[all.order[t]] = r.group_route[u];
		if (!exact) {
			++r.n_graph_groups;
			continue;
		}
		++r.n_exact_groups;
		r.exact.groups.push_back(all.groups[u]);
		r.exact.group_query.push_back((uint32_t)r.exact.order.size());
		r.exact.order.insert(r.exact.order.end(), all.order.begin() + all.group_query[u], all.order.begin() + all.group_query[u + 1]);
		r.exact_lengths.push_back(lengths[u]);
		r.exact_rows.push_back((uint32_t)u);
	}
	r.exact.group_query.push_back((uint32_t)r.exact.order.size());
	r.exact.n_known = r.exact.order.size();
	for (uint64_t q = 0; q != n_queries; ++q) {
		if (r.route[q] == FILTER_ROUTE_GRAPH) {
			r.graph_queries.push_back((uint32_t)q);
			if (group_of)
				r.graph_groups.push_back(group_of[q]);
		} else if (r.route[q] == FILTER_ROUTE_UNKNOWN) {
			r.unknown_queries.push_back((uint32_t)q);
		}
	}
}

} // namespace host
} // namespace vss
