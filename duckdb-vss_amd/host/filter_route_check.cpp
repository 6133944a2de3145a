// filter_route_check — the rule and the partition plan of vss_search_batch_filtered_groups_auto (csrc/filter_route.h) without a
// GPU: pure C++, built stand-alone (tests/test_filter_route_plan.py builds it under the address and undefined-behaviour
// sanitizers).  Prints one "rule len L limit C exact" line per random case for the test to hold against its own restatement of
// the rule, and "filter route check ok" at the end.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../csrc/filter_route.h"

using namespace vss::host;

#define CHECK(cond)                                                                                                    \
	do {                                                                                                               \
		if (!(cond)) {                                                                                                 \
			std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond);                              \
			return 1;                                                                                                  \
		}                                                                                                              \
	} while (0)

// the largest len with len^2 * 64 <= C * limit * L, by bisection on the rule's two sides in 128 bits (small operands only)
static uint64_t boundary(uint64_t L, uint64_t limit, uint64_t C) {
	const unsigned __int128 rhs = (unsigned __int128)C * limit * L;
	uint64_t lo = 0, hi = 0xFFFFFFFFull;
	while (lo < hi) {
		const uint64_t mid = lo + (hi - lo + 1) / 2;
		if ((unsigned __int128)mid * mid * 64 <= rhs)
			lo = mid;
		else
			hi = mid - 1;
	}
	return lo;
}

static_assert(filter_route_exact(250000, 1000000, 64, FILTER_ROUTE_C), "the record's faster-exact point");
static_assert(!filter_route_exact(500000, 1000000, 64, FILTER_ROUTE_C), "the record's faster-graph point");
static_assert(filter_route_limit(10, 0, 64) == 64 && filter_route_limit(100, 0, 64) == 100 && filter_route_limit(10, 256, 64) == 256,
              "ef == 0 is the index's ef_search");

int main() {
	// ---- the rule at its boundary: equality goes exact, one row more goes graph
	{
		// len^2 * 64 == C * limit * L exactly: C = 62500, limit = 64, L = 10^6 -> len = 250 000
		CHECK(filter_route_exact(250000, 1000000, 64, 62500));
		CHECK(!filter_route_exact(250001, 1000000, 64, 62500));
		CHECK(boundary(1000000, 64, 62500) == 250000);
		// a boundary that is no square: the floor goes exact, the next row graph
		const uint64_t L = 5000, limit = 64, C = 62500, b = boundary(L, limit, C);
		CHECK(b > 0 && b < L * 4);
		CHECK(filter_route_exact(b, L, limit, C) && !filter_route_exact(b + 1, L, limit, C));
		// C = 1, small tables: only tiny groups stay exact
		CHECK(filter_route_exact(8, 64, 64, 1) && !filter_route_exact(9, 64, 64, 1));
	}
	// ---- nothing admitted, nothing linked
	CHECK(filter_route_exact(0, 1000, 64, 1));
	CHECK(filter_route_exact(0, 0, 64, FILTER_ROUTE_C));
	CHECK(filter_route_exact(5, 0, 64, 1)); // (an empty index routes everything exact, whatever the count pass said)
	CHECK(!filter_route_exact(1, 1000, 0, FILTER_ROUTE_C)); // a limit of 0 makes the right side 0
	// ---- no overflow at the ends of the ranges
	{
		const uint64_t top = 0xFFFFFFFFull;
		CHECK(filter_route_exact(top, top, 64, UINT64_MAX));
		CHECK(filter_route_exact(top, top, 1, UINT64_MAX));
		CHECK(filter_route_exact(top, 1, UINT64_MAX, UINT64_MAX));
		CHECK(!filter_route_exact(top, top, 1, 1));
		CHECK(!filter_route_exact(top, 1, 1, UINT64_MAX >> 1)); // 2^70 - ... > 2^63 - 1
		CHECK(filter_route_exact(top, top, UINT64_MAX, 1));
	}
	// ---- ef == 0 resolves to the index's value
	CHECK(filter_route_limit(10, 0, 128) == 128);
	CHECK(filter_route_limit(10, 0, 0) == 64);
	CHECK(filter_route_limit(600, 64, 128) == 600);
	CHECK(filter_route_limit(1, 32, 128) == 32);

	// ---- the partition: 4 table groups, L = 1000, limit 64, C = 1  ->  exact iff len^2 <= 1000, i.e. len <= 31
	{
		const uint32_t group_of[] = {2, 0, 3, 2, 9, 0, 1, 2, 7, 3}; // queries 4 and 8 name groups the table does not hold
		const uint64_t nq = 10, n_groups = 4;
		ExactFilterPlan all;
		exact_filter_order(group_of, nq, n_groups, all);
		CHECK(all.groups.size() == 4 && all.first_unknown == 4);
		const uint32_t lengths[] = {31, 32, 900, 0}; // used groups 0..3 = table groups 0..3
		FilterRoutePlan r;
		filter_route_partition(all, lengths, group_of, nq, 1000, 64, 1, 0, r);
		const uint8_t want_group[] = {1, 0, 0, 1};
		for (int u = 0; u != 4; ++u)
			CHECK(r.group_route[u] == want_group[u]);
		const uint8_t want[] = {0, 1, 1, 0, 255, 1, 0, 0, 255, 1};
		for (uint64_t q = 0; q != nq; ++q)
			CHECK(r.route[q] == want[q]);
		// graph-routed queries keep the caller's order, their group numbers travel with them
		const uint32_t want_graph[] = {0, 3, 6, 7}, want_graph_groups[] = {2, 2, 1, 2};
		CHECK(r.graph_queries.size() == 4 && r.graph_groups.size() == 4);
		for (int i = 0; i != 4; ++i)
			CHECK(r.graph_queries[i] == want_graph[i] && r.graph_groups[i] == want_graph_groups[i]);
		CHECK(r.unknown_queries.size() == 2 && r.unknown_queries[0] == 4 && r.unknown_queries[1] == 8);
		CHECK(r.n_graph_groups == 2 && r.n_exact_groups == 2);
		// the exact part: a plan over the exact-routed groups only — groups 0 and 3 — by (group, query)
		CHECK(r.exact.groups.size() == 2 && r.exact.groups[0] == 0 && r.exact.groups[1] == 3);
		const uint32_t want_order[] = {1, 5, 2, 9};
		CHECK(r.exact.order.size() == 4 && r.exact.n_known == 4);
		for (int i = 0; i != 4; ++i)
			CHECK(r.exact.order[i] == want_order[i]);
		CHECK(r.exact.group_query.size() == 3 && r.exact.group_query[0] == 0 && r.exact.group_query[1] == 2 && r.exact.group_query[2] == 4);
		CHECK(r.exact_rows.size() == 2 && r.exact_rows[0] == 0 && r.exact_rows[1] == 3);
		CHECK(r.exact_lengths.size() == 2 && r.exact_lengths[0] == 31 && r.exact_lengths[1] == 0);
		// ... which packs like any other: lists for exact-routed groups only
		exact_filter_pack(r.exact_lengths.data(), 1u << 20, 4, r.exact);
		CHECK(r.exact.listed == 31 && r.exact.distances == 62);
		CHECK(r.exact.tiles.size() == 1 && r.exact.tiles[0].group == 0 && r.exact.tiles[0].n_queries == 2 && r.exact.tiles[0].list_length == 31);
		CHECK(r.exact.passes.size() == 1 && r.exact.passes[0].entries == 31);
		// every query is in exactly one part
		CHECK(r.graph_queries.size() + r.exact.order.size() + r.unknown_queries.size() == nq);

		// the same queries against an empty index: all exact, no walk
		const uint32_t none[] = {0, 0, 0, 0};
		filter_route_partition(all, none, group_of, nq, 0, 64, FILTER_ROUTE_C, FILTER_ROUTE_MIN_WALK, r);
		CHECK(r.graph_queries.empty() && r.exact.order.size() == 8 && r.n_exact_groups == 4 && r.unknown_queries.size() == 2);
		// everything graph: no exact plan at all
		const uint32_t big[] = {900, 900, 900, 900};
		filter_route_partition(all, big, group_of, nq, 1000, 64, 1, 0, r);
		CHECK(r.exact.order.empty() && r.exact.groups.empty() && r.exact.group_query.size() == 1 && r.graph_queries.size() == 8);
		for (size_t i = 1; i < r.graph_queries.size(); ++i)
			CHECK(r.graph_queries[i - 1] < r.graph_queries[i]);
	}
	// ---- the minimum walk: L = 10^6, limit 64, the default C  ->  the rule walks groups of more than 250 000 rows
	{
		static_assert(FILTER_ROUTE_MIN_WALK == 16777216, "2^24 distance evaluations");
		// group 0: 500 000 rows, group 1: 4000 rows, group 2: nothing admitted
		const uint32_t lengths[] = {500000, 4000, 0};
		auto routes = [&](uint32_t n_big, uint32_t n_small, uint32_t n_none, uint64_t min_walk, FilterRoutePlan &r) {
			std::vector<uint32_t> group_of;
			for (uint32_t i = 0; i != n_big + n_small + n_none; ++i)
				group_of.push_back(i < n_big ? 0 : i < n_big + n_small ? 1 : 2);
			ExactFilterPlan all;
			exact_filter_order(group_of.data(), group_of.size(), 3, all);
			std::vector<uint32_t> used;
			for (uint32_t g : all.groups)
				used.push_back(lengths[g]);
			filter_route_partition(all, used.data(), group_of.data(), group_of.size(), 1000000, 64, FILTER_ROUTE_C, min_walk, r);
		};
		FilterRoutePlan r;
		routes(8, 196, 0, FILTER_ROUTE_MIN_WALK, r); // 8 * 500 000 = 4 * 10^6 < 2^24 beside a scan: folded
		CHECK(r.walk_folded && r.graph_queries.empty() && r.exact.order.size() == 204 && r.n_exact_groups == 2 && r.n_graph_groups == 0);
		CHECK(r.route[0] == FILTER_ROUTE_EXACT && r.exact_lengths[0] == 500000);
		routes(8, 196, 0, 0, r); // the bare rule
		CHECK(!r.walk_folded && r.graph_queries.size() == 8 && r.exact.order.size() == 196);
		routes(33, 100, 0, FILTER_ROUTE_MIN_WALK, r); // 33 * 500 000 = 1.65 * 10^7 < 2^24 = 16 777 216: still folded
		CHECK(r.walk_folded && r.graph_queries.empty());
		routes(34, 100, 0, FILTER_ROUTE_MIN_WALK, r); // 34 * 500 000 = 1.7 * 10^7 >= 2^24: walked
		CHECK(!r.walk_folded && r.graph_queries.size() == 34 && r.exact.order.size() == 100);
		routes(8, 0, 0, FILTER_ROUTE_MIN_WALK, r); // nothing to scan: the walk stays
		CHECK(!r.walk_folded && r.graph_queries.size() == 8 && r.exact.order.empty());
		routes(8, 0, 5, FILTER_ROUTE_MIN_WALK, r); // a group that admits nothing builds no list: still nothing to scan
		CHECK(!r.walk_folded && r.graph_queries.size() == 8 && r.exact.order.size() == 5);
		routes(0, 50, 3, FILTER_ROUTE_MIN_WALK, r); // nothing to walk
		CHECK(!r.walk_folded && r.graph_queries.empty() && r.exact.order.size() == 53);
	}
	// ---- group_of == nullptr: one used group, every query follows it; no group numbers to compact
	{
		ExactFilterPlan all;
		exact_filter_order(nullptr, 5, 3, all);
		CHECK(all.groups.size() == 1 && all.groups[0] == 0);
		FilterRoutePlan r;
		const uint32_t big[] = {700}, small[] = {3};
		filter_route_partition(all, big, nullptr, 5, 1000, 64, 1, 0, r);
		CHECK(r.graph_queries.size() == 5 && r.graph_groups.empty() && r.exact.order.empty() && r.n_graph_groups == 1);
		for (uint32_t q = 0; q != 5; ++q)
			CHECK(r.graph_queries[q] == q && r.route[q] == FILTER_ROUTE_GRAPH);
		filter_route_partition(all, small, nullptr, 5, 1000, 64, 1, 0, r);
		CHECK(r.graph_queries.empty() && r.exact.order.size() == 5 && r.n_exact_groups == 1);
		for (uint32_t q = 0; q != 5; ++q)
			CHECK(r.exact.order[q] == q && r.route[q] == FILTER_ROUTE_EXACT);
	}
	// ---- no queries
	{
		ExactFilterPlan all;
		exact_filter_order(nullptr, 0, 1, all);
		FilterRoutePlan r;
		filter_route_partition(all, nullptr, nullptr, 0, 10, 64, 1, FILTER_ROUTE_MIN_WALK, r);
		CHECK(r.route.empty() && r.graph_queries.empty() && r.exact.order.empty() && r.exact.group_query.size() == 1);
	}

	// ---- the table the test restates the rule against
	std::mt19937_64 rng(20240611);
	for (int i = 0; i != 600; ++i) {
		const uint64_t L = i % 7 == 0 ? rng() % 0x100000000ull : 1 + rng() % 20000000;
		const uint64_t limit = i % 5 == 0 ? rng() : 1 + rng() % 4096;
		const uint64_t C = i % 11 == 0 ? UINT64_MAX : i % 3 == 0 ? 1 + rng() % 1000000 : rng() >> (rng() % 64);
		uint64_t len = rng() % 0x100000000ull;
		if (i % 2 == 0 && C < (1ull << 20) && limit < (1ull << 20)) { // half of them at the boundary, where a wrong rounding shows
			const uint64_t b = boundary(L, limit, C);
			len = b + (i % 4 == 0 ? 0 : 1);
			if (len > 0xFFFFFFFFull)
				len = 0xFFFFFFFFull;
		}
		std::printf("rule %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %d\n", len, L, limit, C, (int)filter_route_exact(len, L, limit, C));
	}
	std::printf("filter route check ok\n");
	return 0;
}
