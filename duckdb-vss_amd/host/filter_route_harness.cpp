// filter_route_harness.cpp — per-query predicates with every group routed to the graph walk or the exact scan
// (vss_search_batch_filtered_groups_auto) through both host classes.
//     ./filter_route_harness
//   1. vss_host::HNSWIndex on device 0: the C entry point against the two existing calls, cell by cell according to its route
//      table, its routes against the rule of csrc/filter_route.h applied to counts this harness makes itself, and
//      ExecuteMultiScanBatchGroupedAuto against the entry point
//   2. vss_host::ShardedHNSWIndex with 1, 2 and 3 shards co-resident on device 0: SearchBatchFilteredGroupsAuto against the CPU
//      merge — by (distance, row id) — of per-shard answers assembled from the two existing per-shard calls according to each
//      shard's route table; every shard's routes against the rule applied to ITS rows; with and without group numbers
//   3. a query of an unknown group is refused by both classes
// Data as in exact_filtered_harness.cpp: 64 seeded Gaussian clusters, dim 32, l2sq, 6001 rows with id = position, every ninth row
// deleted; 257 queries, k = 10, ef_search 64; sixteen tenants and one all-ones group whose padding bits are set, over
// n_bits = 5998, query q in group q % 17.  ROUTE_C = 1500 puts the boundary between the two: a shard of L live rows scans
// groups of at most sqrt(1500 * L) rows — the tenants — and walks the all-ones group.  The first failed check or exception
// ends the process with a non-zero exit code.  Prints "filter route ok" last.  Needs a MI355X.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../csrc/filter_route.h"
#include "filter_group_tables.hpp"
#include "harness_common.hpp"

using namespace vss_host;

namespace {

constexpr idx_t DIM = 32, N = 6001, NQ = 257, K = 10, EF = 64, TENANTS = 16, N_BITS = N - 3;
constexpr uint64_t ROUTE_C = 1500;

using Results = ResultsOf<K, NQ>;

std::vector<float> vecs(N *DIM), queries(NQ *DIM);
std::vector<row_t> ids(N), dead;
bool Live(uint64_t id) {
	return id % 9 != 4;
}

std::unique_ptr<HNSWIndex> single_p;
std::unique_ptr<ShardedHNSWIndex> sharded_p[3];

// the route of every query by the rule, from this harness's own counts over the rows `mine` selects
template <class Mine>
std::vector<uint8_t> RuleRoutes(const FilterGroupTables &t, const uint32_t *group_of, uint64_t table_group0, Mine mine) {
	uint64_t L = 0;
	std::vector<uint64_t> len(t.n_groups, 0);
	for (idx_t i = 0; i != N; ++i)
		if (Live(i) && mine((row_t)i)) {
			++L;
			for (uint64_t g = 0; g != t.n_groups; ++g)
				len[g] += t.Admits(g, (row_t)i);
		}
	std::vector<uint8_t> route(NQ);
	for (idx_t q = 0; q != NQ; ++q)
		route[q] = vss::host::filter_route_exact(len[group_of ? group_of[q] : table_group0], L, vss::host::filter_route_limit(K, EF, 64), ROUTE_C);
	return route;
}

// cells of `from` for the queries `route` sends `which` way
void Take(Results &into, const Results &from, const uint8_t *route, uint8_t which) {
	for (idx_t q = 0; q != NQ; ++q)
		if (route[q] == which) {
			std::copy(from.ids.begin() + q * K, from.ids.begin() + (q + 1) * K, into.ids.begin() + q * K);
			std::copy(from.dist.begin() + q * K, from.dist.begin() + (q + 1) * K, into.dist.begin() + q * K);
			into.counts[q] = from.counts[q];
		}
}

// what one index answers when every query goes the way `route` says: assembled from the two existing calls
Results Assembled(vss_index *h, const uint64_t *allowed, uint64_t n_groups, uint64_t n_bits, const uint32_t *group_of,
                  const uint8_t *route) {
	Results graph, exact, both;
	if (group_of)
		EXPECT(vss_search_batch_filtered_groups(h, queries.data(), NQ, K, EF, allowed, n_groups, n_bits, group_of, graph.ids.data(),
		                                        graph.dist.data(), graph.counts.data()) == VSS_OK);
	else
		EXPECT(vss_search_batch_filtered(h, queries.data(), NQ, K, EF, allowed, n_bits, graph.ids.data(), graph.dist.data(),
		                                 graph.counts.data()) == VSS_OK);
	EXPECT(vss_search_exact_batch_filtered_groups(h, queries.data(), NQ, K, allowed, n_groups, n_bits, group_of, exact.ids.data(),
	                                              exact.dist.data(), exact.counts.data()) == VSS_OK);
	Take(both, graph, route, 0);
	Take(both, exact, route, 1);
	return both;
}

Results SingleIndex(const FilterGroupTables &t, std::vector<uint8_t> &route) {
	HNSWIndex &index = BuildSingle(single_p, DIM, vecs, ids, dead);
	EXPECT(index.Count() == N - dead.size());

	Results routed;
	route.assign(NQ, 9);
	EXPECT(vss_search_batch_filtered_groups_auto(index.Handle(), queries.data(), NQ, K, EF, t.allowed.data(), t.n_groups, t.n_bits,
	                                             t.group_of.data(), ROUTE_C, routed.ids.data(), routed.dist.data(),
	                                             routed.counts.data(), route.data()) == VSS_OK);
	uint64_t how[8], work[4];
	EXPECT(vss_last_filter_route(index.Handle(), how) == VSS_OK && vss_last_exact_filtered(index.Handle(), work) == VSS_OK);
	EXPECT(route == RuleRoutes(t, t.group_of.data(), 0, [](row_t) { return true; }));
	const uint64_t n_exact = std::count(route.begin(), route.end(), 1), n_graph = std::count(route.begin(), route.end(), 0);
	EXPECT(n_exact > 0 && n_graph > 0 && n_exact + n_graph == NQ); // both ways in one call
	EXPECT(how[0] == n_graph && how[1] == n_exact && how[2] == 1 && how[3] == TENANTS && how[4] == N - dead.size() &&
	       how[5] == ROUTE_C && how[6] == EF && how[7] == 0);
	EXPECT(work[0] > 0 && work[0] < N - dead.size()); // lists of the tenants only: together they hold every admitted live row once
	EXPECT(routed == Assembled(index.Handle(), t.allowed.data(), t.n_groups, t.n_bits, t.group_of.data(), route.data()));
	// the mirror's chunk call: row ids appended query after query, the routes handed on
	auto state = index.InitializeMultiScan();
	std::vector<uint32_t> counts;
	std::vector<uint8_t> mirror_route;
	const idx_t total = index.ExecuteMultiScanBatchGroupedAuto(*state, queries.data(), NQ, K, t.allowed.data(), t.n_groups, t.n_bits,
	                                                           t.group_of.data(), &counts, &mirror_route, ROUTE_C);
	const auto &appended = index.GetMultiScanResult(*state);
	EXPECT(counts == routed.counts && mirror_route == route && appended.size() == total);
	for (idx_t q = 0, at = 0; q != NQ; at += counts[q++])
		for (idx_t j = 0; j != counts[q]; ++j)
			EXPECT(appended[at + j] == routed.ids[q * K + j]);
	// refused: nothing runs, the message names the first query, the cells stay the caller's
	std::vector<uint32_t> bad = t.group_of;
	bad[200] = (uint32_t)t.n_groups, bad[100] = 4000000000u;
	Results refused;
	EXPECT(vss_search_batch_filtered_groups_auto(index.Handle(), queries.data(), NQ, K, EF, t.allowed.data(), t.n_groups, t.n_bits,
	                                             bad.data(), ROUTE_C, refused.ids.data(), refused.dist.data(), refused.counts.data(),
	                                             nullptr) == VSS_ERROR);
	EXPECT(std::strstr(vss_last_error(index.Handle()), "query 100 names group 4000000000"));
	EXPECT(refused.ids[0] == -2 && refused.counts[0] == 77);
	std::printf("one index: %zu queries, %llu walked and %llu scanned over %llu listed rows, equal to the two calls cell by cell\n",
	            (size_t)NQ, (unsigned long long)n_graph, (unsigned long long)n_exact, (unsigned long long)work[0]);
	return routed;
}

void Sharded(const FilterGroupTables &t, const std::vector<int> &devices, std::unique_ptr<ShardedHNSWIndex> &holder) {
	ShardedHNSWIndex &index = BuildSharded(holder, DIM, vecs, ids, dead, devices);
	const idx_t G = index.ShardCount();

	// with group numbers, then without (every query under bitmap 0 — here the all-ones group's words, a table of one)
	for (int leg = 0; leg != 2; ++leg) {
		const uint64_t *allowed = leg ? t.Group(TENANTS) : t.allowed.data();
		const uint64_t n_groups = leg ? 1 : t.n_groups;
		const uint32_t *group_of = leg ? nullptr : t.group_of.data();
		Results got;
		std::vector<uint8_t> routes;
		index.SearchBatchFilteredGroupsAuto(queries.data(), NQ, K, EF, allowed, n_groups, t.n_bits, group_of, ROUTE_C, got.ids.data(),
		                                    got.dist.data(), got.counts.data(), &routes);
		EXPECT(routes.size() == G * NQ);
		std::vector<Results> per_shard;
		uint64_t n_exact = 0, n_graph = 0;
		for (idx_t g = 0; g != G; ++g) {
			const uint8_t *route = routes.data() + g * NQ;
			const std::vector<uint8_t> want = RuleRoutes(t, group_of, TENANTS, [&](row_t id) { return index.OwnerOf(id) == g; });
			EXPECT(!std::memcmp(route, want.data(), NQ)); // each shard by its own counts and its own L
			n_exact += std::count(route, route + NQ, 1), n_graph += std::count(route, route + NQ, 0);
			per_shard.push_back(Assembled(index.ShardHandle(g), allowed, n_groups, t.n_bits, group_of, route));
		}
		EXPECT(n_exact + n_graph == G * NQ && n_graph > 0 && (leg || n_exact > 0));
		EXPECT(got == Merge(per_shard, NQ));
	}
	std::vector<uint32_t> bad = t.group_of;
	bad[NQ - 1] = (uint32_t)t.n_groups;
	bool threw = false;
	try {
		Results refused;
		index.SearchBatchFilteredGroupsAuto(queries.data(), NQ, K, EF, t.allowed.data(), t.n_groups, t.n_bits, bad.data(), ROUTE_C,
		                                    refused.ids.data(), refused.dist.data(), refused.counts.data());
	} catch (const std::exception &e) {
		threw = std::strstr(e.what(), "query 256 names group 17") != nullptr;
	}
	EXPECT(threw);
	std::printf("%zu shard(s), exchange %s: equal to the merge of the per-shard calls, cell by cell\n", devices.size(), index.ExchangeKind());
}

} // namespace

int main() {
	ClusteredData(20260926, DIM, N, NQ, 64, 0.3f, vecs, queries);
	for (idx_t i = 0; i != N; ++i)
		ids[i] = (row_t)i;
	for (idx_t i = 0; i != N; ++i)
		if (!Live(i))
			dead.push_back((row_t)i);
	// the bitmaps admit deleted rows too (a predicate knows nothing of tombstones): the engine excludes them
	const FilterGroupTables t = TenantTables(TENANTS, N_BITS, NQ, [](uint64_t) { return true; });
	try {
		std::vector<uint8_t> route;
		SingleIndex(t, route);
		Sharded(t, {0}, sharded_p[0]);
		Sharded(t, {0, 0}, sharded_p[1]);
		Sharded(t, {0, 0, 0}, sharded_p[2]);
	} catch (const std::exception &e) {
		std::fprintf(stderr, "EXCEPTION: %s\n", e.what());
		std::fflush(nullptr);
		std::_Exit(1);
	}
	std::printf("filter route ok\n");
	std::fflush(nullptr);
	std::_Exit(0);
}
