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
#include <random>

#include "../csrc/filter_route.h"
#include "filter_group_tables.hpp"
#include "sharded_index.hpp"

using namespace vss_host;

#define EXPECT(cond)                                                                                                   \
	do {                                                                                                               \
		if (!(cond)) {                                                                                                 \
			std::fprintf(stderr, "CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                               \
			std::fflush(nullptr);                                                                                      \
			std::_Exit(1);                                                                                             \
		}                                                                                                              \
	} while (0)

namespace {

constexpr idx_t DIM = 32, N = 6001, NQ = 257, K = 10, EF = 64, TENANTS = 16, N_BITS = N - 3;
constexpr uint64_t ROUTE_C = 1500;

struct Results {
	std::vector<row_t> ids;
	std::vector<float> dist;
	std::vector<uint32_t> counts;
	Results() : ids(NQ * K, -2), dist(NQ * K, -1.f), counts(NQ, 77) {
	}
	bool operator==(const Results &o) const {
		return ids == o.ids && counts == o.counts && !std::memcmp(dist.data(), o.dist.data(), NQ * K * sizeof(float));
	}
};

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
	const OptionMap options = {{"metric", OptionValue::String("l2sq")}};
	single_p = std::make_unique<HNSWIndex>(DIM, options, N);
	HNSWIndex &index = *single_p;
	index.BulkReserve(N, 8);
	for (idx_t c = 0; c < N; c += STANDARD_VECTOR_SIZE) {
		const idx_t cnt = std::min<idx_t>(STANDARD_VECTOR_SIZE, N - c);
		index.BulkAppendChunk(vecs.data() + c * DIM, ids.data() + c, nullptr, cnt);
	}
	index.BulkFinalize();
	index.Delete(dead.data(), dead.size());
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

// the union of the shards' answers by (distance, row id): the k best per query
Results Merge(const std::vector<Results> &per_shard) {
	Results out;
	for (idx_t q = 0; q != NQ; ++q) {
		std::vector<std::pair<float, row_t>> all;
		for (const Results &r : per_shard)
			for (idx_t j = 0; j != r.counts[q]; ++j)
				all.push_back({r.dist[q * K + j], r.ids[q * K + j]});
		std::sort(all.begin(), all.end());
		out.counts[q] = (uint32_t)std::min<size_t>(K, all.size());
		for (idx_t j = 0; j != K; ++j) {
			out.ids[q * K + j] = j < out.counts[q] ? all[j].second : -1;
			out.dist[q * K + j] = j < out.counts[q] ? all[j].first : INFINITY;
		}
	}
	return out;
}

void Sharded(const FilterGroupTables &t, const std::vector<int> &devices, std::unique_ptr<ShardedHNSWIndex> &holder) {
	const OptionMap options = {{"metric", OptionValue::String("l2sq")}};
	holder = std::make_unique<ShardedHNSWIndex>(DIM, options, N, devices);
	ShardedHNSWIndex &index = *holder;
	index.BulkReserve(8);
	for (idx_t c = 0; c < N; c += STANDARD_VECTOR_SIZE) {
		const idx_t cnt = std::min<idx_t>(STANDARD_VECTOR_SIZE, N - c);
		index.BulkAppendChunk(vecs.data() + c * DIM, ids.data() + c, nullptr, cnt);
	}
	index.BulkFinalize();
	EXPECT(index.Delete(dead.data(), dead.size()) == dead.size());
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
		EXPECT(got == Merge(per_shard));
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
	std::mt19937 rng(20260926);
	std::normal_distribution<float> gauss(0.f, 1.f);
	std::vector<float> centres(64 * DIM);
	for (auto &c : centres)
		c = gauss(rng);
	auto draw = [&](float *dst) {
		const size_t c = rng() % 64;
		for (idx_t d = 0; d != DIM; ++d)
			dst[d] = centres[c * DIM + d] + 0.3f * gauss(rng);
	};
	for (idx_t i = 0; i != N; ++i)
		draw(&vecs[i * DIM]), ids[i] = (row_t)i;
	for (idx_t i = 0; i != NQ; ++i)
		draw(&queries[i * DIM]);
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
