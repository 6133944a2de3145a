// exact_filtered_harness.cpp — exact top-k under per-query predicates (vss_search_exact_batch_filtered_groups) through both
// host classes.
//     ./exact_filtered_harness
//   1. vss_host::HNSWIndex on device 0: the C entry point against a brute force this harness computes itself over the live rows
//      each query's group admits (row ids everywhere, distances within 1e-5 relative — sharded_lifecycle_harness.cpp's tolerance
//      for its filtered brute force), and ExecuteMultiScanBatchGroupedExact against the entry point
//   2. vss_host::ShardedHNSWIndex with 1, 2 and 3 shards co-resident on device 0: SearchExactBatchFilteredGroups against the one
//      index, CELL BY CELL on row ids, distance bits and counts (the data is tie-free, so the merge's (distance, row id) order
//      is the one index's (distance, slot) order), with and without group numbers
//   3. a query of an unknown group is refused by both classes
// Data as in filter_groups_harness.cpp: 64 seeded Gaussian clusters, dim 32, l2sq, 6001 rows with id = position, every ninth row
// deleted; 257 queries, k = 10; sixteen tenants and one all-ones group whose padding bits are set, over n_bits = 5998.  The
// first failed check or exception ends the process with a non-zero exit code.  Prints "exact filtered ok" last.  Needs a MI355X.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "filter_group_tables.hpp"
#include "harness_common.hpp"

using namespace vss_host;

namespace {

constexpr idx_t DIM = 32, N = 6001, NQ = 257, K = 10, TENANTS = 16, N_BITS = N - 3;

using Results = ResultsOf<K, NQ>;

std::vector<float> vecs(N *DIM), queries(NQ *DIM);
std::vector<row_t> ids(N), dead;
bool Live(uint64_t id) {
	return id % 9 != 4;
}

std::unique_ptr<HNSWIndex> single_p;
std::unique_ptr<ShardedHNSWIndex> sharded_p[3];

// the harness's own answer: every live row the query's group admits, by (distance, row id)
void ExpectBruteForce(const FilterGroupTables &t, const Results &r) {
	idx_t short_lists = 0;
	for (idx_t q = 0; q != NQ; ++q) {
		std::vector<std::pair<float, row_t>> all;
		for (idx_t i = 0; i != N; ++i)
			if (Live(i) && t.Admits(t.group_of[q], (row_t)i)) {
				float d = 0;
				for (idx_t c = 0; c != DIM; ++c) {
					const float x = queries[q * DIM + c] - vecs[i * DIM + c];
					d += x * x;
				}
				all.push_back({d, (row_t)i});
			}
		std::sort(all.begin(), all.end());
		const idx_t want = std::min<idx_t>(K, all.size());
		EXPECT(r.counts[q] == want);
		short_lists += want < K;
		for (idx_t j = 0; j != K; ++j) {
			if (j < want) {
				EXPECT(r.ids[q * K + j] == all[j].second);
				EXPECT(std::fabs(r.dist[q * K + j] - all[j].first) <= 1e-5f * std::max(all[j].first, 1e-6f));
			} else {
				EXPECT(r.ids[q * K + j] == -1 && std::isinf(r.dist[q * K + j]) && r.dist[q * K + j] > 0);
			}
		}
	}
	EXPECT(short_lists == 0); // (tenants of 1/16 of 5998 rows: every query fills its k — which the graph call does not promise)
}

Results SingleIndex(const FilterGroupTables &t) {
	HNSWIndex &index = BuildSingle(single_p, DIM, vecs, ids, dead);
	EXPECT(index.Count() == N - dead.size());

	Results exact;
	EXPECT(vss_search_exact_batch_filtered_groups(index.Handle(), queries.data(), NQ, K, t.allowed.data(), t.n_groups, t.n_bits,
	                                              t.group_of.data(), exact.ids.data(), exact.dist.data(),
	                                              exact.counts.data()) == VSS_OK);
	ExpectBruteForce(t, exact);
	EXPECT(vss_last_exact_fallbacks(index.Handle()) == 0);
	uint64_t work[4];
	EXPECT(vss_last_exact_filtered(index.Handle(), work) == VSS_OK && work[0] > 0 && work[1] >= work[0] && work[2] == 1 && work[3] > 0);
	// the mirror's chunk call: row ids appended query after query
	auto state = index.InitializeMultiScan();
	std::vector<uint32_t> counts;
	const idx_t total = index.ExecuteMultiScanBatchGroupedExact(*state, queries.data(), NQ, K, t.allowed.data(), t.n_groups, t.n_bits,
	                                                            t.group_of.data(), &counts);
	const auto &appended = index.GetMultiScanResult(*state);
	EXPECT(counts == exact.counts && appended.size() == total && total == NQ * K);
	for (idx_t q = 0; q != NQ; ++q)
		for (idx_t j = 0; j != K; ++j)
			EXPECT(appended[q * K + j] == exact.ids[q * K + j]);
	// refused: nothing runs, the message names the first query, the cells stay the caller's
	std::vector<uint32_t> bad = t.group_of;
	bad[200] = (uint32_t)t.n_groups, bad[100] = 4000000000u;
	Results refused;
	EXPECT(vss_search_exact_batch_filtered_groups(index.Handle(), queries.data(), NQ, K, t.allowed.data(), t.n_groups, t.n_bits,
	                                              bad.data(), refused.ids.data(), refused.dist.data(),
	                                              refused.counts.data()) == VSS_ERROR);
	EXPECT(std::strstr(vss_last_error(index.Handle()), "query 100 names group 4000000000"));
	EXPECT(refused.ids[0] == -2 && refused.counts[0] == 77);
	std::printf("one index: %zu queries in %zu groups, %zu rows returned, %llu distances over %llu listed rows, equal to the brute force\n",
	            (size_t)NQ, (size_t)t.n_groups, (size_t)total, (unsigned long long)work[1], (unsigned long long)work[0]);
	return exact;
}

void Sharded(const FilterGroupTables &t, const Results &single, const Results &single_ones, const std::vector<int> &devices,
             std::unique_ptr<ShardedHNSWIndex> &holder) {
	ShardedHNSWIndex &index = BuildSharded(holder, DIM, vecs, ids, dead, devices);

	Results got;
	index.SearchExactBatchFilteredGroups(queries.data(), NQ, K, t.allowed.data(), t.n_groups, t.n_bits, t.group_of.data(),
	                                     got.ids.data(), got.dist.data(), got.counts.data());
	EXPECT(got == single);
	ExpectBruteForce(t, got);
	// no group numbers: every query under bitmap 0 — here the all-ones group's words, handed over as a table of one
	Results ones;
	index.SearchExactBatchFilteredGroups(queries.data(), NQ, K, t.Group(TENANTS), 1, t.n_bits, nullptr, ones.ids.data(),
	                                     ones.dist.data(), ones.counts.data());
	EXPECT(ones == single_ones);
	std::vector<uint32_t> bad = t.group_of;
	bad[NQ - 1] = (uint32_t)t.n_groups;
	bool threw = false;
	try {
		Results refused;
		index.SearchExactBatchFilteredGroups(queries.data(), NQ, K, t.allowed.data(), t.n_groups, t.n_bits, bad.data(),
		                                     refused.ids.data(), refused.dist.data(), refused.counts.data());
	} catch (const std::exception &e) {
		threw = std::strstr(e.what(), "query 256 names group 17") != nullptr;
	}
	EXPECT(threw);
	std::printf("%zu shard(s), exchange %s: equal to the one index, cell by cell\n", devices.size(), index.ExchangeKind());
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
	FilterGroupTables t = TenantTables(TENANTS, N_BITS, NQ, [](uint64_t) { return true; });
	for (idx_t q = 0; q != NQ; ++q) // tenants only (the all-ones group is the second leg)
		t.group_of[q] = (uint32_t)(q % TENANTS);
	try {
		const Results single = SingleIndex(t);
		Results single_ones;
		EXPECT(vss_search_exact_batch_filtered_groups(single_p->Handle(), queries.data(), NQ, K, t.Group(TENANTS), 1, t.n_bits, nullptr,
		                                              single_ones.ids.data(), single_ones.dist.data(),
		                                              single_ones.counts.data()) == VSS_OK);
		Sharded(t, single, single_ones, {0}, sharded_p[0]);
		Sharded(t, single, single_ones, {0, 0}, sharded_p[1]);
		Sharded(t, single, single_ones, {0, 0, 0}, sharded_p[2]);
	} catch (const std::exception &e) {
		std::fprintf(stderr, "EXCEPTION: %s\n", e.what());
		std::fflush(nullptr);
		std::_Exit(1);
	}
	std::printf("exact filtered ok\n");
	std::fflush(nullptr);
	std::_Exit(0);
}
