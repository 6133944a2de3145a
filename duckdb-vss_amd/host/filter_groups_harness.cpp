// filter_groups_harness.cpp — one launch for a join chunk whose outer rows each carry their own predicate
// (vss_search_batch_filtered_groups), through the host classes, checked CELL BY CELL against what a caller had to do before:
// one filtered call per distinct predicate, over the queries of that predicate.
//     ./filter_groups_harness
//   1. vss_host::HNSWIndex on device 0: ExecuteMultiScanBatchGrouped against vss_search_batch_filtered per group (row ids and
//      counts), and the C entry point itself against the same calls (row ids, distance bits, counts)
//   2. vss_host::ShardedHNSWIndex, one shard, and two shards co-resident on device 0: SearchBatchFilteredGroups against
//      SearchBatchFiltered per group (row ids, distance bits, counts); every returned row is live and admitted by its OWN group
//   3. refusals: a query of an unknown group, a missing table — and the index answers as before afterwards
// Data as in sharded_lifecycle_harness.cpp: 64 seeded Gaussian clusters, dim 32, l2sq, 6001 rows with id = position, every
// ninth row deleted; 257 queries, k = 10, ef 64; four tenants and one all-ones group whose padding bits are set, over
// n_bits = 5998 (the last three rows are beyond every bitmap).  The first failed check or exception ends the process with a
// non-zero exit code, without unwinding.  Prints "filter groups ok" last.  Needs a MI355X.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "filter_group_tables.hpp"
#include "harness_common.hpp"

using namespace vss_host;

namespace {

constexpr idx_t DIM = 32, N = 6001, NQ = 257, K = 10, EF = 64, TENANTS = 4, N_BITS = N - 3;

using Results = ResultsOf<K>;

std::vector<float> vecs(N *DIM), queries(NQ *DIM);
std::vector<row_t> ids(N), dead;
bool Live(uint64_t id) {
	return id % 9 != 4;
}

// the holders live outside main's try block: an exception ends the process before any destructor runs
std::unique_ptr<HNSWIndex> single_p;
std::unique_ptr<ShardedHNSWIndex> sharded_p[2];

void ExpectOwnPredicate(const FilterGroupTables &t, const Results &r) {
	idx_t returned = 0;
	for (idx_t q = 0; q != NQ; ++q) {
		EXPECT(r.counts[q] <= K);
		for (idx_t j = 0; j != K; ++j) {
			const row_t id = r.ids[q * K + j];
			if (j < r.counts[q])
				EXPECT(id >= 0 && Live((uint64_t)id) && t.Admits(t.group_of[q], id));
			else
				EXPECT(id == -1);
		}
		returned += r.counts[q];
	}
	EXPECT(returned > NQ * K / 2); // (tenants of a quarter of the rows at ef 64: most queries fill their k)
}

void SingleIndex(const FilterGroupTables &t) {
	HNSWIndex &index = BuildSingle(single_p, DIM, vecs, ids, dead);
	EXPECT(index.Count() == N - dead.size());

	// the C entry point: ids, distance bits and counts of every query are those of its group's own filtered call
	Results grouped(NQ);
	EXPECT(vss_search_batch_filtered_groups(index.Handle(), queries.data(), NQ, K, EF, t.allowed.data(), t.n_groups, t.n_bits,
	                                        t.group_of.data(), grouped.ids.data(), grouped.dist.data(),
	                                        grouped.counts.data()) == VSS_OK);
	ExpectOwnPredicate(t, grouped);
	// the mirror's chunk call: row ids appended query after query
	auto state = index.InitializeMultiScan(EF);
	std::vector<uint32_t> counts;
	const idx_t total = index.ExecuteMultiScanBatchGrouped(*state, queries.data(), NQ, K, t.allowed.data(), t.n_groups, t.n_bits,
	                                                       t.group_of.data(), &counts);
	const auto &appended = index.GetMultiScanResult(*state);
	EXPECT(counts == grouped.counts && appended.size() == total);
	idx_t at = 0;
	for (idx_t q = 0; q != NQ; ++q)
		for (idx_t j = 0; j != counts[q]; ++j)
			EXPECT(appended[at++] == grouped.ids[q * K + j]);
	EXPECT(at == total);
	for (idx_t g = 0; g != t.n_groups; ++g) {
		const auto mine = t.QueriesOf(g);
		const auto q = GatherRows(queries.data(), DIM, mine);
		Results alone(mine.size());
		EXPECT(vss_search_batch_filtered(index.Handle(), q.data(), mine.size(), K, EF, t.Group(g), t.n_bits, alone.ids.data(),
		                                 alone.dist.data(), alone.counts.data()) == VSS_OK);
		EXPECT(FirstDifference(grouped.ids.data(), alone.ids.data(), K, mine) == -1);
		EXPECT(FirstDifference(grouped.dist.data(), alone.dist.data(), K, mine) == -1);
		EXPECT(FirstDifference(grouped.counts.data(), alone.counts.data(), 1, mine) == -1);
	}

	// refusals: nothing is launched, the message names the first query, and the index answers as before
	std::vector<uint32_t> bad = t.group_of;
	bad[200] = (uint32_t)t.n_groups, bad[100] = 4000000000u;
	Results refused(NQ);
	EXPECT(vss_search_batch_filtered_groups(index.Handle(), queries.data(), NQ, K, EF, t.allowed.data(), t.n_groups, t.n_bits,
	                                        bad.data(), refused.ids.data(), refused.dist.data(), refused.counts.data()) == VSS_ERROR);
	EXPECT(std::strstr(vss_last_error(index.Handle()), "query 100 names group 4000000000"));
	EXPECT(refused.ids[0] == -2 && refused.counts[0] == 77); // (untouched)
	bool threw = false;
	try {
		index.ExecuteMultiScanBatchGrouped(*state, queries.data(), NQ, K, nullptr, t.n_groups, t.n_bits, t.group_of.data(), nullptr);
	} catch (const std::exception &) {
		threw = true;
	}
	EXPECT(threw);
	Results again(NQ);
	EXPECT(vss_search_batch_filtered_groups(index.Handle(), queries.data(), NQ, K, EF, t.allowed.data(), t.n_groups, t.n_bits,
	                                        t.group_of.data(), again.ids.data(), again.dist.data(), again.counts.data()) == VSS_OK);
	EXPECT(again.ids == grouped.ids && again.counts == grouped.counts &&
	       !std::memcmp(again.dist.data(), grouped.dist.data(), NQ * K * sizeof(float)));
	std::printf("one index: %zu queries in %zu groups, %zu rows returned, equal to the per-group calls\n", (size_t)NQ,
	            (size_t)t.n_groups, (size_t)total);
}

void Sharded(const FilterGroupTables &t, const std::vector<int> &devices, std::unique_ptr<ShardedHNSWIndex> &holder) {
	ShardedHNSWIndex &index = BuildSharded(holder, DIM, vecs, ids, dead, devices);

	Results grouped(NQ);
	index.SearchBatchFilteredGroups(queries.data(), NQ, K, EF, t.allowed.data(), t.n_groups, t.n_bits, t.group_of.data(),
	                                grouped.ids.data(), grouped.dist.data(), grouped.counts.data());
	ExpectOwnPredicate(t, grouped);
	for (idx_t g = 0; g != t.n_groups; ++g) {
		const auto mine = t.QueriesOf(g);
		const auto q = GatherRows(queries.data(), DIM, mine);
		Results alone(mine.size());
		index.SearchBatchFiltered(q.data(), mine.size(), K, EF, t.Group(g), t.n_bits, alone.ids.data(), alone.dist.data(),
		                          alone.counts.data());
		EXPECT(FirstDifference(grouped.ids.data(), alone.ids.data(), K, mine) == -1);
		EXPECT(FirstDifference(grouped.dist.data(), alone.dist.data(), K, mine) == -1);
		EXPECT(FirstDifference(grouped.counts.data(), alone.counts.data(), 1, mine) == -1);
	}
	// a query of an unknown group: refused before any device is touched
	std::vector<uint32_t> bad = t.group_of;
	bad[NQ - 1] = (uint32_t)t.n_groups;
	bool threw = false;
	try {
		Results refused(NQ);
		index.SearchBatchFilteredGroups(queries.data(), NQ, K, EF, t.allowed.data(), t.n_groups, t.n_bits, bad.data(),
		                                refused.ids.data(), refused.dist.data(), refused.counts.data());
	} catch (const std::exception &e) {
		threw = std::strstr(e.what(), "query 256 names group 5") != nullptr;
	}
	EXPECT(threw);
	std::printf("%zu shard(s), exchange %s: equal to the per-group calls\n", devices.size(), index.ExchangeKind());
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
		SingleIndex(t);
		Sharded(t, {0}, sharded_p[0]);
		Sharded(t, {0, 0}, sharded_p[1]);
	} catch (const std::exception &e) {
		std::fprintf(stderr, "EXCEPTION: %s\n", e.what());
		std::fflush(nullptr);
		std::_Exit(1);
	}
	std::printf("filter groups ok\n");
	std::fflush(nullptr);
	std::_Exit(0);
}
