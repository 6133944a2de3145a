// label_set_harness.cpp — IN-list predicates on the resident label column (vss_search_batch_by_label_set) through both host
// classes.
//     ./label_set_harness
//   1. vss_host::HNSWIndex on device 0: in every mode ExecuteMultiScanBatchByLabelSet against the bitmap method of that mode —
//      ExecuteMultiScanBatchGrouped / GroupedExact / GroupedAuto — on the table the contract derives from the column
//      (csrc/label_filter.h: the distinct raw rows are the groups): appended row ids, counts and routes; and the C entry point
//      against the bitmap entry point, cell by cell, distances by their bits
//   2. vss_host::ShardedHNSWIndex with 3 shards co-resident on device 0, every shard holding the whole column:
//      SearchBatchByLabelSet against SearchBatchFilteredGroups / SearchExactBatchFilteredGroups / SearchBatchFilteredGroupsAuto
//      on the same table, cell by cell, the shards' route tables included
// Data as in label_search_harness.cpp: 64 seeded Gaussian clusters, dim 32, l2sq, 6001 rows with id = position, every ninth row
// deleted; 257 queries, k = 10, ef_search 64.  Labels for ids below 5998: v = (id * 7919) % 1000, folded to v % 8 where v < 500
// (eight large groups) and kept otherwise, every 97th id none.  Query q brings one of eleven rows of eight words: the eight large
// groups in two orders, four of them in two orders, a singleton, a repeat, three small values, padding around values, all
// padding, and values no row holds.  ROUTE_C = 1000: the single index (5334 live rows: lists of at most 2309 rows are scanned)
// walks the two widest sets and scans the others; a shard decides by its own rows.  The first failed check or exception ends the
// process with a non-zero exit code.  Prints "label set ok" last.  Needs a MI355X.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../csrc/label_filter.h"
#include "harness_common.hpp"

using namespace vss_host;

namespace {

constexpr idx_t DIM = 32, N = 6001, NQ = 257, K = 10, EF = 64, LABELLED = N - 3;
constexpr uint64_t ROUTE_C = 1000;
constexpr int MODES[3] = {VSS_BY_LABEL_GRAPH, VSS_BY_LABEL_EXACT, VSS_BY_LABEL_AUTO};
constexpr uint32_t WIDTH = 8, P = VSS_NO_LABEL;
constexpr uint32_t SETS[11][WIDTH] = {{0, 1, 2, 3, 4, 5, 6, 7}, {7, 6, 5, 4, 3, 2, 1, 0}, {0, 1, 2, 3, P, P, P, P}, {3, 2, 1, 0, P, P, P, P},
                                      {4, P, P, P, P, P, P, P}, {5, 5, 5, P, P, P, P, P}, {600, 601, 602, P, P, P, P, P},
                                      {P, 7, P, 6, P, P, P, P}, {P, P, P, P, P, P, P, P}, {2000, 3000, P, P, P, P, P, P},
                                      {700, 701, 702, 703, 704, 705, 706, 1}};
constexpr bool NONE[11] = {false, false, false, false, false, false, false, false, true, true, false};

using Results = ResultsOf<K, NQ>;

std::vector<float> vecs(N *DIM), queries(NQ *DIM);
std::vector<row_t> ids(N), dead;
std::vector<uint32_t> labels(LABELLED), sets(NQ *WIDTH);

// the table of the contract
std::vector<uint64_t> allowed;
std::vector<uint32_t> group_of;
idx_t n_groups;

std::unique_ptr<HNSWIndex> single_p;
std::unique_ptr<ShardedHNSWIndex> sharded_p;

void DeriveTable() {
	std::vector<uint32_t> rows;
	vss::host::label_set_groups(sets.data(), NQ, WIDTH, rows, group_of);
	n_groups = rows.size() / WIDTH;
	EXPECT(n_groups == 11);
	const uint64_t words = (LABELLED + 63) / 64;
	allowed.assign(n_groups * words, 0);
	for (size_t g = 0; g != n_groups; ++g)
		for (uint64_t r = 0; r != LABELLED; ++r)
			if (vss::host::label_set_admits(labels.data(), LABELLED, (int64_t)r, rows.data() + g * WIDTH, WIDTH))
				allowed[g * words + r / 64] |= 1ull << (r % 64);
}

Results BySet(vss_index *h, int mode) {
	Results r;
	EXPECT(vss_search_batch_by_label_set(h, queries.data(), NQ, K, EF, sets.data(), WIDTH, mode, ROUTE_C, r.ids.data(), r.dist.data(),
	                                     r.counts.data(), r.route.data()) == VSS_OK);
	return r;
}

// the bitmap call of `mode` on the table of the contract
Results ByBitmaps(vss_index *h, int mode) {
	Results r;
	int rc;
	if (mode == VSS_BY_LABEL_GRAPH) {
		rc = vss_search_batch_filtered_groups(h, queries.data(), NQ, K, EF, allowed.data(), n_groups, LABELLED, group_of.data(), r.ids.data(),
		                                      r.dist.data(), r.counts.data());
		r.route.assign(NQ, 0);
	} else if (mode == VSS_BY_LABEL_EXACT) {
		rc = vss_search_exact_batch_filtered_groups(h, queries.data(), NQ, K, allowed.data(), n_groups, LABELLED, group_of.data(),
		                                            r.ids.data(), r.dist.data(), r.counts.data());
		r.route.assign(NQ, 1);
	} else {
		rc = vss_search_batch_filtered_groups_auto(h, queries.data(), NQ, K, EF, allowed.data(), n_groups, LABELLED, group_of.data(), ROUTE_C,
		                                           r.ids.data(), r.dist.data(), r.counts.data(), r.route.data());
	}
	EXPECT(rc == VSS_OK);
	return r;
}

void SingleIndex() {
	HNSWIndex &index = BuildSingle(single_p, DIM, vecs, ids, dead, [](idx_t c, idx_t cnt) {
		if (c < LABELLED)
			single_p->SetLabels(c, labels.data() + c, std::min<idx_t>(cnt, LABELLED - c));
	});
	EXPECT(index.LabelledRows() == LABELLED);
	uint64_t n_exact = 0, n_graph = 0;
	for (int m = 0; m != 3; ++m) {
		const Results answers = BySet(index.Handle(), MODES[m]);
		EXPECT(answers == ByBitmaps(index.Handle(), MODES[m]));
		// the mirror's chunk call against its bitmap methods: row ids appended query after query, counts, routes
		auto state = index.InitializeMultiScan(), state_b = index.InitializeMultiScan();
		std::vector<uint32_t> counts, counts_b;
		std::vector<uint8_t> route, route_b;
		const idx_t total =
		    index.ExecuteMultiScanBatchByLabelSet(*state, queries.data(), NQ, K, sets.data(), WIDTH, &counts, &route, MODES[m], ROUTE_C);
		idx_t total_b;
		if (MODES[m] == VSS_BY_LABEL_GRAPH)
			total_b = index.ExecuteMultiScanBatchGrouped(*state_b, queries.data(), NQ, K, allowed.data(), n_groups, LABELLED, group_of.data(),
			                                             &counts_b);
		else if (MODES[m] == VSS_BY_LABEL_EXACT)
			total_b = index.ExecuteMultiScanBatchGroupedExact(*state_b, queries.data(), NQ, K, allowed.data(), n_groups, LABELLED,
			                                                  group_of.data(), &counts_b);
		else
			total_b = index.ExecuteMultiScanBatchGroupedAuto(*state_b, queries.data(), NQ, K, allowed.data(), n_groups, LABELLED,
			                                                 group_of.data(), &counts_b, &route_b, ROUTE_C);
		EXPECT(total == total_b && counts == counts_b && index.GetMultiScanResult(*state) == index.GetMultiScanResult(*state_b));
		EXPECT(counts == answers.counts && route == answers.route);
		if (MODES[m] == VSS_BY_LABEL_AUTO) {
			EXPECT(route == route_b);
			n_exact = std::count(route.begin(), route.end(), 1), n_graph = std::count(route.begin(), route.end(), 0);
			EXPECT(n_exact > 0 && n_graph > 0 && n_exact + n_graph == NQ); // both ways in one call
		}
		for (idx_t q = 0; q != NQ; ++q) {
			if (NONE[q % 11])
				EXPECT(answers.counts[q] == 0 && answers.ids[q * K] == -1 && std::isinf(answers.dist[q * K]));
			else if (MODES[m] == VSS_BY_LABEL_EXACT && q % 11 < 6)
				EXPECT(answers.counts[q] == K);
			// the same members in another order: another group, the same rows (queries q and q + 1 differ, so by their counts)
			if (MODES[m] == VSS_BY_LABEL_EXACT && q % 11 == 2 && q + 1 < NQ)
				EXPECT(answers.counts[q] == answers.counts[q + 1]);
		}
	}
	std::printf("one index: %zu queries, %llu walked and %llu scanned, equal to the bitmap methods cell by cell in three modes\n", (size_t)NQ,
	            (unsigned long long)n_graph, (unsigned long long)n_exact);
}

void Sharded(const std::vector<int> &devices) {
	ShardedHNSWIndex &index = BuildSharded(sharded_p, DIM, vecs, ids, dead, devices);
	index.SetLabels(0, labels.data(), LABELLED);
	EXPECT(index.ShardCount() == devices.size());
	for (int m = 0; m != 3; ++m) {
		Results got, by_bitmaps;
		std::vector<uint8_t> routes, routes_b;
		index.SearchBatchByLabelSet(queries.data(), NQ, K, EF, sets.data(), WIDTH, MODES[m], ROUTE_C, got.ids.data(), got.dist.data(),
		                            got.counts.data(), &routes);
		EXPECT(routes.size() == devices.size() * NQ);
		if (MODES[m] == VSS_BY_LABEL_GRAPH)
			index.SearchBatchFilteredGroups(queries.data(), NQ, K, EF, allowed.data(), n_groups, LABELLED, group_of.data(), by_bitmaps.ids.data(),
			                                by_bitmaps.dist.data(), by_bitmaps.counts.data());
		else if (MODES[m] == VSS_BY_LABEL_EXACT)
			index.SearchExactBatchFilteredGroups(queries.data(), NQ, K, allowed.data(), n_groups, LABELLED, group_of.data(),
			                                     by_bitmaps.ids.data(), by_bitmaps.dist.data(), by_bitmaps.counts.data());
		else {
			index.SearchBatchFilteredGroupsAuto(queries.data(), NQ, K, EF, allowed.data(), n_groups, LABELLED, group_of.data(), ROUTE_C,
			                                    by_bitmaps.ids.data(), by_bitmaps.dist.data(), by_bitmaps.counts.data(), &routes_b);
			EXPECT(routes == routes_b); // each shard by its own counts, the same under both forms
		}
		EXPECT(got.SameAnswers(by_bitmaps));
	}
	std::printf("%zu shards, exchange %s: equal to the bitmap methods cell by cell in three modes\n", devices.size(), index.ExchangeKind());
}

} // namespace

int main() {
	ClusteredData(20261020, DIM, N, NQ, 64, 0.3f, vecs, queries);
	for (idx_t i = 0; i != N; ++i)
		ids[i] = (row_t)i;
	for (idx_t i = 0; i != N; ++i)
		if (i % 9 == 4)
			dead.push_back((row_t)i);
	// the column labels deleted rows too (it knows nothing of tombstones): the engine excludes them
	for (idx_t i = 0; i != LABELLED; ++i)
		labels[i] = i % 97 == 5 ? VSS_NO_LABEL : (uint32_t)((i * 7919) % 1000 < 500 ? (i * 7919) % 8 : (i * 7919) % 1000);
	for (idx_t q = 0; q != NQ; ++q)
		std::copy(SETS[q % 11], SETS[q % 11] + WIDTH, sets.begin() + q * WIDTH);
	DeriveTable();
	try {
		SingleIndex();
		Sharded({0, 0, 0});
	} catch (const std::exception &e) {
		std::fprintf(stderr, "EXCEPTION: %s\n", e.what());
		std::fflush(nullptr);
		std::_Exit(1);
	}
	std::printf("label set ok\n");
	std::fflush(nullptr);
	std::_Exit(0);
}
