// label_set_box_harness.cpp — an IN-list on one resident label column inside a box of ranges
// (vss_search_batch_by_label_set_box) through both host classes.
//     ./label_set_box_harness
//   1. vss_host::HNSWIndex on device 0: in every mode ExecuteMultiScanBatchByLabelSetBox against the bitmap method of that mode —
//      ExecuteMultiScanBatchGrouped / GroupedExact / GroupedAuto — on the table the contract derives from the columns
//      (csrc/label_filter.h: the distinct raw rows of (set words, lo, hi), as unsigned 64-bit words, are the groups, n_bits the
//      shortest of the set column and the range column): appended row ids, counts and routes; and the C entry point against the
//      bitmap entry point, cell by cell, distances by their bits
//   2. vss_host::ShardedHNSWIndex with 2 shards co-resident on device 0, every shard holding the whole columns:
//      SearchBatchByLabelSetBox against SearchBatchFilteredGroups / SearchExactBatchFilteredGroups / SearchBatchFilteredGroupsAuto
//      on the same table, cell by cell, the shards' route tables included — and against the single index's answers
// Data as in label_box64_harness.cpp: 64 seeded Gaussian clusters, dim 32, l2sq, 6001 rows with id = position, every ninth row
// deleted; 257 queries, k = 10, ef_search 64.  Column 1 (a group, 32 bits wide) for ids below 5998: (id * 7919) % 10, every 97th
// id none; column 3 (a timestamp, 64 BITS wide) for ids below 5500: BASE + (id * 104729) % 1000 with BASE = 2^63 + 10^15, every
// 89th id VSS_NO_LABEL64.  The set column is 1, the range column 3, the lists three words wide.  Query q brings one of ten
// predicates: lists of one to three groups, a repeated member, a permuted duplicate, an all-padding row, an empty range, a word
// beyond 32 bits, "no upper bound".  ROUTE_C = 300: the single index walks the widest predicate and scans the others; a shard
// decides by its own rows.  The first failed check or exception ends the process with a non-zero exit code.  Prints
// "label set box ok" last.  Needs a MI355X.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../csrc/label_filter.h"
#include "harness_common.hpp"

using namespace vss_host;

namespace {

constexpr idx_t DIM = 32, N = 6001, NQ = 257, K = 10, EF = 64, TENANTS = N - 3, STAMPS = 5500, M = 1, W = 3, PREDICATES = 10;
constexpr uint64_t ROUTE_C = 300; // (a list of three of the ten groups over every timestamp, some 1 400 live rows, is walked)
constexpr int MODES[3] = {VSS_BY_LABEL_GRAPH, VSS_BY_LABEL_EXACT, VSS_BY_LABEL_AUTO};
constexpr uint64_t TOP = VSS_NO_LABEL64, BASE = (1ull << 63) + 1000000000000000ull;
constexpr uint64_t PAD = VSS_NO_LABEL64;
constexpr uint32_t SET_COLUMN = 1;  // the group
const uint32_t COLUMNS[M] = {3};    // the timestamp
// (three set words, timestamp lo, hi)
constexpr uint64_t PREDICATE[PREDICATES][5] = {
    {4, 7, 2, BASE + 0, BASE + 499},     {4, PAD, PAD, BASE + 100, TOP},          {7, 4, 2, BASE + 0, BASE + 499}, // (a permuted duplicate)
    {3, 3, PAD, BASE + 300, BASE + 700}, {0, 1, 2, 0, TOP},                       {PAD, PAD, PAD, 0, TOP},         // (all padding)
    {4, 7, 2, BASE + 9, BASE + 2},       {(1ull << 32) + 4, 77, PAD, 0, TOP},     {PAD, 9, 8, BASE + 900, TOP},
    {5, 6, PAD, BASE + 2000, BASE + 3000}};
constexpr bool NONE[PREDICATES] = {false, false, false, false, false, true, true, true, false, true};

using Results = ResultsOf<K, NQ>;

std::vector<float> vecs(N *DIM), queries(NQ *DIM);
std::vector<row_t> ids(N), dead;
std::vector<uint32_t> tenant(TENANTS);
std::vector<uint64_t> stamp(STAMPS), sets(NQ *W), lo(NQ *M), hi(NQ *M);

// the table of the contract
std::vector<uint64_t> allowed;
std::vector<uint32_t> group_of;
idx_t n_groups;
constexpr idx_t N_BITS = STAMPS; // the shortest named column

Results single_answers; // mode exact: what the shards' merged answers must equal too
std::unique_ptr<HNSWIndex> single_p;
std::unique_ptr<ShardedHNSWIndex> sharded_p;

void DeriveTable() {
	std::vector<uint32_t> travelling, rows;
	vss::host::label_set_box_rows(sets.data(), W, lo.data(), hi.data(), NQ, M, travelling);
	vss::host::label_set_box_groups(travelling.data(), NQ, W, M, rows, group_of);
	const uint32_t per = vss::host::label_set_box_row_words(W, M);
	n_groups = rows.size() / per;
	EXPECT(n_groups == PREDICATES);
	const vss::host::LabelColumn64 index_columns[VSS_LABEL_COLUMNS_MAX] = {
	    {nullptr, nullptr, 0}, {tenant.data(), nullptr, TENANTS}, {nullptr, nullptr, 0}, {nullptr, stamp.data(), STAMPS}};
	const uint64_t words = (N_BITS + 63) / 64;
	allowed.assign(n_groups * words, 0);
	for (size_t g = 0; g != n_groups; ++g) {
		uint64_t word[W + 2 * M];
		for (idx_t e = 0; e != W + 2 * M; ++e)
			word[e] = vss::host::label_word64(rows.data() + g * per + 2 * e);
		for (uint64_t r = 0; r != N_BITS; ++r)
			if (vss::host::label_set_box_admits(index_columns, SET_COLUMN, word, W, COLUMNS, M, (int64_t)r, word + W))
				allowed[g * words + r / 64] |= 1ull << (r % 64);
	}
}

Results ByBox(vss_index *h, int mode) {
	Results r;
	EXPECT(vss_search_batch_by_label_set_box(h, queries.data(), NQ, K, EF, SET_COLUMN, sets.data(), W, COLUMNS, M, lo.data(), hi.data(), mode,
	                                         ROUTE_C, r.ids.data(), r.dist.data(), r.counts.data(), r.route.data()) == VSS_OK);
	return r;
}

// the bitmap call of `mode` on the table of the contract
Results ByBitmaps(vss_index *h, int mode) {
	Results r;
	int rc;
	if (mode == VSS_BY_LABEL_GRAPH) {
		rc = vss_search_batch_filtered_groups(h, queries.data(), NQ, K, EF, allowed.data(), n_groups, N_BITS, group_of.data(), r.ids.data(),
		                                      r.dist.data(), r.counts.data());
		r.route.assign(NQ, 0);
	} else if (mode == VSS_BY_LABEL_EXACT) {
		rc = vss_search_exact_batch_filtered_groups(h, queries.data(), NQ, K, allowed.data(), n_groups, N_BITS, group_of.data(), r.ids.data(),
		                                            r.dist.data(), r.counts.data());
		r.route.assign(NQ, 1);
	} else {
		rc = vss_search_batch_filtered_groups_auto(h, queries.data(), NQ, K, EF, allowed.data(), n_groups, N_BITS, group_of.data(), ROUTE_C,
		                                           r.ids.data(), r.dist.data(), r.counts.data(), r.route.data());
	}
	EXPECT(rc == VSS_OK);
	return r;
}

void SingleIndex() {
	HNSWIndex &index = BuildSingle(single_p, DIM, vecs, ids, dead, [](idx_t c, idx_t cnt) {
		if (c < TENANTS)
			single_p->SetLabelColumn(1, c, tenant.data() + c, std::min<idx_t>(cnt, TENANTS - c));
		if (c < STAMPS)
			single_p->SetLabelColumn64(3, c, stamp.data() + c, std::min<idx_t>(cnt, STAMPS - c));
	});
	EXPECT(index.LabelColumnRows(1) == TENANTS && index.LabelColumnRows(3) == STAMPS);
	EXPECT(index.LabelColumnWidth(1) == 32 && index.LabelColumnWidth(3) == 64 && index.LabelColumnWidth(0) == 0 && index.LabelColumnWidth(2) == 0);
	uint64_t n_exact = 0, n_graph = 0;
	for (int m = 0; m != 3; ++m) {
		const Results answers = ByBox(index.Handle(), MODES[m]);
		EXPECT(answers == ByBitmaps(index.Handle(), MODES[m]));
		// the mirror's chunk call against its bitmap methods: row ids appended query after query, counts, routes
		auto state = index.InitializeMultiScan(), state_b = index.InitializeMultiScan();
		std::vector<uint32_t> counts, counts_b;
		std::vector<uint8_t> route, route_b;
		const idx_t total = index.ExecuteMultiScanBatchByLabelSetBox(*state, queries.data(), NQ, K, SET_COLUMN, sets.data(), W, COLUMNS, M,
		                                                             lo.data(), hi.data(), &counts, &route, MODES[m], ROUTE_C);
		idx_t total_b;
		if (MODES[m] == VSS_BY_LABEL_GRAPH)
			total_b = index.ExecuteMultiScanBatchGrouped(*state_b, queries.data(), NQ, K, allowed.data(), n_groups, N_BITS, group_of.data(),
			                                             &counts_b);
		else if (MODES[m] == VSS_BY_LABEL_EXACT)
			total_b = index.ExecuteMultiScanBatchGroupedExact(*state_b, queries.data(), NQ, K, allowed.data(), n_groups, N_BITS, group_of.data(),
			                                                  &counts_b);
		else
			total_b = index.ExecuteMultiScanBatchGroupedAuto(*state_b, queries.data(), NQ, K, allowed.data(), n_groups, N_BITS, group_of.data(),
			                                                 &counts_b, &route_b, ROUTE_C);
		EXPECT(total == total_b && counts == counts_b && index.GetMultiScanResult(*state) == index.GetMultiScanResult(*state_b));
		EXPECT(counts == answers.counts && route == answers.route);
		if (MODES[m] == VSS_BY_LABEL_AUTO) {
			EXPECT(route == route_b);
			n_exact = std::count(route.begin(), route.end(), 1), n_graph = std::count(route.begin(), route.end(), 0);
			EXPECT(n_exact > 0 && n_graph > 0 && n_exact + n_graph == NQ); // both ways in one call
		}
		for (idx_t q = 0; q != NQ; ++q) {
			if (NONE[q % PREDICATES])
				EXPECT(answers.counts[q] == 0 && answers.ids[q * K] == -1 && std::isinf(answers.dist[q * K]));
			else if (MODES[m] == VSS_BY_LABEL_EXACT)
				EXPECT(answers.counts[q] == K);
		}
	}
	single_answers = ByBox(index.Handle(), VSS_BY_LABEL_EXACT);
	std::printf("one index: %zu queries, %llu walked and %llu scanned, equal to the bitmap methods cell by cell in three modes\n", (size_t)NQ,
	            (unsigned long long)n_graph, (unsigned long long)n_exact);
}

void Sharded(const std::vector<int> &devices) {
	ShardedHNSWIndex &index = BuildSharded(sharded_p, DIM, vecs, ids, dead, devices);
	index.SetLabelColumn(1, 0, tenant.data(), TENANTS);
	index.SetLabelColumn64(3, 0, stamp.data(), STAMPS);
	EXPECT(index.ShardCount() == devices.size());
	for (int m = 0; m != 3; ++m) {
		Results got, by_bitmaps;
		std::vector<uint8_t> routes, routes_b;
		index.SearchBatchByLabelSetBox(queries.data(), NQ, K, EF, SET_COLUMN, sets.data(), W, COLUMNS, M, lo.data(), hi.data(), MODES[m],
		                               ROUTE_C, got.ids.data(), got.dist.data(), got.counts.data(), &routes);
		EXPECT(routes.size() == devices.size() * NQ);
		if (MODES[m] == VSS_BY_LABEL_GRAPH)
			index.SearchBatchFilteredGroups(queries.data(), NQ, K, EF, allowed.data(), n_groups, N_BITS, group_of.data(), by_bitmaps.ids.data(),
			                                by_bitmaps.dist.data(), by_bitmaps.counts.data());
		else if (MODES[m] == VSS_BY_LABEL_EXACT)
			index.SearchExactBatchFilteredGroups(queries.data(), NQ, K, allowed.data(), n_groups, N_BITS, group_of.data(), by_bitmaps.ids.data(),
			                                     by_bitmaps.dist.data(), by_bitmaps.counts.data());
		else {
			index.SearchBatchFilteredGroupsAuto(queries.data(), NQ, K, EF, allowed.data(), n_groups, N_BITS, group_of.data(), ROUTE_C,
			                                    by_bitmaps.ids.data(), by_bitmaps.dist.data(), by_bitmaps.counts.data(), &routes_b);
			EXPECT(routes == routes_b); // each shard by its own counts, the same under both forms
		}
		EXPECT(got.SameAnswers(by_bitmaps));
		if (MODES[m] == VSS_BY_LABEL_EXACT) // every shard scans its own rows and the merge keeps the k nearest: the single index's answers
			EXPECT(got.SameAnswers(single_answers));
	}
	std::printf("%zu shards, exchange %s: equal to the bitmap methods cell by cell in three modes\n", devices.size(), index.ExchangeKind());
}

} // namespace

int main() {
	ClusteredData(20261021, DIM, N, NQ, 64, 0.3f, vecs, queries);
	for (idx_t i = 0; i != N; ++i)
		ids[i] = (row_t)i;
	for (idx_t i = 0; i != N; ++i)
		if (i % 9 == 4)
			dead.push_back((row_t)i);
	// the columns label deleted rows too (they know nothing of tombstones): the engine excludes them
	for (idx_t i = 0; i != TENANTS; ++i)
		tenant[i] = i % 97 == 5 ? VSS_NO_LABEL : (uint32_t)((i * 7919) % 10);
	for (idx_t i = 0; i != STAMPS; ++i)
		stamp[i] = i % 89 == 7 ? VSS_NO_LABEL64 : BASE + (i * 104729) % 1000;
	for (idx_t q = 0; q != NQ; ++q) {
		const uint64_t *p = PREDICATE[q % PREDICATES];
		std::copy(p, p + W, sets.begin() + q * W);
		lo[q] = p[W], hi[q] = p[W + 1];
	}
	DeriveTable();
	try {
		SingleIndex();
		Sharded({0, 0});
	} catch (const std::exception &e) {
		std::fprintf(stderr, "EXCEPTION: %s\n", e.what());
		std::fflush(nullptr);
		std::_Exit(1);
	}
	std::printf("label set box ok\n");
	std::fflush(nullptr);
	std::_Exit(0);
}
