// label_box64_harness.cpp — conjunctions of ranges with 64-bit ends over resident label columns of either width
// (vss_search_batch_by_label_box64) through both host classes.
//     ./label_box64_harness
//   1. vss_host::HNSWIndex on device 0: in every mode ExecuteMultiScanBatchByLabelBox64 against the bitmap method of that mode —
//      ExecuteMultiScanBatchGrouped / GroupedExact / GroupedAuto — on the table the contract derives from the columns
//      (csrc/label_filter.h: the distinct raw rows of (lo, hi) pairs, as unsigned 64-bit words, are the groups, n_bits the shortest
//      named column): appended row ids, counts and routes; and the C entry point against the bitmap entry point, cell by cell,
//      distances by their bits
//   2. vss_host::ShardedHNSWIndex with 3 shards co-resident on device 0, every shard holding the whole columns:
//      SearchBatchByLabelBox64 against SearchBatchFilteredGroups / SearchExactBatchFilteredGroups / SearchBatchFilteredGroupsAuto
//      on the same table, cell by cell, the shards' route tables included
// Data as in label_box_harness.cpp: 64 seeded Gaussian clusters, dim 32, l2sq, 6001 rows with id = position, every ninth row
// deleted; 257 queries, k = 10, ef_search 64.  Column 1 (a tenant, 32 bits wide) for ids below 5998: (id * 7919) % 10, every 97th
// id none; column 3 (a timestamp, 64 BITS wide) for ids below 5500: BASE + (id * 104729) % 1000 with BASE = 2^63 + 10^15 — a
// TIMESTAMP of our days under x ^ 2^63, so that every comparison needs the high word — every 89th id VSS_NO_LABEL64.  The call names
// {3, 1}.  Query q brings one of eleven boxes, label_box_harness.cpp's with the timestamps moved up by BASE.  ROUTE_C = 1000: the
// single index walks the widest boxes and scans the others; a shard decides by its own rows.  The first failed check or
// exception ends the process with a non-zero exit code.  Prints "label box64 ok" last.  Needs a MI355X.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../csrc/label_filter.h"
#include "harness_common.hpp"

using namespace vss_host;

namespace {

constexpr idx_t DIM = 32, N = 6001, NQ = 257, K = 10, EF = 64, TENANTS = N - 3, STAMPS = 5500, M = 2;
constexpr uint64_t ROUTE_C = 1000;
constexpr int MODES[3] = {VSS_BY_LABEL_GRAPH, VSS_BY_LABEL_EXACT, VSS_BY_LABEL_AUTO};
constexpr uint64_t TOP = VSS_NO_LABEL64, BASE = (1ull << 63) + 1000000000000000ull;
const uint32_t COLUMNS[M] = {3, 1}; // the timestamp first, then the tenant
// (timestamp lo, hi, tenant lo, hi)
constexpr uint64_t BOXES[11][4] = {{BASE + 0, BASE + 499, 4, 4},   {BASE + 100, BASE + 199, 4, 4}, {BASE + 150, BASE + 400, 7, 7},
                                   {BASE + 300, BASE + 700, 7, 7}, {0, TOP, 2, 6},                 {0, TOP, 0, TOP},
                                   {BASE + 9, BASE + 2, 4, 4},     {BASE, TOP, 8, 3},              {0, TOP, 77, 77},
                                   {BASE + 900, TOP, 0, 9},        {BASE + 2000, BASE + 3000, 0, 9}};

using Results = ResultsOf<K, NQ>;

std::vector<float> vecs(N *DIM), queries(NQ *DIM);
std::vector<row_t> ids(N), dead;
std::vector<uint32_t> tenant(TENANTS);
std::vector<uint64_t> stamp(STAMPS), lo(NQ *M), hi(NQ *M);

// the table of the contract
std::vector<uint64_t> allowed;
std::vector<uint32_t> group_of;
idx_t n_groups;
constexpr idx_t N_BITS = STAMPS; // the shortest named column

std::unique_ptr<HNSWIndex> single_p;
std::unique_ptr<ShardedHNSWIndex> sharded_p;

void DeriveTable() {
	std::vector<uint32_t> boxes, rows;
	vss::host::label_box64_rows(lo.data(), hi.data(), NQ, M, boxes);
	vss::host::label_box64_groups(boxes.data(), NQ, M, rows, group_of);
	n_groups = rows.size() / (4 * M);
	EXPECT(n_groups == 11);
	const vss::host::LabelColumn64 index_columns[VSS_LABEL_COLUMNS_MAX] = {
	    {nullptr, nullptr, 0}, {tenant.data(), nullptr, TENANTS}, {nullptr, nullptr, 0}, {nullptr, stamp.data(), STAMPS}};
	const uint64_t words = (N_BITS + 63) / 64;
	allowed.assign(n_groups * words, 0);
	for (size_t g = 0; g != n_groups; ++g) {
		uint64_t box[2 * M];
		for (idx_t e = 0; e != 2 * M; ++e)
			box[e] = vss::host::label_word64(rows.data() + g * 4 * M + 2 * e);
		for (uint64_t r = 0; r != N_BITS; ++r)
			if (vss::host::label_box64_admits(index_columns, COLUMNS, M, (int64_t)r, box))
				allowed[g * words + r / 64] |= 1ull << (r % 64);
	}
}

Results ByBox(vss_index *h, int mode) {
	Results r;
	EXPECT(vss_search_batch_by_label_box64(h, queries.data(), NQ, K, EF, COLUMNS, M, lo.data(), hi.data(), mode, ROUTE_C, r.ids.data(),
	                                       r.dist.data(), r.counts.data(), r.route.data()) == VSS_OK);
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
		const idx_t total = index.ExecuteMultiScanBatchByLabelBox64(*state, queries.data(), NQ, K, COLUMNS, M, lo.data(), hi.data(), &counts,
		                                                            &route, MODES[m], ROUTE_C);
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
			const uint64_t *box = BOXES[q % 11];
			const bool none = box[0] > box[1] || box[2] > box[3] || box[2] == 77 || box[0] == BASE + 2000;
			if (none)
				EXPECT(answers.counts[q] == 0 && answers.ids[q * K] == -1 && std::isinf(answers.dist[q * K]));
			else if (MODES[m] == VSS_BY_LABEL_EXACT)
				EXPECT(answers.counts[q] == K);
		}
	}
	// a setter of the other width is refused while the column has cells, and the 32-bit box call refuses the wide column
	EXPECT(vss_set_label_column(index.Handle(), 3, 0, tenant.data(), 4) != VSS_OK);
	EXPECT(vss_set_label_column64(index.Handle(), 1, 0, stamp.data(), 4) != VSS_OK);
	EXPECT(index.LabelColumnWidth(1) == 32 && index.LabelColumnWidth(3) == 64);
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
		index.SearchBatchByLabelBox64(queries.data(), NQ, K, EF, COLUMNS, M, lo.data(), hi.data(), MODES[m], ROUTE_C, got.ids.data(),
		                              got.dist.data(), got.counts.data(), &routes);
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
	for (idx_t q = 0; q != NQ; ++q)
		for (idx_t j = 0; j != M; ++j)
			lo[q * M + j] = BOXES[q % 11][2 * j], hi[q * M + j] = BOXES[q % 11][2 * j + 1];
	DeriveTable();
	try {
		SingleIndex();
		Sharded({0, 0, 0});
	} catch (const std::exception &e) {
		std::fprintf(stderr, "EXCEPTION: %s\n", e.what());
		std::fflush(nullptr);
		std::_Exit(1);
	}
	std::printf("label box64 ok\n");
	std::fflush(nullptr);
	std::_Exit(0);
}
