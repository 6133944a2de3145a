// label_search_harness.cpp — equality predicates on the resident label column (vss_search_batch_by_label) through both host
// classes.
//     ./label_search_harness
//   1. vss_host::HNSWIndex on device 0: in every mode the C entry point against the bitmap call of that mode on the table the
//      contract derives from the column (csrc/label_filter.h: the distinct wanted values are the groups), cell by cell, routes
//      included; ExecuteMultiScanBatchByLabel against the entry point; a search after ClearLabels is refused
//   2. vss_host::ShardedHNSWIndex with 1 and 3 shards co-resident on device 0, every shard holding the whole column:
//      SearchBatchByLabel in mode exact against the single index's answers, cell by cell; in modes graph and auto against the
//      CPU merge — by (distance, row id) — of the per-shard entry point's answers, and its route tables against theirs; one
//      shard is the single index in every mode
// Data as in filter_route_harness.cpp: 64 seeded Gaussian clusters, dim 32, l2sq, 6001 rows with id = position, every ninth row
// deleted; 257 queries, k = 10, ef_search 64.  Labels for ids below 5998: even ids tenant 100 (half the table), odd ids tenant
// id % 16 (eight tenants), every 97th id none; query q wants one of the eight small tenants, tenant 100, VSS_NO_LABEL or a
// value no row carries.  ROUTE_C = 1000: the single index (5334 live rows: lists of at most 2309 rows are scanned) walks tenant
// 100 and scans the others; a shard decides by its own rows.  The first failed check or exception ends the process with a
// non-zero exit code.  Prints "label search ok" last.  Needs a MI355X.
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

using Results = ResultsOf<K, NQ>;

std::vector<float> vecs(N *DIM), queries(NQ *DIM);
std::vector<row_t> ids(N), dead;
std::vector<uint32_t> labels(LABELLED), want(NQ);

std::unique_ptr<HNSWIndex> single_p;
std::unique_ptr<ShardedHNSWIndex> sharded_p[2];

Results ByLabel(vss_index *h, int mode) {
	Results r;
	EXPECT(vss_search_batch_by_label(h, queries.data(), NQ, K, EF, want.data(), mode, ROUTE_C, r.ids.data(), r.dist.data(),
	                                 r.counts.data(), r.route.data()) == VSS_OK);
	return r;
}

// the bitmap call of `mode` on the table of the contract
Results ByBitmaps(vss_index *h, int mode) {
	std::vector<uint32_t> values, group_of;
	vss::host::label_groups(want.data(), NQ, values, group_of);
	const uint64_t words = (LABELLED + 63) / 64;
	std::vector<uint64_t> allowed(values.size() * words, 0);
	for (size_t g = 0; g != values.size(); ++g)
		for (uint64_t r = 0; r != LABELLED; ++r)
			if (vss::host::label_admits(labels.data(), LABELLED, (int64_t)r, values[g]))
				allowed[g * words + r / 64] |= 1ull << (r % 64);
	Results r;
	int rc;
	if (mode == VSS_BY_LABEL_GRAPH) {
		rc = vss_search_batch_filtered_groups(h, queries.data(), NQ, K, EF, allowed.data(), values.size(), LABELLED, group_of.data(),
		                                      r.ids.data(), r.dist.data(), r.counts.data());
		r.route.assign(NQ, 0);
	} else if (mode == VSS_BY_LABEL_EXACT) {
		rc = vss_search_exact_batch_filtered_groups(h, queries.data(), NQ, K, allowed.data(), values.size(), LABELLED, group_of.data(),
		                                            r.ids.data(), r.dist.data(), r.counts.data());
		r.route.assign(NQ, 1);
	} else {
		rc = vss_search_batch_filtered_groups_auto(h, queries.data(), NQ, K, EF, allowed.data(), values.size(), LABELLED, group_of.data(),
		                                           ROUTE_C, r.ids.data(), r.dist.data(), r.counts.data(), r.route.data());
	}
	EXPECT(rc == VSS_OK);
	return r;
}

void SingleIndex(Results (&answers)[3]) {
	// the labels travel with the rows, chunk by chunk: the column grows as the table does
	HNSWIndex &index = BuildSingle(single_p, DIM, vecs, ids, dead, [](idx_t c, idx_t cnt) {
		if (c < LABELLED)
			single_p->SetLabels(c, labels.data() + c, std::min<idx_t>(cnt, LABELLED - c));
	});
	EXPECT(index.LabelledRows() == LABELLED);
	for (int m = 0; m != 3; ++m) {
		answers[m] = ByLabel(index.Handle(), MODES[m]);
		EXPECT(answers[m] == ByBitmaps(index.Handle(), MODES[m]));
		// the mirror's chunk call: row ids appended query after query, the routes handed on
		auto state = index.InitializeMultiScan();
		std::vector<uint32_t> counts;
		std::vector<uint8_t> route;
		const idx_t total = index.ExecuteMultiScanBatchByLabel(*state, queries.data(), NQ, K, want.data(), &counts, &route, MODES[m], ROUTE_C);
		const auto &appended = index.GetMultiScanResult(*state);
		EXPECT(counts == answers[m].counts && route == answers[m].route && appended.size() == total);
		for (idx_t q = 0, at = 0; q != NQ; at += counts[q++])
			for (idx_t j = 0; j != counts[q]; ++j)
				EXPECT(appended[at + j] == answers[m].ids[q * K + j]);
	}
	const Results &routed = answers[2];
	const uint64_t n_exact = std::count(routed.route.begin(), routed.route.end(), 1);
	const uint64_t n_graph = std::count(routed.route.begin(), routed.route.end(), 0);
	EXPECT(n_exact > 0 && n_graph > 0 && n_exact + n_graph == NQ); // both ways in one call
	for (idx_t q = 0; q != NQ; ++q) {
		EXPECT(routed.route[q] == (want[q] == 100 ? 0 : 1));
		if (want[q] == VSS_NO_LABEL || want[q] == 777)
			for (int m = 0; m != 3; ++m)
				EXPECT(answers[m].counts[q] == 0 && answers[m].ids[q * K] == -1 && std::isinf(answers[m].dist[q * K]));
		else
			EXPECT(answers[1].counts[q] == K);
	}
	std::printf("one index: %zu queries, %llu walked and %llu scanned, equal to the bitmap calls cell by cell in three modes\n", (size_t)NQ,
	            (unsigned long long)n_graph, (unsigned long long)n_exact);
}

void Refused() {
	// a second small index: cleared labels refuse the search, and so does an index that never had any
	const OptionMap options = {{"metric", OptionValue::String("l2sq")}};
	HNSWIndex index(DIM, options, 100);
	index.BulkReserve(100, 1);
	index.BulkAppendChunk(vecs.data(), ids.data(), nullptr, 100);
	index.BulkFinalize();
	for (int leg = 0; leg != 2; ++leg) {
		bool threw = false;
		try {
			auto state = index.InitializeMultiScan();
			index.ExecuteMultiScanBatchByLabel(*state, queries.data(), 4, K, want.data(), nullptr);
		} catch (const std::exception &e) {
			threw = std::strstr(e.what(), "no label column") != nullptr;
		}
		EXPECT(threw);
		index.SetLabels(0, labels.data(), 100);
		EXPECT(index.LabelledRows() == 100);
		index.ClearLabels();
		EXPECT(index.LabelledRows() == 0);
	}
}

void Sharded(const std::vector<int> &devices, std::unique_ptr<ShardedHNSWIndex> &holder, const Results (&single)[3]) {
	ShardedHNSWIndex &index = BuildSharded(holder, DIM, vecs, ids, dead, devices);
	index.SetLabels(0, labels.data(), LABELLED);
	const idx_t G = index.ShardCount();
	for (int m = 0; m != 3; ++m) {
		Results got;
		std::vector<uint8_t> routes;
		index.SearchBatchByLabel(queries.data(), NQ, K, EF, want.data(), MODES[m], ROUTE_C, got.ids.data(), got.dist.data(),
		                         got.counts.data(), &routes);
		EXPECT(routes.size() == G * NQ);
		std::vector<Results> per_shard;
		for (idx_t g = 0; g != G; ++g) {
			per_shard.push_back(ByLabel(index.ShardHandle(g), MODES[m]));
			EXPECT(!std::memcmp(routes.data() + g * NQ, per_shard.back().route.data(), NQ)); // each shard by its own counts
		}
		EXPECT(got.SameAnswers(Merge(per_shard, NQ)));
		if (MODES[m] == VSS_BY_LABEL_EXACT || G == 1) // the exact answer does not depend on the sharding; one shard is the single index
			EXPECT(got.SameAnswers(single[m]));
	}
	std::printf("%zu shard(s), exchange %s: equal to the single index (exact) and to the merge of the per-shard calls, cell by cell\n",
	            devices.size(), index.ExchangeKind());
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
		labels[i] = i % 97 == 5 ? VSS_NO_LABEL : i % 2 == 0 ? 100u : (uint32_t)(i % 16);
	for (idx_t q = 0; q != NQ; ++q) {
		const idx_t w = q % 11;
		want[q] = w < 8 ? (uint32_t)(2 * w + 1) : w == 8 ? 100u : w == 9 ? VSS_NO_LABEL : 777u;
	}
	try {
		Results single[3];
		SingleIndex(single);
		Refused();
		Sharded({0}, sharded_p[0], single);
		Sharded({0, 0, 0}, sharded_p[1], single);
	} catch (const std::exception &e) {
		std::fprintf(stderr, "EXCEPTION: %s\n", e.what());
		std::fflush(nullptr);
		std::_Exit(1);
	}
	std::printf("label search ok\n");
	std::fflush(nullptr);
	std::_Exit(0);
}
