// filter_probe_harness.cpp — filtered probes through the calling conventions a join operator is fast with: a search context
// per pipeline thread (vss_search_batch_filtered_device_begin, vss_search_batch_filtered_groups_device_begin, completed by
// vss_search_batch_end) and several chunks answered by one launch (vss_search_multi_filtered_device_begin).
//     ./filter_probe_harness
//   1. one index, directly on the C ABI: the three calls, CELL BY CELL (row ids, distance bits, counts) against their blocking
//      counterparts — three contexts in flight under three bitmaps, the grouped form, and one launch of four chunks with a table
//      each (one of them a single bitmap without group numbers)
//   2. vss_host::ShardedHNSWIndex with one shard, 3. with two shards co-resident on device 0: SearchBatchFiltered and
//      SearchBatchFilteredGroups — which start every shard through the _begin forms — against the merge, done here on the CPU
//      by ascending (distance, row id), of one blocking call per shard
// Data as in filter_groups_harness.cpp: 64 seeded Gaussian clusters, dim 32, l2sq, 6001 rows with id = position, every ninth
// row deleted; 256 queries, k = 10, ef 64; tenants over n_bits = 5998.  The first failed check or exception ends the process
// with a non-zero exit code, without unwinding.  Prints "filter probes ok" last.  Needs a MI355X.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "filter_group_tables.hpp"
#include "harness_common.hpp"

using namespace vss_host;

namespace {

constexpr idx_t DIM = 32, N = 6001, NQ = 256, K = 10, EF = 64, N_BITS = N - 3, CHUNKS = 4, PER_CHUNK = NQ / CHUNKS;

using Results = ResultsOf<K>;

std::vector<float> vecs(N *DIM), queries(NQ *DIM);
std::vector<row_t> ids(N), dead;
bool Live(uint64_t id) {
	return id % 9 != 4;
}

// device memory that lives to the end of the process (the process ends without unwinding)
template <class T>
T *Device(const T *host, size_t n) {
	T *p = nullptr;
	EXPECT(hipMalloc((void **)&p, std::max<size_t>(n, 1) * sizeof(T)) == hipSuccess);
	if (host)
		EXPECT(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice) == hipSuccess);
	return p;
}

// the device cells of one batch of answers, pre-filled so that a cell nobody wrote shows
struct Cells {
	idx_t nq;
	row_t *ids;
	float *dist;
	uint32_t *counts;
	explicit Cells(idx_t n) : nq(n) {
		const Results fill(n);
		ids = Device(fill.ids.data(), n * K), dist = Device(fill.dist.data(), n * K), counts = Device(fill.counts.data(), n);
	}
	Results Fetch() const {
		Results r(nq);
		EXPECT(hipMemcpy(r.ids.data(), ids, nq * K * sizeof(row_t), hipMemcpyDeviceToHost) == hipSuccess);
		EXPECT(hipMemcpy(r.dist.data(), dist, nq * K * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess);
		EXPECT(hipMemcpy(r.counts.data(), counts, nq * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess);
		return r;
	}
};

// the holders live outside main's try block: an exception ends the process before any destructor runs
std::unique_ptr<HNSWIndex> single_p;
std::unique_ptr<ShardedHNSWIndex> sharded_p[2];

void SingleIndex(const FilterGroupTables &t) {
	HNSWIndex &index = BuildSingle(single_p, DIM, vecs, ids, dead);
	vss_index *h = index.Handle();
	const float *d_q = Device(queries.data(), NQ * DIM);
	const uint64_t *d_table = Device(t.allowed.data(), t.allowed.size());
	const uint32_t *d_groups = Device(t.group_of.data(), NQ);

	// one bitmap per context, three contexts in flight, completed out of order
	std::vector<Results> blocking;
	for (idx_t g = 0; g != 3; ++g) {
		Cells cells(NQ);
		EXPECT(vss_search_batch_filtered_device(h, d_q, NQ, K, EF, d_table + g * t.words, t.n_bits, cells.ids, cells.dist,
		                                        cells.counts) == VSS_OK);
		blocking.push_back(cells.Fetch());
	}
	std::vector<Cells> flight;
	for (idx_t g = 0; g != 3; ++g) {
		flight.emplace_back(NQ);
		EXPECT(vss_search_batch_filtered_device_begin(h, (int)g, d_q, NQ, K, EF, d_table + g * t.words, t.n_bits, flight[g].ids,
		                                              flight[g].dist, flight[g].counts) == VSS_OK);
	}
	EXPECT(vss_search_batch_filtered_device_begin(h, 1, d_q, NQ, K, EF, d_table, t.n_bits, flight[1].ids, flight[1].dist,
	                                              flight[1].counts) == VSS_ERROR);
	EXPECT(std::strstr(vss_last_error(h), "already has a batch in flight"));
	for (int context : {2, 0, 1})
		EXPECT(vss_search_batch_end(h, context) == VSS_OK);
	for (idx_t g = 0; g != 3; ++g)
		EXPECT(flight[g].Fetch() == blocking[g]);

	// one predicate per query
	Cells grouped_blocking(NQ), grouped(NQ);
	EXPECT(vss_search_batch_filtered_groups_device(h, d_q, NQ, K, EF, d_table, t.n_groups, t.n_bits, d_groups, grouped_blocking.ids,
	                                               grouped_blocking.dist, grouped_blocking.counts) == VSS_OK);
	EXPECT(vss_search_batch_filtered_groups_device_begin(h, 3, d_q, NQ, K, EF, d_table, t.n_groups, t.n_bits, d_groups, grouped.ids,
	                                                     grouped.dist, grouped.counts) == VSS_OK);
	EXPECT(vss_search_batch_end(h, 3) == VSS_OK);
	const Results expected = grouped_blocking.Fetch();
	EXPECT(grouped.Fetch() == expected);
	idx_t returned = 0;
	for (idx_t q = 0; q != NQ; ++q) {
		for (idx_t j = 0; j != expected.counts[q]; ++j)
			EXPECT(Live((uint64_t)expected.ids[q * K + j]) && t.Admits(t.group_of[q], expected.ids[q * K + j]));
		returned += expected.counts[q];
	}
	EXPECT(returned > NQ * K / 2);

	// four chunks, one launch: chunk b under its own table — chunks 0 and 2 the tenants' (with each chunk's own slice of the group
	// numbers), chunk 1 a table of ONE bitmap without group numbers, chunk 3 the first two tenants with group numbers 0 / 1 / 2,
	// the last of which the table does not hold
	std::vector<uint32_t> three(PER_CHUNK);
	for (idx_t q = 0; q != PER_CHUNK; ++q)
		three[q] = (uint32_t)(q % 3);
	const uint32_t *d_three = Device(three.data(), PER_CHUNK);
	const float *qs[CHUNKS];
	const uint64_t *tables[CHUNKS] = {d_table, d_table + 2 * t.words, d_table, d_table};
	const uint64_t n_groups[CHUNKS] = {t.n_groups, 1, t.n_groups, 2};
	const uint32_t *groups[CHUNKS] = {d_groups, nullptr, d_groups + 2 * PER_CHUNK, d_three};
	std::vector<uint32_t> zeros(PER_CHUNK, 0);
	const uint32_t *d_zeros = Device(zeros.data(), PER_CHUNK);
	std::vector<Cells> alone, together;
	row_t *out_ids[CHUNKS];
	float *out_dist[CHUNKS];
	uint32_t *out_counts[CHUNKS];
	uint64_t work[2] = {0, 0};
	for (idx_t b = 0; b != CHUNKS; ++b) {
		qs[b] = d_q + b * PER_CHUNK * DIM;
		alone.emplace_back(PER_CHUNK), together.emplace_back(PER_CHUNK);
		EXPECT(vss_search_batch_filtered_groups_device(h, qs[b], PER_CHUNK, K, EF, tables[b], n_groups[b], t.n_bits,
		                                               groups[b] ? groups[b] : d_zeros, alone[b].ids, alone[b].dist,
		                                               alone[b].counts) == VSS_OK);
		uint64_t stats[4];
		EXPECT(vss_last_search_stats(h, stats) == VSS_OK);
		work[0] += stats[0], work[1] += stats[1];
		out_ids[b] = together[b].ids, out_dist[b] = together[b].dist, out_counts[b] = together[b].counts;
	}
	EXPECT(vss_search_multi_filtered_device_begin(h, 1, CHUNKS, qs, PER_CHUNK, K, EF, tables, n_groups, t.n_bits, groups, out_ids,
	                                              out_dist, out_counts) == VSS_OK);
	EXPECT(vss_search_batch_end(h, 1) == VSS_OK);
	uint64_t stats[4];
	EXPECT(vss_last_search_stats(h, stats) == VSS_OK);
	EXPECT(stats[0] == work[0] && stats[1] == work[1] && stats[2] == NQ);
	for (idx_t b = 0; b != CHUNKS; ++b)
		EXPECT(together[b].Fetch() == alone[b].Fetch());
	const Results unknown = together[3].Fetch();
	for (idx_t q = 2; q < PER_CHUNK; q += 3)
		EXPECT(unknown.counts[q] == 0 && unknown.ids[q * K] == -1 && std::isinf(unknown.dist[q * K]));
	// refused with the batch's number, nothing written
	Cells untouched(PER_CHUNK);
	out_ids[0] = untouched.ids, out_dist[0] = untouched.dist, out_counts[0] = untouched.counts;
	const uint64_t no_groups[CHUNKS] = {t.n_groups, 1, 0, 2};
	EXPECT(vss_search_multi_filtered_device_begin(h, 1, CHUNKS, qs, PER_CHUNK, K, EF, tables, no_groups, t.n_bits, groups, out_ids,
	                                              out_dist, out_counts) == VSS_ERROR);
	EXPECT(std::strstr(vss_last_error(h), "batch 2 needs at least one group"));
	EXPECT(vss_search_batch_end(h, 1) == VSS_OK); // (nothing pending)
	EXPECT(untouched.Fetch() == Results(PER_CHUNK));
	std::printf("one index: three contexts in flight, the grouped form and %zu chunks in one launch equal the blocking calls\n",
	            (size_t)CHUNKS);
}

void Sharded(const FilterGroupTables &t, const std::vector<int> &devices, std::unique_ptr<ShardedHNSWIndex> &holder) {
	ShardedHNSWIndex &index = BuildSharded(holder, DIM, vecs, ids, dead, devices);

	// one bitmap: tenant 1's
	std::vector<Results> parts;
	for (idx_t g = 0; g != index.ShardCount(); ++g) {
		parts.emplace_back(NQ);
		EXPECT(vss_search_batch_filtered(index.ShardHandle(g), queries.data(), NQ, K, EF, t.Group(1), t.n_bits, parts[g].ids.data(),
		                                 parts[g].dist.data(), parts[g].counts.data()) == VSS_OK);
	}
	Results one(NQ);
	index.SearchBatchFiltered(queries.data(), NQ, K, EF, t.Group(1), t.n_bits, one.ids.data(), one.dist.data(), one.counts.data());
	EXPECT(one == Merge(parts, NQ));
	// one predicate per query
	parts.clear();
	for (idx_t g = 0; g != index.ShardCount(); ++g) {
		parts.emplace_back(NQ);
		EXPECT(vss_search_batch_filtered_groups(index.ShardHandle(g), queries.data(), NQ, K, EF, t.allowed.data(), t.n_groups,
		                                        t.n_bits, t.group_of.data(), parts[g].ids.data(), parts[g].dist.data(),
		                                        parts[g].counts.data()) == VSS_OK);
	}
	Results grouped(NQ);
	index.SearchBatchFilteredGroups(queries.data(), NQ, K, EF, t.allowed.data(), t.n_groups, t.n_bits, t.group_of.data(),
	                                grouped.ids.data(), grouped.dist.data(), grouped.counts.data());
	EXPECT(grouped == Merge(parts, NQ));
	idx_t returned = 0;
	for (idx_t q = 0; q != NQ; ++q)
		returned += grouped.counts[q];
	EXPECT(returned > NQ * K / 2);
	// a refused probe (a query of an unknown group) leaves no context in flight: the next probe answers as before
	std::vector<uint32_t> bad = t.group_of;
	bad[7] = (uint32_t)t.n_groups;
	bool threw = false;
	try {
		Results refused(NQ);
		index.SearchBatchFilteredGroups(queries.data(), NQ, K, EF, t.allowed.data(), t.n_groups, t.n_bits, bad.data(),
		                                refused.ids.data(), refused.dist.data(), refused.counts.data());
	} catch (const std::exception &) {
		threw = true;
	}
	EXPECT(threw);
	Results again(NQ);
	index.SearchBatchFiltered(queries.data(), NQ, K, EF, t.Group(1), t.n_bits, again.ids.data(), again.dist.data(),
	                          again.counts.data());
	EXPECT(again == one);
	std::printf("%zu shard(s), exchange %s: both filtered probes equal the merge of per-shard blocking calls\n", devices.size(),
	            index.ExchangeKind());
}

} // namespace

int main() {
	ClusteredData(20260926, DIM, N, NQ, 64, 0.3f, vecs, queries);
	for (idx_t i = 0; i != N; ++i)
		ids[i] = (row_t)i;
	for (idx_t i = 0; i != N; ++i)
		if (!Live(i))
			dead.push_back((row_t)i);
	// four tenants and one all-ones group whose padding bits are set; the bitmaps admit deleted rows too
	const FilterGroupTables t = TenantTables(4, N_BITS, NQ, [](uint64_t) { return true; });
	try {
		SingleIndex(t);
		Sharded(t, {0}, sharded_p[0]);
		Sharded(t, {0, 0}, sharded_p[1]);
	} catch (const std::exception &e) {
		std::fprintf(stderr, "EXCEPTION: %s\n", e.what());
		std::fflush(nullptr);
		std::_Exit(1);
	}
	std::printf("filter probes ok\n");
	std::fflush(nullptr);
	std::_Exit(0);
}
