// label_pipeline_harness.cpp — label predicates in the pipelined and multi-batch launches (vss_search_by_label_device_begin,
// vss_search_multi_by_label_device_begin) through both host classes.
//     ./label_pipeline_harness
//   1. vss_host::ShardedHNSWIndex with 2 shards co-resident on device 0, every shard holding the whole columns: in mode
//      VSS_BY_LABEL_GRAPH the six SearchBatchByLabel* methods — which start every shard through the _begin call and then end every
//      shard — against what they did before: the form's BLOCKING _device call on every shard's own handle, one shard after the
//      other, called here directly, merged on the CPU by (distance, row id).  Row ids, distance bits, counts; shard_routes all 0.
//   2. vss_host::HNSWIndex on device 0: ExecuteMultiScanChunksByLabel — three join chunks with a predicate each in one launch on
//      context 1 — against the form's per-chunk method in mode graph, chunk by chunk: counts and the row ids appended.
// Data: 64 seeded Gaussian clusters, dim 32, l2sq, 4000 rows with id = position, every ninth row deleted; 96 queries, k = 10,
// ef_search 64.  Column 0 (a tenant, 32 bits) for ids below 3997: (id * 7919) % 10, every 97th id none; column 1 (a group, 32 bits)
// for ids below 3900: (id * 31) % 7; column 3 (a timestamp, 64 BITS) for ids below 3500: BASE + (id * 104729) % 1000, every 89th id
// VSS_NO_LABEL64.  Query q's predicate changes with q, so the three chunks differ; every twelfth admits nothing.  The first failed
// check or exception ends the process with a non-zero exit code.  Prints "label pipeline ok" last.  Needs a MI355X.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <hip/hip_runtime.h>

#include "harness_common.hpp"

using namespace vss_host;

namespace {

constexpr idx_t DIM = 32, N = 4000, NQ = 96, K = 10, EF = 64, TENANTS = N - 3, GROUPS = 3900, STAMPS = 3500, W = 3, CHUNKS = 3,
                PER_CHUNK = NQ / CHUNKS;
constexpr uint64_t BASE = (1ull << 63) + 1000000000000000ull;
const uint32_t BOX_COLUMNS[2] = {0, 1}, BOX64_COLUMNS[2] = {1, 3}, RANGE_COLUMNS[1] = {3};
constexpr uint32_t SET_COLUMN = 1;

using Results = ResultsOf<K, NQ>;

std::vector<float> vecs(N *DIM), queries(NQ *DIM);
std::vector<row_t> ids(N), dead;
std::vector<uint32_t> tenant(TENANTS), group(GROUPS);
std::vector<uint64_t> stamp(STAMPS);
// the per-query words of the six forms
std::vector<uint32_t> want(NQ), lo(NQ), hi(NQ), sets(NQ *W), box_lo(NQ * 2), box_hi(NQ * 2);
std::vector<uint64_t> box64_lo(NQ * 2), box64_hi(NQ * 2), sets64(NQ *W), range_lo(NQ), range_hi(NQ);

std::unique_ptr<HNSWIndex> single_p;
std::unique_ptr<ShardedHNSWIndex> sharded_p;

#define HIP_OK(call) EXPECT((call) == hipSuccess)

// n cells on device 0: uploaded from the host, or answered into and read back
template <class T>
struct Dev {
	T *p = nullptr;
	size_t n;
	explicit Dev(size_t cells) : n(cells) {
		HIP_OK(hipSetDevice(0));
		HIP_OK(hipMalloc((void **)&p, std::max<size_t>(n, 1) * sizeof(T)));
	}
	explicit Dev(const std::vector<T> &host) : Dev(host.size()) {
		HIP_OK(hipMemcpy(p, host.data(), n * sizeof(T), hipMemcpyHostToDevice));
	}
	Dev(const Dev &) = delete;
	~Dev() {
		(void)hipFree(p);
	}
	void Read(T *host) const {
		HIP_OK(hipMemcpy(host, p, n * sizeof(T), hipMemcpyDeviceToHost));
	}
};

enum Form { EQ, RANGE, SET, BOX, BOX64, SET_BOX, FORMS };
const char *const FORM_NAME[FORMS] = {"eq", "range", "set", "box", "box64", "set box"};

// every form's words on device 0
struct DeviceWords {
	Dev<float> q {queries};
	Dev<uint32_t> want {::want}, lo {::lo}, hi {::hi}, sets {::sets}, box_lo {::box_lo}, box_hi {::box_hi};
	Dev<uint64_t> box64_lo {::box64_lo}, box64_hi {::box64_hi}, sets64 {::sets64}, range_lo {::range_lo}, range_hi {::range_hi};
};

// the form's blocking _device call in mode graph, as the sharded methods made it per shard
Results Blocking(vss_index *h, Form form, const DeviceWords &d) {
	Dev<row_t> keys(NQ * K);
	Dev<float> dist(NQ * K);
	Dev<uint32_t> counts(NQ);
	Dev<uint8_t> route(NQ);
	const int mode = VSS_BY_LABEL_GRAPH;
	int rc = VSS_ERROR;
	if (form == EQ)
		rc = vss_search_batch_by_label_device(h, d.q.p, NQ, K, EF, d.want.p, mode, 0, keys.p, dist.p, counts.p, route.p);
	else if (form == RANGE)
		rc = vss_search_batch_by_label_range_device(h, d.q.p, NQ, K, EF, d.lo.p, d.hi.p, mode, 0, keys.p, dist.p, counts.p, route.p);
	else if (form == SET)
		rc = vss_search_batch_by_label_set_device(h, d.q.p, NQ, K, EF, d.sets.p, W, mode, 0, keys.p, dist.p, counts.p, route.p);
	else if (form == BOX)
		rc = vss_search_batch_by_label_box_device(h, d.q.p, NQ, K, EF, BOX_COLUMNS, 2, d.box_lo.p, d.box_hi.p, mode, 0, keys.p, dist.p, counts.p,
		                                          route.p);
	else if (form == BOX64)
		rc = vss_search_batch_by_label_box64_device(h, d.q.p, NQ, K, EF, BOX64_COLUMNS, 2, d.box64_lo.p, d.box64_hi.p, mode, 0, keys.p, dist.p,
		                                            counts.p, route.p);
	else
		rc = vss_search_batch_by_label_set_box_device(h, d.q.p, NQ, K, EF, SET_COLUMN, d.sets64.p, W, RANGE_COLUMNS, 1, d.range_lo.p, d.range_hi.p,
		                                              mode, 0, keys.p, dist.p, counts.p, route.p);
	if (rc != VSS_OK)
		std::fprintf(stderr, "%s: %s\n", FORM_NAME[form], vss_last_error(h));
	EXPECT(rc == VSS_OK);
	Results r;
	keys.Read(r.ids.data()), dist.Read(r.dist.data()), counts.Read(r.counts.data()), route.Read(r.route.data());
	return r;
}

void Sharded(const std::vector<int> &devices) {
	ShardedHNSWIndex &index = BuildSharded(sharded_p, DIM, vecs, ids, dead, devices);
	index.SetLabels(0, tenant.data(), TENANTS);
	index.SetLabelColumn(1, 0, group.data(), GROUPS);
	index.SetLabelColumn64(3, 0, stamp.data(), STAMPS);
	EXPECT(index.ShardCount() == devices.size());
	const DeviceWords d;
	for (int form = 0; form != FORMS; ++form) {
		Results got;
		std::vector<uint8_t> routes;
		const int mode = VSS_BY_LABEL_GRAPH;
		if (form == EQ)
			index.SearchBatchByLabel(queries.data(), NQ, K, EF, want.data(), mode, 0, got.ids.data(), got.dist.data(), got.counts.data(), &routes);
		else if (form == RANGE)
			index.SearchBatchByLabelRange(queries.data(), NQ, K, EF, lo.data(), hi.data(), mode, 0, got.ids.data(), got.dist.data(),
			                              got.counts.data(), &routes);
		else if (form == SET)
			index.SearchBatchByLabelSet(queries.data(), NQ, K, EF, sets.data(), W, mode, 0, got.ids.data(), got.dist.data(), got.counts.data(),
			                            &routes);
		else if (form == BOX)
			index.SearchBatchByLabelBox(queries.data(), NQ, K, EF, BOX_COLUMNS, 2, box_lo.data(), box_hi.data(), mode, 0, got.ids.data(),
			                            got.dist.data(), got.counts.data(), &routes);
		else if (form == BOX64)
			index.SearchBatchByLabelBox64(queries.data(), NQ, K, EF, BOX64_COLUMNS, 2, box64_lo.data(), box64_hi.data(), mode, 0, got.ids.data(),
			                              got.dist.data(), got.counts.data(), &routes);
		else
			index.SearchBatchByLabelSetBox(queries.data(), NQ, K, EF, SET_COLUMN, sets64.data(), W, RANGE_COLUMNS, 1, range_lo.data(),
			                               range_hi.data(), mode, 0, got.ids.data(), got.dist.data(), got.counts.data(), &routes);
		EXPECT(routes.size() == devices.size() * NQ && std::count(routes.begin(), routes.end(), 0) == (long)routes.size());
		std::vector<Results> per_shard;
		for (idx_t g = 0; g != devices.size(); ++g) {
			per_shard.push_back(Blocking(index.ShardHandle(g), (Form)form, d));
			EXPECT(std::count(per_shard.back().route.begin(), per_shard.back().route.end(), 0) == (long)NQ);
		}
		EXPECT(got.SameAnswers(Merge(per_shard, NQ)));
		idx_t found = 0, none = 0;
		for (idx_t q = 0; q != NQ; ++q)
			found += got.counts[q], none += got.counts[q] == 0;
		EXPECT(found > NQ && none >= NQ / 12); // neither nothing nor everything
		std::printf("%zu shards, %s: %zu rows, %zu empty answers, equal to the merge of the blocking per-shard calls\n", devices.size(),
		            FORM_NAME[form], (size_t)found, (size_t)none);
	}
}

void SingleIndex() {
	HNSWIndex &index = BuildSingle(single_p, DIM, vecs, ids, dead);
	index.SetLabels(0, tenant.data(), TENANTS);
	index.SetLabelColumn(1, 0, group.data(), GROUPS);
	index.SetLabelColumn64(3, 0, stamp.data(), STAMPS);
	const DeviceWords d;
	for (int form = 0; form != FORMS; ++form) {
		Dev<row_t> keys(NQ * K);
		Dev<uint32_t> counts(NQ);
		const float *chunk_q[CHUNKS];
		row_t *chunk_keys[CHUNKS];
		float *chunk_dist[CHUNKS] = {};
		uint32_t *chunk_counts[CHUNKS];
		vss_label_predicate preds[CHUNKS] = {};
		for (idx_t b = 0; b != CHUNKS; ++b) {
			const idx_t at = b * PER_CHUNK;
			chunk_q[b] = d.q.p + at * DIM, chunk_keys[b] = keys.p + at * K, chunk_counts[b] = counts.p + at;
			vss_label_predicate &p = preds[b];
			if (form == EQ) {
				p.kind = VSS_LABEL_EQ, p.d_want = d.want.p + at;
			} else if (form == RANGE) {
				p.kind = VSS_LABEL_RANGE, p.d_lo = d.lo.p + at, p.d_hi = d.hi.p + at;
			} else if (form == SET) {
				p.kind = VSS_LABEL_SET, p.set_width = W, p.d_sets = d.sets.p + at * W;
			} else if (form == BOX) {
				p.kind = VSS_LABEL_BOX, p.n_columns = 2, p.columns[0] = BOX_COLUMNS[0], p.columns[1] = BOX_COLUMNS[1];
				p.d_lo = d.box_lo.p + at * 2, p.d_hi = d.box_hi.p + at * 2;
			} else if (form == BOX64) {
				p.kind = VSS_LABEL_BOX64, p.n_columns = 2, p.columns[0] = BOX64_COLUMNS[0], p.columns[1] = BOX64_COLUMNS[1];
				p.d_lo = d.box64_lo.p + at * 2, p.d_hi = d.box64_hi.p + at * 2;
			} else {
				p.kind = VSS_LABEL_SET_BOX, p.set_column = SET_COLUMN, p.set_width = W, p.n_columns = 1, p.columns[0] = RANGE_COLUMNS[0];
				p.d_sets = d.sets64.p + at * W, p.d_lo = d.range_lo.p + at, p.d_hi = d.range_hi.p + at;
			}
		}
		auto state = index.InitializeMultiScan(EF);
		index.ExecuteMultiScanChunksByLabel(*state, 1, CHUNKS, chunk_q, PER_CHUNK, K, preds, chunk_keys, chunk_dist, chunk_counts);
		std::vector<row_t> got_ids(NQ * K);
		std::vector<uint32_t> got_counts(NQ);
		keys.Read(got_ids.data()), counts.Read(got_counts.data());
		idx_t found = 0;
		for (idx_t b = 0; b != CHUNKS; ++b) {
			const idx_t at = b * PER_CHUNK;
			auto chunk_state = index.InitializeMultiScan(EF);
			std::vector<uint32_t> chunk_counts_h;
			const float *q = queries.data() + at * DIM;
			const int mode = VSS_BY_LABEL_GRAPH;
			if (form == EQ)
				index.ExecuteMultiScanBatchByLabel(*chunk_state, q, PER_CHUNK, K, want.data() + at, &chunk_counts_h, nullptr, mode);
			else if (form == RANGE)
				index.ExecuteMultiScanBatchByLabelRange(*chunk_state, q, PER_CHUNK, K, lo.data() + at, hi.data() + at, &chunk_counts_h, nullptr, mode);
			else if (form == SET)
				index.ExecuteMultiScanBatchByLabelSet(*chunk_state, q, PER_CHUNK, K, sets.data() + at * W, W, &chunk_counts_h, nullptr, mode);
			else if (form == BOX)
				index.ExecuteMultiScanBatchByLabelBox(*chunk_state, q, PER_CHUNK, K, BOX_COLUMNS, 2, box_lo.data() + at * 2, box_hi.data() + at * 2,
				                                      &chunk_counts_h, nullptr, mode);
			else if (form == BOX64)
				index.ExecuteMultiScanBatchByLabelBox64(*chunk_state, q, PER_CHUNK, K, BOX64_COLUMNS, 2, box64_lo.data() + at * 2,
				                                        box64_hi.data() + at * 2, &chunk_counts_h, nullptr, mode);
			else
				index.ExecuteMultiScanBatchByLabelSetBox(*chunk_state, q, PER_CHUNK, K, SET_COLUMN, sets64.data() + at * W, W, RANGE_COLUMNS, 1,
				                                         range_lo.data() + at, range_hi.data() + at, &chunk_counts_h, nullptr, mode);
			std::vector<row_t> appended;
			for (idx_t i = 0; i != PER_CHUNK; ++i) {
				EXPECT(got_counts[at + i] == chunk_counts_h[i]);
				appended.insert(appended.end(), got_ids.begin() + (at + i) * K, got_ids.begin() + (at + i) * K + got_counts[at + i]);
				for (idx_t j = got_counts[at + i]; j != K; ++j)
					EXPECT(got_ids[(at + i) * K + j] == -1);
			}
			EXPECT(appended == index.GetMultiScanResult(*chunk_state));
			found += appended.size();
		}
		EXPECT(found > NQ);
		std::printf("one index, %s: %zu chunks in one launch, %zu rows, equal to the per-chunk calls\n", FORM_NAME[form], (size_t)CHUNKS,
		            (size_t)found);
	}
}

} // namespace

int main() {
	ClusteredData(20261022, DIM, N, NQ, 64, 0.3f, vecs, queries);
	for (idx_t i = 0; i != N; ++i)
		ids[i] = (row_t)i;
	for (idx_t i = 0; i != N; ++i)
		if (i % 9 == 4)
			dead.push_back((row_t)i);
	// the columns label deleted rows too (they know nothing of tombstones): the engine excludes them
	for (idx_t i = 0; i != TENANTS; ++i)
		tenant[i] = i % 97 == 5 ? VSS_NO_LABEL : (uint32_t)((i * 7919) % 10);
	for (idx_t i = 0; i != GROUPS; ++i)
		group[i] = (uint32_t)((i * 31) % 7);
	for (idx_t i = 0; i != STAMPS; ++i)
		stamp[i] = i % 89 == 7 ? VSS_NO_LABEL64 : BASE + (i * 104729) % 1000;
	for (idx_t q = 0; q != NQ; ++q) {
		const bool none = q % 12 == 7; // this query's predicate admits nothing, in every form
		const uint32_t t = (uint32_t)(q % 10), g = (uint32_t)(q % 7);
		const uint64_t since = BASE + (q * 37) % 600;
		want[q] = none ? VSS_NO_LABEL : t;
		lo[q] = none ? 5 : t, hi[q] = none ? 4 : std::min<uint32_t>(t + q % 3, 9);
		sets[q * W] = none ? VSS_NO_LABEL : t, sets[q * W + 1] = none ? VSS_NO_LABEL : (t + 3) % 10, sets[q * W + 2] = VSS_NO_LABEL;
		box_lo[q * 2] = t, box_hi[q * 2] = none ? 0xFFFFFFFFu : t + 2; // (column 0: no upper bound still rejects the unlabelled rows)
		box_lo[q * 2 + 1] = none ? 7 : 0, box_hi[q * 2 + 1] = none ? 6 : g + 2;
		box64_lo[q * 2] = g ? g - 1 : 0, box64_hi[q * 2] = g + 1;
		box64_lo[q * 2 + 1] = since, box64_hi[q * 2 + 1] = none ? since - 1 : VSS_NO_LABEL64;
		sets64[q * W] = none ? VSS_NO_LABEL64 : g, sets64[q * W + 1] = VSS_NO_LABEL64, sets64[q * W + 2] = none ? (1ull << 32) + g : (g + 2) % 7;
		range_lo[q] = since, range_hi[q] = q % 5 ? VSS_NO_LABEL64 : since + 300;
	}
	try {
		Sharded({0, 0});
		SingleIndex();
	} catch (const std::exception &e) {
		std::fprintf(stderr, "EXCEPTION: %s\n", e.what());
		std::fflush(nullptr);
		std::_Exit(1);
	}
	std::printf("label pipeline ok\n");
	std::fflush(nullptr);
	std::_Exit(0);
}
