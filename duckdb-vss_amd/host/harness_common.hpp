// harness_common.hpp — what the GPU harnesses of this directory share: the check macro, the seeded clustered data, the cells a
// search answers into, the CPU merge of per-shard answers, and the bulk build of both host classes.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <utility>
#include <vector>

#include "sharded_index.hpp"

// the first failed check ends the process with a non-zero exit code, without unwinding
#define EXPECT(cond)                                                                                                   \
	do {                                                                                                               \
		if (!(cond)) {                                                                                                 \
			std::fprintf(stderr, "CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                               \
			std::fflush(nullptr);                                                                                      \
			std::_Exit(1);                                                                                             \
		}                                                                                                              \
	} while (0)

namespace vss_host {

// `clusters` seeded Gaussian centres, then `rows` vectors and `n_queries` queries, each a centre picked at random plus `noise`
// times a Gaussian: one generator, drawn from in that order, so a seed names the data bit for bit
inline void ClusteredData(uint32_t seed, idx_t dim, idx_t rows, idx_t n_queries, idx_t clusters, float noise, std::vector<float> &vecs,
                          std::vector<float> &queries) {
	std::mt19937 rng(seed);
	std::normal_distribution<float> gauss(0.f, 1.f);
	std::vector<float> centres(clusters * dim);
	for (auto &c : centres)
		c = gauss(rng);
	auto draw = [&](float *dst) {
		const size_t c = rng() % clusters;
		for (idx_t d = 0; d != dim; ++d)
			dst[d] = centres[c * dim + d] + noise * gauss(rng);
	};
	vecs.resize(rows * dim), queries.resize(n_queries * dim);
	for (idx_t i = 0; i != rows; ++i)
		draw(&vecs[i * dim]);
	for (idx_t i = 0; i != n_queries; ++i)
		draw(&queries[i * dim]);
}

// The cells of one batch of answers, K per query, pre-filled so that a cell nobody wrote shows.  NQ: the batch a harness that
// has one size only constructs without saying so.  route is compared too: a harness that asks for no routes leaves the fill.
template <idx_t K, idx_t NQ = 0>
struct ResultsOf {
	std::vector<row_t> ids;
	std::vector<float> dist;
	std::vector<uint32_t> counts;
	std::vector<uint8_t> route;
	explicit ResultsOf(idx_t nq = NQ) : ids(nq * K, -2), dist(nq * K, -1.f), counts(nq, 77), route(nq, 9) {
	}
	bool SameAnswers(const ResultsOf &o) const { // (distances by their bits)
		return ids == o.ids && counts == o.counts && dist.size() == o.dist.size() &&
		       !std::memcmp(dist.data(), o.dist.data(), dist.size() * sizeof(float));
	}
	bool operator==(const ResultsOf &o) const {
		return SameAnswers(o) && route == o.route;
	}
};

// the union of the shards' answers by ascending (distance, row id), the K best per query: what vss_merge_topk_device computes
template <idx_t K, idx_t NQ>
ResultsOf<K, NQ> Merge(const std::vector<ResultsOf<K, NQ>> &parts, idx_t nq) {
	ResultsOf<K, NQ> merged(nq);
	for (idx_t q = 0; q != nq; ++q) {
		std::vector<std::pair<float, row_t>> all;
		for (auto &p : parts)
			for (idx_t j = 0; j != p.counts[q]; ++j)
				all.emplace_back(p.dist[q * K + j], p.ids[q * K + j]);
		std::sort(all.begin(), all.end());
		const idx_t n = std::min<idx_t>(all.size(), K);
		for (idx_t j = 0; j != K; ++j) {
			merged.ids[q * K + j] = j < n ? all[j].second : -1;
			merged.dist[q * K + j] = j < n ? all[j].first : INFINITY;
		}
		merged.counts[q] = (uint32_t)n;
	}
	return merged;
}

// The bulk build every harness starts from, l2sq: ids.size() rows appended in STANDARD_VECTOR_SIZE chunks — per_chunk(first, rows)
// after each —, finalized, `dead` deleted.  The holders live outside main's try block: an exception ends the process before any
// destructor runs.
template <class Index, class PerChunk>
void AppendInChunks(Index &index, idx_t dim, const std::vector<float> &vecs, const std::vector<row_t> &ids, PerChunk per_chunk) {
	for (idx_t c = 0; c < ids.size(); c += STANDARD_VECTOR_SIZE) {
		const idx_t cnt = std::min<idx_t>(STANDARD_VECTOR_SIZE, ids.size() - c);
		index.BulkAppendChunk(vecs.data() + c * dim, ids.data() + c, nullptr, cnt);
		per_chunk(c, cnt);
	}
	index.BulkFinalize();
}
template <class PerChunk>
HNSWIndex &BuildSingle(std::unique_ptr<HNSWIndex> &holder, idx_t dim, const std::vector<float> &vecs, const std::vector<row_t> &ids,
                       const std::vector<row_t> &dead, PerChunk per_chunk) {
	holder = std::make_unique<HNSWIndex>(dim, OptionMap {{"metric", OptionValue::String("l2sq")}}, ids.size());
	holder->BulkReserve(ids.size(), 8);
	AppendInChunks(*holder, dim, vecs, ids, per_chunk);
	holder->Delete(dead.data(), dead.size());
	return *holder;
}
inline HNSWIndex &BuildSingle(std::unique_ptr<HNSWIndex> &holder, idx_t dim, const std::vector<float> &vecs, const std::vector<row_t> &ids,
                              const std::vector<row_t> &dead) {
	return BuildSingle(holder, dim, vecs, ids, dead, [](idx_t, idx_t) {});
}
// ... and the same rows over the shards on `devices`
inline ShardedHNSWIndex &BuildSharded(std::unique_ptr<ShardedHNSWIndex> &holder, idx_t dim, const std::vector<float> &vecs,
                                      const std::vector<row_t> &ids, const std::vector<row_t> &dead, const std::vector<int> &devices) {
	holder = std::make_unique<ShardedHNSWIndex>(dim, OptionMap {{"metric", OptionValue::String("l2sq")}}, ids.size(), devices);
	holder->BulkReserve(8);
	AppendInChunks(*holder, dim, vecs, ids, [](idx_t, idx_t) {});
	EXPECT(holder->Delete(dead.data(), dead.size()) == dead.size());
	return *holder;
}

} // namespace vss_host
