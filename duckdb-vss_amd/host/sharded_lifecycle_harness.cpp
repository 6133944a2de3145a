// sharded_lifecycle_harness.cpp — drives vss_host::ShardedHNSWIndex through what DuckDB does to an index after CREATE INDEX
// (BASELINE configs[4] on shards): bulk build, GetStats, exact probe, inserts after the build (Construct), Delete, filtered
// probe, checkpoint (PersistToBlocks) and reload (LoadFromBlocks), Compact, and loads that must be refused.
//     ./sharded_lifecycle_harness [device ...]
// Without arguments: three shards on device 0 (peer-copy exchange); `./sharded_lifecycle_harness 0` = one shard, RCCL path.
// Data as in sharded_harness.cpp: 64 seeded Gaussian clusters, dim 32, l2sq, 6001 built rows with id = position, 257 queries,
// k = 10, ef 128.  The first failed check or exception ends the process with a non-zero exit code, without unwinding (nothing
// more is started on a device).  Prints "sharded lifecycle ok" and the exchange kind last.  Needs a MI355X.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <random>
#include <set>

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

constexpr idx_t DIM = 32, NQ = 257, K = 10, EF = 128;
constexpr idx_t N_BUILT = 6001, N_INSERTED = 2 * 2048 + 100, N_LATE = 10, N_ALL = N_BUILT + N_INSERTED + N_LATE;

using Answers = std::vector<std::pair<float, row_t>>;

struct Results {
	std::vector<row_t> ids;
	std::vector<float> dist;
	std::vector<uint32_t> counts;
	explicit Results(idx_t nq) : ids(nq * K), dist(nq * K), counts(nq) {
	}
};

std::vector<float> vecs(N_ALL *DIM), queries(NQ *DIM);
std::vector<char> live(N_ALL, 0);
std::set<row_t> never; // NULL rows and deleted rows: no probe may return them

float L2(const float *a, const float *b) {
	float s = 0;
	for (idx_t d = 0; d != DIM; ++d)
		s += (a[d] - b[d]) * (a[d] - b[d]);
	return s;
}

// host brute force over the live rows `admit` lets through: the k + 1 best by (distance, row id)
Answers Truth(const float *q, const std::function<bool(row_t)> &admit) {
	Answers all;
	for (idx_t i = 0; i != N_ALL; ++i)
		if (live[i] && admit((row_t)i))
			all.push_back({L2(q, &vecs[i * DIM]), (row_t)i});
	const size_t keep = std::min<size_t>(K + 1, all.size());
	std::partial_sort(all.begin(), all.begin() + keep, all.end());
	all.resize(keep);
	return all;
}

void ExpectNoneOf(const Results &r, const std::set<row_t> &banned) {
	for (row_t id : r.ids)
		EXPECT(!banned.count(id));
}

// SearchExactBatch == the host's brute force over all live rows: the same ids wherever the host's k-th and (k+1)-th
// distances differ, distances within 1e-5 relative (sharded_harness.cpp's tolerance), ascending, k rows per query
Results ExpectExact(ShardedHNSWIndex &index) {
	Results r(NQ);
	index.SearchExactBatch(queries.data(), NQ, K, r.ids.data(), r.dist.data(), r.counts.data());
	ExpectNoneOf(r, never);
	for (idx_t q = 0; q != NQ; ++q) {
		EXPECT(r.counts[q] == K);
		const Answers truth = Truth(&queries[q * DIM], [](row_t) { return true; });
		EXPECT(truth.size() == K + 1);
		std::set<row_t> want, got;
		for (idx_t j = 0; j != K; ++j) {
			want.insert(truth[j].second);
			got.insert(r.ids[q * K + j]);
			if (j)
				EXPECT(r.dist[q * K + j - 1] <= r.dist[q * K + j]);
			EXPECT(std::fabs(r.dist[q * K + j] - truth[j].first) <= 1e-5f * std::max(truth[j].first, 1e-6f));
		}
		EXPECT(got.size() == K);
		if (truth[K - 1].first != truth[K].first)
			EXPECT(got == want);
	}
	return r;
}

bool SameStats(const HNSWIndexStats &a, const HNSWIndexStats &b) {
	if (a.max_level != b.max_level || a.count != b.count || a.level_stats.size() != b.level_stats.size())
		return false;
	for (size_t l = 0; l != a.level_stats.size(); ++l)
		if (a.level_stats[l].nodes != b.level_stats[l].nodes || a.level_stats[l].edges != b.level_stats[l].edges ||
		    a.level_stats[l].max_edges != b.level_stats[l].max_edges ||
		    a.level_stats[l].allocated_bytes != b.level_stats[l].allocated_bytes)
			return false;
	return true;
}

std::vector<uint8_t> Concatenate(const std::vector<std::vector<uint8_t>> &blocks, idx_t payload) {
	std::vector<uint8_t> all;
	for (size_t b = 0; b != blocks.size(); ++b) {
		EXPECT(blocks[b].size() <= payload && !blocks[b].empty());
		EXPECT(b + 1 == blocks.size() || blocks[b].size() == payload); // only the last block may be short
		all.insert(all.end(), blocks[b].begin(), blocks[b].end());
	}
	return all;
}

// the three holders live outside main's try block: an exception ends the process before any destructor runs
std::unique_ptr<ShardedHNSWIndex> index_p, loaded_p, other_p;

int Run(const std::vector<int> &devices) {
	const idx_t G = devices.size();
	const OptionMap options = {{"metric", OptionValue::String("l2sq")}};

	// clustered data (seeded): the built rows and the queries are sharded_harness.cpp's, the inserted rows follow
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
	for (idx_t i = 0; i != N_BUILT; ++i)
		draw(&vecs[i * DIM]);
	for (idx_t i = 0; i != NQ; ++i)
		draw(&queries[i * DIM]);
	for (idx_t i = N_BUILT; i != N_ALL; ++i)
		draw(&vecs[i * DIM]);
	std::vector<row_t> ids(N_ALL);
	for (idx_t i = 0; i != N_ALL; ++i)
		ids[i] = (row_t)i;

	// ---- 1. build
	index_p = std::make_unique<ShardedHNSWIndex>(DIM, options, N_BUILT, devices);
	ShardedHNSWIndex &index = *index_p;
	EXPECT(index.ShardCount() == G && index.BuildRows() == N_BUILT);
	std::printf("exchange: %s\n", index.ExchangeKind());
	index.BulkReserve(8);
	for (idx_t c = 0; c < N_BUILT; c += STANDARD_VECTOR_SIZE) {
		const idx_t cnt = std::min<idx_t>(STANDARD_VECTOR_SIZE, N_BUILT - c);
		index.BulkAppendChunk(vecs.data() + c * DIM, ids.data() + c, nullptr, cnt);
	}
	index.BulkFinalize();
	for (idx_t i = 0; i != N_BUILT; ++i)
		live[i] = 1;
	{
		const auto stats = index.GetStats();
		EXPECT(stats->count == N_BUILT && index.Count() == N_BUILT);
		idx_t max_level = 0, capacity = 0, approx_size = 0;
		std::vector<idx_t> nodes, edges;
		for (idx_t g = 0; g != G; ++g) {
			const auto part = index.ShardStats(g);
			const auto range = ShardedHNSWIndex::ShardRange(g, G, N_BUILT);
			EXPECT(part->count == range.second - range.first && part->level_stats.size() == part->max_level);
			max_level = std::max(max_level, part->max_level);
			capacity += part->capacity, approx_size += part->approx_size;
			nodes.resize(std::max(nodes.size(), part->level_stats.size()), 0);
			edges.resize(nodes.size(), 0);
			for (size_t l = 0; l != part->level_stats.size(); ++l)
				nodes[l] += part->level_stats[l].nodes, edges[l] += part->level_stats[l].edges;
		}
		EXPECT(stats->max_level == max_level && stats->capacity == capacity && stats->approx_size == approx_size);
		EXPECT(stats->capacity >= N_BUILT && stats->level_stats.size() == max_level);
		for (size_t l = 0; l != nodes.size(); ++l)
			EXPECT(stats->level_stats[l].nodes == nodes[l] && stats->level_stats[l].edges == edges[l]);
		if (max_level)
			EXPECT(stats->level_stats[0].nodes == N_BUILT); // every row has a level-0 node
	}

	// ---- 2. exact probe over the shards == host brute force
	(void)ExpectExact(index);

	// ---- 3. inserts after the build: ids N_BUILT .. N_BUILT + 4195 in three Construct calls — [2000, 4048) first, so the
	// first chunk straddles the route-block edge at 2048 (and carries the validity mask: five NULL rows, on both sides of that
	// edge and at both ends of the runs), then the rest [4048, 4196) (straddles the edge at 4096), then [0, 2000)
	const idx_t nulls[5] = {2005, 2047, 2048, 3000, 4047}; // offsets into the inserted rows
	{
		const idx_t a0 = 2000, a1 = 4048;
		std::vector<uint64_t> validity((a1 - a0 + 63) / 64, ~0ull);
		for (idx_t off : nulls) {
			validity[(off - a0) >> 6] &= ~(1ull << ((off - a0) & 63));
			never.insert((row_t)(N_BUILT + off));
		}
		index.Construct(&vecs[(N_BUILT + a0) * DIM], &ids[N_BUILT + a0], validity.data(), a1 - a0);
		index.Construct(&vecs[(N_BUILT + a1) * DIM], &ids[N_BUILT + a1], nullptr, N_INSERTED - a1);
		index.Construct(&vecs[N_BUILT * DIM], &ids[N_BUILT], nullptr, a0);
		for (idx_t off = 0; off != N_INSERTED; ++off)
			live[N_BUILT + off] = !never.count((row_t)(N_BUILT + off));
	}
	EXPECT(index.Count() == N_BUILT + N_INSERTED - 5 && index.IsDirty());
	std::vector<idx_t> expected_rows(G, 0); // what the routing rule deals to every shard
	for (idx_t i = 0; i != N_BUILT + N_INSERTED; ++i)
		if (live[i])
			expected_rows[shard_layout::OwnerOf((row_t)i, G, N_BUILT)]++;
	for (idx_t g = 0; g != G; ++g) {
		const auto range = ShardedHNSWIndex::ShardRange(g, G, N_BUILT);
		const idx_t received = index.ShardRowCount(g) - (range.second - range.first);
		std::printf("shard %zu received %zu inserted rows\n", (size_t)g, (size_t)received);
		EXPECT(index.ShardRowCount(g) == expected_rows[g]);
		if (G == 3)
			EXPECT(received >= 100 - 5 && received < N_INSERTED - 5);
	}
	{
		// 64 of the inserted vectors as queries: each finds its own row first, at distance 0
		std::vector<float> own(64 * DIM);
		std::vector<row_t> own_id(64);
		for (idx_t i = 0; i != 64; ++i) {
			idx_t off = i * 65 + 7; // spread over all three route blocks: 7 .. 4102
			while (never.count((row_t)(N_BUILT + off)))
				off++;
			own_id[i] = (row_t)(N_BUILT + off);
			std::copy(&vecs[own_id[i] * DIM], &vecs[own_id[i] * DIM] + DIM, &own[i * DIM]);
		}
		Results r(64);
		index.SearchBatch(own.data(), 64, K, EF, r.ids.data(), r.dist.data(), r.counts.data());
		for (idx_t i = 0; i != 64; ++i)
			EXPECT(r.counts[i] == K && r.ids[i * K] == own_id[i] && r.dist[i * K] == 0.f);
		ExpectNoneOf(r, never);
		Results all(NQ);
		index.SearchBatch(queries.data(), NQ, K, EF, all.ids.data(), all.dist.data(), all.counts.data());
		ExpectNoneOf(all, never);
		(void)ExpectExact(index);
	}

	// ---- 4. delete 50 inserted and 50 built ids: both sides of every range boundary and of the route-block edge at 4096
	{
		std::set<row_t> dead;
		for (idx_t g = 1; g != G; ++g) {
			const auto range = ShardedHNSWIndex::ShardRange(g, G, N_BUILT);
			dead.insert((row_t)range.first - 1), dead.insert((row_t)range.first);
		}
		dead.insert(0), dead.insert((row_t)N_BUILT - 1);
		for (idx_t i = 0; dead.size() < 50; ++i)
			dead.insert((row_t)(17 + 113 * i) % (row_t)N_BUILT);
		dead.insert((row_t)(N_BUILT + 4095)), dead.insert((row_t)(N_BUILT + 4096));
		dead.insert((row_t)N_BUILT), dead.insert((row_t)(N_BUILT + N_INSERTED - 1));
		for (idx_t i = 0; dead.size() < 100; ++i) {
			const row_t id = (row_t)(N_BUILT + (11 + 83 * i) % N_INSERTED);
			if (!never.count(id))
				dead.insert(id);
		}
		const std::vector<row_t> dead_list(dead.begin(), dead.end());
		idx_t built = 0;
		for (row_t id : dead_list)
			built += (idx_t)id < N_BUILT;
		EXPECT(dead_list.size() == 100 && built == 50);
		const idx_t before = index.Count();
		EXPECT(index.Delete(dead_list.data(), dead_list.size()) == 100);
		EXPECT(index.Count() == before - 100);
		for (row_t id : dead_list)
			live[id] = 0, never.insert(id);
		Results r(NQ);
		index.SearchBatch(queries.data(), NQ, K, EF, r.ids.data(), r.dist.data(), r.counts.data());
		ExpectNoneOf(r, never);
		(void)ExpectExact(index); // (none of them comes back, and the answers are the brute force over the live rows)
	}

	// ---- 5. filtered probe: the bitmap admits every third live row id, built and inserted alike
	{
		const idx_t n_bits = N_BUILT + N_INSERTED;
		std::vector<uint64_t> allowed((n_bits + 63) / 64, 0);
		auto admitted = [&](row_t id) { return (idx_t)id < n_bits && ((allowed[id >> 6] >> (id & 63)) & 1); };
		for (idx_t i = 0; i < n_bits; i += 3)
			if (live[i])
				allowed[i >> 6] |= 1ull << (i & 63);
		Results r(NQ);
		index.SearchBatchFiltered(queries.data(), NQ, K, EF, allowed.data(), n_bits, r.ids.data(), r.dist.data(),
		                          r.counts.data());
		idx_t hits = 0;
		for (idx_t q = 0; q != NQ; ++q) {
			EXPECT(r.counts[q] == K);
			const Answers truth = Truth(&queries[q * DIM], admitted);
			std::set<row_t> want;
			for (idx_t j = 0; j != K; ++j)
				want.insert(truth[j].second);
			for (idx_t j = 0; j != K; ++j) {
				const row_t id = r.ids[q * K + j];
				EXPECT(id >= 0 && admitted(id) && live[id]);
				hits += want.count(id);
			}
		}
		const double recall = (double)hits / (NQ * K);
		std::printf("filtered recall@%zu %.4f (ef %zu)\n", (size_t)K, recall, (size_t)EF);
		EXPECT(recall >= 0.95);
	}

	// ---- 6. persist and reload
	const auto blocks = index.PersistToBlocks(262136);
	EXPECT(!index.IsDirty());
	const auto small_blocks = index.PersistToBlocks(4099); // the header and the stream lengths straddle blocks
	EXPECT(!index.IsDirty());
	{
		const auto bytes = Concatenate(blocks, 262136);
		EXPECT(bytes == Concatenate(small_blocks, 4099));
		shard_layout::ContainerHeader header;
		EXPECT(shard_layout::Decode(bytes.data(), bytes.size(), header).empty());
		EXPECT(header.n_shards == G && header.n_total == N_BUILT && header.dim == DIM && header.route_block == 2048);
	}
	Results original(NQ);
	index.SearchBatch(queries.data(), NQ, K, EF, original.ids.data(), original.dist.data(), original.counts.data());
	loaded_p = std::make_unique<ShardedHNSWIndex>(DIM, options, 0, devices);
	ShardedHNSWIndex &loaded = *loaded_p;
	loaded.LoadFromBlocks(small_blocks);
	EXPECT(!loaded.IsDirty() && loaded.BuildRows() == N_BUILT);
	EXPECT(loaded.Count() == index.Count());
	{
		// what a checkpoint persists is equal: counts, levels, every per-level figure, shard by shard and summed.  `capacity`
		// and `approx_size` describe the allocation, which a load sizes to the stream's rows (as usearch's load does)
		const auto a = index.GetStats(), b = loaded.GetStats();
		std::printf("stats: count %zu / %zu, capacity %zu / %zu\n", (size_t)a->count, (size_t)b->count, (size_t)a->capacity,
		            (size_t)b->capacity);
		EXPECT(SameStats(*a, *b) && b->capacity >= b->count);
		for (idx_t g = 0; g != G; ++g)
			EXPECT(SameStats(*index.ShardStats(g), *loaded.ShardStats(g)));
		Results again(NQ);
		loaded.SearchBatch(queries.data(), NQ, K, EF, again.ids.data(), again.dist.data(), again.counts.data());
		EXPECT(again.ids == original.ids && again.counts == original.counts);
		EXPECT(!std::memcmp(again.dist.data(), original.dist.data(), NQ * K * sizeof(float))); // the same bits
	}
	{
		// the reloaded index routes as the original: one inserted and one built id are found by their owners ...
		const row_t two[2] = {(row_t)(N_BUILT + 2100), 3000};
		EXPECT(live[two[0]] && live[two[1]]);
		EXPECT(loaded.Delete(two, 2) == 2);
		live[two[0]] = live[two[1]] = 0, never.insert(two[0]), never.insert(two[1]);
		// ... and ten more rows land on the shard the rule names
		const idx_t first = N_BUILT + N_INSERTED, owner = shard_layout::OwnerOf((row_t)first, G, N_BUILT);
		EXPECT(owner == (N_INSERTED / 2048) % G && loaded.OwnerOf((row_t)first) == owner &&
		       loaded.OwnerOf((row_t)(first + N_LATE - 1)) == owner);
		std::vector<idx_t> rows_before(G);
		for (idx_t g = 0; g != G; ++g)
			rows_before[g] = loaded.ShardRowCount(g);
		loaded.Construct(&vecs[first * DIM], &ids[first], nullptr, N_LATE);
		for (idx_t i = 0; i != N_LATE; ++i)
			live[first + i] = 1;
		for (idx_t g = 0; g != G; ++g)
			EXPECT(loaded.ShardRowCount(g) == rows_before[g] + (g == owner ? N_LATE : 0));
		EXPECT(loaded.IsDirty());
	}

	// ---- 7. compact the reloaded index: same count, same exact answers
	{
		const Results before = ExpectExact(loaded);
		const idx_t count = loaded.Count();
		loaded.Compact();
		EXPECT(loaded.Count() == count);
		const Results after = ExpectExact(loaded);
		for (idx_t q = 0; q != NQ; ++q)
			EXPECT(std::set<row_t>(&before.ids[q * K], &before.ids[q * K] + K) ==
			       std::set<row_t>(&after.ids[q * K], &after.ids[q * K] + K));
	}

	// ---- an index created empty (n_total = 0), every row inserted: two shards, block-cyclic from id 0.  Its container is the
	// "different G" of step 8.
	const std::vector<int> other_devices(G == 2 ? 3 : 2, devices[0]);
	other_p = std::make_unique<ShardedHNSWIndex>(DIM, options, 0, other_devices);
	ShardedHNSWIndex &other = *other_p;
	{
		const idx_t OG = other_devices.size();
		other.Construct(&vecs[N_BUILT * DIM], ids.data(), nullptr, N_INSERTED); // the inserted vectors as rows 0 .. 4195
		EXPECT(other.Count() == N_INSERTED);
		std::vector<idx_t> want(OG, 0);
		for (idx_t i = 0; i != N_INSERTED; ++i)
			want[(i / 2048) % OG]++;
		for (idx_t g = 0; g != OG; ++g)
			EXPECT(other.ShardRowCount(g) == want[g]);
		Results r(16);
		other.SearchBatch(&vecs[(N_BUILT + 2040) * DIM], 16, K, EF, r.ids.data(), r.dist.data(), r.counts.data());
		for (idx_t i = 0; i != 16; ++i) // rows 2040 .. 2055: both sides of the first route-block edge
			EXPECT(r.counts[i] == K && r.ids[i * K] == (row_t)(2040 + i) && r.dist[i * K] == 0.f);
	}

	// ---- 8. refused loads leave the index exactly as it was
	{
		const idx_t count = loaded.Count();
		Results q0(1), now(1);
		loaded.SearchBatch(queries.data(), 1, K, EF, q0.ids.data(), q0.dist.data(), q0.counts.data());
		auto refused = [&](const std::vector<std::vector<uint8_t>> &container, const char *what) {
			bool thrown = false;
			try {
				loaded.LoadFromBlocks(container);
			} catch (const InternalException &e) {
				std::printf("refused (%s): %s\n", what, e.what());
				thrown = true;
			}
			if (!thrown)
				return false;
			loaded.SearchBatch(queries.data(), 1, K, EF, now.ids.data(), now.dist.data(), now.counts.data());
			return loaded.Count() == count && loaded.BuildRows() == N_BUILT && now.ids == q0.ids && now.counts == q0.counts &&
			       !std::memcmp(now.dist.data(), q0.dist.data(), K * sizeof(float));
		};
		auto truncated = small_blocks; // its last block is gone: the last shard's stream ends early, after the others loaded
		truncated.pop_back();
		EXPECT(refused(truncated, "truncated"));
		EXPECT(refused(other.PersistToBlocks(262136), "another shard count"));
		auto bad_magic = small_blocks;
		bad_magic[0][5] ^= 0x01;
		EXPECT(refused(bad_magic, "magic"));
		// and the container itself still loads
		loaded.LoadFromBlocks(blocks);
		EXPECT(loaded.Count() == index.Count());
	}

	std::printf("sharded lifecycle ok\nexchange: %s\n", index.ExchangeKind());
	return 0;
}

} // namespace

int main(int argc, char **argv) {
	std::vector<int> devices;
	for (int i = 1; i < argc; ++i)
		devices.push_back(std::atoi(argv[i]));
	if (devices.empty())
		devices = {0, 0, 0};
	try {
		const int rc = Run(devices);
		if (rc)
			std::_Exit(rc);
	} catch (const std::exception &e) {
		std::fprintf(stderr, "EXCEPTION: %s\n", e.what());
		std::fflush(nullptr);
		std::_Exit(1);
	}
	std::fflush(nullptr);
	other_p.reset(), loaded_p.reset(), index_p.reset();
	return 0;
}
