// sharded_index.hpp — one HNSW index spread over the GPUs of a node, driven from ONE process (the shape a DuckDB
// process needs; BASELINE configs[3]/[4]).
//
//   * Row-range shards: shard g owns rows [g*N/G, (g+1)*N/G) and holds an independent graph on its own device
//     (one vss_index per device).  Building needs no communication; a chunk of the ARRAY column is cut into the runs
//     that fall into each shard and staged there.
//   * Delete is routed to the owning shard.
//   * A probe runs the SAME query batch on every shard with the same k (all shards search concurrently, each on its own
//     stream); every shard's answers land in its block of the packed exchange layout (row ids, then distances:
//     vss_packed_block_bytes), ONE RCCL all-gather over xGMI (vss_exchange_allgather, one communicator per device, grouped)
//     moves the blocks, and vss_merge_topk_packed_device does the k-way merge on the merging device.  Row ids are global
//     table positions and the distances are the index metric on every shard, so the blocks merge as they are.
//   * RCCL wants one rank per device: when two shards share a device (how the logic is tested on a one-GPU box), or no
//     RCCL library can be loaded, the blocks travel by hipMemcpyPeerAsync instead and vss_merge_topk_device merges them
//     (VSS_SHARDED_EXCHANGE=peer forces that path).
//
//   * Rows that arrive after the build (Construct = the reference's Append / Insert) have ids past the build's range and are
//     dealt to the shards block-cyclically, 2048 ids at a time (shard_layout.hpp states the rule).  The rule is stateless, so
//     Delete finds such a row by the same function and nothing but the build's row count has to survive a checkpoint.
//   * PersistToBlocks writes one container — a 40-byte header (shard_layout.hpp), then every shard's usearch stream behind its
//     length — through one linked-block writer; LoadFromBlocks checks the header against this index, loads all G streams into
//     fresh shards built aside and swaps them in only when all G loaded.
//   * GetStats sums the shards' statistics; SearchBatchFiltered and SearchExactBatch are SearchBatch with another per-shard call.
//
// Concurrency is the caller's, as for the reference under DuckDB's IndexLock: Construct, Delete, Compact, PersistToBlocks and
// LoadFromBlocks are not to overlap each other or a probe, and the probes share one set of exchange buffers, so one probe
// runs at a time.
//
// The multi-process flavour of the same exchange — one rank per GPU — is duckdb-vss_amd/sharded.py + `bench.py --gpus N`.
// Nothing here computes anything: all arithmetic is behind `vss_*`.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>
#include <thread>

#include "../csrc/filter_groups.h"
#include "hnsw_index.hpp"
#include "shard_layout.hpp"

namespace vss_host {

class ShardedHNSWIndex {
public:
	// `devices[g]` = HIP device ordinal of shard g (ordinals may repeat: several shards on one GPU is legal, and is how
	// the logic is tested on a one-GPU box); `total_rows` fixes the row ranges (0: created empty, every row is inserted).
	ShardedHNSWIndex(idx_t vector_size, const OptionMap &options, idx_t total_rows, const std::vector<int> &devices)
	    : dim(vector_size), n_total(total_rows), options(options) {
		HNSWIndex::VerifyOptions(options);
		for (size_t g = 0; g != devices.size(); ++g) {
			auto range = ShardRange(g, devices.size(), total_rows);
			Shard s;
			s.device = devices[g];
			s.lo = range.first, s.hi = range.second;
			s.index = std::make_unique<HNSWIndex>(vector_size, options, s.hi - s.lo, s.device);
			// the row-id bitmap of a filtered probe is uploaded once per device: shards of one device share a slot
			for (s.bitmap = 0; s.bitmap != bitmaps.size() && bitmaps[s.bitmap].device != s.device;)
				s.bitmap++;
			if (s.bitmap == bitmaps.size())
				bitmaps.push_back({s.device, nullptr, 0});
			shards.push_back(std::move(s));
		}
		if (shards.empty())
			throw InternalException("a sharded index needs at least one device");
		// one RCCL communicator per device when every shard has a device of its own
		bool distinct = true;
		for (size_t g = 0; g != devices.size(); ++g)
			for (size_t o = 0; o != g; ++o)
				distinct = distinct && devices[g] != devices[o];
		const char *how = std::getenv("VSS_SHARDED_EXCHANGE");
		if (distinct && !(how && !std::strcmp(how, "peer")) && vss_exchange_available()) {
			comms.assign(devices.size(), nullptr);
			if (vss_exchange_init_all(comms.data(), (int)devices.size(), devices.data()) != VSS_OK)
				comms.clear(); // (the peer-copy path below)
		}
	}
	~ShardedHNSWIndex() {
		for (auto *c : comms)
			(void)vss_exchange_destroy(c);
		for (auto &s : shards)
			s.Release();
		for (auto &b : bitmaps) {
			(void)hipSetDevice(b.device);
			(void)hipFree(b.words), (void)hipFree(b.group_of);
		}
		if (m_dist) {
			(void)hipSetDevice(shards[0].device);
			(void)hipFree(m_dist), (void)hipFree(m_keys), (void)hipFree(o_dist), (void)hipFree(o_keys), (void)hipFree(o_cnt);
		}
	}

	static std::pair<idx_t, idx_t> ShardRange(idx_t g, idx_t n_shards, idx_t n_total) {
		return shard_layout::ShardRange(g, n_shards, n_total);
	}
	// shard_layout.hpp's rule: the row-range owner inside the build's range, block-cyclic past it, negative ids refused
	idx_t OwnerOf(row_t rowid) const {
		if (rowid < 0)
			throw InternalException("Row id " + std::to_string(rowid) + " is negative: no shard owns it");
		return shard_layout::OwnerOf(rowid, shards.size(), n_total);
	}
	idx_t ShardCount() const {
		return shards.size();
	}
	// the build's row count: the routing rule's n_total (adopted from the container by LoadFromBlocks)
	idx_t BuildRows() const {
		return n_total;
	}
	// live rows / statistics of one shard (the tests read how the inserts were dealt out)
	idx_t ShardRowCount(idx_t g) {
		return shards.at(g).index->Count();
	}
	std::unique_ptr<HNSWIndexStats> ShardStats(idx_t g) {
		return shards.at(g).index->GetStats();
	}
	// the engine's handle of one shard (filter_probe_harness.cpp asks every shard on its own and merges the answers itself)
	vss_index *ShardHandle(idx_t g) {
		return shards.at(g).index->Handle();
	}
	// "rccl": one all-gather per probe over one communicator per device; "peer": hipMemcpyPeerAsync to the merging device
	const char *ExchangeKind() const {
		return comms.empty() ? "peer" : "rccl";
	}
	idx_t Count() {
		idx_t n = 0;
		for (auto &s : shards)
			n += s.index->Count();
		return n;
	}

	// ---- bulk build: PhysicalCreateHNSWIndex::Finalize / HNSWIndexConstructTask (hnsw_index_physical_create.cpp:148-310)
	void BulkReserve(idx_t threads) {
		for (auto &s : shards)
			s.index->BulkReserve(s.hi - s.lo, threads);
	}
	// one chunk of the collection: rows are cut into runs owned by the same shard (row ids of a scan chunk are ascending,
	// so a chunk normally is one run, two at a shard boundary)
	void BulkAppendChunk(const float *vec_child_data, const row_t *rowid_data, const uint64_t *validity, idx_t count) {
		for (auto &run : CutIntoRuns(rowid_data, validity, count))
			shards[run.owner].index->BulkAppendChunk(vec_child_data + run.begin * dim, rowid_data + run.begin,
			                                         validity ? run.validity.data() : nullptr, run.end - run.begin);
	}
	void BulkFinalize() { // the devices do not interact: every shard links its rows at the same time, one host thread each
		std::vector<std::thread> pool;
		std::vector<std::string> errors(shards.size());
		for (size_t g = 0; g != shards.size(); ++g)
			pool.emplace_back([this, g, &errors] {
				try {
					shards[g].index->BulkFinalize();
				} catch (const std::exception &e) {
					errors[g] = e.what();
				}
			});
		for (auto &t : pool)
			t.join();
		for (auto &e : errors)
			if (!e.empty())
				throw InternalException(e);
	}

	// ---- HNSWIndex::Construct (Append / Insert) — hnsw_index.cpp:421-479, 519-530 — over the shards: the chunk is cut into
	// runs with one owner exactly as BulkAppendChunk cuts it, every owner's HNSWIndex::Construct links its runs (it grows the
	// shard's capacity by NextPowerOfTwo as the reference does), shards that received rows link at the same time, one host
	// thread each.  Rows keep the chunk's order inside a shard; NULL rows (cleared validity bit) are skipped by the shard.
	void Construct(const float *vec_child_data, const row_t *rowid_data, const uint64_t *validity, idx_t count) {
		const auto runs = CutIntoRuns(rowid_data, validity, count); // (a negative id throws here, before any shard changes)
		std::vector<std::thread> pool;
		std::vector<std::string> errors(shards.size());
		for (size_t g = 0; g != shards.size(); ++g) {
			bool receives = false;
			for (auto &run : runs)
				receives = receives || run.owner == g;
			if (!receives)
				continue;
			pool.emplace_back([this, g, &runs, &errors, vec_child_data, rowid_data, validity] {
				try {
					for (auto &run : runs)
						if (run.owner == g)
							shards[g].index->Construct(vec_child_data + run.begin * dim, rowid_data + run.begin,
							                           validity ? run.validity.data() : nullptr, run.end - run.begin);
				} catch (const std::exception &e) {
					errors[g] = e.what();
				}
			});
		}
		for (auto &t : pool)
			t.join();
		for (auto &e : errors)
			if (!e.empty())
				throw InternalException(e);
	}

	// ---- HNSWIndex::Delete (hnsw_index.cpp:496-512), routed to the owners
	idx_t Delete(const row_t *rowid_data, idx_t count) {
		std::vector<std::vector<row_t>> per(shards.size());
		for (idx_t i = 0; i != count; ++i)
			per[OwnerOf(rowid_data[i])].push_back(rowid_data[i]);
		const idx_t before = Count();
		for (size_t g = 0; g != shards.size(); ++g)
			if (!per[g].empty())
				shards[g].index->Delete(per[g].data(), per[g].size());
		return before - Count();
	}
	void Compact() {
		for (auto &s : shards)
			s.index->Compact();
	}

	// ---- HNSWIndex::GetStats (hnsw_index.cpp:292-306) over the shards: count, capacity and approx_size are sums, max_level
	// is the maximum, and the per-level statistics are summed level by level (a shard with fewer levels adds nothing above
	// its top; every shard's list has the reference's `i < max_level` length).
	std::unique_ptr<HNSWIndexStats> GetStats() {
		auto result = std::make_unique<HNSWIndexStats>();
		result->max_level = result->count = result->capacity = result->approx_size = 0;
		for (auto &s : shards) {
			const auto part = s.index->GetStats();
			result->max_level = std::max(result->max_level, part->max_level);
			result->count += part->count;
			result->capacity += part->capacity;
			result->approx_size += part->approx_size;
			if (result->level_stats.size() < part->level_stats.size())
				result->level_stats.resize(part->level_stats.size(), HNSWLevelStats {0, 0, 0, 0});
			for (size_t l = 0; l != part->level_stats.size(); ++l) {
				result->level_stats[l].nodes += part->level_stats[l].nodes;
				result->level_stats[l].edges += part->level_stats[l].edges;
				result->level_stats[l].max_edges += part->level_stats[l].max_edges;
				result->level_stats[l].allocated_bytes += part->level_stats[l].allocated_bytes;
			}
		}
		return result;
	}

	// ---- persistence (hnsw_index.cpp:532-554, 223-236): ONE container through one linked-block writer, split into blocks of
	// `block_payload` bytes exactly as HNSWIndex::PersistToBlocks splits its stream — the header of shard_layout.hpp, then
	// for every shard its stream's length and the stream vss_save writes.
	bool IsDirty() const {
		for (auto &s : shards)
			if (s.index->IsDirty())
				return true;
		return false;
	}
	std::vector<std::vector<uint8_t>> PersistToBlocks(idx_t block_payload) {
		if (!block_payload)
			throw InternalException("Failed to serialize the HNSW index: blocks without payload");
		BlockWriter w {{}, block_payload, 0};
		shard_layout::ContainerHeader header;
		header.n_shards = (uint32_t)shards.size();
		header.n_total = n_total;
		header.dim = dim;
		uint8_t bytes[shard_layout::HEADER_BYTES];
		shard_layout::Encode(header, bytes);
		w.Write(bytes, sizeof bytes);
		for (auto &s : shards) {
			const uint64_t length = vss_serialized_length(s.index->Handle());
			uint8_t le[8];
			shard_layout::PutLE(le, length, 8);
			w.Write(le, 8);
			const uint64_t before = w.written;
			if (vss_save(s.index->Handle(), &BlockWriter::Callback, &w) != VSS_OK)
				throw InternalException(std::string("Failed to serialize the HNSW index: ") + vss_last_error(s.index->Handle()));
			if (w.written - before != length)
				throw InternalException("Failed to serialize the HNSW index: a shard wrote " +
				                        std::to_string(w.written - before) + " bytes, " + std::to_string(length) + " announced");
		}
		for (auto &s : shards)
			s.index->ClearDirty();
		return std::move(w.blocks);
	}
	// Checks the header against this index before any shard is touched (G = ShardCount(), dim, route block 2048), loads every
	// stream into a fresh HNSWIndex on its shard's device, and swaps all G in — adopting the container's n_total, hence its
	// row ranges — only when all G loaded.  A refused or failed load throws and leaves the index exactly as it was.
	void LoadFromBlocks(const std::vector<std::vector<uint8_t>> &blocks) {
		BlockReader r {&blocks, 0, 0};
		uint8_t bytes[shard_layout::HEADER_BYTES];
		const size_t got = r.Read(bytes, sizeof bytes);
		shard_layout::ContainerHeader header;
		const std::string why = shard_layout::Decode(bytes, got, header);
		if (!why.empty())
			throw InternalException("Failed to load the sharded HNSW index: " + why);
		if (header.n_shards != shards.size())
			throw InternalException("Failed to load the sharded HNSW index: the container holds " +
			                        std::to_string(header.n_shards) + " shards, this index has " + std::to_string(shards.size()));
		if (header.dim != dim)
			throw InternalException("Failed to load the sharded HNSW index: the container's vectors have " +
			                        std::to_string(header.dim) + " dimensions, this index has " + std::to_string(dim));
		if (header.route_block != shard_layout::ROUTE_BLOCK)
			throw InternalException("Failed to load the sharded HNSW index: the container routes inserted rows in blocks of " +
			                        std::to_string(header.route_block) + ", this code in blocks of " +
			                        std::to_string(shard_layout::ROUTE_BLOCK));
		std::vector<std::unique_ptr<HNSWIndex>> fresh;
		for (size_t g = 0; g != shards.size(); ++g) {
			const std::string shard_name = "shard " + std::to_string(g);
			uint8_t le[8];
			if (r.Read(le, 8) != 8)
				throw InternalException("Failed to load the sharded HNSW index: the container ends before the stream of " + shard_name);
			r.limit = shard_layout::GetLE(le, 8);
			fresh.push_back(std::make_unique<HNSWIndex>(dim, options, 0, shards[g].device));
			HNSWIndex &index = *fresh.back();
			if (vss_load(index.Handle(), &BlockReader::Callback, &r) != VSS_OK)
				throw InternalException("Failed to load the sharded HNSW index: " + shard_name + ": " + vss_last_error(index.Handle()));
			if (r.limit)
				throw InternalException("Failed to load the sharded HNSW index: " + shard_name + " left " + std::to_string(r.limit) +
				                        " bytes of its stream unread");
			if (index.GetVectorSize() != dim)
				throw InternalException("Failed to load the sharded HNSW index: " + shard_name + " holds vectors of " +
				                        std::to_string(index.GetVectorSize()) + " dimensions");
			index.SyncSize();
		}
		n_total = header.n_total;
		for (size_t g = 0; g != shards.size(); ++g) {
			const auto range = ShardRange(g, shards.size(), n_total);
			shards[g].lo = range.first, shards[g].hi = range.second;
			shards[g].index = std::move(fresh[g]);
		}
	}

	// ---- the batched probe (PhysicalHNSWIndexJoin::Execute, hnsw_optimize_join.cpp:111-168) over all shards.
	// queries = n x dim host floats; out_rowids = n x k (unused cells -1), out_distances optional, out_counts optional.
	void SearchBatch(const float *queries, idx_t n, idx_t k, idx_t ef, row_t *out_rowids, float *out_distances,
	                 uint32_t *out_counts) {
		if (!n || !k)
			return;
		Ensure(n, k);
		Probe(
		    queries, n, k, out_rowids, out_distances, out_counts,
		    [&](Shard &s, row_t *keys, float *dist) {
			    Vss(s, vss_search_batch_device_begin(s.index->Handle(), 0, s.d_q, n, k, ef, keys, dist, s.d_cnt));
		    },
		    [&](Shard &s) { Vss(s, vss_search_batch_end(s.index->Handle(), 0)); });
	}

	// ---- the same probe with a predicate pushed into the traversal (vss_search_batch_filtered_device per shard): a row is
	// admitted iff it is live and bit `rowid` of `allowed` is set.  The bitmap is over GLOBAL row ids, (n_bits + 63) / 64 host
	// words (UploadTables).  Same exchange and merge as SearchBatch, and like it every shard is started through the engine's
	// _begin form before the first is waited for: all G search at once.  The uploaded bitmap stays in bitmaps[] until every shard's
	// vss_search_batch_end has returned (the engine reads it again when it re-runs a query), on the error path too: DrainProbes.
	void SearchBatchFiltered(const float *queries, idx_t n, idx_t k, idx_t ef, const uint64_t *allowed, idx_t n_bits,
	                         row_t *out_rowids, float *out_distances, uint32_t *out_counts) {
		if (!n || !k)
			return;
		if (!allowed)
			throw InternalException("Failed to search the HNSW index: filtered search needs a row-id bitmap");
		Ensure(n, k);
		UploadTables(allowed, vss::host::filter_group_words(n_bits), nullptr, 0);
		ProbeThroughBegin(queries, n, k, out_rowids, out_distances, out_counts, [&](Shard &s, row_t *keys, float *dist) {
			Vss(s, vss_search_batch_filtered_device_begin(s.index->Handle(), 0, s.d_q, n, k, ef, bitmaps[s.bitmap].words, n_bits,
			                                              keys, dist, s.d_cnt));
		});
	}

	// ---- the same probe with a predicate PER QUERY (vss_search_batch_filtered_groups_device per shard): the chunk of a join whose
	// subquery is correlated.  `allowed` = n_groups bitmaps over GLOBAL row ids laid end to end, (n_bits + 63) / 64 host words
	// each; query q is filtered by bitmap group_of[q] < n_groups (CheckTables).  Exchange and merge are SearchBatchFiltered's.
	void SearchBatchFilteredGroups(const float *queries, idx_t n, idx_t k, idx_t ef, const uint64_t *allowed, idx_t n_groups,
	                               idx_t n_bits, const uint32_t *group_of, row_t *out_rowids, float *out_distances,
	                               uint32_t *out_counts) {
		if (!n || !k)
			return;
		CheckTables(allowed, n_groups, n_bits, group_of, true, n);
		Ensure(n, k);
		UploadTables(allowed, vss::host::filter_group_words(n_bits) * n_groups, group_of, n); // (checked: no wrap)
		ProbeThroughBegin(queries, n, k, out_rowids, out_distances, out_counts, [&](Shard &s, row_t *keys, float *dist) {
			Vss(s, vss_search_batch_filtered_groups_device_begin(s.index->Handle(), 0, s.d_q, n, k, ef, bitmaps[s.bitmap].words,
			                                                     n_groups, n_bits, bitmaps[s.bitmap].group_of, keys, dist, s.d_cnt));
		});
	}

	// ---- brute force over every live row of every shard (vss_search_exact_batch_device per shard, the same exchange and
	// merge): the recall oracle of a sharded index.  Every shard returns its k best rows by (distance, slot); the merge orders
	// the union by (distance, row id) — so rows at exactly equal distance come back in (distance, row id) order, and where
	// more rows tie at the k-th distance than fit, which of them a shard hands over is its slot order's choice.
	void SearchExactBatch(const float *queries, idx_t n, idx_t k, row_t *out_rowids, float *out_distances,
	                      uint32_t *out_counts) {
		if (!n || !k)
			return;
		Ensure(n, k);
		Probe(
		    queries, n, k, out_rowids, out_distances, out_counts,
		    [&](Shard &s, row_t *keys, float *dist) {
			    Vss(s, vss_search_exact_batch_device(s.index->Handle(), s.d_q, n, k, keys, dist, s.d_cnt));
		    },
		    [&](Shard &s) { Vss(s, vss_synchronize(s.index->Handle())); });
	}

	// ---- the exact answer under a predicate PER QUERY, scoring only the admitted rows (vss_search_exact_batch_filtered_groups_device
	// per shard): every shard answers under the same table over GLOBAL row ids, uploaded as SearchBatchFilteredGroups uploads it
	// (group_of may be nullptr here: every query takes bitmap 0).  Exchange and merge are SearchExactBatch's, and so is the order
	// of rows at exactly equal distance: (distance, row id).
	void SearchExactBatchFilteredGroups(const float *queries, idx_t n, idx_t k, const uint64_t *allowed, idx_t n_groups, idx_t n_bits,
	                                    const uint32_t *group_of, row_t *out_rowids, float *out_distances, uint32_t *out_counts) {
		if (!n || !k)
			return;
		CheckTables(allowed, n_groups, n_bits, group_of, false, n);
		Ensure(n, k);
		UploadTables(allowed, vss::host::filter_group_words(n_bits) * n_groups, group_of, n);
		Probe(
		    queries, n, k, out_rowids, out_distances, out_counts,
		    [&](Shard &s, row_t *keys, float *dist) {
			    Vss(s, vss_search_exact_batch_filtered_groups_device(s.index->Handle(), s.d_q, n, k, bitmaps[s.bitmap].words, n_groups,
			                                                         n_bits, group_of ? bitmaps[s.bitmap].group_of : nullptr, keys,
			                                                         dist, s.d_cnt));
		    },
		    [&](Shard &s) { Vss(s, vss_synchronize(s.index->Handle())); });
	}

	// ---- the same chunk with every group answered by the cheaper of the two calls above (vss_search_batch_filtered_groups_auto_device
	// per shard): each shard routes by ITS OWN counts of live admitted rows and ITS OWN live rows — a tenant that is large in
	// one shard and tiny in another is walked here and scanned there.  route_c as in the engine (0: the default constant).
	// shard_routes (optional) receives the route tables, shard after shard: [g * n + q] = 0 graph, 1 exact.  Upload, exchange and
	// merge are SearchExactBatchFilteredGroups'; rows at exactly equal distance come back by (distance, row id).
	void SearchBatchFilteredGroupsAuto(const float *queries, idx_t n, idx_t k, idx_t ef, const uint64_t *allowed, idx_t n_groups,
	                                   idx_t n_bits, const uint32_t *group_of, uint64_t route_c, row_t *out_rowids, float *out_distances,
	                                   uint32_t *out_counts, std::vector<uint8_t> *shard_routes = nullptr) {
		if (shard_routes)
			shard_routes->assign(shards.size() * n, 0);
		if (!n || !k)
			return;
		CheckTables(allowed, n_groups, n_bits, group_of, false, n);
		Ensure(n, k);
		UploadTables(allowed, vss::host::filter_group_words(n_bits) * n_groups, group_of, n);
		Probe(
		    queries, n, k, out_rowids, out_distances, out_counts,
		    [&](Shard &s, row_t *keys, float *dist) {
			    Vss(s, vss_search_batch_filtered_groups_auto_device(s.index->Handle(), s.d_q, n, k, ef, bitmaps[s.bitmap].words, n_groups,
			                                                        n_bits, group_of ? bitmaps[s.bitmap].group_of : nullptr, route_c,
			                                                        keys, dist, s.d_cnt, s.d_route));
		    },
		    [&](Shard &s) { Vss(s, vss_synchronize(s.index->Handle())); });
		for (size_t g = 0; shard_routes && g != shards.size(); ++g) {
			Hip(hipSetDevice(shards[g].device), "hipSetDevice");
			Hip(hipMemcpy(shard_routes->data() + g * n, shards[g].d_route, n, hipMemcpyDeviceToHost), "copy routes");
		}
	}

	// ---- equality predicates on the label column (vss_search_batch_by_label_device per shard), no bitmaps.  Row ids are GLOBAL,
	// so every shard's engine gets the whole column: SetLabels writes the same cells into each (4 bytes per row id and shard).
	// Not persisted: set again after Load.
	void SetLabels(idx_t first_rowid, const uint32_t *labels, idx_t n) {
		for (auto &s : shards)
			s.index->SetLabels(first_rowid, labels, n);
	}
	void ClearLabels() {
		for (auto &s : shards)
			s.index->ClearLabels();
	}
	// Query q admits the live rows labelled want[q] (VSS_NO_LABEL: none).  mode VSS_BY_LABEL_AUTO: every shard routes every
	// value by ITS OWN count of such rows and ITS OWN live rows, as in SearchBatchFilteredGroupsAuto; _GRAPH / _EXACT force one
	// way in all of them.  shard_routes (optional): [g * n + q].  The wanted values travel as UploadTables' group numbers; the
	// exchange and merge are SearchExactBatchFilteredGroups' — rows at exactly equal distance come back by (distance, row id).
	void SearchBatchByLabel(const float *queries, idx_t n, idx_t k, idx_t ef, const uint32_t *want, int mode, uint64_t route_c,
	                        row_t *out_rowids, float *out_distances, uint32_t *out_counts, std::vector<uint8_t> *shard_routes = nullptr) {
		if (shard_routes)
			shard_routes->assign(shards.size() * n, 0);
		if (!n || !k)
			return;
		if (!want)
			throw InternalException("Failed to search the HNSW index: search by label needs the wanted label of every query");
		Ensure(n, k);
		UploadTables(nullptr, 0, want, n);
		if (mode == VSS_BY_LABEL_GRAPH) {
			ProbeByLabelGraph(queries, n, k, ef, out_rowids, out_distances, out_counts, [&](Shard &s) {
				vss_label_predicate p = {};
				p.kind = VSS_LABEL_EQ, p.d_want = bitmaps[s.bitmap].group_of;
				return p;
			});
			return;
		}
		Probe(
		    queries, n, k, out_rowids, out_distances, out_counts,
		    [&](Shard &s, row_t *keys, float *dist) {
			    Vss(s, vss_search_batch_by_label_device(s.index->Handle(), s.d_q, n, k, ef, bitmaps[s.bitmap].group_of, mode, route_c, keys,
			                                            dist, s.d_cnt, s.d_route));
		    },
		    [&](Shard &s) { Vss(s, vss_synchronize(s.index->Handle())); });
		for (size_t g = 0; shard_routes && g != shards.size(); ++g) {
			Hip(hipSetDevice(shards[g].device), "hipSetDevice");
			Hip(hipMemcpy(shard_routes->data() + g * n, shards[g].d_route, n, hipMemcpyDeviceToHost), "copy routes");
		}
	}
	// Query q admits the live rows whose label lies in [lo[q], hi[q]], both ends inclusive and unsigned (lo > hi: none; a
	// VSS_NO_LABEL cell is in no range): vss_search_batch_by_label_range_device per shard.  Modes, shard_routes, exchange and merge
	// are SearchBatchByLabel's; the ends travel as UploadTables' group numbers, the n lower ends ahead of the n upper ones.
	void SearchBatchByLabelRange(const float *queries, idx_t n, idx_t k, idx_t ef, const uint32_t *lo, const uint32_t *hi, int mode,
	                             uint64_t route_c, row_t *out_rowids, float *out_distances, uint32_t *out_counts,
	                             std::vector<uint8_t> *shard_routes = nullptr) {
		if (shard_routes)
			shard_routes->assign(shards.size() * n, 0);
		if (!n || !k)
			return;
		if (!lo || !hi)
			throw InternalException("Failed to search the HNSW index: search by label range needs both ends of every query's range");
		Ensure(n, k);
		std::vector<uint32_t> ends(lo, lo + n);
		ends.insert(ends.end(), hi, hi + n);
		UploadTables(nullptr, 0, ends.data(), 2 * n);
		if (mode == VSS_BY_LABEL_GRAPH) {
			ProbeByLabelGraph(queries, n, k, ef, out_rowids, out_distances, out_counts, [&](Shard &s) {
				vss_label_predicate p = {};
				p.kind = VSS_LABEL_RANGE, p.d_lo = bitmaps[s.bitmap].group_of, p.d_hi = bitmaps[s.bitmap].group_of + n;
				return p;
			});
			return;
		}
		Probe(
		    queries, n, k, out_rowids, out_distances, out_counts,
		    [&](Shard &s, row_t *keys, float *dist) {
			    const uint32_t *d_ends = bitmaps[s.bitmap].group_of;
			    Vss(s, vss_search_batch_by_label_range_device(s.index->Handle(), s.d_q, n, k, ef, d_ends, d_ends + n, mode, route_c, keys,
			                                                  dist, s.d_cnt, s.d_route));
		    },
		    [&](Shard &s) { Vss(s, vss_synchronize(s.index->Handle())); });
		for (size_t g = 0; shard_routes && g != shards.size(); ++g) {
			Hip(hipSetDevice(shards[g].device), "hipSetDevice");
			Hip(hipMemcpy(shard_routes->data() + g * n, shards[g].d_route, n, hipMemcpyDeviceToHost), "copy routes");
		}
	}
	// Label columns 0 .. VSS_LABEL_COLUMNS_MAX - 1 (column 0 is the column of SetLabels): every shard gets the whole column, as
	// SetLabels gives it.  ClearLabels clears every column.  Not persisted: set again after Load.
	void SetLabelColumn(uint32_t column, idx_t first_rowid, const uint32_t *labels, idx_t n) {
		for (auto &s : shards)
			s.index->SetLabelColumn(column, first_rowid, labels, n);
	}
	void ClearLabelColumn(uint32_t column) {
		for (auto &s : shards)
			s.index->ClearLabelColumn(column);
	}
	// Query q admits the live rows whose cell in columns[j] lies in [lo[q * n_columns + j], hi[q * n_columns + j]] for EVERY j <
	// n_columns (any lo > hi: none; hi = 0xFFFFFFFF: no upper bound; VSS_NO_LABEL or no cell in a named column: in no box):
	// vss_search_batch_by_label_box_device per shard, every shard holding the whole columns.  Modes, shard_routes, exchange and
	// merge are SearchBatchByLabelRange's; both matrices travel as UploadTables' group numbers, lo's n * n_columns words first.
	void SearchBatchByLabelBox(const float *queries, idx_t n, idx_t k, idx_t ef, const uint32_t *columns, idx_t n_columns, const uint32_t *lo,
	                           const uint32_t *hi, int mode, uint64_t route_c, row_t *out_rowids, float *out_distances, uint32_t *out_counts,
	                           std::vector<uint8_t> *shard_routes = nullptr) {
		if (shard_routes)
			shard_routes->assign(shards.size() * n, 0);
		if (!n || !k)
			return;
		if (n_columns < 1 || n_columns > VSS_LABEL_COLUMNS_MAX || !columns)
			throw InternalException("Failed to search the HNSW index: search by label box names 1 to 4 label columns");
		if (!lo || !hi)
			throw InternalException("Failed to search the HNSW index: search by label box needs both ends of every query's ranges");
		Ensure(n, k);
		std::vector<uint32_t> ends(lo, lo + n * n_columns);
		ends.insert(ends.end(), hi, hi + n * n_columns);
		UploadTables(nullptr, 0, ends.data(), 2 * n * n_columns);
		if (mode == VSS_BY_LABEL_GRAPH) {
			ProbeByLabelGraph(queries, n, k, ef, out_rowids, out_distances, out_counts, [&](Shard &s) {
				vss_label_predicate p = {};
				p.kind = VSS_LABEL_BOX, p.n_columns = (uint32_t)n_columns;
				std::copy(columns, columns + n_columns, p.columns);
				p.d_lo = bitmaps[s.bitmap].group_of, p.d_hi = bitmaps[s.bitmap].group_of + n * n_columns;
				return p;
			});
			return;
		}
		Probe(
		    queries, n, k, out_rowids, out_distances, out_counts,
		    [&](Shard &s, row_t *keys, float *dist) {
			    const uint32_t *d_ends = bitmaps[s.bitmap].group_of;
			    Vss(s, vss_search_batch_by_label_box_device(s.index->Handle(), s.d_q, n, k, ef, columns, n_columns, d_ends, d_ends + n * n_columns,
			                                                mode, route_c, keys, dist, s.d_cnt, s.d_route));
		    },
		    [&](Shard &s) { Vss(s, vss_synchronize(s.index->Handle())); });
		for (size_t g = 0; shard_routes && g != shards.size(); ++g) {
			Hip(hipSetDevice(shards[g].device), "hipSetDevice");
			Hip(hipMemcpy(shard_routes->data() + g * n, shards[g].d_route, n, hipMemcpyDeviceToHost), "copy routes");
		}
	}
	// A label column of 64-bit cells: every shard gets the whole column, as SetLabelColumn gives it.
	void SetLabelColumn64(uint32_t column, idx_t first_rowid, const uint64_t *labels, idx_t n) {
		for (auto &s : shards)
			s.index->SetLabelColumn64(column, first_rowid, labels, n);
	}
	// SearchBatchByLabelBox with 64-bit ends over columns of either width (vss_search_batch_by_label_box64_device per shard; hi =
	// VSS_NO_LABEL64: no upper bound).  Modes, shard_routes, exchange and merge are SearchBatchByLabelBox's; both matrices travel
	// as UploadTables' group numbers, every 64-bit end as a PAIR of words in memory order, lo's 2 * n * n_columns words first —
	// hi's then begin 8 * n * n_columns bytes in, aligned for the device to read them as 64-bit ends again.
	void SearchBatchByLabelBox64(const float *queries, idx_t n, idx_t k, idx_t ef, const uint32_t *columns, idx_t n_columns, const uint64_t *lo,
	                             const uint64_t *hi, int mode, uint64_t route_c, row_t *out_rowids, float *out_distances, uint32_t *out_counts,
	                             std::vector<uint8_t> *shard_routes = nullptr) {
		if (shard_routes)
			shard_routes->assign(shards.size() * n, 0);
		if (!n || !k)
			return;
		if (n_columns < 1 || n_columns > VSS_LABEL_COLUMNS_MAX || !columns)
			throw InternalException("Failed to search the HNSW index: search by label box64 names 1 to 4 label columns");
		if (!lo || !hi)
			throw InternalException("Failed to search the HNSW index: search by label box64 needs both ends of every query's ranges");
		Ensure(n, k);
		const idx_t words = 2 * n * n_columns; // of one matrix
		std::vector<uint32_t> ends(2 * words);
		std::memcpy(ends.data(), lo, words * 4);
		std::memcpy(ends.data() + words, hi, words * 4);
		UploadTables(nullptr, 0, ends.data(), 2 * words);
		if (mode == VSS_BY_LABEL_GRAPH) {
			ProbeByLabelGraph(queries, n, k, ef, out_rowids, out_distances, out_counts, [&](Shard &s) {
				vss_label_predicate p = {};
				p.kind = VSS_LABEL_BOX64, p.n_columns = (uint32_t)n_columns;
				std::copy(columns, columns + n_columns, p.columns);
				p.d_lo = bitmaps[s.bitmap].group_of, p.d_hi = bitmaps[s.bitmap].group_of + words;
				return p;
			});
			return;
		}
		Probe(
		    queries, n, k, out_rowids, out_distances, out_counts,
		    [&](Shard &s, row_t *keys, float *dist) {
			    const uint32_t *d_ends = bitmaps[s.bitmap].group_of;
			    Vss(s, vss_search_batch_by_label_box64_device(s.index->Handle(), s.d_q, n, k, ef, columns, n_columns,
			                                                  reinterpret_cast<const uint64_t *>(d_ends),
			                                                  reinterpret_cast<const uint64_t *>(d_ends + words), mode, route_c, keys, dist, s.d_cnt,
			                                                  s.d_route));
		    },
		    [&](Shard &s) { Vss(s, vss_synchronize(s.index->Handle())); });
		for (size_t g = 0; shard_routes && g != shards.size(); ++g) {
			Hip(hipSetDevice(shards[g].device), "hipSetDevice");
			Hip(hipMemcpy(shard_routes->data() + g * n, shards[g].d_route, n, hipMemcpyDeviceToHost), "copy routes");
		}
	}
	// An IN-list on one label column inside a box of ranges (vss_search_batch_by_label_set_box_device per shard, every shard over
	// its own copy of the columns, the answers merged as SearchBatchByLabelBox64 merges them).  Modes, shard_routes, exchange and
	// merge are SearchBatchByLabelBox64's; the three matrices travel as UploadTables' group numbers, every 64-bit word as a PAIR
	// of words in memory order: the sets' 2 * n * set_width words first, then lo's and hi's 2 * n * n_columns each — every matrix
	// begins a multiple of 8 bytes in, aligned for the device to read it as 64-bit words again.
	void SearchBatchByLabelSetBox(const float *queries, idx_t n, idx_t k, idx_t ef, uint32_t set_column, const uint64_t *sets, uint32_t set_width,
	                              const uint32_t *columns, idx_t n_columns, const uint64_t *lo, const uint64_t *hi, int mode, uint64_t route_c,
	                              row_t *out_rowids, float *out_distances, uint32_t *out_counts, std::vector<uint8_t> *shard_routes = nullptr) {
		if (shard_routes)
			shard_routes->assign(shards.size() * n, 0);
		if (!n || !k)
			return;
		if (set_width < 1 || set_width > VSS_LABEL_SET_MAX || !sets)
			throw InternalException("Failed to search the HNSW index: search by label set box needs 1 to 32 words per query");
		if (n_columns > VSS_LABEL_COLUMNS_MAX - 1 || (n_columns && (!columns || !lo || !hi)))
			throw InternalException("Failed to search the HNSW index: search by label set box names 0 to 3 range columns with both ends of "
			                        "every query's ranges");
		Ensure(n, k);
		const idx_t set_words = 2 * n * set_width, end_words = 2 * n * n_columns; // of one matrix
		std::vector<uint32_t> words(set_words + 2 * end_words);
		std::memcpy(words.data(), sets, set_words * 4);
		if (end_words) {
			std::memcpy(words.data() + set_words, lo, end_words * 4);
			std::memcpy(words.data() + set_words + end_words, hi, end_words * 4);
		}
		UploadTables(nullptr, 0, words.data(), words.size());
		if (mode == VSS_BY_LABEL_GRAPH) {
			ProbeByLabelGraph(queries, n, k, ef, out_rowids, out_distances, out_counts, [&](Shard &s) {
				const uint32_t *d_words = bitmaps[s.bitmap].group_of;
				vss_label_predicate p = {};
				p.kind = VSS_LABEL_SET_BOX, p.set_column = set_column, p.set_width = set_width, p.n_columns = (uint32_t)n_columns;
				std::copy(columns, columns + n_columns, p.columns);
				p.d_sets = d_words;
				p.d_lo = end_words ? d_words + set_words : nullptr, p.d_hi = end_words ? d_words + set_words + end_words : nullptr;
				return p;
			});
			return;
		}
		Probe(
		    queries, n, k, out_rowids, out_distances, out_counts,
		    [&](Shard &s, row_t *keys, float *dist) {
			    const uint32_t *d_words = bitmaps[s.bitmap].group_of;
			    Vss(s, vss_search_batch_by_label_set_box_device(
			               s.index->Handle(), s.d_q, n, k, ef, set_column, reinterpret_cast<const uint64_t *>(d_words), set_width, columns, n_columns,
			               end_words ? reinterpret_cast<const uint64_t *>(d_words + set_words) : nullptr,
			               end_words ? reinterpret_cast<const uint64_t *>(d_words + set_words + end_words) : nullptr, mode, route_c, keys, dist,
			               s.d_cnt, s.d_route));
		    },
		    [&](Shard &s) { Vss(s, vss_synchronize(s.index->Handle())); });
		for (size_t g = 0; shard_routes && g != shards.size(); ++g) {
			Hip(hipSetDevice(shards[g].device), "hipSetDevice");
			Hip(hipMemcpy(shard_routes->data() + g * n, shards[g].d_route, n, hipMemcpyDeviceToHost), "copy routes");
		}
	}
	// Query q admits the live rows whose label is one of sets[q * width .. (q + 1) * width) (VSS_NO_LABEL pads a shorter list and
	// equals nothing; a VSS_NO_LABEL cell is in no set): vss_search_batch_by_label_set_device per shard, every shard holding the
	// whole column.  Modes, shard_routes, exchange and merge are SearchBatchByLabel's; the matrix travels as UploadTables' group
	// numbers, n * width words.
	void SearchBatchByLabelSet(const float *queries, idx_t n, idx_t k, idx_t ef, const uint32_t *sets, idx_t width, int mode, uint64_t route_c,
	                           row_t *out_rowids, float *out_distances, uint32_t *out_counts, std::vector<uint8_t> *shard_routes = nullptr) {
		if (shard_routes)
			shard_routes->assign(shards.size() * n, 0);
		if (!n || !k)
			return;
		if (width < 1 || width > VSS_LABEL_SET_MAX)
			throw InternalException("Failed to search the HNSW index: search by label set takes a width of 1 to 32 labels per query");
		if (!sets)
			throw InternalException("Failed to search the HNSW index: search by label set needs every query's row of labels");
		Ensure(n, k);
		UploadTables(nullptr, 0, sets, n * width);
		if (mode == VSS_BY_LABEL_GRAPH) {
			ProbeByLabelGraph(queries, n, k, ef, out_rowids, out_distances, out_counts, [&](Shard &s) {
				vss_label_predicate p = {};
				p.kind = VSS_LABEL_SET, p.set_width = (uint32_t)width, p.d_sets = bitmaps[s.bitmap].group_of;
				return p;
			});
			return;
		}
		Probe(
		    queries, n, k, out_rowids, out_distances, out_counts,
		    [&](Shard &s, row_t *keys, float *dist) {
			    Vss(s, vss_search_batch_by_label_set_device(s.index->Handle(), s.d_q, n, k, ef, bitmaps[s.bitmap].group_of, width, mode,
			                                                route_c, keys, dist, s.d_cnt, s.d_route));
		    },
		    [&](Shard &s) { Vss(s, vss_synchronize(s.index->Handle())); });
		for (size_t g = 0; shard_routes && g != shards.size(); ++g) {
			Hip(hipSetDevice(shards[g].device), "hipSetDevice");
			Hip(hipMemcpy(shard_routes->data() + g * n, shards[g].d_route, n, hipMemcpyDeviceToHost), "copy routes");
		}
	}

private:
	// A table of per-query predicates, refused here before any device is touched: the rules of csrc/filter_groups.h in this
	// layer's words.  An unknown group is reported ahead of a table too large to exist, as it always was.
	static void CheckTables(const uint64_t *allowed, idx_t n_groups, idx_t n_bits, const uint32_t *group_of, bool group_of_required,
	                        idx_t n) {
		using vss::host::FilterTableFault;
		const std::string failed = "Failed to search the HNSW index: ";
		const FilterTableFault fault = vss::host::check_filter_table(allowed, n_groups, n_bits, group_of, group_of_required);
		if (fault != FilterTableFault::NONE && fault != FilterTableFault::TOO_LARGE)
			throw InternalException(failed + "filtered search needs " +
			                        (fault == FilterTableFault::NO_GROUPS          ? "at least one group"
			                         : fault == FilterTableFault::NO_GROUP_NUMBERS ? "the group of every query"
			                                                                       : "the groups' row-id bitmaps"));
		const uint64_t bad = group_of ? vss::host::first_unknown_group(group_of, n, n_groups) : vss::host::NO_BAD_GROUP;
		if (bad != vss::host::NO_BAD_GROUP)
			throw InternalException(failed + "query " + std::to_string(bad) + " names group " + std::to_string(group_of[bad]) +
			                        ", the table holds " + std::to_string(n_groups));
		if (fault == FilterTableFault::TOO_LARGE)
			throw InternalException(failed + std::to_string(n_groups) + " groups of " + std::to_string(n_bits) +
			                        " bits are more than a table can hold");
	}

	// `words` bitmap words and, where the call has them, the group numbers of n queries to every device that holds a shard (once
	// per device, not once per shard).  A slot grows by "allocate, then free": a failed allocation leaves it as it was.
	void UploadTables(const uint64_t *allowed, idx_t words, const uint32_t *group_of, idx_t n) {
		auto grow = [](auto *&p, idx_t &capacity, idx_t want) {
			if (capacity >= want)
				return;
			std::remove_reference_t<decltype(p)> grown = nullptr;
			Hip(hipMalloc((void **)&grown, want * sizeof *p), "hipMalloc");
			(void)hipFree(p);
			p = grown, capacity = want;
		};
		for (auto &b : bitmaps) {
			Hip(hipSetDevice(b.device), "hipSetDevice");
			grow(b.words, b.capacity, std::max<idx_t>(words, 1));
			if (group_of)
				grow(b.group_of, b.group_capacity, n);
			if (words) // (none: SearchBatchByLabel brings wanted labels only)
				Hip(hipMemcpy(b.words, allowed, words * sizeof(uint64_t), hipMemcpyHostToDevice), "copy bitmaps");
			if (group_of)
				Hip(hipMemcpy(b.group_of, group_of, n * sizeof(uint32_t), hipMemcpyHostToDevice), "copy groups");
		}
	}

	// A filtered probe through the engine's _begin form: `begin(shard, keys, dist)` starts a shard, vss_search_batch_end finishes it.
	template <class Begin>
	void ProbeThroughBegin(const float *queries, idx_t n, idx_t k, row_t *out_rowids, float *out_distances, uint32_t *out_counts,
	                       Begin begin) {
		try {
			Probe(queries, n, k, out_rowids, out_distances, out_counts, begin,
			      [&](Shard &s) { Vss(s, vss_search_batch_end(s.index->Handle(), 0)); });
		} catch (...) {
			DrainProbes();
			throw;
		}
	}
	// Mode VSS_BY_LABEL_GRAPH of the six calls by label: `predicate(shard)` names the shard's uploaded words, every shard is started
	// through vss_search_by_label_device_begin before the first is waited for — all G walk at once, as under a bitmap — and
	// vss_search_batch_end finishes each.  Every query walks in every shard: shard_routes stays all 0.
	template <class Predicate>
	void ProbeByLabelGraph(const float *queries, idx_t n, idx_t k, idx_t ef, row_t *out_rowids, float *out_distances, uint32_t *out_counts,
	                       Predicate predicate) {
		ProbeThroughBegin(queries, n, k, out_rowids, out_distances, out_counts, [&](Shard &s, row_t *keys, float *dist) {
			const vss_label_predicate p = predicate(s);
			Vss(s, vss_search_by_label_device_begin(s.index->Handle(), 0, s.d_q, n, k, ef, &p, keys, dist, s.d_cnt));
		});
	}
	// An error between launch and finish of a filtered probe: every shard's probe is completed and its stream drained before the
	// error leaves the call, so that no kernel (and no re-run round of vss_search_batch_end) still reads the tables in bitmaps[]
	// when a later call grows or frees them, and context 0 of every shard is free again.
	void DrainProbes() noexcept {
		for (auto &s : shards) {
			(void)hipSetDevice(s.device);
			(void)vss_search_batch_end(s.index->Handle(), 0);
			(void)hipStreamSynchronize(s.stream);
		}
	}

	// One probe: `launch(shard, keys, dist)` starts (or runs) the shard's search of the uploaded batch into the given device
	// cells, `finish(shard)` returns when they are valid; the answers are exchanged and merged, results to the host.
	template <class Launch, class Finish>
	void Probe(const float *queries, idx_t n, idx_t k, row_t *out_rowids, float *out_distances, uint32_t *out_counts,
	           Launch launch, Finish finish) {
		const size_t G = shards.size();
		if (!comms.empty()) {
			ProbeRccl(queries, n, k, out_rowids, out_distances, out_counts, launch, finish);
			return;
		}
		// 1. the batch goes to every device and every shard starts searching (asynchronous: own stream per shard)
		UploadThenLaunch(queries, n, [&](Shard &s) { launch(s, s.d_keys, s.d_dist); });
		// 2. as each shard finishes, its block travels to the merging device (shard 0's)
		for (size_t g = 0; g != G; ++g) {
			Shard &s = shards[g];
			finish(s);
			Hip(hipSetDevice(shards[0].device), "hipSetDevice");
			Hip(hipMemcpyPeerAsync(m_dist + g * n * k, shards[0].device, s.d_dist, s.device, n * k * sizeof(float),
			                       shards[0].stream),
			    "peer copy");
			Hip(hipMemcpyPeerAsync(m_keys + g * n * k, shards[0].device, s.d_keys, s.device, n * k * sizeof(row_t),
			                       shards[0].stream),
			    "peer copy");
		}
		// 3. k-way merge on the merging device, results to the host
		if (vss_merge_topk_device(m_dist, m_keys, G, n, k, o_dist, o_keys, o_cnt, shards[0].stream) != VSS_OK)
			throw InternalException("Failed to merge the shard results");
		Hip(hipMemcpyAsync(out_rowids, o_keys, n * k * sizeof(row_t), hipMemcpyDeviceToHost, shards[0].stream), "copy out");
		if (out_distances)
			Hip(hipMemcpyAsync(out_distances, o_dist, n * k * sizeof(float), hipMemcpyDeviceToHost, shards[0].stream),
			    "copy out");
		if (out_counts)
			Hip(hipMemcpyAsync(out_counts, o_cnt, n * sizeof(uint32_t), hipMemcpyDeviceToHost, shards[0].stream),
			    "copy out");
		Hip(hipStreamSynchronize(shards[0].stream), "sync");
	}

	// The probe with every shard on a device of its own: the engine writes a shard's answers straight into its block of
	// the packed exchange (row ids, then distances), one grouped RCCL all-gather leaves all G blocks on every device, the
	// merging device (shard 0's) runs the packed k-way merge.
	template <class Launch, class Finish>
	void ProbeRccl(const float *queries, idx_t n, idx_t k, row_t *out_rowids, float *out_distances, uint32_t *out_counts,
	               Launch launch, Finish finish) {
		const size_t G = shards.size();
		const uint64_t block = vss_packed_block_bytes(n, k);
		UploadThenLaunch(queries, n, [&](Shard &s) {
			row_t *keys = reinterpret_cast<row_t *>(s.d_block);
			float *dist = reinterpret_cast<float *>(s.d_block + n * k * sizeof(row_t));
			launch(s, keys, dist);
		});
		for (auto &s : shards)
			finish(s);
		// ONE grouped all-gather (not G gathers to the merging device): the blocks are small — 12 bytes x n x k per shard, 120 KiB
		// at n = 1024, k = 10 — so the exchange is bound by the latency of its ring steps, which a gather to one root over
		// point-to-point xGMI links does not have fewer of; and every device ends up able to merge, which is what the
		// multi-process host (sharded.py, one rank per GPU, every rank answering its own caller) needs anyway.
		// The group is closed on every path (an open ncclGroup would poison the process), and no shard stream is left with
		// work that still names d_block / d_gathered when an error leaves this frame.
		{
			Xchg(vss_exchange_group_begin());
			int rc = VSS_OK;
			for (size_t g = 0; g != G && rc == VSS_OK; ++g)
				rc = vss_exchange_allgather(comms[g], shards[g].d_block, shards[g].d_gathered, block, shards[g].stream);
			const int rc_end = vss_exchange_group_end();
			if (rc != VSS_OK || rc_end != VSS_OK) {
				const std::string why = vss_exchange_last_error();
				for (auto &s : shards) {
					(void)hipSetDevice(s.device);
					(void)hipStreamSynchronize(s.stream);
				}
				throw InternalException("Failed to exchange the shard results: " + why);
			}
		}
		Hip(hipSetDevice(shards[0].device), "hipSetDevice");
		if (vss_merge_topk_packed_device(shards[0].d_gathered, G, n, k, o_dist, o_keys, o_cnt, shards[0].stream) != VSS_OK)
			throw InternalException("Failed to merge the shard results");
		Hip(hipMemcpyAsync(out_rowids, o_keys, n * k * sizeof(row_t), hipMemcpyDeviceToHost, shards[0].stream), "copy out");
		if (out_distances)
			Hip(hipMemcpyAsync(out_distances, o_dist, n * k * sizeof(float), hipMemcpyDeviceToHost, shards[0].stream),
			    "copy out");
		if (out_counts)
			Hip(hipMemcpyAsync(out_counts, o_cnt, n * sizeof(uint32_t), hipMemcpyDeviceToHost, shards[0].stream),
			    "copy out");
		for (auto &s : shards) { // every rank's part of the collective has retired before the blocks are reused
			Hip(hipSetDevice(s.device), "hipSetDevice");
			Hip(hipStreamSynchronize(s.stream), "sync");
		}
	}
	// The batch goes to every device and every shard starts searching — in three sweeps, so that with G real devices nothing
	// one shard does holds back the next: (1) all G uploads are issued (asynchronous copies, each on its shard's stream),
	// (2) each is waited for once (the engine launches on the index's own stream, so the copy has to have landed), (3) all G
	// launches are issued back to back.  (Round 4 ran upload -> wait -> launch per shard: G serialised uploads.)
	template <class Launch>
	void UploadThenLaunch(const float *queries, idx_t n, Launch launch) {
		for (auto &s : shards) {
			Hip(hipSetDevice(s.device), "hipSetDevice");
			Hip(hipMemcpyAsync(s.d_q, queries, n * dim * sizeof(float), hipMemcpyHostToDevice, s.stream), "copy queries");
		}
		for (auto &s : shards) {
			Hip(hipSetDevice(s.device), "hipSetDevice");
			Hip(hipStreamSynchronize(s.stream), "sync");
		}
		for (auto &s : shards) {
			Hip(hipSetDevice(s.device), "hipSetDevice");
			launch(s);
		}
	}
	static void Xchg(int rc) {
		if (rc != VSS_OK)
			throw InternalException(std::string("Failed to exchange the shard results: ") + vss_exchange_last_error());
	}

	// rows [begin, end) of a chunk owned by one shard, with the validity words of the run re-based to bit 0 (when the chunk
	// has a validity mask).  Row ids of a scan chunk are ascending, so a chunk normally is one run, two at a boundary.
	struct Run {
		idx_t owner, begin, end;
		std::vector<uint64_t> validity;
	};
	std::vector<Run> CutIntoRuns(const row_t *rowid_data, const uint64_t *validity, idx_t count) const {
		std::vector<Run> runs;
		for (idx_t i = 0; i < count;) {
			const idx_t g = OwnerOf(rowid_data[i]);
			idx_t j = i + 1;
			while (j < count && OwnerOf(rowid_data[j]) == g)
				j++;
			Run run {g, i, j, {}};
			if (validity) {
				run.validity.assign((j - i + 63) / 64, 0);
				for (idx_t r = i; r != j; ++r)
					if ((validity[r >> 6] >> (r & 63)) & 1)
						run.validity[(r - i) >> 6] |= 1ull << ((r - i) & 63);
			}
			runs.push_back(std::move(run));
			i = j;
		}
		return runs;
	}

	// the linked-block writer / reader of HNSWIndex::PersistToBlocks / LoadFromBlocks, shared by the header and all G streams
	struct BlockWriter {
		std::vector<std::vector<uint8_t>> blocks;
		idx_t payload;
		uint64_t written;
		void Write(const uint8_t *p, uint64_t size) {
			written += size;
			while (size) {
				if (blocks.empty() || blocks.back().size() == payload)
					blocks.emplace_back();
				const idx_t take = std::min<idx_t>(size, payload - blocks.back().size());
				blocks.back().insert(blocks.back().end(), p, p + take);
				p += take;
				size -= take;
			}
		}
		static int Callback(void *ctx, const void *data, uint64_t size) {
			static_cast<BlockWriter *>(ctx)->Write(static_cast<const uint8_t *>(data), size);
			return 1;
		}
	};
	struct BlockReader {
		const std::vector<std::vector<uint8_t>> *blocks;
		size_t block, off;
		uint64_t limit = 0; // bytes left of the stream a shard is loading: vss_load may not read past them
		size_t Read(uint8_t *p, size_t size) { // returns the bytes copied: fewer than `size` where the blocks end
			size_t done = 0;
			while (done != size && block < blocks->size()) {
				const auto &b = (*blocks)[block];
				const size_t take = std::min<size_t>(size - done, b.size() - off);
				if (take)
					std::memcpy(p + done, b.data() + off, take);
				done += take, off += take;
				if (off == b.size())
					block++, off = 0;
			}
			return done;
		}
		static int Callback(void *ctx, void *data, uint64_t size) {
			auto &r = *static_cast<BlockReader *>(ctx);
			if (size > r.limit || r.Read(static_cast<uint8_t *>(data), size) != size)
				return 0;
			r.limit -= size;
			return 1;
		}
	};

	struct DeviceBitmap { // the row-id bitmap of a filtered probe on one device
		int device;
		uint64_t *words;
		idx_t capacity;
		uint32_t *group_of = nullptr; // SearchBatchFilteredGroups: the group of every query of the batch
		idx_t group_capacity = 0;
	};

	struct Shard {
		int device = 0;
		idx_t lo = 0, hi = 0;
		size_t bitmap = 0; // slot of this shard's device in `bitmaps`
		std::unique_ptr<HNSWIndex> index;
		hipStream_t stream = nullptr;
		float *d_q = nullptr, *d_dist = nullptr;
		row_t *d_keys = nullptr;
		uint32_t *d_cnt = nullptr;
		uint8_t *d_route = nullptr; // SearchBatchFilteredGroupsAuto: this shard's route of every query
		unsigned char *d_block = nullptr, *d_gathered = nullptr; // RCCL exchange: this shard's packed block, all G blocks
		void Release() {
			if (!stream)
				return;
			(void)hipSetDevice(device);
			(void)hipFree(d_q), (void)hipFree(d_dist), (void)hipFree(d_keys), (void)hipFree(d_cnt), (void)hipFree(d_route);
			(void)hipFree(d_block), (void)hipFree(d_gathered);
			(void)hipStreamDestroy(stream);
			stream = nullptr;
		}
	};

	static void Hip(hipError_t e, const char *what) {
		if (e != hipSuccess)
			throw InternalException(std::string("HIP error in ") + what + ": " + hipGetErrorString(e));
	}
	static void Vss(Shard &s, int rc) {
		if (rc != VSS_OK)
			throw InternalException(std::string("Failed to search the HNSW index: ") + vss_last_error(s.index->Handle()));
	}

	// per-shard and merge buffers for batches of up to n queries x k results
	void Ensure(idx_t n, idx_t k) {
		if (n <= cap_n && k <= cap_k)
			return;
		cap_n = std::max(cap_n, n), cap_k = std::max(cap_k, k);
		for (auto &s : shards) {
			Hip(hipSetDevice(s.device), "hipSetDevice");
			if (!s.stream)
				Hip(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking), "stream");
			(void)hipFree(s.d_q), (void)hipFree(s.d_dist), (void)hipFree(s.d_keys), (void)hipFree(s.d_cnt), (void)hipFree(s.d_route);
			Hip(hipMalloc((void **)&s.d_q, cap_n * dim * sizeof(float)), "hipMalloc");
			Hip(hipMalloc((void **)&s.d_dist, cap_n * cap_k * sizeof(float)), "hipMalloc");
			Hip(hipMalloc((void **)&s.d_keys, cap_n * cap_k * sizeof(row_t)), "hipMalloc");
			Hip(hipMalloc((void **)&s.d_cnt, cap_n * sizeof(uint32_t)), "hipMalloc");
			Hip(hipMalloc((void **)&s.d_route, cap_n), "hipMalloc");
			if (!comms.empty()) {
				(void)hipFree(s.d_block), (void)hipFree(s.d_gathered);
				const uint64_t block = vss_packed_block_bytes(cap_n, cap_k);
				Hip(hipMalloc((void **)&s.d_block, block), "hipMalloc");
				Hip(hipMalloc((void **)&s.d_gathered, block * shards.size()), "hipMalloc");
			}
		}
		Hip(hipSetDevice(shards[0].device), "hipSetDevice");
		(void)hipFree(m_dist), (void)hipFree(m_keys), (void)hipFree(o_dist), (void)hipFree(o_keys), (void)hipFree(o_cnt);
		const size_t G = shards.size();
		Hip(hipMalloc((void **)&m_dist, G * cap_n * cap_k * sizeof(float)), "hipMalloc");
		Hip(hipMalloc((void **)&m_keys, G * cap_n * cap_k * sizeof(row_t)), "hipMalloc");
		Hip(hipMalloc((void **)&o_dist, cap_n * cap_k * sizeof(float)), "hipMalloc");
		Hip(hipMalloc((void **)&o_keys, cap_n * cap_k * sizeof(row_t)), "hipMalloc");
		Hip(hipMalloc((void **)&o_cnt, cap_n * sizeof(uint32_t)), "hipMalloc");
	}

	idx_t dim, n_total;
	OptionMap options; // what a reload creates its fresh shards with
	std::vector<Shard> shards;
	std::vector<DeviceBitmap> bitmaps; // one per distinct device
	std::vector<vss_comm *> comms; // one per shard when every shard has its own device and RCCL is available, else empty
	idx_t cap_n = 0, cap_k = 0;
	float *m_dist = nullptr, *o_dist = nullptr; // on shards[0].device
	row_t *m_keys = nullptr, *o_keys = nullptr;
	uint32_t *o_cnt = nullptr;
};

} // namespace vss_host
