// range_filtered_plan.h — the host plan of vss_search_range_batch_by_label_box64: pure arithmetic, no HIP, so that it can be
// compiled and run on a CPU (tests/range_filtered_plan_probe.cpp, under the sanitizers).  vss_engine.hip only carries it out.
//
// exact_filtered_plan.h does the first half as it stands: exact_filter_order puts the queries in group order (a group = one
// distinct raw box of the call), exact_filter_pack packs the groups' lists of live admitted slots into passes and cuts every
// group's queries into tiles of at most RANGE_LIST_QT queries.  On top of that range_filter_plan cuts each pass into LAUNCHES of
// the gathered candidate tile (k_range_candidates_lists, exact_range_kernels.h) such that no launch can propose more pairs than
// the candidate buffer of the range search holds, RANGE_QUERY_BLOCK x RANGE_ROW_CHUNK cells.  A launch is
//   * the positions of ONE aligned block [b RANGE_QUERY_BLOCK, (b + 1) RANGE_QUERY_BLOCK) of the group order that lie in the
//     pass — a tile that spans a block boundary is cut in two there —
//   * times list positions [pos_begin, pos_end), at most RANGE_ROW_CHUNK of them, of every tile's own list.
// Its tiles hold at most RANGE_QUERY_BLOCK queries together and each of them meets at most RANGE_ROW_CHUNK list positions, so
// the bound holds by construction: no overflow path, nothing re-run.  A tile whose list ends before pos_begin is left out of
// the launch; a group without admitted rows has no tile at all (exact_filter_pack) and its queries keep their zero counts.
// Each tile runs in one of two shapes, chosen here: at most RANGE_LIST_SMALL_QUERIES queries -> the 32-query tile, else the
// 128-query tile.  A launch names its tiles of either shape through its own run of an index array.
#pragma once
#include "exact_filtered_plan.h"
#include "exact_range.h"

namespace vss {
namespace host {

constexpr uint32_t RANGE_LIST_QT = 128;           // queries of the tall tile: exact_filter_pack's qt
constexpr uint32_t RANGE_LIST_SMALL_QUERIES = 32; // a tile of at most this many queries takes the 32-query shape

struct RangeFilterLaunch {
	uint32_t pass;                   // of ExactFilterPlan::passes: its lists are in the list buffer while the launch runs
	uint32_t pos_begin, pos_end;     // of every tile's list
	uint32_t small_begin, small_end; // RangeFilterPlan::small
	uint32_t tall_begin, tall_end;   // RangeFilterPlan::tall
	uint64_t pairs;                  // (query, list position) pairs it scores
};

struct RangeFilterPlan {
	std::vector<ExactFilterTile> tiles; // ExactFilterPlan::tiles cut at the block boundaries (at most one per known query)
	std::vector<uint32_t> small, tall;  // indices into `tiles`, launch after launch
	std::vector<RangeFilterLaunch> launches;
	uint64_t pairs = 0, largest = 0;    // over all launches; the largest launch
};

// p: after exact_filter_order and exact_filter_pack(lengths, budget, RANGE_LIST_QT, p)
inline void range_filter_plan(const ExactFilterPlan &p, RangeFilterPlan &r, uint32_t query_block = RANGE_QUERY_BLOCK,
                              uint32_t row_chunk = RANGE_ROW_CHUNK) {
	r = RangeFilterPlan();
	for (size_t ps = 0; ps != p.passes.size(); ++ps) {
		const ExactFilterPass &pass = p.passes[ps];
		// the pass's tiles, cut at the block boundaries (they are in order of first_query)
		const size_t cut_begin = r.tiles.size();
		for (uint32_t t = pass.tile_begin; t != pass.tile_end; ++t) {
			ExactFilterTile tile = p.tiles[t];
			while (tile.n_queries) {
				const uint32_t room = query_block - tile.first_query % query_block;
				ExactFilterTile head = tile;
				head.n_queries = tile.n_queries < room ? tile.n_queries : room;
				r.tiles.push_back(head);
				tile.first_query += head.n_queries, tile.n_queries -= head.n_queries;
			}
		}
		// block after block: runs of cut tiles that share first_query / query_block
		for (size_t b0 = cut_begin, b1; b0 != r.tiles.size(); b0 = b1) {
			const uint32_t block = r.tiles[b0].first_query / query_block;
			uint32_t longest = 0;
			for (b1 = b0; b1 != r.tiles.size() && r.tiles[b1].first_query / query_block == block; ++b1)
				longest = r.tiles[b1].list_length > longest ? r.tiles[b1].list_length : longest;
			for (uint64_t pos = 0; pos < longest; pos += row_chunk) {
				RangeFilterLaunch l = {};
				l.pass = (uint32_t)ps, l.pos_begin = (uint32_t)pos;
				l.pos_end = (uint32_t)(pos + row_chunk < longest ? pos + row_chunk : longest);
				l.small_begin = (uint32_t)r.small.size(), l.tall_begin = (uint32_t)r.tall.size();
				for (size_t t = b0; t != b1; ++t) {
					const ExactFilterTile &tile = r.tiles[t];
					if (tile.list_length <= l.pos_begin)
						continue;
					(tile.n_queries <= RANGE_LIST_SMALL_QUERIES ? r.small : r.tall).push_back((uint32_t)t);
					const uint32_t end = tile.list_length < l.pos_end ? tile.list_length : l.pos_end;
					l.pairs += (uint64_t)tile.n_queries * (end - l.pos_begin);
				}
				l.small_end = (uint32_t)r.small.size(), l.tall_end = (uint32_t)r.tall.size();
				r.launches.push_back(l);
				r.pairs += l.pairs;
				r.largest = l.pairs > r.largest ? l.pairs : r.largest;
			}
		}
	}
}

} // namespace host
} // namespace vss
