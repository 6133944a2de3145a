// range_filtered_plan_probe.cpp — csrc/range_filtered_plan.h on the CPU (tests/test_range_filtered_plan.py builds it with the
// address and undefined-behaviour sanitizers).  For hand-picked layouts of groups (queries per group, rows per list): every (known
// query, list position) pair lies in exactly one launch; every launch stays within query_block x row_chunk pairs and states its
// true pair count; no tile spans a block boundary, and each tile sits in the index array of its shape.
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "../duckdb-vss_amd/csrc/range_filtered_plan.h"

using namespace vss;
using namespace vss::host;

#define REQUIRE(cond) \
	if (!(cond))      \
	std::exit((std::printf("%s: line %d: %s\n", what, __LINE__, #cond), 1))

struct Group {
	uint32_t queries, rows;
};

// unknown: queries of a group the table does not hold, mixed in; budget: list entries per pass
static void check(const char *what, const std::vector<Group> &groups, uint32_t unknown, uint64_t budget, uint32_t query_block,
                  uint32_t row_chunk) {
	std::vector<uint32_t> group_of, lengths_all;
	for (size_t g = 0; g != groups.size(); ++g) {
		group_of.insert(group_of.end(), groups[g].queries, (uint32_t)g);
		lengths_all.push_back(groups[g].rows);
	}
	for (uint32_t i = 0; i != unknown; ++i)
		group_of.insert(group_of.begin() + (i * 7) % (group_of.size() + 1), (uint32_t)groups.size() + i);
	ExactFilterPlan p;
	exact_filter_order(group_of.data(), group_of.size(), groups.size(), p);
	std::vector<uint32_t> lengths;
	for (uint32_t g : p.groups)
		lengths.push_back(lengths_all[g]);
	exact_filter_pack(lengths.data(), budget, RANGE_LIST_QT, p);
	RangeFilterPlan r;
	range_filter_plan(p, r, query_block, row_chunk);

	std::vector<std::vector<std::pair<uint32_t, uint32_t>>> covered(p.n_known); // per position: the runs of its list that launches score
	std::vector<int> in_small(r.tiles.size(), 0), in_tall(r.tiles.size(), 0);
	uint64_t pairs = 0, largest = 0;
	uint32_t last_pass = 0;
	for (const RangeFilterLaunch &l : r.launches) {
		REQUIRE(l.pass < p.passes.size() && l.pass >= last_pass); // pass after pass: one listing per pass
		last_pass = l.pass;
		REQUIRE(l.pos_begin < l.pos_end && l.pos_end - l.pos_begin <= row_chunk);
		REQUIRE(l.small_begin <= l.small_end && l.small_end <= r.small.size() && l.tall_begin <= l.tall_end && l.tall_end <= r.tall.size());
		REQUIRE(l.small_end - l.small_begin + l.tall_end - l.tall_begin > 0);
		uint64_t here = 0, queries = 0;
		uint32_t block = UINT32_MAX;
		for (int shape = 0; shape != 2; ++shape)
			for (uint32_t i = shape ? l.tall_begin : l.small_begin; i != (shape ? l.tall_end : l.small_end); ++i) {
				const uint32_t ti = shape ? r.tall[i] : r.small[i];
				REQUIRE(ti < r.tiles.size());
				(shape ? in_tall : in_small)[ti]++;
				const ExactFilterTile &t = r.tiles[ti];
				REQUIRE(shape == (t.n_queries > RANGE_LIST_SMALL_QUERIES) && t.n_queries <= RANGE_LIST_QT);
				REQUIRE(t.first_query >= p.passes[l.pass].query_begin && t.first_query + t.n_queries <= p.passes[l.pass].query_end);
				REQUIRE(block == UINT32_MAX || block == t.first_query / query_block);
				block = t.first_query / query_block;
				REQUIRE(t.list_length > l.pos_begin);
				const uint32_t end = t.list_length < l.pos_end ? t.list_length : l.pos_end;
				here += (uint64_t)t.n_queries * (end - l.pos_begin), queries += t.n_queries;
				for (uint32_t q = t.first_query; q != t.first_query + t.n_queries; ++q)
					covered[q].push_back({l.pos_begin, end});
			}
		REQUIRE(here == l.pairs && queries <= query_block && here <= (uint64_t)query_block * row_chunk);
		pairs += here, largest = here > largest ? here : largest;
	}
	REQUIRE(pairs == r.pairs && pairs == p.distances && largest == r.largest);
	for (size_t ti = 0; ti != r.tiles.size(); ++ti) {
		const ExactFilterTile &t = r.tiles[ti];
		REQUIRE(t.n_queries >= 1 && t.first_query / query_block == (t.first_query + t.n_queries - 1) / query_block);
		REQUIRE((in_small[ti] == 0) != (in_tall[ti] == 0));
		for (uint32_t q = t.first_query; q != t.first_query + t.n_queries; ++q)
			REQUIRE(p.query_offset[q] == t.list_offset && p.query_length[q] == t.list_length);
	}
	for (size_t q = 0; q != p.n_known; ++q) { // the runs are made in ascending order: they must tile [0, length) exactly
		uint32_t at = 0;
		for (const auto &run : covered[q]) {
			REQUIRE(run.first == at && run.second > at);
			at = run.second;
		}
		REQUIRE(at == p.query_length[q]);
	}
	std::printf("%s: %zu tiles (%zu small, %zu tall entries), %zu launches, %llu pairs\n", what, r.tiles.size(), r.small.size(), r.tall.size(),
	            r.launches.size(), (unsigned long long)r.pairs);
}

int main() {
	// the shapes of the GPU test: groups of 1, 32 and 33 queries and more, one list longer than a chunk, an empty group
	check("test layout", {{1, 1}, {32, 4300}, {33, 8600}, {60, 0}, {3, 7}}, 0, 1u << 23, RANGE_QUERY_BLOCK, RANGE_ROW_CHUNK);
	// tiles that meet the block boundary from both sides; lists of exactly one chunk, one more, two
	check("block edges", {{1000, 8192}, {24, 8193}, {130, 16384}, {1, 5}, {2047, 3}}, 5, 1u << 23, RANGE_QUERY_BLOCK, RANGE_ROW_CHUNK);
	// small blocks and chunks: every cut at once, several passes (a budget of 40 entries), unknown groups mixed in
	check("small blocks", {{5, 17}, {9, 16}, {1, 0}, {300, 33}, {7, 1}, {129, 40}, {33, 15}}, 11, 40, 8, 16);
	check("one query block", {{128, 100}, {129, 100}, {32, 100}}, 0, 1000, 1024, 64);
	check("nothing listed", {{4, 0}, {1, 0}}, 2, 100, 8, 16);
	check("no queries", {}, 0, 100, 8, 16);
	std::printf("range filtered plan ok\n");
	return 0;
}
