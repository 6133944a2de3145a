// exact_filtered_check.cpp — the host plan and the admission rule of vss_search_exact_batch_filtered_groups
// (csrc/exact_filtered_plan.h) as a stand-alone program: pure C++, no GPU.  The listing kernels run exact_filter_admits itself,
// vss_engine.hip carries exact_filter_order / exact_filter_pack out.  tests/test_exact_filtered_plan.py builds this again under
// the address and undefined-behaviour sanitizers.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/exact_filtered_plan.h"

using namespace vss::host;

static int failures = 0;
#define CHECK(cond)                                                                                                    \
	do {                                                                                                               \
		if (!(cond)) {                                                                                                 \
			std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                                              \
			++failures;                                                                                                \
		}                                                                                                              \
	} while (0)

// ---- admission: the rule as a sentence, against the function, on the keys where it can go wrong
static void check_admission() {
	for (uint64_t n_bits : {uint64_t(0), uint64_t(1), uint64_t(63), uint64_t(64), uint64_t(65), uint64_t(127), uint64_t(128),
	                        uint64_t(129), uint64_t(1000)}) {
		const uint64_t words = filter_group_words(n_bits);
		// two groups end to end: group 0 all ones INCLUDING its padding bits, group 1 all zeros behind it (one spare word so that
		// n_bits == 0 still has something to point at)
		std::vector<uint64_t> table(2 * words + 1, 0);
		for (uint64_t w = 0; w != words; ++w)
			table[w] = ~uint64_t(0);
		const uint64_t *ones = table.data(), *zeros = table.data() + words;
		const int64_t probes[] = {-1, INT64_MIN, INT64_MAX, INT64_MAX - 1, 0, 1, 62, 63, 64, 65, (int64_t)n_bits - 1, (int64_t)n_bits,
		                          (int64_t)n_bits + 1, (int64_t)(words * 64) - 1, (int64_t)(words * 64)};
		for (int64_t key : probes) {
			const bool in_range = key >= 0 && (uint64_t)key < n_bits; // (INT64_MAX, the free key, is never below an n_bits we can hold)
			CHECK(exact_filter_admits(key, ones, n_bits) == in_range);
			CHECK(!exact_filter_admits(key, zeros, n_bits));
		}
		// a padding bit of group 0 — set — admits nothing, whatever follows it
		if (n_bits % 64)
			CHECK(!exact_filter_admits((int64_t)n_bits, ones, n_bits) && !exact_filter_admits((int64_t)(words * 64 - 1), ones, n_bits));
		// single bits
		for (uint64_t bit = 0; bit < n_bits; bit += (n_bits > 130 ? 37 : 1)) {
			std::vector<uint64_t> one(words, 0);
			one[bit >> 6] = uint64_t(1) << (bit & 63);
			for (uint64_t key = 0; key < n_bits; ++key)
				CHECK(exact_filter_admits((int64_t)key, one.data(), n_bits) == (key == bit));
		}
	}
	// the free key is rejected even where a table could name it
	static_assert(!exact_filter_admits(EXACT_FILTER_FREE_KEY, nullptr, ~uint64_t(0)), "free key");
	static_assert(!exact_filter_admits(-1, nullptr, ~uint64_t(0)), "negative key");
}

// ---- the plan's invariants, whatever the input
static void check_plan(const std::vector<uint32_t> &group_of, bool null_groups, uint64_t n_groups, const std::vector<uint32_t> &len_of_group,
                       uint64_t budget, uint32_t qt) {
	const uint64_t nq = group_of.size();
	ExactFilterPlan p;
	exact_filter_order(null_groups ? nullptr : group_of.data(), nq, n_groups, p);
	auto group = [&](uint64_t q) { return null_groups ? 0u : group_of[q]; };
	// order: a permutation; the known queries first, by (group, query); the unknown ones behind, in query order
	CHECK(p.order.size() == nq);
	std::vector<int> seen(nq, 0);
	for (uint32_t q : p.order) {
		CHECK(q < nq);
		if (q < nq)
			++seen[q];
	}
	for (uint64_t q = 0; q != nq; ++q)
		CHECK(seen[q] == 1);
	uint64_t known = 0, first_unknown = NO_BAD_GROUP;
	for (uint64_t q = 0; q != nq; ++q) {
		if (group(q) < n_groups)
			++known;
		else if (first_unknown == NO_BAD_GROUP)
			first_unknown = q;
	}
	CHECK(p.n_known == known && p.first_unknown == first_unknown);
	if (!null_groups) // the report the host form refuses the call with
		CHECK(p.first_unknown == first_unknown_group(group_of.data(), nq, n_groups));
	for (uint64_t t = 0; t + 1 < nq; ++t) {
		const uint32_t a = p.order[t], b = p.order[t + 1];
		if (t + 1 < known)
			CHECK(group(a) < group(b) || (group(a) == group(b) && a < b));
		else if (t >= known)
			CHECK(a < b && group(a) >= n_groups && group(b) >= n_groups);
	}
	// groups in use: ascending, each with at least one query, exactly the groups the known queries name
	CHECK(p.group_query.size() == p.groups.size() + 1 && p.group_query.front() == 0 && p.group_query.back() == known);
	for (size_t u = 0; u != p.groups.size(); ++u) {
		CHECK(p.group_query[u] < p.group_query[u + 1]);
		CHECK(u == 0 || p.groups[u - 1] < p.groups[u]);
		for (uint32_t t = p.group_query[u]; t != p.group_query[u + 1]; ++t)
			CHECK(group(p.order[t]) == p.groups[u]);
	}
	// pack
	std::vector<uint32_t> lengths(p.groups.size());
	for (size_t u = 0; u != p.groups.size(); ++u)
		lengths[u] = len_of_group[p.groups[u] % len_of_group.size()];
	exact_filter_pack(lengths.data(), budget, qt, p);
	uint64_t listed = 0, distances = 0;
	std::vector<int> in_tile(nq, 0);
	uint32_t next_group = 0, next_tile = 0;
	for (const ExactFilterPass &pass : p.passes) {
		CHECK(pass.group_begin == next_group && pass.group_end > pass.group_begin && pass.tile_begin == next_tile);
		CHECK(pass.query_begin == p.group_query[pass.group_begin] && pass.query_end == p.group_query[pass.group_end]);
		uint64_t entries = 0;
		uint32_t longest = 0;
		for (uint32_t u = pass.group_begin; u != pass.group_end; ++u) {
			CHECK(p.list_base[u] == entries); // lists end to end, in group order
			entries += lengths[u];
			longest = lengths[u] > longest ? lengths[u] : longest;
		}
		CHECK(entries == pass.entries && longest == pass.longest);
		// the bound: within the budget — or one group alone, which the caller promises is never longer than the budget
		CHECK(pass.entries <= budget || pass.group_end == pass.group_begin + 1);
		// greedy: the next group would not have fitted
		if (pass.group_end < p.groups.size())
			CHECK(pass.entries + lengths[pass.group_end] > budget);
		for (uint32_t i = pass.tile_begin; i != pass.tile_end; ++i) {
			const ExactFilterTile &t = p.tiles[i];
			CHECK(t.n_queries >= 1 && t.n_queries <= qt && t.list_length > 0);
			CHECK(t.first_query >= pass.query_begin && t.first_query + t.n_queries <= pass.query_end);
			CHECK(t.list_offset + (uint64_t)t.list_length <= pass.entries);
			for (uint32_t q = t.first_query; q != t.first_query + t.n_queries; ++q) {
				++in_tile[q];
				CHECK(group(p.order[q]) == t.group); // no tile spans two groups
				CHECK(p.query_offset[q] == t.list_offset && p.query_length[q] == t.list_length);
			}
		}
		next_group = pass.group_end, next_tile = pass.tile_end;
	}
	CHECK(next_group == p.groups.size() && next_tile == p.tiles.size());
	for (size_t u = 0; u != p.groups.size(); ++u) {
		listed += lengths[u];
		distances += (uint64_t)lengths[u] * (p.group_query[u + 1] - p.group_query[u]);
		for (uint32_t t = p.group_query[u]; t != p.group_query[u + 1]; ++t) {
			CHECK(in_tile[t] == (lengths[u] ? 1 : 0)); // every known query with rows to score is in exactly one tile
			CHECK(p.query_length[t] == lengths[u]);
		}
	}
	for (uint64_t t = known; t != nq; ++t)
		CHECK(in_tile[t] == 0 && p.query_length[t] == 0);
	CHECK(p.listed == listed && p.distances == distances);
}

int main() {
	check_admission();
	uint64_t rng = 0x9E3779B97F4A7C15ull;
	auto next = [&] {
		rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
		return rng;
	};
	// the edges by hand
	check_plan({}, false, 4, {10}, 100, 8);                                   // no query
	check_plan({}, true, 0, {10}, 100, 8);
	check_plan({0}, false, 1, {0}, 100, 8);                                   // one query, an empty list
	check_plan({0, 0, 0}, true, 1, {70000}, 70000, 8);                        // no group numbers: bitmap 0
	check_plan({7, 7, 7}, true, 0, {5}, 100, 8);                              // ... and no table: every query unknown
	check_plan({3, 3, 3, 3, 3, 3, 3, 3, 3}, false, 4, {5}, 100, 8);           // MS_QT + 1 queries of one group
	check_plan({5, 4, 3, 2, 1, 0}, false, 6, {100}, 100, 8);                  // every outer row its own tenant, a pass each
	check_plan({5, 4, 3, 2, 1, 0}, false, 6, {100}, 1, 8);                    // every group alone exceeds the budget
	check_plan({2, 9, 2, 4000000000u, 0, 9}, false, 3, {40, 0, 60}, 100, 1);  // unknown groups in between
	check_plan({1999, 3, 1024, 3, 77, 500, 1999, 77}, false, 2000, {17, 0, 300}, 317, 2); // 5 of 2000 groups in use
	check_plan({0, 1}, false, 2, {4294967295u}, 4294967296ull, 8);            // lists of nearly 2^32 entries
	// and at random
	for (int round = 0; round != 400; ++round) {
		const uint64_t nq = next() % 70, n_groups = next() % 40, span = n_groups + (next() % 3 ? 0 : 3) + 1;
		std::vector<uint32_t> group_of(nq), lens(1 + next() % 9);
		for (auto &g : group_of)
			g = (uint32_t)(next() % span);
		uint32_t longest = 1;
		for (auto &l : lens) {
			l = next() % 4 ? (uint32_t)(next() % 5000) : 0;
			longest = l > longest ? l : longest;
		}
		const uint64_t budget = next() % 2 ? longest : longest + next() % 20000;
		check_plan(group_of, next() % 8 == 0, n_groups, lens, budget, 1 + (uint32_t)(next() % 8));
	}
	if (failures) {
		std::printf("%d check(s) failed\n", failures);
		return 1;
	}
	std::printf("exact filtered check ok\n");
	return 0;
}
