// filter_groups_check.cpp — the group table of vss_search_batch_filtered_groups on a CPU: the engine's own arithmetic and
// validation (csrc/filter_groups.h: the words of a group, whether a table fits, the first rule a table's description breaks, the
// first query of an unknown group — the very functions vss_engine.hip and sharded_index.hpp call) and the host's packing of a correlated join chunk (filter_group_tables.hpp).  How the
// KERNELS read a bitmap is not restated here: tests/test_gpu_filter_groups.py checks that on the device.  A
// stand-alone program: no HIP, no GPU; tests/test_gpu_filter_groups_host.py builds it under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>

#include "../csrc/filter_groups.h"
#include "filter_group_tables.hpp"

using namespace vss_host;
using namespace vss::host;

#define EXPECT(cond)                                                                                                   \
	do {                                                                                                               \
		if (!(cond)) {                                                                                                 \
			std::fprintf(stderr, "CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                               \
			std::exit(1);                                                                                              \
		}                                                                                                              \
	} while (0)

int main() {
	// words per group, the wrap at the top of the range included
	EXPECT(filter_group_words(0) == 0 && filter_group_words(1) == 1 && filter_group_words(63) == 1);
	EXPECT(filter_group_words(64) == 1 && filter_group_words(65) == 2 && filter_group_words(7997) == 125);
	EXPECT(filter_group_words(~uint64_t(0)) == (uint64_t(1) << 58));
	EXPECT(filter_group_table_fits(16, 1000000) && filter_group_table_fits(0xFFFFFFFFull, 0));
	EXPECT(!filter_group_table_fits(uint64_t(1) << 40, uint64_t(1) << 40));

	// validation: the FIRST query of an unknown group
	const uint32_t groups[6] = {0, 2, 1, 3, 7, 3};
	EXPECT(first_unknown_group(groups, 6, 8) == NO_BAD_GROUP && first_unknown_group(groups, 0, 1) == NO_BAD_GROUP);
	EXPECT(first_unknown_group(groups, 6, 3) == 3 && first_unknown_group(groups, 6, 7) == 4);
	EXPECT(first_unknown_group(groups, 3, 3) == NO_BAD_GROUP && first_unknown_group(groups, 6, 0) == 0);

	// validation of a table's description: the FIRST rule it breaks, in the order no bitmaps, no group numbers, no groups,
	// too large (nothing is dereferenced: any non-null address stands for a table)
	{
		using F = FilterTableFault;
		const uint64_t bitmaps[1] = {0}, *const B = bitmaps, *const NO_B = nullptr;
		const uint32_t *const G = groups, *const NO_G = nullptr;
		const uint64_t two_32 = uint64_t(1) << 32, two_40 = uint64_t(1) << 40;
		const struct {
			const uint64_t *allowed;
			uint64_t n_groups, n_bits;
			const uint32_t *group_of;
			bool required;
			F expected;
		} cases[] = {
		    {B, 3, 1000, G, true, F::NONE},
		    {B, 3, 1000, G, false, F::NONE},
		    // each rule alone
		    {NO_B, 3, 1000, G, true, F::NO_BITMAPS},
		    {B, 3, 1000, NO_G, true, F::NO_GROUP_NUMBERS},
		    {B, 0, 1000, G, true, F::NO_GROUPS},
		    {B, two_40, two_40, G, true, F::TOO_LARGE}, // 2^40 groups of 2^34 words: does not fit
		    // group numbers optional: their absence is no fault, and the rules after it still hold
		    {B, 3, 1000, NO_G, false, F::NONE},
		    {NO_B, 3, 1000, NO_G, false, F::NO_BITMAPS},
		    {B, 0, 1000, NO_G, false, F::NO_GROUPS},
		    {B, two_40, two_40, NO_G, false, F::TOO_LARGE},
		    // two rules broken at once: the first in the order is reported
		    {NO_B, 3, 1000, NO_G, true, F::NO_BITMAPS},
		    {NO_B, 0, 1000, G, true, F::NO_BITMAPS},
		    {NO_B, two_32, 1000, G, true, F::NO_BITMAPS},
		    {B, 0, 1000, NO_G, true, F::NO_GROUP_NUMBERS},
		    {B, two_32, 1000, NO_G, true, F::NO_GROUP_NUMBERS},
		    {B, 0, ~uint64_t(0), G, true, F::NO_GROUPS}, // (no groups of any width: not "too large")
		    // group numbers are 32 bits wide: 2^32 - 1 groups are the most, whatever their width
		    {B, two_32 - 1, 0, G, true, F::NONE},
		    {B, two_32, 0, G, true, F::TOO_LARGE},
		    {B, two_32, 64, G, false, F::TOO_LARGE},
		    // no bits: groups of no words, a table that always fits
		    {B, 1, 0, G, true, F::NONE},
		    {B, two_32 - 1, 0, NO_G, false, F::NONE},
		    {B, 0, 0, G, true, F::NO_GROUPS},
		    // the widest group there is: one fits a size_t, sixteen do not
		    {B, 1, ~uint64_t(0), G, true, F::NONE},
		    {B, 16, ~uint64_t(0), G, true, F::TOO_LARGE},
		};
		for (const auto &c : cases)
			EXPECT(check_filter_table(c.allowed, c.n_groups, c.n_bits, c.group_of, c.required) == c.expected);
	}

	// the packing, at widths on both sides of a word edge
	for (uint64_t n_bits : {1ull, 63ull, 64ull, 65ull, 7997ull}) {
		const uint64_t n_tenants = 4, n_queries = 23;
		auto live = [](uint64_t id) { return id % 9 != 0; };
		const FilterGroupTables t = TenantTables(n_tenants, n_bits, n_queries, live);
		EXPECT(t.n_groups == 5 && t.words == filter_group_words(n_bits) && t.allowed.size() == 5 * t.words);
		EXPECT(t.group_of.size() == n_queries && first_unknown_group(t.group_of.data(), n_queries, t.n_groups) == NO_BAD_GROUP);
		for (uint64_t id = 0; id != n_bits + 130; ++id) {
			uint64_t holders = 0;
			for (uint64_t g = 0; g != n_tenants; ++g)
				holders += t.Admits(g, (int64_t)id);
			EXPECT(holders == (id < n_bits && live(id) ? 1u : 0u)); // tenants are disjoint and cover the live rows
			// the all-ones group: every row below n_bits and nothing after, although its padding bits are set
			EXPECT(t.Admits(n_tenants, (int64_t)id) == (id < n_bits));
			// ... and a set bit in the NEXT group's first word admits nothing into the group before it
			EXPECT(id < n_bits || !t.Admits(n_tenants - 1, (int64_t)id));
		}
		EXPECT(!t.Admits(0, -1));
		if (n_bits % 64)
			EXPECT(t.Group(n_tenants)[t.words - 1] == ~0ull); // (the padding IS set)
		uint64_t seen = 0;
		for (uint64_t g = 0; g != t.n_groups; ++g) {
			const auto at = t.QueriesOf(g);
			for (uint64_t q : at)
				EXPECT(t.group_of[q] == g);
			seen += at.size();
		}
		EXPECT(seen == n_queries);
	}

	// gather / compare
	const int64_t rows[4 * 2] = {10, 11, 20, 21, 30, 31, 40, 41};
	const std::vector<uint64_t> at = {3, 1};
	auto packed = GatherRows(rows, 2, at);
	EXPECT(packed.size() == 4 && packed[0] == 40 && packed[1] == 41 && packed[2] == 20 && packed[3] == 21);
	EXPECT(FirstDifference(rows, packed.data(), 2, at) == -1);
	packed[3] = 22;
	EXPECT(FirstDifference(rows, packed.data(), 2, at) == 1);
	std::printf("filter groups check ok\n");
	return 0;
}
