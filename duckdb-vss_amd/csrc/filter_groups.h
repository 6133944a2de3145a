// filter_groups.h — the group table of vss_search_batch_filtered_groups: pure arithmetic and validation, no HIP, so that it
// can be compiled and run on a CPU (host/filter_groups_check.cpp, under the sanitizers).
//
// The table is n_groups bitmaps over row ids laid end to end, each filter_group_words(n_bits) 64-bit words; query q is
// filtered by the bitmap that starts at word group_of[q] * filter_group_words(n_bits).
#pragma once
#include <cstddef>
#include <cstdint>

namespace vss {
namespace host {

constexpr uint64_t NO_BAD_GROUP = ~uint64_t(0);

inline uint64_t filter_group_words(uint64_t n_bits) {
	return n_bits / 64 + (n_bits % 64 ? 1 : 0); // (n_bits + 63) / 64 without the wrap at 2^64 - 63
}

// false where n_groups * words * 8 bytes is more than a size_t holds (a table nobody can have allocated)
inline bool filter_group_table_fits(uint64_t n_groups, uint64_t n_bits) {
	const uint64_t words = filter_group_words(n_bits);
	return !words || n_groups <= (SIZE_MAX / 8) / words;
}

// the first query whose group is not in the table, or NO_BAD_GROUP
inline uint64_t first_unknown_group(const uint32_t *group_of, uint64_t n_queries, uint64_t n_groups) {
	for (uint64_t q = 0; q != n_queries; ++q)
		if (group_of[q] >= n_groups)
			return q;
	return NO_BAD_GROUP;
}

} // namespace host
} // namespace vss
