// filter_groups.h — the group table of vss_search_batch_filtered_groups: pure arithmetic and validation, no HIP, so that it
// can be compiled and run on a CPU (host/filter_groups_check.cpp, host/filter_probe_check.cpp, under the sanitizers).
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

// What a caller's description of one table violates: the first rule, in this order, or none.  Every layer that takes a table
// (the engine's entry points, host/sharded_index.hpp) asks this and words the answer itself.
enum class FilterTableFault { NONE, NO_BITMAPS, NO_GROUP_NUMBERS, NO_GROUPS, TOO_LARGE };

inline FilterTableFault check_filter_table(const uint64_t *allowed, uint64_t n_groups, uint64_t n_bits, const uint32_t *group_of,
                                           bool group_of_required) {
	const bool too_large = n_groups > 0xFFFFFFFFull || !filter_group_table_fits(n_groups, n_bits); // (group numbers have 32 bits)
	return !allowed                         ? FilterTableFault::NO_BITMAPS
	       : group_of_required && !group_of ? FilterTableFault::NO_GROUP_NUMBERS
	       : !n_groups                      ? FilterTableFault::NO_GROUPS
	       : too_large                      ? FilterTableFault::TOO_LARGE
	                                        : FilterTableFault::NONE;
}

// the first query whose group is not in the table, or NO_BAD_GROUP
inline uint64_t first_unknown_group(const uint32_t *group_of, uint64_t n_queries, uint64_t n_groups) {
	for (uint64_t q = 0; q != n_queries; ++q)
		if (group_of[q] >= n_groups)
			return q;
	return NO_BAD_GROUP;
}

// A launch of several batches (vss_search_multi_filtered_device_begin): every batch brings its own table.  Batch b of the
// launch is described by one of these; the launch numbers its queries q = b * n_per_batch + row.
struct FilterGroupBatch {
	const uint64_t *allowed;  // n_groups bitmaps end to end
	const uint32_t *group_of; // the group of every query of the batch, or nullptr: all of them take bitmap 0
	uint64_t n_groups;
};
constexpr uint32_t MAX_FILTER_GROUP_BATCHES = 32; // the launch's batches (MAX_COALESCED of the engine)
constexpr uint64_t NO_GROUP_BITMAP = ~uint64_t(0);

inline constexpr uint64_t filter_group_batch_of(uint64_t n_per_batch, uint64_t q) {
	return q / n_per_batch;
}

// Where the bitmap of launch-wide query q starts, in words from `allowed` of ITS batch's descriptor `d`
// (= batches[filter_group_batch_of(n_per_batch, q)]), or NO_GROUP_BITMAP if its group is not in that table.  constexpr, so
// that the resolve kernel and the CPU check run this very code; a table that filter_group_table_fits cannot wrap here.
inline constexpr uint64_t filter_group_word_offset(const FilterGroupBatch &d, uint64_t n_per_batch, uint64_t words, uint64_t q) {
	const uint64_t row = q - filter_group_batch_of(n_per_batch, q) * n_per_batch;
	const uint64_t group = d.group_of ? d.group_of[row] : 0;
	return group < d.n_groups ? group * words : NO_GROUP_BITMAP;
}

} // namespace host
} // namespace vss
