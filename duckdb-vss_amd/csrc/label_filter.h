// label_filter.h — the label column of vss_search_batch_by_label: pure arithmetic and validation, no HIP, so that it can be
// compiled and run on a CPU (host/label_filter_check.cpp, under the sanitizers).
//
// The column holds one 32-bit label per ROW ID (not per slot), cells [0, labelled_rows).  Query q of a call wants one value,
// want[q], and admits the live rows whose cell holds it.  The engine answers such a call as the bitmap calls answer the table
// this header defines: the distinct values of `want`, ascending, are the groups, group g's bitmap has bit r set iff
// label_admits(labels, labelled_rows, r, value g), and query q takes the group label_groups() gives it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace vss {
namespace host {

constexpr uint32_t NO_LABEL = 0xFFFFFFFFu;      // VSS_NO_LABEL: the cell of a row without a label; as a wanted value it equals nothing
constexpr uint32_t NO_LABEL_GROUP = 0xFFFFFFFFu; // label_lookup: the label is none of the values
constexpr uint64_t LABEL_ROWS_MAX = 1ull << 32;  // row ids with a cell are below this

// THE admission rule, but for the row being live (its key is not the free key): the row id has a cell, the cell holds the
// wanted value, and that value is a label at all.  constexpr: the kernels and the CPU check run this very code.
inline constexpr bool label_admits(const uint32_t *labels, uint64_t labelled_rows, int64_t key, uint32_t want) {
	return key >= 0 && (uint64_t)key < labelled_rows && want != NO_LABEL && labels[key] == want;
}

// What the walker compares a row's cell with: the wanted value widened to 64 bits, or — for NO_LABEL — a value no 32-bit cell
// widens to.  (admission is then ONE comparison: (uint64_t)labels[key] == label_want_cell(want))
inline constexpr uint64_t label_want_cell(uint32_t want) {
	return want == NO_LABEL ? (1ull << 32) : (uint64_t)want;
}

// Which of the n ASCENDING distinct values `label` is, or NO_LABEL_GROUP: a lower bound by halving [lo, hi), then one
// comparison.  In pieces, so that the listing kernels can run the steps of several lookups side by side: a step halves the
// interval (or leaves an empty one alone), label_lookup_steps(n) steps empty any interval of n values, and the result is read
// off `lo`.  NO_LABEL is never found, even where it is among the values (a query may want it: it gets nothing).
inline constexpr void label_lookup_step(const uint32_t *values, uint32_t label, uint32_t &lo, uint32_t &hi) {
	if (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (values[mid] < label)
			lo = mid + 1;
		else
			hi = mid;
	}
}
inline constexpr uint32_t label_lookup_steps(uint32_t n) { // floor(log2(n)) + 1, 0 for no values
	uint32_t steps = 0;
	for (; n; n >>= 1)
		++steps;
	return steps;
}
inline constexpr uint32_t label_lookup_result(const uint32_t *values, uint32_t n, uint32_t label, uint32_t lo) {
	return label != NO_LABEL && lo < n && values[lo] == label ? lo : NO_LABEL_GROUP;
}
inline constexpr uint32_t label_lookup(const uint32_t *values, uint32_t n, uint32_t label) {
	uint32_t lo = 0, hi = n; // the answer, if any, is in [lo, hi)
	for (uint32_t step = label_lookup_steps(n); step; --step)
		label_lookup_step(values, label, lo, hi);
	return label_lookup_result(values, n, label, lo);
}

// the distinct values of want[0 .. n), ascending (NO_LABEL, where wanted, is the last), and the group of every query
inline void label_groups(const uint32_t *want, uint64_t n, std::vector<uint32_t> &values, std::vector<uint32_t> &group_of) {
	values.assign(want, want + n);
	std::sort(values.begin(), values.end());
	values.erase(std::unique(values.begin(), values.end()), values.end());
	group_of.resize(n);
	for (uint64_t q = 0; q != n; ++q)
		group_of[q] = (uint32_t)(std::lower_bound(values.begin(), values.end(), want[q]) - values.begin());
}

// vss_set_labels(first_rowid, n): what the range breaks, or NONE.  Cells end at 2^32 (first_rowid + n == 2^32 is the last range
// that fits); the sum is formed without wrapping.
enum class LabelRangeFault { NONE, NO_LABELS, TOO_FAR };

inline constexpr LabelRangeFault check_label_range(const void *labels, uint64_t first_rowid, uint64_t n) {
	return !n                                                           ? LabelRangeFault::NONE
	       : !labels                                                    ? LabelRangeFault::NO_LABELS
	       : first_rowid > LABEL_ROWS_MAX || n > LABEL_ROWS_MAX - first_rowid ? LabelRangeFault::TOO_FAR
	                                                                    : LabelRangeFault::NONE;
}

// What a write of cells [first_rowid, first_rowid + n), n > 0, does to a column of `labelled_rows` cells: the cells it has
// afterwards, and the gap [gap_begin, gap_end) it skips over, which is filled with NO_LABEL (empty where the write touches
// or overlaps the column).
struct LabelWrite {
	uint64_t rows_after, gap_begin, gap_end;
};
inline constexpr LabelWrite label_write(uint64_t labelled_rows, uint64_t first_rowid, uint64_t n) {
	return {first_rowid + n > labelled_rows ? first_rowid + n : labelled_rows, labelled_rows,
	        first_rowid > labelled_rows ? first_rowid : labelled_rows};
}

} // namespace host
} // namespace vss
