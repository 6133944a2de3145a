// label_filter.h — the label column of vss_search_batch_by_label: pure arithmetic and validation, no HIP, so that it can be
// compiled and run on a CPU (host/label_filter_check.cpp, under the sanitizers).
//
// The column holds one 32-bit label per ROW ID (not per slot), cells [0, labelled_rows).  Query q of a call wants one value,
// want[q], and admits the live rows whose cell holds it.  The engine answers such a call as the bitmap calls answer the table
// this header defines: the distinct values of `want`, ascending, are the groups, group g's bitmap has bit r set iff
// label_admits(labels, labelled_rows, r, value g), and query q takes the group label_groups() gives it.
// vss_search_batch_by_label_range tests the same column against one inclusive range per query: its rule, the walker's and the
// listing's forms of it and its groups are further down (host/label_range_check.cpp), and so are those of
// vss_search_batch_by_label_set, which tests it against a short list of values per query (host/label_set_check.cpp).  The index
// keeps LABEL_COLUMNS_MAX such columns — the one above is column 0 — and vss_search_batch_by_label_box tests up to four of them
// against one range each per query: the last part (host/label_box_check.cpp).
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

// ---- per-query RANGES over the same column (vss_search_batch_by_label_range): query q admits the live rows whose cell holds a
// label in [lo[q], hi[q]], both ends inclusive, compared as unsigned 32-bit values.  lo > hi is the empty predicate, hi = NO_LABEL
// is "no upper bound", and a cell holding NO_LABEL is admitted by nothing.  The derived table: the distinct RAW pairs of the call,
// ascending by (lo, hi), are the groups — nothing is canonicalised, two different empty pairs are two groups — and bitmap g has
// bit r set iff label_range_admits(labels, labelled_rows, r, pair g).

// what a range makes of one cell's value (the listing kernels keep cells in registers; NO_LABEL there is also "no cell at all"):
// hi is cut below NO_LABEL, so that two comparisons exclude the NO_LABEL cell and every lo > hi without a third
inline constexpr bool label_in_range(uint32_t label, uint32_t lo, uint32_t hi) {
	return lo <= label && label <= (hi == NO_LABEL ? NO_LABEL - 1 : hi);
}

// THE admission rule of a range, but for the row being live: the row id has a cell, the cell holds a label, and the label lies
// within the query's ends.  constexpr: the kernels and the CPU check (host/label_range_check.cpp) run this very code.
inline constexpr bool label_range_admits(const uint32_t *labels, uint64_t labelled_rows, int64_t key, uint32_t lo, uint32_t hi) {
	return key >= 0 && (uint64_t)key < labelled_rows && labels[key] != NO_LABEL && lo <= labels[key] && labels[key] <= hi;
}

// What the walker tests a row's cell with: two 64-bit cells per query, {lo, min(hi, NO_LABEL - 1) - lo}, and for a range that
// admits no label {2^32, 0}.  Admission is then ONE subtraction and ONE comparison, label_range_cell_admits: the difference
// wraps beyond every width for a label below lo (and for every 32-bit label under the empty form), and the NO_LABEL cell lies
// beyond every width because hi is cut below it.
struct LabelRangeCells {
	uint64_t lo, width;
};
inline constexpr LabelRangeCells label_range_cells(uint32_t lo, uint32_t hi) {
	const uint32_t top = hi == NO_LABEL ? NO_LABEL - 1 : hi;
	return lo > top ? LabelRangeCells {1ull << 32, 0} : LabelRangeCells {lo, (uint64_t)(top - lo)};
}
inline constexpr bool label_range_cell_admits(uint32_t label, uint64_t cell_lo, uint64_t cell_width) {
	return (uint64_t)label - cell_lo <= cell_width;
}

// one pair of a call; ordered by (lo, hi)
struct LabelRange {
	uint32_t lo, hi;
};
inline constexpr bool operator<(const LabelRange &a, const LabelRange &b) {
	return a.lo != b.lo ? a.lo < b.lo : a.hi < b.hi;
}
inline constexpr bool operator==(const LabelRange &a, const LabelRange &b) {
	return a.lo == b.lo && a.hi == b.hi;
}

// the distinct raw pairs (lo[q], hi[q]) of q in [0, n), ascending, and the group of every query: label_groups' counterpart
inline void label_range_groups(const uint32_t *lo, const uint32_t *hi, uint64_t n, std::vector<LabelRange> &pairs,
                               std::vector<uint32_t> &group_of) {
	pairs.resize(n);
	for (uint64_t q = 0; q != n; ++q)
		pairs[q] = {lo[q], hi[q]};
	std::sort(pairs.begin(), pairs.end());
	pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
	group_of.resize(n);
	for (uint64_t q = 0; q != n; ++q)
		group_of[q] = (uint32_t)(std::lower_bound(pairs.begin(), pairs.end(), LabelRange {lo[q], hi[q]}) - pairs.begin());
}

// ---- per-query SETS over the same column (vss_search_batch_by_label_set): a call brings `sets`, a row-major n_queries x width
// matrix of 32-bit words, 1 <= width <= LABEL_SET_MAX, and query q admits the live rows whose cell holds one of the words of row q.
// NO_LABEL is the padding of a shorter list: a word holding it equals nothing, a row that is all padding is the empty predicate,
// order and repeats inside a row change nothing of what it admits — and a cell holding NO_LABEL is admitted by no set: the
// padding must not match it.  The derived table: the distinct RAW rows of the call, ascending lexicographically as unsigned
// words, are the groups — nothing is canonicalised, the same members in another order are another group — and bitmap g has bit r
// set iff label_set_admits(labels, labelled_rows, r, row g, width).
//
// The cap is a design limit, not a measurement: the walker's test has to stay a short loop of register compares against
// wave-uniform words, and the listing loop does the same per group.  Beyond a few dozen values a bitmap's one load per row is the
// cheaper test, and the bitmap calls stay for that.
constexpr uint32_t LABEL_SET_MAX = 32; // VSS_LABEL_SET_MAX

// THE admission rule of a set, but for the row being live: the row id has a cell, the cell holds a label, and one of the row's
// words is that label.  constexpr: the kernels and the CPU check (host/label_set_check.cpp) run this very code.
inline constexpr bool label_set_admits(const uint32_t *labels, uint64_t labelled_rows, int64_t key, const uint32_t *set, uint32_t width) {
	if (key < 0 || (uint64_t)key >= labelled_rows || labels[key] == NO_LABEL)
		return false;
	for (uint32_t j = 0; j != width; ++j)
		if (labels[key] == set[j])
			return true;
	return false;
}

// The register form: `label` is a cell's value, or NO_LABEL for "no cell at all" (a free slot, a row id beyond the column).  No
// early exit — every lane of a wave runs the same `width` compares against wave-uniform words — and ONE test of the label
// against NO_LABEL at the end keeps the padding from matching the unlabelled cell.
inline constexpr bool label_hits2(uint32_t label, uint32_t a, uint32_t b) { // (one step of the walker's loop)
	return (label == a) | (label == b);
}
inline constexpr bool label_in_set(uint32_t label, const uint32_t *set, uint32_t width) {
	bool hit = false;
	for (uint32_t j = 0; j != width; ++j)
		hit |= label == set[j];
	return hit & (label != NO_LABEL);
}

// What the walker's table holds of one row: the raw words, padded with NO_LABEL to a multiple of FOUR, so that every row is whole,
// aligned 16-byte chunks.  Padding equals nothing, so the padded row admits what the raw row admits.  The walker reads it by
// two-word scalar loads (label_in_padded_set is its loop: label_in_set over the padded row, two words a step;
// host/label_set_check.cpp proves both against the rule) — four words a step cost the few-query kernels, which sit at their
// scalar-register limit, 36-52 bytes of scratch in seven instantiations.
inline constexpr uint32_t label_set_chunks(uint32_t width) {
	return (width + 3) / 4;
}
inline constexpr uint32_t label_set_table_word(const uint32_t *set, uint32_t width, uint32_t j) { // j < 4 * label_set_chunks(width)
	return j < width ? set[j] : NO_LABEL;
}
inline constexpr bool label_in_padded_set(uint32_t label, const uint32_t *padded, uint32_t chunks) {
	bool hit = false;
	for (uint32_t j = 0; j != 2 * chunks; ++j)
		hit |= label_hits2(label, padded[2 * j], padded[2 * j + 1]);
	return hit & (label != NO_LABEL);
}

// the distinct raw rows of `sets` (n rows of `width` words), ascending lexicographically as unsigned words and flattened into
// `rows` (rows.size() / width groups), and the group of every query: label_range_groups' counterpart
inline void label_set_groups(const uint32_t *sets, uint64_t n, uint32_t width, std::vector<uint32_t> &rows, std::vector<uint32_t> &group_of) {
	std::vector<uint64_t> order(n);
	for (uint64_t q = 0; q != n; ++q)
		order[q] = q;
	const auto less = [&](uint64_t a, uint64_t b) {
		return std::lexicographical_compare(sets + a * width, sets + (a + 1) * width, sets + b * width, sets + (b + 1) * width);
	};
	std::sort(order.begin(), order.end(), less);
	rows.clear();
	group_of.resize(n);
	uint64_t groups = 0;
	for (uint64_t i = 0; i != n; ++i) {
		if (i == 0 || less(order[i - 1], order[i])) {
			rows.insert(rows.end(), sets + order[i] * width, sets + (order[i] + 1) * width);
			++groups;
		}
		group_of[order[i]] = (uint32_t)(groups - 1);
	}
}

// ---- per-query BOXES over several columns (vss_search_batch_by_label_box): the index keeps LABEL_COLUMNS_MAX columns, each what
// the one column is above (column 0 IS that column), and a call names m distinct ones, columns[0 .. m), 1 <= m <= 4, for all its
// queries.  Query q brings one range per named column, lo[q * m + j] .. hi[q * m + j], and admits the live rows that
// label_range_admits admits in EVERY named column: the row id has a cell there, the cell holds a label, the label lies within the
// ends.  One empty range empties the box.  A column that is not named constrains nothing — not even its NO_LABEL cells.
// Inside the engine a box travels as ONE row of 2m words, (lo_0, hi_0, lo_1, hi_1, ...): label_box_rows interleaves a call's two
// matrices.  The derived table: the distinct RAW rows, ascending lexicographically as unsigned words, nothing canonicalised, are
// the groups, and bitmap g has bit r set iff label_box_admits(..., r, row g); its n_bits is the smallest rows(c) of the named columns.
constexpr uint32_t LABEL_COLUMNS_MAX = 4; // VSS_LABEL_COLUMNS_MAX

// THE admission rule of a box, but for the row being live.  cells[c] / rows[c]: column c of the index; box: 2m words.
// constexpr: the kernels and the CPU check (host/label_box_check.cpp) run this very code.
inline constexpr bool label_box_admits(const uint32_t *const *cells, const uint64_t *rows, const uint32_t *columns, uint32_t m, int64_t key,
                                       const uint32_t *box) {
	for (uint32_t j = 0; j != m; ++j)
		if (!label_range_admits(cells[columns[j]], rows[columns[j]], key, box[2 * j], box[2 * j + 1]))
			return false;
	return true;
}

// The register form of the listing kernels: label[j] is the row's cell in named column j, or NO_LABEL for "no cell at all".  No
// early exit: 2m compares against wave-uniform words, ANDed.
template <uint32_t M>
inline constexpr bool label_in_box(const uint32_t (&label)[M], const uint32_t *box) {
	bool in = true;
	for (uint32_t j = 0; j != M; ++j)
		in &= label_in_range(label[j], box[2 * j], box[2 * j + 1]);
	return in;
}

// What the walker's table holds: cell 0 the number of named columns m, cells 1 .. m their addresses in call order, and from cell
// 1 + m on 2m cells per query — named column j's pair at 2j and 2j + 1, exactly label_range_cells(lo, hi).
inline constexpr uint64_t label_box_table_cells(uint32_t m, uint64_t n_queries) {
	return 1 + m + 2 * (uint64_t)m * n_queries;
}
inline constexpr uint64_t label_box_query_cell(uint32_t m, uint64_t query) { // the first of query's 2m cells
	return 1 + m + 2 * (uint64_t)m * query;
}
// the walker's test of a row whose cells are label[0 .. m) against a query's 2m table cells: m label_range_cell_admits, ANDed
// without a branch per column
inline constexpr bool label_box_cells_admit(const uint32_t *label, const uint64_t *cells, uint32_t m) {
	bool in = true;
	for (uint32_t j = 0; j != m; ++j)
		in &= label_range_cell_admits(label[j], cells[2 * j], cells[2 * j + 1]);
	return in;
}

// the n x 2m matrix of a call's boxes from its two n x m matrices
inline void label_box_rows(const uint32_t *lo, const uint32_t *hi, uint64_t n, uint32_t m, std::vector<uint32_t> &boxes) {
	boxes.resize(2 * (size_t)m * n);
	for (uint64_t i = 0; i != n * m; ++i)
		boxes[2 * i] = lo[i], boxes[2 * i + 1] = hi[i];
}

// the distinct raw rows of `boxes` (n rows of 2m words), ascending, flattened into `rows`, and the group of every query:
// label_range_groups' counterpart (with m == 1 the same groups in the same order)
inline void label_box_groups(const uint32_t *boxes, uint64_t n, uint32_t m, std::vector<uint32_t> &rows, std::vector<uint32_t> &group_of) {
	label_set_groups(boxes, n, 2 * m, rows, group_of);
}

// the named columns of a call: which one breaks the rules (a number >= LABEL_COLUMNS_MAX, or one named before), or m for none
inline constexpr uint32_t label_box_bad_column(const uint32_t *columns, uint32_t m) {
	for (uint32_t j = 0; j != m; ++j) {
		if (columns[j] >= LABEL_COLUMNS_MAX)
			return j;
		for (uint32_t i = 0; i != j; ++i)
			if (columns[i] == columns[j])
				return j;
	}
	return m;
}

// vss_set_labels(first_rowid, n): what the range breaks, or NONE. Cells end at 2^32 (first_rowid + n == 2^32 is the last range
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
