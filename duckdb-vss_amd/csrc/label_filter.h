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
// against one range each per query (host/label_box_check.cpp).  A column's cells are 32 or 64 bits wide, and
// vss_search_batch_by_label_box64 tests columns of either width against ranges with 64-bit ends (host/label_box64_check.cpp).
// vss_search_batch_by_label_set_box tests one column against a short list of 64-bit words per query and up to three more against
// such ranges: the last part (host/label_set_box_check.cpp).
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

// ---- 64-bit columns and per-query boxes with 64-bit ends (vss_search_batch_by_label_box64): each of the LABEL_COLUMNS_MAX columns
// has a WIDTH, 32 or 64 bits a cell (vss_set_label_column64 writes the wide ones; a column keeps one width until it is cleared).
// The NULL cell of a wide column is NO_LABEL64.  A call names m distinct columns of either width, mixed, and query q brings one
// range of 64-bit ends per named column.  A 32-bit cell is read ZERO-EXTENDED, and its NO_LABEL reads as NO_LABEL64
// (label_widen), so one rule serves both widths: query q admits the live rows that label_range64_admits admits in EVERY named
// column — the row id has a cell there, the widened cell is not NO_LABEL64, and lo <= cell <= hi, unsigned.  One empty range
// empties the box; hi = NO_LABEL64 is "no upper bound" and still rejects the NULL cells.
// Inside the engine a box travels as ONE row of 4m 32-bit words: per named column lo then hi, each 64-bit end as the pair (HIGH
// word, low word) — label_box64_rows.  High word first, so that the lexicographic order of the rows as 32-bit words IS their
// lexicographic order as 2m unsigned 64-bit words: label_set_groups' order is the contract's order, and everything that carries
// rows of 32-bit words per query or per group (the plans, the compact batch of the graph-routed queries, the sharded exchange)
// carries these unchanged.  The derived table: the distinct RAW rows, ascending, nothing canonicalised, are the groups; bitmap g
// has bit r set iff label_box64_admits(..., r, row g); its n_bits is the smallest rows(c) of the named columns.
constexpr uint64_t NO_LABEL64 = 0xFFFFFFFFFFFFFFFFull; // VSS_NO_LABEL64

inline constexpr uint64_t label_widen(uint32_t cell) {
	return cell == NO_LABEL ? NO_LABEL64 : (uint64_t)cell;
}

// One column of the index as the 64-bit rule reads it: `rows` cells, 32 bits wide (narrow) or 64 (wide); the other pointer is null.
struct LabelColumn64 {
	const uint32_t *narrow;
	const uint64_t *wide;
	uint64_t rows;
};
inline constexpr uint64_t label_cell64(const LabelColumn64 &c, uint64_t key) { // key < c.rows
	return c.wide ? c.wide[key] : label_widen(c.narrow[key]);
}

inline constexpr bool label_range64_admits(const LabelColumn64 &c, int64_t key, uint64_t lo, uint64_t hi) {
	if (key < 0 || (uint64_t)key >= c.rows)
		return false;
	const uint64_t cell = label_cell64(c, (uint64_t)key);
	return cell != NO_LABEL64 && lo <= cell && cell <= hi;
}

// THE admission rule of a 64-bit box, but for the row being live.  index_columns[c]: column c of the index; box: 2m 64-bit words
// (lo_0, hi_0, lo_1, hi_1, ...).  constexpr: the kernels' forms below are proven against this very code (host/label_box64_check.cpp).
inline constexpr bool label_box64_admits(const LabelColumn64 *index_columns, const uint32_t *columns, uint32_t m, int64_t key,
                                         const uint64_t *box) {
	for (uint32_t j = 0; j != m; ++j)
		if (!label_range64_admits(index_columns[columns[j]], key, box[2 * j], box[2 * j + 1]))
			return false;
	return true;
}

// a 64-bit end out of its (high word, low word) pair, and back
inline constexpr uint64_t label_word64(const uint32_t *pair) {
	return (uint64_t)pair[0] << 32 | pair[1];
}
inline constexpr uint64_t label_word64(uint32_t high, uint32_t low) {
	return (uint64_t)high << 32 | low;
}

// The register form of the listing kernels: label[j] is the row's WIDENED cell in named column j, or NO_LABEL64 for "no cell at
// all"; box: the group's 4m 32-bit words.  hi is cut below NO_LABEL64 as label_in_range cuts it below NO_LABEL.  No early exit.
inline constexpr bool label64_in_range(uint64_t label, uint64_t lo, uint64_t hi) {
	return lo <= label && label <= (hi == NO_LABEL64 ? NO_LABEL64 - 1 : hi);
}
template <uint32_t M>
inline constexpr bool label_in_box64(const uint64_t (&label)[M], const uint32_t *box) {
	bool in = true;
	for (uint32_t j = 0; j != M; ++j)
		in &= label64_in_range(label[j], label_word64(box + 4 * j), label_word64(box + 4 * j + 2));
	return in;
}

// What the walker tests a row's widened cell with: two 64-bit cells per query and named column, {lo, count}, count the number of
// admitted values: top = min(hi, NO_LABEL64 - 1), count = lo > top ? 0 : top - lo + 1 (at most 2^64 - 1: no wrap).  Admission is ONE
// subtraction and ONE comparison, (cell - lo) < count, without a branch: the empty range has count 0, a cell below lo wraps to at
// least 2^64 - lo > count, and the NO_LABEL64 cell gives 2^64 - 1 - lo >= count.  (The 32-bit box's {lo, width} form needs a
// value beyond every cell for its empty range; 64 bits have none.)
struct LabelRange64Cells {
	uint64_t lo, count;
};
inline constexpr LabelRange64Cells label_range64_cells(uint64_t lo, uint64_t hi) {
	const uint64_t top = hi == NO_LABEL64 ? NO_LABEL64 - 1 : hi;
	return {lo, lo > top ? 0 : top - lo + 1};
}
inline constexpr bool label_range64_cell_admits(uint64_t cell, uint64_t cell_lo, uint64_t cell_count) {
	return cell - cell_lo < cell_count;
}

// What the walker's table holds — label_box_table_cells(m, n_queries) cells, as the 32-bit box's: cell 0 is
// label_box64_table_head: the number of named columns m in its low byte and from bit 8 on one bit per named column, set where the
// column is 64 bits wide; cells 1 .. m the columns' addresses in call order; from cell 1 + m (label_box_query_cell) on 2m cells
// per query, named column j's label_range64_cells pair at 2j and 2j + 1.
inline constexpr uint64_t label_box64_table_head(uint32_t m, uint32_t wide_mask) {
	return (uint64_t)m | (uint64_t)wide_mask << 8;
}
inline constexpr uint32_t label_box64_head_columns(uint64_t head) {
	return (uint32_t)(head & 0xFF);
}
inline constexpr bool label_box64_head_wide(uint64_t head, uint32_t j) {
	return (head >> (8 + j)) & 1;
}
// the walker's test of a row whose widened cells are label[0 .. m) against a query's 2m table cells
inline constexpr bool label_box64_cells_admit(const uint64_t *label, const uint64_t *cells, uint32_t m) {
	bool in = true;
	for (uint32_t j = 0; j != m; ++j)
		in &= label_range64_cell_admits(label[j], cells[2 * j], cells[2 * j + 1]);
	return in;
}

// the n x 4m matrix of a call's boxes from its two n x m matrices of 64-bit ends
inline void label_box64_rows(const uint64_t *lo, const uint64_t *hi, uint64_t n, uint32_t m, std::vector<uint32_t> &boxes) {
	boxes.resize(4 * (size_t)m * n);
	for (uint64_t i = 0; i != n * m; ++i) {
		boxes[4 * i] = (uint32_t)(lo[i] >> 32), boxes[4 * i + 1] = (uint32_t)lo[i];
		boxes[4 * i + 2] = (uint32_t)(hi[i] >> 32), boxes[4 * i + 3] = (uint32_t)hi[i];
	}
}

// the distinct raw rows of `boxes` (n rows of 4m words), ascending — as 2m unsigned 64-bit words, see above — flattened into
// `rows`, and the group of every query
inline void label_box64_groups(const uint32_t *boxes, uint64_t n, uint32_t m, std::vector<uint32_t> &rows, std::vector<uint32_t> &group_of) {
	label_set_groups(boxes, n, 4 * m, rows, group_of);
}

// ---- per-query IN-LISTS on one column INSIDE a box of ranges (vss_search_batch_by_label_set_box): a call names one SET column and
// m further distinct RANGE columns, 0 <= m <= 3, all of either width, mixed.  Query q brings `width` 64-bit words for the set column,
// 1 <= width <= LABEL_SET_MAX (NO_LABEL64 pads a shorter list and equals nothing), and one range of 64-bit ends per range column.
// Cells are read as the box64 call reads them (label_widen).  Query q admits the live rows whose row id has a cell in the set column
// and in every range column, whose widened set cell is not NO_LABEL64 and equals one of the query's words, and which
// label_range64_admits admits in every range column.  A row of words that is all padding is the empty predicate, and so is any
// lo > hi; order and repeats among the words change nothing; a word of 2^32 or above matches no cell of a 32-bit column, and neither
// does 0xFFFFFFFF there, because the cell it would match reads as NULL.  m == 0 is the set call over 64-bit words.
// Inside the engine a predicate travels as ONE row of 2 width + 4m 32-bit words (label_set_box_rows): the set words first, then per
// range column lo then hi, every 64-bit word as the pair (HIGH word, low word) — so the lexicographic order of the rows as 32-bit
// words IS their order as width + 2m unsigned 64-bit words, label_set_groups' order is the contract's, and whatever carries rows of
// 32-bit words per query or per group carries these unchanged.  The derived table: the distinct RAW rows, ascending, nothing
// canonicalised (the same members in another order are another group), are the groups; bitmap g has bit r set iff
// label_set_box_admits(..., r, row g); its n_bits is the smallest rows(c) over the set column and the range columns.
constexpr uint32_t LABEL_SET_BOX_RANGES_MAX = LABEL_COLUMNS_MAX - 1;
constexpr uint32_t LABEL_SET_BOX_ROW_WORDS_MAX = 2 * LABEL_SET_MAX + 4 * LABEL_SET_BOX_RANGES_MAX; // 76

// THE admission rule, but for the row being live.  index_columns[c]: column c of the index; set: `width` 64-bit words; box: 2m 64-bit
// words (lo_0, hi_0, ...) for the range columns columns[0 .. m).  constexpr: the kernels' forms below are proven against this very
// code (host/label_set_box_check.cpp).
inline constexpr bool label_set_box_admits(const LabelColumn64 *index_columns, uint32_t set_column, const uint64_t *set, uint32_t width,
                                           const uint32_t *columns, uint32_t m, int64_t key, const uint64_t *box) {
	const LabelColumn64 &sc = index_columns[set_column];
	if (key < 0 || (uint64_t)key >= sc.rows)
		return false;
	for (uint32_t j = 0; j != m; ++j)
		if (!label_range64_admits(index_columns[columns[j]], key, box[2 * j], box[2 * j + 1]))
			return false;
	const uint64_t cell = label_cell64(sc, (uint64_t)key);
	if (cell == NO_LABEL64)
		return false;
	for (uint32_t j = 0; j != width; ++j)
		if (cell == set[j])
			return true;
	return false;
}

// words of 32 bits in a travelling row, and where its range part begins
inline constexpr uint32_t label_set_box_row_words(uint32_t width, uint32_t m) {
	return 2 * width + 4 * m;
}

// The register form of the listing kernels: label[0] is the row's WIDENED cell in the set column, label[1 + j] in range column j,
// each NO_LABEL64 for "no cell at all"; row: the group's travelling row.  No early exit: `width` 64-bit compares ORed, ONE test of
// the set cell against NO_LABEL64 (which keeps the padding from matching the NULL cell), then label64_in_range per range column,
// all ANDed.
template <uint32_t M>
inline constexpr bool label_in_set_box(const uint64_t (&label)[M + 1], const uint32_t *row, uint32_t width) {
	bool hit = false;
	for (uint32_t j = 0; j != width; ++j)
		hit |= label[0] == label_word64(row + 2 * j);
	bool in = hit & (label[0] != NO_LABEL64);
	const uint32_t *box = row + 2 * width;
	for (uint32_t j = 0; j != M; ++j)
		in &= label64_in_range(label[1 + j], label_word64(box + 4 * j), label_word64(box + 4 * j + 2));
	return in;
}

// What the walker's table holds.  Cell 0 is the head: the number of range columns m in its low byte, the PADDED set length in the
// next byte — the words of a row padded with NO_LABEL64 to an even number, so that every query's words are whole, aligned 16-byte
// chunks for two-word scalar loads — and from bit 16 on one bit per column, set where it is 64 bits wide: bit 16 the set column, bit
// 17 + j range column j.  Cells 1 .. 1 + m hold the columns' addresses, the set column first.  The per-query cells begin at the next
// EVEN cell (label_set_box_query_base): `padded` set words, then 2m cells, range column j's label_range64_cells pair at 2j, 2j + 1.
inline constexpr uint32_t label_set_box_padded(uint32_t width) {
	return (width + 1) & ~1u;
}
inline constexpr uint64_t label_set_box_table_head(uint32_t m, uint32_t padded, uint32_t wide_mask) {
	return (uint64_t)m | (uint64_t)padded << 8 | (uint64_t)wide_mask << 16;
}
inline constexpr uint32_t label_set_box_head_ranges(uint64_t head) {
	return (uint32_t)(head & 0xFF);
}
inline constexpr uint32_t label_set_box_head_padded(uint64_t head) {
	return (uint32_t)(head >> 8 & 0xFF);
}
inline constexpr bool label_set_box_head_wide(uint64_t head, uint32_t j) { // j == 0: the set column; 1 + j: range column j
	return (head >> (16 + j)) & 1;
}
inline constexpr uint64_t label_set_box_query_base(uint32_t m) {
	return (2 + (uint64_t)m + 1) & ~1ull;
}
inline constexpr uint64_t label_set_box_query_cells(uint32_t m, uint32_t padded) {
	return (uint64_t)padded + 2 * m;
}
inline constexpr uint64_t label_set_box_query_cell(uint32_t m, uint32_t padded, uint64_t query) { // the first of query's cells
	return label_set_box_query_base(m) + label_set_box_query_cells(m, padded) * query;
}
inline constexpr uint64_t label_set_box_table_cells(uint32_t m, uint32_t padded, uint64_t n_queries) {
	return label_set_box_query_cell(m, padded, n_queries);
}
// cell j < label_set_box_query_cells(m, padded) of a query whose travelling row is `row`
inline constexpr uint64_t label_set_box_table_cell(const uint32_t *row, uint32_t width, uint32_t m, uint32_t j) {
	const uint32_t padded = label_set_box_padded(width);
	if (j < padded)
		return j < width ? label_word64(row + 2 * j) : NO_LABEL64;
	const uint32_t *pair = row + 2 * width + 4 * ((j - padded) / 2);
	const LabelRange64Cells c = label_range64_cells(label_word64(pair), label_word64(pair + 2));
	return (j - padded) & 1 ? c.count : c.lo;
}
// the walker's loop: one step tests the set cell against a chunk of two words
inline constexpr bool label64_hits2(uint64_t label, uint64_t a, uint64_t b) {
	return (label == a) | (label == b);
}
// the walker's test of a row whose widened cells are label[0] (set column) and label[1 .. 1 + m) against a query's cells
inline constexpr bool label_set_box_cells_admit(const uint64_t *label, const uint64_t *cells, uint32_t m, uint32_t padded) {
	bool hit = false;
	for (uint32_t j = 0; j != padded; j += 2)
		hit |= label64_hits2(label[0], cells[j], cells[j + 1]);
	bool in = hit & (label[0] != NO_LABEL64);
	for (uint32_t j = 0; j != m; ++j)
		in &= label_range64_cell_admits(label[1 + j], cells[padded + 2 * j], cells[padded + 2 * j + 1]);
	return in;
}

// the n x (2 width + 4m) matrix of a call's travelling rows from its three matrices (lo, hi: not read where m == 0)
inline void label_set_box_rows(const uint64_t *sets, uint32_t width, const uint64_t *lo, const uint64_t *hi, uint64_t n, uint32_t m,
                               std::vector<uint32_t> &rows) {
	const uint32_t per = label_set_box_row_words(width, m);
	rows.resize((size_t)per * n);
	for (uint64_t q = 0; q != n; ++q) {
		uint32_t *row = rows.data() + q * per;
		for (uint32_t j = 0; j != width; ++j)
			row[2 * j] = (uint32_t)(sets[q * width + j] >> 32), row[2 * j + 1] = (uint32_t)sets[q * width + j];
		row += 2 * width;
		for (uint32_t j = 0; j != m; ++j) {
			const uint64_t l = lo[q * m + j], h = hi[q * m + j];
			row[4 * j] = (uint32_t)(l >> 32), row[4 * j + 1] = (uint32_t)l;
			row[4 * j + 2] = (uint32_t)(h >> 32), row[4 * j + 3] = (uint32_t)h;
		}
	}
}

// the distinct raw rows, ascending as width + 2m unsigned 64-bit words (see above), flattened, and the group of every query
inline void label_set_box_groups(const uint32_t *rows_in, uint64_t n, uint32_t width, uint32_t m, std::vector<uint32_t> &rows,
                                 std::vector<uint32_t> &group_of) {
	label_set_groups(rows_in, n, label_set_box_row_words(width, m), rows, group_of);
}

// the columns of a call: which one breaks the rules, or m + 1 for none.  0: the set column is >= LABEL_COLUMNS_MAX.  1 + j: range
// column j is >= LABEL_COLUMNS_MAX, was named before, or is the set column.
inline constexpr uint32_t label_set_box_bad_column(uint32_t set_column, const uint32_t *columns, uint32_t m) {
	if (set_column >= LABEL_COLUMNS_MAX)
		return 0;
	for (uint32_t j = 0; j != m; ++j) {
		if (columns[j] >= LABEL_COLUMNS_MAX || columns[j] == set_column)
			return 1 + j;
		for (uint32_t i = 0; i != j; ++i)
			if (columns[i] == columns[j])
				return 1 + j;
	}
	return m + 1;
}

// ---- SEVERAL BATCHES in one launch (vss_search_by_label_device_begin, vss_search_multi_by_label_device_begin): a launch carries 1 to
// LABEL_BATCHES_MAX batches of per_batch queries each, all of one kind, over the same columns and of the same set width, and every
// batch brings its OWN per-query words as the form's _device call takes them — separate matrices in DEVICE memory, no travelling
// rows.  The launch numbers its queries q = batch * per_batch + row, and the walk table is the one of the single-batch forms above
// over all n_batches * per_batch queries: query q's cells sit where the form's table puts query q, and each of them is what the
// form's cell function makes of row `row` of batch `batch`'s matrices.  Everything here is constexpr: the resolve kernels and the
// CPU check (host/label_batches_check.cpp) run this very code.
constexpr uint32_t LABEL_BATCHES_MAX = 32; // the launch's batches (MAX_COALESCED of the engine)

enum class LabelKind : uint32_t { EQ, RANGE, SET, BOX, BOX64, SET_BOX }; // VSS_LABEL_EQ .. VSS_LABEL_SET_BOX

// launch-wide query -> (batch, row of the batch)
struct LabelBatchAt {
	uint64_t batch, row;
};
inline constexpr LabelBatchAt label_batch_at(uint64_t per_batch, uint64_t q) {
	return {q / per_batch, q % per_batch};
}

// One batch's words, W = uint32_t for EQ / RANGE / SET / BOX and uint64_t for BOX64 / SET_BOX.  words: EQ's `want` (per_batch
// values), SET's and SET_BOX's `sets` (per_batch x width); lo, hi: RANGE's ends (per_batch values), BOX's, BOX64's and SET_BOX's
// matrices (per_batch x m).  What a kind does not use is not read.
template <class W>
struct LabelBatch {
	const W *words, *lo, *hi;
};

// what all batches of a launch share.  width: the set's (SET, SET_BOX); m: the named columns of a BOX / BOX64, the RANGE columns of
// a SET_BOX
struct LabelBatchShape {
	LabelKind kind;
	uint32_t width, m, per_batch;
};

// A query's share of the table, in UNITS: 64-bit cells, but for SET, whose table is written by 32-bit words.  And the cell where
// query 0's share begins — the head of the table ends there.
inline constexpr uint64_t label_batches_query_units(const LabelBatchShape &s) {
	return s.kind == LabelKind::EQ      ? 1
	       : s.kind == LabelKind::RANGE ? 2
	       : s.kind == LabelKind::SET   ? 4 * (uint64_t)label_set_chunks(s.width)
	       : s.kind == LabelKind::SET_BOX ? label_set_box_query_cells(s.m, label_set_box_padded(s.width))
	                                      : 2 * (uint64_t)s.m;
}
inline constexpr uint64_t label_batches_query_base(const LabelBatchShape &s) {
	return s.kind == LabelKind::EQ || s.kind == LabelKind::RANGE ? 1
	       : s.kind == LabelKind::SET                            ? 2
	       : s.kind == LabelKind::SET_BOX                        ? label_set_box_query_base(s.m)
	                                                             : label_box_query_cell(s.m, 0);
}
// the cells of the table of a launch of n_queries queries (the context's buffer holds this many for the largest launch it may carry)
inline constexpr uint64_t label_batches_table_cells(const LabelBatchShape &s, uint64_t n_queries) {
	const uint64_t units = label_batches_query_units(s) * n_queries;
	return label_batches_query_base(s) + (s.kind == LabelKind::SET ? units / 2 : units);
}

// Unit i of the launch — unit i % units of launch-wide query i / units — for the kinds with 32-bit words whose table holds 64-bit
// cells: EQ, RANGE (a box over one column) and BOX.
inline constexpr uint64_t label_batches_cell(const LabelBatch<uint32_t> *batches, const LabelBatchShape &s, uint64_t i) {
	const uint64_t units = label_batches_query_units(s);
	const LabelBatchAt at = label_batch_at(s.per_batch, i / units);
	const LabelBatch<uint32_t> &b = batches[at.batch];
	if (s.kind == LabelKind::EQ)
		return label_want_cell(b.words[at.row]);
	const uint64_t j = i % units, end = at.row * (units / 2) + j / 2;
	const LabelRangeCells c = label_range_cells(b.lo[end], b.hi[end]);
	return j & 1 ? c.width : c.lo;
}
// ... for SET, whose units are the 32-bit words of the padded rows
inline constexpr uint32_t label_batches_set_word(const LabelBatch<uint32_t> *batches, const LabelBatchShape &s, uint64_t i) {
	const uint64_t units = label_batches_query_units(s);
	const LabelBatchAt at = label_batch_at(s.per_batch, i / units);
	return label_set_table_word(batches[at.batch].words + at.row * s.width, s.width, (uint32_t)(i % units));
}
// ... for the kinds with 64-bit words: BOX64 (no set words) and SET_BOX (the padded set words, then the range cells)
inline constexpr uint64_t label_batches_cell64(const LabelBatch<uint64_t> *batches, const LabelBatchShape &s, uint64_t i) {
	const uint64_t units = label_batches_query_units(s);
	const LabelBatchAt at = label_batch_at(s.per_batch, i / units);
	const LabelBatch<uint64_t> &b = batches[at.batch];
	const uint64_t j = i % units, padded = s.kind == LabelKind::SET_BOX ? label_set_box_padded(s.width) : 0;
	if (j < padded)
		return j < s.width ? b.words[at.row * s.width + j] : NO_LABEL64;
	const uint64_t end = at.row * s.m + (j - padded) / 2;
	const LabelRange64Cells c = label_range64_cells(b.lo[end], b.hi[end]);
	return (j - padded) & 1 ? c.count : c.lo;
}

// The head of the table, cells [0, label_batches_query_base): what the single-batch resolve kernels write ahead of query 0.
// addresses: the columns' device addresses in table order — column 0 alone for EQ / RANGE / SET, the named columns for BOX / BOX64,
// the set column and then the range columns for SET_BOX; wide_mask as the form's table head takes it.
constexpr uint32_t LABEL_TABLE_HEAD_MAX = 6;
struct LabelTableHead {
	uint64_t cell[LABEL_TABLE_HEAD_MAX];
	uint32_t n;
};
inline constexpr LabelTableHead label_batches_table_head(const LabelBatchShape &s, const uint64_t *addresses, uint32_t wide_mask) {
	LabelTableHead h = {{0, 0, 0, 0, 0, 0}, (uint32_t)label_batches_query_base(s)};
	if (s.kind == LabelKind::EQ || s.kind == LabelKind::RANGE || s.kind == LabelKind::SET) {
		h.cell[0] = addresses[0];
		if (s.kind == LabelKind::SET)
			h.cell[1] = s.width;
		return h;
	}
	const uint32_t n_addresses = s.kind == LabelKind::SET_BOX ? s.m + 1 : s.m;
	h.cell[0] = s.kind == LabelKind::BOX     ? s.m
	            : s.kind == LabelKind::BOX64 ? label_box64_table_head(s.m, wide_mask)
	                                         : label_set_box_table_head(s.m, label_set_box_padded(s.width), wide_mask);
	for (uint32_t j = 0; j != n_addresses; ++j)
		h.cell[1 + j] = addresses[j];
	return h; // (a SET_BOX's cell 2 + m, where there is one, stays 0: it keeps the per-query cells on an even index)
}
static_assert(1 + LABEL_COLUMNS_MAX <= LABEL_TABLE_HEAD_MAX && label_set_box_query_base(LABEL_SET_BOX_RANGES_MAX) <= LABEL_TABLE_HEAD_MAX,
              "the head of every kind fits LabelTableHead");

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
