// label_set_box_check.cpp — the last part of csrc/label_filter.h on a CPU: the admission rule of an IN-list on one label column
// inside a box of ranges (vss_search_batch_by_label_set_box), the register form the listing kernels apply, the walker's form over
// the cells k_resolve_label_set_boxes writes, the table's layout, the travelling rows and the groups of a call.  A stand-alone
// program (tests/test_label_set_box_logic.py builds it under the address and undefined-behaviour sanitizers and checks its count of
// cases); it proves both forms against the rule and exits non-zero on a difference.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/label_filter.h"

using namespace vss::host;

static int failures = 0;
static unsigned long long admit_cases = 0, group_cases = 0;
#define EXPECT(cond)                                                                                                   \
	do {                                                                                                               \
		if (!(cond)) {                                                                                                 \
			if (failures < 20)                                                                                         \
				std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                                          \
			++failures;                                                                                                \
		}                                                                                                              \
	} while (0)

// the index's four columns: different lengths, so that a row id may have a cell in one named column and none in a shorter one
constexpr uint64_t COLUMN_ROWS[LABEL_COLUMNS_MAX] = {11, 7, 9, 5};
constexpr int64_t FREE_KEY = 0x7FFFFFFFFFFFFFFFll;
constexpr uint64_t FILLER = 7; // a member that is none of the edge values

// what one range column contributes to a case: its width, the value every cell of it holds (a 32-bit column keeps the low word), and
// the query's ends for it
struct Clause {
	uint32_t width;
	uint64_t label, lo, hi;
};

struct Index {
	std::vector<uint32_t> narrow[LABEL_COLUMNS_MAX];
	std::vector<uint64_t> wide[LABEL_COLUMNS_MAX];
	LabelColumn64 columns[LABEL_COLUMNS_MAX] = {};
	void fill(uint32_t c, uint32_t width, uint64_t label) {
		if (width == 64) {
			wide[c].assign(COLUMN_ROWS[c], label);
			columns[c] = {nullptr, wide[c].data(), COLUMN_ROWS[c]};
		} else {
			narrow[c].assign(COLUMN_ROWS[c], (uint32_t)label);
			columns[c] = {narrow[c].data(), nullptr, COLUMN_ROWS[c]};
		}
	}
};

// One predicate against one index: the rule, and against it the listing kernels' register form over the travelling row and the
// walker's form over the table cells (label_set_box_table_cell is what k_resolve_label_set_boxes writes).
template <uint32_t M>
static void admit_case(uint32_t set_column, uint32_t set_col_width, uint64_t set_label, const std::vector<uint64_t> &set, const uint32_t *columns,
                       const Clause *clause) {
	Index index;
	index.fill(set_column, set_col_width, set_label);
	uint64_t box[2 * M + 1] = {}, lo[M + 1] = {}, hi[M + 1] = {}, shortest = COLUMN_ROWS[set_column];
	for (uint32_t j = 0; j != M; ++j) {
		index.fill(columns[j], clause[j].width, clause[j].label);
		box[2 * j] = lo[j] = clause[j].lo, box[2 * j + 1] = hi[j] = clause[j].hi;
		shortest = std::min(shortest, COLUMN_ROWS[columns[j]]);
	}
	const uint32_t width = (uint32_t)set.size(), padded = label_set_box_padded(width);
	std::vector<uint32_t> row;
	label_set_box_rows(set.data(), width, lo, hi, 1, M, row);
	EXPECT(row.size() == label_set_box_row_words(width, M));
	std::vector<uint64_t> cells(label_set_box_query_cells(M, padded));
	for (uint32_t j = 0; j != cells.size(); ++j)
		cells[j] = label_set_box_table_cell(row.data(), width, M, j);
	for (uint32_t j = 0; j != padded; ++j)
		EXPECT(cells[j] == (j < width ? set[j] : NO_LABEL64));
	for (int64_t key : {(int64_t)-1, (int64_t)0, (int64_t)shortest - 1, (int64_t)shortest, FREE_KEY}) {
		const bool in = label_set_box_admits(index.columns, set_column, set.data(), width, columns, M, key, box);
		// the listing kernels: a live key reads every column that has a cell for it, widened; NO_LABEL64 stands for "no cell"
		uint64_t label[M + 1];
		const bool live = key != FREE_KEY && key >= 0;
		label[0] = live && (uint64_t)key < COLUMN_ROWS[set_column] ? label_cell64(index.columns[set_column], (uint64_t)key) : NO_LABEL64;
		for (uint32_t j = 0; j != M; ++j)
			label[1 + j] = live && (uint64_t)key < COLUMN_ROWS[columns[j]] ? label_cell64(index.columns[columns[j]], (uint64_t)key) : NO_LABEL64;
		EXPECT(in == label_in_set_box<M>(label, row.data(), width));
		// the walker (GraphView::admitted_set_box) gets to its cells only below the SHORTEST of the set column and the range columns
		if (live && (uint64_t)key < shortest)
			EXPECT(in == label_set_box_cells_admit(label, cells.data(), M, padded));
		else
			EXPECT(!in);
		++admit_cases;
	}
}

// a row of `width` words that holds `word` at position `at`, and elsewhere the filler or padding, by `pattern`
static std::vector<uint64_t> set_around(uint32_t width, uint32_t at, uint64_t word, uint32_t pattern) {
	std::vector<uint64_t> set(width);
	for (uint32_t j = 0; j != width; ++j)
		set[j] = j == at ? word : pattern == 0 ? NO_LABEL64 : pattern == 1 ? FILLER : (j & 1 ? NO_LABEL64 : FILLER);
	return set;
}

// the groups of n predicates against an independent sort of their rows as vectors of 64-bit words
static void groups_case(uint32_t width, uint32_t m, const std::vector<uint64_t> &sets, const std::vector<uint64_t> &lo, const std::vector<uint64_t> &hi) {
	const uint64_t n = sets.size() / width;
	const uint32_t per = label_set_box_row_words(width, m), per64 = width + 2 * m;
	std::vector<uint32_t> travelling, rows, group_of;
	label_set_box_rows(sets.data(), width, lo.data(), hi.data(), n, m, travelling);
	label_set_box_groups(travelling.data(), n, width, m, rows, group_of);
	EXPECT(travelling.size() == per * n && group_of.size() == n && rows.size() % per == 0);
	std::vector<std::vector<uint64_t>> want(n);
	for (uint64_t q = 0; q != n; ++q) {
		want[q].assign(sets.begin() + q * width, sets.begin() + (q + 1) * width);
		for (uint32_t j = 0; j != m; ++j)
			want[q].push_back(lo[q * m + j]), want[q].push_back(hi[q * m + j]);
		for (uint32_t j = 0; j != per64; ++j) // every 64-bit word travels as (high word, low word)
			EXPECT(label_word64(&travelling[q * per + 2 * j]) == want[q][j] && travelling[q * per + 2 * j] == (uint32_t)(want[q][j] >> 32));
	}
	std::vector<std::vector<uint64_t>> distinct = want;
	std::sort(distinct.begin(), distinct.end());
	distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
	EXPECT(rows.size() / per == distinct.size());
	for (size_t g = 0; g != distinct.size() && rows.size() / per == distinct.size(); ++g)
		for (uint32_t j = 0; j != per64; ++j)
			EXPECT(label_word64(&rows[g * per + 2 * j]) == distinct[g][j]);
	for (uint64_t q = 0; q != n; ++q)
		EXPECT(group_of[q] < distinct.size() && distinct[group_of[q]] == want[q]);
	++group_cases;
}

int main() {
	constexpr uint64_t T31 = 1ull << 31, T32 = 1ull << 32, T63 = 1ull << 63;
	const uint64_t edge[] = {0, 1, T31, T32 - 2, T32 - 1, T32, T63, NO_LABEL64 - 1, NO_LABEL64};
	const uint32_t widths[] = {1, 2, 3, 4, 5, 31, 32};

	// ---- n_columns 0: every (cell, word) of the edge values, both widths of the set column, every width, the word at every position
	// of a short row and at the first, a middle and the last position of a long one, among padding, fillers and both
	for (uint32_t col_width : {32u, 64u})
		for (uint32_t width : widths)
			for (uint64_t cell : edge)
				for (uint64_t word : edge)
					for (uint32_t at : {0u, width / 2, width - 1})
						for (uint32_t pattern : {0u, 1u, 2u})
							admit_case<0>(col_width == 64 ? 2 : 0, col_width, cell, set_around(width, at, word, pattern), nullptr, nullptr);
	// the filler IS the cell: admitted through another word than the edge one, wherever the padding lies
	for (uint32_t col_width : {32u, 64u})
		for (uint32_t width : widths)
			for (uint32_t pattern : {0u, 1u, 2u})
				admit_case<0>(1, col_width, FILLER, set_around(width, width - 1, T32 + FILLER, pattern), nullptr, nullptr);

	// ---- n_columns 1: every (cell, word, lo, hi) of the edge values — the range column, of the OTHER width, holds the same cell — and
	// n_columns 3 with widths mixed, the two further columns each once holding, once NULL under "everything", once empty
	const Clause reduced64[] = {{64, T32 + 5, T32, NO_LABEL64}, {64, NO_LABEL64, 0, NO_LABEL64}, {64, 5, 6, 4}};
	const Clause reduced32[] = {{32, 5, 0, NO_LABEL64}, {32, NO_LABEL, 0, NO_LABEL64}, {32, 5, 6, 4}};
	uint32_t turn = 0;
	for (uint32_t col_width : {32u, 64u})
		for (uint32_t width : widths)
			for (uint64_t cell : edge)
				for (uint64_t word : edge)
					for (uint64_t lo : edge)
						for (uint64_t hi : edge) {
							++turn;
							const std::vector<uint64_t> set = set_around(width, turn % width, word, turn % 3);
							const uint32_t one[] = {3};
							const Clause first = {col_width == 64 ? 32u : 64u, cell, lo, hi};
							admit_case<1>(1, col_width, cell, set, one, &first);
							const uint32_t three[] = {0, 3, 2};
							const Clause all[] = {first, reduced64[turn % 3], reduced32[turn / 3 % 3]};
							admit_case<3>(1, col_width, cell, set, three, all);
						}
	// the set column the short one, the range column the longer: a cell there and none in the set column
	for (uint64_t label : edge) {
		const uint32_t one[] = {0};
		const Clause c = {64, label, label, label};
		admit_case<1>(3, 32, 5, {5}, one, &c);
	}
	// two words that differ in the HIGH 32 bits only, and in the low 32 bits only, on a wide set column; on a narrow one a word
	// of 2^32 or above and the word 0xFFFFFFFF admit nothing
	admit_case<0>(2, 64, T32 + 9, {T32 + 9, 2 * T32 + 9}, nullptr, nullptr);
	admit_case<0>(2, 64, 2 * T32 + 9, {T32 + 9}, nullptr, nullptr);
	admit_case<0>(2, 64, T32 + 9, {T32 + 8}, nullptr, nullptr);
	admit_case<0>(0, 32, 9, {T32 + 9}, nullptr, nullptr);
	admit_case<0>(0, 32, NO_LABEL, {0xFFFFFFFFull}, nullptr, nullptr);

	// ---- the walker's table: the head's fields, the even base of the per-query cells, whole chunks
	for (uint32_t m = 0; m <= LABEL_SET_BOX_RANGES_MAX; ++m)
		for (uint32_t width : widths) {
			const uint32_t padded = label_set_box_padded(width), wide_mask = (m * 5 + width) & ((2u << m) - 1);
			const uint64_t head = label_set_box_table_head(m, padded, wide_mask);
			EXPECT(label_set_box_head_ranges(head) == m && label_set_box_head_padded(head) == padded);
			for (uint32_t j = 0; j != LABEL_COLUMNS_MAX; ++j)
				EXPECT(label_set_box_head_wide(head, j) == (((wide_mask >> j) & 1) != 0));
			EXPECT(padded % 2 == 0 && padded >= width && padded <= width + 1);
			EXPECT(label_set_box_query_base(m) >= 2 + m && label_set_box_query_base(m) % 2 == 0);
			for (uint64_t q : {0ull, 1ull, 203ull})
				EXPECT(label_set_box_query_cell(m, padded, q) % 2 == 0 &&
				       label_set_box_query_cell(m, padded, q + 1) - label_set_box_query_cell(m, padded, q) == padded + 2 * m);
			EXPECT(label_set_box_table_cells(m, padded, 204) == label_set_box_query_cell(m, padded, 204));
			EXPECT(label_set_box_row_words(width, m) <= LABEL_SET_BOX_ROW_WORDS_MAX);
		}

	// ---- the column check
	{
		const uint32_t ok[] = {1, 3, 0}, twice[] = {1, 3, 1}, is_set[] = {1, 2, 0}, far[] = {1, 4};
		EXPECT(label_set_box_bad_column(2, ok, 3) == 4 && label_set_box_bad_column(2, ok, 0) == 1 && label_set_box_bad_column(4, ok, 3) == 0);
		EXPECT(label_set_box_bad_column(2, twice, 3) == 3 && label_set_box_bad_column(2, is_set, 3) == 2 && label_set_box_bad_column(2, far, 2) == 2);
		EXPECT(label_set_box_bad_column(2, twice, 2) == 3);
	}

	// ---- the groups: the order of the travelling rows as 32-bit words is the order of their 64-bit words
	groups_case(1, 0, {3, 3, 3}, {}, {});
	groups_case(2, 0, {T32 + 1, 5, 1, 0xFFFFFFFFull, T32, 0, 1, 0xFFFFFFFFull}, {}, {}); // rows that differ in a HIGH word only
	groups_case(3, 0, {5, NO_LABEL64, NO_LABEL64, NO_LABEL64, 5, NO_LABEL64, NO_LABEL64, NO_LABEL64, 5, 5, NO_LABEL64, NO_LABEL64}, {}, {}); // ... in padding position only
	groups_case(2, 1, {4, 9, 9, 4, 4, 9}, {T63, T63, T63}, {NO_LABEL64, NO_LABEL64, T63 - 1}); // a permuted duplicate; the same set, another range
	groups_case(2, 1, {4, 9, 4, 9}, {2 * T32, T32 + 7}, {NO_LABEL64, NO_LABEL64}); // a range end that differs in the high word
	groups_case(1, 3, {T63, T63}, {1, 2, 3, 1, 2, 3}, {1, 2, T32 + 3, 1, 2, 3});
	groups_case(32, 0, {}, {}, {});
	{
		uint64_t s = 0x9E3779B97F4A7C15ull;
		auto rnd = [&]() {
			s ^= s << 13, s ^= s >> 7, s ^= s << 17;
			return (uint32_t)(s >> 32);
		};
		for (uint32_t width : widths)
			for (uint32_t m : {0u, 1u, 3u}) {
				std::vector<uint64_t> sets(300 * width), lo(300 * m), hi(300 * m);
				for (uint64_t &w : sets)
					w = rnd() % 4 == 0 ? NO_LABEL64 : (uint64_t)(rnd() % 2) << 32 | rnd() % 2;
				for (size_t i = 0; i != lo.size(); ++i)
					lo[i] = (uint64_t)(rnd() % 2) << 32 | rnd() % 2, hi[i] = (uint64_t)(rnd() % 2) << 32 | rnd() % 2;
				groups_case(width, m, sets, lo, hi);
			}
	}

	std::printf("admit cases %llu\ngroup cases %llu\n", admit_cases, group_cases);
	if (failures) {
		std::printf("label set box check FAILED: %d\n", failures);
		return 1;
	}
	std::printf("label set box check ok\n");
	return 0;
}
