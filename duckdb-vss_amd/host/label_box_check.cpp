// label_box_check.cpp — the box part of csrc/label_filter.h on a CPU: the admission rule of a conjunction of ranges over several
// label columns, the walker's AND of two-cell forms, the register form the listing kernels apply, the layout of the walker's table
// and the distinct rows and group numbers of a call.  A stand-alone program (tests/test_label_box_logic.py builds it under the
// address and undefined-behaviour sanitizers and restates every line it prints in NumPy); it also checks the three forms against
// each other and exits non-zero on a difference.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/label_filter.h"

using namespace vss::host;

static int failures = 0;
#define EXPECT(cond)                                                                                                   \
	do {                                                                                                               \
		if (!(cond)) {                                                                                                 \
			std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                                              \
			++failures;                                                                                                \
		}                                                                                                              \
	} while (0)

static void print_list(const char *tag, const std::vector<uint32_t> &v) {
	std::printf("%s", tag);
	for (uint32_t x : v)
		std::printf(" %u", x);
	std::printf("\n");
}

// the index's four columns: different lengths, so that a row id may have a cell in one named column and none in a shorter one
constexpr uint64_t COLUMN_ROWS[LABEL_COLUMNS_MAX] = {11, 7, 9, 5};
constexpr int64_t FREE_KEY = 0x7FFFFFFFFFFFFFFFll;

// what one named column contributes to a case: the label every cell of it holds, and the query's ends for it
struct Clause {
	uint32_t label, lo, hi;
};

// "admit m key result (column rows label lo hi) x m": the rule, and against it the walker's and the listing kernels' forms
template <uint32_t M>
static void admit_case(const uint32_t (&columns)[M], const Clause (&clause)[M]) {
	std::vector<uint32_t> storage[LABEL_COLUMNS_MAX];
	const uint32_t *cells[LABEL_COLUMNS_MAX] = {};
	uint32_t box[2 * M];
	uint64_t table[2 * M], shortest = ~0ull, longest = 0;
	for (uint32_t j = 0; j != M; ++j) {
		const uint32_t c = columns[j];
		storage[c].assign(COLUMN_ROWS[c], clause[j].label);
		cells[c] = storage[c].data();
		box[2 * j] = clause[j].lo, box[2 * j + 1] = clause[j].hi;
		const LabelRangeCells rc = label_range_cells(clause[j].lo, clause[j].hi);
		table[2 * j] = rc.lo, table[2 * j + 1] = rc.width;
		shortest = std::min(shortest, COLUMN_ROWS[c]), longest = std::max(longest, COLUMN_ROWS[c]);
	}
	for (int64_t key : {(int64_t)-1, (int64_t)0, (int64_t)shortest - 1, (int64_t)shortest, (int64_t)longest - 1, FREE_KEY}) {
		const bool in = label_box_admits(cells, COLUMN_ROWS, columns, M, key, box);
		std::printf("admit %u %lld %d", M, (long long)key, in ? 1 : 0);
		for (uint32_t j = 0; j != M; ++j)
			std::printf(" %u %llu %u %u %u", columns[j], (unsigned long long)COLUMN_ROWS[columns[j]], clause[j].label, clause[j].lo, clause[j].hi);
		std::printf("\n");
		// the listing kernels: a live key reads every named column that has a cell for it, NO_LABEL stands for "no cell at all"
		uint32_t label[M];
		const bool live = key != FREE_KEY && key >= 0;
		for (uint32_t j = 0; j != M; ++j)
			label[j] = live && (uint64_t)key < COLUMN_ROWS[columns[j]] ? cells[columns[j]][key] : NO_LABEL;
		EXPECT(in == label_in_box<M>(label, box));
		// the walker (GraphView::admitted_box) gets to its cells only below the SHORTEST named column
		if (live && (uint64_t)key < shortest)
			EXPECT(in == label_box_cells_admit(label, table, M));
		else
			EXPECT(!in);
	}
}

// "boxes m" / "lo ..." / "hi ..." / "rows ..." / "group_of ..." quintuples: lo and hi are n x m matrices, rows the groups' 2m words
static void groups_case(uint32_t m, const std::vector<uint32_t> &lo, const std::vector<uint32_t> &hi) {
	const uint64_t n = lo.size() / m;
	std::vector<uint32_t> boxes, rows, group_of;
	label_box_rows(lo.data(), hi.data(), n, m, boxes);
	label_box_groups(boxes.data(), n, m, rows, group_of);
	std::printf("boxes %u\n", m);
	print_list("lo", lo);
	print_list("hi", hi);
	print_list("rows", rows);
	print_list("group_of", group_of);
	EXPECT(group_of.size() == n && boxes.size() == 2 * m * n && rows.size() % (2 * m) == 0);
	const uint64_t groups = rows.size() / (2 * m);
	for (uint64_t g = 1; g < groups; ++g)
		EXPECT(std::lexicographical_compare(rows.begin() + (g - 1) * 2 * m, rows.begin() + g * 2 * m, rows.begin() + g * 2 * m,
		                                    rows.begin() + (g + 1) * 2 * m));
	for (uint64_t q = 0; q != n; ++q) {
		EXPECT(group_of[q] < groups);
		for (uint32_t j = 0; j != m && group_of[q] < groups; ++j)
			EXPECT(rows[group_of[q] * 2 * m + 2 * j] == lo[q * m + j] && rows[group_of[q] * 2 * m + 2 * j + 1] == hi[q * m + j]);
	}
	if (m == 1) { // one column: the groups of the range call, in its order
		std::vector<LabelRange> pairs;
		std::vector<uint32_t> range_group_of;
		label_range_groups(lo.data(), hi.data(), n, pairs, range_group_of);
		EXPECT(range_group_of == group_of && pairs.size() == groups);
		for (uint64_t g = 0; g != groups && g != pairs.size(); ++g)
			EXPECT(pairs[g].lo == rows[2 * g] && pairs[g].hi == rows[2 * g + 1]);
	}
}

int main() {
	// the values whose neighbourhoods decide: both ends of the labels, the sign bit, NO_LABEL and the two below it
	const uint32_t edge[] = {0u, 1u, 2u, 7u, 8u, 9u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFDu, 0xFFFFFFFEu, 0xFFFFFFFFu};
	// the other named columns: a clause that holds, a NO_LABEL cell under "everything", an empty range over a label it would hold
	const Clause reduced[] = {{5, 0, NO_LABEL}, {NO_LABEL, 0, NO_LABEL}, {5, 6, 4}};

	// ---- the rule against both encodings, m = 1, 2 and 4: every (label, lo, hi) of the edge values in the first named column
	for (uint32_t label : edge)
		for (uint32_t lo : edge)
			for (uint32_t hi : edge) {
				const Clause first = {label, lo, hi};
				admit_case<1>({0}, {first});
				for (const Clause &b : reduced) {
					admit_case<2>({2, 1}, {first, b});
					for (const Clause &c : reduced)
						for (const Clause &d : reduced)
							admit_case<4>({3, 0, 2, 1}, {first, b, c, d});
				}
			}
	// the first named column the short one, the full set in the LONGER: a cell there and none in the shorter one
	for (uint32_t label : edge)
		admit_case<2>({3, 0}, {{5, 5, 5}, {label, label, label}});

	// ---- the walker's table: "table m n_queries cells" then "cell q j index lo hi cell_lo cell_width"
	for (uint32_t m : {1u, 2u, 4u}) {
		const uint64_t nq = 3;
		std::printf("table %u %llu %llu\n", m, (unsigned long long)nq, (unsigned long long)label_box_table_cells(m, nq));
		for (uint64_t q = 0; q != nq; ++q)
			for (uint32_t j = 0; j != m; ++j) {
				const uint32_t lo = edge[(3 * q + j) % 11], hi = edge[(5 * q + 2 * j + 4) % 11];
				const LabelRangeCells c = label_range_cells(lo, hi);
				std::printf("cell %llu %u %llu %u %u %llu %llu\n", (unsigned long long)q, j,
				            (unsigned long long)(label_box_query_cell(m, q) + 2 * j), lo, hi, (unsigned long long)c.lo, (unsigned long long)c.width);
			}
		EXPECT(label_box_query_cell(m, nq) == label_box_table_cells(m, nq));
	}

	// ---- the named columns of a call
	{
		const uint32_t good[] = {3, 0, 2, 1}, twice[] = {1, 2, 1}, far[] = {0, 4}, first_far[] = {7};
		EXPECT(label_box_bad_column(good, 4) == 4 && label_box_bad_column(good, 1) == 1);
		EXPECT(label_box_bad_column(twice, 3) == 2 && label_box_bad_column(twice, 2) == 2);
		EXPECT(label_box_bad_column(far, 2) == 1 && label_box_bad_column(first_far, 1) == 0);
	}

	// ---- distinct rows and group numbers
	groups_case(1, {3, 3, 3}, {9, 9, 9});                                   // one box
	groups_case(1, {4, 9, 4, 7, 9, 4}, {8, 2, 8, 1, 2, 8});                 // duplicates; two DIFFERENT empty rows
	groups_case(2, {1, 5, 1, 5, 1, 5}, {1, 9, 1, 9, 1, 9});                 // duplicates of a two-column box
	groups_case(2, {1, 5, 1, 5, 1, 6, 1, 5}, {1, 9, 1, 8, 1, 9, 1, 9});     // rows that differ in the LAST column only (hi, then lo)
	groups_case(2, {9, 0, 0, 7, 9, 0}, {2, NO_LABEL, NO_LABEL, 1, 2, NO_LABEL}); // empty through column 0, through column 1, repeated
	groups_case(2, {0x80000000u, 0, 0x7FFFFFFFu, 0, 0, 0x80000000u}, {0x80000001u, 1, 0x80000000u, 1, 1, 0x80000000u}); // unsigned order
	groups_case(4, {1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3, 5}, {1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3, 5}); // four columns, last differs
	groups_case(1, {}, {});
	groups_case(4, {}, {});
	{
		uint64_t s = 0x9E3779B97F4A7C15ull;
		auto rnd = [&]() {
			s ^= s << 13, s ^= s >> 7, s ^= s << 17;
			return (uint32_t)(s >> 32);
		};
		std::vector<uint32_t> lo(300 * 3), hi(300 * 3);
		for (size_t i = 0; i != lo.size(); ++i)
			lo[i] = rnd() % 3, hi[i] = rnd() % 3;
		groups_case(3, lo, hi);
	}

	if (failures) {
		std::printf("label box check FAILED: %d\n", failures);
		return 1;
	}
	std::printf("label box check ok\n");
	return 0;
}
