// label_box64_check.cpp — the 64-bit part of csrc/label_filter.h on a CPU: the admission rule of a conjunction of ranges with
// 64-bit ends over label columns of either width, the walker's (cell - lo) < count form, the register form the listing kernels
// apply, the layout of the walker's table, the word pairs a box travels as, and the distinct rows and group numbers of a call.  A
// stand-alone program (tests/test_label_box64_logic.py builds it under the address and undefined-behaviour sanitizers and restates
// every line it prints in NumPy); it also checks the three forms against each other and exits non-zero on a difference.
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

template <class T>
static void print_list(const char *tag, const std::vector<T> &v) {
	std::printf("%s", tag);
	for (T x : v)
		std::printf(" %llu", (unsigned long long)x);
	std::printf("\n");
}

// the index's four columns: different lengths, so that a row id may have a cell in one named column and none in a shorter one
constexpr uint64_t COLUMN_ROWS[LABEL_COLUMNS_MAX] = {11, 7, 9, 5};
constexpr int64_t FREE_KEY = 0x7FFFFFFFFFFFFFFFll;

// what one named column contributes to a case: its width, the value every cell of it holds (a 32-bit column keeps the low word),
// and the query's ends for it
struct Clause {
	uint32_t width;
	uint64_t label, lo, hi;
};

// "admit m key result (column rows width cell lo hi) x m": the rule, and against it the walker's and the listing kernels' forms;
// `cell` is the cell as the column stores it
template <uint32_t M>
static void admit_case(const uint32_t (&columns)[M], const Clause (&clause)[M]) {
	std::vector<uint32_t> narrow[LABEL_COLUMNS_MAX];
	std::vector<uint64_t> wide[LABEL_COLUMNS_MAX];
	LabelColumn64 index_columns[LABEL_COLUMNS_MAX] = {};
	uint64_t box[2 * M], table[2 * M], stored[M], shortest = ~0ull;
	for (uint32_t j = 0; j != M; ++j) {
		const uint32_t c = columns[j];
		if (clause[j].width == 64) {
			wide[c].assign(COLUMN_ROWS[c], clause[j].label);
			index_columns[c] = {nullptr, wide[c].data(), COLUMN_ROWS[c]};
			stored[j] = clause[j].label;
		} else {
			narrow[c].assign(COLUMN_ROWS[c], (uint32_t)clause[j].label);
			index_columns[c] = {narrow[c].data(), nullptr, COLUMN_ROWS[c]};
			stored[j] = (uint32_t)clause[j].label;
		}
		box[2 * j] = clause[j].lo, box[2 * j + 1] = clause[j].hi;
		const LabelRange64Cells rc = label_range64_cells(clause[j].lo, clause[j].hi);
		table[2 * j] = rc.lo, table[2 * j + 1] = rc.count;
		shortest = std::min(shortest, COLUMN_ROWS[c]);
	}
	// the box as it travels: 4M words, every end high word first
	std::vector<uint64_t> lo(M), hi(M);
	for (uint32_t j = 0; j != M; ++j)
		lo[j] = box[2 * j], hi[j] = box[2 * j + 1];
	std::vector<uint32_t> words;
	label_box64_rows(lo.data(), hi.data(), 1, M, words);
	for (int64_t key : {(int64_t)-1, (int64_t)0, (int64_t)shortest - 1, (int64_t)shortest, FREE_KEY}) {
		const bool in = label_box64_admits(index_columns, columns, M, key, box);
		std::printf("admit %u %lld %d", M, (long long)key, in ? 1 : 0);
		for (uint32_t j = 0; j != M; ++j)
			std::printf(" %u %llu %u %llu %llu %llu", columns[j], (unsigned long long)COLUMN_ROWS[columns[j]], clause[j].width,
			            (unsigned long long)stored[j], (unsigned long long)clause[j].lo, (unsigned long long)clause[j].hi);
		std::printf("\n");
		// the listing kernels: a live key reads every named column that has a cell for it, widened; NO_LABEL64 stands for "no cell"
		uint64_t label[M];
		const bool live = key != FREE_KEY && key >= 0;
		for (uint32_t j = 0; j != M; ++j)
			label[j] = live && (uint64_t)key < COLUMN_ROWS[columns[j]] ? label_cell64(index_columns[columns[j]], (uint64_t)key) : NO_LABEL64;
		EXPECT(in == label_in_box64<M>(label, words.data()));
		// the walker (GraphView::admitted_box64) gets to its cells only below the SHORTEST named column
		if (live && (uint64_t)key < shortest)
			EXPECT(in == label_box64_cells_admit(label, table, M));
		else
			EXPECT(!in);
	}
}

// "boxes m" / "lo ..." / "hi ..." / "rows ..." / "group_of ..." quintuples: lo and hi are n x m matrices of 64-bit ends, rows the
// groups' 2m 64-bit words, put together again from the word pairs
static void groups_case(uint32_t m, const std::vector<uint64_t> &lo, const std::vector<uint64_t> &hi) {
	const uint64_t n = lo.size() / m;
	std::vector<uint32_t> boxes, rows, group_of;
	label_box64_rows(lo.data(), hi.data(), n, m, boxes);
	label_box64_groups(boxes.data(), n, m, rows, group_of);
	EXPECT(group_of.size() == n && boxes.size() == 4 * m * n && rows.size() % (4 * m) == 0);
	// the layout of a travelling row: per named column lo then hi, each as (high word, low word)
	for (uint64_t i = 0; i != n * m; ++i) {
		EXPECT(boxes[4 * i] == (uint32_t)(lo[i] >> 32) && boxes[4 * i + 1] == (uint32_t)lo[i]);
		EXPECT(boxes[4 * i + 2] == (uint32_t)(hi[i] >> 32) && boxes[4 * i + 3] == (uint32_t)hi[i]);
		EXPECT(label_word64(&boxes[4 * i]) == lo[i] && label_word64(boxes[4 * i + 2], boxes[4 * i + 3]) == hi[i]);
	}
	std::vector<uint64_t> rows64(rows.size() / 2);
	for (size_t i = 0; i != rows64.size(); ++i)
		rows64[i] = label_word64(&rows[2 * i]);
	std::printf("boxes %u\n", m);
	print_list("lo", lo);
	print_list("hi", hi);
	print_list("rows", rows64);
	print_list("group_of", group_of);
	const uint64_t groups = rows64.size() / (2 * m);
	for (uint64_t g = 1; g < groups; ++g) // ascending as 2m unsigned 64-bit words
		EXPECT(std::lexicographical_compare(rows64.begin() + (g - 1) * 2 * m, rows64.begin() + g * 2 * m, rows64.begin() + g * 2 * m,
		                                    rows64.begin() + (g + 1) * 2 * m));
	for (uint64_t q = 0; q != n; ++q) {
		EXPECT(group_of[q] < groups);
		for (uint32_t j = 0; j != m && group_of[q] < groups; ++j)
			EXPECT(rows64[group_of[q] * 2 * m + 2 * j] == lo[q * m + j] && rows64[group_of[q] * 2 * m + 2 * j + 1] == hi[q * m + j]);
	}
}

int main() {
	constexpr uint64_t T31 = 1ull << 31, T32 = 1ull << 32, T63 = 1ull << 63;
	// the values whose neighbourhoods decide: both ends of the 32-bit cells, NO_LABEL and its neighbours, the first value that
	// needs the high word, the sign bit, NO_LABEL64 and the value below it
	const uint64_t edge[] = {0, 1, T31, T32 - 2, T32 - 1, T32, T63 - 1, T63, NO_LABEL64 - 1, NO_LABEL64};
	// the other named columns, per width: a clause that holds, a NULL cell under "everything", an empty range over a cell it would hold
	const Clause reduced64[] = {{64, T32 + 5, T32, NO_LABEL64}, {64, NO_LABEL64, 0, NO_LABEL64}, {64, 5, 6, 4}};
	const Clause reduced32[] = {{32, 5, 0, NO_LABEL64}, {32, NO_LABEL, 0, NO_LABEL64}, {32, 5, 6, 4}};

	// ---- the rule against both encodings: every (cell, lo, hi) of the edge values in the first named column, of BOTH widths (a
	// 32-bit column stores the low word of the value), at m = 1, at m = 2 beside a column of the OTHER width, and at m = 4 with
	// widths 64, 32, 64, 32
	for (uint32_t width : {32u, 64u})
		for (uint64_t label : edge)
			for (uint64_t lo : edge)
				for (uint64_t hi : edge) {
					const Clause first = {width, label, lo, hi};
					admit_case<1>({0}, {first});
					for (const Clause &b : width == 64 ? reduced32 : reduced64) {
						admit_case<2>({2, 1}, {first, b});
						if (width == 64)
							for (const Clause &c : reduced64)
								for (const Clause &d : reduced32)
									admit_case<4>({3, 0, 2, 1}, {first, b, c, d});
					}
				}
	// the first named column the short one, the full set in the LONGER: a cell there and none in the shorter one
	for (uint64_t label : edge)
		admit_case<2>({3, 0}, {{32, 5, 5, 5}, {64, label, label, label}});
	// a pair that differs in the high word only
	admit_case<2>({1, 3}, {{32, 7, 7, 7}, {64, T32 + 7, T32 + 5, T32 + 9}});
	admit_case<2>({1, 3}, {{32, 7, 7, 7}, {64, 7, T32 + 5, T32 + 9}});
	admit_case<2>({1, 3}, {{32, 7, T32 + 5, T32 + 9}, {64, T32 + 7, T32 + 5, T32 + 9}});

	// ---- the walker's table: "table m n_queries cells wide_mask head" then "cell q j index lo hi cell_lo cell_count"
	for (uint32_t m : {1u, 2u, 4u}) {
		const uint64_t nq = 3;
		const uint32_t wide_mask = m == 1 ? 1u : m == 2 ? 2u : 5u;
		const uint64_t head = label_box64_table_head(m, wide_mask);
		std::printf("table %u %llu %llu %u %llu\n", m, (unsigned long long)nq, (unsigned long long)label_box_table_cells(m, nq), wide_mask,
		            (unsigned long long)head);
		EXPECT(label_box64_head_columns(head) == m);
		for (uint32_t j = 0; j != LABEL_COLUMNS_MAX; ++j)
			EXPECT(label_box64_head_wide(head, j) == (((wide_mask >> j) & 1) != 0));
		for (uint64_t q = 0; q != nq; ++q)
			for (uint32_t j = 0; j != m; ++j) {
				const uint64_t lo = edge[(3 * q + j) % 10], hi = edge[(7 * q + 3 * j + 5) % 10];
				const LabelRange64Cells c = label_range64_cells(lo, hi);
				std::printf("cell %llu %u %llu %llu %llu %llu %llu\n", (unsigned long long)q, j,
				            (unsigned long long)(label_box_query_cell(m, q) + 2 * j), (unsigned long long)lo, (unsigned long long)hi,
				            (unsigned long long)c.lo, (unsigned long long)c.count);
			}
		EXPECT(label_box_query_cell(m, nq) == label_box_table_cells(m, nq));
	}

	// ---- distinct rows and group numbers
	groups_case(1, {3, 3, 3}, {9, 9, 9});                                   // one box
	groups_case(1, {4, 9, 4, 7, 9, 4}, {8, 2, 8, 1, 2, 8});                 // duplicates; two DIFFERENT empty rows
	groups_case(2, {1, T63 + 5, 1, T63 + 5, 1, T63 + 5}, {1, T63 + 9, 1, T63 + 9, 1, T63 + 9}); // duplicates of a two-column box
	groups_case(2, {1, 5, 1, 5, 1, 6, 1, 5}, {1, 9, 1, 8, 1, 9, 1, 9});     // rows that differ in the LAST column only (hi, then lo)
	groups_case(2, {9, 0, 0, 7, 9, 0}, {2, NO_LABEL64, NO_LABEL64, 1, 2, NO_LABEL64}); // empty through column 0, through column 1, repeated
	// order: a LOW word that is larger under a HIGH word that is smaller must sort first (word pairs high word first), and the
	// sign bit sorts unsigned
	groups_case(1, {T32 + 1, 0xFFFFFFFFull, T63, T63 - 1, 2 * T32, 7}, {T32 + 1, 0xFFFFFFFFull, T63, T63 - 1, 2 * T32, 7});
	groups_case(2, {5, T32, 5, T32 - 1, 5, T32 + 1}, {5, T32 + 9, 5, T32 + 9, 5, 3}); // ... in the last column
	groups_case(4, {1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3, 5}, {1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3, T32 + 5}); // four columns, last differs
	groups_case(1, {}, {});
	groups_case(4, {}, {});
	{
		uint64_t s = 0x9E3779B97F4A7C15ull;
		auto rnd = [&]() {
			s ^= s << 13, s ^= s >> 7, s ^= s << 17;
			return (uint32_t)(s >> 32);
		};
		std::vector<uint64_t> lo(300 * 3), hi(300 * 3);
		for (size_t i = 0; i != lo.size(); ++i)
			lo[i] = (uint64_t)(rnd() % 3) << 32 | rnd() % 2, hi[i] = (uint64_t)(rnd() % 3) << 32 | rnd() % 2;
		groups_case(3, lo, hi);
	}

	if (failures) {
		std::printf("label box64 check FAILED: %d\n", failures);
		return 1;
	}
	std::printf("label box64 check ok\n");
	return 0;
}
