// label_range_check.cpp — the range half of csrc/label_filter.h on a CPU: the admission rule of a label range, the two-cell form
// the walker tests with one subtraction and one comparison, the two-comparison form the listing kernels apply to a cell in a
// register, and the distinct pairs and group numbers of a call.  A stand-alone program (tests/test_label_range_logic.py builds it
// under the address and undefined-behaviour sanitizers and restates every line it prints in NumPy); it also checks the three
// forms against each other and exits non-zero on a difference.
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

// "lo ..." / "hi ..." / "pairs lo hi lo hi ..." / "group_of ..." quadruples
static void groups_case(const std::vector<uint32_t> &lo, const std::vector<uint32_t> &hi) {
	std::vector<LabelRange> pairs;
	std::vector<uint32_t> group_of, flat;
	label_range_groups(lo.data(), hi.data(), lo.size(), pairs, group_of);
	for (const LabelRange &p : pairs)
		flat.push_back(p.lo), flat.push_back(p.hi);
	print_list("lo", lo);
	print_list("hi", hi);
	print_list("pairs", flat);
	print_list("group_of", group_of);
	EXPECT(group_of.size() == lo.size());
	for (size_t i = 1; i < pairs.size(); ++i)
		EXPECT(pairs[i - 1] < pairs[i] && !(pairs[i - 1] == pairs[i]));
	for (size_t q = 0; q != lo.size(); ++q)
		EXPECT(group_of[q] < pairs.size() && pairs[group_of[q]].lo == lo[q] && pairs[group_of[q]].hi == hi[q]);
}

int main() {
	// the values whose neighbourhoods decide: both ends of the labels, the sign bit, NO_LABEL and the two below it
	const uint32_t edge[] = {0u, 1u, 2u, 7u, 8u, 9u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFDu, 0xFFFFFFFEu, 0xFFFFFFFFu};
	constexpr uint64_t labelled_rows = 11;
	constexpr int64_t free_key = 0x7FFFFFFFFFFFFFFFll;

	// ---- the walker's cells: "cells lo hi cell_lo cell_width"
	for (uint32_t lo : edge)
		for (uint32_t hi : edge) {
			const LabelRangeCells c = label_range_cells(lo, hi);
			std::printf("cells %u %u %llu %llu\n", lo, hi, (unsigned long long)c.lo, (unsigned long long)c.width);
		}

	// ---- the rule against both encodings: every (lo, hi, label) of the edge values, the label in a column of its own so that
	// every key reads it: "admit lo hi label key result", keys -1, 0, labelled_rows - 1, labelled_rows, the free key
	for (uint32_t label : edge) {
		std::vector<uint32_t> column(labelled_rows, label);
		for (uint32_t lo : edge)
			for (uint32_t hi : edge) {
				const LabelRangeCells c = label_range_cells(lo, hi);
				for (int64_t key : {(int64_t)-1, (int64_t)0, (int64_t)labelled_rows - 1, (int64_t)labelled_rows, free_key}) {
					const bool in = label_range_admits(column.data(), labelled_rows, key, lo, hi);
					std::printf("admit %u %u %u %lld %d\n", lo, hi, label, (long long)key, in ? 1 : 0);
					if (key >= 0 && (uint64_t)key < labelled_rows) {
						// the walker (GraphView::admitted_range) and the listing kernels get here only with a cell
						EXPECT(in == label_range_cell_admits(column[key], c.lo, c.width));
						EXPECT(in == label_in_range(column[key], lo, hi));
					} else
						EXPECT(!in);
				}
				// a slot without a cell is NO_LABEL in the listing kernels' registers: in no range
				EXPECT(!label_in_range(NO_LABEL, lo, hi));
				EXPECT(!label_range_cell_admits(NO_LABEL, c.lo, c.width));
			}
	}
	// a shorter column: the row id has no cell although the array goes on
	{
		const std::vector<uint32_t> column = {5, 5, 5, 5};
		EXPECT(label_range_admits(column.data(), 4, 3, 5, 5) && !label_range_admits(column.data(), 3, 3, 5, 5));
		EXPECT(!label_range_admits(column.data(), 0, 0, 0, NO_LABEL));
	}
	// equality is the degenerate range: label_admits says the same
	for (uint32_t label : edge)
		for (uint32_t want : edge)
			EXPECT(label_admits(&label, 1, 0, want) == label_range_admits(&label, 1, 0, want, want));

	// ---- distinct pairs and group numbers
	groups_case({3, 3, 3}, {9, 9, 9});                                        // one pair
	groups_case({5, 1, 5, 1, 0}, {6, 9, 2, 3, NO_LABEL});                     // all distinct; same lo, different hi
	groups_case({4, 9, 4, 7, 9, 4}, {8, 2, 8, 1, 2, 8});                      // duplicates, and two DIFFERENT empty pairs (9,2) (7,1)
	groups_case({0, NO_LABEL, 0, 2}, {NO_LABEL, NO_LABEL, 0, 2});             // everything, [NO_LABEL, NO_LABEL], two equalities
	groups_case({0x80000000u, 0x7FFFFFFFu, 0}, {0x80000001u, 0x80000000u, 0x7FFFFFFFu}); // ordered as unsigned
	groups_case({}, {});
	{
		uint64_t s = 0x9E3779B97F4A7C15ull;
		auto rnd = [&]() {
			s ^= s << 13, s ^= s >> 7, s ^= s << 17;
			return (uint32_t)(s >> 32);
		};
		std::vector<uint32_t> lo(300), hi(300);
		for (size_t q = 0; q != lo.size(); ++q)
			lo[q] = rnd() % 12, hi[q] = rnd() % 12;
		groups_case(lo, hi);
	}

	if (failures) {
		std::printf("label range check FAILED: %d\n", failures);
		return 1;
	}
	std::printf("label range check ok\n");
	return 0;
}
